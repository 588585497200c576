"""The contract of attention rescoring (tests/dec_rescore_ref.py) against the oracle decoder
(oracle/ref_port.py) in float64, its fusing / ranking / status rules bit for bit, and the measurement of kappa_ref - the
kappa a plain fp32 evaluation of sequence attention needs against float64 - that tests/test_gpu_dec_rescore.py holds the
kernel to.  No GPU."""
import math

import numpy as np
import pytest
import torch

import dec_rescore_ref as DR
from helpers import CFGS, oracle_model

LENGTHS = (0, 1, 2, 17)
FRAMES = (1, 7, 33)
# kappa_ref per family, measured by test_kappa_ref_of_an_fp32_evaluation below over DR.attention_cases (the shapes of the GPU
# test): flat 1.645 (rounded up here), dominant 0.  tests/test_gpu_dec_rescore.py asserts 4 x these.  The dominant
# family's IS zero: ahead by 80, its key has the weight 1 and every other key exp(-80) = 1.8e-35, which no sum beside a
# value of order 1 can see, in fp32 or in float64 - both evaluations return the dominant key's value row EXACTLY.  Four
# times zero is zero: in this family the kernel is held to the exact result.
KAPPA_REF = {"flat": 1.7, "dominant": 0.0}


def _model64(name):
    model = oracle_model(name)
    sd = {k: v.double() for k, v in model.sd.items()}
    w = DR.weights64(sd, model.cfg)
    w["pe"] = model.pe[0].double().numpy()
    return model.cfg, sd, model.pe.double(), w


def _oracle_teacher_forced(cfg, sd, pe, E, y):
    from oracle import ref_port as RP
    ys = torch.tensor([[cfg.sos_id] + list(y)], dtype=torch.long)
    x = RP.pos_enc(torch.nn.functional.embedding(ys, sd["decoder.embed.0.weight"]), pe, cfg.d_model, 0)
    mem = torch.from_numpy(E)[None]
    for li in range(cfg.dec_layers):
        x = RP.decoder_layer(sd, li, cfg, x, mem, None)
    logp = torch.log_softmax(RP.linear(RP.layer_norm(x, sd, "decoder.after_norm", cfg.ln_eps), sd, "decoder.output_layer"), -1)
    targets = list(y) + [cfg.eos_id]
    return logp[0, torch.arange(len(targets)), torch.tensor(targets)].numpy()


def _oracle_step_chain(cfg, sd, pe, E, y):
    from oracle import ref_port as RP
    mem, states, out = torch.from_numpy(E)[None], [None], []
    targets = list(y) + [cfg.eos_id]
    for t in range(len(y) + 1):
        ys = torch.tensor([[cfg.sos_id] + list(y[:t])], dtype=torch.long)
        logp, states = RP.decoder_batch_score(sd, cfg, pe, ys, states, mem)
        out.append(float(logp[0, targets[t]]))
    return np.asarray(out)


@pytest.mark.parametrize("name", ["MICRO", "TINY"])
def test_contract_equals_the_oracle_decoder_teacher_forced_and_step_by_step(name):
    cfg, sd, pe, w = _model64(name)
    rng = np.random.default_rng(11)
    worst = 0.0
    for T in FRAMES:
        E = rng.standard_normal((T, cfg.d_model))
        for m in LENGTHS:
            y = [int(c) for c in rng.integers(0, cfg.vocab_size, m)]
            got = DR.tok_att(w, cfg, E, y)
            assert got.shape == (m + 1,)
            a, b = _oracle_teacher_forced(cfg, sd, pe, E, y), _oracle_step_chain(cfg, sd, pe, E, y)
            worst = max(worst, float(np.abs(got - a).max()), float(np.abs(got - b).max()))
    print(f"{name}: largest |contract - oracle| over tok_att: {worst:.3g}")
    assert worst <= 1e-9


def test_rows_sharing_a_prefix_share_its_values():
    cfg, _, _, w = _model64("MICRO")
    rng = np.random.default_rng(5)
    E = rng.standard_normal((7, cfg.d_model))
    a = [int(c) for c in rng.integers(0, cfg.vocab_size, 9)]
    for k in (0, 1, 4, 9):
        b = a[:k] + [int(c) for c in rng.integers(0, cfg.vocab_size, 6)]
        if k < 9 and b[k] == a[k]:
            b[k] = (b[k] + 1) % cfg.vocab_size
        ta, tb = DR.tok_att(w, cfg, E, a), DR.tok_att(w, cfg, E, b)
        # causality: position t sees the labels before it alone.  Equal up to float64 rounding here - numpy's matrix
        # products block by the row count -, bit-equal on the GPU, whose sums are canonical (tests/test_gpu_dec_rescore.py)
        assert ta[:k].shape == tb[:k].shape == (k,) and np.abs(ta[:k] - tb[:k]).max(initial=0.0) <= 1e-11
        if k < 9:
            assert abs(ta[k] - tb[k]) > 1e-6              # ... and the first differing label shows


def _u64(x):
    return np.asarray(x, np.float64).view(np.uint64)


def test_fused_order_and_status_follow_the_rules_bit_for_bit():
    cfg, _, _, w = _model64("MICRO")
    V = cfg.vocab_size
    rng = np.random.default_rng(3)
    E = rng.standard_normal((7, cfg.d_model))
    base = [int(c) for c in rng.integers(0, V, 5)]
    rows = [base, base, base[:3], [1, V, 2], base + [7] * 20, base, [cfg.eos_id, cfg.sos_id], base[:2], []]
    lens = [5, 5, 3, 3, 25, 5, 2, 9, 0]
    lens[7] = 26                                        # a bad length: beyond L
    scores = [-3.0, -3.0, -1.0, -1.0, -1.0, float("nan"), -2.0, -1.0, float("inf")]
    out = DR.rescore(w, cfg, E, rows, lens, scores, w_att=0.7, w_ctc=0.3, beta=0.25, L=25, pe_rows=20, LCAP=64)
    st = out["status"]
    assert list(st) == [0, 0, 0, DR.BAD_TOKEN, DR.TOO_LONG, DR.NONFINITE, 0, DR.BAD_TOKEN, DR.NONFINITE]
    # fused and att, operation by operation
    for h in (0, 1, 2, 6):
        t = DR.tok_att(w, cfg, E, rows[h][:lens[h]])
        att = 0.0
        for v in t:
            att = att + float(v)
        assert _u64(out["att"][h]) == _u64(att)
        want = (np.float64(0.3) * np.float64(scores[h]) + np.float64(0.7) * np.float64(att)) + np.float64(0.25) * np.float64(lens[h])
        assert _u64(out["fused"][h]) == _u64(want)
        assert (_u64(out["tok_att"][h]) == _u64(t)).all()
    for h in (3, 4, 7):                                 # a row with a status: zeros and THE quiet NaN
        assert out["att"][h] == 0.0 and _u64(out["fused"][h]) == np.uint64(0x7FF8000000000000)
        assert out["tok_att"][h].shape == (26,) and not out["tok_att"][h].any()
    assert _u64(out["fused"][5]) == np.uint64(0x7FF8000000000000) and out["att"][5] != 0.0     # NaN score: att is computed
    assert out["fused"][8] == float("inf")
    # rows 0 and 1 tie: the lower row first; rows with a status behind all others in row order
    good = sorted((h for h in range(9) if not st[h]), key=lambda h: (-out["fused"][h], h))
    assert list(out["order"]) == good + [3, 4, 5, 7, 8]
    assert good.index(0) + 1 == good.index(1)
    # a label equal to sos / eos is an ordinary label
    assert st[6] == 0 and math.isfinite(out["fused"][6])
    # T == 0: every row of the job
    none = DR.rescore(w, cfg, np.zeros((0, cfg.d_model)), rows[:3], lens[:3], scores[:3], L=25)
    assert list(none["status"]) == [DR.NO_FRAMES] * 3 and list(none["order"]) == [0, 1, 2] and not none["att"].any()
    # LCAP alone makes a row too long
    assert list(DR.rescore(w, cfg, E, [base], [5], [0.0], L=5, LCAP=5)["status"]) == [DR.TOO_LONG]


def measured_kappa_ref(family):
    worst = 0.0
    for dk in DR.ATTN_DK:
        for causal in (True, False):
            for H, Lq, Lk, q, k, v in DR.attention_cases(family, dk, causal):
                ref, A = DR.seq_attention(q, k, v, H, causal)
                got, _ = DR.seq_attention(q, k, v, H, causal, dtype=np.float32)
                worst = max(worst, DR.kappa(got, ref, A))
    return worst


@pytest.mark.parametrize("family", ["flat", "dominant"])
def test_kappa_ref_of_an_fp32_evaluation(family):
    """the constant the GPU test multiplies by 4 is what a plain fp32 evaluation needs, neither less nor much more"""
    k = measured_kappa_ref(family)
    print(f"kappa_ref[{family}] measured {k:.4g}, constant {KAPPA_REF[family]}")
    assert k <= KAPPA_REF[family]
    assert k >= KAPPA_REF[family] / 2


def test_dominant_family_has_its_key_ahead_by_80():
    rng = np.random.default_rng(1)
    for dk in DR.ATTN_DK:
        q, k, v = DR.attention_family("dominant", 17, 33, 2, dk, rng)
        for h in range(2):
            c = slice(h * dk, (h + 1) * dk)
            s = q[:, c] @ k[:, c].T / math.sqrt(dk)
            assert (s[:, 0] - s[:, 1:].max(-1) >= 80.0).all()


def test_cfgs_cover_the_three_head_dims():
    assert {CFGS[n].d_model // CFGS[n].dec_heads for n in ("MICRO", "TINY", "XL", "L_LIKE")} == {16, 32, 64}
