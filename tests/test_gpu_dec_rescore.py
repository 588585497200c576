"""Attention rescoring on the GPU (csrc/dec_rescore.hip) against the float64 contract of tests/dec_rescore_ref.py.

1. sc_seq_attention alone: head dims 16 / 32 / 64, 1 / 2 / 8 heads, the lengths at which a tile of 16 queries or keys
   fills, overflows by one or is left almost empty, causal and full, ragged sequences of one launch, row strides wider
   than the rows.  The bar is kappa <= 4 x KAPPA_REF (tests/dec_attn_ref.py's convention; kappa with A of a context
   element), KAPPA_REF being what tests/test_dec_rescore_spec.py measured on a plain fp32 evaluation of the same
   operands: flat 1.645 -> 1.7; dominant 0 -> 0, i.e. the exact result.  K|V rows at or beyond Lk and every padding
   element hold NaN: the output is finite and bit-identical to the run with zeros there; a causal row i is bit-identical
   when Lq is cut to i + 1.
2. sc_dec_rescore against the contract at MICRO, TINY and XL dims: integers equal, att within 1e-3 absolute (the
   project's bar for cumulative fp32 scores; README, Parity), every status.
3. Bits: a row alone, in a list of 16, beside other jobs and with the workspace cut into slabs; rows sharing a prefix."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dec_rescore_ref as DR
from helpers import oracle_model
from speechcatcher_amd import _abi

pytestmark = pytest.mark.gpu

KAPPA_REF = {"flat": 1.7, "dominant": 0.0}      # tests/test_dec_rescore_spec.py::test_kappa_ref_of_an_fp32_evaluation
ATT_BAR = 1e-3
LCAP = 64
PAD = 12                                         # extra floats per row: strides wider than the rows, still 16-byte steps


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


# ---- 1. sc_seq_attention ---------------------------------------------------------------------------------------------
def _padded(a, rows, fill, dev):
    """a [n][w] inside a [rows][w + PAD] tensor of ``fill``"""
    t = torch.full((rows, a.shape[1] + PAD), fill, dtype=torch.float32)
    t[:a.shape[0], :a.shape[1]] = torch.from_numpy(a.astype(np.float32))
    return t.to(dev)


def _attn_jobs(cases, dk, causal, fill, dev, cuts=()):
    jobs = []
    for H, Lq, Lk, q, k, v in cases:
        jobs.append({"q": _padded(q, Lq + 2, fill, dev), "k": _padded(k, Lk + 3, fill, dev), "v": _padded(v, Lk + 3, fill, dev),
                     "o": torch.full((Lq + 2, H * dk + PAD), -77.25, dtype=torch.float32, device=dev),
                     "Lq": Lq, "Lk": Lk, "H": H, "causal": causal})
    for src, i in cuts:     # the same sequence with Lq (= Lk) cut to i + 1
        j = dict(jobs[src])
        j.update(o=torch.full_like(j["o"], -77.25), Lq=i + 1, Lk=i + 1)
        jobs.append(j)
    return jobs


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dk", DR.ATTN_DK)
@pytest.mark.parametrize("family", DR.FAMILIES)
def test_seq_attention_against_float64(be, family, dk, causal):
    cases = list(DR.attention_cases(family, dk, causal))
    # causal: the longest sequence of every H again with Lq cut to i + 1
    longest = [n for n, c in enumerate(cases) if c[1] == max(DR.ATTN_LQ)]
    cuts = [(n, i) for n in longest for i in (0, 14, 15, 16, 40)] if causal else []
    runs = []
    for fill in (float("nan"), 0.0):
        jobs = _attn_jobs(cases, dk, causal, fill, be.device, cuts)
        be.seq_attention(jobs, dk)
        runs.append([j["o"].cpu().numpy() for j in jobs])
    worst = 0.0
    for n, (H, Lq, Lk, q, k, v) in enumerate(cases):
        o = runs[0][n]
        ref, A = DR.seq_attention(q, k, v, H, causal)
        got = o[:Lq, :H * dk]
        assert np.isfinite(got).all()
        assert (o[Lq:] == -77.25).all() and (o[:, H * dk:] == -77.25).all()          # nothing else is written
        worst = max(worst, DR.kappa(got, ref, A))
        assert (o.view(np.uint32) == runs[1][n].view(np.uint32)).all()               # NaN or zeros behind Lk: the same bits
    print(f"sc_seq_attention {family} dk {dk} {'causal' if causal else 'full'}: kappa {worst:.3f} "
          f"(bar {4 * KAPPA_REF[family]:.1f})")
    assert worst <= 4 * KAPPA_REF[family]
    for c, (src, i) in enumerate(cuts):
        whole, cut = runs[0][src], runs[0][len(cases) + c]
        assert (whole[i].view(np.uint32) == cut[i].view(np.uint32)).all(), (src, i)
        assert (cut[i + 1:] == -77.25).all()


def test_seq_attention_malformed_jobs_write_nothing(be):
    H, dk = 2, 16
    case = next(iter(DR.attention_cases("flat", dk, False)))
    bad = [("q", 0), ("o", 0), ("Lq", -1), ("Lq", 1000), ("H", 0), ("H", 9), ("causal", 2), ("Lk", 0), ("k_stride", 3),
           ("v_stride", H * dk + 2), ("q", "odd")]
    jobs = _attn_jobs([case] * (len(bad) + 1), dk, False, 0.0, be.device)

    def tweak(k, j):
        if k < len(bad):
            name, val = bad[k]
            setattr(j, name, getattr(j, name) + 4 if val == "odd" else val)
    be.seq_attention(jobs, dk, tweak=tweak)
    for k in range(len(bad)):
        assert (jobs[k]["o"] == -77.25).all(), bad[k]
    assert torch.isfinite(jobs[-1]["o"][:case[1], :case[0] * dk]).all()


# ---- 2. sc_dec_rescore against the contract ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name):
    from speechcatcher_amd.weights import PackedWeights
    om = oracle_model(name)
    w64 = DR.weights64(om.sd, om.cfg)
    w64["pe"] = om.pe[0].double().numpy()
    return om.cfg, w64, PackedWeights(om.sd, om.cfg, "cuda:0")


def _labels(rng, V, m):
    return [int(c) for c in rng.integers(0, V, m)]


def _plan_scores(ref_att, lens, w_att, w_ctc, beta, rng, ties=()):
    """first-pass totals under which the CONTRACT's fused values lie 0.05 apart (or tie exactly, for the pairs in ties)"""
    n = len(lens)
    slot = rng.permutation(n).astype(np.float64)
    for a, b in ties:
        slot[b] = slot[a]
    target = -20.0 - 0.05 * slot
    sc = (target - w_att * ref_att - beta * np.asarray(lens, np.float64)) / w_ctc
    for a, b in ties:
        sc[b] = sc[a]
    return sc


def _dev_job(rows, lens, scores, E, L, dev, **kw):
    yseq = torch.full((len(rows), L + 3), -5, dtype=torch.int32)
    for h, r in enumerate(rows):
        yseq[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
    job = {"rows": yseq.to(dev), "scores": torch.tensor(np.asarray(scores, np.float64)).to(dev), "lens": list(lens), "L": L,
           "E": None if E is None else torch.from_numpy(np.asarray(E, np.float32)).to(dev)}
    job.update(kw)
    return job


def _check(got, ref, lens, tag):
    """integers equal; att within the bar; returns the largest att and tok_att error"""
    assert list(got["status"]) == list(ref["status"]), tag
    assert list(got["order"]) == list(ref["order"]), tag
    e_att = e_tok = 0.0
    for h in range(len(lens)):
        if ref["status"][h] & ~DR.NONFINITE:
            assert got["att"][h] == 0.0 and np.isnan(got["fused"][h]) and not got["tok_att"][h].any(), (tag, h)
            continue
        m = lens[h]
        e_att = max(e_att, abs(got["att"][h] - ref["att"][h]))
        e_tok = max(e_tok, float(np.abs(got["tok_att"][h][:m + 1] - ref["tok_att"][h]).max()))
        assert (got["tok_att"][h][m + 1:] == -7.0).all(), (tag, h)       # nothing behind the m + 1 values is written
        if np.isfinite(ref["fused"][h]):
            assert abs(got["fused"][h] - ref["fused"][h]) <= ATT_BAR * 2, (tag, h)
    assert e_att <= ATT_BAR, (tag, e_att)
    return e_att, e_tok


@pytest.mark.parametrize("name", ["MICRO", "TINY"])
def test_dec_rescore_against_the_contract(be, name):
    cfg, w64, pw = _model(name)
    model = be.decoder_model(pw, LCAP)
    rng = np.random.default_rng(17)
    lengths = (0, 1, 2, 5, 17, 33)
    w_att, w_ctc, beta = 0.8, 0.4, 0.125
    jobs, refs, all_lens = [], [], []
    for T, N in ((1, 1), (7, 3), (33, 16), (70, 3), (7, 16), (70, 1)):
        E = rng.standard_normal((T, cfg.d_model)).astype(np.float32)
        lens = [lengths[(h + T) % len(lengths)] for h in range(N)]
        rows = [_labels(rng, cfg.vocab_size, m) for m in lens]
        ties = []
        if N == 16:
            rows[9], lens[9] = list(rows[4]), lens[4]        # the same row twice: an exact tie, the lower row first
            ties = [(4, 9)]
        L = max(lens) + (T % 3)                              # row capacities above the longest row too
        pre = DR.rescore(w64, cfg, E, rows, lens, np.zeros(N), w_att, w_ctc, beta, L=L, LCAP=LCAP)
        scores = _plan_scores(pre["att"], lens, w_att, w_ctc, beta, rng, ties)
        ref = DR.rescore(w64, cfg, E, rows, lens, scores, w_att, w_ctc, beta, L=L, LCAP=LCAP)
        # from the contract alone: neighbouring fused values tie exactly or lie at least 4e-3 apart
        f = np.sort(ref["fused"])
        gaps = np.diff(f)
        assert ((gaps == 0.0) | (gaps >= 4e-3)).all() and not ref["status"].any()
        assert (gaps == 0.0).sum() == len(ties)
        jobs.append(_dev_job(rows, lens, scores, E, L, be.device, w_att=w_att, w_ctc=w_ctc, beta=beta))
        refs.append(ref)
        all_lens.append(lens)
    got = be.dec_rescore(jobs, model)
    e_att = e_tok = 0.0
    for k in range(len(jobs)):
        a, t = _check(got[k], refs[k], all_lens[k], (name, k))
        e_att, e_tok = max(e_att, a), max(e_tok, t)
        assert (got[k]["raw"]["f64"][:, len(all_lens[k]):] == -7.0).all() and (got[k]["raw"]["i32"][:, len(all_lens[k]):] == -7).all()
    print(f"sc_dec_rescore {name}: largest |att - contract| {e_att:.3g}, per token {e_tok:.3g}")


def test_dec_rescore_xl_dims(be):
    cfg, w64, pw = _model("XL")
    model = be.decoder_model(pw, LCAP)
    rng = np.random.default_rng(23)
    E = rng.standard_normal((40, cfg.d_model)).astype(np.float32)
    lens = [12, 7, 0, 11]
    rows = [_labels(rng, cfg.vocab_size, m) for m in lens]
    pre = DR.rescore(w64, cfg, E, rows, lens, np.zeros(4), L=12, LCAP=LCAP)
    scores = _plan_scores(pre["att"], lens, 1.0, 0.5, 0.0, rng)
    ref = DR.rescore(w64, cfg, E, rows, lens, scores, L=12, LCAP=LCAP)
    gaps = np.diff(np.sort(ref["fused"]))
    assert (gaps >= 4e-3).all()
    got = be.dec_rescore([_dev_job(rows, lens, scores, E, 12, be.device)], model)[0]
    e_att, e_tok = _check(got, ref, lens, "XL")
    print(f"sc_dec_rescore XL: largest |att - contract| {e_att:.3g}, per token {e_tok:.3g}")


def test_dec_rescore_every_status(be):
    cfg, w64, pw = _model("MICRO")
    model = be.decoder_model(pw, LCAP)
    V = cfg.vocab_size
    rng = np.random.default_rng(3)
    E = rng.standard_normal((7, cfg.d_model)).astype(np.float32)
    base = _labels(rng, V, 5)
    rows = [base, base, base[:3], [1, V, 2], base + [7] * 20, base, [cfg.eos_id, cfg.sos_id], base[:2], [], [3, -1]]
    lens = [5, 5, 3, 3, 25, 5, 2, 26, 0, 2]
    scores = [-3.0, -3.0, -1.0, -1.0, -1.0, float("nan"), -2.0, -1.0, float("inf"), -1.0]
    kw = dict(w_att=0.7, w_ctc=0.3, beta=0.25)
    ref = DR.rescore(w64, cfg, E, rows, lens, scores, L=25, pe_rows=20, LCAP=LCAP, **kw)
    assert list(ref["status"]) == [0, 0, 0, DR.BAD_TOKEN, DR.TOO_LONG, DR.NONFINITE, 0, DR.BAD_TOKEN, DR.NONFINITE, DR.BAD_TOKEN]
    jobs = [_dev_job(rows, lens, scores, E, 25, be.device, pe_rows=20, **kw),
            _dev_job(rows[:3], lens[:3], scores[:3], None, 25, be.device, **kw),                  # T == 0
            _dev_job([base + [1] * (LCAP - 5)], [LCAP], [0.0], E, LCAP, be.device, **kw)]         # LCAP alone: too long
    got = be.dec_rescore(jobs, model)
    assert list(got[0]["status"]) == list(ref["status"]) and list(got[0]["order"]) == list(ref["order"])
    for h in range(len(rows)):
        if ref["status"][h] & ~DR.NONFINITE:
            assert got[0]["att"][h] == 0.0 and not got[0]["tok_att"][h].any()
            assert got[0]["fused"][h:h + 1].view(np.uint64)[0] == 0x7FF8000000000000
        else:
            assert abs(got[0]["att"][h] - ref["att"][h]) <= ATT_BAR
    assert got[0]["fused"][5:6].view(np.uint64)[0] == 0x7FF8000000000000 and got[0]["fused"][8] == float("inf")
    assert got[0]["fused"][0:1].view(np.uint64)[0] == got[0]["fused"][1:2].view(np.uint64)[0]     # the tie is exact
    none = DR.rescore(w64, cfg, None, rows[:3], lens[:3], scores[:3], L=25, **kw)
    assert list(got[1]["status"]) == list(none["status"]) == [DR.NO_FRAMES] * 3 and list(got[1]["order"]) == [0, 1, 2]
    assert not got[1]["att"].any() and np.isnan(got[1]["fused"]).all() and not got[1]["tok_att"].any()
    assert list(got[2]["status"]) == [DR.TOO_LONG]


def test_dec_rescore_errors_write_nothing(be):
    cfg, w64, pw = _model("MICRO")
    model = be.decoder_model(pw, LCAP)
    rng = np.random.default_rng(4)
    E = rng.standard_normal((7, cfg.d_model)).astype(np.float32)
    job = _dev_job([_labels(rng, cfg.vocab_size, 5)], [5], [0.0], E, 5, be.device)
    with pytest.raises(_abi.ScasrError, match="workspace"):
        be.dec_rescore([job], model, ws_bytes=4096)
    with pytest.raises(_abi.ScasrError, match="n_hyp"):
        be.dec_rescore([job, job], model, tweak=lambda k, j: setattr(j, "n_hyp", 17 if k else 1))
    model.layers[1].wo2 = None
    try:
        with pytest.raises(_abi.ScasrError, match=r"\(-5\).*fp32 decoder weights"):
            be.dec_rescore([job], model)
    finally:
        model.layers[1].wo2 = pw.dec[1]["wo2"].data_ptr()
    assert np.isfinite(be.dec_rescore([job], model)[0]["att"]).all()


# ---- 3. bits ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ["MICRO", "XL"])
def test_a_rows_bits_do_not_depend_on_its_company_or_on_the_slabs(be, name):
    cfg, _, pw = _model(name)
    model = be.decoder_model(pw, LCAP)
    rng = np.random.default_rng(29)
    V, d = cfg.vocab_size, cfg.d_model
    E = rng.standard_normal((33, d)).astype(np.float32)
    E2 = rng.standard_normal((7, d)).astype(np.float32)
    m = 17
    row = _labels(rng, V, m)
    alone = be.dec_rescore([_dev_job([row], [m], [0.0], E, m, be.device)], model)[0]["tok_att"][0]
    assert np.isfinite(alone).all()
    others = [_labels(rng, V, (3 * h) % 20) for h in range(15)]
    rows16, lens16 = others[:6] + [row] + others[6:], [len(r) for r in others[:6]] + [m] + [len(r) for r in others[6:]]
    big = _dev_job(rows16, lens16, np.zeros(16), E, 20, be.device)
    side = [_dev_job(others[:3], [len(r) for r in others[:3]], np.zeros(3), E2, 9, be.device) for _ in range(2)]
    in16 = be.dec_rescore([big], model)[0]["tok_att"][6][:m + 1]
    beside = be.dec_rescore([side[0], big, side[1]], model)
    assert (_bits(in16) == _bits(alone[:m + 1])).all()
    assert (_bits(beside[1]["tok_att"][6][:m + 1]) == _bits(alone[:m + 1])).all()
    # a workspace that holds the largest job and no second one: the call runs in slabs, with the same bits
    need = int(be.lib.sc_dec_rescore_ws_bytes(ctypes.addressof(model.struct), 16 * 21, 33, 16, 1))
    assert need < int(be.lib.sc_dec_rescore_ws_bytes(ctypes.addressof(model.struct), 16 * 21 + 30, 40, 19, 2))
    slabs = be.dec_rescore([side[0], big, side[1]], model, ws_bytes=need)
    for k in range(3):
        assert (_bits(slabs[k]["tok_att"]) == _bits(beside[k]["tok_att"])).all()
        assert (_bits(slabs[k]["att"]) == _bits(beside[k]["att"])).all() and list(slabs[k]["order"]) == list(beside[k]["order"])
    # rows sharing their first k labels: tok_att[0..k) bit-equal
    for k in (0, 1, 4, 16, 17):
        b = row[:k] + _labels(rng, V, 6)
        if k < m and b[k] == row[k]:
            b[k] = (b[k] + 1) % V
        got = be.dec_rescore([_dev_job([b, row], [len(b), m], [0.0, 0.0], E, max(len(b), m), be.device)], model)[0]["tok_att"]
        assert (_bits(got[0][:k]) == _bits(got[1][:k])).all() and (_bits(got[1][:m + 1]) == _bits(alone[:m + 1])).all()
        if k < m:
            assert got[0][k] != got[1][k]
