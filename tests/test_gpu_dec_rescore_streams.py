"""Attention rescoring at stream level (csrc/stream_readback.hip: sc_attention_rescore_beam, sc_attention_rescore_lists; DESIGN.md
8n) on the tiny synthetic model.

On a handle whose streams are all decoder-free, attention_rescore_beam equals the contract (tests/dec_rescore_ref.py) run
on the stream's encoder output (sc_streams_read_enc) and the entries of sc_ctc_beam_hyps: integers equal - the order
wherever the contract's neighbouring fused values tie or lie 4e-3 apart, twice the bar on att -, att within 1e-3.
attention_rescore_lists gives the same bits for the same entries, also with the workspace limited so that the call runs
in slabs.  In a mixed batch under continuous batching at queue depth 2 and across a reset, the FULL streams' hypotheses
and the decoder-free streams' beam states are bit-identical with the calls made and not made.  The scheduler on the native
batch: a "rescore" session's final carries the new fields in the contract's order."""
import numpy as np
import pytest

import dec_rescore_ref as DR
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import synth
from speechcatcher_amd.native import EngineError
from test_gpu_ctc_beam_streams import CHUNK, KW, _chunks, _hyp_bits, _snapshot

pytestmark = pytest.mark.gpu

S, N, B = 2, 6, 8
W_ATT, W_CTC, BETA = 0.9, 0.4, 0.1
ATT_BAR = 1e-3


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).tolist()


def _lae(a, b):
    hi, lo = max(a, b), min(a, b)
    return hi if lo == -np.inf else hi + np.log1p(np.exp(lo - hi))


@pytest.fixture(scope="module")
def probe():
    p = {"w": packed_weights("mixed", "TINY", "cuda:0"), "S": S, "n": N, "share": {}}
    p["w64"] = DR.weights64_packed(p["w"])
    p["audio"] = [synth.synth_audio([7, 10][s], CHUNK * N - 1000 * s) for s in range(S)]
    return p


def _batch(p, none=(), depth=1):
    sb = make_batch("mixed", "TINY", "native", S, weights=p["w"], **dict(KW, **p["share"]))
    p["share"]["engine"] = sb.engine
    for s in none:
        sb.set_decoder(s, "ctc")
    sb.set_ctc_beam(B, B)
    if depth > 1:
        sb.set_queue_depth(depth)
    return sb


def _against_contract(p, sb, streams):
    cfg = sb.cfg
    hyps = sb.ctc_beam_hyps(streams, B)
    before = [_snapshot(sb, s, B) for s in streams]
    got = sb.attention_rescore_beam(streams, B, W_ATT, W_CTC, BETA)
    assert [_snapshot(sb, s, B) for s in streams] == before                    # the call changed nothing
    worst = 0.0
    for s in streams:
        rows = [h["ids"] for h in hyps[s]]
        scores = [_lae(h["pb"], h["pnb"]) for h in hyps[s]]
        E = sb.encoder_buffer(s)
        want = DR.rescore(p["w64"], cfg, E, rows, [len(r) for r in rows], scores, W_ATT, W_CTC, BETA, LCAP=sb.LCAP)
        g = got[s]
        assert len(g["order"]) == len(rows) and _u64(g["ctc_score"]) == _u64(scores)
        assert g["status"].tolist() == want["status"].tolist() and not want["status"].any()
        worst = max(worst, float(np.abs(g["att"] - want["att"]).max()))
        gaps = np.diff(np.sort(want["fused"]))
        if ((gaps == 0.0) | (gaps >= 4e-3)).all():
            assert g["order"].tolist() == want["order"].tolist(), s
        assert sorted(g["order"].tolist()) == list(range(len(rows)))
        f = g["fused"][g["order"]]
        assert (np.diff(f) <= 0).all()                                         # ranked by its own fused values
        assert np.abs(g["fused"] - want["fused"]).max() <= 2 * ATT_BAR
        # the same entries as caller-given lists: the same bits
        li = sb.attention_rescore_lists([s], [rows], [scores], W_ATT, W_CTC, BETA)[0]
        for key in ("att", "fused"):
            assert _u64(li[key]) == _u64(g[key]), key
        assert li["order"].tolist() == g["order"].tolist() and li["status"].tolist() == g["status"].tolist()
    assert worst <= ATT_BAR
    return got, worst


def test_decoder_free_streams_equal_the_contract_and_lists_equal_the_beam(probe):
    p = probe
    sb = _batch(p, none=range(S))
    assert sb.attention_rescore_workspace() == (256 << 20, 0)                  # nothing is allocated before the first call
    empty = sb.attention_rescore_beam([0, 1], B, W_ATT, W_CTC, BETA)          # no frames yet: one empty prefix, NO_FRAMES
    assert all(empty[s]["status"].tolist() == [DR.NO_FRAMES] and empty[s]["att"].tolist() == [0.0] for s in range(S))
    worst = 0.0
    for k in range(N):
        sb.push(_chunks(p, k))
        if k in (2, N - 1):                                                    # a partial and the final
            got, w = _against_contract(p, sb, [0, 1])
            worst = max(worst, w)
    print(f"\nattention_rescore_beam TINY: largest |att - contract| {worst:.3g}")
    limit, allocated = sb.attention_rescore_workspace()
    assert 0 < allocated <= limit
    # a limit one stream's list fits and two do not: the call runs in slabs, with the same bits
    sb.set_attention_rescore_workspace(max(1 << 20, int(0.7 * allocated)))
    again = sb.attention_rescore_beam([0, 1], B, W_ATT, W_CTC, BETA)
    assert sb.attention_rescore_workspace()[1] <= max(1 << 20, int(0.7 * allocated))
    for s in range(S):
        for key in ("att", "fused"):
            assert _u64(again[s][key]) == _u64(got[s][key])
        assert again[s]["order"].tolist() == got[s]["order"].tolist()
    with pytest.raises(EngineError, match="listed twice"):
        sb.attention_rescore_beam([0, 0], B)
    with pytest.raises(EngineError, match="finite"):
        sb.attention_rescore_beam([0], B, w_att=float("nan"))
    sb.reset(0)                                                                # after a reset a stream has no frames
    assert sb.attention_rescore_beam([0], B)[0]["status"].tolist() == [DR.NO_FRAMES]


def _run_mixed(p, calls):
    """streams 0 FULL, 1 decoder-free, queue depth 2: two chunks submitted per round, then polled; -> the FULL stream's
    hypotheses and the other's beam after every round, and across a reset"""
    sb = _batch(p, none=[1], depth=2)
    trace, outs = [], []
    for k in range(0, N, 2):
        sb.submit(_chunks(p, k))
        sb.submit(_chunks(p, k + 1))
        if calls and k == 0:
            with pytest.raises(EngineError, match="outstanding"):
                sb.attention_rescore_beam([1], B)
        while sb.outstanding:
            sb.poll(1)
        if calls:
            # (the first chunks may leave the encoder without a block: no frames yet)
            want = [DR.NO_FRAMES if sb.encoder_buffer(s) is None else 0 for s in range(S)]
            outs.append(sb.attention_rescore_beam([1], B, W_ATT, W_CTC, BETA)[1])
            assert set(outs[-1]["status"].tolist()) == {want[1]}
            rows = [h["yseq"][1:] for h in sb.hypotheses(0)][:4]
            rows = [[t for t in r if t != sb.cfg.eos_id] for r in rows]
            if rows:                                                           # a FULL stream's own hypotheses against its enc
                li = sb.attention_rescore_lists([0, 1], [rows, rows], [[0.0] * len(rows)] * 2, W_ATT, W_CTC, BETA)
                for s in range(S):
                    assert set(li[s]["status"].tolist()) == {want[s]} and np.isfinite(li[s]["att"]).all()
        trace.append((_hyp_bits(sb, [0]), _snapshot(sb, 1, B)))
    sb.reset(1)
    if calls:
        assert sb.attention_rescore_beam([1], B)[1]["status"].tolist() == [DR.NO_FRAMES]
    sb.push(_chunks(p, 0, [1]))
    if calls:
        outs.append(sb.attention_rescore_beam([1], B, W_ATT, W_CTC, BETA)[1])
    trace.append((_hyp_bits(sb, [0]), _snapshot(sb, 1, B)))
    return trace, outs


def test_mixed_batch_at_queue_depth_2_the_calls_only_read(probe):
    plain, _ = _run_mixed(probe, calls=False)
    with_calls, outs = _run_mixed(probe, calls=True)
    assert with_calls == plain
    assert all(np.isfinite(o["att"]).all() for o in outs) and not outs[-2]["status"].any()      # (the final's list)
    assert sum(1 for o in outs if not o["status"].any()) >= 2


def test_scheduler_on_the_native_batch_a_rescore_final_carries_the_contracts_order(probe):
    from speechcatcher_amd.scheduler import CtcBeamResults, StreamScheduler
    p = probe
    sb = make_batch("mixed", "TINY", "native", S, weights=p["w"], **dict(KW, **p["share"]))
    sch = StreamScheduler(sb, None, ctc_beam=(B, B), attention_rescore=(W_ATT, W_CTC, BETA), reset_after_final=False)
    free, full = sch.open(decoder="rescore"), sch.open()
    out = {}
    for k in range(N):
        for sid, s in ((free, 0), (full, 1)):
            sch.feed(sid, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == N - 1)
        out = sch.step()
        if k < N - 1:
            assert all("att" not in e for e in out[free].ctc_nbest)             # partials: the beam's entries as they are
    nb = out[free].ctc_nbest
    assert isinstance(out[free], CtcBeamResults) and nb and all({"att", "ctc_score", "am_rank", "score", "conf"} <= set(e) for e in nb)
    assert "att" not in (out[full].ctc_nbest or [{}])[0]                       # the FULL session is untouched
    hyps = sb.ctc_beam_hyps([0], B)[0]
    rows, scores = [h["ids"] for h in hyps], [_lae(h["pb"], h["pnb"]) for h in hyps]
    want = DR.rescore(p["w64"], sb.cfg, sb.encoder_buffer(0), rows, [len(r) for r in rows], scores, W_ATT, W_CTC, BETA,
                      LCAP=sb.LCAP)
    assert [e["ids"] for e in nb] == [rows[e["am_rank"]] for e in nb] and sorted(e["am_rank"] for e in nb) == list(range(len(rows)))
    gaps = np.diff(np.sort(want["fused"]))
    if ((gaps == 0.0) | (gaps >= 4e-3)).all():
        assert [e["am_rank"] for e in nb] == want["order"].tolist()
    assert max(abs(e["att"] - want["att"][e["am_rank"]]) for e in nb) <= ATT_BAR
    assert [e["score"] for e in nb] == sorted((e["score"] for e in nb), reverse=True)
    assert abs(sum(e["conf"] for e in nb) - 1.0) < 1e-9
