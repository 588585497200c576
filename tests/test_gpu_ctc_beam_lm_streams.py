"""The n-gram model fused into the CTC beam at stream level (csrc/streams.hip: sc_streams_set_ctc_beam_lm /
sc_stream_ctc_beam_lm; csrc/stream_readback.hip: sc_ctc_beam_hyps_lm) on the tiny synthetic model.

As in tests/test_gpu_ctc_beam_streams.py the contract (tests/ctc_beam_lm_ref.py) is run on the RAW CTC rows of a handle
whose streams are all decoder-free (sc_streams_read_ctc_projected; DESIGN.md 8j says why that handle): every int32 and
every ctx equal, lm bit-equal, pb / pnb within 64 n_frames 2^-53 max(1, |want|), under the condition - asserted first -
that every gap between fused totals at a cut of the contract's run is exactly 0 or at least 1e-6.  Everything else is
compared bit for bit with that handle: FULL streams, a batch of both kinds at queue depth 2 across a reset; the
hypotheses of FULL streams with the model attached, detached and the beam off; the beam without a model against a
handle that never had one."""
import numpy as np
import pytest

import ctc_beam_lm_ref as L
import ctc_beam_ref as R
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import ngram, synth
from speechcatcher_amd.native import EngineError
from test_gpu_ctc_beam_lm import _model
from test_gpu_ctc_beam_streams import BAR, CHUNK, KW, MIN_GAP, NEG, _bits, _chunks, _hyp_bits, _snapshot

pytestmark = pytest.mark.gpu

S, N, BC = 2, 8, (8, 8)
ALPHA, BETA = 0.5, 0.3
AUDIO_SEEDS = [7, 10]


def _snap_lm(sb, s):
    """(the beam's snapshot, the model's side of it)"""
    return _snapshot(sb, s, BC[0]), sb.ctc_beam_lm([s])[0]


def _lm_bits(snap):
    (st, hy), side = snap
    return _bits((st, hy)), np.asarray(side["lm"] + side["fused"], np.float64).tobytes(), side["ctx"]


def _handle(p, none=(), lm=True, beam=True, weights=(ALPHA, BETA), **kw):
    sb = make_batch("mixed", "TINY", "native", S, weights=p["w"], **dict(KW, engine=p["engine"], **kw))
    for s in none:
        sb.set_decoder(s, "ctc")
    if beam:
        sb.set_ctc_beam(*BC)
        if lm:
            sb.set_ctc_beam_lm(p["blob"], *weights)
    return sb


@pytest.fixture(scope="module")
def probe():
    p = {"w": packed_weights("mixed", "TINY", "cuda:0"), "S": S, "n": N}
    p["audio"] = [synth.synth_audio(AUDIO_SEEDS[s], CHUNK * N - 1000 * s) for s in range(S)]
    # a handle that never has a model: its beams, and the raw rows the model is estimated from
    sb = make_batch("mixed", "TINY", "native", S, weights=p["w"], **KW)
    p["engine"] = sb.engine
    for s in range(S):
        sb.set_decoder(s, "ctc")
    with pytest.raises(EngineError, match="beam option is off"):
        sb.set_ctc_beam_lm(ngram.pack({}, sb.cfg.vocab_size), 0.5, 0.0)
    sb.set_ctc_beam(*BC)
    with pytest.raises(EngineError):
        sb.ctc_beam_lm([0])                                          # no model attached
    p["plain"] = []
    for k in range(N):
        sb.push(_chunks(p, k))
        p["plain"].append([_bits(_snapshot(sb, s, BC[0])) for s in range(S)])
    p["table"] = [sb.read_ctc_projected(s) for s in range(S)]
    p["blank"], V = sb.cfg.blank_id, sb.cfg.vocab_size
    assert p["blank"] == 0
    p["lm"] = _model(np.concatenate(p["table"]), V, 3, "dense", 0.5, 5)
    p["blob"] = p["lm"].blob
    with pytest.raises(EngineError, match="vocabulary"):
        sb.set_ctc_beam_lm(ngram.pack({}, V + 1), 0.5, 0.0)
    with pytest.raises(EngineError, match="language model blob"):
        sb.set_ctc_beam_lm(p["blob"][:-3], 0.5, 0.0)
    with pytest.raises(EngineError, match="finite"):
        sb.set_ctc_beam_lm(p["blob"], float("nan"), 0.0)
    # the all-decoder-free handle with the model attached
    sb = _handle(p, none=range(S))
    first = _snap_lm(sb, 0)
    assert first[1] == {"lm": [0.0], "ctx": [p["lm"].start_state], "fused": [0.0]}
    p["T"], p["snaps"] = [[] for _ in range(S)], []
    for k in range(N):
        sb.push(_chunks(p, k))
        for s in range(S):
            p["T"][s].append(int(sb.st[s].T_enc))
        p["snaps"].append([_snap_lm(sb, s) for s in range(S)])
    assert [np.array_equal(sb.read_ctc_projected(s), p["table"][s]) for s in range(S)] == [True] * S
    p["sb"] = sb
    return p


def test_decoder_free_streams_with_the_model_equal_the_contract_on_the_raw_rows(probe):
    p = probe
    B, C = BC
    lm = p["lm"]
    worst, gap, n_tok, differs = 0.0, np.inf, 0, 0
    for s in range(S):
        rws = R.rows(p["table"][s], p["blank"], C)
        gaps, store = [], []
        state, t_done = L.scan(L.initial(lm), [], store, 1 << 30, B, lm, ALPHA, BETA), 0
        for k in range(N):
            t = p["T"][s][k]
            state = L.scan(state, rws[t_done:t], store, 1 << 30, B, lm, ALPHA, BETA, gaps)
            t_done = t
            near = [g for g in gaps if g != 0.0 and not g >= MIN_GAP]   # the condition, before anything is compared
            assert not near, (s, k, min(near))
            (st, hy), side = p["snaps"][k][s]
            assert (st["n_frames"], st["n_bad"], st["n_nodes"]) == state[:3], (s, k, st, state[:3])
            assert [e[:4] for e in st["entries"]] == [e[:4] for e in state[3]], (s, k)
            assert side["ctx"] == [sd[1] for sd in state[4]], (s, k)
            assert np.asarray(side["lm"], np.float64).tobytes() == np.asarray([sd[0] for sd in state[4]]).tobytes(), (s, k)
            for g, w in zip(st["entries"], state[3]):
                for a, b in zip(g[4:], w[4:]):
                    if a == NEG or b == NEG:
                        assert a == b, (s, k, g, w)
                    else:
                        assert abs(a - b) <= BAR(state[0], b), (s, k, a, b)
                        worst = max(worst, abs(a - b) / BAR(state[0], b))
            for f, e, sd in zip(side["fused"], state[3], state[4]):   # the fused score the reader reports
                want = L.fused(e, sd, ALPHA, BETA)
                assert abs(f - want) <= BAR(state[0], want), (s, k, f, want)
            assert side["fused"] == sorted(side["fused"], reverse=True)
            for r, (h, e) in enumerate(zip(hy, state[3])):           # the pack launch: the contract's backtrace
                assert (h[0], h[1]) == R.backtrace(e, store), (s, k, r)
            differs += p["plain"][k][s][1] != [e[:4] for e in state[3]]
        gap = min([gap] + [g for g in gaps if g != 0.0])
        n_tok += state[3][0][2]
    print(f"\nTINY-mixed B, C = {BC}, order {lm.b.order}, {lm.b.n_arcs} arcs: smallest non-zero gap between fused totals "
          f"{gap:.3e}; {n_tok} tokens in the best prefixes; largest |pb, pnb - contract| = {worst:.4f} of the bar; the "
          f"beam differs from the unfused one after {differs} of {S * N} chunks; lookups by backoff depth {lm.depth[:4]}")
    assert n_tok >= 8 * S and differs > 0
    sb = p["sb"]
    # a reset: the next utterance starts clean, the other stream keeps its state
    sb.reset(0)
    assert _lm_bits(_snap_lm(sb, 0))[1:] == (np.asarray([0.0, 0.0]).tobytes(), [lm.start_state])
    assert _lm_bits(_snap_lm(sb, 1)) == _lm_bits(p["snaps"][-1][1])
    sb.push(_chunks(p, 0, [0]))
    assert _lm_bits(_snap_lm(sb, 0)) == _lm_bits(p["snaps"][0][0])


def test_full_streams_give_the_same_beams_and_their_hypotheses_do_not_depend_on_the_model(probe):
    p = probe
    runs = {}
    for what, kw in {"attached": dict(), "detached": dict(lm=False), "beam off": dict(beam=False)}.items():
        sb = _handle(p, **kw)
        hyps = []
        for k in range(N):
            sb.push(_chunks(p, k))
            hyps.append(_hyp_bits(sb, range(S)))
            if what == "attached":
                for s in range(S):
                    assert _lm_bits(_snap_lm(sb, s)) == _lm_bits(p["snaps"][k][s]), (k, s)
            if what == "detached":                                   # no model: the beams of a handle that never had one
                assert [_bits(_snapshot(sb, s, BC[0])) for s in range(S)] == p["plain"][k], k
        assert all(int(sb.st[s].n_steps_total) > 0 for s in range(S))
        runs[what] = hyps
    assert runs["attached"] == runs["detached"] == runs["beam off"]
    assert len(runs["attached"][-1][0][0][0]) > 1                    # (yseq of stream 0's best hypothesis)


def test_without_a_model_the_beam_is_the_one_of_a_handle_that_never_had_one(probe):
    p = probe
    for what in ("attached and detached", "zero weights"):
        sb = _handle(p, none=[1], weights=(0.0, 0.0))
        if what == "attached and detached":
            sb.set_ctc_beam_lm(None)
            with pytest.raises(EngineError):
                sb.ctc_beam_lm([0])
        for k in range(N):
            sb.push(_chunks(p, k))
            assert [_bits(_snapshot(sb, s, BC[0])) for s in range(S)] == p["plain"][k], (what, k)


def test_a_batch_of_both_kinds_at_queue_depth_2_across_a_reset_is_bit_identical(probe):
    p = probe
    # (strict_reference off: with it on a reset keeps the stale table, and rows that are not projected again are not
    # searched - sc_streams_set_ctc_beam)
    sb = _handle(p, none=[1], strict_reference=False)
    sb.set_queue_depth(2)
    for rnd, n in enumerate((N, 3)):                                 # the whole utterance; a reset; its first chunks again
        nxt, rep, queued_behind = [0] * S, [0] * S, 0

        def feed(s):
            k = nxt[s]
            nxt[s] += 1
            return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == N - 1)

        sb.submit([feed(s) for s in range(S)])
        with pytest.raises(EngineError):
            sb.set_ctc_beam_lm(p["blob"], ALPHA, BETA)               # refused while chunks are outstanding
        sb.submit([feed(s) for s in range(S)])
        while sb.outstanding:
            done = sb.poll(1)
            for s in sorted(done):
                queued_behind += nxt[s] > rep[s] + 1
                assert _lm_bits(_snap_lm(sb, s)) == _lm_bits(p["snaps"][rep[s]][s]), (rnd, s, rep[s])
                rep[s] += 1
            again = [feed(s) for s in sorted(done) if nxt[s] < n]
            if again:
                sb.submit(again)
        assert rep == [n] * S and queued_behind >= S
        for s in range(S):
            sb.reset(s)
    assert sb.decoder(1) == "ctc"
