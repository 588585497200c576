"""CTC prefix beam search at stream level (csrc/streams.hip: sc_streams_set_ctc_beam / sc_stream_ctc_beam;
csrc/stream_readback.hip: sc_ctc_beam_hyps) and decoder-free streams (sc_stream_set_decoder) on the tiny and the XL synthetic model.

The contract (tests/ctc_beam_ref.py) is run on the RAW CTC rows: a handle whose streams are all SC_DECODER_NONE never
runs a decode block, so the rows it holds are the logits its beam launches read (the first decode block of a FULL
stream log-softmaxes its rows in place, in fp32, behind those launches).  Against that run: every int32 equal, pb / pnb
within 64 n_frames 2^-53 max(1, |want|), under the condition that every prune gap of the contract's run is exactly 0 or
at least 1e-6.  Everything else is compared bit for bit with that handle: FULL streams, a batch of both kinds,
continuous batching at queue depth 2, and the Python engine over the HIP kernels.

Measured on an MI355X (printed by the tests): largest |pb, pnb - contract| 0.0015 of the bar; smallest
non-zero prune gap 4.5e-5 (TINY mixed), 4.4e-5 (TINY plain), 5.0e-5 (XL mixed); the Python engine over the HIP kernels
against the C++ engine: 0.0."""
import functools

import numpy as np
import pytest

import ctc_beam_ref as R
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import synth
from speechcatcher_amd.native import EngineError

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-6
NEG = -np.inf
BAR = lambda n_frames, want: 64.0 * max(n_frames, 1) * 2.0 ** -53 * max(1.0, abs(want))   # noqa: E731
CHUNK = 10240
SHAPE = {"TINY": (2, 8), "XL": (8, 6)}      # streams, chunks
# audio seeds per stream slot (those of tests/test_gpu_ctc_draft.py) and (B, C): on the CPU spec engine the smallest
# non-zero prune gap of these tables is 4.4e-5 (TINY, (8, 8)) and 5.0e-5 (XL, (4, 4)); XL at (8, 8) comes down to 5e-6
SEEDS = {"TINY": [7, 10], "XL": [5, 6, 7, 8, 9, 10, 11, 12]}
PROBES = [("TINY", "mixed", (8, 8)), ("TINY", "plain", (8, 8)), ("XL", "mixed", (4, 4))]
KW = dict(max_frames=160, max_tokens=200, pcm_capacity=1 << 17)


@functools.lru_cache(maxsize=None)
def _weights(model, name):
    return packed_weights(model, name, "cuda:0")


def _snapshot(sb, s, nbest):
    st = sb.ctc_beam([s])[0]
    hy = sb.ctc_beam_hyps([s], nbest)[s]
    return st, [(h["ids"], h["frames"], h["pb"], h["pnb"]) for h in hy]


def _bits(snap):
    st, hy = snap
    floats = [v for e in st["entries"] for v in e[4:]] + [v for h in hy for v in h[2:]]
    return ((st["n_frames"], st["n_bad"], st["n_nodes"]), [e[:4] for e in st["entries"]], [h[:2] for h in hy],
            np.asarray(floats, np.float64).tobytes())


def _hyp_bits(sb, ids):
    """(floats compare exactly; not hypotheses_arrays: its padding depends on which streams are listed)"""
    return {s: [(h["yseq"], h["xpos"], h["score"], h["score_dec"], h["score_ctc"]) for h in sb.hypotheses(s)] for s in ids}


INITIAL = ({"n_frames": 0, "n_bad": 0, "n_nodes": 1, "entries": [(0, -1, 0, -1, 0.0, NEG)]}, [([], [], 0.0, NEG)])


def _chunks(p, k, streams=None):
    return [(s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == p["n"] - 1)
            for s in (range(p["S"]) if streams is None else streams)]


def _lockstep(p, none=(), beam=True, read_hyps=False):
    """a handle pushed chunk by chunk; the streams in ``none`` are decoder-free -> (snapshots [k][s] of the beam, hypotheses
    [k] {stream: bits} of the others, the handle)"""
    sb = make_batch(p["model"], p["name"], "native", p["S"], weights=p["w"], **dict(KW, **p["share"]))
    p["share"]["engine"] = sb.engine                                 # (the weights are uploaded once)
    for s in none:
        sb.set_decoder(s, "ctc")
    if beam:
        sb.set_ctc_beam(*p["BC"])
    snaps, hyps = [], []
    full = [s for s in range(p["S"]) if s not in none]
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
        if beam:
            snaps.append([_snapshot(sb, s, p["BC"][0]) for s in range(p["S"])])
        if read_hyps:
            hyps.append(_hyp_bits(sb, full) if full else {})
    return snaps, hyps, sb


@pytest.fixture(scope="module", params=PROBES, ids=lambda q: f"{q[0]}-{q[1]}-B{q[2][0]}C{q[2][1]}")
def probe(request):
    """per model, computed once: the weights, the audio, the lock-step run of a handle whose streams are all decoder-free
    with the option on - beam and n-best of every stream after every chunk -, and its raw CTC rows"""
    name, model, BC = request.param
    S, n = SHAPE[name]
    p = {"name": name, "model": model, "BC": BC, "S": S, "n": n, "w": _weights(model, name), "share": {}}
    p["audio"] = [synth.synth_audio(SEEDS[name][s], CHUNK * n - 1000 * s) for s in range(S)]
    sb = make_batch(model, name, "native", S, weights=p["w"], **KW)
    p["share"]["engine"] = sb.engine
    with pytest.raises(EngineError):
        sb.ctc_beam([0])                                             # off by default
    with pytest.raises(EngineError):
        sb.ctc_beam_hyps([0])
    with pytest.raises(EngineError):
        sb.set_ctc_beam(17, 8)
    with pytest.raises(EngineError):
        sb.set_ctc_beam(8, 0)
    for s in range(S):
        assert sb.decoder(s) == "full"
        sb.set_decoder(s, "ctc")
        assert sb.decoder(s) == "ctc"
    sb.set_ctc_beam(*BC)
    assert _bits(_snapshot(sb, 0, BC[0])) == _bits(INITIAL)
    T, snaps = [[] for _ in range(S)], []
    for k in range(n):
        sb.push(_chunks(p, k))
        for s in range(S):
            T[s].append(int(sb.st[s].T_enc))
        snaps.append([_snapshot(sb, s, BC[0]) for s in range(S)])
        if k == 0:
            with pytest.raises(EngineError):
                sb.set_decoder(0, "full")                            # only before anything of the utterance is taken
    p.update(T=T, snaps=snaps, sb=sb, table=[sb.read_ctc_projected(s) for s in range(S)], blank=sb.cfg.blank_id)
    assert [len(t) for t in p["table"]] == [t[-1] for t in T]
    return p


def test_lockstep_push_of_decoder_free_streams_equals_the_contract_on_the_raw_rows(probe):
    p = probe
    B, C = p["BC"]
    worst, gap, n_tok = 0.0, np.inf, 0
    for s in range(p["S"]):
        rws = R.rows(p["table"][s], p["blank"], C)
        gaps, store = [], []
        state, t_done = R.scan(R.initial(), [], store, 1 << 30, B), 0
        for k in range(p["n"]):
            t = p["T"][s][k]
            state = R.scan(state, rws[t_done:t], store, 1 << 30, B, gaps)
            t_done = t
            near = [g for g in gaps if g != 0.0 and not g >= MIN_GAP]   # the condition, before anything is compared
            assert not near, (s, k, min(near))
            st, hy = p["snaps"][k][s]
            assert (st["n_frames"], st["n_bad"], st["n_nodes"]) == state[:3], (s, k, st, state[:3])
            assert [e[:4] for e in st["entries"]] == [e[:4] for e in state[3]], (s, k)
            for g, w in zip(st["entries"], state[3]):
                for a, b in zip(g[4:], w[4:]):
                    if a == NEG or b == NEG:
                        assert a == b, (s, k, g, w)
                    else:
                        assert abs(a - b) <= BAR(state[0], b), (s, k, a, b)
                        worst = max(worst, abs(a - b) / BAR(state[0], b))
            assert len(hy) == len(state[3])
            for r, (h, e) in enumerate(zip(hy, state[3])):           # the pack launch: the contract's backtrace
                ids, frames = R.backtrace(e, store)
                assert (h[0], h[1]) == (ids, frames) and h[2:] == tuple(st["entries"][r][4:]), (s, k, r)
        gap = min([gap] + [g for g in gaps if g != 0.0])
        n_tok += state[3][0][2]
    print(f"\n{p['name']}-{p['model']} B, C = {p['BC']}: smallest non-zero prune gap {gap:.3e}; {n_tok} tokens in the best "
          f"prefixes; largest |pb, pnb - contract| = {worst:.4f} of the bar")
    assert n_tok >= 8 * p["S"]
    sb = p["sb"]
    # a decoder-free stream: no decode step, the initial hypothesis, the chunk's status as for any stream
    for s in range(p["S"]):
        assert int(sb.st[s].n_steps_total) == 0 and int(sb.st[s].processed_block) == 0
        hy = sb.hypotheses(s)
        assert len(hy) == 1 and hy[0]["yseq"] == [sb.cfg.sos_id] and hy[0]["score"] == 0.0
    # a final chunk, then a reset: the next utterance starts clean, the other streams keep their states, the mode stays
    sb.reset(0)
    assert _bits(_snapshot(sb, 0, B)) == _bits(INITIAL) and sb.decoder(0) == "ctc"
    assert _bits(_snapshot(sb, 1, B)) == _bits(p["snaps"][-1][1])
    sb.push(_chunks(p, 0, [0]))
    assert _bits(_snapshot(sb, 0, B)) == _bits(p["snaps"][0][0])
    assert int(sb.st[0].n_steps_total) == 0
    sb.reset(0)                                                      # (in mid-utterance)
    assert _bits(_snapshot(sb, 0, B)) == _bits(INITIAL)
    sb.set_ctc_beam(0)
    with pytest.raises(EngineError):
        sb.ctc_beam([0])


def test_full_streams_give_the_same_beams_and_the_option_leaves_their_hypotheses_alone(probe):
    p = probe
    on, hyp_on, sb = _lockstep(p, read_hyps=True)
    assert all(int(sb.st[s].n_steps_total) > 0 for s in range(p["S"]))
    _, hyp_off, _ = _lockstep(p, beam=False, read_hyps=True)
    for k in range(p["n"]):
        for s in range(p["S"]):
            assert _bits(on[k][s]) == _bits(p["snaps"][k][s]), (k, s)
        assert hyp_on[k] == hyp_off[k], k
    p["hyp_full"] = hyp_off


def test_a_batch_of_both_kinds_serves_each_as_a_batch_of_its_own_kind(probe):
    p = probe
    none = tuple(range(0, p["S"], 2))
    if "hyp_full" not in p:
        _, p["hyp_full"], _ = _lockstep(p, beam=False, read_hyps=True)
    snaps, hyps, sb = _lockstep(p, none=none, read_hyps=True)
    for k in range(p["n"]):
        for s in range(p["S"]):
            assert _bits(snaps[k][s]) == _bits(p["snaps"][k][s]), (k, s)
        assert hyps[k] == {s: v for s, v in p["hyp_full"][k].items() if s not in none}, k
    for s in range(p["S"]):
        steps = int(sb.st[s].n_steps_total)
        assert (steps == 0) == (s in none), (s, steps)
        if s in none:
            hy = sb.hypotheses(s)
            assert len(hy) == 1 and hy[0]["yseq"] == [sb.cfg.sos_id]


def test_continuous_queue_depth_2_is_bit_identical_to_push(probe):
    p = probe
    S, n = p["S"], p["n"]
    none = tuple(range(1, S, 2))
    sb = make_batch(p["model"], p["name"], "native", S, weights=p["w"], **dict(KW, **p["share"]))
    sb.set_queue_depth(2)
    for s in none:
        sb.set_decoder(s, "ctc")
    sb.set_ctc_beam(*p["BC"])
    nxt, rep, queued_behind = [0] * S, [0] * S, 0

    def feed(s):
        k = nxt[s]
        nxt[s] += 1
        return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == n - 1)

    sb.submit([feed(s) for s in range(S)])
    with pytest.raises(EngineError):
        sb.set_ctc_beam(*p["BC"])                                    # refused while chunks are outstanding
    sb.submit([feed(s) for s in range(S)])
    while sb.outstanding:
        done = sb.poll(1)
        for s in sorted(done):
            queued_behind += nxt[s] > rep[s] + 1                     # a later chunk of the stream is at the engine:
            got = _snapshot(sb, s, p["BC"][0])                       # the state of the chunk that was REPORTED
            assert _bits(got) == _bits(p["snaps"][rep[s]][s]), (s, rep[s])
            rep[s] += 1
        again = [feed(s) for s in sorted(done) if nxt[s] < n]
        if again:
            sb.submit(again)
    assert rep == [n] * S and queued_behind >= S


def test_python_engine_on_the_hip_backend_gives_the_same_states(probe):
    """the same launch over the Python engine's own table, whose CTC rows come from the same GEMM kernel in the same
    summation order: bit for bit the C++ engine's states"""
    p = probe
    from speechcatcher_amd.hip_backend import HipBackend
    sb = make_batch(p["model"], p["name"], HipBackend("cuda:0"), p["S"], weights=p["w"], **KW)
    sb.set_ctc_beam(*p["BC"])
    assert _bits(_snapshot(sb, 0, p["BC"][0])) == _bits(INITIAL)
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
        for s in range(p["S"]):
            assert _bits(_snapshot(sb, s, p["BC"][0])) == _bits(p["snaps"][k][s]), (s, k)
