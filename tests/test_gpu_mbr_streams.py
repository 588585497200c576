"""Consensus finals at stream level (csrc/stream_readback.hip: sc_mbr_hyps, sc_mbr_lists) on the tiny synthetic
model.

sc_mbr_hyps on FULL streams against the contract (tests/mbr_ref.py) evaluated on what sc_get_hyps_batch returned: the
scores go through the library's exp(), so the comparison is made in two exact halves that leave no near-tie to argue
about - (1) weight_out lies within the bar of tests/test_gpu_mbr.py of the contract's softmax of the totals, and (2) with
THOSE weights handed to the contract, every other output is the contract's bit for bit.  After a lock-step run (the pivot
free and pinned to row 0) and under continuous batching at queue depth 2 (the snapshot path); the hypotheses and their
scores are bit-identical with the calls made and not made; the call interleaves with rescore_hyps and hyps_delta on one
handle in both orders with identical results, with a regrow of the scratch area in between; sc_mbr_lists serves the CTC
n-best of a decoder-free stream, with scores and with weights, and in slabs under a small workspace limit."""
import numpy as np
import pytest

import ctc_beam_ref as R
import mbr_ref as M
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import _abi, ngram, synth
from speechcatcher_amd.native import EngineError
from test_gpu_ctc_beam_streams import CHUNK, KW, _chunks, _hyp_bits

pytestmark = pytest.mark.gpu

S, N, W = 2, 8, 5
BAR = 64 * 2.0 ** -52
AUDIO_SEEDS = [7, 10]
COUNT = {"lists": 0, "moved": 0, "worst": 0.0}


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).tolist()


def _batch(p, **kw):
    return make_batch("mixed", "TINY", "native", S, beam=W, weights=p["w"], **dict(KW, engine=p.get("engine"), **kw))


def _same(got, want, n, what):
    """a stream-level entry against the contract evaluated with the entry's own weights: bit for bit"""
    for key in ("weight", "risk", "conf", "alt_mass", "gap_mass"):
        assert _u64(got[key]) == _u64(want[key]), (what, key, got[key], want[key])
    for key in ("order", "status", "alt_tok"):
        assert got[key].tolist() == want[key].tolist(), (what, key)
    assert (got["pivot"], got["n_in"]) == (int(want["header"][0]), int(want["header"][2])), what
    assert got["dist"].tolist() == want["dist"][:n, :n].tolist(), what


def _check_scored(got, rows, totals, scale, what, **kw):
    n = len(totals)
    soft = M.mbr(rows, score=totals, scale=scale, **kw)
    assert got["status"].tolist() == soft["status"].tolist(), what
    err = np.abs(got["weight"] - soft["weight"]).max() if n else 0.0
    assert err <= BAR, (what, err)
    COUNT["worst"] = max(COUNT["worst"], float(err))
    want = M.mbr(rows, weight=got["weight"], **kw)
    _same(got, want, n, what)
    COUNT["lists"] += 1
    COUNT["moved"] += int(want["header"][0] > 0)
    return want


def _check(p, sb, streams, scale=1.0, pivot_best=False):
    """sc_mbr_hyps of the listed streams against the contract on what sc_get_hyps_batch returns for them"""
    a = sb.hypotheses_arrays(streams)
    got = sb.mbr_hyps(streams, scale=scale, pivot_best=pivot_best)
    again = sb.hypotheses_arrays(streams)
    assert all(a[k].tobytes() == again[k].tobytes() for k in a)     # the call changed nothing
    for i, s in enumerate(streams):
        nh = int(a["n_hyps"][i])
        g = got[int(s)]
        assert len(g["order"]) == nh
        if nh == 0:
            assert g["pivot"] == -1 and len(g["conf"]) == 0
            continue
        want = _check_scored(g, a["ids"][i, :nh], a["score"][i, :nh], scale, (s, scale, pivot_best), lens=a["lens"][i, :nh],
                             L=a["ids"].shape[2], skip=1, strip=p["eos"], V=p["V"], pivot=0 if pivot_best else -1)
        if pivot_best:
            assert g["pivot"] == 0 and len(g["conf"]) == len(want["y"][0])
    return got


@pytest.fixture(scope="module")
def probe():
    p = {"w": packed_weights("mixed", "TINY", "cuda:0"), "S": S, "n": N}
    p["audio"] = [synth.synth_audio(AUDIO_SEEDS[s], CHUNK * N - 1000 * s) for s in range(S)]
    sb = _batch(p)                                                   # a handle on which the calls are never made
    p["engine"] = sb.engine
    p["eos"], p["V"] = sb.cfg.eos_id, sb.cfg.vocab_size
    p["hyps"] = []
    for k in range(N):
        sb.push(_chunks(p, k))
        p["hyps"].append(_hyp_bits(sb, range(S)))
    assert sb.mbr_workspace()[1] == 0                                # ... and which allocated nothing for them
    return p


def _big_lists(rng, n, rows, length, V):
    lists = [[[int(v) for v in y] for y in M.family(rng, rows, length, V)] for _ in range(n)]
    weights = [list(rng.uniform(0.1, 1.0, rows)) for _ in range(n)]
    return lists, weights


def test_full_streams_in_lockstep_and_interleaved_with_the_other_services(probe):
    p = probe
    sb = _batch(p)
    blob = ngram.pack({(t,): (-1.0 - 0.01 * t, 0.0) for t in range(p["V"])}, p["V"])
    dev = sb.language_model(blob)
    rng = np.random.default_rng(3)
    for k in range(N):
        sb.push(_chunks(p, k))
        both = list(range(S))
        first = _check(p, sb, both)
        _check(p, sb, [1], scale=0.5, pivot_best=True)               # one stream of the batch, the pivot pinned
        # interleaved with the other read-back services on the one scratch area, in both orders: identical results
        r0 = sb.rescore_hyps(both, dev, 0.5, 0.3)
        d0 = sb.hyps_delta(both, [0] * S)
        second = sb.mbr_hyps(both)
        if k == N // 2:                                              # a regrow of the area in between
            lists, weights = _big_lists(rng, 3, 16, 150, p["V"])
            big = sb.mbr_lists(lists, weights, weights=True)
            for li, ws, g in zip(lists, weights, big):
                L = max(map(len, li))
                rows = [y + [0] * (L - len(y)) for y in li]
                _same(g, M.mbr(rows, weight=ws, lens=[len(y) for y in li], L=L, V=p["V"]), 16, "regrow")
        d1 = sb.hyps_delta(both, [0] * S)
        third = sb.mbr_hyps(both)
        r1 = sb.rescore_hyps(both, dev, 0.5, 0.3)
        for s in both:
            for key in first[s]:
                assert np.asarray(first[s][key]).tobytes() == np.asarray(second[s][key]).tobytes() \
                    == np.asarray(third[s][key]).tobytes(), (k, s, key)
            assert all(np.asarray(r0[s][key]).tobytes() == np.asarray(r1[s][key]).tobytes() for key in r0[s])
            assert all(np.asarray(d0[s][key]).tobytes() == np.asarray(d1[s][key]).tobytes() for key in d0[s])
        assert _hyp_bits(sb, range(S)) == p["hyps"][k], k            # hypotheses and scores as on the handle that never asks
    # the refusals
    with pytest.raises(EngineError, match="listed twice"):
        sb.mbr_hyps([0, 0])
    with pytest.raises(EngineError, match="scale"):
        sb.mbr_hyps([0], scale=float("nan"))
    with pytest.raises(EngineError, match="scale"):
        sb.mbr_hyps([0], scale=-1.0)
    sid, nh = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert sb.lib.sc_mbr_hyps(sb.handle, sid.ctypes.data_as(_abi.c_int_p), 1, _abi.MBR_MAX_HYPS + 1, 1.0, 0, 16, None, None,
                              None, None, None, None, None, None, None, None, nh.ctypes.data_as(_abi.c_int_p)) == -1   # nbest > 16
    assert sb.lib.sc_mbr_hyps(sb.handle, sid.ctypes.data_as(_abi.c_int_p), 1, W, 1.0, 0, 1, None, None, None, None, None, None,
                              None, None, None, None, nh.ctypes.data_as(_abi.c_int_p)) == -1
    assert b"max_len" in sb.lib.sc_last_error()
    sb.reset(0)                                                      # a stream without hypotheses: an empty list
    _check(p, sb, [0, 1])
    sb.push(_chunks(p, 0, [0]))
    _check(p, sb, [0, 1])
    sb.submit([(0, p["audio"][0][CHUNK:2 * CHUNK], True)])           # a chunk that has not been reported yet
    for streams in ([0], [1, 0]):
        with pytest.raises(EngineError, match="inside a decode block"):
            sb.mbr_hyps(streams)
    while sb.outstanding:
        sb.poll(1)
    _check(p, sb, [0, 1])
    dev.close()
    print(f"\nsc_mbr_hyps: the minimum-risk row is not the search's best in {COUNT['moved']} of {COUNT['lists']} lists "
          f"(beam {W}; scale is a parameter, not tuned); largest weight error {COUNT['worst']:.3e} (bar {BAR:.3e})")


def test_continuous_batching_at_queue_depth_2_reads_the_snapshot(probe):
    p = probe
    sb = _batch(p)
    sb.set_queue_depth(2)
    nxt, rep, queued_behind = [0] * S, [0] * S, 0

    def feed(s):
        k = nxt[s]
        nxt[s] += 1
        return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == N - 1)

    sb.submit([feed(s) for s in range(S)])
    sb.submit([feed(s) for s in range(S)])
    while sb.outstanding:
        done = sb.poll(1)
        for s in sorted(done):
            queued_behind += nxt[s] > rep[s] + 1
            _check(p, sb, [s], pivot_best=bool(rep[s] % 2))
            assert _hyp_bits(sb, [s])[s] == p["hyps"][rep[s]][s], (s, rep[s])
            rep[s] += 1
        again = [feed(s) for s in sorted(done) if nxt[s] < N]
        if again:
            sb.submit(again)
    assert rep == [N] * S and queued_behind >= S


def test_lists_of_a_decoder_free_stream_and_slabs_under_a_small_workspace_limit(probe):
    p = probe
    sb = _batch(p)
    for s in range(S):
        sb.set_decoder(s, "ctc")
    sb.set_ctc_beam(8, 8)
    for k in range(N):
        sb.push(_chunks(p, k))
    hyps = sb.ctc_beam_hyps(list(range(S)), 8)
    lists = [[h["ids"] for h in hyps[s]] for s in range(S)]
    totals = [[R.lae(h["pb"], h["pnb"]) for h in hyps[s]] for s in range(S)]
    assert all(len(li) == 8 and max(map(len, li)) > 3 for li in lists)
    got = sb.mbr_lists(lists, totals, scale=0.7)
    pinned = sb.mbr_lists(lists, totals, scale=0.7, pivots=[0, 3])
    for s in range(S):
        L = max(map(len, lists[s]))
        rows = [list(y) + [0] * (L - len(y)) for y in lists[s]]
        kw = dict(lens=[len(y) for y in lists[s]], L=L, V=p["V"])
        _check_scored(got[s], rows, totals[s], 0.7, ("ctc n-best", s), **kw)
        _check_scored(pinned[s], rows, totals[s], 0.7, ("ctc n-best, pivot", s), pivot=[0, 3][s], **kw)
        assert pinned[s]["pivot"] == [0, 3][s]
    # lists of other shapes: an empty list, an empty row, a bad token, weights
    odd = sb.mbr_lists([[], [[], [3, 4]], [[1, 2], [p["V"]], [1, 3]]], [[], [0.25, 0.75], [0.5, 0.2, 0.3]], weights=True)
    assert odd[0]["pivot"] == -1 and len(odd[0]["order"]) == 0
    _same(odd[1], M.mbr([[0, 0], [3, 4]], weight=[0.25, 0.75], lens=[0, 2], L=2, V=p["V"]), 2, "an empty row")
    _same(odd[2], M.mbr([[1, 2], [p["V"], 0], [1, 3]], weight=[0.5, 0.2, 0.3], lens=[2, 1, 2], L=2, V=p["V"]), 3, "a bad token")
    assert odd[2]["status"].tolist() == [0, M.BAD_TOKEN, 0]
    with pytest.raises(EngineError, match="pivot"):
        sb.mbr_lists([[[1]]], [[0.0]], pivots=[1])
    with pytest.raises(ValueError, match="more than 16"):
        sb.mbr_lists([[[1]] * 17], [[0.0] * 17])
    # slabs: six lists of 600 labels need about 11 MiB of direction bits, the limit allows 8
    rng = np.random.default_rng(9)
    lists, weights = _big_lists(rng, 6, 3, 600, p["V"])
    free = sb.mbr_lists(lists, weights, weights=True)
    assert sb.mbr_workspace()[1] > 8 << 20
    with pytest.raises(_abi.ScasrError):
        sb.set_mbr_workspace(1 << 20)
    sb.set_mbr_workspace(8 << 20)
    slabbed = sb.mbr_lists(lists, weights, weights=True)
    assert 0 < sb.mbr_workspace()[1] <= 8 << 20
    for li, ws, a, b in zip(lists, weights, free, slabbed):
        L = max(map(len, li))
        rows = [y + [0] * (L - len(y)) for y in li]
        want = M.mbr(rows, weight=ws, lens=[len(y) for y in li], L=L, V=p["V"])
        _same(a, want, 3, "one slab")
        _same(b, want, 3, "slabs")
