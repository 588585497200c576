"""CTC token alternates on the GPU (csrc/alternates.hip: sc_ctc_alternates; csrc/stream_readback.hip: sc_alternates_hyps) against
the float64 contract of tests/ctc_alt_ref.py: the kernel on constructed tables - every int32 (alt_ids, own_rank, status)
equal with no case excluded, alt_logp within 1e-11 on the tables with |x| <= 50 -, the stream level on the tiny and the XL
synthetic model (lock-step and served at queue depth 2), the scheduler / ServerLoop / CLI round trips.

The bar on alt_logp: the float64 sum of exp over a row in another order than v ascending is bounded by 2 V 2^-53 = 1.8e-12
at V = 8192 (relative, on a sum >= 1: the same bound on its log); 1e-11 is a few times that, for the device's exp / log
against numpy's.

Measured on an MI355X (printed by the tests): kernel against the contract, largest |alt_logp - contract|
7.1e-15 (V = 8192 and the 300-job launch; 3.6e-15 at V = 1024); stream level 159 (tiny) / 339 (XL) token spans equal to the
contract on the table read back."""
import functools
import json

import numpy as np
import pytest
import torch

import ctc_alt_ref as R
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import _abi, synth

pytestmark = pytest.mark.gpu

LOGP_BAR = 1e-11
INT_MAX = 2 ** 31 - 1
NINF = -np.inf
WORST = {"logp": 0.0}


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


def _strided(x, pad=3):
    """the table on the device as a view with a row stride of V + pad floats (NaN between the rows: never read)"""
    T, V = x.shape
    buf = torch.full((T, V + pad), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :V] = torch.from_numpy(x).to("cuda:0")
    return buf[:, :V]


def _check(be, jobs, K, name, logp=True, max_L=None):
    """jobs: (x [T, V] numpy fp32, blank, labels, start, end) -> ONE launch; every int32 equal to the contract's, -inf where
    the contract has -inf, alt_logp within LOGP_BAR elsewhere (``logp``: the tables hold |x| <= 50 or -inf), and nothing
    written at or past a job's L.  Returns the raw outputs."""
    tabs = {}
    dev_jobs = []
    for x, blank, y, a, e in jobs:
        if id(x) not in tabs:
            tabs[id(x)] = _strided(x)
        dev_jobs.append((tabs[id(x)], blank, y, a, e))
    got = be.ctc_alternates(dev_jobs, K, max_L=max_L)
    ids, lp, rank, st = got
    worst = 0.0
    for k, (x, blank, y, a, e) in enumerate(jobs):
        L = len(y)
        w_ids, w_lp, w_rank, w_st = R.alternates(x, blank, y, a, e, K)
        np.testing.assert_array_equal(st[k, :L], w_st, err_msg=f"{name} job {k}: status")
        np.testing.assert_array_equal(ids[k, :L], w_ids, err_msg=f"{name} job {k}: alt_ids")
        np.testing.assert_array_equal(rank[k, :L], w_rank, err_msg=f"{name} job {k}: own_rank")
        assert ((lp[k, :L] == NINF) == (w_lp == NINF)).all(), f"{name} job {k}: -inf slots"
        assert not np.isnan(lp[k, :L]).any()
        fin = np.isfinite(w_lp)
        if logp and fin.any():
            worst = max(worst, float(np.abs(lp[k, :L][fin] - w_lp[fin]).max()))
        assert (ids[k, L:] == -7).all() and (lp[k, L:] == -7.0).all(), f"{name} job {k}: written past L"
        assert (rank[k, L:] == -7).all() and (st[k, L:] == -7).all(), f"{name} job {k}: written past L"
    WORST["logp"] = max(WORST["logp"], worst)
    print(f"\n{name}: largest |alt_logp - contract| {worst:.3e} (so far {WORST['logp']:.3e}, bar {LOGP_BAR:.0e})")
    assert worst <= LOGP_BAR, (name, worst)
    return got


def _spans(rng, T, lengths):
    """non-overlapping spans of the given lengths where they fit, plus a few that overlap (the kernel does not care)"""
    start, end, t = [], [], 0
    for n in lengths:
        if t + n > T:
            t = int(rng.integers(0, T - n + 1))
        start.append(t)
        end.append(t + n)
        t += n
    return start, end


@functools.lru_cache(maxsize=None)
def _random_table(V, T=320, seed=0):
    rng = np.random.default_rng(1000 + V + seed)
    return np.clip(rng.standard_normal((T, V)) * 6.0, -50, 50).astype(np.float32)


@pytest.mark.parametrize("V", [2, 5, 64, 255, 256, 257, 1024, 2049, 8192])
def test_kernel_equals_the_contract_at_every_vocabulary(be, V):
    """span lengths 1, 2, 3, 64, 300 in a table of 320 rows, stride > V with NaN between the rows, the blank first, last
    and in the middle, K = 1 and 8 (above V - 1 for V = 2 and 5), labels all over the vocabulary"""
    rng = np.random.default_rng(V)
    x = _random_table(V)
    T = x.shape[0]
    lengths = [300, 1, 2, 3, 64, 1, 2, 3, 1]
    start, end = _spans(rng, T, lengths)
    for blank in sorted({0, V - 1, V // 2}):
        y = rng.integers(0, V, len(lengths)).tolist()
        y[1] = int(np.argmax(x[start[1]]))                       # the frame's best entry (rank 0 unless it is the blank)
        for K in (1, 8):
            ids, lp, rank, st = _check(be, [(x, blank, y, start, end)], K, f"V {V} blank {blank} K {K}")
            assert (st[0, :len(y)] == R.OK).all()
            if K > V - 1:
                assert (ids[0, :len(y), V - 1:] == -1).all() and (lp[0, :len(y), V - 1:] == NINF).all()
            for k in range(len(y)):
                if 0 <= rank[0, k] < K:
                    assert ids[0, k, rank[0, k]] == y[k]


@pytest.mark.parametrize("V", [5, 300, 2049])
def test_exact_ties(be, V):
    """tables drawn from multiples of 0.25 (sums collide all the time) and duplicated columns: the lower id is ahead"""
    rng = np.random.default_rng(50 + V)
    x = (rng.integers(-8, 9, size=(40, V)) * 0.25).astype(np.float32)
    x[:, V - 1] = x[:, 1]
    x[:, V // 2] = x[:, 1]
    start, end = _spans(rng, 40, [7, 2, 3, 1, 20, 4])
    start[1] = start[2] = start[0]                               # the three copies of one column over the same span
    end[1] = end[2] = end[0]
    y = [1, V // 2, V - 1, 2, 1, 3]
    for blank in (0, 1):
        ids, _, rank, _ = _check(be, [(x, blank, y, start, end)], 8, f"ties V {V} blank {blank}")
    S = R.span_sums(x, start[4], end[4])
    assert len(np.unique(S)) < V or V == 5                       # (there are ties to break)
    ids, _, rank, _ = _check(be, [(x, 0, y, start, end)], 8, f"ties V {V}")
    assert 0 <= rank[0, 0] < rank[0, 1] < rank[0, 2]             # equal sums: the copies stand in the order of their ids


def test_minus_inf_columns(be):
    rng = np.random.default_rng(60)
    V = 70
    x = np.clip(rng.standard_normal((30, V)) * 5, -50, 50).astype(np.float32)
    x[:, 3] = NINF
    x[5:9, 10] = NINF                                           # -inf in some rows of a span: the sum is -inf
    start, end = [0, 4, 5, 20], [4, 10, 9, 30]
    _check(be, [(x, 0, [3, 10, 10, 3], start, end)], 8, "-inf columns")
    only = np.full((6, V), NINF, np.float32)                     # all candidates but one -inf (the blank is finite too)
    only[:, 0] = 0.5
    only[:, 7] = -1.0
    ids, lp, rank, st = _check(be, [(only, 0, [7, 9, 1], [0, 2, 0], [6, 3, 1])], 4, "one finite candidate")
    assert ids[0, 0].tolist() == [7, 1, 2, 3] and rank[0, :3].tolist() == [0, 8, 1]
    assert np.isfinite(lp[0, :3, 0]).all() and (lp[0, :3, 1:] == NINF).all()


def test_bad_rows_inside_and_outside_spans_and_bad_spans(be):
    """the three kinds of bad row; spans that are negative, empty, reversed, past T or INT_MAX come back NO_SPAN with the
    sentinel outputs, and NO_SPAN wins over a bad row"""
    rng = np.random.default_rng(61)
    V, T = 300, 40
    x = np.clip(rng.standard_normal((T, V)) * 5, -50, 50).astype(np.float32)
    x[10, 17] = np.nan
    x[20, 299] = np.inf
    x[30] = NINF
    start = [0, 9, 10, 11, 15, 20, 21, 25, 30, 31, 0, -1, -INT_MAX - 1, 5, 8, 0, 39, INT_MAX, INT_MAX - 1, 12, 35, 0]
    end = [10, 11, 11, 20, 21, 21, 30, 31, 31, 40, 40, 5, 3, 5, 4, T + 1, INT_MAX, INT_MAX, INT_MAX, 13, 40, 1]
    y = rng.integers(1, V, len(start)).tolist()
    ids, lp, rank, st = _check(be, [(x, 0, y, start, end)], 3, "bad rows and spans")
    want = [0, 2, 2, 0, 2, 2, 0, 2, 2, 0, 2, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    assert st[0, :len(start)].tolist() == want
    for k, s in enumerate(want):
        if s:
            assert ids[0, k].tolist() == [-1] * 3 and (lp[0, k] == NINF).all() and rank[0, k] == -1
    # a table of nothing but bad rows outside the one span that is asked for
    poisoned = np.full_like(x, np.nan)
    poisoned[12:15] = x[12:15]
    _, _, _, st = _check(be, [(poisoned, 0, [4], [12], [15])], 3, "poison outside the span")
    assert st[0, 0] == R.OK


def test_labels_out_of_range_or_blank(be):
    rng = np.random.default_rng(62)
    V = 257
    x = np.clip(rng.standard_normal((12, V)) * 5, -50, 50).astype(np.float32)
    y = [-1, V, INT_MAX, -INT_MAX - 1, 128, 0, 256, 100]
    n = len(y)
    ids, _, rank, st = _check(be, [(x, 128, y, [0] * n, [12] * n)], 8, "labels")
    assert st[0, :n].tolist() == [0] * n and rank[0, :5].tolist() == [-1] * 5 and (rank[0, 5:n] >= 0).all()
    assert all(ids[0, k].tolist() == ids[0, 0].tolist() for k in range(n))


def test_the_cancellation_case_pins_the_frame_order(be):
    x = np.full((3, 4), -1.0, np.float32)
    x[:, 1] = [1e30, 1e-3, -1e30]
    x[:, 2] = [0.0, 5e-4, 0.0]
    big = np.full((3, 2049), -1.0, np.float32)                   # ... and in the 32-sums-per-thread instantiation
    big[:, 2048] = [1e30, 1e-3, -1e30]
    big[:, 7] = [0.0, 5e-4, 0.0]
    ids, _, rank, _ = _check(be, [(x, 0, [1, 1], [0, 1], [3, 3]), (big, 0, [2048, 7], [0, 0], [3, 3])], 3,
                             "cancellation", logp=False)
    assert ids[0, 0].tolist() == [2, 1, 3] and ids[0, 1].tolist() == [2, 3, 1] and rank[0, :2].tolist() == [1, 2]
    assert ids[1, 0, :2].tolist() == [7, 2048] and rank[1, :2].tolist() == [1, 0]


def test_300_jobs_of_mixed_length_and_one_job(be):
    """300 jobs with L from 0 to 9 over three tables in ONE launch: nothing at or past a job's L is written (_check)"""
    rng = np.random.default_rng(63)
    tables = [(_random_table(64, 50, 1), 0), (_random_table(257, 50, 2), 256), (_random_table(1024, 50, 3), 5)]
    jobs = []
    for i in range(300):
        x, blank = tables[i % 3]
        L = int(rng.integers(0, 10)) if i not in (0, 7, 299) else 0
        a = rng.integers(0, 47, L)
        jobs.append((x, blank, rng.integers(0, x.shape[1], L).tolist(), a.tolist(), (a + rng.integers(1, 4, L)).tolist()))
    assert max(len(j[2]) for j in jobs) >= 5 and min(len(j[2]) for j in jobs) == 0
    _check(be, jobs, 5, "300 jobs")
    _check(be, jobs[1:2], 8, "1 job")
    _check(be, [jobs[0]], 8, "1 job, L = 0")
    # max_L above every L: the extra workgroups leave at once
    _check(be, jobs[:20], 2, "max_L 64", max_L=64)


def test_two_runs_give_the_same_bits(be):
    x = _random_table(2049)
    rng = np.random.default_rng(64)
    start, end = _spans(rng, 320, [300, 5, 2, 1])
    jobs = [(_strided(x), 9, rng.integers(0, 2049, 4).tolist(), start, end)]
    a = be.ctc_alternates(jobs, 8)
    b = be.ctc_alternates(jobs, 8)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_malformed_jobs_write_nothing_and_bad_arguments_are_refused(be):
    rng = np.random.default_rng(65)
    V = 65
    x = _random_table(V, 20, 4)
    tab = _strided(x)
    job = (tab, 0, [3, 4], [0, 5], [5, 9])

    def setter(**kw):
        def tweak(k, j):
            if k == 1:
                for f, v in kw.items():
                    setattr(j, f, v)
        return tweak

    want = R.alternates(x, 0, *job[2:], 3)
    for kw in (dict(emis=None), dict(labels=None), dict(start=None), dict(end=None), dict(alt_ids=None), dict(alt_logp=None),
               dict(own_rank=None), dict(status=None), dict(V=0), dict(V=_abi.MAX_VOCAB + 1), dict(blank=-1), dict(blank=V),
               dict(T=-1), dict(L=3), dict(stride=V - 1)):
        ids, lp, rank, st = be.ctc_alternates([job] * 3, 3, tweak=setter(**kw))
        assert (ids[1] == -7).all() and (lp[1] == -7.0).all() and (rank[1] == -7).all() and (st[1] == -7).all(), kw
        for k in (0, 2):                                         # its neighbours in the same launch are served
            np.testing.assert_array_equal(ids[k, :2], want[0])
            np.testing.assert_array_equal(st[k, :2], want[3])
    lib = _abi.load()
    assert lib.sc_ctc_alternates(None, 0, 4, 3, None) == 0
    assert lib.sc_ctc_alternates(None, 2, 4, 3, None) == -1 and lib.sc_ctc_alternates(None, -1, 4, 3, None) == -1
    p = tab.data_ptr()
    assert lib.sc_ctc_alternates(p, _abi.ALT_MAX_JOBS + 1, 4, 3, None) == -1
    assert lib.sc_ctc_alternates(p, 1, _abi.ALIGN_MAX_L + 1, 3, None) == -1
    assert lib.sc_ctc_alternates(p, 1, 4, 0, None) == -1 and lib.sc_ctc_alternates(p, 1, 4, _abi.ALT_MAX_K + 1, None) == -1
    assert lib.sc_ctc_alternates(p, 1, -1, 3, None) == -1


# ---- stream level ----------------------------------------------------------------------------------------------------
CHUNK = 10240
SHAPE = {"TINY": (2, 6), "XL": (4, 5)}      # streams, chunks
KW = dict(max_frames=160, max_tokens=200, pcm_capacity=1 << 17)
ALIGN_KEYS = ("start", "end", "logp_mean", "path_score", "status", "n_hyps")
K_STREAM = 4


@functools.lru_cache(maxsize=None)
def _weights(name):
    return packed_weights("mixed", name, "cuda:0")


def _audio(name):
    S, n = SHAPE[name]
    return [synth.synth_audio(70 + s, CHUNK * n - 1000 * s) for s in range(S)]


def _against_contract(sb, streams, name):
    """at a final, before the reset: alternates() carries align()'s arrays bit for bit; ids, ranks and statuses equal the
    contract run on the table read back over the spans; a token among its own K best stands at its rank.  Returns the
    number of spans compared."""
    nb = sb.W
    al = sb.align(streams, nb)
    alt = sb.alternates(streams, nb, K_STREAM)
    for key in ALIGN_KEYS:
        assert al[key].tobytes() == alt[key].tobytes(), (name, key)
    hy = sb.hypotheses_arrays(streams)
    n_ok = 0
    for i, s in enumerate(streams):
        table = sb.read_ctc(s)
        assert int(alt["n_hyps"][i]) == int(hy["n_hyps"][i])
        for h in range(int(alt["n_hyps"][i])):
            y = hy["ids"][i, h, 1:int(hy["lens"][i, h])].tolist()
            if y and y[-1] == sb.cfg.eos_id:
                y = y[:-1]
            L = len(y)
            a, e = alt["start"][i, h, :L], alt["end"][i, h, :L]
            w_ids, w_lp, w_rank, w_st = R.alternates(table, sb.cfg.blank_id, y, a, e, K_STREAM)
            np.testing.assert_array_equal(alt["span_status"][i, h, :L], w_st, err_msg=f"{name} stream {s} hyp {h}")
            np.testing.assert_array_equal(alt["alt_ids"][i, h, :L], w_ids, err_msg=f"{name} stream {s} hyp {h}")
            np.testing.assert_array_equal(alt["own_rank"][i, h, :L], w_rank, err_msg=f"{name} stream {s} hyp {h}")
            if int(alt["status"][i, h]) != _abi.ALIGN_OK:          # a failed alignment: NO_SPAN for every token
                assert (alt["span_status"][i, h, :L] == _abi.ALT_NO_SPAN).all()
                assert (alt["alt_ids"][i, h, :L] == -1).all() and (alt["own_rank"][i, h, :L] == -1).all()
                continue
            assert (w_st == R.OK).all()
            fin = np.isfinite(w_lp)
            assert np.abs(alt["alt_logp"][i, h, :L][fin] - w_lp[fin]).max() <= LOGP_BAR
            for k in range(L):
                r = int(alt["own_rank"][i, h, k])
                assert r >= 0
                if r < K_STREAM:
                    assert int(alt["alt_ids"][i, h, k, r]) == y[k]
                    # the token's own slot and the alignment's confidence are the same quantity (float64 / fp32)
                    assert abs(alt["alt_logp"][i, h, k, r] - float(alt["logp_mean"][i, h, k])) <= 1e-3
            n_ok += L
    return n_ok


@pytest.mark.parametrize("name", ["TINY", "XL"])
def test_lockstep_final_equals_align_and_the_contract(name):
    S, n = SHAPE[name]
    sb = make_batch("mixed", name, "native", S, weights=_weights(name), **KW)
    audio = _audio(name)
    for k in range(n):
        sb.push([(s, audio[s][k * CHUNK:(k + 1) * CHUNK], k == n - 1) for s in range(S)])
    n_ok = _against_contract(sb, list(range(S)), name)
    print(f"\n{name}: {n_ok} token spans equal the contract on the table read back")
    assert n_ok >= 4 * S
    with pytest.raises(ValueError):
        sb.alternates([0], 1, 0)
    with pytest.raises(ValueError):
        sb.alternates([0], 1, _abi.ALT_MAX_K + 1)
    # the alignment itself is what it was: align() after alternates() gives the same bits again
    a, b = sb.align([0], 2), sb.alternates([0], 2, 1)
    assert all(a[key].tobytes() == b[key].tobytes() for key in ALIGN_KEYS)


@pytest.mark.parametrize("name", ["TINY", "XL"])
def test_served_at_queue_depth_2_equals_the_contract_and_changes_no_hypothesis(name):
    """continuous batching, queue depth 2: a run that asks for alternates at every final (checked against align() and
    the contract there) reports the hypotheses and scores of the run that does not, bit for bit"""
    S, n = SHAPE[name]
    audio = _audio(name)

    def run(on):
        sb = make_batch("mixed", name, "native", S, weights=_weights(name), **KW)
        sb.set_queue_depth(2)
        nxt, rep, replies, n_ok = [0] * S, [0] * S, {}, 0

        def feed(s):
            k = nxt[s]
            nxt[s] += 1
            return (s, audio[s][k * CHUNK:(k + 1) * CHUNK], k == n - 1)

        sb.submit([feed(s) for s in range(S)])
        sb.submit([feed(s) for s in range(S)])
        while sb.outstanding:
            ids = sorted(sb.poll(1))
            a = sb.hypotheses_arrays(ids)
            for i, s in enumerate(ids):
                replies.setdefault(s, []).append((a["ids"][i].tobytes(), a["xpos"][i].tobytes(), a["lens"][i].tobytes(),
                                                  a["score"][i].tobytes(), a["score_dec"][i].tobytes(),
                                                  a["score_ctc"][i].tobytes()))
                rep[s] += 1
            finals = [s for s in ids if rep[s] == n]
            if on and finals:
                n_ok += _against_contract(sb, finals, f"{name} served")
            for s in finals:
                sb.reset(s)
            again = [feed(s) for s in ids if nxt[s] < n]
            if again:
                sb.submit(again)
        assert rep == [n] * S
        return replies, n_ok

    plain, _ = run(False)
    asked, n_ok = run(True)
    assert n_ok >= 4 * S
    assert plain == asked


def _serve(config=None, **kw):
    from test_engine_spec import make_batch as plain_batch
    from speechcatcher_amd.config import TINY
    from speechcatcher_amd.scheduler import StreamScheduler
    from speechcatcher_amd.server_session import ServerLoop
    tokens = [("▁" if v % 3 == 0 else "") + f"t{v}" for v in range(TINY.vocab_size)]
    chunks = [(synth.synth_audio(40 + k, 10240) * 32767).astype(np.int16) for k in range(9)]
    sb = plain_batch("TINY", 1234, "meanstd", 3, True, n_streams=1, backend="native", max_frames=400, max_tokens=300,
                     pcm_capacity=1 << 18)
    loop = ServerLoop(StreamScheduler(sb, tokens, result_format="espnet"), vosk_output_format=True,
                      finalize_update_iters=2, max_partial_iters=5, **kw)
    sid = loop.connect()
    if config is not None:
        loop.submit(sid, json.dumps({"config": config}))
    for c in chunks:
        loop.submit(sid, c)
    loop.submit(sid, '{"eof" : 1}')
    reps = []
    while loop.pending():
        for _sid, r in loop.step().items():
            reps.extend(r)
    return reps[1:] if config is not None else reps


def test_server_round_trip_alternatives_for_3_and_the_old_message_for_0():
    old = _serve(vosk_alignment=True)
    assert _serve(dict(max_alternatives=0), vosk_alignment=True, vosk_alternatives=3) == old
    assert _serve(vosk_alignment=True, vosk_alternatives=3) == old
    new = _serve(dict(max_alternatives=3), vosk_alignment=True, vosk_alternatives=3)
    assert len(new) == len(old)
    n_final = 0
    for o, m in zip(old, new):
        if not (isinstance(o, dict) and "result" in o):
            assert o == m
            continue
        n_final += 1
        assert set(m) == {"alternatives"} and 1 <= len(m["alternatives"]) <= 3
        alts = m["alternatives"]
        conf = [a["confidence"] for a in alts]
        assert abs(sum(conf) - 1.0) <= 1e-12 and conf == sorted(conf, reverse=True) and all(0 < c <= 1 for c in conf)
        assert alts[0]["text"] == o["text"] and alts[0]["result"] == o["result"]
        for a in alts:
            assert set(a) == {"text", "confidence", "result"}
            for w in a["result"]:
                assert set(w) == {"conf", "start", "end", "word"} and 0 <= w["start"] < w["end"]
    assert n_final > 0
    # token alternates ride on the entries of the classic result and of the first alternative
    tok = _serve(dict(max_alternatives=2), vosk_alignment=True, vosk_alternatives=2, token_alternates=3)
    cls = _serve(vosk_alignment=True, token_alternates=3)
    n_rec = 0
    for o, m, c in zip(old, tok, cls):
        if not (isinstance(o, dict) and "result" in o):
            assert o == m == c
            continue
        first = m["alternatives"][0]["result"]
        assert first == c["result"] and c["text"] == o["text"]
        assert [{k: v for k, v in w.items() if k != "tokens"} for w in first] == o["result"]
        for w in first:
            assert "".join(r["token"] for r in w["tokens"]).replace("▁", "") == w["word"].replace(" ", "")
            for r in w["tokens"]:
                assert set(r) == {"id", "token", "conf", "own_rank", "alternates"}
                if r["own_rank"] is None:
                    continue
                n_rec += 1
                assert len(r["alternates"]) == 3 and all(0 <= a["conf"] <= 1 for a in r["alternates"])
                assert [a["conf"] for a in r["alternates"]] == sorted((a["conf"] for a in r["alternates"]), reverse=True)
                if r["own_rank"] < 3:
                    assert r["alternates"][r["own_rank"]]["id"] == r["id"]
                    assert abs(r["alternates"][r["own_rank"]]["conf"] - r["conf"]) <= 1e-3
        assert not any("tokens" in w for a in m["alternatives"][1:] for w in a["result"])
    assert n_rec > 0


def test_scheduler_round_trip_carries_the_records():
    from test_engine_spec import make_batch as plain_batch
    from speechcatcher_amd.scheduler import StreamScheduler
    sb = plain_batch("TINY", 1234, "meanstd", 3, True, n_streams=1, backend="native", max_frames=400, max_tokens=300,
                     pcm_capacity=1 << 18)
    sch = StreamScheduler(sb, None, result_format="espnet", align_final=True, alternates=2)
    sid = sch.open()
    audio = synth.synth_audio(41, 3 * CHUNK)
    for k in range(3):
        sch.feed(sid, audio[k * CHUNK:(k + 1) * CHUNK], is_final=k == 2, finalize_all=k == 2)
    res = sch.drain()[sid]
    al = res.alignment
    assert res and al is not None and len(al["alternates"]) == len(al["token_ids"]) == len(res[0][2]) > 0
    assert [r["id"] for r in al["alternates"]] == al["token_ids"]
    assert [r["conf"] for r in al["alternates"]] == al["conf"]
    assert any(r["own_rank"] is not None and len(r["alternates"]) == 2 for r in al["alternates"])


def test_cli_round_trip_writes_token_alternates(tmp_path):
    """recognize_file with --token-alternates 3: token_alternates of the length of tokens next to the alignment's keys;
    without the flag the .json is what it was"""
    from test_gpu_ctc_align import _tiny_s2t, _write_wav
    from speechcatcher_amd.__main__ import make_parser, recognize_file
    s2t = _tiny_s2t(tmp_path)
    wav = tmp_path / "a.wav"
    _write_wav(wav, synth.synth_audio(21, 16000 * 5 + 1234))
    args = make_parser().parse_args(["--token-alternates", "3", str(wav)])
    assert args.token_alternates == 3
    recognize_file(s2t, str(wav), output_file=str(tmp_path / "with"), token_alignment=args.token_alignment,
                   token_alternates=args.token_alternates)
    recognize_file(s2t, str(wav), output_file=str(tmp_path / "without"))
    plain = (tmp_path / "without.json").read_text()
    withal = json.loads((tmp_path / "with.json").read_text())
    n_rec = 0
    for par in withal["paragraphs"]:
        n = len(par["tokens"])
        assert len(par["token_alternates"]) == len(par["token_conf"]) == len(par["token_start"]) == n
        for tok, conf, r in zip(par["tokens"], par["token_conf"], par["token_alternates"]):
            assert r["token"] == tok and r["conf"] == conf
            if r["own_rank"] is not None:
                n_rec += 1
                assert len(r["alternates"]) == 3
        for key in ("token_start", "token_end", "token_conf", "token_alternates"):
            del par[key]
    assert n_rec > 0
    assert json.loads(plain) == withal and "token_alternates" not in plain
