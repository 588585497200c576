"""Stable partials on the GPU (csrc/commit.hip: sc_hyp_commit; csrc/stream_readback.hip: sc_get_hyps_delta) against the float64
contract of tests/hyp_commit_ref.py: the kernel on constructed beams - every int32 equal, stability within 1e-12, the two
exact properties on the device output itself -, the stream level on the tiny and the XL synthetic model (lock-step,
continuous batching at queue depth 2), the call's effect on decoding (none) and its refusals.

The non-vacuity condition of the tiny runs without block-boundary detection is the one seen on the CPU spec engine: at
least three replies of a stream with 1 < commit < L, growing.  The XL run has 6 chunks, of which the first three replies
hold the <sos> alone on the spec engine and the last is final: two replies with 1 < commit < L, growing, are asked of it
(the deviation is recorded in DESIGN.md 8i; over 8 chunks the spec engine gives four such replies at XL dims)."""
import functools

import numpy as np
import pytest
import torch

import hyp_commit_ref as R
from commit_helpers import CHUNK, N_CHUNKS, RUNS, SEEDS, STAB_TOL, Follower, audio, beam, exact_properties, make_batch, \
    non_vacuous, same_delta
from draft_helpers import packed_weights
from speechcatcher_amd import _abi

pytestmark = pytest.mark.gpu

STRIDE = 300
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 300]
N_HYPS = [1, 2, 3, 10, 16]
WORST = {"stab": 0.0}


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


def _mismatches(L):
    """where the rival hypotheses first differ: one place for all of them, or a mix"""
    return [[0], [63], [64], [L - 1], [None], [64, None, 63, L - 1, 0, 200]]


def _guards_untouched(raw, t, n):
    assert (raw["header"][4:] == -7).all() and (raw["agree"][n:] == -7).all() and (raw["totals"][3:] == -7.0).all()
    assert (raw["ids"][t:] == -7).all() and (raw["pos"][t:] == -7).all() and (raw["stability"][t:] == -7.0).all()


# ---- the kernel against the contract ----------------------------------------------------------------------------------
def test_kernel_equals_the_contract_on_mixed_jobs_of_one_launch(be):
    rng = np.random.default_rng(0)
    bases = [(L, n, m) for L in LENGTHS for n in N_HYPS for m in _mismatches(L)]
    nb = len(bases)
    # every row of every beam is STRIDE long and 16 rows are there: garbage, different in every row, behind L and n
    ybuf = rng.integers(-5, 1 << 20, size=(nb, 16, STRIDE), dtype=np.int32)
    xbuf = rng.integers(-5, 1 << 20, size=(nb, 16, STRIDE), dtype=np.int32)
    sbuf = rng.standard_normal((nb, 16, 3)) * 50.0
    beams = []
    for b, (L, n, m) in enumerate(bases):
        y, x = beam(rng, n, L, m)
        ybuf[b, :n, :L], xbuf[b, :n, :L] = y, x
        s = -np.sort(rng.random(n) * float(rng.choice([0.5, 6.0, 40.0, 900.0])))
        if b % 7 == 3 and n > 1:                                     # a non-finite score: +inf, -inf, a NaN in turn
            s[int(rng.integers(n))] = [np.inf, -np.inf, np.nan][(b // 7) % 3]
        if b % 41 == 5:
            s[:] = -np.inf                                           # nothing finite: the mass is shared evenly
        sbuf[b, :n, 0] = s
        beams.append((y, x, s))
    yd, xd = torch.from_numpy(ybuf).to("cuda:0"), torch.from_numpy(xbuf).to("cuda:0")
    s3 = torch.from_numpy(sbuf).to("cuda:0")                         # {total, dec, ctc} triples: stride 3
    s1 = [s3[:, :, c].contiguous() for c in range(3)]                # three arrays: stride 1
    jobs, want, meta = [], [], []
    for b, (L, n, m) in enumerate(bases):
        y, x, s = beams[b]
        commit = R.hyp_commit(y, x, s)["commit"]
        for frm in sorted({0, commit, L}):
            for triples in (False, True):
                for final in (False, True):
                    sc = s3[b, :n] if triples else tuple(a[b, :n] for a in s1)
                    jobs.append((yd[b, :n], xd[b, :n], sc, L, frm, final))
                    want.append(R.hyp_commit(y, x, s, frm, final, sbuf[b, :n, 1], sbuf[b, :n, 2]))
                    meta.append((L, n, m, frm, triples, final))
    assert len(jobs) > 2000
    got = be.hyp_commit(jobs)                                        # ONE launch
    n_mid = n_flag = 0
    for g, w, (L, n, m, frm, triples, final) in zip(got, want, meta):
        assert g["raw"]["header"][:4].tolist() == [w["L"], w["commit"], n, w["status"]], (L, n, m, frm, triples, final)
        err = same_delta(g, w, STAB_TOL)                             # every int32 equal, totals the same bits
        WORST["stab"] = max(WORST["stab"], err)
        exact_properties(g, frm)                                     # ... on the device output itself
        _guards_untouched(g["raw"], L - frm, n)
        n_mid += 0 < w["commit"] < L and not final
        n_flag += w["status"] == R.NONFINITE
    print(f"\n{len(jobs)} jobs: largest |stability - contract| = {WORST['stab']:.3e} (bar {STAB_TOL:.0e})")
    assert n_mid > 300 and n_flag > 100


def test_scores_far_apart_and_equal_scores(be):
    rng = np.random.default_rng(1)
    y, x = beam(rng, 16, 130, [100, 5, None, 64, 129, 63])
    cases = [np.zeros(16), -np.arange(16.0) * 1e-9, -np.arange(16.0) * 50.0, -np.arange(16.0) ** 3,
             np.full(16, -1e300), np.full(16, 1e308) - np.arange(16.0) * 1e293, -745.0 - np.arange(16.0),
             np.where(np.arange(16) % 2 == 0, -1.0, -np.inf), np.where(np.arange(16) == 0, np.nan, -2.0)]
    yd, xd = torch.from_numpy(y).to("cuda:0"), torch.from_numpy(x).to("cuda:0")
    jobs, want = [], []
    for s in cases:
        sd = torch.from_numpy(np.stack([s, s - 1.0, s + 1.0], 1).copy()).to("cuda:0")
        for frm in (0, 5, 64):
            jobs.append((yd, xd, sd, 130, frm, False))
            want.append(R.hyp_commit(y, x, s, frm, False, s - 1.0, s + 1.0))
    for g, w in zip(be.hyp_commit(jobs), want):
        WORST["stab"] = max(WORST["stab"], same_delta(g, w, STAB_TOL))
        exact_properties(g, w["L"] - len(w["tokens"]))
        assert np.isfinite(g["stability"]).all()
    print(f"\nlargest |stability - contract| so far {WORST['stab']:.3e}")


def test_a_malformed_job_writes_nothing_while_its_neighbours_are_served_and_launch_arguments(be):
    rng = np.random.default_rng(2)
    y, x = beam(rng, 5, 70, [40, 66, None, 3])
    s = -np.sort(rng.random(5))
    yd, xd = torch.from_numpy(y).to("cuda:0"), torch.from_numpy(x).to("cuda:0")
    sd = tuple(torch.from_numpy(a.copy()).to("cuda:0") for a in (s, s - 1.0, s + 1.0))
    want = R.hyp_commit(y, x, s, 2, False, s - 1.0, s + 1.0)

    def setter(**kw):
        def tweak(k, j):
            if k == 1:
                for f, v in kw.items():
                    setattr(j, f, v)
        return tweak

    bad = [dict(yseq=None), dict(xpos=None), dict(score=None), dict(score_dec=None), dict(score_ctc=None),
           dict(header=None), dict(agree=None), dict(ids=None), dict(pos=None), dict(stability=None), dict(totals=None),
           dict(n_hyp=0), dict(n_hyp=17), dict(L=-1), dict(frm=-1), dict(frm=71), dict(row_stride=69),
           dict(score_stride=0), None]
    for kw in bad:
        got = be.hyp_commit([(yd, xd, sd, 70, 2, False)] * 3, tweak=setter(**kw) if kw else None)
        if kw is not None:
            raw = got[1]["raw"]
            assert all((raw[k] == -7).all() for k in raw), kw
        for k in (0, 2) if kw is not None else (0, 1, 2):
            same_delta(got[k], want, STAB_TOL)
    lib = _abi.load()
    assert lib.sc_hyp_commit(None, 0, None) == 0                     # the empty launch
    assert lib.sc_hyp_commit(None, 2, None) == -1 and lib.sc_hyp_commit(None, -1, None) == -1
    assert lib.sc_hyp_commit(yd.data_ptr(), _abi.COMMIT_MAX_JOBS + 1, None) == -1
    assert be.hyp_commit([]) == []


# ---- stream level ----------------------------------------------------------------------------------------------------
KW = dict(max_frames=400, max_tokens=300, pcm_capacity=1 << 18)
XL_KW = dict(max_frames=160, max_tokens=200, pcm_capacity=1 << 17)
XL = ("XL", "plain", 10, False)
SHAPES = [("TINY",) + r for r in RUNS] + [XL]


@functools.lru_cache(maxsize=None)
def _weights(model, name):
    return packed_weights(model, name, "cuda:0")


def _bits(hyps):
    return [(h["yseq"], h["xpos"], np.asarray([h["score"], h["score_dec"], h["score_ctc"]]).tobytes()) for h in hyps]


def _shape(name):
    return (2, N_CHUNKS, KW) if name == "TINY" else (2, 6, XL_KW)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda r: f"{r[0]}-{r[1]}-beam{r[2]}-{'bbd' if r[3] else 'nobbd'}")
def probe(request):
    """per run, computed once: the lock-step run of the C++ engine that reads the delta at every reply - two streams, the
    last chunk final, stream 1 reset after chunk 3 and fed its audio again from the start - with the hypotheses of every
    reply, and the same run without a single delta call"""
    name, model, w, bbd = request.param
    S, n, kw = _shape(name)
    wts = _weights(model, name)
    pcm = [audio(s, n) for s in SEEDS]

    def run(read):
        sb = make_batch(model, name, "native", S, w, bbd, weights=wts, **kw)
        fol = [Follower(), Follower()]
        replies, deltas, worst = [], [], 0.0
        pos = [0, 0]
        for k in range(n):
            if k == 4:
                sb.reset(1)
                fol[1], pos[1] = Follower(), 0
            fin = k == n - 1
            sb.push([(s, pcm[s][pos[s] * CHUNK:(pos[s] + 1) * CHUNK], fin and s == 0) for s in (0, 1)])
            pos = [q + 1 for q in pos]
            if read:
                frm = [f.frm for f in fol]
                got = sb.hyps_delta([1, 0], [frm[1], frm[0]], final=[0] if fin else [])
            hy = sb.hypotheses_batch([0, 1])
            replies.append([_bits(hy[s]) for s in (0, 1)])
            if read:
                for s in (0, 1):
                    want = R.of_hypotheses(hy[s], frm[s], fin and s == 0)
                    worst = max(worst, same_delta(got[s], want, STAB_TOL))   # ints equal, stability within the bar
                    fol[s].reply(got[s], hy[s], fin and s == 0)
                deltas.append((frm, got))
        return sb, replies, deltas, [f.trace for f in fol], worst

    sb, replies, deltas, traces, worst = run(True)
    _, silent, _, _, _ = run(False)
    return {"param": request.param, "sb": sb, "replies": replies, "silent": silent, "deltas": deltas, "traces": traces,
            "worst": worst, "pcm": pcm, "n": n, "wts": wts, "kw": kw}


def test_lockstep_deltas_equal_the_contract_and_reading_them_changes_nothing(probe):
    p = probe
    name, model, w, bbd = p["param"]
    tr = p["traces"]
    print(f"\n{name}-{model}-beam{w}-{'bbd' if bbd else 'nobbd'}: (L, commit) per reply {tr[0]} | after the reset {tr[1]}; "
          f"largest |stability - contract| = {p['worst']:.3e}")
    assert p["replies"] == p["silent"]                               # hypotheses and scores bit-identical without the calls
    assert tr[0][-1][0] == tr[0][-1][1] > 1                          # the final commits everything
    if name == "TINY" and not bbd:
        assert non_vacuous(tr[0][:-1]), tr[0]
    if name == "XL":
        mid = [c for L, c in tr[0][:-1] if 1 < c < L]
        assert len(mid) >= 2 and mid == sorted(set(mid)), tr[0]


def test_continuous_queue_depth_2_reads_the_snapshot(probe):
    """submit / poll with two chunks of a stream at the engine: the delta of a reported chunk comes from the snapshot rows,
    equals the contract over the snapshot's hypotheses and the lock-step run's delta for the same chunk"""
    p = probe
    name, model, w, bbd = p["param"]
    n = p["n"]
    sb = make_batch(model, name, "native", 2, w, bbd, weights=p["wts"], engine=p["sb"].engine, **p["kw"])
    sb.set_queue_depth(2)
    nxt, rep, queued_behind = [0, 0], [0, 0], 0
    fol = [Follower(), Follower()]
    stop = [n, 4]                                                    # stream 1: the chunks before its reset in the lock-step run

    def feed(s):
        k = nxt[s]
        nxt[s] += 1
        return (s, p["pcm"][s][k * CHUNK:(k + 1) * CHUNK], k == n - 1 and s == 0)

    sb.submit([feed(0), feed(1)])
    sb.submit([feed(0), feed(1)])
    while sb.outstanding:
        done = sorted(sb.poll(1))
        frm = [fol[s].frm for s in done]
        fin = [s for s in done if s == 0 and rep[0] == n - 1]
        got = sb.hyps_delta(done, frm, final=fin)
        hy = sb.hypotheses_batch(done)
        for s, f in zip(done, frm):
            k = rep[s]
            queued_behind += nxt[s] > k + 1                          # a later chunk of the stream is at the engine
            same_delta(got[s], R.of_hypotheses(hy[s], f, s in fin), STAB_TOL)
            lock_frm, lock = p["deltas"][k]
            assert lock_frm[s] == f
            same_delta(got[s], lock[s], 0.0)                         # the same rows, the same kernel: the same bits
            assert _bits(hy[s]) == p["replies"][k][s]
            fol[s].reply(got[s], hy[s], s in fin)
            rep[s] += 1
        again = [feed(s) for s in done if nxt[s] < stop[s]]
        if again:
            sb.submit(again)
    assert rep == stop and queued_behind >= 2


def test_refusals_leave_the_handle_usable():
    from speechcatcher_amd.engine import EngineError
    model, w = "plain", 3
    sb = make_batch(model, "TINY", "native", 3, w, False, weights=_weights(model, "TINY"), **KW)
    pcm = audio(5, 5)
    idle = sb.hyps_delta([0, 2], [0, 0])                              # streams that have not started
    assert all((idle[s]["n_hyp"], idle[s]["L"], idle[s]["commit"], len(idle[s]["tokens"])) == (0, 0, 0, 0) for s in (0, 2))
    with pytest.raises(EngineError, match="from"):
        sb.hyps_delta([2], [1])
    for k in range(4):                                                # (the first three replies hold the <sos> alone)
        sb.push([(s, pcm[k * CHUNK:(k + 1) * CHUNK], False) for s in (0, 1)])
    ok = sb.hyps_delta([0, 1], [0, 0])
    L = ok[0]["L"]
    assert L > 3 and 1 <= ok[0]["n_hyp"] <= w
    ip, dp = _abi.c_int_p, _abi.c_double_p

    def raw(streams, frm, max_tail):
        """the C call itself, with a caller-chosen max_tail"""
        sid, f = np.asarray(streams, np.int32), np.asarray(frm, np.int32)
        m = len(sid)
        out_i = [np.full(m, -7, np.int32) for _ in range(4)]
        ids, xp = np.full((m, max(max_tail, 1)), -7, np.int32), np.full((m, max(max_tail, 1)), -7, np.int32)
        st, sc = np.full((m, max(max_tail, 1)), -7.0), np.full((m, 3), -7.0)
        rc = sb.lib.sc_get_hyps_delta(sb.handle, sid.ctypes.data_as(ip), m, f.ctypes.data_as(ip), None, max_tail,
                                      out_i[0].ctypes.data_as(ip), out_i[1].ctypes.data_as(ip), out_i[2].ctypes.data_as(ip),
                                      ids.ctypes.data_as(ip), xp.ctypes.data_as(ip), st.ctypes.data_as(dp),
                                      sc.ctypes.data_as(dp), out_i[3].ctypes.data_as(ip))
        return rc, out_i, ids, st

    rc, out_i, ids, st = raw([0], [2], L - 2)                         # max_tail exactly the tail: served
    assert rc == 0 and out_i[0][0] == L and ids[0].tolist() == ok[0]["tokens"][2:].tolist()
    for streams, frm, max_tail in (([0], [L + 1], L), ([0], [2], L - 3), ([0, 0], [0, 0], L), ([0], [-1], L), ([7], [0], L)):
        rc, out_i, ids, st = raw(streams, frm, max_tail)
        assert rc == -1, (streams, frm, max_tail)                     # SC_ERR_ARG, nothing written
        assert all((a == -7).all() for a in out_i) and (ids == -7).all() and (st == -7.0).all()
    # a stream whose chunk has not been reported yet is inside a block: refused, also beside one that could be served
    sb.submit([(0, pcm[4 * CHUNK:5 * CHUNK], True)])
    for streams in ([0], [1, 0]):
        with pytest.raises(EngineError, match="inside a decode block"):
            sb.hyps_delta(streams, [0] * len(streams))
    same_delta(sb.hyps_delta([1], [0])[1], ok[1], 0.0)                # the other stream is served meanwhile, unchanged
    assert sorted(sb.poll(1)) == [0]
    # every refusal left the handle usable: the final's delta, against the contract
    fin = sb.hyps_delta([0, 1], [L, 0], final=[0])
    hy = sb.hypotheses_batch([0, 1])
    same_delta(fin[0], R.of_hypotheses(hy[0], L, True), STAB_TOL)
    same_delta(fin[1], R.of_hypotheses(hy[1], 0, False), STAB_TOL)
    assert fin[0]["commit"] == fin[0]["L"] >= L


def test_python_engine_on_the_hip_backend_uses_the_kernel(be):
    """StreamBatch.hyps_delta with a backend that has hyp_commit: the device rows go to the kernel, the result is the
    contract's over hypotheses()"""
    from speechcatcher_amd.hip_backend import HipBackend
    model = "plain"
    sb = make_batch(model, "TINY", HipBackend("cuda:0"), 2, 10, False, weights=_weights(model, "TINY"), **KW)
    calls, real = [], sb.be.hyp_commit
    sb.be.hyp_commit = lambda jobs, **kw: (calls.append(len(jobs)), real(jobs, **kw))[1]
    pcm = audio(5, 4)
    fol = Follower()
    for k in range(4):
        sb.push([(0, pcm[k * CHUNK:(k + 1) * CHUNK], k == 3)])
        frm = fol.frm
        got = sb.hyps_delta([0, 1], [frm, 0], final=[0] if k == 3 else [])
        hy = sb.hypotheses(0)
        same_delta(got[0], R.of_hypotheses(hy, frm, k == 3), STAB_TOL)
        assert got[1]["L"] == 0 and "raw" not in got[0] and "agree" not in got[0]
        fol.reply(got[0], hy, k == 3)
    assert calls == [1, 1, 1, 1] and fol.trace[-1][0] > 2
