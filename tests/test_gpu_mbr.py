"""Consensus of n-best lists on the GPU (csrc/mbr.hip: sc_mbr) against the float64 contract of tests/mbr_ref.py.

With WEIGHTS given every byte of every output buffer is the contract's - float64 as uint64, every int32, the guard words
behind every buffer - no case excluded.  With SCORES given the library's exp() stands in for numpy's: the integers
(order, status, header, dist, alt_tok, slots) must be equal, the doubles within the bar below, and every case first
asserts FROM THE CONTRACT ALONE that no decision is a near-tie - every gap between two risks of a list, and between the two
largest rival masses of a column, is at least 1e-9 or lies between rows with identical labels and scores.

The bar: a weight is exp(z - M) / Z.  Each exp is within 1 ulp of the true value on either side (2 ulp
between them); Z sums at most 16 such terms (their 2 ulp, plus up to 16 roundings that may fall differently) and the
division rounds once: a weight differs by at most about 21 ulp of itself.  A mass or a risk sums at most 16 weights or
products (one more rounding each) with up to 16 roundings of its own: below 64 ulp of the result - 64 * 2^-52 *
max(1, |want|) = 1.42e-14 * max(1, |want|), two orders under the 1e-12 of section 8i.  The largest error is printed.

Shapes: label counts 0, 1, 2, 63, 64, 65, 127, 128, 130 (the lane-stride edges of a 64-lane column split: one, two and three
columns a lane), SC_MBR_MAX_LEN and SC_MBR_MAX_LEN + 1; 1, 2, 3 and 16 rows; V = 3 (ties in the backtrace rule everywhere)
and 1024; rows as mutated copies of a base, and the special lists named in SPECIAL below."""
import functools
import math

import numpy as np
import pytest
import torch

import mbr_ref as M
from speechcatcher_amd import _abi

pytestmark = pytest.mark.gpu

BAR = 64 * 2.0 ** -52
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 130)
SOS, EOS = 1 << 20, 1     # a first token no vocabulary holds (it must be skipped, never judged), and the token rows may end in


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


def _pack(ys, skip=0, ends=None, pad=2, uniform=False):
    """label lists -> (rows [n, width] int32, lens or None, L): ``skip`` SOS tokens in front, EOS behind the rows named in
    ``ends``, -99 (no label anywhere) behind a row's tokens; uniform: every row has L tokens and there is no lens"""
    n = len(ys)
    ends = ends or [False] * n
    lens = [skip + len(y) + int(e) for y, e in zip(ys, ends)]
    L = max(lens) + (0 if uniform else pad % 2)
    rows = np.full((n, L + pad), -99, np.int32)
    for h, y in enumerate(ys):
        rows[h, :skip] = SOS
        rows[h, skip:skip + len(y)] = y
        if ends[h]:
            rows[h, lens[h] - 1] = EOS
    if uniform:
        assert len(set(lens)) == 1
        return rows, None, L
    return rows, lens, L


def _subs(rng, y, V, k):
    y = np.array(y, np.int64)
    for t in rng.choice(len(y), min(k, len(y)), replace=False) if len(y) else []:
        y[t] = (y[t] + 1 + rng.integers(0, V - 1)) % V
    return y


def _family_job(rng, n, length, V, **kw):
    """row 0 the base itself (exactly ``length`` labels), row 1 a copy with substitutions only, the others mutated"""
    base = rng.integers(0, V, length)
    ys = [base]
    if n > 1:
        ys.append(_subs(rng, base, V, 1 + length // 10))
    while len(ys) < n:
        ys.append(M.family(rng, 2, length, V)[0] if rng.random() < 0.2 else _mutate(rng, base, V))
    return dict(ys=ys, V=V, **kw)


def _mutate(rng, base, V, rate=0.15):
    y = []
    for c in base:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            y.append(int(rng.integers(0, V)))
            continue
        y.append(int(c))
        if r > 1 - rate / 3:
            y.append(int(rng.integers(0, V)))
    return np.asarray(y, np.int64)


def _lists(seed):
    """the label side of every case, as dicts: ys, V, and the job's options"""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    for V in (3, 1024):
        for n in (1, 2, 3, 16):
            for length in LENGTHS:
                k += 1
                out.append(_family_job(rng, n, length, V, skip=k % 2, ends=k % 3 == 0, name=f"family V{V} n{n} m{length}"))
    # ---- SPECIAL ------------------------------------------------------------------------------------------------------
    for V in (3, 1024):
        base = rng.integers(0, V, 70)
        mut = [_mutate(rng, base, V) for _ in range(4)]
        out.append(dict(ys=[mut[0], base, mut[0], base, mut[1], base], V=V, name=f"duplicates V{V}"))
        out.append(dict(ys=[mut[0], np.zeros(0, np.int64), mut[1], base], V=V, name=f"one empty row among long ones V{V}"))
        ins = np.insert(base, [0, 5, 5, 33, 70], rng.integers(0, V, 5))
        dele = np.delete(base, [0, 7, 8, 40, 69])
        out.append(dict(ys=[base, ins, dele, mut[2]], V=V, pivot=0, name=f"insertions only, deletions only; named pivot V{V}"))
        out.append(dict(ys=[mut[0], mut[1], mut[2], base], V=V, pivot=2, skip=1, name=f"named pivot V{V}"))
        out.append(dict(ys=[mut[3], mut[1], base], V=V, uniform_of=66, name=f"L instead of lens V{V}"))
        out.append(dict(ys=[base, mut[0], mut[1], mut[2], mut[3]], V=V, bad={0: "token", 2: "value"}, pivot=0,
                        name=f"named pivot that is out V{V}"))
        out.append(dict(ys=[mut[0], mut[1], mut[2]], V=V, bad={0: "token", 1: "value", 2: "lens"}, name=f"all rows out V{V}"))
        out.append(dict(ys=[mut[0], base, mut[1], mut[2], mut[3], base[:60], base[:50], base[:40]], V=V,
                        bad={0: "token", 2: "negative token", 3: "lens", 4: "negative lens", 5: "value", 6: "value2", 7: "value3"},
                        name=f"every kind of bad row V{V}"))
        out.append(dict(ys=[mut[0], mut[1], base, mut[2]], V=V, minus_inf=[1], name=f"a score of -inf V{V}"))
        out.append(dict(ys=[base, base, base], V=V, minus_inf=[0, 1, 2], name=f"all scores -inf V{V}"))
        out.append(dict(ys=[mut[0], mut[1], base], V=V, strided=True, name=f"non-unit strides V{V}"))
    long = rng.integers(0, 3, M.MAX_LEN)
    out.append(dict(ys=[long, _subs(rng, long, 3, 40), _mutate(rng, long[:1000], 3, 0.05)[:M.MAX_LEN]], V=3, name="SC_MBR_MAX_LEN"))
    out.append(dict(ys=[long[:200], rng.integers(0, 3, M.MAX_LEN + 1), _mutate(rng, long[:200], 3)], V=3, name="SC_MBR_MAX_LEN + 1"))
    return out


def _job_of(case, mode, rng):
    """a case's label side -> (host job dict for HipBackend.mbr minus the device tensors, kwargs of the contract)"""
    ys = [np.asarray(y, np.int64) for y in case["ys"]]
    n, V = len(ys), case["V"]
    bad = case.get("bad", {})
    skip = case.get("skip", 0)
    ends = [bool(case.get("ends")) and h % 2 == 0 for h in range(n)]
    if "uniform_of" in case:
        ys = [np.resize(y, case["uniform_of"]) if len(y) else np.zeros(case["uniform_of"], np.int64) for y in ys]
        rows, lens, L = _pack(ys, skip, None, uniform=True)
    else:
        rows, lens, L = _pack(ys, skip, ends)
    for h, kind in bad.items():
        if kind == "token":
            rows[h, skip + len(ys[h]) // 2] = V
        elif kind == "negative token":
            rows[h, skip] = -1
        elif kind == "lens":
            lens[h] = L + 1
        elif kind == "negative lens":
            lens[h] = -1
    if mode == "weight":
        v = rng.uniform(0.0, 1.0, n)
        v = v / v.sum()
        specials = {"value": math.nan, "value2": math.inf, "value3": -0.25}
    else:
        v = rng.uniform(-6.0, 0.0, n)
        specials = {"value": math.nan, "value2": math.inf, "value3": math.nan}
        for h in case.get("minus_inf", []):
            v[h] = -math.inf
    # rows with identical labels carry identical values: their exact ties are no near-ties.  (A row without the trailing
    # EOS whose last label happens to be EOS loses that label, as the contract says.)
    eff = [y[:-1] if case.get("ends") and not ends[h] and len(y) and y[-1] == EOS else y for h, y in enumerate(ys)]
    for h in range(n):
        for g in range(h):
            if np.array_equal(eff[g], eff[h]):
                v[h] = v[g]
                break
    for h, kind in bad.items():
        if kind in specials:
            v[h] = specials[kind]
    scale = 1.0 if mode == "weight" else (0.5 if n == 3 else 1.0)
    job = {"rows": rows, "lens": lens, "L": L, "skip": skip, "strip": EOS if case.get("ends") else -1, "V": V,
           "pivot": case.get("pivot", -1), "scale": scale, "strided": bool(case.get("strided")), "v": v, "name": case["name"]}
    kw = dict(lens=lens, L=L, skip=skip, strip=job["strip"], V=V, scale=scale, pivot=job["pivot"])
    kw["weight" if mode == "weight" else "score"] = v
    return job, kw


_MEMO = {}


@functools.lru_cache(maxsize=None)
def _cases(mode):
    """(jobs, contract outputs) of one mode - computed once, shared by the tests"""
    rng = np.random.default_rng(7 if mode == "weight" else 11)
    jobs, refs = [], []
    for case in _lists(20260):
        job, kw = _job_of(case, mode, rng)
        jobs.append(job)
        refs.append(M.mbr(job["rows"], memo=_MEMO, **kw))
    return jobs, refs


def _device_jobs(jobs, mode, dev="cuda:0"):
    out = []
    for job in jobs:
        rows = torch.from_numpy(job["rows"]).to(dev)
        v = torch.from_numpy(np.asarray(job["v"], np.float64)).to(dev)
        if job["strided"]:
            wide = torch.full((rows.shape[0], rows.shape[1] + 5), -99, dtype=torch.int32, device=dev)
            wide[:, :rows.shape[1]] = rows
            rows = wide[:, :rows.shape[1]]
            if mode == "score":
                tri = torch.full((v.shape[0], 3), math.nan, dtype=torch.float64, device=dev)
                tri[:, 0] = v
                v = tri[:, 0]
        d = {"rows": rows, "L": job["L"], "lens": job["lens"], "skip": job["skip"], "strip": job["strip"], "V": job["V"],
             "pivot": job["pivot"], "scale": job["scale"]}
        d["weights" if mode == "weight" else "scores"] = v
        out.append(d)
    return out


def _expect_raw(job, ref, guard=2, slots=True):
    """the output buffers of HipBackend.mbr as the contract fills them: -7 wherever nothing is written"""
    H = M.MAX_HYPS
    n = job["rows"].shape[0]
    cap = min(max(0, job["L"] - job["skip"]), M.MAX_LEN)
    P, mP = int(ref["header"][0]), int(ref["header"][1])
    f64 = np.full((2, H + guard), -7.0)
    f64[0, :n], f64[1, :n] = ref["weight"], ref["risk"]
    i32 = np.full((2, H + guard), -7, np.int32)
    i32[0, :n], i32[1, :n] = ref["order"], ref["status"]
    dist = np.full(H * H + guard, -7, np.int32)
    dist[:H * H] = ref["dist"].reshape(-1)
    head = np.full(4 + guard, -7, np.int32)
    head[:4] = ref["header"]
    pos = np.full((3, cap + 1 + guard), -7.0)
    atok = np.full(cap + 1 + guard, -7, np.int32)
    sl = np.full(n * cap + guard, -7, np.int32)
    if P >= 0:
        pos[0, :mP], pos[1, :mP], pos[2, :mP + 1] = ref["conf"], ref["alt_mass"], ref["gap_mass"]
        atok[:mP] = ref["alt_tok"]
        sl[:n * cap].reshape(n, cap)[:, :mP] = ref["slots"]
    return {"f64": f64, "i32": i32, "dist": dist, "header": head, "pos": pos, "alt_tok": atok,
            "slots": sl if slots else np.zeros(0, np.int32)}


def _same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
        bad = np.flatnonzero(got.reshape(-1).view(np.uint64 if got.dtype == np.float64 else np.uint32)
                             != want.reshape(-1).view(np.uint64 if got.dtype == np.float64 else np.uint32))
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[:6]}: got {got.reshape(-1)[bad[:6]]} "
                             f"want {want.reshape(-1)[bad[:6]]}")


def _close(got, want, what):
    """doubles within the bar wherever their bits differ; -> the largest error in units of the bar's scale"""
    got, want = got.reshape(-1), want.reshape(-1)
    diff = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    worst = 0.0
    for k in diff:
        assert math.isfinite(want[k]) and math.isfinite(got[k]), f"{what}[{k}]: got {got[k]} want {want[k]}"
        err = abs(got[k] - want[k]) / max(1.0, abs(want[k]))
        assert err <= BAR, f"{what}[{k}]: got {got[k]!r} want {want[k]!r} ({err:.3e} > {BAR:.3e})"
        worst = max(worst, err)
    return worst


def test_with_weights_every_byte_is_the_contracts(be):
    jobs, refs = _cases("weight")
    outs = be.mbr(_device_jobs(jobs, "weight"))
    assert be.mbr_slabs == 1
    for job, ref, out in zip(jobs, refs, outs):
        want = _expect_raw(job, ref)
        for key in want:
            _same_bytes(out["raw"][key], want[key], f"{job['name']}: {key}")
    seen = set()
    for job, ref in zip(jobs, refs):
        seen |= {int(s) for s in ref["status"]}
    assert {0, M.BAD_TOKEN, M.NONFINITE, M.TOO_LONG} <= seen and any(s & M.NO_PIVOT for s in seen)
    assert any(int(ref["header"][0]) != int(np.argmax(job["v"])) for job, ref in zip(jobs, refs)
               if ref["n_in"] == len(job["v"]) and job["pivot"] < 0)       # the minimum-risk row is not always the heaviest


def _no_near_tie(job, ref):
    """from the contract alone: every gap between two risks, and between the two largest rival masses of a column, is at
    least 1e-9 or lies between rows with identical labels and scores"""
    inn = [h for h in range(len(ref["status"])) if not ref["status"][h] & M.OUT]
    same = lambda h, g: np.array_equal(ref["y"][h], ref["y"][g]) and (job["v"][h] == job["v"][g])     # noqa: E731
    for a, h in enumerate(inn):
        for g in inn[a + 1:]:
            assert abs(ref["risk"][h] - ref["risk"][g]) >= 1e-9 or same(h, g), (job["name"], "risk", h, g)
    P = ref["P"]
    if P < 0:
        return
    w = ref["weight"]
    for t in range(len(ref["conf"])):
        col = {}
        for j in inn:
            col.setdefault(int(ref["slots"][j, t]), []).append(j)
        rivals = sorted(((M.mass_sum(w, r), s, r) for s, r in col.items() if s != int(ref["y"][P][t])), reverse=True)
        if len(rivals) >= 2:
            (m0, _, r0), (m1, _, r1) = rivals[:2]
            assert m0 - m1 >= 1e-9 or (len(r0) == len(r1) and all(same(a, b) for a, b in zip(r0, r1))), (job["name"], "mass", t)


def test_with_scores_integers_equal_and_doubles_within_the_bar(be):
    jobs, refs = _cases("score")
    for job, ref in zip(jobs, refs):
        _no_near_tie(job, ref)
    outs = be.mbr(_device_jobs(jobs, "score"))
    worst = 0.0
    for job, ref, out in zip(jobs, refs, outs):
        want = _expect_raw(job, ref)
        for key in ("i32", "dist", "header", "alt_tok", "slots"):
            _same_bytes(out["raw"][key], want[key], f"{job['name']}: {key}")
        for key in ("f64", "pos"):
            worst = max(worst, _close(out["raw"][key], want[key], f"{job['name']}: {key}"))
    print(f"\nsc_mbr with scores: largest error {worst:.3e} of max(1, |want|) over {len(jobs)} lists (bar {BAR:.3e})")


def test_scores_that_need_no_exp_are_bit_exact(be):
    """(beyond the near-tie cases above) when every score is -inf the weights are 1 / n_in and no exp is taken: every
    output is the contract's bit for bit although the risks and masses tie everywhere - ties go to the lower row / symbol"""
    rng = np.random.default_rng(5)
    jobs, refs = [], []
    for V in (3, 1024):
        job, kw = _job_of(_family_job(rng, 6, 40, V, name=f"all -inf family V{V}", minus_inf=range(6)), "score", rng)
        jobs.append(job)
        refs.append(M.mbr(job["rows"], **kw))
    outs = be.mbr(_device_jobs(jobs, "score"))
    for job, ref, out in zip(jobs, refs, outs):
        assert np.all(ref["weight"] == 1.0 / 6)
        want = _expect_raw(job, ref)
        for key in want:
            _same_bytes(out["raw"][key], want[key], f"{job['name']}: {key}")


def test_a_workspace_limit_forces_slabs_and_slots_are_optional(be):
    jobs, refs = _cases("weight")
    pick = [k for k, j in enumerate(jobs) if j["name"].startswith(("family V3 n16", "duplicates", "named pivot"))]
    sub = [jobs[k] for k in pick]
    dj = _device_jobs(sub, "weight")
    for d in dj[::2]:
        d["slots"] = False
    caps = [min(max(0, j["L"] - j["skip"]), M.MAX_LEN) for j in sub]
    limit = int(be.lib.sc_mbr_ws_bytes(3, max(caps)))
    outs = be.mbr(dj, ws_limit=limit)
    assert be.mbr_slabs > 1
    for k, (job, out) in enumerate(zip(sub, outs)):
        want = _expect_raw(job, refs[pick[k]], slots=k % 2 == 1)
        for key in want:
            _same_bytes(out["raw"][key], want[key], f"{job['name']}: {key}")


MALFORMED = {
    "null rows": lambda j: setattr(j, "yseq", None),
    "score and weight": lambda j: setattr(j, "score", j.weight),
    "neither score nor weight": lambda j: setattr(j, "weight", None),
    "null weight_out": lambda j: setattr(j, "weight_out", None),
    "null risk": lambda j: setattr(j, "risk", None),
    "null order": lambda j: setattr(j, "order", None),
    "null status": lambda j: setattr(j, "status", None),
    "null alt_mass": lambda j: setattr(j, "alt_mass", None),
    "null alt_tok": lambda j: setattr(j, "alt_tok", None),
    "null dist": lambda j: setattr(j, "dist", None),
    "null header": lambda j: setattr(j, "header", None),
    "null conf": lambda j: setattr(j, "conf", None),
    "null gap_mass": lambda j: setattr(j, "gap_mass", None),
    "n_hyp 0": lambda j: setattr(j, "n_hyp", 0),
    "n_hyp 17": lambda j: setattr(j, "n_hyp", 17),
    "L < 0": lambda j: setattr(j, "L", -1),
    "row_stride < L": lambda j: setattr(j, "row_stride", j.L - 1),
    "slot_stride too small": lambda j: setattr(j, "slot_stride", j.slot_stride - 1),
    "skip < 0": lambda j: setattr(j, "skip", -1),
    "strip < -1": lambda j: setattr(j, "strip", -2),
    "V 0": lambda j: setattr(j, "V", 0),
    "scale NaN": lambda j: setattr(j, "scale", math.nan),
    "scale inf": lambda j: setattr(j, "scale", math.inf),
    "scale negative": lambda j: setattr(j, "scale", -1.0),
    "pivot -2": lambda j: setattr(j, "pivot", -2),
    "pivot n_hyp": lambda j: setattr(j, "pivot", j.n_hyp),
    "flags": lambda j: setattr(j, "flags", 1),
    "reserved": lambda j: setattr(j, "reserved", 1),
}


def test_malformed_jobs_write_nothing_and_their_neighbours_are_served(be):
    jobs, refs = _cases("weight")
    good = next(k for k, j in enumerate(jobs) if j["name"] == "family V3 n3 m65")
    kinds = list(MALFORMED)
    launch = [jobs[good]] * (2 * len(kinds) + 1)            # good, bad, good, bad, ..., good
    dj = _device_jobs(launch, "weight")

    def tweak(k, j):
        if k % 2 == 1:
            MALFORMED[kinds[k // 2]](j)

    outs = be.mbr(dj, tweak=tweak)
    want = _expect_raw(jobs[good], refs[good])
    for k, out in enumerate(outs):
        for key in want:
            if k % 2 == 0:
                _same_bytes(out["raw"][key], want[key], f"neighbour {k}: {key}")
            else:
                assert np.all(out["raw"][key] == -7), f"{kinds[k // 2]}: {key} was written"
    # score_stride < 1 is malformed where scores are given
    sj, sr = _cases("score")
    dj = _device_jobs([sj[good]] * 2, "score")
    outs = be.mbr(dj, tweak=lambda k, j: setattr(j, "score_stride", 0) if k == 1 else None)
    assert all(np.all(outs[1]["raw"][key] == -7) for key in want)
    _same_bytes(outs[0]["raw"]["header"], _expect_raw(sj[good], sr[good])["header"], "neighbour of score_stride 0")


def test_a_workspace_share_too_small_for_a_job_writes_nothing_of_it(be):
    jobs, refs = _cases("weight")
    small = next(k for k, j in enumerate(jobs) if j["name"] == "family V1024 n3 m2")
    big = next(k for k, j in enumerate(jobs) if j["name"] == "family V1024 n3 m130")
    cap_small = min(max(0, jobs[small]["L"] - jobs[small]["skip"]), M.MAX_LEN)
    outs = be.mbr(_device_jobs([jobs[small], jobs[big]], "weight"), ws_bytes=int(be.lib.sc_mbr_ws_bytes(2, cap_small)))
    want = _expect_raw(jobs[small], refs[small])
    for key in want:
        _same_bytes(outs[0]["raw"][key], want[key], f"the small list: {key}")
        assert np.all(outs[1]["raw"][key] == -7), f"the list whose share is too small: {key} was written"


def test_argument_errors_come_before_any_launch(be):
    lib = be.lib
    assert lib.sc_mbr(None, 0, None, 0, None) == 0
    assert lib.sc_mbr(None, 1, None, 0, None) == -1 and b"null job table" in lib.sc_last_error()
    assert lib.sc_mbr(64, 1, None, 0, None) == -1 and b"null workspace" in lib.sc_last_error()
    assert lib.sc_mbr(64, -1, 64, 0, None) == -1
    assert lib.sc_mbr(64, _abi.MBR_MAX_JOBS + 1, 64, 0, None) == -1 and b"SC_MBR_MAX_JOBS" in lib.sc_last_error()
