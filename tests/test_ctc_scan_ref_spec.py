"""The float64 reference of tests/ctc_scan_ref.py against the fp32 torch spec (SpecBackend.ctc_prefix_scan / ctc_gather_state) on
the CPU, on every case of the table that tests/test_gpu_ctc_scan.py launches on the GPU.  The same run measures kappa_ref for the
GPU module.  Also here: which outputs are logzero follows from the lengths alone (nothing hides behind the -1e9 mask), and the
error model is tight enough to see five deliberate mistakes planted into the float32 transcription of the segment-affine form."""
import math

import numpy as np
import pytest

import ctc_scan_ref as cr

# A charges every walked frame ONE unit 2^-24 of 1 + the largest magnitude the frame handles.  An fp32 evaluation rounds, per frame
# and forward variable, the difference, the exponential, 1 + e and the logarithm (units of at most 1), the maximum + logarithm and
# the added table entry (units of the magnitude), and reads phi as an fp32 sum: at most 8 units.  A reference that takes phi or
# x from a neighbouring frame is off by 1e4 and more.
KAPPA_MAX = 8.0


def _walks(c):
    return any(c.streams[s].start < c.streams[s].Te for s in c.live)


@pytest.mark.parametrize("name", list(cr.CASES))
def test_reference_against_the_spec(name, capsys):
    """psi, psi_eos, r[t] and r^n (+) r^b of every (stream, hypothesis, candidate), the checkpoints the spec stores and the rows
    its rebuild hands the winners: within the fp32 error of the spec, the same entries logzero; kappa_ref of every output that
    has walked frames is a positive number (an output whose every value is exact measures nothing)."""
    c = cr.case(name)
    kref, kspec, kaff = cr.kappa_ref(name)       # (asserts that the masks agree)
    with capsys.disabled():
        print(f"\n{name}: " + "; ".join(f"{n}: spec {kspec[n]:.3g} affine-f32 {kaff[n]:.3g}" for n in cr.OUTPUTS))
    for n in cr.OUTPUTS:
        assert math.isfinite(kref[n]) and kspec[n] <= KAPPA_MAX and kaff[n] <= KAPPA_MAX, (name, n, kspec[n], kaff[n])
        if _walks(c) and n != "psi_eos":
            assert kref[n] > 0, (name, n)
    assert kref["psi_eos"] >= 0


@pytest.mark.parametrize("name", list(cr.CASES))
def test_only_structural_zeros_are_excluded(name):
    """The entries of the reference at or below -1e9 are exactly those the lengths make logzero (cr.expected_live).  For psi
    these are the blank candidates, every pair of a stream with L > 1 and L - 1 >= T, and the candidates that repeat the last
    token of a prefix WITH a state when a single frame is walked (phi of that frame is the prefix's r^b, logzero there); for
    the forward variables behind start, r^b at frame start when L > 1 (both states in front of it are logzero), and for a
    repeat with a state r^n at start and r^b at start + 1.  Everything else the tests compare as numbers."""
    c = cr.case(name)
    for s in c.live:
        st, d = c.streams[s], c.data[s]
        ref, ids = d["ref"], d["ids"][:st.nh]
        exp = cr.expected_live(st, ref["same"], ids, c.blank, c.eos)
        for n in ("psi", "psi_eos", "r", "rs"):
            assert np.array_equal(ref[n] > cr.LIVE, exp[n]), (name, s, n)
        T, L, start = st.Te, st.L, st.start
        nothing = L > 1 and L - 1 >= T
        repeat = ref["same"] & bool(st.has) & (L > 1)
        normal = (ids != c.blank) & (ids != c.eos)
        dead = ~(ref["psi"] > cr.LIVE)
        assert np.array_equal(dead & normal, normal & (nothing | (repeat & (T - start == 1)))), (name, s)
        assert dead[ids == c.blank].all()
        live_r = ref["r"] > cr.LIVE
        for t in range(start, T):
            assert np.array_equal(live_r[t, 0], ~(repeat & (t == start))), (name, s, t)
            assert np.array_equal(live_r[t, 1], ~((L > 1) & ((t == start) | (repeat & (t == start + 1))))), (name, s, t)
        assert not live_r[:start - 1].any() and not live_r[start - 1, 1].any()
        assert live_r[start - 1, 0].all() == (L == 1) and live_r[start - 1, 0].any() == (L == 1)


def test_the_table_covers_the_edges():
    """what the issue lists, read off the table itself"""
    seq = [c for c in cr.CASES.values() if c.split_min == 0]
    par = [c for c in cr.CASES.values() if c.split_min == 16]
    live = lambda cs: [(c, cr.Stream(*r)) for c in cs for r in c.streams if r[0]]   # noqa: E731
    pairs = {(st.T, st.L) for _, st in live(seq)}
    assert {(T, L) for T in (1, 2, 15, 16, 17, 31, 32, 33) for L in (1, 2, 3)} <= pairs
    assert {(40, 16), (40, 17), (40, 18)} <= pairs
    assert any(st.L - 1 == st.T for _, st in live(seq)) and any(st.L - 1 == st.T + 4 for _, st in live(seq))
    assert any(st.T == c.max_frames and c.max_frames % 16 for c, st in live(seq))
    assert any(st.tctc == 24 and st.T == 40 for _, st in live(seq))
    assert {c.V for c in seq} >= {1024, 1182, 37} and {c.W for c in seq} == {10, 5} == {c.W for c in par}
    for cs in (seq, par):
        assert {st.has for _, st in live(cs)} == {0, 1}
        assert all(sum(1 for r in c.streams if not r[0]) == 1 for c in cs)
        assert all(c.max_frames <= 640 for c in cs)
    assert all({r[3] for r in c.streams if r[0]} == {c.W, c.W - 3, 1} for c in seq)
    assert all((c.max_frames + 15) // 16 >= 32 for c in par)
    thr = cr.CASES["par_threshold_15_16"]
    gaps = {st.Te - st.start: cr.is_split(st, thr.max_frames, 16) for c, st in live([thr])}
    assert gaps[15] is False and gaps[16] is True
    splits = [(c, st) for c, st in live(par) if cr.is_split(st, c.max_frames, 16)]
    assert {(st.start % 16, st.Te % 16) for _, st in splits} >= {(a, b) for a in (0, 1, 15) for b in (0, 1, 15)}
    assert {st.Te - (st.start & ~15) for _, st in splits} >= {17, 512, 513}
    assert sum(1 for lo, hi in cr.Stream(1, 17, 2, 10, 1).segments() if lo >= hi) == 30
    assert any((st.nh * min(40, c.V)) % 8 for c, st in splits)
    assert all(3 <= len(c.streams) <= 4 for c in seq)
    for c in par:            # every T-parallel case splits some streams and leaves others to the sequential kernel
        forms = {cr.is_split(st, c.max_frames, 16) for c_, st in live([c])}
        assert forms == {False, True}, c.name


@pytest.mark.parametrize("plant", cr.PLANTS)
def test_the_error_model_sees_a_planted_mistake(plant, capsys):
    """each mistake, planted into the float32 transcription of the segment-affine form, pushes some kappa above 4 x kappa_ref on
    at least one case of the table (the T-parallel cases are tried first: the plants sit in segments behind the first)"""
    names = sorted(cr.CASES, key=lambda n: (cr.CASES[n].split_min == 0, cr.CASES[n].max_frames))
    for name in names:
        c = cr.case(name)
        kref = cr.kappa_ref(name)[0]
        k = cr.affine_kappas(c, plant)
        seen = {n: k[n][0] for n in cr.OUTPUTS if k[n][0] > 4 * kref[n]}
        if seen:
            with capsys.disabled():
                print(f"\n{plant}: seen on {name}: " + "; ".join(f"{n} kappa {v:.3g} (kappa_ref {kref[n]:.3g})" for n, v in seen.items()))
            return
    pytest.fail(f"{plant}: no case of the table sees it")
