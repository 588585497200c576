"""The row pass of csrc/ctc_row.h on the GPU through its three users - sc_ctc_activity (batches of 8 x 64 values),
sc_ctc_draft (8 x 64, the arg-max beside it) and sc_ctc_beam (4 x 64, the register cache of 16 x 64 beside it) - at the
widths where the batch loop can go wrong, against the float64 contracts (tests/ctc_row_ref.py through ctc_activity_ref,
ctc_draft_ref and ctc_beam_ref).  Every int32 equal; floats within the bar of the kernel's own test: p_blank and conf 1e-12
(test_gpu_ctc_activity, test_gpu_ctc_draft), pb / pnb 64 n_frames 2^-53 max(1, |want|) (test_gpu_ctc_beam)."""
import functools

import numpy as np
import pytest
import torch

import ctc_activity_ref as RA
import ctc_beam_ref as RB
import ctc_draft_ref as RD

pytestmark = pytest.mark.gpu

# the lane count, the beam's batch of 4 * 64, the 8 * 64 batch of activity and draft, the beam's cache of 16 * 64: each +- 1
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
T = 20                # sixteen waves take a row each, four of them a second one
THR = 0.8
P_BAR = 1e-12         # test_gpu_ctc_activity's bar on p_blank, test_gpu_ctc_draft's CONF_BAR
BEAM_BAR = lambda n_frames, want: 64.0 * max(n_frames, 1) * 2.0 ** -53 * max(1.0, abs(want))   # noqa: E731 (test_gpu_ctc_beam)
B, C = 16, 8          # nothing is pruned: at most C new prefixes and the stay
NEG = -np.inf
FIXED = {"max_first": 1, "max_last": 4, "one_finite": 7, "all_neg_inf": 10, "nan_last": 13, "inf_last": 16, "tied_ends": 18}


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


@functools.lru_cache(maxsize=None)
def _case(V):
    """(table [T, V] fp32, blank).  Good rows: a seeded permutation of arange(V) * 2^-6 shifted to straddle zero - exact in
    fp32, no ties; the rows of FIXED are edited copies of them"""
    rng = np.random.default_rng(1000 + V)
    vals = ((np.arange(V) - V // 2) * 2.0 ** -6).astype(np.float32)
    x = np.stack([vals[rng.permutation(V)] for _ in range(T)])
    top = np.float32(vals.max() + 1.0)
    x[FIXED["max_first"], 0] = top
    x[FIXED["max_last"], V - 1] = top
    x[FIXED["one_finite"]] = NEG
    x[FIXED["one_finite"], V // 3] = 0.5
    x[FIXED["all_neg_inf"]] = NEG
    x[FIXED["nan_last"], V - 1] = np.nan
    x[FIXED["inf_last"], V - 1] = np.inf
    x[FIXED["tied_ends"], 0] = x[FIXED["tied_ends"], V - 1] = top
    x.setflags(write=False)
    return x, V // 2


def _strided(x, pad=3):
    """the table on the device as a view with a row stride of V + pad floats (NaN between the rows: never read)"""
    n, V = x.shape
    buf = torch.full((n, V + pad), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :V] = torch.from_numpy(x.copy()).to("cuda:0")   # (the shared table itself is read-only)
    return buf[:, :V]


BAD_ROWS = sorted(FIXED[k] for k in ("all_neg_inf", "nan_last", "inf_last"))


@pytest.mark.parametrize("V", WIDTHS)
def test_activity_p_blank(be, V):
    x, blank = _case(V)
    want = RA.p_blank(x, blank)
    assert np.flatnonzero(np.isnan(want)).tolist() == BAD_ROWS
    state, tracks, _ = be.ctc_activity([(_strided(x), blank, 0, T, None)], THR)
    got = tracks[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (V, got, want)
    ok = ~np.isnan(want)
    assert np.abs(want[ok] - THR).min() >= 1e-3, V   # no posterior near the threshold: the state compares exactly
    err = float(np.abs(got[ok] - want[ok]).max())
    print(f"\nV={V}: largest |p_blank - contract| {err:.3e}")
    assert err <= P_BAR, (V, err)
    assert tuple(int(v) for v in state[0]) == RA.scan(RA.INITIAL, want, THR), V


@pytest.mark.parametrize("V", WIDTHS)
def test_draft_label_and_conf(be, V):
    x, blank = _case(V)
    lab, p = RD.rows(x, blank)
    assert np.flatnonzero(lab == RD.BAD).tolist() == BAD_ROWS
    assert lab[FIXED["tied_ends"]] == 0 and lab[FIXED["max_first"]] == 0 and lab[FIXED["max_last"]] == V - 1
    assert lab[FIXED["one_finite"]] == V // 3 and p[FIXED["one_finite"]] == 1.0
    store = []
    want = RD.scan(RD.INITIAL, lab, p, blank, store, T)
    got, after = be.ctc_draft([(_strided(x), blank, 0, T, None, T)])
    g = got[0]
    assert tuple(g[f] for f in RD.FIELDS[:6]) == tuple(want[:6]), (V, g, want)
    assert tuple(after[0][:6]) == tuple(want[:6]), (V, after[0])
    assert [t[:3] for t in g["tokens"]] == [t[:3] for t in store], (V, g["tokens"], store)   # (id, start, end): the labels
    err = max([abs(g["open_conf"] - want[6])] + [abs(a[3] - b[3]) for a, b in zip(g["tokens"], store)])
    print(f"\nV={V}: {len(store)} tokens, largest |conf - contract| {err:.3e}")
    assert err <= P_BAR, (V, err)
    if V > 1:   # the tied row's token is 0, one frame long (its neighbours are good rows with another arg-max)
        t = FIXED["tied_ends"]
        assert lab[t - 1] != 0 and lab[t + 1] != 0
        assert (0, t, t) in [tk[:3] for tk in g["tokens"]], (V, g["tokens"])


@pytest.mark.parametrize("V", WIDTHS)
def test_beam_candidates_and_lse(be, V):
    x, blank = _case(V)
    rows = RB.rows(x, blank, C)
    assert [t for t, r in enumerate(rows) if r is None] == BAD_ROWS
    tab = _strided(x)
    got, _ = be.ctc_beam([(tab, blank, t, t + 1, None, 1 + B, B, C) for t in range(T)])   # one job per row
    worst = 0.0
    for t, (g, r) in enumerate(zip(got, rows)):
        ent = g["entries"]
        if r is None:
            assert (g["n_frames"], g["n_bad"], g["n_nodes"]) == (1, 1, 1) and ent == [(0, -1, 0, -1, 0.0, NEG)], (V, t, g)
            continue
        cand, lp, lpb = r
        assert len(cand) == min(C, V - 1) or t == FIXED["one_finite"]
        assert (g["n_frames"], g["n_bad"], g["n_nodes"]) == (1, 0, 1 + len(cand)), (V, t, g)
        new = [e for e in ent if e[0] != 0]
        stay = [e for e in ent if e[0] == 0]
        # the new prefixes are the candidates, in their order (lp descending, then the lower token): pnb = 0 + lp
        assert [e[1] for e in new] == cand, (V, t, [e[1] for e in new], cand)
        assert [e[:1] + e[2:5] for e in new] == [(1 + i, 1, 0, NEG) for i in range(len(cand))], (V, t, new)
        for e, w in zip(new, lp):
            worst = max(worst, abs(e[5] - w) / BEAM_BAR(1, w))
            assert abs(e[5] - w) <= BEAM_BAR(1, w), (V, t, e, w)
        if lpb == NEG:   # a stay at -inf is dropped
            assert not stay, (V, t, stay)
        else:            # the stay of the empty prefix: pb = 0 + lp(blank)
            assert len(stay) == 1 and stay[0][:4] == (0, -1, 0, -1) and stay[0][5] == NEG, (V, t, stay)
            worst = max(worst, abs(stay[0][4] - lpb) / BEAM_BAR(1, lpb))
            assert abs(stay[0][4] - lpb) <= BEAM_BAR(1, lpb), (V, t, stay, lpb)
        totals = [max(e[4], e[5]) for e in ent]
        assert totals == sorted(totals, reverse=True), (V, t, ent)
    print(f"\nV={V}: largest |pb, pnb - contract| / bar {worst:.3f}")
