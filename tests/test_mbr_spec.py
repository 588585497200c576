"""The contract of consensus finals (tests/mbr_ref.py) checked against itself and against brute force, on
the CPU: the distances against the textbook table, the row-scan form the kernel uses against that table, the metric's
axioms, the minimum-risk row against exhaustive expected edit distance, the backtrace (its slots and gaps reproduce the
row and cost exactly dist edits), the slot statistics' invariants, and two constructed lists."""
import itertools
import math

import numpy as np
import pytest

import mbr_ref as M


def _rows(ys):
    L = max([len(y) for y in ys] + [1])
    return [list(y) + [0] * (L - len(y)) for y in ys], [len(y) for y in ys], L


def _mbr(ys, **kw):
    rows, lens, L = _rows(ys)
    return M.mbr(rows, lens=lens, L=L, **kw)


def _random_lists(seed, count):
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = int(rng.choice([1, 2, 3, 8, 16]))
        V = int(rng.choice([3, 17, 1024]))
        ys = M.family(rng, n, int(rng.integers(0, 131 if k % 5 == 0 else 40)), V, rate=float(rng.uniform(0.05, 0.5)))
        yield ys, V, rng.uniform(-6.0, 0.0, n)


def test_row_scan_form_equals_the_plain_table_and_the_distance_is_a_metric():
    rng = np.random.default_rng(1)
    for _ in range(60):
        V = int(rng.choice([2, 3, 17]))
        a, b, c = (rng.integers(0, V, int(rng.integers(0, 24))) for _ in range(3))
        plain = M.table_plain(a, b)
        assert np.array_equal(M.table_rowscan(a, b), plain)
        d = M.dist_rowscan
        assert d(a, b) == int(plain[-1, -1]) == d(b, a)
        assert d(a, a) == 0 and (d(a, b) == 0) == (len(a) == len(b) and np.array_equal(a, b))
        assert d(a, c) <= d(a, b) + d(b, c)
        assert abs(len(a) - len(b)) <= d(a, b) <= max(len(a), len(b))
    assert M.dist_rowscan([], []) == 0 and M.dist_rowscan([], [1, 2]) == 2 and M.dist_rowscan([5], []) == 1
    assert M.dist_rowscan([1, 2, 3, 4], [2, 3, 4, 5]) == 2
    assert M.dist_rowscan(list(b"kitten"), list(b"sitting")) == 3


def test_dist_matrix_of_a_list_is_symmetric_with_a_zero_diagonal():
    for ys, V, sc in _random_lists(2, 25):
        out = _mbr(ys, score=sc, V=V)
        n = len(ys)
        d = out["dist"][:n, :n]
        assert np.array_equal(d, d.T) and not d.diagonal().any() and (d >= 0).all()
        assert (out["dist"][n:] == -7).all() and (out["dist"][:, n:] == -7).all()
        for h, g in itertools.combinations(range(n), 2):
            assert d[h, g] == int(M.table_plain(out["y"][h], out["y"][g])[-1, -1])


def test_minimum_risk_row_against_exhaustive_expected_edit_distance():
    """N = 3, L <= 4, V = 3: the pivot minimises the expectation of the edit distance under the list's weights, computed
    here with the plain table and exact fractions of the weights' sum"""
    strings = [s for m in range(5) for s in itertools.product(range(3), repeat=m)]
    rng = np.random.default_rng(3)
    moved = 0
    for _ in range(300):
        ys = [list(strings[int(k)]) for k in rng.integers(0, len(strings), 3)]
        w = rng.integers(1, 9, 3) / 16.0                              # dyadic: every product and sum is exact
        out = _mbr(ys, weight=w, V=3)
        expect = [sum(w[j] * int(M.table_plain(ys[h], ys[j])[-1, -1]) for j in range(3)) for h in range(3)]
        assert out["risk"].tolist() == expect
        best = min(range(3), key=lambda h: (expect[h], h))
        assert int(out["header"][0]) == best == int(out["order"][0]) and int(out["header"][1]) == len(ys[best])
        assert sorted(out["order"].tolist()) == [0, 1, 2]
        moved += best != int(np.argmax(w))
    assert moved > 10


def _replay(p, slots, gaps):
    """the row the backtrace describes, and the edits it costs"""
    y, edits = [], 0
    for i in range(len(p) + 1):
        k = gaps.count(i)
        y += [None] * k                                              # insertions in gap i (their symbols come from the row)
        edits += k
        if i < len(p):
            if slots[i] == -1:
                edits += 1
            else:
                y.append(int(slots[i]))
                edits += int(slots[i] != p[i])
    return y, edits


def test_backtrace_reproduces_the_row_and_costs_exactly_the_distance():
    for ys, V, sc in _random_lists(4, 25):
        out = _mbr(ys, score=sc, V=V)
        P = int(out["header"][0])
        p = out["y"][P]
        for j in range(len(ys)):
            shape, edits = _replay(p, out["slots"][j], out["ins"][j])
            assert edits == out["dist"][P, j], (P, j)
            assert len(shape) == len(out["y"][j])
            kept = [c for c in shape if c is not None]
            it = iter(out["y"][j].tolist())
            assert all(any(c == x for x in it) for c in kept)        # the aligned symbols are a subsequence of the row, in order
            assert out["ins"][j] == sorted(out["ins"][j], reverse=True)
        assert out["slots"][P].tolist() == p.tolist() and out["ins"][P] == []


def test_slot_statistics_invariants():
    for ys, V, sc in _random_lists(5, 25):
        out = _mbr(ys, score=sc, V=V)
        P, w = int(out["header"][0]), out["weight"]
        assert math.isclose(w.sum(), 1.0, rel_tol=0, abs_tol=1e-12) and (w >= 0).all()
        for t in range(len(out["conf"])):
            assert out["conf"][t] >= w[P]
            col = out["slots"][:, t]
            masses = {int(s): M.mass_sum(w, [j for j in range(len(ys)) if col[j] == s]) for s in set(col.tolist())}
            assert math.isclose(sum(masses.values()), w.sum(), rel_tol=0, abs_tol=1e-12)
            rivals = {s: m for s, m in masses.items() if s != int(out["y"][P][t])}
            if rivals:
                top = max(rivals.values())
                assert out["alt_mass"][t] == top and out["alt_tok"][t] == min(s for s, m in rivals.items() if m == top)
            else:
                assert out["alt_tok"][t] == -2 and out["alt_mass"][t] == 0.0
        assert len(out["gap_mass"]) == len(out["conf"]) + 1 and (out["gap_mass"] <= w.sum() + 1e-12).all()


def test_identical_rows_agree_completely():
    out = _mbr([[4, 5, 6]] * 4, score=[-1.0, -2.0, -3.0, -4.0], V=10)
    assert np.allclose(out["conf"], 1.0, rtol=0, atol=4 * 2.0 ** -53)    # the four weights' sum, rounded four times
    assert out["alt_tok"].tolist() == [-2] * 3 and not out["alt_mass"].any() and not out["gap_mass"].any()
    assert not out["risk"].any() and out["order"].tolist() == [0, 1, 2, 3] and int(out["header"][0]) == 0


def test_two_weaker_rows_that_agree_move_the_pivot():
    ys = [[1, 2, 3, 4], [1, 2, 9, 4], [1, 2, 9, 4, 7]]
    out = _mbr(ys, weight=[0.4, 0.35, 0.25], V=10)
    assert int(np.argmax(out["weight"])) == 0 and int(out["header"][0]) == 1
    assert out["risk"].tolist() == [0.35 * 1 + 0.25 * 2, 0.4 * 1 + 0.25 * 1, 0.4 * 2 + 0.35 * 1]
    assert out["conf"].tolist() == [1.0, 1.0, 0.35 + 0.25, 1.0]
    assert out["alt_tok"].tolist() == [-2, -2, 3, -2] and out["alt_mass"].tolist() == [0.0, 0.0, 0.4, 0.0]
    assert out["gap_mass"].tolist() == [0.0, 0.0, 0.0, 0.0, 0.25]
    pinned = _mbr(ys, weight=[0.4, 0.35, 0.25], V=10, pivot=0)       # the transcript stays the first row's
    assert int(pinned["header"][0]) == 0 and pinned["order"].tolist() == out["order"].tolist()
    assert pinned["conf"].tolist() == [1.0, 1.0, 0.4, 1.0] and pinned["alt_tok"].tolist() == [-2, -2, 9, -2]


def test_rows_that_are_out_and_lists_without_a_pivot():
    ys = [[1, 2, 3], [1, 99, 3], [1, 3], [2, 2]]
    out = _mbr(ys, score=[-1.0, 0.0, math.nan, -math.inf], V=10)
    assert out["status"].tolist() == [0, M.BAD_TOKEN, M.NONFINITE, 0]
    assert out["weight"].tolist() == [1.0, 0.0, 0.0, 0.0] and out["order"].tolist() == [0, 3, 1, 2]
    assert out["dist"][:4, :4].tolist() == [[0, -1, -1, 2], [-1] * 4, [-1] * 4, [2, -1, -1, 0]]
    assert np.isnan(out["risk"][[1, 2]]).all() and out["risk"][[0, 3]].tolist() == [0.0, 2.0]
    assert out["slots"][1].tolist() == [-2] * 3
    none = _mbr(ys, score=[-1.0, 0.0, math.nan, -math.inf], V=10, pivot=1)
    assert int(none["header"][0]) == -1 and (none["status"] & M.NO_PIVOT).all() and len(none["gap_mass"]) == 0
    even = _mbr(ys, score=[-math.inf] * 4, V=100)
    assert even["weight"].tolist() == [0.25] * 4
    long = M.mbr([[1] * (M.MAX_LEN + 1), [1] * M.MAX_LEN], weight=[0.5, 0.5], L=M.MAX_LEN + 1, lens=[M.MAX_LEN + 1, M.MAX_LEN], V=3)
    assert long["status"].tolist() == [M.TOO_LONG, 0] and int(long["header"][0]) == 1
    for bad in (-0.1, math.inf, math.nan):
        assert _mbr([[1], [2]], weight=[bad, 1.0], V=3)["status"].tolist() == [M.NONFINITE, 0]
    with pytest.raises(AssertionError):
        _mbr([[1]], weight=[1.0], V=3, scale=-1.0)
