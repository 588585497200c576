"""The contract of n-gram rescoring (tests/lm_rescore_ref.py) against the textbook recursion on the plain
dict (tests/ngram_ref.py), the window guess of the kernel's phase A against the sequential walk, the rounding of
``fused``, the ranking rules, and the fused beam of 8k (tests/ctc_beam_lm_ref.py).  No GPU."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import ctc_beam_lm_ref as BL
import ctc_beam_ref as BR
import lm_rescore_ref as RS
import ngram_ref as NR
from speechcatcher_amd import ngram

V3 = 3
SEQS = [seq for n in range(6) for seq in itertools.product(range(V3), repeat=n)]      # every one of length <= 5


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


@functools.lru_cache(maxsize=None)
def _small(order, bos, load=0.95):
    """(dict, Blob) of a random model over three tokens, closed under prefixes and not under suffixes: about half of
    the extensions of every n-gram it holds, random values (the contract is arithmetic: nothing needs to sum to one).
    Orders above 1 leave token 2 without a unigram - it scores FLOOR and no n-gram holds it."""
    rng = np.random.default_rng(100 * order + (7 if bos is not None else 0))
    val = lambda: (float(-rng.uniform(0.1, 4.0)), float(-rng.uniform(0.0, 1.5)))    # noqa: E731
    model = {(w,): val() for w in range(V3 if order == 1 else V3 - 1)}
    for n in range(2, order + 1):
        for g in [g for g in model if len(g) == n - 1]:
            for w in range(V3 - 1):
                if rng.random() < 0.55 or g + (w,) == (0, 1):
                    model[g + (w,)] = val()
    return model, ngram.Blob(ngram.pack(model, V3, order, bos=bos, load=load))


def _held(model, order):
    """the packer's state ids, from its documented rule: the contexts by (length, tuple), 0 the empty one; and the state
    of the longest suffix of a history that the model holds"""
    sid = {(): 0}
    for g in sorted((g for g in model if len(g) < order), key=lambda g: (len(g), g)):
        sid[g] = len(sid)

    def held(h):
        h = tuple(h)[max(0, len(h) - (order - 1)):] if order > 1 else ()
        while h not in sid:
            h = h[1:]
        return sid[h]
    return held


CASES = [(o, b) for o in (1, 2, 4) for b in (None, 0)]


@pytest.mark.parametrize("order,bos", CASES)
def test_the_walk_is_the_textbook_recursion_bit_for_bit(order, bos):
    model, b = _small(order, bos)
    assert b.order == order and (order == 1 or b.n_arcs > 0)
    held = _held(model, order)
    start = () if bos is None or order == 1 or (bos,) not in model else (bos,)
    assert b.start_state == held(start) and (bos is None or order == 1 or b.start_state != 0)
    for seq in SEQS:
        out = RS.rescore(b, [list(seq)], [0.0], L=len(seq), skip=0)
        want = [NR.logp(model, order, start + seq[:t], seq[t]) for t in range(len(seq))]
        assert _bits(out["tok_lm"][0]) == _bits(want), seq
        assert _bits([out["lm"][0]]) == _bits([NR.sequence(model, order, seq, start)]), seq
        assert out["end_state"][0] == held(start + seq), seq
        assert out["status"][0] == 0 and out["m"][0] == len(seq)


@pytest.mark.parametrize("order,bos", CASES)
def test_the_window_guess_is_the_sequential_state_for_every_packed_model(order, bos):
    """why packed models are expected to take the kernel's fast path: no check of phase B can fail on them"""
    for load in (0.5, 0.95):
        model, b = _small(order, bos, load)
        for state0 in [-1] + list(range(b.n_states)):
            for seq in SEQS:
                s = b.start_state if state0 < 0 else state0
                for t in range(len(seq) + 1):
                    assert RS.window_guess(b, seq, t, state0) == s, (seq, t, state0)
                    if t < len(seq):
                        s = b.score(s, seq[t])[1]


def test_fused_is_rounded_term_by_term_and_not_as_a_fused_multiply_add():
    b = ngram.Blob(ngram.pack({(0,): (-1.0 / 3.0, 0.0), (1,): (-0.1, 0.0)}, 2))
    found = 0
    for alpha in (0.7, 0.3, 1.1, 0.9, 0.123):
        lm, beta, m, score = -1.0 / 3.0, 0.3, 1, 0.0
        exact = Fraction(alpha) * Fraction(lm) + Fraction(beta * m)                  # one rounding: what an fma gives
        fma = float(exact)
        plain = float(np.float64(alpha) * np.float64(lm)) + beta * m
        out = RS.rescore(b, [[0]], [score], L=1, skip=0, alpha=alpha, beta=beta)
        assert _bits(out["lm"]) == _bits([lm])
        assert _bits(out["fused"]) == _bits([plain])
        found += fma != plain
    assert found >= 1                                                                # the case tells the two forms apart


def test_ranking_ties_bad_rows_and_a_single_row():
    b = ngram.Blob(ngram.pack({(0,): (-1.0, 0.0), (1,): (-2.0, 0.0), (2,): (-3.0, 0.0)}, 3))
    rows = [[0, 1], [1, 0], [2, 2], [0, 7], [0, 0], [1, 1]]
    scores = [-5.0, -5.0, float("nan"), 3.0, -5.0, float("inf")]
    out = RS.rescore(b, rows, scores, L=2, skip=0, alpha=1.0)
    assert out["fused"][0] == out["fused"][1] == -8.0 and out["fused"][4] == -7.0    # an exact tie behind the best
    assert out["order"].tolist() == [4, 0, 1, 2, 3, 5]
    assert out["status"].tolist() == [0, 0, RS.NONFINITE, RS.BAD_TOKEN, 0, RS.NONFINITE]
    assert _bits([out["fused"][2], out["fused"][3]]) == [0x7FF8000000000000] * 2 and out["fused"][5] == np.inf
    assert (out["lm"][3], out["eos_lm"][3], out["end_state"][3]) == (0.0, 0.0, -1) and not out["tok_lm"][3].any()
    one = RS.rescore(b, [[0, 1]], [-1.0], L=2, skip=0, alpha=0.5)
    assert one["order"].tolist() == [0] and one["fused"][0] == -2.5
    neg = RS.rescore(b, [[0, -1], [0, 1]], [0.0, 0.0], L=2, skip=0)
    assert neg["status"].tolist() == [RS.BAD_TOKEN, 0] and neg["order"].tolist() == [1, 0]
    # lens: a length outside [0, L] is a bad row; skip and strip cut the labels
    cut = RS.rescore(b, [[9, 0, 1, 2], [9, 0, 2, 0], [9, 2, 0, 0]], [0.0] * 3, lens=[4, 3, 5], L=4, skip=1, strip=2)
    assert cut["m"].tolist() == [2, 1, 0] and cut["status"].tolist() == [0, 0, RS.BAD_TOKEN]
    assert cut["lm"].tolist() == [-3.0, -1.0, 0.0]
    assert RS.labels([9, 2], 2, 1, 2) == [] and RS.labels([2], 1, 1, 2) == [] and RS.labels([9], 1, 3, -1) == []


def test_a_beam_entry_of_the_fused_search_carries_the_rescoring_of_its_ids():
    rng = np.random.default_rng(5)
    T, V = 60, 9
    x = rng.standard_normal((T, V)).astype(np.float32)
    for t in range(T):
        x[t, int(rng.integers(V))] += 3.0
    seq = BR.collapse([int(v) for v in np.argmax(x, 1)], 0)
    model = NR.estimate([seq[k:k + 6] for k in range(0, len(seq), 6)] +
                        [[int(v) for v in rng.integers(1, V, 5)] for _ in range(30)], V, 3)
    b = ngram.Blob(ngram.pack(model, V, 3))
    state, store = BL.scan_table(x, 0, 8, 8, b, 0.5, 0.3)
    ent, side = state[3], state[4]
    assert len(ent) == 8
    ids = [BR.backtrace(e, store)[0] for e in ent]
    L = max(len(y) for y in ids)
    assert L > 5
    rows = [y + [0] * (L - len(y)) for y in ids]
    out = RS.rescore(b, rows, [BR.total(e) for e in ent], lens=[len(y) for y in ids], L=L, skip=0, alpha=0.5, beta=0.3)
    assert _bits(out["lm"]) == _bits([s[0] for s in side])
    assert out["end_state"].tolist() == [s[1] for s in side]
    assert _bits(out["fused"]) == _bits([BL.fused(e, s, 0.5, 0.3) for e, s in zip(ent, side)])
    assert out["order"].tolist() == list(range(8))                                   # the beam keeps its entries by fused


def test_the_model_flips_a_close_list_and_zero_weight_does_not():
    # the model has seen "1 2" and never "2 1"
    model = NR.estimate([[1, 2]] * 8 + [[2]], 3, 2)
    b = ngram.Blob(ngram.pack(model, 3, 2))
    rows, scores = [[0, 2, 1], [0, 1, 2]], [-4.0, -4.001]
    off = RS.rescore(b, rows, scores, L=3, skip=1, alpha=0.0)
    on = RS.rescore(b, rows, scores, L=3, skip=1, alpha=0.5)
    assert off["order"].tolist() == [0, 1] and _bits(off["fused"]) == _bits(scores)
    assert on["order"].tolist() == [1, 0] and on["lm"][1] > on["lm"][0]


def test_the_end_term_prefers_the_row_that_ends_where_the_model_expects_an_end():
    # sentences end in 2 (then </s> = 3); 1 is never last
    eos = 3
    model = NR.estimate([[1, 2, eos]] * 6 + [[1, 1, 2, eos]] * 3, 4, 3)
    b = ngram.Blob(ngram.pack(model, 4, 3))
    rows, scores = [[1, 2, 1], [1, 1, 2]], [-3.0, -3.0]
    plain = RS.rescore(b, rows, scores, L=3, skip=0, alpha=1.0)
    ended = RS.rescore(b, rows, scores, L=3, skip=0, alpha=1.0, lm_eos=eos)
    assert _bits(plain["lm"]) == _bits(ended["lm"]) and not plain["eos_lm"].any()
    assert ended["eos_lm"][1] > ended["eos_lm"][0]
    gap = plain["lm"][0] - plain["lm"][1]
    # weights at which only the end term decides: the rows' totals are set so that row 0 leads without it
    scores = [-3.0, -3.0 + gap - 0.5 * (ended["eos_lm"][1] - ended["eos_lm"][0])]
    plain = RS.rescore(b, rows, scores, L=3, skip=0, alpha=1.0)
    ended = RS.rescore(b, rows, scores, L=3, skip=0, alpha=1.0, lm_eos=eos)
    assert plain["order"].tolist() == [0, 1] and ended["order"].tolist() == [1, 0]
    for h in range(2):
        s = ended["end_state"][h]
        assert _bits([ended["eos_lm"][h]]) == _bits([b.score(int(s), eos)[0]])
        assert _bits([ended["fused"][h]]) == _bits([scores[h] + 1.0 * float(ended["lm"][h] + ended["eos_lm"][h])])
