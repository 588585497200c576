"""The contract of the CTC prefix beam search with a fused n-gram model (tests/ctc_beam_lm_ref.py): against
brute force over every path plus the model's score of the prefix, against ctc_beam_ref at alpha = beta = 0, chaining, and a
constructed table on which only the model separates two tokens.  No GPU."""
import itertools

import numpy as np

import ctc_beam_lm_ref as L
import ctc_beam_ref as R
import ngram_ref as NR
from speechcatcher_amd import ngram
from test_ctc_beam_spec import _bits, _structured

NEG = -np.inf


def _lm(V, order, seed=7, n=80, bos=None):
    rng = np.random.default_rng(seed)
    sents = [[int(t) for t in rng.integers(1, V, int(rng.integers(2, 9)))] for _ in range(n)]
    model = NR.estimate(sents, V, order, bos=bos)
    return model, ngram.Blob(ngram.pack(model, V, order, bos=bos))


def _lm_bits(state, store):
    return _bits(state[:4], store) + (np.asarray([s[0] for s in state[4]], np.float64).tobytes(), [s[1] for s in state[4]])


def test_unpruned_fused_scores_equal_brute_force_plus_the_models_score():
    rng = np.random.default_rng(0)
    V, T, blank = 3, 5, 0
    x = rng.standard_normal((T, V)).astype(np.float32)
    row = x.astype(np.float64)
    logp = row - np.log(np.exp(row).sum(1, keepdims=True))
    want = {}
    for path in itertools.product(range(V), repeat=T):
        key = R.collapse(path, blank)
        want[key] = want.get(key, 0.0) + float(np.exp(sum(logp[t, k] for t, k in enumerate(path))))
    assert len(list(itertools.product(range(V), repeat=T))) == 243
    for order, alpha, beta in ((1, 0.7, 0.0), (2, 0.5, 0.3), (3, 1.25, -0.4)):
        model, lm = _lm(V, order)
        state, store = L.scan_table(x, blank, 10 ** 6, V - 1, lm, alpha, beta)
        assert len(state[3]) == len(want) == 25
        fused = []
        for e, sd in zip(state[3], state[4]):
            ids = tuple(R.backtrace(e, store)[0])
            # pb / pnb are the pure CTC prefix probability: the bar of ctc_beam_spec's brute-force test
            assert abs(np.exp(R.total(e)) - want[ids]) <= 1e-15, ids
            # lm is the textbook recursion's sum along the prefix, bit for bit, ctx the state of the prefix
            assert np.float64(sd[0]).tobytes() == np.float64(NR.sequence(model, order, ids)).tobytes(), ids
            s = 0
            for c in ids:
                s = lm.score(s, c)[1]
            assert sd[1] == s
            w = float(float(alpha * NR.sequence(model, order, ids)) + float(beta * float(len(ids))))
            fused.append(float(R.total(e) + w))
            assert L.fused(e, sd, alpha, beta) == fused[-1]
            assert abs(np.exp(fused[-1] - w) - want[ids]) <= 1e-15, ids
        assert fused == sorted(fused, reverse=True)                  # the entries are ranked by the fused score
        pure, _ = R.scan_table(x, blank, 10 ** 6, V - 1)
        assert [e[:4] for e in pure[3]] != [e[:4] for e in state[3]]  # ... which is another order than the acoustic one


def test_zero_weights_give_the_bits_of_the_plain_contract():
    rng = np.random.default_rng(5)
    x = _structured(rng, 90, 12)
    x[17, 3] = np.nan
    x[40] = NEG
    _, lm = _lm(12, 3)
    for B, C, cap in ((4, 3, 1 << 30), (16, 16, 1 << 30), (3, 2, 20), (1, 1, 5)):
        gp, gl = [], []
        plain, pstore = R.scan_table(x, 0, B, C, capacity=cap, gaps=gp)
        got, store = L.scan_table(x, 0, B, C, lm, 0.0, 0.0, capacity=cap, gaps=gl)
        assert _bits(got[:4], store) == _bits(plain, pstore) and gp == gl
        assert all(sd[0] < 0.0 for e, sd in zip(got[3], got[4]) if e[2] > 0)   # the model's sums are carried all the same


def test_chained_spans_give_the_bits_of_one_span():
    rng = np.random.default_rng(4)
    x = _structured(rng, 90, 12)
    x[17, 3] = np.nan
    x[40] = NEG
    _, lm = _lm(12, 4, bos=11)
    assert lm.start_state != 0
    for B, C, cap in ((4, 3, 1 << 30), (16, 16, 1 << 30), (3, 2, 20)):
        one, one_store = L.scan_table(x, 0, B, C, lm, 0.6, 0.2, capacity=cap)
        rws = R.rows(x, 0, C)
        state, store = L.initial(lm), []
        for a, b in zip([0, 0, 1, 16, 17, 18, 18, 64], [0, 1, 16, 17, 18, 18, 64, 90]):
            state = L.scan(state, rws[a:b], store, cap, B, lm, 0.6, 0.2)
        assert _lm_bits(state, store) == _lm_bits(one, one_store)
        assert len(one_store) == min(one[2], cap) and one[1] == 2 and one[0] == 90


def test_the_model_separates_two_tokens_that_tie_acoustically():
    """tokens 2 and 3 tie within 1e-3 at the frames where "1 ?" is decided, token 2 a hair ahead; the model has seen
    "1 3" often and "1 2" never.  Without the model (alpha = 0) the best prefix is 1 2, with it 1 3."""
    V, blank = 5, 0
    x = np.full((6, V), -6.0, np.float32)
    x[0:2, 1] = 4.0                                                  # "1"
    x[2, blank] = 4.0
    x[3:5, 2] = 4.0                                                  # "2" ...
    x[3:5, 3] = 4.0 - 1e-3                                           # ... and "3", within the margin
    x[5, blank] = 4.0
    sents = [[1, 3]] * 30 + [[2, 1], [4, 2], [3, 4]]
    model = NR.estimate(sents, V, 2)
    lm = ngram.Blob(ngram.pack(model, V, 2))
    assert NR.logp(model, 2, (1,), 3) - NR.logp(model, 2, (1,), 2) > 2.0
    best = {}
    for alpha in (0.0, 0.5):
        state, store = L.scan_table(x, blank, 4, 4, lm, alpha, 0.0)
        best[alpha] = R.backtrace(state[3][0], store)[0]
        tot = {tuple(R.backtrace(e, store)[0]): R.total(e) for e in state[3]}
        assert 0.0 < tot[(1, 2)] - tot[(1, 3)] < 3e-3                # the acoustic near-tie, whatever the model says
    assert best[0.0] == [1, 2] and best[0.5] == [1, 3]
    plain, pstore = R.scan_table(x, blank, 4, 4)
    assert R.backtrace(plain[3][0], pstore)[0] == [1, 2]
