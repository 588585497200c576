"""The contract of the CTC prefix beam search (tests/ctc_beam_ref.py) against brute force over every
path, against the greedy draft (tests/ctc_draft_ref.py), and its own rules: chaining, ties, bad rows, -inf entries.
No GPU."""
import itertools

import numpy as np

import ctc_beam_ref as R
import ctc_draft_ref as D

NEG = -np.inf


def _structured(rng, T, V, blank=0, longest=4, lead=(1.0, 3.0)):
    """label runs of 1..longest frames (blank among the labels) with a lead of lead[0]..lead[1] over unit noise"""
    x = rng.standard_normal((T, V)).astype(np.float32)
    t = 0
    while t < T:
        lab = int(rng.integers(V))
        for _ in range(int(rng.integers(1, longest + 1))):
            if t < T:
                x[t, lab] = x[t].max() + np.float32(rng.uniform(*lead))
                t += 1
    return x


def _bits(state, store):
    n, nbad, nn, ent = state
    return ((n, nbad, nn), [e[:4] for e in ent], np.asarray([v for e in ent for v in e[4:]], np.float64).tobytes(),
            list(store))


def test_unpruned_equals_brute_force_over_all_paths_and_sums_to_one():
    rng = np.random.default_rng(0)
    V, T, blank = 3, 5, 0
    x = rng.standard_normal((T, V)).astype(np.float32)
    row = x.astype(np.float64)
    logp = row - np.log(np.exp(row).sum(1, keepdims=True))
    want = {}
    for path in itertools.product(range(V), repeat=T):
        key = R.collapse(path, blank)
        want[key] = want.get(key, 0.0) + float(np.exp(sum(logp[t, k] for t, k in enumerate(path))))
    state, store = R.scan_table(x, blank, B=10 ** 6, C=V - 1)
    got = {tuple(R.backtrace(e, store)[0]): np.exp(R.total(e)) for e in state[3]}
    assert len(got) == len(state[3]) == len(want) == 25
    worst = max(abs(got[k] - want[k]) for k in want)
    print(f"\nlargest |prefix probability - brute force| {worst:.1e}")
    assert worst <= 1e-15
    assert abs(sum(got.values()) - 1.0) <= 1e-15
    assert state[:3] == (T, 0, len(store)) and store[0] == R.ROOT
    for e in state[3]:                                               # the tree: len, last, parent and frames hang together
        ids, frames = R.backtrace(e, store)
        assert len(ids) == e[2] and (ids[-1] if ids else -1) == e[1] and frames == sorted(set(frames))
        assert e[3] == (store[e[0]][0] if e[0] else -1)
    totals = [R.total(e) for e in state[3]]
    assert totals == sorted(totals, reverse=True)


def test_beam_1_candidate_1_is_the_collapsed_arg_max_path_on_peaked_rows():
    """B = C = 1 follows the arg-max path wherever every row's winner holds most of the mass (a flat row lets the stay's
    two terms outweigh a repeat across a blank): asserted here at a posterior of at least 0.75."""
    for seed, V in ((1, 5), (2, 64), (3, 300)):
        rng = np.random.default_rng(seed)
        x = _structured(rng, 160, V, lead=(np.log(3.0 * V) + 1.0, np.log(3.0 * V) + 3.0))
        lab, p = D.rows(x, 0)
        assert p.min() >= 0.75
        dstate, dstore = D.scan_table(x, 0)
        draft = D.draft(dstate, dstore)
        state, store = R.scan_table(x, 0, B=1, C=1)
        assert len(state[3]) == 1
        ids, frames = R.backtrace(state[3][0], store)
        assert ids == [t[0] for t in draft] and frames == [t[1] for t in draft] and len(ids) >= 30


def test_beam_1_candidate_1_leaves_the_arg_max_path_on_a_flat_row():
    """the limit of the property above, pinned: "a", then a blank at 0.55 against 0.45, then "a" at 0.55 against 0.45.
    The arg-max path a - a spells "a a".  The one entry holds "a" with pb = 0.495 and pnb = 0.405 after the blank; its
    stay is worth (0.495 + 0.405) 0.45 + 0.405 0.55 = 0.628, the repeat across the blank pb 0.55 = 0.272: it stays "a"."""
    x = np.log(np.asarray([[0.1, 0.9], [0.55, 0.45], [0.45, 0.55]])).astype(np.float32)
    lab, _ = D.rows(x, 0)
    assert lab.tolist() == [1, 0, 1]
    dstate, dstore = D.scan_table(x, 0)
    assert [t[0] for t in D.draft(dstate, dstore)] == [1, 1]
    state, store = R.scan_table(x, 0, B=1, C=1)
    assert R.backtrace(state[3][0], store)[0] == [1]
    assert abs(np.exp(R.total(state[3][0])) - 0.62775) < 1e-6
    wide, wstore = R.scan_table(x, 0, B=4, C=1)                       # a wider beam holds both, "a" ahead of "a a"
    assert [R.backtrace(e, wstore)[0] for e in wide[3][:2]] == [[1], [1, 1]]
    assert abs(np.exp(R.total(wide[3][1])) - 0.27225) < 1e-6


def test_chained_spans_give_the_bits_of_one_span():
    rng = np.random.default_rng(4)
    x = _structured(rng, 90, 12)
    x[17, 3] = np.nan
    x[40] = NEG
    for B, C, cap in ((4, 3, 1 << 30), (16, 16, 1 << 30), (3, 2, 20)):
        one, one_store = R.scan_table(x, 0, B, C, capacity=cap)
        rws = R.rows(x, 0, C)
        state, store = R.initial(), []
        for a, b in zip([0, 0, 1, 16, 17, 18, 18, 64], [0, 1, 16, 17, 18, 18, 64, 90]):
            state = R.scan(state, rws[a:b], store, cap, B)
        assert _bits(state, store) == _bits(one, one_store)
        assert len(one_store) == min(one[2], cap) and one[1] == 2 and one[0] == 90


def test_tie_rules_on_duplicated_columns():
    blank = 0
    # frame 0: the blank ties token 1 (stay before a new prefix), tokens 1 and 2 tie (the lower token first)
    x = np.asarray([[1.0, 1.0, 1.0, 0.0]], np.float32)
    state, store = R.scan_table(x, blank, B=4, C=3)
    assert [e[:4] for e in state[3]] == [(0, -1, 0, -1), (1, 1, 1, 0), (2, 2, 1, 0), (3, 3, 1, 0)]
    assert store == [R.ROOT, (0, 1, 0), (0, 2, 0), (0, 3, 0)]
    t = [R.total(e) for e in state[3]]
    assert t[0] == t[1] == t[2] > t[3]
    # the C-th candidate: of two equal columns the lower one is taken
    state, store = R.scan_table(x, blank, B=4, C=1)
    assert [e[1] for e in state[3]] == [-1, 1]
    state, store = R.scan_table(x[:, [0, 3, 1, 2]], blank, B=4, C=2)    # tokens 2 and 3 tie ahead of token 1
    assert [e[1] for e in state[3]] == [-1, 2, 3]
    # two entries of equal total extended by one token: the lower parent rank first
    x = np.asarray([[0.0, 2.0, 2.0, -1.0], [0.0, -1.0, -1.0, 3.0]], np.float32)
    gaps = []
    state, store = R.scan_table(x, blank, B=4, C=3, gaps=gaps)
    assert [e[:4] for e in state[3]][:2] == [(4, 3, 2, 1), (5, 3, 2, 2)]
    assert R.total(state[3][0]) == R.total(state[3][1])
    assert [R.backtrace(e, store)[0] for e in state[3][:2]] == [[1, 3], [2, 3]]
    assert gaps[0] == 0.0 and all(g >= 0.0 for g in gaps)
    # duplicated columns all along: the two prefixes keep the same bits, the lower token stays ahead
    rng = np.random.default_rng(5)
    y = _structured(rng, 60, 6)
    y = np.concatenate([y, y[:, 2:3]], 1)                               # column 6 = column 2
    state, store = R.scan_table(y, blank, B=16, C=16)
    seqs = [tuple(R.backtrace(e, store)[0]) for e in state[3]]
    swap = {2: 6, 6: 2}
    for e, s in zip(state[3], seqs):
        twin = tuple(swap.get(k, k) for k in s)
        if twin != s and twin in seqs:
            f = state[3][seqs.index(twin)]
            assert (e[4], e[5]) == (f[4], f[5])
    assert any(6 in s for s in seqs)


def test_bad_rows_and_minus_inf_entries():
    rng = np.random.default_rng(6)
    V, blank = 9, 0
    x = _structured(rng, 40, V)
    clean = x.copy()
    bad = [3, 4, 20, 39]
    x = np.insert(x, bad, 0.0, axis=0)
    rows_bad = [3, 5, 22, 42]
    x[3, 2] = np.nan
    x[5, 7] = np.inf
    x[22] = NEG
    x[42, 0] = np.nan
    state, store = R.scan_table(x, blank, 4, 3)
    want, wstore = R.scan_table(clean, blank, 4, 3)
    assert state[:3] == (44, 4, want[2]) and want[:2] == (40, 0)
    assert [e for e in state[3]] == [e for e in want[3]]               # a bad row changes nothing but the counts ...
    shift = lambda f: f + sum(r <= f + k for k, r in enumerate(rows_bad))   # noqa: E731
    assert [(p, t) for p, t, _ in store] == [(p, t) for p, t, _ in wstore]
    assert [f for _, _, f in store[1:]] == [shift(f) for _, _, f in wstore[1:]]   # ... and the frame numbers behind it
    # a blank at -inf: the stay's pb is -inf, the beam goes on through its pnb and the extensions
    y = clean.copy()
    y[:, blank] = NEG
    state, store = R.scan_table(y, blank, 4, 3)
    assert all(e[4] == NEG and np.isfinite(e[5]) for e in state[3]) and state[1] == 0 and len(state[3]) == 4
    # tokens at -inf are no candidates; a row with the blank alone keeps every prefix, the empty one included
    z = np.full((3, V), NEG, np.float32)
    z[:, blank] = 0.0
    z[1, 4] = 0.0
    state, store = R.scan_table(z, blank, 4, 8)
    assert [e[:4] for e in state[3]] == [(0, -1, 0, -1), (1, 4, 1, 0)] and store == [R.ROOT, (0, 4, 1)]
    assert [R.total(e) for e in state[3]] == [np.log(0.5)] * 2
    assert R.rows(z, blank, 8)[0] == ([], [], 0.0) and R.rows(z[:, :1], blank, 8)[0] == ([], [], 0.0)
    # a state of more entries than B is cut to its first B
    wide, _ = R.scan_table(clean[:10], blank, 8, 3)
    cut = R.scan(wide, [], [], 0, 2)
    assert cut[3] == wide[3][:2] and cut[:3] == wide[:3]
