"""The contract of the grammar-constrained CTC prefix beam (tests/ctc_beam_grammar_ref.py) on its own:
against brute force over every path, against the plain contract under the free grammar, chaining, a constructed table
on which the grammar changes the answer, and the compiler of speechcatcher_amd/grammar.py.  No GPU."""
import itertools

import numpy as np
import pytest

import ctc_beam_grammar_ref as G
import ctc_beam_ref as R
from speechcatcher_amd import grammar

NEG = -np.inf


def _structured(rng, T, V, longest=4, lead=(1.0, 3.0)):
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
    n, nbad, nn, ent = state[:4]
    return ((n, nbad, nn), [e[:4] for e in ent], np.asarray([v for e in ent for v in e[4:]], np.float64).tobytes(),
            list(store)) + tuple(state[4:])


def test_unpruned_equals_brute_force_over_the_grammars_prefixes():
    rng = np.random.default_rng(0)
    V, T, blank = 4, 5, 0
    gr = grammar.Grammar(grammar.compile([[1, 2], [1], [3, 3, 1]], V, blank, loop=True))
    x = rng.standard_normal((T, V)).astype(np.float32)
    row = x.astype(np.float64)
    logp = row - np.log(np.exp(row).sum(1, keepdims=True))
    want = {}
    for path in itertools.product(range(V), repeat=T):               # all 1024 paths
        key = R.collapse(path, blank)
        if gr.walk(key) >= 0:                                        # a prefix of the grammar's language
            want[key] = want.get(key, 0.0) + float(np.exp(sum(logp[t, k] for t, k in enumerate(path))))
    state, store = G.scan_table(x, blank, B=10 ** 6, C=16, gr=gr)
    got = {tuple(R.backtrace(e, store)[0]): np.exp(R.total(e)) for e in state[3]}
    assert len(got) == len(state[3]) and set(got) == set(want) and 10 < len(want) < 4 ** 5
    worst = max(abs(got[k] - want[k]) for k in want)
    print(f"\n{len(want)} prefixes; largest |prefix probability - brute force| {worst:.1e}")
    assert worst <= 1e-15
    assert sum(got.values()) < 1.0                                   # the paths outside the grammar are gone
    for e, g in zip(state[3], state[4]):                             # g is the automaton's state after the prefix
        assert g == gr.walk(R.backtrace(e, store)[0])
    totals = [R.total(e) for e in state[3]]
    assert totals == sorted(totals, reverse=True)


@pytest.mark.parametrize("V,B", [(2, 4), (5, 16), (9, 3), (17, 16), (17, 5)])
def test_the_free_grammar_is_the_plain_contract(V, B):
    rng = np.random.default_rng(100 + V)
    for blank in (0, V - 1):
        x = _structured(rng, 60, V)
        x[7, blank] = NEG
        x[9, (blank + 1) % V] = NEG
        x[11, :] = NEG                                               # a bad row
        x[13, 0] = np.nan
        gr = grammar.Grammar(grammar.free(V, blank))
        want, wstore = R.scan_table(x, blank, B, 16)
        got, store = G.scan_table(x, blank, B, 16, gr)
        assert _bits(got[:4], store) == _bits(want, wstore)
        assert got[4] == [0] * len(got[3]) and got[1] == 2


def test_chained_spans_give_the_bits_of_one_span():
    rng = np.random.default_rng(3)
    V, blank = 12, 0
    phrases = [[int(t) for t in rng.integers(1, V, int(rng.integers(1, 5)))] for _ in range(12)]
    gr = grammar.Grammar(grammar.compile(phrases, V, blank))
    x = _structured(rng, 90, V)
    x[40, 3] = np.inf
    one, store1 = G.scan_table(x, blank, 6, 4, gr, capacity=200)
    state, store = None, []
    for a, b in ((0, 1), (1, 1), (1, 17), (17, 64), (64, 90), (90, 90)):
        state, store = G.scan_table(x[a:b], blank, 6, 4, gr, state=state, store=store, capacity=200)
    assert _bits(state, store) == _bits(one, store1) and one[1] == 1 and one[2] > 20


def test_the_grammar_changes_the_answer_on_a_constructed_table():
    """the arg-max path spells (1, 2), which the grammar does not hold; the beam's best is the in-grammar phrase (1, 3);
    the plain contract returns (1, 2)"""
    V, blank = 5, 0
    x = np.full((8, V), -4.0, np.float32)
    for t, k in enumerate((0, 1, 1, 0, 2, 2, 0, 0)):
        x[t, k] = 4.0
    x[4:6, 3] = 2.0                                                  # token 3 is second where 2 wins
    gr = grammar.Grammar(grammar.compile([[1, 3], [4, 4]], V, blank, loop=False))
    plain, pstore = R.scan_table(x, blank, 4, 4)
    got, store = G.scan_table(x, blank, 4, 4, gr)
    assert R.backtrace(plain[3][0], pstore)[0] == [1, 2]
    assert R.backtrace(got[3][0], store)[0] == [1, 3] and gr.accepts(got[4][0])
    for e, g in zip(got[3], got[4]):
        assert g == gr.walk(R.backtrace(e, store)[0]) >= 0
    # a state without arcs only stays: after (1, 3) nothing follows without the loop
    assert gr.arcs(got[4][0]) == []
    # C = 1: the one candidate is the best arc of the ENTRY's state, whatever the row's arg max is
    got1, store1 = G.scan_table(x, blank, 4, 1, gr)
    assert R.backtrace(got1[3][0], store1)[0] == [1, 3]


def test_the_stays_repeat_term_survives_a_last_token_that_is_no_arc():
    """rule 2: an accepted phrase whose last token is not an out-arc of the state it reached keeps its pnb"""
    V, blank = 4, 0
    x = np.zeros((3, V), np.float32)
    x[:, 1] = 3.0                                                    # token 1 three frames long, never a blank
    x[:, blank] = NEG
    gr = grammar.Grammar(grammar.compile([[1]], V, blank, loop=False))
    got, store = G.scan_table(x, blank, 4, 4, gr)
    best = got[3][0]
    assert R.backtrace(best, store)[0] == [1] and best[4] == NEG and best[5] > -1.0
    assert [R.backtrace(e, store)[0] for e in got[3]] == [[1]]       # the empty prefix died with the -inf blank


def test_compile_is_deterministic_and_walked_by_step():
    V, blank = 30, 0
    rng = np.random.default_rng(5)
    phrases = [[int(t) for t in rng.integers(1, V, int(rng.integers(1, 6)))] for _ in range(25)]
    phrases += [phrases[0] + [7, 8], phrases[0][:1], [5], [5, 5], [5, 5, 6]]   # phrases that are prefixes of others
    blob = grammar.compile(phrases, V, blank)
    assert blob == grammar.compile(list(reversed(phrases)) + phrases[:3], V, blank)
    gr = grammar.Grammar(blob)
    for g in range(gr.n_states):                                     # the blob's own rules
        toks = [t for t, _ in gr.arcs(g)]
        assert toks == sorted(set(toks)) and blank not in toks and all(0 <= n < gr.n_states for _, n in gr.arcs(g))
    assert not gr.accepts(gr.start_state)
    for a in phrases:
        assert gr.accepts(gr.walk(a)), a
        for b in phrases:
            assert gr.accepts(gr.walk(a + b)), (a, b)
    held = {tuple(p) for p in phrases}
    flat = grammar.Grammar(grammar.compile(phrases, V, blank, loop=False))
    for a in phrases:
        assert flat.accepts(flat.walk(a))
        for b in phrases:
            s = flat.walk(a + b)
            assert (s >= 0 and flat.accepts(s)) == (tuple(a + b) in held), (a, b)
    # what is no concatenation of phrases is not accepted
    for _ in range(200):
        ids = [int(t) for t in rng.integers(1, V, int(rng.integers(1, 7)))]
        s = gr.walk(ids)

        def splits(seq):
            return not seq or any(tuple(seq[:k]) in held and splits(seq[k:]) for k in range(1, len(seq) + 1))
        assert (s >= 0 and gr.accepts(s)) == splits(ids), ids
    assert gr.step(gr.start_state, blank) == -1 and gr.step(-1, 1) == -1 and gr.step(gr.n_states, 1) == -1


def test_compile_refuses_what_the_blob_cannot_hold():
    for bad in ([[]], [], [[1, 9]], [[-1]], [[1, 0]]):
        with pytest.raises(ValueError):
            grammar.compile(bad, 9, 0)
    with pytest.raises(ValueError):
        grammar.compile([[1]], 4, 4)
    with pytest.raises(ValueError):
        grammar.Grammar(grammar.free(5, 0)[:-8])
    with pytest.raises(ValueError):
        grammar.Grammar(b"\0" * 64)
    free = grammar.Grammar(grammar.free(5, 2))
    assert free.arcs(0) == [(0, 0), (1, 0), (3, 0), (4, 0)] and free.accepts(0)


def test_the_packing_tool_tokenises_phrases_line_by_line(tmp_path):
    tokens = ["<blank>", "▁yes", "▁no", "▁may", "be", "▁"]
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n", encoding="utf-8")
    (tmp_path / "phrases.txt").write_text("yes\nno\n\nmaybe\n", encoding="utf-8")
    out = tmp_path / "menu.scgr"
    assert grammar.main([str(tmp_path / "phrases.txt"), str(tmp_path / "tokens.txt"), str(out)]) == 0
    blob = out.read_bytes()
    assert blob == grammar.compile([[1], [2], [3, 4]], len(tokens), 0) == grammar.load(str(out)) == grammar.load(blob)
    assert grammar.main([]) == 2
