"""The packed backoff automaton of speechcatcher_amd/ngram.py against the textbook recursion on the plain dict
(tests/ngram_ref.py), bit for bit, for EVERY context shorter than the order over a small vocabulary - contexts the model
does not hold included - at orders 1, 2 and 4, at the default load and at load 0.95 (long probe runs); a model estimated
from counts sums to 1 in every context; ARPA text round trip; the command-line packer.  No GPU."""
import itertools
import math
import subprocess
import sys

import numpy as np
import pytest

import ngram_ref as NR
from conftest import ROOT
from speechcatcher_amd import ngram

V = 5


def _sentences(rng, n=60, longest=9, V=V):
    return [[int(t) for t in rng.integers(1, V, int(rng.integers(2, longest)))] for _ in range(n)]


def _model(order, seed=1):
    return NR.estimate(_sentences(np.random.default_rng(seed)), V, order)


def _contexts(order):
    for n in range(order):
        yield from itertools.product(range(V), repeat=n)


def _walk(b: ngram.Blob, ctx):
    s = 0
    for c in ctx:
        s = b.score(s, c)[1]
    return s


@pytest.mark.parametrize("load", [0.5, 0.95])
@pytest.mark.parametrize("order", [1, 2, 4])
def test_packed_score_equals_the_dict_recursion_bit_for_bit(order, load):
    model = _model(order)
    b = ngram.Blob(ngram.pack(model, V, order, load=load))
    assert (b.order, b.V) == (order, V) and b.n_arcs == sum(len(g) > 1 for g in model)
    assert b.n_arcs <= load * b.n_slots and (order == 1 or b.n_arcs > 10)
    unseen = 0
    for ctx in _contexts(order):
        s = _walk(b, ctx)                              # the state the automaton is in after ctx, from state 0
        unseen += bool(ctx) and ctx not in model
        for c in range(V):
            got, nxt = b.score(s, c)
            want = NR.logp(model, order, ctx, c)
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (ctx, c, got, want)
            assert nxt == _walk(b, (ctx + (c,))[-(order - 1):] if order > 1 else ())
    assert order < 4 or unseen > 50
    if load == 0.95 and order == 4:
        assert b.longest_probe >= 8, b.longest_probe   # the load does force long probe runs
    # a whole sequence: the raw sum along it, left to right
    seq = [1, 2, 3, 4, 4, 0, 2, 2, 1]
    lm, s = 0.0, 0
    for c in seq:
        l, s = b.score(s, c)
        lm = float(lm + l)
    assert lm == NR.sequence(model, order, seq)


@pytest.mark.parametrize("order", [1, 2, 4])
def test_an_estimated_model_sums_to_one_in_every_context(order):
    model = _model(order, seed=2)
    for ctx in _contexts(order):
        total = math.fsum(math.exp(NR.logp(model, order, ctx, c)) for c in range(V))
        assert abs(total - 1.0) <= 1e-12, (ctx, total)


def test_arpa_text_round_trip_and_the_floor():
    tokens = ["<blank>", "a", "b", "c", "<s>"]
    model = _model(3, seed=3)
    text = ngram.to_arpa(model, tokens, 3)
    back, order = ngram.parse_arpa(text, tokens)
    assert order == 3 and set(back) == set(model)
    for g in model:
        for a, b in zip(back[g], model[g]):
            assert abs(a - b) <= 4 * 2.0 ** -52 * max(1.0, abs(b)), (g, a, b)
    # a hand-written text: log10 -> ln, -99 -> FLOOR, a missing backoff column is 0, unknown words drop their n-grams
    text = "\\data\\\nngram 1=3\nngram 2=2\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1\ta\t-0.25\n-2\tzzz\n\n\\2-grams:\n-0.125\t<s> a\n" \
           "-0.5\ta zzz\n\n\\end\\\n"
    m, order = ngram.parse_arpa(text, tokens)
    assert order == 2 and m == {(4,): (-99 * ngram.LN10, -0.5 * ngram.LN10), (1,): (-ngram.LN10, -0.25 * ngram.LN10),
                                (4, 1): (-0.125 * ngram.LN10, 0.0)}
    b = ngram.Blob(ngram.pack(m, V, order, bos=4))
    assert b.start_state != 0 and b.score(b.start_state, 1)[0] == -0.125 * ngram.LN10
    assert b.score(0, 2) == (ngram.FLOOR, 0)           # a token without a unigram
    for bad in ("\\data\\\n\\1-grams:\n-inf\ta\n\\end\\\n", "\\data\\\n\\1-grams:\nnan\ta\n\\end\\\n"):
        with pytest.raises(ValueError):
            ngram.parse_arpa(bad, tokens)


def test_pack_refuses_what_the_device_must_not_see():
    ok = {(1,): (-1.0, -0.5), (1, 2): (-0.5, 0.0)}
    ngram.pack(ok, V)
    for bad in ({(1, 2): (-0.5, 0.0)},                                # its context is missing
                {(1,): (-np.inf, 0.0)}, {(1,): (-1.0, float("nan"))},  # not finite
                {(7,): (-1.0, 0.0)},                                  # a token outside [0, V)
                {(1,): (-1.0, 0.0), (1, 1): (-1.0, 0.0), (1, 1, 1): (-1.0, 0.0), (1, 1, 1, 1): (-1.0, 0.0),
                 (1, 1, 1, 1, 1): (-1.0, 0.0), (1, 1, 1, 1, 1, 1): (-1.0, 0.0)}):   # order 6
        with pytest.raises(ValueError):
            ngram.pack(bad, V)


def test_the_command_line_packs_an_arpa_file(tmp_path):
    tokens = ["<blank>", "a", "b", "c", "<s>"]
    model = _model(2, seed=4)
    (tmp_path / "m.arpa").write_text(ngram.to_arpa(model, tokens, 2), encoding="utf-8")
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n", encoding="utf-8")
    res = subprocess.run([sys.executable, "-m", "speechcatcher_amd.ngram", str(tmp_path / "m.arpa"),
                          str(tmp_path / "tokens.txt"), str(tmp_path / "m.sclm")], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    b = ngram.Blob((tmp_path / "m.sclm").read_bytes())
    assert (b.V, b.order) == (5, 2) and b.n_arcs == sum(len(g) == 2 for g in model)
