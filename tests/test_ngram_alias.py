"""``python -m speechcatcher_amd.ngram --alias WORD=TOKEN``: ARPA words that stand for entries of the token list, the merge
of <s> and </s> on ONE <sos/eos> id (logp from </s>, backoff from <s>), and the unchanged three-argument form."""
import math

import pytest

from speechcatcher_amd import ngram

LN10 = math.log(10.0)
ARPA = """\\data\\
ngram 1=4
ngram 2=4

\\1-grams:
-99\t<s>\t-0.5
-0.7\t</s>
-0.4\ta\t-0.3
-0.6\tb\t-0.2

\\2-grams:
-0.1\t<s> a
-0.2\ta b
-0.3\tb </s>
-0.9\ta </s>

\\end\\
"""
TOKENS = ["<blank>", "a", "b", "<sos/eos>"]
ALIAS = {"<s>": "<sos/eos>", "</s>": "<sos/eos>"}


def test_two_words_on_one_id_merge_logp_from_the_end_and_backoff_from_the_start():
    model, order = ngram.parse_arpa(ARPA, TOKENS, ALIAS)
    assert order == 2
    assert model[(3,)] == (-0.7 * LN10, -0.5 * LN10)                 # predicted as </s>, conditions as <s>
    assert model[(3, 1)] == (-0.1 * LN10, 0.0) and model[(2, 3)] == (-0.3 * LN10, 0.0) and model[(1, 3)] == (-0.9 * LN10, 0.0)
    assert set(model) == {(1,), (2,), (3,), (3, 1), (1, 2), (2, 3), (1, 3)}
    # the order of the two unigrams in the file does not matter
    swapped = ARPA.replace("-99\t<s>\t-0.5\n-0.7\t</s>\n", "-0.7\t</s>\n-99\t<s>\t-0.5\n")
    assert swapped != ARPA and ngram.parse_arpa(swapped, TOKENS, ALIAS)[0] == model
    # the automaton: it starts behind <s>, and the end term of "a b" is p(</s> | b)
    b = ngram.Blob(ngram.pack(model, len(TOKENS), order, bos=3))
    assert b.start_state != 0
    l, s = b.score(b.start_state, 1)
    assert l == -0.1 * LN10
    l, s = b.score(s, 2)
    assert l == -0.2 * LN10 and b.score(s, 3)[0] == -0.3 * LN10
    assert b.score(0, 3)[0] == -0.7 * LN10                           # the unigram of the end


def test_other_words_on_one_id_and_unknown_targets_are_errors():
    with pytest.raises(ValueError, match="neither is <s>"):
        ngram.parse_arpa(ARPA, TOKENS, {"b": "a"})
    with pytest.raises(ValueError, match="not in the token list"):
        ngram.parse_arpa(ARPA, TOKENS, {"<s>": "<eos>"})
    # one alias alone is a plain renaming
    model, _ = ngram.parse_arpa(ARPA, TOKENS, {"</s>": "<sos/eos>"})
    assert model[(3,)] == (-0.7 * LN10, 0.0) and (3, 1) not in model and (2, 3) in model


def test_the_command_line_with_aliases_and_the_unchanged_three_argument_form(tmp_path, capsys):
    arpa, toks = tmp_path / "m.arpa", tmp_path / "tokens.txt"
    arpa.write_text(ARPA)
    toks.write_text("\n".join(TOKENS) + "\n")
    out = tmp_path / "m.sclm"
    assert ngram.main(["--alias", "<s>=<sos/eos>", str(arpa), str(toks), "--alias", "</s>=<sos/eos>", str(out)]) == 0
    said = capsys.readouterr().out
    assert "bos 3, eos 3" in said
    want = ngram.pack(*ngram.parse_arpa(ARPA, TOKENS, ALIAS)[:1], len(TOKENS), 2, bos=3)
    assert out.read_bytes() == want and ngram.Blob(want).start_state != 0
    assert ngram.main(["--alias", "<s>", str(arpa), str(toks), str(out)]) == 2
    with pytest.raises(ValueError, match="not in the token list"):
        ngram.main(["--alias", "<s>=nope", str(arpa), str(toks), str(out)])
    # three arguments: <s> and </s> are no entries of this list, their n-grams are left out, as before
    plain = tmp_path / "plain.sclm"
    assert ngram.main([str(arpa), str(toks), str(plain)]) == 0
    said = capsys.readouterr().out
    assert "bos" not in said and "order 2, V 4" in said
    model, order = ngram.parse_arpa(ARPA, TOKENS)
    assert set(model) == {(1,), (2,), (1, 2)}
    assert plain.read_bytes() == ngram.pack(model, len(TOKENS), order, bos=None)
    toks.write_text("\n".join(["<blank>", "a", "b", "<s>"]) + "\n")      # a list that holds <s> itself: bos as before
    assert ngram.main([str(arpa), str(toks), str(plain)]) == 0
    assert ngram.Blob(plain.read_bytes()).start_state != 0
    assert ngram.main([str(arpa), str(toks)]) == 2
