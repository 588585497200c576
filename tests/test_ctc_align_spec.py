"""The float32 spec of the CTC forced alignment (tests/ctc_align_ref.py) against brute force over every CTC path,
its edge cases, and the host-side helpers of speechcatcher_amd/align.py (frames -> seconds, SentencePiece words).
No GPU."""
import numpy as np
import pytest

import ctc_align_ref as ref
from speechcatcher_amd import align
from conftest import GOLDEN, load_case
from speechcatcher_amd.config import TINY, XL


@pytest.mark.parametrize("seed", range(40))
def test_spec_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    T, L, V = int(rng.integers(1, 9)), int(rng.integers(0, 4)), 5
    y = rng.integers(1, V, L)
    if seed % 3 == 0 and L >= 2:
        y[1] = y[0]                                           # a repeat: the skip over the blank is not allowed
    exact = seed % 2 == 0
    e = rng.integers(-3, 1, (T, V)).astype(np.float32) if exact else rng.standard_normal((T, V)).astype(np.float32)
    st, path, score = ref.viterbi(e, y, 0)
    best, bpath = ref.brute_force(e, y, 0)
    if st != ref.OK:
        assert st == ref.INFEASIBLE and best is None
        return
    assert best == score
    if exact:                                                 # integer sums: the tie rule decides among equal paths
        np.testing.assert_array_equal(path, bpath)


def test_constant_table_all_ties():
    e = np.zeros((8, 4), np.float32)
    st, path, score = ref.viterbi(e, [1, 2], 0)
    best, bpath = ref.brute_force(e, [1, 2], 0)
    assert st == ref.OK and score == best == 0.0
    np.testing.assert_array_equal(path, bpath)
    # ties go to staying: the path enters state 1 at frame 0 and ends in the last label state, not the trailing blank
    assert path[0] == 1 and path[-1] == 3


def test_repeats_and_feasibility():
    y = [3, 3, 3]
    e = np.random.default_rng(1).standard_normal((5, 6)).astype(np.float32)   # L + repeats = 5: just feasible
    r = ref.align(e, y, 0)
    assert r["status"] == ref.OK
    np.testing.assert_array_equal(r["path"], [1, 2, 3, 4, 5])
    np.testing.assert_array_equal(r["start"], [0, 2, 4])
    np.testing.assert_array_equal(r["end"], [1, 3, 5])
    assert ref.align(e[:4], y, 0)["status"] == ref.INFEASIBLE
    assert ref.align(e[:3], [3, 4, 5], 0)["status"] == ref.OK       # no repeats: T = L suffices
    assert ref.align(e[:0], [], 0)["status"] == ref.OK
    assert ref.align(e[:0], [1], 0)["status"] == ref.INFEASIBLE
    assert ref.align(e, [0, 1], 0)["status"] == ref.BAD_INPUT        # the blank is not a label
    assert ref.align(e, [9], 0)["status"] == ref.BAD_INPUT
    bad = e.copy()
    bad[2, 5] = np.inf
    assert ref.align(bad, [1], 0)["status"] == ref.NONFINITE


def test_score_is_the_sequential_fp32_sum_and_rows_shift_freely():
    rng = np.random.default_rng(3)
    e = (rng.standard_normal((40, 16)) * 5).astype(np.float32)
    y = [4, 7, 7, 2]
    r = ref.align(e, y, 0)
    lab = ref.state_labels(np.array(y), 0)[r["path"]]
    acc = np.float32(0.0)
    for t in range(40):
        acc = np.float32(acc + e[t, lab[t]])
    assert acc.tobytes() == r["path_score"].tobytes()
    # raw logits (quirk A1) vs log-softmaxed rows: same path, same confidences
    lsm = (e - np.log(np.exp(e.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)
    r2 = ref.align(lsm, y, 0)
    np.testing.assert_array_equal(r["path"], r2["path"])
    np.testing.assert_allclose(r["logp_mean"], r2["logp_mean"], atol=1e-5)
    assert np.all(r["logp_mean"] <= 0)


def test_frame_to_time_geometry():
    hop, sub, sr = XL.hop_length, XL.subsample, XL.sample_rate
    assert align.frame_span_samples(0, hop, sub) == (hop, 5 * hop)
    assert align.frame_span_samples(10, hop, sub) == (41 * hop, 45 * hop)
    a, b = align.cfg_frames_to_seconds(XL, [0, 25], [1, 50], offset_s=60.0)
    assert a == [60.0 + 0.01, 60.0 + 1.01] and b == [60.0 + 0.05, 60.0 + 2.01]   # 40 ms per frame, 25 frames per s


FIXTURES = sorted(p.stem for p in GOLDEN.glob("*_c*_b*.json"))


@pytest.mark.parametrize("name", FIXTURES)
def test_feature_clock_reproduces_the_fixture_frame_counts(name):
    """FeatureClock replays SURVEY Appendix D item 1 over the calls of a fixture of the real reference (10 240-, 8 192-
    and 25 600-sample calls): the feature frames it keeps, subsampled, are the encoder frames the reference's stream
    ends with - 2 STFT frames fewer per call boundary than one continuous STFT of the audio would give"""
    js, _ = load_case(name)
    m = js["meta"]
    cfg = XL if m["model"] == "XL" else TINY
    clk = align.FeatureClock(cfg.win_length, cfg.hop_length)
    pos = 0
    for call in js["calls"]:
        end = min(pos + m["chunk"], m["n_samples"])
        clk.call(end - pos, end >= m["n_samples"])
        pos = end
    assert align.subsampled_frames(len(clk.centres)) == js["calls"][-1]["enc_buffer_len"]
    n_calls = len(js["calls"])
    assert len(clk.centres) == 1 + m["n_samples"] // cfg.hop_length - 2 * (n_calls - 1)
    gaps = np.diff(clk.centres)
    assert set(gaps.tolist()) <= {cfg.hop_length, 3 * cfg.hop_length}      # a hop, or a hop + the 2 dropped frames
    assert int(np.sum(gaps == 3 * cfg.hop_length)) == n_calls - 1
    # the continuous rule is right on the first call only; after k boundaries it is 2k hops early
    t = len(clk.centres) // 4 - 2
    assert clk.frame_span(t, cfg.subsample)[0] - align.frame_span_samples(t, cfg.hop_length, cfg.subsample)[0] == \
        2 * cfg.hop_length * int(np.sum(gaps[:4 * t + 3] == 3 * cfg.hop_length))


def test_cli_token_alignment_argument():
    from speechcatcher_amd.__main__ import make_parser
    assert make_parser().parse_args(["--token-alignment", "a.wav"]).token_alignment is True
    assert make_parser().parse_args(["a.wav"]).token_alignment is False


def test_paragraph_merge_carries_the_alignment_keys():
    from speechcatcher_amd.segmenter import merge_paragraphs
    seg = lambda text, k: {"start": k, "end": k + 1, "text": text, "tokens": [text], "token_timestamps": [k],  # noqa: E731
                           "token_start": [k + 0.1], "token_end": [k + 0.2], "token_conf": [0.5]}
    _, info = merge_paragraphs([seg("a", 0), seg("b", 1), seg("c.", 2)])
    assert info[0]["token_start"] == [0.1, 1.1, 2.1] and info[0]["token_conf"] == [0.5] * 3
    plain = [{k: v for k, v in seg(t, i).items() if not k.startswith("token_") or k == "token_timestamps"}
             for i, t in enumerate(("a", "b."))]
    _, info = merge_paragraphs(plain)
    assert not any(k in info[0] for k in ("token_start", "token_end", "token_conf"))


def test_vosk_result_aligned():
    from speechcatcher_amd.server_session import vosk_result, vosk_result_aligned
    toks = ["▁Hal", "lo", "▁Welt"]
    al = {"start_s": [0.1, 0.3, 0.5], "end_s": [0.3, 0.4, 0.9], "conf": [0.5, 0.8, None]}
    al["start_s"][2] = None
    r = vosk_result_aligned(toks, al)
    assert r["text"] == vosk_result(toks)["text"] == "Hallo Welt"
    assert r["result"] == [{"conf": pytest.approx(0.4), "start": 0.1, "end": 0.4, "word": "Hallo"}]


def test_vosk_word_merge():
    toks = ["▁Hal", "lo", "▁", "Welt", "▁!"]
    w = align.merge_words(toks, [0.0, 0.1, 0.3, 0.35, 0.6], [0.1, 0.2, 0.35, 0.5, 0.7], [0.9, 0.5, 1.0, 0.8, 0.6])
    assert [x["word"] for x in w] == ["Hallo", "Welt", "!"]
    assert w[0]["start"] == 0.0 and w[0]["end"] == 0.2 and w[0]["conf"] == pytest.approx(0.45)
    assert w[1]["start"] == 0.3 and w[1]["end"] == 0.5 and w[1]["conf"] == pytest.approx(0.8)
    assert w[2]["conf"] == pytest.approx(0.6)
    assert align.merge_words(["ab", "▁c"], [0, 1], [1, 2], [0.5, 0.5])[0]["word"] == "ab"
