"""The contract of the CTC token alternates (tests/ctc_alt_ref.py) on hand-made tables, and the host side
built on it - posteriors of an n-best list, token records, the Vosk messages of a ServerLoop over a fake batch, the ctypes
mirror of the job struct.  No GPU."""
import ctypes
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ctc_alt_ref as ref
from speechcatcher_amd import _abi, alternates
from speechcatcher_amd.config import TINY
from speechcatcher_amd.scheduler import StreamScheduler
from speechcatcher_amd.server_session import ServerLoop

ROOT = Path(__file__).resolve().parent.parent
NINF = -np.inf


def _peaked(path, V, hot=5.0, rest=-5.0):
    x = np.full((len(path), V), rest, np.float32)
    x[np.arange(len(path)), path] = hot
    return x


def test_a_span_on_the_argmax_path_has_rank_0_and_is_its_own_first_alternate():
    path = [3, 3, 0, 7, 7, 7, 0, 2]
    x = _peaked(path, 9)
    ids, logp, rank, st = ref.alternates(x, 0, [3, 7, 2], [0, 3, 7], [2, 6, 8], 3)
    assert st.tolist() == [0, 0, 0] and rank.tolist() == [0, 0, 0]
    assert ids[:, 0].tolist() == [3, 7, 2]
    # every other candidate has the same sum: v ascending behind the winner
    assert ids[0].tolist() == [3, 1, 2] and ids[1].tolist() == [7, 1, 2] and ids[2].tolist() == [2, 1, 3]
    # logp is the mean log-posterior: the same for a span of 2 and of 3 equal frames
    lse = 5.0 + np.log(1.0 + 8 * np.exp(-10.0))
    np.testing.assert_allclose(logp[:, 0], 5.0 - lse, rtol=0, atol=1e-14)
    np.testing.assert_allclose(logp[:, 1], -5.0 - lse, rtol=0, atol=1e-14)
    # a label that is not the best of its frames [2, 6): 7 is ahead of everything, the blank is no candidate, and among
    # the equal sums of the rest the lower ids are ahead
    for y, want in ((1, 1), (4, 4), (8, 7), (7, 0)):
        assert ref.alternates(x, 0, [y], [2], [6], 3)[2].tolist() == [want]


def test_a_constant_added_to_a_row_changes_no_id():
    rng = np.random.RandomState(3)
    x = (rng.randint(-40, 40, size=(10, 17)) * 0.25).astype(np.float32)   # multiples of 0.25: the shifted sums stay exact
    y = x + (rng.randint(-8, 8, size=(10, 1)) * 0.5).astype(np.float32)
    args = ([4, 9, 2], [0, 3, 4], [3, 4, 10], 8)
    a, b = ref.alternates(x, 16, *args), ref.alternates(y, 16, *args)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_allclose(a[1], b[1], rtol=0, atol=1e-13)   # and the posteriors agree


def test_ties_go_to_the_lower_id():
    x = np.zeros((4, 6), np.float32)
    x[:, 4] = 1.0
    x[:, 2] = 1.0
    ids, logp, rank, _ = ref.alternates(x, 1, [4, 2, 5, 0], [0, 0, 0, 0], [4, 4, 4, 4], 5)
    assert ids[0].tolist() == [2, 4, 0, 3, 5]
    assert rank.tolist() == [1, 0, 4, 2]
    assert logp[0, 0] == logp[0, 1] and logp[0, 2] == logp[0, 3] == logp[0, 4]


def test_the_sum_runs_in_ascending_frame_order():
    """1e30 + 1e-3 - 1e30 is 0 in frame order and 1e-3 in any order that cancels first: column 1 must lose to column 2"""
    x = np.full((3, 4), -1.0, np.float32)
    x[:, 1] = [1e30, 1e-3, -1e30]
    x[:, 2] = [0.0, 5e-4, 0.0]
    assert ref.span_sums(x, 0, 3)[1] == 0.0
    ids, _, rank, st = ref.alternates(x, 0, [1], [0], [3], 3)
    assert st.tolist() == [0] and ids[0].tolist() == [2, 1, 3] and rank.tolist() == [1]
    # the rows reversed: (-1e30 + 1e-3) + 1e30 is 0 as well, but two of the three frames alone are not
    ids, _, _, _ = ref.alternates(x, 0, [1], [1], [3], 3)
    assert ids[0].tolist() == [2, 3, 1]


@pytest.mark.parametrize("bad", ["nan", "+inf", "all -inf"])
def test_status_precedence_and_bad_rows_only_inside_the_span(bad):
    x = _peaked([1, 2, 3, 1, 2, 3], 4)
    x[2] = {"nan": [0, np.nan, 0, 0], "+inf": [0, 0, np.inf, 0], "all -inf": [NINF] * 4}[bad]
    T = x.shape[0]
    start = [-1, 3, 5, 0, 2, 1, 3, 0, 2 ** 31 - 1, 0]
    end = [2, 3, 4, T + 1, 2 ** 31 - 1, 3, 6, 2, 2 ** 31 - 1, 6]
    ids, logp, rank, st = ref.alternates(x, 0, [1] * len(start), start, end, 2)
    #          negative, empty, reversed, past T, past T from a bad row: NO_SPAN wins; bad inside; clean; clean; INT_MAX; bad
    assert st.tolist() == [1, 1, 1, 1, 1, 2, 0, 0, 1, 2]
    for k in np.nonzero(st)[0]:
        assert ids[k].tolist() == [-1, -1] and (logp[k] == NINF).all() and rank[k] == -1
    assert ids[6].tolist() == [1, 2] and rank[6] == 0   # frames 3..5: one frame each of 1, 2, 3 - a tie, the lowest id


def test_minus_inf_columns_and_k_above_the_candidates():
    x = np.zeros((2, 3), np.float32)
    x[:, 2] = NINF
    ids, logp, rank, st = ref.alternates(x, 1, [2, 0], [0, 0], [2, 1], 8)
    assert st.tolist() == [0, 0]
    assert ids[0].tolist() == [0, 2] + [-1] * 6 and ids[1].tolist() == [0, 2] + [-1] * 6
    assert logp[0, 0] == -np.log(2.0) and logp[0, 1] == NINF and (logp[0, 2:] == NINF).all()
    assert rank.tolist() == [1, 0]
    # V = 2: one candidate; V = 1: none
    ids, _, rank, st = ref.alternates(np.zeros((1, 2), np.float32), 0, [1], [0], [1], 2)
    assert ids[0].tolist() == [1, -1] and rank.tolist() == [0] and st.tolist() == [0]
    ids, _, rank, st = ref.alternates(np.zeros((1, 1), np.float32), 0, [0], [0], [1], 2)
    assert ids[0].tolist() == [-1, -1] and rank.tolist() == [-1] and st.tolist() == [0]


def test_a_label_that_is_no_candidate_has_rank_minus_one_and_the_span_is_still_computed():
    x = _peaked([2, 2], 5)
    ids, logp, rank, st = ref.alternates(x, 0, [0, 5, -1, 2], [0] * 4, [2] * 4, 2)
    assert st.tolist() == [0] * 4 and rank.tolist() == [-1, -1, -1, 0]
    assert all(ids[k].tolist() == [2, 1] for k in range(4)) and np.isfinite(logp).all()


def test_nbest_posterior_on_hand_numbers():
    p = alternates.nbest_posterior(np.log([0.5, 0.25, 0.25]) - 123.0)
    np.testing.assert_allclose(p, [0.5, 0.25, 0.25], rtol=0, atol=1e-15)
    assert alternates.nbest_posterior([-3.0]) == [1.0]
    assert alternates.nbest_posterior([NINF, -2.0]) == [0.0, 1.0]
    assert alternates.nbest_posterior([]) == []
    assert alternates.nbest_posterior([NINF, NINF]) == [0.5, 0.5]
    p = alternates.nbest_posterior([-1e4, -1e4 - np.log(3.0)])   # far below exp's range: the difference decides
    np.testing.assert_allclose(p, [0.75, 0.25], rtol=0, atol=1e-12)


# ---- the host side over a fake batch ----------------------------------------------------------------------------------
TOKENS = [("▁w%d" if t % 2 == 0 else "x%d") % t for t in range(1024)]
HYPS = [[1023, 6, 7, 8, 1023], [1023, 6, 9, 1023], [1023, 10, 1023]]
SCORES = [-1.0, -1.0 - np.log(2.0), -1.0 - np.log(2.0)]


class FakeBatch:
    """what StreamScheduler needs of a C++-engine batch: three finished hypotheses per final, an alignment that gives
    token k of every hypothesis the frames [2k, 2k + 2), and alternates computed by the contract over a fixed table"""
    S, W, LCAP = 1, 3, 8
    cfg = TINY

    def __init__(self):
        rng = np.random.RandomState(5)
        self.table = rng.randn(12, 1024).astype(np.float32)
        self.calls = []

    def reset(self, slot):
        pass

    def push(self, items, isolate_faults=False):
        return {slot: True for slot, _, _ in items}

    def hypotheses_arrays(self, want):
        n = len(want)
        ids = np.zeros((n, 3, self.LCAP), np.int32)
        lens = np.zeros((n, 3), np.int32)
        for j, y in enumerate(HYPS):
            ids[:, j, :len(y)] = y
            lens[:, j] = len(y)
        sc = np.tile(np.asarray(SCORES), (n, 1))
        return {"ids": ids, "xpos": np.zeros_like(ids), "lens": lens, "n_hyps": np.full(n, 3, np.int32), "score": sc,
                "score_dec": sc, "score_ctc": sc}

    def align(self, streams, nbest=None):
        self.calls.append(("align", int(nbest)))
        return self._align(len(streams), int(nbest))

    def _align(self, n, nb):
        start = np.tile(2 * np.arange(self.LCAP, dtype=np.int32), (n, nb, 1))
        lp = np.full((n, nb, self.LCAP), np.log(0.5), np.float32)
        return {"start": start, "end": start + 2, "logp_mean": lp, "path_score": np.zeros((n, nb)),
                "status": np.zeros((n, nb), np.int32), "n_hyps": np.full(n, min(nb, 3), np.int32)}

    def alternates(self, streams, nbest=None, k=3):
        self.calls.append(("alternates", int(nbest), int(k)))
        n, nb = len(streams), int(nbest)
        al = self._align(n, nb)
        al["alt_ids"] = np.full((n, nb, self.LCAP, k), -1, np.int32)
        al["alt_logp"] = np.full((n, nb, self.LCAP, k), NINF)
        al["own_rank"] = np.full((n, nb, self.LCAP), -1, np.int32)
        al["span_status"] = np.full((n, nb, self.LCAP), ref.NO_SPAN, np.int32)
        for j in range(min(nb, 3)):
            y = HYPS[j][1:-1]
            L = len(y)
            a = ref.alternates(self.table, 0, y, al["start"][0, j, :L], al["end"][0, j, :L], k)
            for i in range(n):
                al["alt_ids"][i, j, :L], al["alt_logp"][i, j, :L] = a[0], a[1]
                al["own_rank"][i, j, :L], al["span_status"][i, j, :L] = a[2], a[3]
        return al


def _final(loop, config=None):
    sid = loop.connect()
    if config is not None:
        loop.submit(sid, json.dumps({"config": config}))
    loop.submit(sid, np.zeros(4000, np.int16))
    loop.submit(sid, '{"eof" : 1}')
    out = []
    while loop.pending():
        out.extend(loop.step().get(sid, []))
    loop.disconnect(sid)
    return [m for m in out if isinstance(m, dict) and "partial" not in m]


def _loop(**kw):
    fb = FakeBatch()
    return ServerLoop(StreamScheduler(fb, TOKENS, result_format="espnet"), vosk_output_format=True, **kw), fb


def test_scheduler_alignment_carries_the_records_from_one_call_in_place_of_align():
    fb = FakeBatch()
    sch = StreamScheduler(fb, TOKENS, result_format="espnet", align_final=True, alternates=4)
    sid = sch.open()
    sch.feed(sid, np.zeros(4000, np.float32), is_final=True, finalize_all=False)
    res = sch.step()[sid]
    assert fb.calls == [("alternates", 1, 4)]
    al = res.alignment
    assert al["token_ids"] == [6, 7, 8] and len(al["alternates"]) == 3
    want = ref.alternates(fb.table, 0, [6, 7, 8], [0, 2, 4], [2, 4, 6], 4)
    for k, r in enumerate(al["alternates"]):
        assert set(r) == {"id", "token", "conf", "own_rank", "alternates"}
        assert r["id"] == al["token_ids"][k] and r["token"] == TOKENS[r["id"]] and r["conf"] == al["conf"][k]
        assert r["own_rank"] == int(want[2][k])
        assert [a["id"] for a in r["alternates"]] == want[0][k].tolist()
        assert [a["token"] for a in r["alternates"]] == [TOKENS[v] for v in want[0][k]]
        assert [a["conf"] for a in r["alternates"]] == np.exp(want[1][k]).tolist()
    json.dumps(al)
    # without the option: today's call and today's alignment
    fb2 = FakeBatch()
    sch2 = StreamScheduler(fb2, TOKENS, result_format="espnet", align_final=True)
    sid = sch2.open()
    sch2.feed(sid, np.zeros(4000, np.float32), is_final=True, finalize_all=False)
    res2 = sch2.step()[sid]
    assert fb2.calls == [("align", 1)]
    assert res2.alignment == {k: v for k, v in al.items() if k != "alternates"}
    with pytest.raises(ValueError):
        StreamScheduler(FakeBatch(), TOKENS, result_format="espnet", alternates=9)


def test_the_python_lock_step_engine_has_no_alternates():
    from test_engine_spec import make_batch
    sb = make_batch("TINY", 1234, "meanstd", 3, True, n_streams=1, max_frames=64, max_tokens=32, pcm_capacity=1 << 16)
    with pytest.raises(NotImplementedError):
        StreamScheduler(sb, None, result_format="espnet", align_final=True, alternates=3)
    with pytest.raises(NotImplementedError):
        ServerLoop(StreamScheduler(sb, None, result_format="espnet"), vosk_output_format=True, token_alternates=3)


def test_vosk_alternatives_message_and_the_old_message_for_zero():
    old = _final(_loop(vosk_alignment=True)[0])
    assert len(old) == 1 and set(old[0]) == {"result", "text"}
    loop, fb = _loop(vosk_alignment=True, vosk_alternatives=3)
    assert _final(loop) == old                                   # no config: today's message
    assert _final(loop, {"max_alternatives": 0}) == old          # m = 0: today's message
    assert json.dumps(_final(loop, {"max_alternatives": 0})) == json.dumps(old)
    assert all(c == ("align", 3) for c in fb.calls)              # one alignment call per final, for the listed hypotheses
    (msg,) = _final(loop, {"max_alternatives": 3})
    assert set(msg) == {"alternatives"} and len(msg["alternatives"]) == 3
    a = msg["alternatives"]
    assert [set(e) for e in a] == [{"text", "confidence", "result"}] * 3
    assert [e["text"] for e in a] == ["w6x7 w8", "w6x9", "w10"]
    np.testing.assert_allclose([e["confidence"] for e in a], [0.5, 0.25, 0.25], rtol=0, atol=1e-15)
    assert a[0]["result"] == old[0]["result"]                    # the first alternative: the classic result's words
    assert [w["word"] for w in a[1]["result"]] == ["w6x9"] and [w["word"] for w in a[2]["result"]] == ["w10"]
    assert all(set(w) == {"conf", "start", "end", "word"} for e in a for w in e["result"])
    assert a[1]["result"][0]["conf"] == pytest.approx(0.25) and a[1]["result"][0]["start"] < a[1]["result"][0]["end"]
    (msg2,) = _final(loop, {"max_alternatives": 2})
    assert [e["text"] for e in msg2["alternatives"]] == ["w6x7 w8", "w6x9"]
    np.testing.assert_allclose([e["confidence"] for e in msg2["alternatives"]], [2 / 3, 1 / 3], rtol=0, atol=1e-15)
    (msg9,) = _final(loop, {"max_alternatives": 9})              # above N: N
    assert msg9 == msg
    # a final is repeated only once, like the classic one
    sid = loop.connect()
    loop.submit(sid, json.dumps({"config": {"max_alternatives": 1}}))
    loop.submit(sid, np.zeros(4000, np.int16))
    loop.submit(sid, '{"eof" : 1}')
    loop.submit(sid, b"")
    out = []
    while loop.pending():
        out.extend(loop.step().get(sid, []))
    assert "alternatives" in out[-2] and out[-1] == {"partial": ""}
    # a malformed request is that client's error, and the option off ignores the field
    loop.disconnect(sid)
    sid = loop.connect()
    loop.submit(sid, json.dumps({"config": {"max_alternatives": -1}}))
    assert isinstance(loop.step()[sid][0], ValueError)
    loop.disconnect(sid)
    assert _final(_loop(vosk_alignment=True)[0], {"max_alternatives": 3}) == old


def test_token_alternates_ride_on_the_word_entries():
    old = _final(_loop(vosk_alignment=True)[0])
    loop, fb = _loop(vosk_alignment=True, token_alternates=2)
    (msg,) = _final(loop)
    assert fb.calls == [("alternates", 1, 2)]
    assert msg["text"] == old[0]["text"]
    assert [{k: v for k, v in w.items() if k != "tokens"} for w in msg["result"]] == old[0]["result"]
    assert [[r["id"] for r in w["tokens"]] for w in msg["result"]] == [[6, 7], [8]]
    want = ref.alternates(fb.table, 0, [6, 7, 8], [0, 2, 4], [2, 4, 6], 2)
    recs = [r for w in msg["result"] for r in w["tokens"]]
    assert [[a["id"] for a in r["alternates"]] for r in recs] == want[0].tolist()
    assert [r["own_rank"] for r in recs] == want[2].tolist()
    # the classic per-token result (no vosk_alignment): one record per entry
    classic = _final(_loop()[0])
    (msg,) = _final(_loop(token_alternates=2)[0])
    assert [{k: v for k, v in w.items() if k != "tokens"} for w in msg["result"]] == classic[0]["result"]
    assert [[r["id"] for r in w["tokens"]] for w in msg["result"]] == [[6], [7], [8]]
    # with alternatives: the first one carries them, the others do not
    loop, fb = _loop(vosk_alternatives=2, token_alternates=2)
    (msg,) = _final(loop, {"max_alternatives": 2})
    assert fb.calls == [("alternates", 2, 2)]
    assert all("tokens" in w for w in msg["alternatives"][0]["result"])
    assert not any("tokens" in w for w in msg["alternatives"][1]["result"])
    json.dumps(msg)


def test_cli_option_implies_the_alignment():
    from speechcatcher_amd.__main__ import make_parser
    args = make_parser().parse_args(["--token-alternates", "3", "x.wav"])
    assert args.token_alternates == 3 and make_parser().parse_args(["x.wav"]).token_alternates == 0
    from speechcatcher_amd.segmenter import ALIGNMENT_KEYS, merge_paragraphs
    assert "token_alternates" in ALIGNMENT_KEYS
    seg = lambda t, r: {"start": 0.0, "end": 1.0, "text": t, "tokens": [t], "token_timestamps": [0.0],   # noqa: E731
                        "token_start": [0.0], "token_end": [1.0], "token_conf": [0.5], "token_alternates": [r]}
    _, info = merge_paragraphs([seg("a", {"id": 1}), seg("b.", {"id": 2}), seg("c", {"id": 3})])
    assert [p["token_alternates"] for p in info] == [[{"id": 1}, {"id": 2}], [{"id": 3}]]


def test_job_struct_layout_and_constants_match_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    hdr = (ROOT / "include" / "scasr.h").read_text()
    for name, val in (("SC_ALT_OK", _abi.ALT_OK), ("SC_ALT_NO_SPAN", _abi.ALT_NO_SPAN), ("SC_ALT_BAD_ROW", _abi.ALT_BAD_ROW),
                      ("SC_ALT_MAX_K", _abi.ALT_MAX_K), ("SC_ALT_MAX_JOBS", _abi.ALT_MAX_JOBS)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == val
    assert (ref.OK, ref.NO_SPAN, ref.BAD_ROW, ref.MAX_K) == (_abi.ALT_OK, _abi.ALT_NO_SPAN, _abi.ALT_BAD_ROW, _abi.ALT_MAX_K)
    assert int(re.search(r"#define SC_ABI_VERSION (\d+)", hdr).group(1)) == _abi.ABI_VERSION >= 11
    cls = _abi.AltJob
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scasr.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(sc_ctc_alt_job));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(sc_ctc_alt_job, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 88
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname
    assert "sc_ctc_alternates" in _abi.EXPORTED_SYMBOLS and "sc_alternates_hyps" in _abi.EXPORTED_SYMBOLS
