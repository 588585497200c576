"""The host-side surfaces of the CTC prefix beam search (speechcatcher_amd/ctc_beam.py; StreamScheduler(ctc_beam=...),
open(decoder="ctc")) on a stub batch: the shapes of the new results.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import ctc_beam_ref as R
from speechcatcher_amd import ctc_beam as M
from speechcatcher_amd.align import FeatureClock
from speechcatcher_amd.scheduler import CtcBeamResults, StreamScheduler

NAMES = ["<blank>", "▁he", "llo", "▁wor", "ld", "▁"] + [f"t{k}" for k in range(6, 20)]


def _table(labels, V=8, lead=6.0, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((len(labels), V)).astype(np.float32)
    for t, lab in enumerate(labels):
        x[t, lab] = x[t].max() + np.float32(lead)
    return x


def test_params_totals_backtrace_and_token_spans():
    assert M.params(None) is None and M.params(0) is None and M.params(False) is None
    assert M.params(True) == M.DEFAULT == (8, 8) and M.params(4) == (4, 8) and M.params((3, 5)) == (3, 5)
    for bad in (17, (0, 4), (4, 17)):
        with pytest.raises(ValueError):
            M.params(bad)
    assert M.total(-1.0, -np.inf) == -1.0 and M.total(-np.inf, -2.0) == -2.0
    assert M.total(np.log(0.25), np.log(0.5)) == R.lae(np.log(0.25), np.log(0.5))
    assert M.initial()["entries"] == R.initial()[3]
    # the module's backtrace and spans on the contract's run: "he llo" <blank> "wor ld"
    x = _table([0, 1, 1, 2, 0, 0, 3, 4, 4, 0])
    state, store = R.scan_table(x, 0, 4, 4)
    st = {"n_frames": state[0], "n_bad": state[1], "n_nodes": state[2], "entries": state[3]}
    hyps = M.hyps_of(st, store, 3)
    assert len(hyps) == 3 and hyps[0]["ids"] == [1, 2, 3, 4] and hyps[0]["frames"] == [1, 3, 6, 7]
    assert (hyps[0]["ids"], hyps[0]["frames"]) == R.backtrace(state[3][0], store)
    assert M.hyps_of(st, store[:3], 3) == []                         # a chain that is not stored: nothing from there on
    toks = M.token_dicts(hyps[0], names=NAMES)
    assert [(t["token"], t["start"], t["end"]) for t in toks] == [("▁he", 1, 2), ("llo", 3, 5), ("▁wor", 6, 6), ("ld", 7, 7)]
    clock = FeatureClock(400, 160)
    clock.call(16000, True)
    secs = M.token_dicts(hyps[0], clock, 4, 16000)
    assert all(a["start"] < a["end"] for a in secs) and all(a["end"] <= b["start"] + 1e-9 for a, b in zip(secs, secs[1:]))
    assert secs[0]["start"] == clock.frame_span(1, 4)[0] / 16000 and secs[1]["end"] == clock.frame_span(5, 4)[1] / 16000
    assert M.text_of(hyps[0]["ids"], NAMES) == "hello world" and M.text_of([1, 2]) == "1 2"
    words = M.words_of(hyps[0], NAMES, clock)
    assert [w["word"] for w in words] == ["hello", "world"] and words[0]["start"] == secs[0]["start"]
    assert words[0]["end"] == secs[1]["end"] and words[1]["end"] == secs[3]["end"]
    nb = M.nbest(hyps, NAMES)
    assert [e["text"] for e in nb][0] == "hello world" and abs(sum(e["conf"] for e in nb) - 1.0) < 1e-12
    assert nb[0]["conf"] > 0.9 and [e["score"] for e in nb] == sorted((e["score"] for e in nb), reverse=True)
    assert nb[0]["score"] == R.total(state[3][0]) and M.nbest([]) == []


class StubWithoutModes:
    """what StreamScheduler asks of a batch, with a beam that follows the contract over canned CTC rows: every pushed
    chunk of n samples stands for n // 640 further frames of the stream's table.  This one has no decoder-free streams."""

    def __init__(self, tables, blank=0):
        self.S = len(tables)
        self.cfg = SimpleNamespace(win_length=400, hop_length=160, subsample=4, sample_rate=16000, sos_id=1)
        self.tables, self.blank = tables, blank
        self.beam = None
        self.mode = ["full"] * self.S
        self.calls = []
        self.reset_all()

    def reset_all(self):
        self.state = [(R.initial(), []) for _ in range(self.S)]
        self.t = [0] * self.S

    def reset(self, s):
        self.state[s], self.t[s] = (R.initial(), []), 0
        self.calls.append(("reset", s))

    def set_ctc_beam(self, beam, candidates):
        self.beam = (beam, candidates)
        self.reset_all()

    def push(self, items, isolate_faults=False):
        has = {}
        for s, pcm, fin in items:
            n = len(pcm) // 640
            has[s] = True
            if self.beam is None:                                    # the option is off: nothing is searched
                self.t[s] += n
                continue
            st, store = self.state[s]
            rws = R.rows(self.tables[s][self.t[s]:self.t[s] + n], self.blank, self.beam[1])
            self.state[s] = (R.scan(st, rws, store, 1 << 30, self.beam[0]), store)
            self.t[s] += n
            has[s] = True
        return has

    def hypotheses(self, s):
        # a full stream: a canned search result that ends in <eos> (1023); a decoder-free one: the initial hypothesis
        ys = [1] if self.mode[s] == "ctc" else [1, 7, 9, 1023]
        return [{"yseq": ys, "xpos": list(range(len(ys))), "score": 0.0, "score_dec": 0.0, "score_ctc": 0.0}]

    def ctc_beam_hyps(self, streams, nbest=1, max_len=None):
        out = {}
        for s in streams:
            st, store = self.state[s]
            out[s] = [{"ids": R.backtrace(e, store)[0], "frames": R.backtrace(e, store)[1], "pb": e[4], "pnb": e[5]}
                      for e in st[3][:nbest]]
        return out


class StubBatch(StubWithoutModes):
    def set_decoder(self, s, decoder):
        if self.t[s]:
            raise RuntimeError("the stream has buffered audio since its last reset")
        self.mode[s] = decoder
        self.calls.append(("set_decoder", s, decoder))


LABELS = [[0, 1, 1, 2, 0, 0, 3, 4, 4, 0], [0, 3, 3, 4, 0, 0, 1, 1, 2, 0]]


def _feed(sch, sid, frames, final=False):
    sch.feed(sid, np.zeros(640 * frames, np.float32), final)


def test_scheduler_replies_carry_the_nbest_and_decoder_free_sessions_are_served_from_it():
    batch = StubBatch([_table(lab, seed=k) for k, lab in enumerate(LABELS)])
    with pytest.raises(ValueError):
        StreamScheduler(batch, NAMES).open(decoder="ctc")            # needs the option
    sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4))
    assert sch.ctc_beam == (4, 4) and batch.beam == (4, 4)
    with pytest.raises(ValueError):
        sch.open(decoder="greedy")
    full, free = sch.open(), sch.open(decoder="ctc")
    assert (sch.decoder(full), sch.decoder(free)) == ("full", "ctc") and ("set_decoder", 1, "ctc") in batch.calls
    _feed(sch, full, 5)
    _feed(sch, free, 5)
    out = sch.step()
    assert all(isinstance(out[sid], CtcBeamResults) for sid in (full, free))
    # partials: the full session's results are the search's (the reference's partial of an <eos> hypothesis: no text);
    # the decoder-free session's are the beam's best so far
    assert [r[0] for r in out[full]] == [""] and out[free][0][:3] == ("wor ld".replace(" ", ""), ["▁wor", "ld"], [3, 4])
    for sid, lab in ((full, [1, 2]), (free, [3, 4])):
        nb = out[sid].ctc_nbest
        assert len(nb) == 4 and nb[0]["ids"] == lab and abs(sum(e["conf"] for e in nb) - 1.0) < 1e-12
        t = nb[0]["tokens"]
        assert [d["token"] for d in t] == [NAMES[k] for k in lab] and all(d["start_s"] < d["end_s"] for d in t)
        assert t[0]["start"] == 1 and t[0]["end"] == 2 and t[1]["start"] == 3
    _feed(sch, full, 5, True)
    _feed(sch, free, 5, True)
    out = sch.step()
    assert out[full][0][0] == "t7t9" and out[full].ctc_nbest[0]["text"] == "hello world"
    assert out[free][0][0] == out[free].ctc_nbest[0]["text"] == "world hello"
    assert out[free][0][2] == [3, 4, 1, 2] and ("reset", 1) in batch.calls
    # the slot goes back to the full decoder for a session that does not ask
    sch.close(free)
    again = sch.open()
    assert sch.decoder(again) == "full" and batch.calls[-1] == ("set_decoder", 1, "full")
    # espnet format: positions are the frames of first emission; an empty prefix is no result
    batch2 = StubBatch([_table([0, 0, 0, 1, 1], seed=3)])
    sch2 = StreamScheduler(batch2, None, result_format="espnet", ctc_beam=2)
    assert sch2.ctc_beam == (2, 8)
    sid = sch2.open(decoder="ctc")
    _feed(sch2, sid, 3)
    out = sch2.step()
    assert list(out[sid]) == [] and out[sid].ctc_nbest[0]["ids"] == [] and out[sid].ctc_nbest[0]["text"] == ""
    _feed(sch2, sid, 2)
    out = sch2.step()
    text, toks, ids, pos, hyp = out[sid][0]
    # (the frame of a token is the frame at which its prefix entered the beam: at the latest where the path emits it)
    assert (text, toks, ids) == ("1", ["1"], [1]) and hyp is out[sid].ctc_nbest[0]
    assert pos == [hyp["tokens"][0]["start"]] and 0 <= pos[0] <= 3


def test_a_batch_without_the_search_or_without_decoder_free_streams_says_so():
    class Plain:
        S = 1
        cfg = SimpleNamespace(win_length=400, hop_length=160, subsample=4, sample_rate=16000)

        def reset(self, s):
            pass

    with pytest.raises(NotImplementedError):
        StreamScheduler(Plain(), None, ctc_beam=8)

    sch = StreamScheduler(StubWithoutModes([_table(LABELS[0])]), None, ctc_beam=4)
    with pytest.raises(NotImplementedError):
        sch.open(decoder="ctc")
    assert sch.open() == 0


# ---- ServerLoop: the Vosk config key, partials, finals and alternatives of a decoder-free connection ---------------------
def _loop(**kw):
    from speechcatcher_amd.server_session import ServerLoop
    batch = StubBatch([_table(lab, seed=k) for k, lab in enumerate(LABELS)])
    sch = StreamScheduler(batch, NAMES, result_format="espnet")
    return ServerLoop(sch, vosk_output_format=True, **kw), batch


def _say(loop, sid, message):
    loop.submit(sid, message)
    out = loop.step().get(sid, [])
    assert len(out) == 1, out
    return out[0]


def _pcm(frames):
    return np.zeros(640 * frames, np.int16)


def test_server_connection_with_decoder_ctc_is_served_from_the_beam():
    loop, batch = _loop(ctc_beam=(4, 4))
    assert loop.sch.ctc_beam == (4, 4)
    full, free = loop.connect(), loop.connect()
    assert _say(loop, free, '{"config": {"decoder": "ctc", "max_alternatives": 9}}') == {"partial": ""}
    assert loop.sch.decoder(free) == "ctc" and ("set_decoder", 1, "ctc") in batch.calls
    assert loop.sessions[free].max_alternatives == 4                 # at most the beam's B, without vosk_alternatives
    # partials are the beam's best so far; the other connection keeps the search's
    assert _say(loop, free, _pcm(5)) == {"partial": "world"}
    assert _say(loop, full, _pcm(5)) == {"partial": ""}
    assert _say(loop, free, _pcm(5)) == {"partial": "world hello"}
    # the decoder can only be chosen before the first audio; unknown values and bad counts are this client's error
    for bad in ('{"config": {"decoder": "full"}}', '{"config": {"decoder": "greedy"}}',
                '{"config": {"max_alternatives": -1}}'):
        assert isinstance(_say(loop, free, bad), ValueError), bad
    assert loop.sch.decoder(free) == "ctc"
    final = _say(loop, free, '{"eof" : 1}')
    alts = final["alternatives"]
    assert 2 <= len(alts) <= 4 and alts[0]["text"] == "world hello" and all(a["text"] for a in alts)
    assert abs(sum(a["confidence"] for a in alts) - 1.0) < 1e-9 and alts[0]["confidence"] > 0.9
    assert [a["confidence"] for a in alts] == sorted((a["confidence"] for a in alts), reverse=True)
    # one entry per token at its tree frame (no vosk_alignment here): the reference's 24 frames a second
    assert [w["word"] for w in alts[0]["result"]] == [" wor", "ld", " he", "llo"]
    # (the frame at which a token's prefix entered the beam: at the latest where the path emits it - 1, 3, 6, 8)
    starts = [round(w["start"] * 24) for w in alts[0]["result"]]
    assert starts[:2] == [1, 3] and 3 < starts[2] <= 6 < starts[3] <= 8
    full_final = _say(loop, full, '{"eof" : 1}')
    assert full_final["text"] == "t7t9" and "alternatives" not in full_final
    # the utterance was reset: the next one starts over, still decoder-free
    assert _say(loop, free, _pcm(5)) == {"partial": "world"}


def test_server_classic_final_words_from_the_tree_frames_and_the_key_without_the_option():
    loop, _ = _loop(ctc_beam=4, vosk_alignment=True)
    assert loop.sch.align_final and loop.sch.align_nbest >= 4
    sid = loop.connect()
    _say(loop, sid, '{"config": {"decoder": "ctc"}}')
    _say(loop, sid, _pcm(10))
    final = _say(loop, sid, '{"eof" : 1}')
    assert final["text"] == "hello world" and [w["word"] for w in final["result"]] == ["hello", "world"]   # (slot 0)
    w0, w1 = final["result"]
    assert 0.0 <= w0["start"] < w0["end"] <= w1["start"] < w1["end"] and w0["conf"] == w1["conf"] == 1.0
    # "full" before any audio goes back; alternatives of a decoder-free connection with word times
    sid2 = loop.connect()
    _say(loop, sid2, '{"config": {"decoder": "ctc", "max_alternatives": 2}}')
    _say(loop, sid2, '{"config": {"decoder": "full"}}')
    assert loop.sch.decoder(sid2) == "full" and loop.sessions[sid2].max_alternatives == 0
    loop.disconnect(sid2)
    loop.disconnect(sid)
    sid3 = loop.connect()
    _say(loop, sid3, '{"config": {"decoder": "ctc", "max_alternatives": 2}}')
    _say(loop, sid3, _pcm(10))
    alts = _say(loop, sid3, '{"eof" : 1}')["alternatives"]
    assert len(alts) == 2 and [w["word"] for w in alts[0]["result"]] == ["world", "hello"]   # (slot 1)
    assert all(w["start"] < w["end"] for a in alts for w in a["result"])
    # without the option the key is refused, and strict_reference does not take the option
    plain, _ = _loop()
    sid = plain.connect()
    assert isinstance(_say(plain, sid, '{"config": {"decoder": "ctc"}}'), ValueError)
    assert _say(plain, sid, '{"config": {"decoder": "full"}}') == {"partial": ""}
    with pytest.raises(ValueError):
        _loop(ctc_beam=4, strict_reference=True)


def test_align_final_of_a_decoder_free_session_is_the_tree_and_alternates_are_refused():
    batch = StubBatch([_table(LABELS[0])])
    sch = StreamScheduler(batch, NAMES, result_format="espnet", ctc_beam=(4, 4), align_final=True, align_nbest=2)
    sid = sch.open(decoder="ctc")
    _feed(sch, sid, 10, True)
    res = sch.step()[sid]
    al, best = res.alignment, res.ctc_nbest[0]
    assert al["source"] == "ctc_beam" and al["token_ids"] == [1, 2, 3, 4] == res[0][2]
    assert al["start_s"] == [t["start_s"] for t in best["tokens"]] and al["end_s"] == [t["end_s"] for t in best["tokens"]]
    assert al["conf"] == [1.0] * 4 and len(al["nbest"]) == 2 and al["nbest"][1]["token_ids"] == res[1][2]
    sch.alternates = 3                                               # (the C++ engine's option; a stub has no alternates call)
    with pytest.raises(ValueError):
        sch.open(decoder="ctc")


# ---- the CLI: --ctc-beam, --ctc-only ------------------------------------------------------------------------------------
def test_cli_flags_and_the_segment_loop():
    from speechcatcher_amd.__main__ import make_parser
    from speechcatcher_amd.scheduler import recognize_segments
    from speechcatcher_amd.segmenter import merge_paragraphs
    args = make_parser().parse_args(["--ctc-only", "--ctc-beam", "4", "a.wav"])
    assert args.ctc_only and args.ctc_beam == 4
    args = make_parser().parse_args(["a.wav"])
    assert not args.ctc_only and args.ctc_beam == 0
    speech = np.zeros(640 * 10, np.float32)
    tables = [_table(lab, seed=k) for k, lab in enumerate(LABELS)]
    # --ctc-only: the text is the beam's best, token_timestamps its tree frames, ctc_nbest beside it
    out = recognize_segments(StubBatch(tables), speech, [(0, 6400)], chunk_length=3200, token_list=NAMES, ctc_only=True,
                             token_alignment=True)[0]
    assert out["text"] == "hello world" and out["token_ids"] == [1, 2, 3, 4]
    stamps = [round(t * 24) for t in out["token_timestamps"]]        # (where each prefix entered the beam: at the latest
    assert stamps == sorted(stamps) and all(a <= b for a, b in zip(stamps, [1, 3, 6, 7]))   # where the path emits it)
    assert len(out["ctc_nbest"]) == 1 and out["ctc_nbest"][0][0]["text"] == "hello world"
    assert set(out["ctc_nbest"][0][0]) == {"text", "score", "conf"} and len(out["ctc_nbest"][0]) == 8
    assert out["token_conf"] == [1.0] * 4 and all(a < b for a, b in zip(out["token_start"], out["token_end"]))
    # --ctc-beam alone: the search's transcript, with the n-best of the beam added
    out = recognize_segments(StubBatch(tables), speech, [(0, 6400)], chunk_length=3200, token_list=NAMES, ctc_beam=4)[0]
    assert out["text"] == "t7t9" and [e["text"] for e in out["ctc_nbest"][0]][0] == "hello world"
    assert len(out["ctc_nbest"][0]) == 4
    plain = recognize_segments(StubBatch(tables), speech, [(0, 6400)], chunk_length=3200, token_list=NAMES)[0]
    assert "ctc_nbest" not in plain
    with pytest.raises(ValueError):
        recognize_segments(StubBatch(tables), speech, [(0, 6400)], token_list=NAMES, ctc_only=True, token_alternates=2)
    # paragraphs append the segments' lists
    seg = {"start": 0.0, "end": 1.0, "text": "a", "tokens": ["a"], "token_timestamps": [0.0], "ctc_nbest": [[{"text": "a"}]]}
    _, info = merge_paragraphs([seg, dict(seg, start=1.0, end=2.0)])
    assert len(info) == 1 and len(info[0]["ctc_nbest"]) == 2
