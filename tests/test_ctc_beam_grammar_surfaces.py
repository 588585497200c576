"""The host-side surfaces of the grammar-constrained CTC beam (StreamScheduler.open(grammar=...) / set_grammar, the Vosk
``phrase_list`` of ServerLoop, the CLI's --ctc-grammar, the Python engine's refusal) on a stub batch whose beam follows the
contract (tests/ctc_beam_grammar_ref.py).  No GPU."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import ctc_beam_grammar_ref as G
import ctc_beam_ref as R
from speechcatcher_amd import grammar
from speechcatcher_amd.scheduler import CtcBeamResults, StreamScheduler
from test_ctc_beam_surfaces import LABELS, NAMES, StubBatch, _feed, _pcm, _say, _table

V = 8


class GrStub(StubBatch):
    """StubBatch with grammars: a stream that names one follows the grammar contract"""

    def __init__(self, tables):
        self.gr = {}                     # stream -> (handle, Grammar)
        self.alive = []                  # device copies that exist
        self.lm_attached = False
        super().__init__(tables)
        self.cfg = SimpleNamespace(**vars(self.cfg), vocab_size=V, blank_id=0)

    def _initial(self, s):
        return (G.initial(self.gr[s][1]), []) if s in self.gr else (R.initial(), [])

    def reset_all(self):
        self.t = [0] * self.S
        self.state = [self._initial(s) for s in range(self.S)]

    def reset(self, s):
        self.state[s], self.t[s] = self._initial(s), 0
        self.calls.append(("reset", s))

    def grammar(self, blob):
        walk = grammar.Grammar(blob)     # (ValueError for what is no blob)
        handle = SimpleNamespace(blob=bytes(blob), walk=walk)
        self.alive.append(handle)
        self.calls.append(("grammar", len(blob)))
        return handle

    def release_grammar(self, handle):
        if any(h is handle for h, _ in self.gr.values()):
            raise RuntimeError("the grammar is still in use")
        self.alive.remove(handle)
        self.calls.append(("release_grammar", len(handle.blob)))

    def set_stream_grammar(self, s, handle=None):
        if self.beam is None:
            raise RuntimeError("the beam option is off")
        if self.t[s]:
            raise RuntimeError("the stream has buffered audio since its last reset")
        if handle is None:
            self.gr.pop(s, None)
        else:
            self.gr[s] = (handle, handle.walk)
        self.state[s] = self._initial(s)
        self.calls.append(("set_stream_grammar", s, None if handle is None else len(handle.blob)))

    def push(self, items, isolate_faults=False):
        has = {}
        for item in items:
            s, pcm, fin = item
            if s not in self.gr:
                has.update(super().push([item], isolate_faults))
                continue
            n = len(pcm) // 640
            st, store = self.state[s]
            rws = G.rows(self.tables[s][self.t[s]:self.t[s] + n])
            self.state[s] = (G.scan(st, rws, store, 1 << 30, self.beam[0], self.beam[1], self.gr[s][1], self.blank), store)
            self.t[s] += n
            has[s] = True
        return has

    def ctc_beam_hyps_grammar(self, streams, nbest=1):
        out = {}
        for s in streams:
            if s not in self.gr:
                out[s] = [(-1, None)] * nbest
                continue
            gs = self.state[s][0][4][:nbest]
            out[s] = [(g, self.gr[s][1].accepts(g)) for g in gs] + [(-1, None)] * (nbest - len(gs))
        return out


def _tables():
    return [_table(lab, seed=k) for k, lab in enumerate(LABELS)]     # "hello world" and "world hello"


def test_scheduler_compiles_caches_and_counts_the_grammars_of_its_sessions(tmp_path):
    menu = ["hello", "world"]
    blob = grammar.compile([[1, 2], [3, 4]], V, 0)
    with pytest.raises(ValueError, match="ctc_beam"):
        StreamScheduler(GrStub(_tables()), NAMES).open(grammar=menu)
    with pytest.raises(NotImplementedError):
        StreamScheduler(StubBatch(_tables()), NAMES, ctc_beam=4).open(decoder="ctc", grammar=blob)
    batch = GrStub(_tables() * 2)
    sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4))
    # phrases as strings, as id lists, as a blob, as a .scgr file and as a text file: one grammar, one device copy
    (tmp_path / "menu.scgr").write_bytes(blob)
    (tmp_path / "menu.txt").write_text("hello\n\nworld\n", encoding="utf-8")
    a = sch.open(decoder="ctc", grammar=menu)
    b = sch.open(decoder="ctc", grammar=[[3, 4], [1, 2]])
    c = sch.open(grammar=blob)
    d = sch.open()
    assert len(batch.alive) == 1 and batch.alive[0].blob == blob and list(sch._gr_cache.values())[0]["uses"] == 3
    sch.set_grammar(d, str(tmp_path / "menu.scgr"))
    sch.set_grammar(d, str(tmp_path / "menu.txt"))
    assert len(batch.alive) == 1 and list(sch._gr_cache.values())[0]["uses"] == 4
    assert sch.grammar(a).accepts(sch.grammar(a).walk([1, 2, 3, 4])) and sch.grammar(d) is sch.grammar(a)
    # another menu: a second copy; back to none
    sch.set_grammar(d, ["held"])
    assert len(batch.alive) == 2 and sorted(e["uses"] for e in sch._gr_cache.values()) == [1, 3]
    sch.set_grammar(d, None)
    assert len(batch.alive) == 1 and sch.grammar(d) is None and batch.calls[-1][0] == "release_grammar"
    # what cannot be compiled is a ValueError and leaves nothing behind
    for bad in (["hello", "xyz"], [[1, 0]], [[1, 99]], [], [[]], b"SCGR-but-not-a-blob"):
        with pytest.raises(ValueError):
            sch.set_grammar(d, bad)
    assert len(batch.alive) == 1 and len(sch._gr_cache) == 1
    with pytest.raises(ValueError, match="token list"):
        StreamScheduler(GrStub(_tables()), None, ctc_beam=4).open(grammar=["hello"])
    # only before the session's first audio
    _feed(sch, a, 5)
    sch.step()
    with pytest.raises(ValueError, match="before its first audio"):
        sch.set_grammar(a, None)
    # the last session that closes frees the device copy
    for k, sid in enumerate((a, b, c)):
        assert len(batch.alive) == 1
        sch.close(sid)
    assert batch.alive == [] and sch._gr_cache == {} and batch.gr == {}
    # a slot's next session starts without a grammar unless it asks
    e = sch.open(decoder="ctc")
    assert sch.grammar(e) is None


def test_final_results_come_complete_entries_first_and_partials_keep_the_beams_order():
    batch = GrStub(_tables())
    sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4), align_final=True, result_format="espnet")
    free = sch.open(decoder="ctc", grammar=["hello world", "hello"], sample_rate=16000)
    plain = sch.open(decoder="ctc")
    # a partial in mid-phrase: the beam's order, "complete" says which entries are whole phrases
    _feed(sch, free, 7)
    _feed(sch, plain, 7)
    out = sch.step()
    nb = out[free].ctc_nbest
    assert isinstance(out[free], CtcBeamResults) and all("complete" in e for e in nb)
    assert [e["score"] for e in nb] == sorted((e["score"] for e in nb), reverse=True)
    assert out[free].grammar_complete == nb[0]["complete"]
    assert "complete" not in out[plain].ctc_nbest[0] and out[plain].grammar_complete is None
    walk = sch.grammar(free)
    for e in nb:
        assert walk.walk(e["ids"]) >= 0 and e["complete"] == walk.accepts(walk.walk(e["ids"]))
    _feed(sch, free, 3, True)
    _feed(sch, plain, 3, True)
    out = sch.step()
    nb = out[free].ctc_nbest
    flags = [e["complete"] for e in nb]
    assert flags == sorted(flags, reverse=True) and flags[0] and not flags[-1]
    for group in (True, False):                                      # each group in beam order
        sc = [e["score"] for e in nb if e["complete"] == group]
        assert sc == sorted(sc, reverse=True)
    assert out[free].grammar_complete is True and out[free][0][0] == nb[0]["text"] == "hello world"
    # align_final keeps working: the tree's times of the entry reported
    al = out[free].alignment
    assert al["source"] == "ctc_beam" and al["token_ids"] == out[free][0][2] == [1, 2, 3, 4]
    # the other session is untouched by its neighbour's grammar: the plain beam's best of its table
    assert out[plain][0][0] == "world hello" and out[plain].grammar_complete is None


def test_a_grammar_that_the_audio_does_not_finish_reports_nothing_complete():
    batch = GrStub(_tables())
    sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4), result_format="espnet")
    sid = sch.open(decoder="ctc", grammar=[[1, 2, 3, 4, 5, 5, 5, 5, 5, 5, 5, 5, 5]])   # longer than the audio has frames
    _feed(sch, sid, 10, True)
    res = sch.step()[sid]
    assert res.grammar_complete is False and not any(e["complete"] for e in res.ctc_nbest)
    assert [e["score"] for e in res.ctc_nbest] == sorted((e["score"] for e in res.ctc_nbest), reverse=True)


def _loop(**kw):
    from speechcatcher_amd.server_session import ServerLoop
    batch = GrStub(_tables())
    return ServerLoop(StreamScheduler(batch, NAMES, result_format="espnet"), vosk_output_format=True, **kw), batch


def test_vosk_phrase_list_sets_the_sessions_grammar_and_the_final_is_the_best_complete_entry():
    loop, batch = _loop(ctc_beam=(4, 4))
    sid, other = loop.connect(), loop.connect()
    cfg = {"config": {"decoder": "ctc", "phrase_list": ["hello world", "hello", "[unk]"]}}
    assert _say(loop, sid, json.dumps(cfg)) == {"partial": "", "ignored": ["[unk]"]}
    assert _say(loop, other, '{"config": {"decoder": "ctc", "phrase_list": ["world hello"]}}') == {"partial": ""}
    assert loop.sch.grammar(sid).accepts(loop.sch.grammar(sid).walk([1, 2])) and len(batch.alive) == 2
    assert _say(loop, sid, _pcm(10))["partial"].startswith("hello")
    final = _say(loop, sid, '{"eof" : 1}')
    assert final["text"] == "hello world" and "incomplete" not in final and "alternatives" not in final
    # the bad configs are this client's error, and change nothing: after audio, on a FULL connection, not a list of
    # strings, nothing left, a phrase that cannot be tokenised
    full = loop.connect() if len(loop.sessions) < batch.S else None
    assert full is None                                              # (two slots: both are taken)
    assert isinstance(_say(loop, other, _pcm(3)), dict)
    assert isinstance(_say(loop, other, '{"config": {"phrase_list": ["hello"]}}'), ValueError)      # after audio
    assert loop.sch.grammar(other).walk([3, 4, 1, 2]) >= 0
    loop.disconnect(sid)
    fresh = loop.connect()
    for bad in ('{"config": {"phrase_list": ["hello"]}}',                                            # a FULL connection
                '{"config": {"decoder": "ctc", "phrase_list": "hello"}}',
                '{"config": {"decoder": "ctc", "phrase_list": ["hello", 3]}}',
                '{"config": {"decoder": "ctc", "phrase_list": ["[unk]"]}}',
                '{"config": {"decoder": "ctc", "phrase_list": []}}',
                '{"config": {"decoder": "ctc", "phrase_list": ["hello", "qqq"]}}'):
        assert isinstance(_say(loop, fresh, bad), ValueError), bad
        assert loop.sch.grammar(fresh) is None and loop.sch.decoder(fresh) == "full", bad
    assert len(batch.alive) == 1                                     # (the menu of `other`)


def test_vosk_final_without_a_complete_entry_and_alternatives_with_complete_first():
    loop, batch = _loop(ctc_beam=(4, 4))
    sid = loop.connect()
    _say(loop, sid, json.dumps({"config": {"decoder": "ctc", "phrase_list": ["hello world hello world hello"]}}))
    _say(loop, sid, _pcm(10))
    final = _say(loop, sid, '{"eof" : 1}')
    assert final["text"] == "" and final["result"] == [] and final["incomplete"].startswith("hello")
    loop, batch = _loop(ctc_beam=(4, 4))
    sid = loop.connect()
    _say(loop, sid, json.dumps({"config": {"decoder": "ctc", "max_alternatives": 4, "phrase_list": ["hello world", "hello"]}}))
    _say(loop, sid, _pcm(10))
    alts = _say(loop, sid, '{"eof" : 1}')["alternatives"]
    flags = [a["complete"] for a in alts]
    assert alts[0]["text"] == "hello world" and flags[0] and flags == sorted(flags, reverse=True)
    assert all(set(a["text"].split()) <= {"hello", "world"} for a in alts if a["complete"])   # (phrases may follow each other)
    assert any(not f for f in flags)


def test_the_cli_takes_the_grammar_and_refuses_it_without_the_beam_or_with_a_model(tmp_path):
    from speechcatcher_amd.__main__ import make_parser, recognize_file
    from speechcatcher_amd.scheduler import recognize_segments
    args = make_parser().parse_args(["--ctc-only", "--ctc-grammar", "menu.scgr", "a.wav"])
    assert args.ctc_grammar == "menu.scgr" and args.ctc_only
    assert make_parser().parse_args(["a.wav"]).ctc_grammar == ""
    with pytest.raises(SystemExit, match="--ctc-beam or --ctc-only"):
        recognize_file(None, "a.wav", ctc_grammar="menu.scgr")
    with pytest.raises(SystemExit, match="together"):
        recognize_file(None, "a.wav", ctc_only=True, ctc_grammar="menu.scgr", ctc_lm="m.sclm")
    with pytest.raises(SystemExit, match="does not exist"):
        recognize_file(None, "a.wav", ctc_only=True, ctc_grammar=str(tmp_path / "missing.scgr"))
    # the segment loop hands it to every session: a text file of phrases
    path = tmp_path / "menu.txt"
    path.write_text("world hello\nhello\n", encoding="utf-8")
    speech = np.zeros(640 * 10, np.float32)
    with pytest.raises(ValueError, match="ctc_beam or ctc_only"):
        recognize_segments(GrStub(_tables()), speech, [(0, 6400)], token_list=NAMES, ctc_grammar=str(path))
    with pytest.raises(ValueError, match="together"):
        recognize_segments(GrStub(_tables()), speech, [(0, 6400)], token_list=NAMES, ctc_only=True, ctc_grammar=str(path),
                           ctc_lm=b"x")
    batch = GrStub(_tables())
    out = recognize_segments(batch, speech, [(0, 6400)], chunk_length=3200, token_list=NAMES, ctc_only=True,
                             ctc_grammar=str(path))[0]
    # table 0 says "hello world", which the menu does not hold: the answer is a phrase or a sequence of phrases
    walk = grammar.Grammar(grammar.compile([[3, 4, 1, 2], [1, 2]], V, 0))
    assert out["text"] != "hello world" and walk.accepts(walk.walk(out["token_ids"])) and out["token_ids"][:2] == [1, 2]
    nb = out["ctc_nbest"][0]
    assert nb[0]["complete"] and set(nb[0]) == {"text", "score", "conf", "complete"}
    assert batch.alive == [] and ("release_grammar", len(grammar.compile([[3, 4, 1, 2], [1, 2]], V, 0))) in batch.calls


def test_the_python_engine_refuses_the_option_with_a_clear_error():
    from speechcatcher_amd.engine import EngineError, StreamBatch
    eng = StreamBatch.__new__(StreamBatch)                           # (the methods need nothing of a built batch)
    eng.set_stream_grammar(0, None)
    with pytest.raises(EngineError, match="native engine"):
        eng.grammar(b"blob")
    with pytest.raises(EngineError, match="native engine"):
        eng.set_stream_grammar(0, object())
    sch = StreamScheduler.__new__(StreamScheduler)
    sch.ctc_beam, sch.ctc_lm, sch.batch, sch.token_list, sch._gr_cache = (4, 4), None, eng, NAMES, {}
    eng.cfg = SimpleNamespace(vocab_size=V, blank_id=0)
    with pytest.raises(ValueError, match="native engine"):         # (the scheduler hands the engine's words on)
        sch._grammar_key([[1, 2]])
