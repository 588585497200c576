"""The host-side surfaces of the language model fusion (StreamScheduler(ctc_beam=..., ctc_lm=...), ServerLoop(ctc_lm=...),
the CLI's --ctc-lm / --lm-weight / --word-bonus, speechcatcher_amd.ctc_beam.nbest with a model's side, the Python engine's
refusal) on a stub batch whose beam follows the fused contract (tests/ctc_beam_lm_ref.py).  No GPU."""
import numpy as np
import pytest

import ctc_beam_lm_ref as L
import ctc_beam_ref as R
import ngram_ref as NR
from speechcatcher_amd import ctc_beam as M
from speechcatcher_amd import ngram
from speechcatcher_amd.scheduler import CtcBeamResults, StreamScheduler
from test_ctc_beam_surfaces import NAMES, StubBatch, _feed, _pcm, _say

V = 8


def _near_tie(first, second, margin=1e-3):
    """label path 1, blank, then `first` a hair ahead of `second` for two frames, blank"""
    x = np.full((6, V), -6.0, np.float32)
    x[0:2, 1] = 4.0
    x[2, 0] = 4.0
    x[3:5, first] = 4.0
    x[3:5, second] = 4.0 - margin
    x[5, 0] = 4.0
    return x


def _model():
    """has seen "he ld" (1 4) often and "he llo" (1 2) never"""
    return NR.estimate([[1, 4]] * 30 + [[2, 1], [3, 2], [4, 3]], V, 2)


class LmStub(StubBatch):
    """StubBatch whose beam follows the fused contract once a model is attached"""

    def __init__(self, tables):
        self.lm = None
        super().__init__(tables)

    def reset_all(self):
        super().reset_all()
        if getattr(self, "lm", None) is not None:
            self.state = [(L.initial(self.lm[0]), []) for _ in range(self.S)]

    def reset(self, s):
        super().reset(s)
        if self.lm is not None:
            self.state[s] = (L.initial(self.lm[0]), [])

    def set_ctc_beam_lm(self, model=None, alpha=0.5, beta=0.0):
        if self.beam is None:
            raise RuntimeError("the beam option is off")
        self.lm = None if model is None else (ngram.Blob(bytes(model)), float(alpha), float(beta))
        self.calls.append(("set_ctc_beam_lm", None if model is None else len(model), alpha, beta))
        self.reset_all()

    def push(self, items, isolate_faults=False):
        if self.lm is None:
            return super().push(items, isolate_faults)
        has = {}
        for s, pcm, fin in items:
            n = len(pcm) // 640
            st, store = self.state[s]
            rws = R.rows(self.tables[s][self.t[s]:self.t[s] + n], self.blank, self.beam[1])
            self.state[s] = (L.scan(st, rws, store, 1 << 30, self.beam[0], *self.lm), store)
            self.t[s] += n
            has[s] = True
        return has

    def ctc_beam_lm(self, streams, nbest=16):
        out = []
        for s in streams:
            st = self.state[s][0]
            out.append({"lm": [sd[0] for sd in st[4][:nbest]], "ctx": [sd[1] for sd in st[4][:nbest]],
                        "fused": [L.fused(e, sd, *self.lm[1:]) for e, sd in zip(st[3][:nbest], st[4][:nbest])]})
        return out


def test_scheduler_attaches_the_model_and_the_nbest_carries_lm_and_the_fused_score(tmp_path):
    blob = ngram.pack(_model(), V, 2)
    path = tmp_path / "m.sclm"
    path.write_bytes(blob)
    tables = [_near_tie(2, 4), _near_tie(2, 4)]
    with pytest.raises(ValueError, match="ctc_beam"):
        StreamScheduler(LmStub(tables), NAMES, ctc_lm=blob)          # needs the beam option
    with pytest.raises(NotImplementedError):
        StreamScheduler(StubBatch(tables), NAMES, ctc_beam=4, ctc_lm=blob)   # a batch without fusion says so
    # without a model: the entries are as they were
    plain = StreamScheduler(LmStub(tables), NAMES, ctc_beam=(4, 4))
    sid = plain.open(decoder="ctc")
    _feed(plain, sid, 6, True)
    out = plain.step()[sid]
    assert out.ctc_nbest[0]["ids"] == [1, 2] and set(out.ctc_nbest[0]) == {"text", "ids", "score", "conf", "tokens"}
    # with one, from a path and from bytes: the best changes, the entries gain "lm" (and the acoustic score beside the fused)
    for source in (str(path), blob):
        batch = LmStub(tables)
        sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4), ctc_lm=source, lm_weight=0.5, word_bonus=0.25)
        assert sch.ctc_lm == (0.5, 0.25) and batch.calls[-1] == ("set_ctc_beam_lm", len(blob), 0.5, 0.25)
        sid = sch.open(decoder="ctc")
        _feed(sch, sid, 6, True)
        res = sch.step()[sid]
        assert isinstance(res, CtcBeamResults) and res[0][0] == "held" and res[0][2] == [1, 4]
        nb = res.ctc_nbest
        assert nb[0]["ids"] == [1, 4] and [1, 2] in [e["ids"] for e in nb[1:]]
        model = _model()
        for e in nb:
            assert e["lm"] == NR.sequence(model, 2, e["ids"])
            assert e["score"] == float(e["ctc_score"] + (float(0.5 * e["lm"]) + float(0.25 * len(e["ids"]))))
        assert [e["score"] for e in nb] == sorted((e["score"] for e in nb), reverse=True)
        assert abs(sum(e["conf"] for e in nb) - 1.0) < 1e-12
        second = next(e for e in nb if e["ids"] == [1, 2])
        assert second["ctc_score"] > nb[0]["ctc_score"] and nb[0]["conf"] > second["conf"]   # conf follows the fused totals
    sch.enable_ctc_lm(None)
    assert sch.ctc_lm is None and batch.calls[-1][:2] == ("set_ctc_beam_lm", None)


def test_nbest_without_a_side_is_unchanged_and_with_one_ranks_by_the_fused_totals():
    hyps = [{"ids": [1, 2], "frames": [0, 3], "pb": -0.5, "pnb": -2.0}, {"ids": [1, 4], "frames": [0, 3], "pb": -1.0, "pnb": -3.0}]
    base = M.nbest(hyps, NAMES)
    assert [set(e) for e in base] == [{"text", "ids", "score", "conf", "tokens"}] * 2 and base[0]["conf"] > base[1]["conf"]
    side = {"lm": [-9.0, -1.0], "fused": [M.total(-0.5, -2.0) - 4.5, M.total(-1.0, -3.0) - 0.5]}
    got = M.nbest(hyps, NAMES, side=side)
    assert [e["lm"] for e in got] == [-9.0, -1.0] and [e["score"] for e in got] == side["fused"]
    assert [e["ctc_score"] for e in got] == [e["score"] for e in base] and got[0]["conf"] < got[1]["conf"]


def test_server_alternatives_of_a_decoder_free_connection_come_from_the_fused_totals(tmp_path):
    from speechcatcher_amd.server_session import ServerLoop
    blob = ngram.pack(_model(), V, 2)
    confs = {}
    for what, kw in {"plain": dict(), "fused": dict(ctc_lm=blob, lm_weight=0.5)}.items():
        batch = LmStub([_near_tie(2, 4), _near_tie(2, 4)])
        loop = ServerLoop(StreamScheduler(batch, NAMES, result_format="espnet"), vosk_output_format=True, ctc_beam=(4, 4), **kw)
        sid = loop.connect()
        _say(loop, sid, '{"config": {"decoder": "ctc", "max_alternatives": 4}}')
        _say(loop, sid, _pcm(6))
        alts = _say(loop, sid, '{"eof" : 1}')["alternatives"]
        confs[what] = {a["text"]: a["confidence"] for a in alts}
        assert abs(sum(a["confidence"] for a in alts) - 1.0) < 1e-9
        assert alts[0]["text"] == ("hello" if what == "plain" else "held")
    assert confs["plain"]["hello"] > confs["plain"]["held"] and confs["fused"]["held"] > confs["fused"]["hello"]
    with pytest.raises(ValueError, match="ctc_beam"):
        ServerLoop(StreamScheduler(LmStub([_near_tie(2, 4)]), NAMES, result_format="espnet"), vosk_output_format=True,
                   ctc_lm=blob)


def test_the_cli_takes_the_model_and_its_weights_and_refuses_them_without_the_beam(tmp_path):
    from speechcatcher_amd.__main__ import make_parser, recognize_file
    args = make_parser().parse_args(["--ctc-only", "--ctc-lm", "m.sclm", "--lm-weight", "0.7", "--word-bonus", "-0.1", "a.wav"])
    assert (args.ctc_lm, args.lm_weight, args.word_bonus, args.ctc_only) == ("m.sclm", 0.7, -0.1, True)
    args = make_parser().parse_args(["a.wav"])
    assert (args.ctc_lm, args.lm_weight, args.word_bonus) == ("", 0.5, 0.0)
    with pytest.raises(SystemExit, match="--ctc-beam or --ctc-only"):
        recognize_file(None, "a.wav", ctc_lm="m.sclm")
    with pytest.raises(SystemExit, match="does not exist"):
        recognize_file(None, "a.wav", ctc_only=True, ctc_lm=str(tmp_path / "missing.sclm"))


def test_recognize_segments_hands_the_model_to_the_scheduler():
    from speechcatcher_amd.scheduler import recognize_segments
    blob = ngram.pack(_model(), V, 2)
    with pytest.raises(ValueError, match="ctc_beam or ctc_only"):
        recognize_segments(LmStub([_near_tie(2, 4)]), np.zeros(640 * 6, np.float32), [(0, 640 * 6)], ctc_lm=blob)
    batch = LmStub([_near_tie(2, 4)])
    out = recognize_segments(batch, np.zeros(640 * 6, np.float32), [(0, 640 * 6)], chunk_length=640 * 3, token_list=NAMES,
                             ctc_beam=(4, 4), ctc_only=True, ctc_lm=blob, lm_weight=0.5)
    assert out[0]["text"] == "held" and out[0]["token_ids"] == [1, 4]
    nb = out[0]["ctc_nbest"][0]
    assert nb[0]["text"] == "held" and set(nb[0]) == {"text", "score", "conf", "lm", "ctc_score"}
    assert ("set_ctc_beam_lm", len(blob), 0.5, 0.0) in batch.calls


def test_the_python_engine_refuses_the_option_with_a_clear_error():
    from speechcatcher_amd.engine import EngineError, StreamBatch
    eng = StreamBatch.__new__(StreamBatch)                           # (the method needs nothing of a built batch)
    eng.set_ctc_beam_lm(None)
    with pytest.raises(EngineError, match="native engine"):
        eng.set_ctc_beam_lm(b"blob", 0.5, 0.0)
