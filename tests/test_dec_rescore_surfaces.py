"""The host-side surfaces of attention rescoring (StreamScheduler(ctc_beam=..., attention_rescore=...), ServerLoop(
attention_rescore=...), the CLI's --attention-rescore, the Python engine's refusal) on a stub batch whose
rescoring follows the contract's fusing and ranking rules (tests/dec_rescore_ref.py) over a canned attention score.
No GPU."""
import numpy as np
import pytest

import ctc_beam_ref as R
import dec_rescore_ref as DR
import ngram_ref as NR
from speechcatcher_amd import ctc_beam as M
from speechcatcher_amd import ngram
from speechcatcher_amd.scheduler import CtcBeamResults, StreamScheduler
from test_ctc_beam_grammar_surfaces import GrStub
from test_lm_rescore_surfaces import EndStub
from test_ctc_beam_surfaces import LABELS, NAMES, StubBatch, _feed, _pcm, _say, _table

V = 8
FAVOURITES = ([1, 3, 4], [3, 6, 1, 2])       # rank 2 of the stub's first pass over LABELS[0], rank 1 over LABELS[1]


def canned_att(ids):
    """the stand-in for the decoder's log probability: it likes short lists of labels, and two entries that the first
    pass ranks behind its best most of all"""
    return -0.25 if list(ids) in FAVOURITES else -2.0 - 1.5 * len(ids)


class AttMixin:
    """attention_rescore_beam by the contract's rules: fused = (w_ctc * first pass + w_att * att) + beta * labels, ranked"""

    def attention_rescore_beam(self, streams, nbest=16, w_att=1.0, w_ctc=0.5, beta=0.0):
        self.calls.append(("attention_rescore_beam", tuple(streams), nbest, w_att, w_ctc, beta))
        hyps = self.ctc_beam_hyps(streams, nbest)
        sides = dict(zip(streams, self.ctc_beam_lm(streams, nbest))) if getattr(self, "lm", None) is not None else {}
        out = {}
        for s in streams:
            first = [R.lae(h["pb"], h["pnb"]) for h in hyps[s]]
            if s in sides:
                first = [float(f) for f in sides[s]["fused"][:len(first)]]
            att = np.asarray([canned_att(h["ids"]) for h in hyps[s]])
            fused = np.asarray([DR.fuse(f, a, len(h["ids"]), w_att, w_ctc, beta) for f, a, h in zip(first, att, hyps[s])])
            status = np.zeros(len(first), np.int32)
            out[s] = {"order": DR.rank(fused, status), "fused": fused, "att": att, "ctc_score": np.asarray(first),
                      "status": status}
        return out


class AttStub(AttMixin, StubBatch):
    pass


class AttLmStub(AttMixin, EndStub):
    pass


class AttGrStub(AttMixin, GrStub):
    pass


def _tables():
    return [_table(lab, seed=k) for k, lab in enumerate(LABELS)]


def test_rescore_sessions_are_re_ranked_at_finals_by_one_call_and_the_others_are_untouched():
    batch = AttStub(_tables() + _tables())
    with pytest.raises(ValueError, match="ctc_beam"):
        StreamScheduler(AttStub(_tables()), NAMES, attention_rescore=True)       # requires the beam
    with pytest.raises(ValueError, match="attention_rescore"):
        StreamScheduler(AttStub(_tables()), NAMES, ctc_beam=(4, 4)).open(decoder="rescore")   # only with the option on
    with pytest.raises(NotImplementedError):
        StreamScheduler(StubBatch(_tables()), NAMES, ctc_beam=(4, 4), attention_rescore=True)   # a batch without the call
    with pytest.raises(ValueError):
        StreamScheduler(AttStub(_tables()), NAMES, ctc_beam=(4, 4), attention_rescore=(1.0, float("nan")))
    assert StreamScheduler(AttStub(_tables()), NAMES, ctc_beam=(4, 4), attention_rescore=True).attention_rescore == (1.0, 0.5, 0.0)
    sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4), attention_rescore=(4.0, 0.5, 0.125))
    assert sch.attention_rescore == (4.0, 0.5, 0.125)
    full, ctc, r1, r2 = sch.open(), sch.open(decoder="ctc"), sch.open(decoder="rescore"), sch.open(decoder="rescore")
    assert [sch.decoder(s) for s in (full, ctc, r1, r2)] == ["full", "ctc", "rescore", "rescore"]
    assert ("set_decoder", 2, "ctc") in batch.calls and ("set_decoder", 3, "ctc") in batch.calls   # decoder-free in the engine
    for sid in (full, ctc, r1, r2):
        _feed(sch, sid, 5)
    out = sch.step()
    assert not [c for c in batch.calls if c[0] == "attention_rescore_beam"]     # partials: the beam's best, as for "ctc"
    assert out[r2][0][:3] == out[ctc][0][:3] and "att" not in out[r2].ctc_nbest[0]
    for sid in (full, ctc, r1, r2):
        _feed(sch, sid, 5, True)
    # the finals reset their slots: take the first pass from a second stub driven the same way
    twin = AttStub(_tables() + _tables())
    twin.set_ctc_beam(4, 4)
    twin.push([(s, np.zeros(6400, np.float32), True) for s in range(4)])
    want = twin.attention_rescore_beam([2, 3], 4, 4.0, 0.5, 0.125)
    out = sch.step()
    calls = [c for c in batch.calls if c[0] == "attention_rescore_beam"]
    assert calls == [("attention_rescore_beam", (2, 3), 4, 4.0, 0.5, 0.125)]    # ONE call for the round's finals
    for sid, slot in ((r1, 2), (r2, 3)):
        nb, w = out[sid].ctc_nbest, want[slot]
        plain = twin.ctc_beam_hyps([slot], 4)[slot]
        assert isinstance(out[sid], CtcBeamResults) and len(nb) == len(plain)
        assert [e["ids"] for e in nb] == [plain[int(r)]["ids"] for r in w["order"]]
        assert [e["am_rank"] for e in nb] == [int(r) for r in w["order"]]
        for e in nb:
            r = e["am_rank"]
            assert e["score"] == w["fused"][r] and e["att"] == w["att"][r] and e["ctc_score"] == w["ctc_score"][r]
        assert [e["score"] for e in nb] == sorted((e["score"] for e in nb), reverse=True)
        assert abs(sum(e["conf"] for e in nb) - 1.0) < 1e-12 and nb[0]["conf"] == max(e["conf"] for e in nb)
        assert out[sid][0][2] == nb[0]["ids"]                                   # the reply's text is the re-ranked best
    assert out[r1].ctc_nbest[0]["ids"] == [1, 3, 4] and out[r1].ctc_nbest[0]["am_rank"] == 2     # the pass changed the best
    assert out[r2].ctc_nbest[0]["ids"] == [3, 6, 1, 2] and out[r2].ctc_nbest[0]["am_rank"] == 1
    # "ctc" and FULL sessions: untouched
    assert "att" not in out[ctc].ctc_nbest[0] and out[ctc].ctc_nbest[0]["ids"] == [3, 4, 1, 2]
    assert out[full][0][0] == "t7t9" and "att" not in out[full].ctc_nbest[0]
    # set_decoder before the first audio; the slot of a closed session goes back to the full decoder
    sch.close(r1)
    again = sch.open()
    assert sch.decoder(again) == "full"
    sch.set_decoder(again, "rescore")
    assert sch.decoder(again) == "rescore"
    sch.set_decoder(again, "ctc")
    assert sch.decoder(again) == "ctc"


def test_composition_with_a_grammar_complete_entries_stay_first():
    from speechcatcher_amd import grammar
    batch = AttGrStub(_tables())
    sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4), attention_rescore=(4.0, 0.5, 0.0))
    sid = sch.open(decoder="rescore", grammar=grammar.compile([[1, 2], [3, 4]], V, 0))
    _feed(sch, sid, 10, True)
    nb = sch.step()[sid].ctc_nbest
    flags = [e["complete"] for e in nb]
    assert flags == sorted(flags, reverse=True) and all("att" in e for e in nb)
    for group in (True, False):                                                  # inside a group: the attention pass's order
        sc = [e["score"] for e in nb if e["complete"] is group]
        assert sc == sorted(sc, reverse=True)


def test_composition_with_the_end_term_of_the_fused_model():
    blob = ngram.pack(NR.estimate([[1, 2, 3, 4]] * 8 + [[3, 4, 1, 2]] * 2 + [[3, 4, 1]], V, 2), V, 2)
    batch = AttLmStub(_tables())
    sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4), ctc_lm=blob, lm_weight=0.5, final_lm_eos=True,
                          attention_rescore=(4.0, 0.5, 0.0))
    sid = sch.open(decoder="rescore")
    _feed(sch, sid, 10, True)
    nb = sch.step()[sid].ctc_nbest
    assert all({"att", "eos_lm", "am_rank", "lm", "first_pass"} <= set(e) for e in nb)
    for e in nb:    # the </s> term is added to the attention-fused total
        want = DR.fuse(e["first_pass"], e["att"], len(e["ids"]), 4.0, 0.5, 0.0) + 0.5 * e["eos_lm"]
        assert e["score"] == want
    assert [e["score"] for e in nb] == sorted((e["score"] for e in nb), reverse=True)


def test_server_connection_with_decoder_rescore():
    from speechcatcher_amd.server_session import ServerLoop
    batch = AttStub(_tables())
    sch = StreamScheduler(batch, NAMES, result_format="espnet")
    with pytest.raises(ValueError):
        ServerLoop(StreamScheduler(AttStub(_tables()), NAMES, result_format="espnet"), vosk_output_format=True,
                   attention_rescore=True)                                       # requires the beam
    loop = ServerLoop(sch, vosk_output_format=True, ctc_beam=(4, 4), attention_rescore=(4.0, 0.5))
    assert loop.sch.attention_rescore == (4.0, 0.5, 0.0)
    _, free = loop.connect(), loop.connect()
    assert _say(loop, free, '{"config": {"decoder": "rescore", "max_alternatives": 9}}') == {"partial": ""}
    assert loop.sch.decoder(free) == "rescore" and loop.sessions[free].max_alternatives == 4
    assert _say(loop, free, _pcm(5)) == {"partial": "world"}                     # partials: the beam's best
    assert _say(loop, free, _pcm(5)) == {"partial": "world hello"}
    final = _say(loop, free, '{"eof" : 1}')
    alts = final["alternatives"]
    assert alts[0]["text"] == M.text_of([3, 6, 1, 2], NAMES) != "world hello" and len(alts) >= 2   # from the re-ranked list
    assert [a["confidence"] for a in alts] == sorted((a["confidence"] for a in alts), reverse=True)
    assert isinstance(_say(loop, free, '{"config": {"decoder": "greedy"}}'), ValueError)
    plain = ServerLoop(StreamScheduler(AttStub(_tables()), NAMES, result_format="espnet"), vosk_output_format=True,
                       ctc_beam=(4, 4))
    c = plain.connect()
    assert isinstance(_say(plain, c, '{"config": {"decoder": "rescore"}}'), ValueError)      # only with the option on


def test_cli_flag_and_the_segment_loop():
    from speechcatcher_amd.__main__ import make_parser
    from speechcatcher_amd.scheduler import recognize_segments
    p = make_parser()
    assert p.parse_args(["a.wav"]).attention_rescore is None
    assert p.parse_args(["--ctc-only", "--attention-rescore", "--", "a.wav"]).attention_rescore == 1.0
    assert p.parse_args(["--ctc-only", "--attention-rescore", "4", "a.wav"]).attention_rescore == 4.0
    speech = np.zeros(640 * 10, np.float32)
    tables = [_table(LABELS[1], seed=1)]
    base = recognize_segments(AttStub(tables), speech, [(0, 6400)], chunk_length=3200, token_list=NAMES, ctc_only=True)[0]
    out = recognize_segments(AttStub(tables), speech, [(0, 6400)], chunk_length=3200, token_list=NAMES, ctc_only=True,
                             ctc_beam=4, attention_rescore=(4.0, 0.5))[0]
    assert base["text"] == "world hello" and out["text"] == M.text_of([3, 6, 1, 2], NAMES) != base["text"]
    assert [e["text"] for e in out["ctc_nbest"][0]][0] == out["text"]
    with pytest.raises(ValueError, match="ctc_only"):
        recognize_segments(AttStub(tables), speech, [(0, 6400)], token_list=NAMES, ctc_beam=4, attention_rescore=True)


def test_python_engine_refuses_the_option():
    from speechcatcher_amd.engine import StreamBatch
    assert not hasattr(StreamBatch, "attention_rescore_beam")
    with pytest.raises(NotImplementedError, match="C\\+\\+ engine"):
        StreamScheduler(StubBatch(_tables()), NAMES, ctc_beam=(4, 4)).enable_attention_rescore(True)
