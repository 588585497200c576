"""The host-side surfaces of consensus finals (StreamScheduler(consensus=...), ServerLoop(consensus=...), the CLI's
--consensus / --consensus-confidence, recognize_segments, speechcatcher_amd.mbr) on stand-in batches whose
consensus calls ARE the contract (tests/mbr_ref.py).  No GPU.

The stand-in's list is HYPS of tests/test_ctc_alt_spec.py: [6 7 8], [6 9], [10] with weights 1/2, 1/4, 1/4 at scale 1 -
risks 1.25, 1.5, 2.0: the first row stays - and 1/3 each at scale 0 - risks 5/3, 4/3, 5/3: the pivot moves to [6 9]."""
import json

import numpy as np
import pytest

import mbr_ref as M
from speechcatcher_amd import mbr
from speechcatcher_amd.scheduler import AlignedResults, StreamScheduler
from speechcatcher_amd.server_session import ServerLoop
from test_ctc_alt_spec import HYPS, TOKENS, FakeBatch, _final
from test_lm_rescore_surfaces import RescoringBatch, _blob, _one_final

EOS = 1023
A = lambda v: pytest.approx(v, rel=0, abs=1e-12)     # noqa: E731  (the stand-in's weights are exp(-ln 2) = 0.25 to an ulp)


def _entry(out, n):
    P, mp = int(out["header"][0]), int(out["header"][1])
    return {"order": out["order"], "risk": out["risk"], "weight": out["weight"], "status": out["status"], "pivot": P,
            "n_in": int(out["header"][2]), "dist": out["dist"][:n, :n], "conf": out["conf"][:mp], "alt_tok": out["alt_tok"][:mp],
            "alt_mass": out["alt_mass"][:mp], "gap_mass": out["gap_mass"]}


class MbrBatch(RescoringBatch):
    """RescoringBatch with the consensus calls of the C++ engine, answered by the contract"""

    def mbr_hyps(self, streams, scale=1.0, pivot_best=False, nbest=None):
        self.calls.append(("mbr_hyps", list(streams), scale, bool(pivot_best), nbest))
        a = self.hypotheses_arrays(streams)
        out = {}
        for i, s in enumerate(streams):
            nh = int(a["n_hyps"][i])
            out[int(s)] = _entry(M.mbr(a["ids"][i, :nh], score=a["score"][i, :nh], lens=a["lens"][i, :nh], L=a["ids"].shape[2],
                                       skip=1, strip=EOS, V=1024, scale=scale, pivot=0 if pivot_best else -1), nh)
        return out

    def mbr_lists(self, lists, values, weights=False, scale=1.0, pivots=None):
        self.calls.append(("mbr_lists", [list(map(list, li)) for li in lists], [list(v) for v in values], scale, pivots))
        out = []
        for k, (li, vs) in enumerate(zip(lists, values)):
            L = max([len(y) for y in li] + [1])
            rows = [list(y) + [0] * (L - len(y)) for y in li]
            kw = {"weight" if weights else "score": vs}
            out.append(_entry(M.mbr(rows, lens=[len(y) for y in li], L=L, V=1024, scale=scale,
                                    pivot=-1 if pivots is None else pivots[k], **kw), len(li)))
        return out


def _calls(fb, name):
    return [c for c in fb.calls if c[0] == name]


def test_default_off_replies_are_todays_and_partials_are_untouched():
    plain = _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet"))
    fb = MbrBatch()
    off = _one_final(StreamScheduler(fb, TOKENS, result_format="espnet"))
    assert off == plain and type(off) is type(plain) and getattr(off, "consensus", None) is None
    assert not _calls(fb, "mbr_hyps") and not _calls(fb, "mbr_lists")
    sch = StreamScheduler(fb, TOKENS, result_format="espnet", consensus=True)
    part = _one_final(sch, final=False)
    assert part == _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet"), final=False)
    assert getattr(part, "consensus", None) is None and not _calls(fb, "mbr_hyps")          # no launch for a partial
    # the Vosk messages of a loop without the option, byte for byte
    old = json.dumps(_final(ServerLoop(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet"), vosk_output_format=True,
                                       vosk_alignment=True)))
    new = json.dumps(_final(ServerLoop(StreamScheduler(MbrBatch(), TOKENS, result_format="espnet"), vosk_output_format=True,
                                       vosk_alignment=True)))
    assert old == new


def test_the_minimum_risk_row_leads_the_reply_and_every_token_says_what_stands_behind_it():
    plain = _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet"))
    fb = MbrBatch()
    res = _one_final(StreamScheduler(fb, TOKENS, result_format="espnet", consensus=True))
    assert _calls(fb, "mbr_hyps") == [("mbr_hyps", [0], 1.0, False, 3)]
    assert isinstance(res, AlignedResults) and [r[2] for r in res] == [r[2] for r in plain]      # scale 1: the first row stays
    assert res.consensus["mbr"] == {"pivot": 0, "risk": A(1.25), "am_rank": 0}
    recs = res.consensus["tokens"]
    assert [r["id"] for r in recs] == [6, 7, 8] and [r["token"] for r in recs] == [TOKENS[6], TOKENS[7], TOKENS[8]]
    assert [r["consensus"] for r in recs] == A([0.75, 0.5, 0.5])
    # [6 9] aligns as 6 . 9 and [10] as . . 10 (diagonal first): the rivals are "nothing here" twice, then 9 before 10 (a tie)
    assert [(r["rival"]["id"], r["rival"]["token"]) for r in recs] == [(-1, ""), (-1, ""), (9, TOKENS[9])]
    assert [r["rival"]["mass"] for r in recs] == A([0.25, 0.5, 0.25])
    # a flat posterior (scale 0): two rows agree on "6 ." against the best-scored row's length - the pivot moves
    fb = MbrBatch()
    res = _one_final(StreamScheduler(fb, TOKENS, result_format="espnet", consensus=True, consensus_scale=0.0))
    assert [r[2] for r in res] == [[6, 9], [6, 7, 8], [10]] and res[0][0] == plain[1][0]
    assert res.consensus["mbr"] == {"pivot": 1, "risk": float((0.0 + (1 / 3) * 2) + (1 / 3) * 2), "am_rank": 1}
    assert [r["id"] for r in res.consensus["tokens"]] == [6, 9]
    assert res.consensus["tokens"][0]["consensus"] == float((0.0 + 1 / 3) + 1 / 3)
    # "confidence": the transcript stays the first-ranked row's, the statistics are those of ITS slots
    fb = MbrBatch()
    res = _one_final(StreamScheduler(fb, TOKENS, result_format="espnet", consensus="confidence", consensus_scale=0.0))
    assert _calls(fb, "mbr_hyps") == [("mbr_hyps", [0], 0.0, True, 3)]
    assert [r[2] for r in res] == [r[2] for r in plain] and res.consensus["mbr"]["pivot"] == 0
    assert [r["id"] for r in res.consensus["tokens"]] == [6, 7, 8]
    # the native result format carries the attribute too
    nat = _one_final(StreamScheduler(MbrBatch(), TOKENS, consensus=True, consensus_scale=0.0))
    assert [r[2] for r in nat] == [[6, 9], [6, 7, 8], [10]] and nat.consensus["mbr"]["pivot"] == 1


def test_one_call_serves_all_finals_of_a_round_and_the_alignment_follows_the_pivot():
    class Two(MbrBatch):
        S = 2

    fb = Two()
    sch = StreamScheduler(fb, TOKENS, result_format="espnet", consensus=True, consensus_scale=0.0, align_final=True)
    a, b = sch.open(), sch.open()
    for sid in (a, b):
        sch.feed(sid, np.zeros(4000, np.float32), is_final=True, finalize_all=False)
    out = sch.step()
    assert len(_calls(fb, "mbr_hyps")) == 1 and sorted(_calls(fb, "mbr_hyps")[0][1]) == [0, 1]
    for sid in (a, b):
        assert out[sid][0][2] == [6, 9] and out[sid].consensus["mbr"]["pivot"] == 1
        assert out[sid].alignment["token_ids"] == [6, 9]
        assert out[sid].alignment["start_s"][0] > 0.3              # the engine's row 1: its frames start at 10 (RescoringBatch)


def test_with_final_lm_the_list_and_the_totals_are_the_re_ranked_ones():
    fb = MbrBatch()
    sch = StreamScheduler(fb, TOKENS, result_format="espnet", final_lm=_blob(), final_lm_weight=1.0, final_lm_eos=True,
                          consensus="confidence")
    res = _one_final(sch)
    (call,) = _calls(fb, "mbr_lists")
    assert not _calls(fb, "mbr_hyps")
    assert call[1] == [[[6, 9], [10], [6, 7, 8]]]                     # the fused order [1, 2, 0] (test_lm_rescore_surfaces)
    assert call[2] == [[e["fused"] for e in res.rescored]] and call[4] == [0]
    assert [r[2] for r in res] == [[6, 9], [10], [6, 7, 8]] and [e["am_rank"] for e in res.rescored] == [1, 2, 0]
    assert res.consensus["mbr"]["pivot"] == 0 and res.consensus["mbr"]["am_rank"] == 1
    assert [r["id"] for r in res.consensus["tokens"]] == [6, 9]
    # True: the minimum-risk row of the re-ranked list leads; the rescored records follow their results
    fb = MbrBatch()
    res = _one_final(StreamScheduler(fb, TOKENS, result_format="espnet", final_lm=_blob(), final_lm_weight=1.0, final_lm_eos=True,
                                     consensus=True, consensus_scale=0.0))
    want = M.mbr([[6, 9, 0], [10, 0, 0], [6, 7, 8]], score=[0.0] * 3, lens=[2, 1, 3], L=3, V=1024, scale=0.0)
    P = int(want["header"][0])
    order = [P] + [r for r in range(3) if r != P]
    assert [r[2] for r in res] == [[[6, 9], [10], [6, 7, 8]][r] for r in order]
    assert [e["am_rank"] for e in res.rescored] == [[1, 2, 0][r] for r in order]
    assert res.consensus["mbr"] == {"pivot": P, "risk": float(want["risk"][P]), "am_rank": [1, 2, 0][P]}


def test_vosk_word_entries_carry_the_consensus_as_conf():
    def loop(**kw):
        return ServerLoop(StreamScheduler(MbrBatch(), TOKENS, result_format="espnet"), vosk_output_format=True, **kw)

    (old,) = _final(loop(vosk_alignment=True))
    (msg,) = _final(loop(vosk_alignment=True, consensus="confidence"))
    assert msg["text"] == old["text"] and "mbr" not in msg and len(msg["result"]) == len(old["result"]) == 2   # "w6x7", "w8"
    for w, o in zip(msg["result"], old["result"]):
        assert w["am_conf"] == o["conf"] and (w["word"], w["start"], w["end"]) == (o["word"], o["start"], o["end"])
    assert [w["conf"] for w in msg["result"]] == A([0.5, 0.5])            # min(0.75, 0.5) over "w6" "x7"; 0.5 for "w8"
    assert msg["result"][0]["rival"] == {"word": "", "mass": A(0.5)} and msg["result"][1]["rival"] == {"word": "x9", "mass": A(0.25)}
    json.dumps(msg)
    (moved,) = _final(loop(vosk_alignment=True, consensus=True, consensus_scale=0.0))
    assert moved["text"] == "w6x9" and moved["mbr"]["pivot"] == 1 and moved["mbr"]["am_rank"] == 1
    assert moved["result"][0]["conf"] == 1 / 3                        # "w6x9": min(2/3 for "w6", 1/3 for "x9")
    # without a forced alignment the entries are per token
    (tok,) = _final(loop(consensus="confidence"))
    assert [w["conf"] for w in tok["result"]] == A([0.75, 0.5, 0.5]) and all(w["am_conf"] == 1.0 for w in tok["result"])
    # alternatives: the first one carries them
    (alt,) = _final(loop(vosk_alignment=True, vosk_alternatives=3, consensus="confidence"), {"max_alternatives": 2})
    assert [w["conf"] for w in alt["alternatives"][0]["result"]] == A([0.5, 0.5])
    assert "am_conf" not in alt["alternatives"][1]["result"][0]


def test_word_slots_take_the_minimum_of_their_tokens():
    recs = [{"id": 6, "token": "▁w6", "consensus": 0.9}, {"id": 7, "token": "x7", "consensus": 0.4,
                                                          "rival": {"id": -1, "token": "", "mass": 0.6}},
            {"id": 8, "token": "▁w8", "consensus": 1.0}]
    slots = mbr.word_slots(["▁w6", "x7", "▁w8"], recs)
    assert [(s["word"], s["consensus"]) for s in slots] == [("w6x7", 0.4), ("w8", 1.0)]
    assert slots[0]["rival"] == {"word": "", "mass": 0.6} and "rival" not in slots[1] and slots[0]["tokens"] == recs[:2]
    words = [{"word": "w6x7", "conf": 0.25, "start": 0.0, "end": 0.1}, {"word": "w8", "conf": 0.5, "start": 0.1, "end": 0.2}]
    got = mbr.vosk_words(words, slots)
    assert [(w["conf"], w["am_conf"]) for w in got] == [(0.4, 0.25), (1.0, 0.5)] and words[0]["conf"] == 0.25
    assert mbr.vosk_words(words[:1], slots) == words[:1]               # entries and slots that do not correspond stay
    assert mbr.labels([1023, 6, 9, 1023, 0], 4, 1023) == [6, 9] and mbr.labels([1023, 6, 9], 3, 1023) == [6, 9]
    assert mbr.labels([1023], 1, 1023) == []


def test_the_refusals():
    class Narrow(MbrBatch):
        W = 1

    with pytest.raises(ValueError, match="beam_size of at least 2"):
        StreamScheduler(Narrow(), TOKENS, consensus=True)
    with pytest.raises(NotImplementedError, match="C\\+\\+ engine"):
        StreamScheduler(FakeBatch(), TOKENS, consensus=True)         # a batch without the call says so
    with pytest.raises(NotImplementedError, match="C\\+\\+ engine"):
        ServerLoop(StreamScheduler(FakeBatch(), TOKENS, result_format="espnet"), vosk_output_format=True, consensus="confidence")
    with pytest.raises(ValueError, match='True or "confidence"'):
        StreamScheduler(MbrBatch(), TOKENS, consensus="best")
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="consensus_scale"):
            StreamScheduler(MbrBatch(), TOKENS, consensus=True, consensus_scale=bad)
    sch = StreamScheduler(MbrBatch(), TOKENS, consensus=True)
    sch.enable_consensus(None)
    assert sch.consensus is None and getattr(_one_final(sch), "consensus", None) is None
    from speechcatcher_amd.engine import StreamBatch
    assert not hasattr(StreamBatch, "mbr_hyps")                      # the Python lock-step engine has none


def test_the_cli_and_recognize_segments_take_the_option():
    from speechcatcher_amd.__main__ import make_parser, recognize_file
    from speechcatcher_amd.scheduler import recognize_segments
    p = make_parser()
    assert p.parse_args(["--consensus", "a.wav"]).consensus is True
    assert p.parse_args(["--consensus-confidence", "a.wav"]).consensus == "confidence"
    assert p.parse_args(["a.wav"]).consensus is None

    class OneBeam:
        beam_size = 1

    with pytest.raises(SystemExit, match="--beamsize of at least 2"):
        recognize_file(OneBeam(), "a.wav", consensus=True)
    kw = dict(chunk_length=4000, token_list=TOKENS)
    plain = recognize_segments(MbrBatch(), np.zeros(4000, np.float32), [(0, 4000)], **kw)
    assert "mbr" not in plain[0] and "token_consensus" not in plain[0]
    out = recognize_segments(MbrBatch(), np.zeros(4000, np.float32), [(0, 4000)], consensus="confidence", **kw)
    assert out[0]["token_ids"] == plain[0]["token_ids"] == [6, 7, 8] and out[0]["token_consensus"] == A([0.75, 0.5, 0.5])
    assert out[0]["mbr"] == [{"pivot": 0, "risk": A(1.25), "am_rank": 0}] and out[0]["token_rival"][2]["id"] == 9
    assert {k: v for k, v in out[0].items() if k not in ("mbr", "token_consensus", "token_rival")} == plain[0]
