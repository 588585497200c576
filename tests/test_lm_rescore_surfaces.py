"""The host-side surfaces of n-gram rescoring of finals (StreamScheduler(final_lm=...), ServerLoop(rescore_lm=...), the CLI's
--rescore-lm / --rescore-weight / --rescore-bonus, recognize_segments, the Python engine's refusal) on
stand-in batches whose rescoring IS the contract (tests/lm_rescore_ref.py).  No GPU."""
import json

import numpy as np
import pytest

import lm_rescore_ref as RS
from speechcatcher_amd import alternates, ngram
from speechcatcher_amd.scheduler import AlignedResults, StreamScheduler
from speechcatcher_amd.server_session import ServerLoop
from test_ctc_alt_spec import HYPS, SCORES, TOKENS, FakeBatch, _final
from test_ctc_beam_lm_surfaces import LmStub, _model, _near_tie
from test_ctc_beam_surfaces import NAMES, StubBatch, _feed

EOS = 1023


def _blob():
    """every unigram -3; "6 9" and "9 </s>" are likely.  With the end term the list HYPS ranks [1, 2, 0], without it
    [2, 1, 0], by its own scores [0, 1, 2]"""
    model = {(t,): (-3.0, 0.0) for t in (6, 7, 8, 9, 10, EOS)}
    model.update({(6, 9): (-0.1, 0.0), (9, EOS): (-0.1, 0.0)})
    return ngram.pack(model, 1024, 2)


class _Model:
    def __init__(self, blob):
        self.blob = ngram.Blob(bytes(blob))


class RescoringBatch(FakeBatch):
    """FakeBatch with the rescoring calls of the C++ engine, answered by the contract; the alignment of the engine's row j
    starts at frame 10 j, so a reply shows which row it was aligned at"""

    def language_model(self, model):
        self.calls.append(("language_model", len(model)))
        return _Model(model)

    def _align(self, n, nb):
        al = super()._align(n, nb)
        al["start"] = al["start"] + 10 * np.arange(nb, dtype=np.int32)[None, :, None]
        al["end"] = al["start"] + 2
        return al

    def rescore_hyps(self, streams, model, alpha=0.5, beta=0.0, lm_eos=-1, final=(), nbest=None):
        self.calls.append(("rescore_hyps", list(streams), alpha, beta, lm_eos, list(final), nbest))
        a = self.hypotheses_arrays(streams)
        out = {}
        for i, s in enumerate(streams):
            nh = int(a["n_hyps"][i])
            r = RS.rescore(model.blob, a["ids"][i, :nh], a["score"][i, :nh], a["lens"][i, :nh], a["ids"].shape[2], skip=1,
                           strip=self.cfg.eos_id, lm_eos=lm_eos if s in final else -1, alpha=alpha, beta=beta)
            out[int(s)] = {k: r[k] for k in ("order", "fused", "lm", "eos_lm", "status")}
        return out


def _one_final(sch, final=True):
    sid = sch.open()
    sch.feed(sid, np.zeros(4000, np.float32), is_final=final, finalize_all=False)
    out = sch.step()[sid]
    sch.close(sid)
    return out


def test_finals_are_re_ranked_partials_are_untouched_and_every_entry_says_what_the_model_added():
    assert RescoringBatch.cfg.eos_id == EOS
    plain = _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet"))
    assert [r[2] for r in plain] == [[6, 7, 8], [6, 9], [10]] and getattr(plain, "rescored", None) is None
    fb = RescoringBatch()
    sch = StreamScheduler(fb, TOKENS, result_format="espnet", final_lm=_blob(), final_lm_weight=1.0, final_lm_eos=True)
    assert sch.final_lm == (1.0, 0.0, True) and fb.calls == [("language_model", len(_blob()))]
    part = _one_final(sch, final=False)
    assert part == _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet"), final=False)
    assert getattr(part, "rescored", None) is None and len(fb.calls) == 1          # no launch for a partial
    res = _one_final(sch)
    assert fb.calls[-1] == ("rescore_hyps", [0], 1.0, 0.0, EOS, [0], 3)
    assert isinstance(res, AlignedResults) and [r[2] for r in res] == [[6, 9], [10], [6, 7, 8]]
    assert res[0][0] == plain[1][0] and [r[0] for r in res] == [plain[k][0] for k in (1, 2, 0)]
    want = RS.rescore(ngram.Blob(_blob()), [np.asarray(y) for y in HYPS[:1]], SCORES[:1], L=5, skip=1, strip=EOS, lm_eos=EOS,
                      alpha=1.0)
    assert [e["am_rank"] for e in res.rescored] == [1, 2, 0]
    assert [set(e) for e in res.rescored] == [{"score", "lm", "fused", "am_rank"}] * 3
    assert res.rescored[2]["fused"] == want["fused"][0] and res.rescored[2]["lm"] == want["lm"][0] + want["eos_lm"][0]
    assert [e["score"] for e in res.rescored] == [SCORES[k] for k in (1, 2, 0)]     # the search's scores do not change
    assert [e["fused"] for e in res.rescored] == sorted((e["fused"] for e in res.rescored), reverse=True)
    for r, e in zip(res, res.rescored):                                           # "espnet": the hypothesis dicts too
        assert {k: r[4][k] for k in e} == e
    # without the end term the model prefers the other short hypothesis; a bonus per label brings the long one back
    noeos = _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet", final_lm=_blob(), final_lm_weight=1.0))
    assert [e["am_rank"] for e in noeos.rescored] == [2, 1, 0]
    bonus = _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet", final_lm=_blob(), final_lm_weight=1.0,
                                       final_word_bonus=10.0, final_lm_eos=True))
    assert [e["am_rank"] for e in bonus.rescored] == [0, 1, 2]
    # the native result format has no hypothesis dicts: the attribute carries the values
    nat = _one_final(StreamScheduler(RescoringBatch(), TOKENS, final_lm=_blob(), final_lm_weight=1.0, final_lm_eos=True))
    assert [len(r) for r in nat] == [3] * 3 and [e["am_rank"] for e in nat.rescored] == [1, 2, 0]
    sch.enable_final_lm(None)
    assert sch.final_lm is None and [r[2] for r in _one_final(sch)] == [r[2] for r in plain]


def test_alignment_and_alternates_belong_to_the_hypothesis_reported():
    base = _one_final(StreamScheduler(RescoringBatch(), TOKENS, result_format="espnet", align_final=True, align_nbest=3))
    fb = RescoringBatch()
    sch = StreamScheduler(fb, TOKENS, result_format="espnet", align_final=True, align_nbest=3, final_lm=_blob(),
                          final_lm_weight=1.0, final_lm_eos=True)
    res = _one_final(sch)
    assert ("align", 3) in fb.calls                                   # wide enough to hold the rows reported
    al = res.alignment
    assert al["token_ids"] == [6, 9] and al == base.alignment["nbest"][1] | {"nbest": al["nbest"]}
    assert al["nbest"][1:] == [base.alignment["nbest"][2], base.alignment["nbest"][0]]
    assert al["start_s"][0] > base.alignment["start_s"][0]            # row 1 of the engine's list: its frames start at 10
    # the first result alone: the call is as wide as the row it sits in
    fb = RescoringBatch()
    res = _one_final(StreamScheduler(fb, TOKENS, result_format="espnet", alternates=2, final_lm=_blob(), final_lm_weight=1.0,
                                     final_lm_eos=True))
    assert ("alternates", 2, 2) in fb.calls and res.alignment["token_ids"] == [6, 9]
    assert [r["id"] for r in res.alignment["alternates"]] == [6, 9]


def test_vosk_final_text_and_alternatives_follow_the_fused_ranking():
    def loop(**kw):
        fb = RescoringBatch()
        return ServerLoop(StreamScheduler(fb, TOKENS, result_format="espnet"), vosk_output_format=True, **kw), fb

    old = _final(loop(vosk_alignment=True)[0])
    lp, fb = loop(vosk_alignment=True, vosk_alternatives=3, rescore_lm=_blob(), rescore_weight=1.0)
    assert lp.sch.final_lm == (1.0, 0.0, True)
    (plain,) = _final(lp)
    assert plain["text"] == "w6x9" != old[0]["text"] and set(plain) == {"result", "text"}
    (msg,) = _final(lp, {"max_alternatives": 3})
    a = msg["alternatives"]
    assert [e["text"] for e in a] == ["w6x9", "w10", "w6x7 w8"]
    want = RS.rescore(ngram.Blob(_blob()), [np.asarray(y + [0] * (5 - len(y))) for y in HYPS], SCORES, [len(y) for y in HYPS], 5,
                      skip=1, strip=EOS, lm_eos=EOS, alpha=1.0)
    assert want["order"].tolist() == [1, 2, 0]
    np.testing.assert_allclose([e["confidence"] for e in a], alternates.nbest_posterior(want["fused"][want["order"]]),
                               rtol=0, atol=1e-15)
    assert a[0]["result"] == plain["result"] and a[0]["result"][0]["start"] > old[0]["result"][0]["start"]
    json.dumps(msg)
    (two,) = _final(lp, {"max_alternatives": 2})
    assert [e["text"] for e in two["alternatives"]] == ["w6x9", "w10"]
    # partials are what they were
    outs = []
    for l in (loop()[0], loop(rescore_lm=_blob(), rescore_weight=1.0)[0]):
        sid = l.connect()
        l.submit(sid, np.zeros(4000, np.int16))
        outs.append(l.step().get(sid))
    assert outs[0] == outs[1] and outs[0]


class EndStub(LmStub):
    """LmStub with the list rescoring of the C++ engine, answered by the contract; token 5 stands for </s>"""

    def __init__(self, tables):
        super().__init__(tables)
        self.cfg.eos_id = 5

    def language_model(self, model):
        return _Model(model)

    def rescore_lists(self, lists, scores, model, alpha=0.5, beta=0.0, lm_eos=-1, state0=None):
        self.calls.append(("rescore_lists", [len(li) for li in lists], alpha, beta, lm_eos))
        out = []
        for li, sc in zip(lists, scores):
            L = max(map(len, li))
            r = RS.rescore(model.blob, [list(y) + [0] * (L - len(y)) for y in li], sc, [len(y) for y in li], L, skip=0,
                           lm_eos=lm_eos, alpha=alpha, beta=beta)
            out.append({k: r[k] for k in ("order", "fused", "lm", "eos_lm", "status", "end_state")})
        return out


def test_a_decoder_free_final_gets_the_end_term_of_the_fused_model():
    import ngram_ref as NR
    # "he ld" is frequent and never last; "he llo" ends sentences
    model = NR.estimate([[1, 4, 3, 5]] * 10 + [[1, 2, 5]] * 8 + [[2, 1], [3, 2], [4, 3]], 8, 2)
    blob = ngram.pack(model, 8, 2)
    tables = [_near_tie(2, 4), _near_tie(2, 4)]
    runs = {}
    for eos in (False, True):
        batch = EndStub(tables)
        sch = StreamScheduler(batch, NAMES, ctc_beam=(4, 4), ctc_lm=blob, lm_weight=0.5, final_lm_eos=eos)
        sid = sch.open(decoder="ctc")
        _feed(sch, sid, 3, False)
        part = sch.step()[sid]
        assert not any(c[0] == "rescore_lists" for c in batch.calls)  # partials are untouched
        _feed(sch, sid, 3, True)
        runs[eos] = (sch.step()[sid], batch, part)
    (off, _, part_off), (on, batch, part_on) = runs[False], runs[True]
    assert part_off.ctc_nbest == part_on.ctc_nbest
    assert ("rescore_lists", [len(off.ctc_nbest)], 0.5, 0.0, 5) in batch.calls
    assert "am_rank" not in off.ctc_nbest[0] and [set(e) - set(off.ctc_nbest[0]) for e in on.ctc_nbest] == \
        [{"eos_lm", "am_rank"}] * len(on.ctc_nbest)
    by_rank = {e["am_rank"]: e for e in on.ctc_nbest}
    for r, e in enumerate(off.ctc_nbest):                             # the same entries, each with its term
        g = by_rank[r]
        assert (g["ids"], g["lm"], g["ctc_score"]) == (e["ids"], e["lm"], e["ctc_score"])
        ctx = RS.walk(ngram.Blob(blob), e["ids"])[2]
        assert g["eos_lm"] == ngram.Blob(blob).score(ctx, 5)[0]
        assert g["score"] == float(e["ctc_score"] + (float(0.5 * float(e["lm"] + g["eos_lm"])) + 0.0))
    assert [e["score"] for e in on.ctc_nbest] == sorted((e["score"] for e in on.ctc_nbest), reverse=True)
    assert abs(sum(e["conf"] for e in on.ctc_nbest) - 1.0) < 1e-12
    assert off[0][2] == [1, 4] and on[0][2] == [1, 2] and on.ctc_nbest[0]["am_rank"] > 0      # the end term flips the final
    # a batch without the call says so
    with pytest.raises(NotImplementedError, match="C\\+\\+ engine"):
        StreamScheduler(LmStub(tables), NAMES, ctc_beam=(4, 4), ctc_lm=blob, final_lm_eos=True)


def test_the_refusals():
    with pytest.raises(NotImplementedError, match="C\\+\\+ engine"):
        StreamScheduler(StubBatch([_near_tie(2, 4)]), NAMES, final_lm=_blob())    # a batch without the call says so
    with pytest.raises(NotImplementedError, match="C\\+\\+ engine"):
        ServerLoop(StreamScheduler(StubBatch([_near_tie(2, 4)]), NAMES, result_format="espnet"), vosk_output_format=True,
                   rescore_lm=_blob())
    with pytest.raises(ValueError, match="finite"):
        StreamScheduler(RescoringBatch(), TOKENS, final_lm=_blob(), final_lm_weight=float("nan"))

    class Wide(RescoringBatch):
        W = 17

    with pytest.raises(ValueError, match="at most 16"):
        StreamScheduler(Wide(), TOKENS, final_lm=_blob())
    from speechcatcher_amd.engine import EngineError, StreamBatch
    eng = StreamBatch.__new__(StreamBatch)                           # (the method needs nothing of a built batch)
    assert not hasattr(eng, "rescore_hyps")
    with pytest.raises(EngineError, match="native engine"):
        eng.language_model(b"blob")


def test_the_cli_and_recognize_segments_take_the_model_and_its_weights(tmp_path):
    from speechcatcher_amd.__main__ import make_parser, recognize_file
    from speechcatcher_amd.scheduler import recognize_segments
    args = make_parser().parse_args(["--rescore-lm", "m.sclm", "--rescore-weight", "0.7", "--rescore-bonus", "-0.1", "a.wav"])
    assert (args.rescore_lm, args.rescore_weight, args.rescore_bonus) == ("m.sclm", 0.7, -0.1)
    args = make_parser().parse_args(["a.wav"])
    assert (args.rescore_lm, args.rescore_weight, args.rescore_bonus) == ("", 0.5, 0.0)
    with pytest.raises(SystemExit, match="not with --ctc-only"):
        recognize_file(None, "a.wav", ctc_only=True, rescore_lm="m.sclm")
    with pytest.raises(SystemExit, match="does not exist"):
        recognize_file(None, "a.wav", rescore_lm=str(tmp_path / "missing.sclm"))
    with pytest.raises(ValueError, match="not with ctc_only"):
        recognize_segments(RescoringBatch(), np.zeros(4000, np.float32), [(0, 4000)], ctc_only=True, rescore_lm=_blob())
    path = tmp_path / "m.sclm"
    path.write_bytes(_blob())
    plain = recognize_segments(RescoringBatch(), np.zeros(4000, np.float32), [(0, 4000)], chunk_length=4000, token_list=TOKENS)
    out = recognize_segments(RescoringBatch(), np.zeros(4000, np.float32), [(0, 4000)], chunk_length=4000, token_list=TOKENS,
                             rescore_lm=str(path), rescore_weight=1.0)
    assert plain[0]["token_ids"] == [6, 7, 8] and "am_rank" not in plain[0]
    assert out[0]["token_ids"] == [6, 9] and out[0]["am_rank"] == 1 and out[0]["score"] == SCORES[1]
    assert out[0]["fused_score"] == SCORES[1] + 1.0 * out[0]["lm_score"]
