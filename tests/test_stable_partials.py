"""Stable partials above the engine, on the spec backend: StreamScheduler(stable_partials=True) owns the trackers and asks
only for what they do not hold, ServerLoop(stable_partials=True) puts the committed text and the open tokens' stability on
its Vosk partials - and with the option off every message is what it was."""
import json

import numpy as np
import pytest

from commit_helpers import CHUNK, N_CHUNKS, audio, make_batch
from speechcatcher_amd import commit
from speechcatcher_amd.scheduler import DraftResults, LevelResults, StableResults, StreamScheduler
from speechcatcher_amd.server_session import ServerLoop, scale_server_pcm
from speechcatcher_amd.speech2text_streaming import TEXT_SKIP_IDS, hyps_to_results

MODEL, BEAM = "plain", 10


def _spec_batch(n_streams=2, bbd=False):
    from oracle.kernel_spec import SpecBackend
    return make_batch(MODEL, "TINY", SpecBackend(), n_streams, BEAM, bbd, max_frames=400, max_tokens=300,
                      pcm_capacity=1 << 18)


def _pcm16(x):
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def lockstep():
    """what a client with its own StablePrefix sees on stream 0 of a plain batch: the tracker's state after every chunk
    (the last chunk is final), for the server's audio (int16 scaled back)"""
    pcm = _pcm16(audio(5))
    x = scale_server_pcm(pcm)
    sb = _spec_batch()
    sp, states, calls = commit.StablePrefix(), [], []
    real = sb.hyps_delta
    for k in range(N_CHUNKS):
        fin = k == N_CHUNKS - 1
        sb.push([(0, x[k * CHUNK:(k + 1) * CHUNK], fin)])
        d = real([0], [sp.next_from], final=[0] if fin else [])[0]
        calls.append((sp.next_from, len(d["tokens"])))
        states.append(sp.update(d, final=fin).state())
    mid = [s["committed"] for s in states[:-1] if 1 < s["committed"] < len(s["tokens"])]
    assert len(set(mid)) >= 3                                        # the committed prefix grows through the utterance
    return {"pcm": pcm, "audio": x, "states": states, "calls": calls, "cfg": sb.cfg}


def test_scheduler_replies_carry_the_trackers_state_and_ask_only_for_the_tail(lockstep):
    p = lockstep
    sb = _spec_batch()
    asked, real = [], sb.hyps_delta

    def spy(streams, from_, final=()):
        out = real(streams, from_, final=final)
        asked.append((list(streams), list(from_), list(final), {s: len(out[s]["tokens"]) for s in streams}))
        return out

    sb.hyps_delta = spy
    sch = StreamScheduler(sb, None, result_format="espnet", stable_partials=True)
    sid = sch.open()
    for k in range(N_CHUNKS):
        sch.feed(sid, p["audio"][k * CHUNK:(k + 1) * CHUNK], is_final=k == N_CHUNKS - 1)
        res = sch.step()[sid]
        assert isinstance(res, StableResults) and isinstance(res, LevelResults) and isinstance(res, list)
        assert res.stable == p["states"][k], k
        assert sorted(res.stable) == ["committed", "stability", "tokens"]
        assert len(res.stable["stability"]) == len(res.stable["tokens"]) - res.stable["committed"]
        assert res.draft is None and res.level is None
    slot = asked[0][0][0]
    assert [(a[1][0], a[3][slot]) for a in asked] == p["calls"]     # one call per reply, from = what the tracker held
    assert asked[-1][2] == [slot] and all(a[2] == [] for a in asked[:-1])
    assert sum(n for _, n in p["calls"]) < sum(len(s["tokens"]) for s in p["states"]) // 2   # far less than whole hypotheses
    last = p["states"][-1]
    assert last["committed"] == len(last["tokens"]) > 1 and last["stability"] == []   # the final commits everything
    # the next utterance of the session starts over: the same audio, the same states
    sch.feed(sid, p["audio"][:CHUNK], is_final=False)
    assert sch.step()[sid].stable == p["states"][0] and asked[-1][1] == [0]
    # a session that is closed and a new one on the slot: a new tracker
    sch.close(sid)
    sid = sch.open()
    sch.feed(sid, p["audio"][:CHUNK], is_final=False)
    assert sch.step()[sid].stable == p["states"][0] and asked[-1][1] == [0]


def test_scheduler_option_composes_and_is_off_by_default(lockstep):
    p = lockstep
    both = StreamScheduler(_spec_batch(), None, result_format="espnet", stable_partials=True, draft=True, activity=True)
    sid = both.open()
    both.feed(sid, p["audio"][:CHUNK])
    res = both.step()[sid]
    assert isinstance(res, StableResults) and isinstance(res, DraftResults)
    assert res.stable == p["states"][0] and res.draft is not None and res.activity is not None
    plain = StreamScheduler(_spec_batch(), None, result_format="espnet")
    sid = plain.open()
    plain.feed(sid, p["audio"][:CHUNK])
    res = plain.step()[sid]
    assert not hasattr(res, "stable") and not isinstance(res, StableResults)
    # a beam wider than the comparison takes is refused when the option is asked for, not at the first reply
    from oracle.kernel_spec import SpecBackend
    wide = make_batch(MODEL, "TINY", SpecBackend(), 1, commit.MAX_HYPS + 1, False, max_frames=64, max_tokens=64,
                      pcm_capacity=1 << 16)
    with pytest.raises(ValueError, match="at most 16"):
        StreamScheduler(wide, None, result_format="espnet", stable_partials=True)
    with pytest.raises(ValueError, match="at most 16"):
        ServerLoop(StreamScheduler(wide, None, result_format="espnet"), vosk_output_format=True, stable_partials=True)
    assert not StreamScheduler(wide, None, result_format="espnet").stable_partials
    # two sessions in one step: one hyps_delta call for both, each reply its own stream's state
    sb = _spec_batch()
    n_calls, real = [], sb.hyps_delta
    sb.hyps_delta = lambda *a, **kw: (n_calls.append(len(a[0])), real(*a, **kw))[1]
    sch = StreamScheduler(sb, None, result_format="espnet", stable_partials=True)
    a, b = sch.open(), sch.open()
    other = scale_server_pcm(_pcm16(audio(6)))
    alone, sp = _spec_batch(), commit.StablePrefix()                 # stream b's audio on a batch of its own
    for k in range(4):
        sch.feed(a, p["audio"][k * CHUNK:(k + 1) * CHUNK])
        sch.feed(b, other[k * CHUNK:(k + 1) * CHUNK])
        out = sch.step()
        alone.push([(0, other[k * CHUNK:(k + 1) * CHUNK], False)])
        # (the spec backend's fp32 products depend on how many rows a call batches: the scores of a stream decoded beside
        # another differ from its scores alone around 1e-8 - the tokens and the committed length do not)
        for got, want in ((out[a].stable, p["states"][k]),
                          (out[b].stable, sp.update(alone.hyps_delta([0], [sp.next_from])[0]).state())):
            assert (got["committed"], got["tokens"]) == (want["committed"], want["tokens"])
            assert np.allclose(got["stability"], want["stability"], rtol=0, atol=1e-5)
    assert n_calls == [2, 2, 2, 2] and out[b].stable["committed"] > 1


def _text(names, ids):
    """the text hyps_to_results makes of a hypothesis' first tokens: without the <sos> in front, without TEXT_SKIP_IDS"""
    return "".join(names[t] for t in ids[1:] if t not in TEXT_SKIP_IDS).replace("▁", " ").strip()


def test_server_partials_carry_stable_text_and_stability(lockstep):
    p = lockstep
    cfg = p["cfg"]
    names = [f"▁t{i}" for i in range(cfg.vocab_size)]

    def run(**kw):
        sch = StreamScheduler(_spec_batch(), names, result_format="espnet")
        loop = ServerLoop(sch, vosk_output_format=True, finalize_update_iters=100, max_partial_iters=1000, **kw)
        sid = loop.connect()
        out = []
        for k in range(N_CHUNKS - 1):
            loop.submit(sid, p["pcm"][k * CHUNK:(k + 1) * CHUNK])
            out.append(loop.step()[sid])
        loop.submit(sid, '{"eof" : 1}')
        out.append(loop.step()[sid])
        loop.submit(sid, p["pcm"][:CHUNK])                            # the next utterance of the connection
        out.append(loop.step()[sid])
        return out

    replies, off, plain = run(stable_partials=True), run(stable_partials=False), run()
    assert json.dumps(off, sort_keys=True, ensure_ascii=False) == json.dumps(plain, sort_keys=True, ensure_ascii=False)
    # ... and what the messages were before the option existed, recorded: a non-final reply of the reference's result
    # assembly carries no tokens (output_index 0), so every partial is the empty one; the final is the classic result
    for k in list(range(N_CHUNKS - 1)) + [N_CHUNKS]:
        assert off[k] == [{"partial": ""}], k
    (final,) = off[N_CHUNKS - 1]
    assert sorted(final) == ["result", "text"] and len(final["result"]) > 10
    assert sorted(final["result"][0]) == ["conf", "end", "start", "word"]
    assert final["text"] == "".join(w["word"] for w in final["result"]).strip()
    prev, grown = "", 0
    for k in range(N_CHUNKS - 1):
        assert len(replies[k]) == len(plain[k]) == 1
        r, st = replies[k][0], p["states"][k]
        assert sorted(r) == ["partial", "stability", "stable"] and r["partial"] == plain[k][0]["partial"]
        assert r["stable"] == _text(names, st["tokens"][:st["committed"]])
        # the one filter of the transcripts: what hyps_to_results would make of the committed tokens as a final result
        as_final = hyps_to_results([{"yseq": st["tokens"][:st["committed"]], "xpos": [0] * st["committed"]}], True, True,
                                   names, "espnet")
        assert r["stable"] == as_final[0][0]
        assert r["stability"] == st["stability"] and all(0.0 <= v <= 1.0 for v in r["stability"])
        assert r["stable"].startswith(prev)                           # what was stable stays, word for word
        grown += r["stable"] != prev
        prev = r["stable"]
        json.dumps(r)                                                 # plain Python values
    assert grown >= 3 and len(prev.split()) >= 3
    assert replies[N_CHUNKS - 1] == plain[N_CHUNKS - 1] and "stable" not in replies[N_CHUNKS - 1][0]   # finals unchanged
    assert final["text"].startswith(prev) and len(final["text"]) > len(prev)    # the final's text begins with what was stable
    after = replies[N_CHUNKS][0]                                      # the text starts over with the next utterance
    assert after["stable"] == _text(names, p["states"][0]["tokens"][:p["states"][0]["committed"]])
    assert after["partial"] == plain[N_CHUNKS][0]["partial"]
    # with the draft's keys beside them
    both = run(stable_partials=True, draft_partials=True)
    draft = run(draft_partials=True)
    for k in range(N_CHUNKS - 1):
        r = both[k][0]
        assert sorted(r) == ["ahead", "ahead_result", "partial", "stability", "stable"]
        assert {q: r[q] for q in ("ahead", "ahead_result", "partial")} == draft[k][0]
        assert (r["stable"], r["stability"]) == (replies[k][0]["stable"], replies[k][0]["stability"])
    assert both[N_CHUNKS - 1] == plain[N_CHUNKS - 1]
    # not in the plain text protocol
    sch = StreamScheduler(_spec_batch(), names, result_format="espnet")
    assert not ServerLoop(sch, vosk_output_format=False, stable_partials=True).stable_partials
    assert not sch.stable_partials
