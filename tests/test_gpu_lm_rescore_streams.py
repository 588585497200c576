"""N-gram rescoring at stream level (csrc/stream_readback.hip: sc_rescore_hyps, sc_lm_rescore_lists) on the tiny
synthetic model, with an order-3 model estimated from the streams' own hypotheses.

sc_rescore_hyps on FULL streams equals the contract (tests/lm_rescore_ref.py) run on what sc_get_hyps_batch returned,
every output bit for bit: at partials (no end term) and at the final (with it), under continuous batching at queue depth
2 (the snapshot path) and across a reset.  The hypotheses and their scores are bit-identical with and without the calls,
with the model created and destroyed in between.  On an all-decoder-free handle with the model fused into the beam (8k),
sc_lm_rescore_lists over sc_ctc_beam_hyps reproduces the beam's own lm and ctx bit for bit, and its order with the end
term is the contract's."""
import numpy as np
import pytest

import ctc_beam_ref as R
import lm_rescore_ref as RS
import ngram_ref as NR
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import ngram, synth
from speechcatcher_amd.native import EngineError
from test_gpu_ctc_beam_streams import CHUNK, KW, _chunks, _hyp_bits

pytestmark = pytest.mark.gpu

S, N, W = 2, 8, 5
ALPHA, BETA = 0.5, 0.3
AUDIO_SEEDS = [7, 10]
COUNT = {"lists": 0, "flipped": 0}


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).tolist()


def _batch(p, **kw):
    return make_batch("mixed", "TINY", "native", S, beam=W, weights=p["w"], **dict(KW, engine=p.get("engine"), **kw))


def _check(p, sb, streams, final, model=None):
    """sc_rescore_hyps of the listed streams against the contract on what sc_get_hyps_batch returns for them"""
    dev = model if model is not None else sb.language_model(p["blob"])
    a = sb.hypotheses_arrays(streams)
    got = sb.rescore_hyps(streams, dev, ALPHA, BETA, lm_eos=p["eos"], final=final)
    again = sb.hypotheses_arrays(streams)
    assert all(a[k].tobytes() == again[k].tobytes() for k in a)     # the call changed nothing
    if model is None:
        dev.close()                                                  # (the call had synchronised)
    for i, s in enumerate(streams):
        nh = int(a["n_hyps"][i])
        g = got[int(s)]
        assert len(g["order"]) == nh
        if nh == 0:
            continue
        want = RS.rescore(p["lm"], a["ids"][i, :nh], a["score"][i, :nh], a["lens"][i, :nh], a["ids"].shape[2], skip=1,
                          strip=p["eos"], lm_eos=p["eos"] if s in final else -1, alpha=ALPHA, beta=BETA)
        for key in ("fused", "lm", "eos_lm"):
            assert _u64(g[key]) == _u64(want[key]), (s, key, g[key], want[key])
        assert g["order"].tolist() == want["order"].tolist() and g["status"].tolist() == want["status"].tolist(), s
        assert bool(want["eos_lm"].any()) == (s in final), (s, want["eos_lm"])
        COUNT["lists"] += 1
        COUNT["flipped"] += int(want["order"][0] != 0)


@pytest.fixture(scope="module")
def probe():
    p = {"w": packed_weights("mixed", "TINY", "cuda:0"), "S": S, "n": N}
    p["audio"] = [synth.synth_audio(AUDIO_SEEDS[s], CHUNK * N - 1000 * s) for s in range(S)]
    # a handle that is never rescored: the hypotheses after every chunk, and the sentences the model is estimated from
    sb = _batch(p)
    p["engine"] = sb.engine
    p["eos"], V = sb.cfg.eos_id, sb.cfg.vocab_size
    p["hyps"], sents = [], []
    for k in range(N):
        sb.push(_chunks(p, k))
        p["hyps"].append(_hyp_bits(sb, range(S)))
        a = sb.hypotheses_arrays(range(S))
        for i in range(S):
            for h in range(int(a["n_hyps"][i])):
                y = RS.labels(a["ids"][i, h], int(a["lens"][i, h]), 1, p["eos"])
                if y:
                    sents.append(y + [p["eos"]])
    assert len(sents) > 20 and max(map(len, sents)) > 4
    p["blob"] = ngram.pack(NR.estimate(sents, V, 3), V, 3)
    p["lm"] = ngram.Blob(p["blob"])
    assert p["lm"].order == 3 and p["lm"].n_arcs > 20
    return p


def test_full_streams_in_lockstep_equal_the_contract_and_their_hypotheses_do_not_change(probe):
    p = probe
    sb = _batch(p)
    other = ngram.pack({}, sb.cfg.vocab_size + 1)
    for k in range(N):
        sb.push(_chunks(p, k))
        _check(p, sb, list(range(S)), final=list(range(S)) if k == N - 1 else [])
        _check(p, sb, [1], final=[1])                                # one stream of the batch, with the end term
        assert _hyp_bits(sb, range(S)) == p["hyps"][k], k            # the model was created and destroyed in between
    dev = sb.language_model(p["blob"])
    with pytest.raises(EngineError, match="listed twice"):
        sb.rescore_hyps([0, 0], dev)
    with pytest.raises(EngineError, match="finite"):
        sb.rescore_hyps([0], dev, alpha=float("nan"))
    with pytest.raises(EngineError, match="lm_eos"):
        sb.rescore_hyps([0], dev, lm_eos=sb.cfg.vocab_size)
    with pytest.raises(EngineError, match="vocabulary"):
        sb.rescore_hyps([0], sb.language_model(other))
    sb.reset(0)                                                      # a stream without hypotheses: an empty list
    assert len(sb.rescore_hyps([0, 1], dev)[0]["order"]) == 0
    _check(p, sb, [0, 1], final=[1], model=dev)
    sb.push(_chunks(p, 0, [0]))
    _check(p, sb, [0, 1], final=[], model=dev)
    assert _hyp_bits(sb, [0])[0] == p["hyps"][0][0]
    sb.submit([(0, p["audio"][0][CHUNK:2 * CHUNK], True)])           # a chunk that has not been reported yet
    for streams in ([0], [1, 0]):
        with pytest.raises(EngineError, match="inside a decode block"):
            sb.rescore_hyps(streams, dev)
    while sb.outstanding:
        sb.poll(1)
    _check(p, sb, [0, 1], final=[0], model=dev)
    dev.close()
    print(f"\nthe fused best is not the acoustic best in {COUNT['flipped']} of {COUNT['lists']} lists "
          f"(alpha {ALPHA}, beta {BETA}, beam {W}; the weights are parameters, not tuned)")


def test_continuous_batching_at_queue_depth_2_across_a_reset_reads_the_snapshot(probe):
    p = probe
    sb = _batch(p)
    sb.set_queue_depth(2)
    dev = sb.language_model(p["blob"])
    for rnd, n in enumerate((N, 3)):                                 # the whole utterance; a reset; its first chunks again
        nxt, rep, queued_behind = [0] * S, [0] * S, 0

        def feed(s):
            k = nxt[s]
            nxt[s] += 1
            return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == N - 1)

        sb.submit([feed(s) for s in range(S)])
        sb.submit([feed(s) for s in range(S)])
        while sb.outstanding:
            done = sb.poll(1)
            for s in sorted(done):
                queued_behind += nxt[s] > rep[s] + 1
                _check(p, sb, [s], final=[s] if rep[s] == N - 1 else [], model=dev)
                assert _hyp_bits(sb, [s])[s] == p["hyps"][rep[s]][s], (rnd, s, rep[s])
                rep[s] += 1
            again = [feed(s) for s in sorted(done) if nxt[s] < n]
            if again:
                sb.submit(again)
        assert rep == [n] * S and queued_behind >= S
        for s in range(S):
            sb.reset(s)
    dev.close()


def test_decoder_free_finals_get_their_end_term_from_rescore_lists(probe):
    p = probe
    sb = _batch(p)
    for s in range(S):
        sb.set_decoder(s, "ctc")
    sb.set_ctc_beam(8, 8)
    sb.set_ctc_beam_lm(p["blob"], ALPHA, BETA)
    for k in range(N):
        sb.push(_chunks(p, k))
    dev = sb.language_model(p["blob"])
    hyps = sb.ctc_beam_hyps(list(range(S)), 8)
    side = sb.ctc_beam_lm(list(range(S)))
    lists = [[h["ids"] for h in hyps[s]] for s in range(S)]
    totals = [[R.lae(h["pb"], h["pnb"]) for h in hyps[s]] for s in range(S)]
    assert all(len(li) == 8 and max(map(len, li)) > 3 for li in lists)
    plain = sb.rescore_lists(lists, totals, dev, ALPHA, BETA)
    ended = sb.rescore_lists(lists, totals, dev, ALPHA, BETA, lm_eos=p["eos"])
    for s in range(S):
        assert _u64(plain[s]["lm"]) == _u64(side[s]["lm"]) == _u64(ended[s]["lm"]), s      # the beam's own sums
        assert plain[s]["end_state"].tolist() == side[s]["ctx"], s
        assert plain[s]["order"].tolist() == list(range(8)) or len(set(side[s]["fused"])) < 8   # the beam is kept by fused
        L = max(map(len, lists[s]))
        rows = [y + [0] * (L - len(y)) for y in lists[s]]
        for got, eos in ((plain[s], -1), (ended[s], p["eos"])):
            want = RS.rescore(p["lm"], rows, totals[s], [len(y) for y in lists[s]], L, skip=0, lm_eos=eos, alpha=ALPHA,
                              beta=BETA)
            for key in ("fused", "lm", "eos_lm"):
                assert _u64(got[key]) == _u64(want[key]), (s, key)
            for key in ("order", "status", "end_state"):
                assert got[key].tolist() == want[key].tolist(), (s, key)
        assert ended[s]["eos_lm"].all()
    # lists of other shapes: an empty list, an empty row, a given state
    odd = sb.rescore_lists([[], [[], [3, 4]]], [[], [-1.0, -2.0]], dev, 1.0, 0.0, state0=[-1, 2])
    want = RS.rescore(p["lm"], [[0, 0], [3, 4]], [-1.0, -2.0], [0, 2], 2, skip=0, state0=2, alpha=1.0)
    assert len(odd[0]["order"]) == 0 and _u64(odd[1]["fused"]) == _u64(want["fused"])
    assert odd[1]["end_state"].tolist() == want["end_state"].tolist() == [2, int(want["end_state"][1])]
    with pytest.raises(EngineError, match="state0"):
        sb.rescore_lists([[[1]]], [[0.0]], dev, state0=[p["lm"].n_states])
    dev.close()
