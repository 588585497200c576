"""A grammar per stream at stream level (csrc/streams.hip: sc_stream_set_grammar / sc_stream_ctc_beam_grammar;
csrc/stream_readback.hip: sc_ctc_beam_hyps_grammar) on the tiny synthetic model, (B, C) = (8, 8).

As in tests/test_gpu_ctc_beam_streams.py the contract (tests/ctc_beam_grammar_ref.py) is run on the RAW CTC rows of a
handle whose streams are all decoder-free (sc_streams_read_ctc_projected): stream 0 carries grammar A (a looped menu),
stream 1 grammar B (three phrases, no loop), stream 2 none.  Grammar streams: every int32 and every g equal, pb / pnb
within 64 n_frames 2^-53 max(1, |want|), under the condition - asserted first - that every prune gap of the contract's
run is exactly 0 or at least 1e-6.  The stream without a grammar gives the bits of a handle on which no grammar was ever
created.  Everything else is compared bit for bit with that handle: continuous batching at queue depth 2 across a reset
that keeps the grammars, FULL streams beside grammars, and the errors of the setters.

Measured on an MI355X (printed by the test): largest |pb, pnb - contract| 0.0012 of the bar; smallest
non-zero prune gap 4.7e-4; the beam differs from the unconstrained one after 12 of 16 chunks."""
import numpy as np
import pytest

import ctc_beam_grammar_ref as G
import ctc_beam_ref as R
from draft_helpers import make_batch, packed_weights
from speechcatcher_amd import _abi, grammar, ngram, synth
from speechcatcher_amd.native import EngineError
from test_gpu_ctc_beam_streams import BAR, CHUNK, KW, MIN_GAP, NEG, _bits, _chunks, _hyp_bits, _snapshot

pytestmark = pytest.mark.gpu

S, N, BC = 3, 8, (8, 8)
AUDIO_SEEDS = [7, 10, 5]
GRAMMAR_SEED = 3             # (picked on the CPU: the condition holds on the tiny model's tables)


def menus(V, blank, seed=GRAMMAR_SEED):
    """grammar A: a looped menu of 30 phrases of 1 to 4 tokens, one a prefix of another; grammar B: three phrases, no loop"""
    rng = np.random.default_rng(seed)
    toks = [t for t in range(V) if t != blank]
    a = [[int(rng.choice(toks)) for _ in range(int(rng.integers(1, 5)))] for _ in range(30)]
    a.append(a[0] + [int(rng.choice(toks))])
    b = [[int(rng.choice(toks)) for _ in range(n)] for n in (2, 3, 5)]
    return grammar.compile(a, V, blank, loop=True), grammar.compile(b, V, blank, loop=False)


def _snap_gr(sb, s):
    """(the beam's snapshot, the grammar's states beside its entries, (g, complete) of the n-best beside its hypotheses)"""
    return _snapshot(sb, s, BC[0]), sb.ctc_beam_grammar([s])[0], sb.ctc_beam_hyps_grammar([s], BC[0])[s]


def _gr_bits(snap):
    return _bits(snap[0]), snap[1], snap[2]


def _handle(p, none=(), grammars=True, beam=True, **kw):
    sb = make_batch("mixed", "TINY", "native", S, weights=p["w"], **dict(KW, engine=p["engine"], **kw))
    for s in none:
        sb.set_decoder(s, "ctc")
    if beam:
        sb.set_ctc_beam(*BC)
        if grammars:
            sb.set_stream_grammar(0, p["dev"][0])
            sb.set_stream_grammar(1, p["dev"][1])
    return sb


@pytest.fixture(scope="module")
def probe():
    p = {"w": packed_weights("mixed", "TINY", "cuda:0"), "S": S, "n": N}
    p["audio"] = [synth.synth_audio(AUDIO_SEEDS[s], CHUNK * N - 1000 * s) for s in range(S)]
    # a handle on which no grammar is ever created: its beams, and the raw rows
    sb = make_batch("mixed", "TINY", "native", S, weights=p["w"], **KW)
    p["engine"] = sb.engine
    for s in range(S):
        sb.set_decoder(s, "ctc")
    V, blank = sb.cfg.vocab_size, sb.cfg.blank_id
    p["blank"] = blank
    p["blobs"] = menus(V, blank)
    p["gr"] = [grammar.Grammar(b) for b in p["blobs"]]
    early = sb.grammar(p["blobs"][0])
    with pytest.raises(EngineError, match="beam option is off"):
        sb.set_stream_grammar(0, early)
    sb.release_grammar(early)
    sb.set_ctc_beam(*BC)
    with pytest.raises(EngineError, match="no grammar"):
        sb.ctc_beam_grammar([0])
    assert sb.ctc_beam_hyps_grammar([0, 2], 2) == {0: [(-1, None)] * 2, 2: [(-1, None)] * 2}
    wrong_v = sb.grammar(grammar.compile([[1, 2]], V + 1, blank))
    wrong_blank = sb.grammar(grammar.compile([[1, 2]], V, 5))
    for wrong in (wrong_v, wrong_blank):
        with pytest.raises(EngineError, match="vocabulary size or blank"):
            sb.set_stream_grammar(0, wrong)
        sb.release_grammar(wrong)
    p["plain"] = []
    for k in range(N):
        sb.push(_chunks(p, k))
        p["plain"].append([_bits(_snapshot(sb, s, BC[0])) for s in range(S)])
    p["table"] = [sb.read_ctc_projected(s) for s in range(S)]
    # the grammars on the device, shared by every handle below
    p["dev"] = [sb.grammar(b) for b in p["blobs"]]
    with pytest.raises(EngineError, match="grammar blob"):
        sb.grammar(p["blobs"][0][:-3])
    # the all-decoder-free handle with the grammars
    sb = _handle(p, none=range(S))
    first = _snap_gr(sb, 0)
    assert first[1] == [p["gr"][0].start_state] and first[2][0] == (p["gr"][0].start_state, False)
    p["T"], p["snaps"] = [[] for _ in range(S)], []
    for k in range(N):
        sb.push(_chunks(p, k))
        for s in range(S):
            p["T"][s].append(int(sb.st[s].T_enc))
        p["snaps"].append([_snap_gr(sb, s) if s < 2 else _snapshot(sb, s, BC[0]) for s in range(S)])
    assert [np.array_equal(sb.read_ctc_projected(s), p["table"][s]) for s in range(S)] == [True] * S
    p["sb"] = sb
    return p


def test_grammar_streams_equal_the_contract_and_the_others_a_handle_without_grammars(probe):
    p = probe
    B, C = BC
    worst, gap, differs = 0.0, np.inf, 0
    for s in range(2):
        gr = p["gr"][s]
        rws = G.rows(p["table"][s])
        gaps, store = [], []
        state, t_done = G.scan(G.initial(gr), [], store, 1 << 30, B, C, gr, p["blank"]), 0
        for k in range(N):
            t = p["T"][s][k]
            state = G.scan(state, rws[t_done:t], store, 1 << 30, B, C, gr, p["blank"], gaps)
            t_done = t
            near = [g for g in gaps if g != 0.0 and not g >= MIN_GAP]   # the condition, before anything is compared
            assert not near, (s, k, min(near))
            (st, hy), gs, nb = p["snaps"][k][s]
            assert (st["n_frames"], st["n_bad"], st["n_nodes"]) == state[:3], (s, k, st, state[:3])
            assert [e[:4] for e in st["entries"]] == [e[:4] for e in state[3]], (s, k)
            assert gs == list(state[4]), (s, k, gs, state[4])
            for g, w in zip(st["entries"], state[3]):
                for a, b in zip(g[4:], w[4:]):
                    if a == NEG or b == NEG:
                        assert a == b, (s, k, g, w)
                    else:
                        assert abs(a - b) <= BAR(state[0], b), (s, k, a, b)
                        worst = max(worst, abs(a - b) / BAR(state[0], b))
            for r, (h, e) in enumerate(zip(hy, state[3])):           # the pack launch: the contract's backtrace
                assert (h[0], h[1]) == R.backtrace(e, store), (s, k, r)
            # the readers: every entry's ids are a walk of the automaton to its g, complete = the accept flag
            want = [(g, gr.accepts(g)) for g in state[4]] + [(-1, None)] * (B - len(state[4]))
            assert nb == want, (s, k, nb, want)
            for (ids, _, _, _), g in zip(hy, gs):
                assert gr.walk(ids) == g >= 0, (s, k, ids, g)
            differs += p["plain"][k][s][1] != [e[:4] for e in state[3]]
        gap = min([gap] + [g for g in gaps if g != 0.0])
        # content: at the final the best complete entry is accepted by the host walk
        (st, hy), gs, nb = p["snaps"][-1][s]
        complete = [r for r, (_, acc) in enumerate(nb) if acc]
        assert complete, (s, nb)
        assert gr.accepts(gr.walk(hy[complete[0]][0])) and len(hy[complete[0]][0]) >= 1
    for k in range(N):                                               # the stream without a grammar
        assert _bits(p["snaps"][k][2]) == p["plain"][k][2], k
    print(f"\nTINY-mixed B, C = {BC}: grammar A {p['gr'][0].n_states} states, B {p['gr'][1].n_states}; smallest non-zero "
          f"prune gap {gap:.3e}; largest |pb, pnb - contract| = {worst:.4f} of the bar; the beam differs from the "
          f"unconstrained one after {differs} of {2 * N} chunks")
    assert differs > 0
    sb = p["sb"]
    # a reset keeps the grammar: the next utterance starts clean in its start state, the other streams keep their states
    sb.reset(0)
    assert _gr_bits(_snap_gr(sb, 0))[1:] == ([p["gr"][0].start_state], [(p["gr"][0].start_state, False)] + [(-1, None)] * 7)
    assert _gr_bits(_snap_gr(sb, 1)) == _gr_bits(p["snaps"][-1][1])
    sb.push(_chunks(p, 0, [0]))
    sb.push(_chunks(p, 1, [0]))
    sb.push(_chunks(p, 2, [0]))
    assert _gr_bits(_snap_gr(sb, 0)) == _gr_bits(p["snaps"][2][0])


def test_a_batch_at_queue_depth_2_across_a_reset_that_keeps_the_grammars_is_bit_identical(probe):
    p = probe
    sb = _handle(p, none=range(S), strict_reference=False)
    sb.set_queue_depth(2)
    for rnd, n in enumerate((N, 3)):                                 # the whole utterance; a reset; its first chunks again
        nxt, rep, queued_behind = [0] * S, [0] * S, 0

        def feed(s):
            k = nxt[s]
            nxt[s] += 1
            return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == N - 1)

        sb.submit([feed(s) for s in range(S)])
        with pytest.raises(EngineError, match="outstanding"):
            sb.set_stream_grammar(0, None)                           # refused while chunks are outstanding
        sb.submit([feed(s) for s in range(S)])
        while sb.outstanding:
            done = sb.poll(1)
            for s in sorted(done):
                queued_behind += nxt[s] > rep[s] + 1
                if s < 2:
                    assert _gr_bits(_snap_gr(sb, s)) == _gr_bits(p["snaps"][rep[s]][s]), (rnd, s, rep[s])
                else:
                    assert _bits(_snapshot(sb, s, BC[0])) == p["plain"][rep[s]][s], (rnd, rep[s])
                rep[s] += 1
            again = [feed(s) for s in sorted(done) if nxt[s] < n]
            if again:
                sb.submit(again)
        assert rep == [n] * S and queued_behind >= S
        for s in range(S):
            sb.reset(s)


def test_full_streams_do_not_depend_on_grammars_beside_them(probe):
    p = probe
    runs = {}
    for what, kw in {"grammars": dict(), "no grammar": dict(grammars=False), "beam off": dict(beam=False)}.items():
        sb = _handle(p, **kw)
        hyps = []
        for k in range(N):
            sb.push(_chunks(p, k))
            hyps.append(_hyp_bits(sb, range(S)))
            if what == "grammars":                                   # FULL streams: the beam is a side result, the same one
                for s in range(2):
                    assert _gr_bits(_snap_gr(sb, s)) == _gr_bits(p["snaps"][k][s]), (k, s)
                assert _bits(_snapshot(sb, 2, BC[0])) == p["plain"][k][2], k
            if what == "no grammar":
                assert [_bits(_snapshot(sb, s, BC[0])) for s in range(S)] == p["plain"][k], k
        assert all(int(sb.st[s].n_steps_total) > 0 for s in range(S))
        runs[what] = hyps
    assert runs["grammars"] == runs["no grammar"] == runs["beam off"]
    assert len(runs["grammars"][-1][0][0][0]) > 1                    # (yseq of stream 0's best hypothesis)


def test_the_setters_errors_and_the_use_count(probe):
    p = probe
    lib = _abi.load()
    sb = _handle(p, none=[1], grammars=False)
    mine = sb.grammar(p["blobs"][1])
    sb.set_stream_grammar(1, mine)
    sb.set_stream_grammar(2, mine)
    assert lib.sc_grammar_destroy(mine.handle) == -1 and b"in use" in lib.sc_last_error()
    # grammar and model together: refused in both directions
    V = sb.cfg.vocab_size
    model = ngram.pack({(1,): (-1.0, -0.5)}, V)
    with pytest.raises(EngineError, match="grammar"):
        sb.set_ctc_beam_lm(model, 0.5, 0.0)
    sb.set_stream_grammar(1, None)
    with pytest.raises(EngineError, match="in use"):
        sb.release_grammar(mine)                                     # stream 2 still names it
    sb.set_stream_grammar(2, None)
    sb.set_ctc_beam_lm(model, 0.5, 0.0)
    with pytest.raises(EngineError, match="language model is attached"):
        sb.set_stream_grammar(1, mine)
    sb.set_ctc_beam_lm(None)
    sb.set_stream_grammar(1, mine)
    # after audio was taken
    sb.push([(1, p["audio"][1][:CHUNK], False)])
    with pytest.raises(EngineError, match="buffered audio"):
        sb.set_stream_grammar(1, None)
    with pytest.raises(EngineError, match="in use"):
        sb.release_grammar(mine)
    # switching the beam option off drops every stream's grammar
    sb.reset(1)
    sb.set_ctc_beam(0)
    sb.release_grammar(mine)
    assert mine.handle is None
    sb.set_ctc_beam(*BC)
    with pytest.raises(EngineError, match="no grammar"):
        sb.ctc_beam_grammar([1])
