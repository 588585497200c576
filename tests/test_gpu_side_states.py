"""The per-chunk side states of the C++ engine with every option on together (csrc/handover.h, csrc/streams.hip: acoustic
activity, phrase spotting, draft transcript and the input level share one span list, one arena slot and one hand-over):
one handle with all four on, at queue depth 2, against handles with exactly one option on that are pushed in lock-step -
bit for bit after every reported chunk -, and across a reset of one stream while the other is in mid-utterance.

The handles are built with strict_reference=False: after a strict reset the reference's stale CTC table stays, the frames
below its extent are not projected again, and a second, shorter utterance would be scanned by no option at all."""
import numpy as np
import pytest

import ctc_activity_ref as RA
import ctc_draft_ref as RD
import ctc_spot_ref as RS
import pcm_ref as RP
from draft_helpers import make_batch, packed_weights, path_mix
from spot_helpers import choose_floors, phrases_from_paths
from speechcatcher_amd import pcm, synth
from test_gpu_ctc_draft import CHUNK, KW, MIN_GAP, SEEDS

pytestmark = pytest.mark.gpu

NAME, MODEL = "TINY", "mixed"      # the blank wins a third of the frames: speech and silence, tokens, phrases to cut
S, N, N2 = 2, 8, 3                 # streams, chunks of the first utterances, chunks of stream 0's second utterance
N_PHRASES = 8
OPTIONS = ("activity", "spot", "draft", "level")
FMT = (RP.S16LE, 1, 0, RP.SCALE_FULL)
ARGS = dict(KW, strict_reference=False)


def _s16(x):
    return np.clip(np.round(np.asarray(x, np.float64) * 32767), -32768, 32767).astype("<i2").tobytes()


def _switch_on(sb, opts, p):
    if "activity" in opts:
        sb.set_activity(True, p["thr"])
    if "spot" in opts:
        sb.set_phrases(p["phrases"], p["floors"])
    if "draft" in opts:
        sb.set_draft(True)
    if "level" in opts:
        sb.set_input_format(1, *FMT)


def _hyps(sb, s):
    """(floats compare exactly; not hypotheses_arrays: its padding depends on the queue depth)"""
    return [(h["yseq"], h["xpos"], h["score"], h["score_dec"], h["score_ctc"]) for h in sb.hypotheses(s)]


def _read(sb, s, opt):
    """the state of stream s's last reported chunk as one option reports it, in a form that compares bit for bit"""
    if opt == "activity":
        a = sb.activity([s])
        return tuple(int(a[k][0]) for k in RA.FIELDS), sb.read_activity(s).tobytes()
    if opt == "spot":
        c = sb.spot([s])
        return int(c["n_frames"][0]), int(c["n_events"][0]), RS.events_bytes(sb.spot_events(s))
    if opt == "draft":
        d = sb.draft([s])
        toks = sb.draft_tokens(s)
        return (tuple(int(d[k][0]) for k in RD.FIELDS[:6]),
                np.asarray([float(d["open_conf"][0])] + [v for t in toks for v in t], np.float64).tobytes())
    if opt == "level":
        return sb.input_level(s)
    return _hyps(sb, s)


INITIAL = {"activity": (tuple(RA.INITIAL), b""), "spot": (0, 0, RS.events_bytes([])),
           "draft": (tuple(RD.INITIAL[:6]), np.asarray([RD.INITIAL[6]], np.float64).tobytes()), "level": RP.ZERO_LEVEL}


def _lockstep(p, feeds, coded, opts=("hyps",) + OPTIONS):
    """per option a handle of its own with exactly that option on ("hyps": none), pushed chunk by chunk in lock-step ->
    {option: [k][stream] the state after chunk k}, and the "hyps" handle.  feeds: {stream: [(floats, is_final)]}; coded:
    {stream: [bytes]} for the streams whose input has a format on the "level" handle."""
    out, plain = {}, None
    for opt in opts:
        sb = make_batch(MODEL, NAME, p["backend"], S, weights=p["w"], **dict(ARGS, **p["share"]))
        if p["backend"] == "native":
            p["share"]["engine"] = sb.engine                         # (the weights are uploaded once)
        _switch_on(sb, (opt,), p)
        snaps = []
        for k in range(max(len(f) for f in feeds.values())):
            items = [(s, coded[s][k] if opt == "level" and s in coded else f[k][0], f[k][1]) for s, f in feeds.items() if k < len(f)]
            sb.push(items)
            snaps.append({s: _read(sb, s, opt) for s, _, _ in items})
        out[opt] = snaps
        if opt == "hyps":
            plain = sb
    return out, plain


def _cut(x, n):
    return [(x[k * CHUNK:(k + 1) * CHUNK], k == n - 1) for k in range(n)]


def build_probe(backend="native", device="cuda:0"):
    """computed once: the audio (stream 1's as the floats its s16le codes decode to, so that every handle sees the same
    samples), the phrase set cut from the CTC tables read back, and the lock-step states of the single-option handles for
    the first utterances of both streams and for the second utterance of stream 0 on fresh handles"""
    p = {"backend": backend, "w": packed_weights(MODEL, NAME, device), "share": {}}
    raw = [synth.synth_audio(SEEDS[NAME][s], CHUNK * N - 1000 * s) for s in range(S)]
    codes = _s16(raw[1])
    audio = [raw[0], pcm.decode(codes, *FMT)]
    second = synth.synth_audio(SEEDS[NAME][0], CHUNK * N2 - 700)[::-1].copy()     # (the same seed's audio, backwards)
    p["feeds"] = {0: _cut(audio[0], N), 1: _cut(audio[1], N)}
    p["coded"] = {1: [codes[2 * k * CHUNK:2 * (k + 1) * CHUNK] for k in range(N)]}
    p["feeds2"] = {0: _cut(second, N2)}
    assert all(len(c) == 2 * len(f[0]) for c, f in zip(p["coded"][1], p["feeds"][1]))
    # the tables: of a handle with every option off (its hypotheses are what the options must not change)
    hyp1, plain = _lockstep(p, p["feeds"], {}, opts=("hyps",))
    tables = [plain.read_ctc(s) for s in range(S)]
    hyp2, plain2 = _lockstep(p, p["feeds2"], {}, opts=("hyps",))
    tables2 = [plain2.read_ctc(0)]
    blank = plain.cfg.blank_id
    gap = np.inf
    for t in tables + tables2:                                        # the condition, before anything is compared
        srt = np.sort(t, 1)
        gap = min(gap, float((srt[:, -1] - srt[:, -2]).min()))
    print(f"\nsmallest gap between a row's best entry and its runner-up {gap:.3e}; rows {[len(t) for t in tables + tables2]}")
    assert gap >= MIN_GAP
    for t in tables:
        path_mix(MODEL, t, blank)
    phrases = phrases_from_paths(tables, blank, 2 * N_PHRASES, lengths=(2, 3, 4, 5))
    p["phrases"], p["floors"] = choose_floors(tables, blank, phrases, N_PHRASES)
    # the activity threshold: in the widest gap of the middle half of the blank posteriors of both streams (this model's
    # rows are nearly flat: the blank wins a frame with a posterior of a few percent)
    pb = np.sort(np.concatenate([RA.p_blank(t, blank) for t in tables]))
    mid = pb[len(pb) // 4:3 * len(pb) // 4]
    i = int(np.argmax(np.diff(mid)))
    p["thr"] = float(0.5 * (mid[i] + mid[i + 1]))
    assert 0.0 < p["thr"] < 1.0
    p["ref"], _ = _lockstep(p, p["feeds"], p["coded"], opts=OPTIONS)
    p["ref2"], _ = _lockstep(p, p["feeds2"], {}, opts=OPTIONS)
    p["ref"]["hyps"], p["ref2"]["hyps"] = hyp1["hyps"], hyp2["hyps"]
    # the options have something to hand over: speech and silence, events, closed tokens, a level
    last = {o: p["ref"][o][N - 1] for o in OPTIONS}
    assert all(0 < last["activity"][s][0][1] < last["activity"][s][0][0] for s in range(S)), last["activity"]
    assert sum(last["spot"][s][1] for s in range(S)) >= 2 and all(last["draft"][s][0][1] >= 4 for s in range(S))
    assert last["level"][1]["frames"] == len(audio[1]) and last["level"][0] == RP.ZERO_LEVEL
    assert p["ref2"]["draft"][N2 - 1][0][0][1] >= 1 and p["ref2"]["activity"][N2 - 1][0][0][0] > 0
    return p


@pytest.fixture(scope="module")
def probe():
    return build_probe()


def test_all_options_on_at_queue_depth_2_equal_the_single_option_handles_across_a_reset(probe):
    p = probe
    every = ("hyps",) + OPTIONS
    sb = make_batch(MODEL, NAME, "native", S, weights=p["w"], **dict(ARGS, **p["share"]))
    sb.set_queue_depth(2)
    _switch_on(sb, OPTIONS, p)
    for s in range(S):
        assert all(_read(sb, s, o) == INITIAL[o] for o in OPTIONS)
    # per stream: the chunks still to submit and those at the engine, as (payload, is_final, reference, chunk index)
    todo = {s: [(p["coded"][s][k] if s in p["coded"] else f[k][0], f[k][1], p["ref"], k) for k in range(N)]
            for s, f in p["feeds"].items()}
    at_engine = {s: [] for s in range(S)}
    active, reported, queued_behind, through, seen_reset = [0], [0] * S, 0, False, False
    last1 = None

    def top_up():
        for _ in range(2):
            items = []
            for s in active:
                if todo[s] and len(at_engine[s]) < 2:
                    at_engine[s].append(todo[s].pop(0))
                    items.append((s,) + at_engine[s][-1][:2])
            if items:
                sb.submit(items)

    top_up()
    while sb.outstanding:
        done = sb.poll(1)
        for s in sorted(done):
            assert not isinstance(done[s], Exception), (s, done[s])
            _, fin, ref, k = at_engine[s].pop(0)
            queued_behind += len(at_engine[s]) > 0                   # a later chunk of the stream is at the engine
            got = {o: _read(sb, s, o) for o in every}                # the states of the chunk that was REPORTED
            for o in every:
                assert got[o] == ref[o][k][s], (o, s, k, "second utterance" if ref is p["ref2"] else "first utterance")
            reported[s] += 1
            if s == 1:
                last1 = got
            through = through or (s == 0 and fin and ref is p["ref"])
        if through and not seen_reset:
            # stream 0's first utterance is through, stream 1 is in mid-utterance with chunks at the engine
            assert 0 < reported[1] < N and at_engine[1] and last1 is not None
            sb.reset(0)
            assert all(_read(sb, 0, o) == INITIAL[o] for o in OPTIONS)
            # stream 1 is undisturbed (its hypotheses are compared with its next reply: they cannot be read again now)
            assert {o: _read(sb, 1, o) for o in OPTIONS} == {o: last1[o] for o in OPTIONS}
            todo[0] = [(f[0], f[1], p["ref2"], k) for k, f in enumerate(p["feeds2"][0])]
            seen_reset = True
        if reported[0] >= 3 and 1 not in active:
            active.append(1)                                         # stream 1 starts three chunks behind stream 0
        top_up()
    assert seen_reset and reported == [N + N2, N] and not any(todo.values())
    assert queued_behind >= S
