"""CTC phrase spotting on the CPU: the numpy contract (tests/ctc_spot_ref.py) and its properties, the engines' host-side
recurrence against it, and the Python lock-step engine / scheduler / server loop on the spec backend."""
import numpy as np
import pytest

import ctc_spot_ref as R
from spot_helpers import ctc_path, make_batch, choose_floors, phrases_from_paths, plant_table, random_phrases, trace_end_values
from speechcatcher_amd import spotting, synth
from speechcatcher_amd.align import FeatureClock
from speechcatcher_amd.scheduler import SpottingResults, StreamScheduler
from speechcatcher_amd.server_session import ServerLoop, scale_server_pcm

V, BLANK = 67, 0
A, B, C = 5, 9, 40


def _scan(x, phrases, floors, mask=R.ALL, state=None):
    return R.scan(state if state is not None else R.initial(len(phrases)), x, BLANK, phrases, np.asarray(floors, float), mask)


def _row(hot, level=0.0, rest=-30.0):
    """a row whose entries `hot` (label -> offset below the maximum) are set, the rest far below"""
    x = np.full(V, rest, np.float32)
    for lab, off in hot.items():
        x[lab] = level - off
    return x


# ---- the contract's own properties ------------------------------------------------------------------------------------
def test_planted_phrases_fire_once_each_at_the_planted_frames():
    rng = np.random.default_rng(0)
    phrases = [[A, B, C], [B, B, A], [C + 1]]
    x, ends = plant_table(rng, 200, V, BLANK, [(20, phrases[0]), (80, phrases[1]), (150, phrases[2])])
    st = _scan(x, phrases, [-2.0, -2.0, -1.0])
    assert [(e[0], e[1], e[2]) for e in st["events"]] == [(ends[0], 0, 20), (ends[1], 1, 80), (ends[2], 2, 150)]
    assert st["n_frames"] == 200 and st["n_events"] == 3 and all(-2.0 <= e[3] <= 0.0 for e in st["events"])
    assert len(ctc_path(phrases[1], BLANK)) == 4 and ends[1] == 83     # the adjacent repeat takes its blank


@pytest.mark.parametrize("seed", range(4))
def test_any_split_gives_the_states_and_events_of_one_span(seed):
    rng = np.random.default_rng(seed)
    T = 200
    phrases = random_phrases(rng, 5, V, BLANK, (1, 2, 3, 6, 32))
    plants = [(10, phrases[1]), (30, phrases[2]), (50, phrases[3]), (70, phrases[4]), (150, phrases[2]), (160, phrases[0])]
    x, _ = plant_table(rng, T, V, BLANK, plants)
    x[55] = np.nan
    floors = [-2.0 * len(y) for y in phrases]
    one = _scan(x, phrases, floors)
    assert one["n_events"] >= 5
    for _ in range(6):
        cuts = np.sort(rng.integers(0, T + 1, size=5))
        cuts = np.concatenate([[0], cuts, cuts[-1:], [T]]).astype(int)     # six spans and more, empty ones among them
        st = R.initial(len(phrases))
        for a, b in zip(cuts[:-1], cuts[1:]):
            st = _scan(x[a:b], phrases, floors, state=st)
            assert R.same(st, _scan(x[:b], phrases, floors))
        assert R.same(st, one)
    assert R.same(_scan(x[:0], phrases, floors), R.initial(len(phrases)))


def test_a_later_candidate_takes_over_only_if_strictly_greater():
    # phrase A B.  Frame 0 starts a path (start 0); frame 1 costs it one nat at A, so at frame 2 a fresh start (start 2)
    # takes state 0 while the blank state keeps the old path at 0.0.  At frame 3 the end state sees the blank state
    # (value 0, start 0) and the skip from state 0 (value 0, start 2): a tie - the earlier candidate in the order wins.
    rows = [_row({A: 0, BLANK: 0}), _row({A: 1, BLANK: 0}), _row({A: 0, BLANK: 0}), _row({A: 0, BLANK: 0, B: 0})]
    x = np.stack(rows)
    x[:3, B] = -np.inf
    st = _scan(x[:3], [[A, B]], [-0.5])
    assert st["values"][0, :3].tolist() == [0.0, 0.0, -np.inf] and st["starts"][0, :3].tolist() == [2, 0, -1]
    st = _scan(x, [[A, B]], [-0.5])
    assert st["events"] == [(3, 0, 0, 0.0)]
    # stay against a fresh start of the same value: the path that is there keeps its start
    st = _scan(np.stack([_row({A: 0}), _row({A: 0})]), [[A, B]], [-0.5])
    assert st["values"][0, 0] == 0.0 and st["starts"][0, 0] == 0


def test_an_adjacent_repeat_needs_its_blank():
    with_blank = np.stack([_row({B: 0}), _row({BLANK: 0}), _row({B: 0})])
    without = np.stack([_row({B: 0}), _row({B: 0}), _row({B: 0})])
    assert _scan(with_blank, [[B, B]], [-1.0])["events"] == [(2, 0, 0, 0.0)]
    assert _scan(without, [[B, B]], [-1.0])["events"] == []
    assert _scan(without[:2], [[A, B]], [-1.0])["events"] == []          # (and A B needs its A)
    assert _scan(np.stack([_row({A: 0}), _row({B: 0})]), [[A, B]], [-1.0])["events"] == [(1, 0, 0, 0.0)]   # no blank needed


@pytest.mark.parametrize("bad", ["nan", "inf", "all_minus_inf"])
def test_a_bad_row_resets_the_states_and_fires_nothing(bad):
    rows = [_row({A: 0}), _row({B: 0}), _row({C: 0})]
    assert _scan(np.stack(rows), [[A, B, C], [C]], [-1.0, -1.0])["events"] == [(2, 0, 0, 0.0), (2, 1, 2, 0.0)]
    r = _row({B: 0, C: 0})
    if bad == "nan":
        r[3] = np.nan
    elif bad == "inf":
        r[3] = np.inf
    else:
        r[:] = -np.inf
    st = _scan(np.stack([rows[0], r]), [[A, B, C], [C]], [-1.0, -1.0])
    assert st["n_frames"] == 2 and st["n_events"] == 0                   # phrase 1's C did not fire on the bad row
    assert (st["values"] == -np.inf).all() and (st["starts"] == -1).all()
    st = _scan(np.stack([rows[0], r, rows[2]]), [[A, B, C], [C]], [-1.0, -1.0])
    assert st["events"] == [(2, 1, 2, 0.0)]
    # a legal row with -inf entries is not bad
    r = _row({B: 0})
    r[10:40] = -np.inf
    assert _scan(np.stack([rows[0], r, rows[2]]), [[A, B, C]], [-1.0])["events"] == [(2, 0, 0, 0.0)]


def test_a_phrase_rearms_by_itself_after_a_fire():
    occ = [_row({A: 0}), _row({B: 0})]
    x = np.stack(occ + [_row({BLANK: 0})] + occ + occ)
    st = _scan(x[:2], [[A, B]], [-1.0])
    assert st["n_events"] == 1 and (st["values"] == -np.inf).all() and (st["starts"] == -1).all()
    assert _scan(x, [[A, B]], [-1.0])["events"] == [(1, 0, 0, 0.0), (4, 0, 3, 0.0), (6, 0, 5, 0.0)]
    # the same occurrence does not fire twice: B going on after the fire finds no path
    x = np.stack(occ + [_row({B: 0}), _row({B: 0})])
    assert _scan(x, [[A, B]], [-1.0])["n_events"] == 1


def test_two_phrases_on_one_frame_are_ordered_by_phrase_and_the_cap_keeps_the_first_64():
    x = np.stack([_row({A: 0}), _row({B: 0})] * 50)
    st = _scan(x, [[B], [A, B], [B]], [-1.0, -1.0, -1.0])
    assert st["n_events"] == 150 and len(st["events"]) == R.MAX_EVENTS == 64
    assert [(e[0], e[1]) for e in st["events"][:6]] == [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)]
    assert st["events"] == sorted(st["events"], key=lambda e: (e[0], e[1]))
    assert st["events"][-1][:2] == (43, 0)                               # event 63: the 22nd frame that fires, phrase 0


def test_the_mask_leaves_disabled_phrases_untouched():
    x = np.stack([_row({A: 0}), _row({B: 0}), _row({A: 0})])
    phrases, floors = [[A, B], [A, B], [A, C]], [-1.0, -1.0, -1.0]
    st = _scan(x, phrases, floors, mask=0b101)
    assert [(e[0], e[1]) for e in st["events"]] == [(1, 0)]
    assert (st["values"][1] == -np.inf).all() and st["values"][2, 0] == 0.0
    half = _scan(x[:1], phrases, floors)                                  # phrase 1 is under way, then disabled: it keeps
    st = _scan(x[1:], phrases, floors, mask=0b101, state=half)           # its states, also across a bad row
    assert st["values"][1].tobytes() == half["values"][1].tobytes() and st["starts"][1, 0] == 0
    bad = np.full((1, V), np.nan, np.float32)
    st = _scan(bad, phrases, floors, mask=0b101, state=half)
    assert st["values"][1, 0] == 0.0 and (st["values"][[0, 2]] == -np.inf).all()


def test_lengths_1_and_32():
    y = [5 + (i % 7) for i in range(32)]
    x, ends = plant_table(np.random.default_rng(1), 60, V, BLANK, [(3, y)])
    st = _scan(x, [y, [y[-1]], y[:31]], [-8.0, -0.5, -8.0])
    assert (ends[0], 0, 3) in [e[:3] for e in st["events"]] and (ends[0] - 1, 2, 3) in [e[:3] for e in st["events"]]
    assert sum(e[1] == 1 for e in st["events"]) == sum(t == y[-1] for t in y)
    assert all(e[2] == e[0] for e in st["events"] if e[1] == 1)          # L = 1: one state, start = end
    with pytest.raises(AssertionError):
        R.check_phrases([y + [5]], [-1.0], V, BLANK)
    with pytest.raises(AssertionError):
        R.check_phrases([[BLANK]], [-1.0], V, BLANK)
    with pytest.raises(ValueError):
        spotting.PhraseSet([y + [5]], None, V, BLANK)
    with pytest.raises(ValueError):
        spotting.PhraseSet([[V]], None, V, BLANK)
    with pytest.raises(ValueError):
        spotting.PhraseSet([[3]], [0.5], V, BLANK)
    assert spotting.PhraseSet([y, [4]], None, V, BLANK).floors.tolist() == [-64.0, -2.0]


@pytest.mark.parametrize("seed", range(3))
def test_the_engines_recurrence_is_the_contract_bit_for_bit(seed):
    rng = np.random.default_rng(100 + seed)
    P = (1, 17, 64)[seed]
    phrases = random_phrases(rng, P, V, BLANK, (1, 2, 31, 32, 3, 5))
    x, _ = plant_table(rng, 150, V, BLANK, [(4, phrases[0]), (70, phrases[min(P - 1, 2)]), (140, phrases[0])])
    x[30] = np.nan
    x[31, rng.random(V) < 0.5] = -np.inf
    x[32] = np.where(rng.random(V) < 0.5, 1e30, -1e30)
    floors = [-2.0 * len(y) for y in phrases]
    mask = R.ALL if seed == 0 else int(rng.integers(1, 1 << 62)) | 1
    ps = spotting.PhraseSet(phrases, floors, V, BLANK)
    st, want = spotting.initial(P), R.initial(P)
    for a, b in ((0, 1), (1, 64), (64, 64), (64, 150)):
        spotting.advance(st, x[a:b], BLANK, ps, mask)
        want = _scan(x[a:b], phrases, floors, mask, want)
        assert R.same(st, want)
    assert want["n_events"] >= 1
    assert (spotting.MAX_EVENTS, spotting.MAX_PHRASES, spotting.MAX_LEN) == (R.MAX_EVENTS, R.MAX_PHRASES, R.MAX_LEN)


def test_phrase_ids_is_a_greedy_longest_match():
    tokens = ["<blank>", "▁a", "▁agent", "▁ag", "ent", "▁please", "▁pl", "ease", "s", "▁"]
    assert spotting.phrase_ids("agent please", tokens) == [2, 5]
    assert spotting.phrase_ids("agents", tokens) == [2, 8]
    assert spotting.phrase_ids("a  pleases", tokens) == [1, 5, 8]
    with pytest.raises(ValueError):
        spotting.phrase_ids("agent x", tokens)


# ---- the Python engine on the spec backend ---------------------------------------------------------------------------
CHUNK, N_CHUNKS = 10240, 8


def _spec_batch(n_streams=2, **kw):
    from oracle.kernel_spec import SpecBackend
    return make_batch("TINY", SpecBackend(), n_streams, max_frames=400, max_tokens=300, pcm_capacity=1 << 18, **kw)


def _pcm16(audio):
    return np.clip(np.round(audio * 32767.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def probe():
    """one run of stream 0 (what the server feeds: int16 audio scaled back; non-final chunks, then a final one) with a
    placeholder phrase, the RAW rows the engine handed its recurrence recorded: the frames after every chunk, phrases from
    the collapsed arg-max path (its tail included), floors in the widest gaps, and the contract's run over those rows"""
    from speechcatcher_amd import engine
    pcm = _pcm16(synth.synth_audio(5, CHUNK * N_CHUNKS))
    audio = scale_server_pcm(pcm)
    rows, real = [], spotting.advance

    def recorder(state, x, *a, **kw):
        rows.append(np.array(x, np.float32))
        return real(state, x, *a, **kw)

    sb = _spec_batch()
    sb.set_phrases([[1]])
    engine.spotting.advance = recorder
    try:
        T = []
        for k in range(N_CHUNKS):
            sb.push([(0, audio[k * CHUNK:(k + 1) * CHUNK], k == N_CHUNKS - 1)])
            T.append(int(sb.st[0].T_enc))
    finally:
        engine.spotting.advance = real
    table = np.concatenate(rows)
    blank = sb.cfg.blank_id
    assert table.shape == (T[-1], sb.cfg.vocab_size) and T[-1] > 64
    tail = [c[0] for c in R.collapse(np.argmax(table, 1), blank)][-3:]
    phrases = phrases_from_paths([table], blank, 6, lengths=(2, 3, 4)) + [tail[-2:]]
    phrases = [y for i, y in enumerate(phrases) if y not in phrases[:i]]
    phrases, floors = choose_floors([table], blank, phrases)
    ref, vals, snaps = trace_end_values(table, blank, phrases, floors, snap_at=set(T))
    assert min(np.abs(np.asarray(vals[p]) - floors[p]).min() for p in range(len(phrases))) >= 1e-3
    assert 3 <= ref["n_events"] <= R.MAX_EVENTS, ref["n_events"]
    assert any(e[0] >= T[-2] for e in ref["events"]), "a phrase must fire in the frames of the final chunk"
    return {"pcm": pcm, "audio": audio, "T": T, "table": table, "blank": blank, "phrases": phrases, "floors": floors,
            "ref": ref, "snaps": snaps, "cfg": sb.cfg}


def _want(p, k):
    """the contract's stored events over the frames the stream had after chunk k"""
    return p["snaps"][p["T"][k]]["events"]


def _new(p, k):
    """... those of the frames chunk k added"""
    return _want(p, k)[len(_want(p, k - 1)) if k else 0:]


def test_engine_events_equal_the_contract_on_the_rows_it_projected(probe):
    p = probe
    sb = _spec_batch(strict_reference=False)                        # (a reset clears the CTC table: the rows come again)
    with pytest.raises(Exception):
        sb.spot([0])                                                # off by default
    sb.set_phrases(p["phrases"], p["floors"])
    assert sb.spot([0, 1])["n_frames"].tolist() == [0, 0] and sb.spot_events(0) == []
    for k in range(N_CHUNKS):
        sb.push([(0, p["audio"][k * CHUNK:(k + 1) * CHUNK], k == N_CHUNKS - 1)])
        c = sb.spot([0])
        assert (int(c["n_frames"][0]), int(c["n_events"][0])) == (p["T"][k], len(_want(p, k))), k
        assert R.events_bytes(sb.spot_events(0)) == R.events_bytes(_want(p, k)), k
    v, st = sb.read_spot_state(0)
    assert v.tobytes() == p["ref"]["values"].tobytes() and st.tobytes() == p["ref"]["starts"].tobytes()
    assert sb.spot([1])["n_frames"].tolist() == [0]                 # the idle stream
    sb.reset(0)
    assert sb.spot([0])["n_events"].tolist() == [0] and sb.spot_events(0) == []
    # the mask: a disabled phrase does not fire
    off = p["ref"]["events"][0][1]
    sb.set_phrase_mask(0, R.ALL & ~(1 << off))
    for k in range(N_CHUNKS):
        sb.push([(0, p["audio"][k * CHUNK:(k + 1) * CHUNK], k == N_CHUNKS - 1)])
    want = R.scan(R.initial(len(p["phrases"])), p["table"], p["blank"], p["phrases"], p["floors"], R.ALL & ~(1 << off))
    assert R.events_bytes(sb.spot_events(0)) == R.events_bytes(want["events"]) and want["n_events"] < p["ref"]["n_events"]
    sb.set_phrases([])
    with pytest.raises(Exception):
        sb.spot([0])


def test_spotting_does_not_change_the_hypotheses(probe):
    a, b = _spec_batch(), _spec_batch()
    b.set_phrases(probe["phrases"], probe["floors"])
    for k in range(4):
        for sb in (a, b):
            sb.push([(0, probe["audio"][k * CHUNK:(k + 1) * CHUNK], k == 3)])
        assert a.hypotheses(0) == b.hypotheses(0)
    assert len(a.hypotheses(0)[0]["yseq"]) > 1


# ---- scheduler and server loop ----------------------------------------------------------------------------------------
def _clock(p, upto):
    c = FeatureClock(p["cfg"].win_length, p["cfg"].hop_length)
    for k in range(upto + 1):
        c.call(CHUNK, k == N_CHUNKS - 1)
    return c


def test_scheduler_delivers_every_detection_once_and_before_the_reset_after_a_final(probe):
    p = probe
    sb = _spec_batch(strict_reference=False)
    sch = StreamScheduler(sb, None, result_format="espnet", phrases=p["phrases"], min_scores=p["floors"])
    sid = sch.open()
    got = []
    for k in range(N_CHUNKS):
        sch.feed(sid, p["audio"][k * CHUNK:(k + 1) * CHUNK], is_final=k == N_CHUNKS - 1)
        res = sch.step()[sid]
        assert isinstance(res, SpottingResults) and isinstance(res, list)
        new = _new(p, k)                                                            # the events of this chunk's frames
        assert [(d["end"], d["phrase"], d["start"], d["score"]) for d in res.detections] == new, k
        cfg, clock = p["cfg"], _clock(p, k)
        for d in res.detections:                                                     # seconds: the frames' sample spans
            assert d["start_s"] == clock.frame_span(d["start"], cfg.subsample)[0] / cfg.sample_rate
            assert d["end_s"] == clock.frame_span(d["end"], cfg.subsample)[1] / cfg.sample_rate
            assert 0.0 <= d["start_s"] < d["end_s"] <= (k + 1) * CHUNK / 16000 + 0.05
            assert d["end_s"] >= 0.04 * (d["end"] + 1) - 1e-9                       # (calls in the middle lose frames)
        got += res.detections
    assert len(got) == p["ref"]["n_events"] and len(res.detections) >= 1               # ... some of them in the final reply,
    assert sb.spot([0])["n_events"].tolist() == [0]                                     # read before the reset
    # the next utterance of the session starts over: the same audio, the same detections
    sch.feed(sid, p["audio"][:CHUNK], is_final=False)
    assert [(d["end"], d["phrase"]) for d in sch.step()[sid].detections] == [(e[0], e[1]) for e in _want(p, 0)]
    # without the option: plain replies
    plain = StreamScheduler(_spec_batch(), None, result_format="espnet")
    sid = plain.open()
    plain.feed(sid, p["audio"][:CHUNK])
    assert not hasattr(plain.step()[sid], "detections")


def test_server_loop_emits_spotted_messages_in_front_of_the_partial(probe):
    p = probe
    names = {f"phrase {i}": y for i, y in enumerate(p["phrases"])}
    floors = {f"phrase {i}": float(f) for i, f in enumerate(p["floors"])}

    def run(spot):
        sch = StreamScheduler(_spec_batch(), None, result_format="espnet")
        loop = ServerLoop(sch, finalize_update_iters=100, max_partial_iters=1000, spotting=names if spot else None,
                          spotting_min_scores=floors if spot else None)
        sid = loop.connect()
        out = []
        for k in range(N_CHUNKS - 1):
            loop.submit(sid, p["pcm"][k * CHUNK:(k + 1) * CHUNK])
            out.append(loop.step()[sid])
        return out

    replies, plain = run(True), run(False)
    cfg = p["cfg"]
    for k in range(N_CHUNKS - 1):
        new = _new(p, k)
        assert len(plain[k]) == 1 and replies[k][-1] == plain[k][0]                  # the partial of today, last
        if not new:
            assert len(replies[k]) == 1
            continue
        assert len(replies[k]) == 2 and list(replies[k][0]) == ["spotted"]
        clock = _clock(p, k)
        assert replies[k][0]["spotted"] == [
            {"phrase": f"phrase {e[1]}", "start": round(clock.frame_span(e[2], cfg.subsample)[0] / cfg.sample_rate, 3),
             "end": round(clock.frame_span(e[0], cfg.subsample)[1] / cfg.sample_rate, 3), "score": e[3]} for e in new]
    assert sum(len(r) == 2 for r in replies) >= 2
    with pytest.raises(ValueError):
        ServerLoop(StreamScheduler(_spec_batch(), None, result_format="espnet"), strict_reference=True, spotting=names)
    # several id sequences may stand for one phrase
    from speechcatcher_amd.server_session import spotting_set
    assert spotting_set({"x": [[1, 2], [3]], "y": [4, 5]}) == ([[1, 2], [3], [4, 5]], ["x", "x", "y"])
