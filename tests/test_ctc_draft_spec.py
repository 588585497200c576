"""CTC draft transcript on the CPU: the numpy contract (tests/ctc_draft_ref.py) and its properties, the engines' host-side
recurrence against it, and the Python lock-step engine / scheduler / server loop on the spec backend."""
import json

import numpy as np
import pytest

import ctc_draft_ref as R
from draft_helpers import MODELS, make_batch, path_mix
from speechcatcher_amd import draft, synth
from speechcatcher_amd.align import FeatureClock
from speechcatcher_amd.scheduler import DraftResults, SpottingResults, StreamScheduler
from speechcatcher_amd.server_session import ServerLoop, scale_server_pcm

V, BLANK = 67, 0
A, B, C = 5, 9, 40


def _row(hot, rest=-30.0):
    """a row whose entries `hot` (label -> value) are set, the rest far below"""
    x = np.full(V, rest, np.float32)
    for lab, val in hot.items():
        x[lab] = val
    return x


def _table(labels, rng=None):
    """one row per label: the label's entry ahead by 4 (None: a NaN row), the runner-up somewhere else"""
    rng = rng or np.random.default_rng(0)
    x = rng.standard_normal((len(labels), V)).astype(np.float32)
    for t, lab in enumerate(labels):
        if lab is None:
            x[t, 3] = np.nan
        else:
            x[t, lab] = x[t].max() + np.float32(4.0)
    return x


def _ids(tokens):
    return [t[:3] for t in tokens]


# ---- the contract's own properties ------------------------------------------------------------------------------------
def test_a_tie_takes_the_lowest_index_also_between_the_blank_and_a_token():
    lab, p = R.rows(np.stack([_row({A: 2.0, B: 2.0}), _row({B: 2.0, C: 2.0}), _row({BLANK: 1.0, A: 1.0}),
                              _row({V - 1: 0.5, V - 2: 0.5})]), BLANK)
    assert lab.tolist() == [A, B, BLANK, V - 2]
    assert np.allclose(p, 0.5, atol=1e-10)                          # two tied entries, the rest 32 nats below
    st, store = R.scan_table(np.stack([_row({BLANK: 1.0, A: 1.0}), _row({A: 1.0, B: 1.0})]), BLANK)
    assert store == [] and st[:6] == (2, 0, 0, A, 1, 1)            # the blank wins its tie, A wins the other


def test_a_blank_between_repeats_gives_two_tokens():
    st, store = R.scan_table(_table([A, A, BLANK, A, B, B, BLANK, BLANK]), BLANK)
    assert _ids(store) == [(A, 0, 1), (A, 3, 3), (B, 4, 5)]
    assert st[:6] == (8, 3, 0, -1, -1, -1) and st[6] == 0.0
    st, store = R.scan_table(_table([A, A, A]), BLANK)
    assert store == [] and st[:6] == (3, 0, 0, A, 0, 2) and _ids(R.draft(st, store)) == [(A, 0, 2)]


@pytest.mark.parametrize("bad", ["nan", "inf", "all_minus_inf"])
def test_a_bad_row_closes_the_token_and_counts(bad):
    x = _table([A, A, A, A, BLANK, A])
    x[2] = {"nan": _row({A: np.nan}), "inf": _row({B: np.inf}), "all_minus_inf": np.full(V, -np.inf, np.float32)}[bad]
    st, store = R.scan_table(x, BLANK)
    assert _ids(store) == [(A, 0, 1), (A, 3, 3)] and st[:6] == (6, 2, 1, A, 5, 5)
    lab, p = R.rows(x, BLANK)
    assert lab[2] == R.BAD and np.isnan(p[2]) and not np.isnan(np.delete(p, 2)).any()
    # -inf entries beside finite ones are no fault, and logits of 1e30 give p = 1 (the formula as written)
    lab, p = R.rows(np.stack([_row({A: 0.0}, rest=-np.inf), _row({B: 1e30, C: 1e30}, rest=-1e30)]), BLANK)
    assert lab.tolist() == [A, B] and p.tolist() == [1.0, 1.0]


def test_conf_is_the_largest_posterior_of_the_run():
    x = np.stack([_row({A: 0.0, B: -1.0}, -60.0), _row({A: 0.0, B: -3.0}, -60.0), _row({A: 0.0, B: -0.5}, -60.0),
                  _row({BLANK: 9.0})])     # (the other 65 entries add 65 * exp(-60) to the sum: below 1e-24)
    (lab, p), (st, store) = R.rows(x, BLANK), R.scan_table(x, BLANK)
    assert lab.tolist() == [A, A, A, BLANK] and store == [(A, 0, 2, float(p[1]))] and p[1] == p[:3].max()
    assert abs(p[1] - 1.0 / (1.0 + np.exp(-3.0))) < 1e-12


@pytest.mark.parametrize("seed", range(4))
def test_any_split_gives_the_state_and_store_of_one_span(seed):
    rng = np.random.default_rng(seed)
    T = 300
    labels = []
    while len(labels) < T:                                          # runs of 1..5 frames over four labels, blanks, bad rows
        labels += [rng.choice([BLANK, A, A, B, C, None])] * int(rng.integers(1, 6))
    x = _table(labels[:T], rng)
    one, store1 = R.scan_table(x, BLANK)
    assert one[1] >= 30 and one[2] >= 5
    for _ in range(6):
        cuts = np.sort(rng.integers(0, T + 1, size=5))
        cuts = np.concatenate([[0], cuts, cuts[-1:], [T]]).astype(int)     # six spans and more, empty ones among them
        st, store = R.INITIAL, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            st, _ = R.scan_table(x[a:b], BLANK, st, store)
            want, wstore = R.scan_table(x[:b], BLANK)
            assert st == want and store == wstore
        assert st == one and store == store1
    assert R.scan_table(x[:0], BLANK) == (R.INITIAL, [])


def test_slots_at_or_beyond_the_capacity_are_counted_not_written():
    x = _table([A, BLANK, B, BLANK, C, BLANK, A, BLANK, B, BLANK, C, C])
    st, store = R.scan_table(x, BLANK, capacity=4)
    full, fstore = R.scan_table(x, BLANK)
    assert st == full and st[1] == 5 and len(fstore) == 5 and store == fstore[:4]
    assert _ids(R.draft(st, store))[-1] == (C, 10, 11)
    st, store = R.scan_table(x, BLANK, capacity=0)
    assert st == full and store == []


# ---- the engines' recurrence ------------------------------------------------------------------------------------------
def _same(state: dict, want, wstore):
    got = tuple(state[k] for k in draft.FIELDS)
    return (got[:6] == tuple(want[:6]) and np.float64(got[6]).tobytes() == np.float64(want[6]).tobytes()
            and np.asarray(state["tokens"], np.float64).tobytes() == np.asarray(wstore, np.float64).tobytes())


@pytest.mark.parametrize("seed", range(3))
def test_the_engines_recurrence_is_the_contract_bit_for_bit(seed):
    rng = np.random.default_rng(10 + seed)
    labels = []
    while len(labels) < 150:
        labels += [rng.choice([BLANK, A, B, C, None])] * int(rng.integers(1, 4))
    x = _table(labels[:150], rng)
    x[7] = _row({A: 1.0, B: 1.0})
    x[8, 11] = -np.inf
    assert draft.INITIAL == R.INITIAL and draft.FIELDS == R.FIELDS
    st = draft.initial()
    ref, store = R.INITIAL, []
    for a, b in ((0, 0), (0, 1), (1, 64), (64, 64), (64, 150)):
        st = draft.advance(st, x[a:b], BLANK)
        ref, _ = R.scan_table(x[a:b], BLANK, ref, store)
        assert _same(st, ref, store), (a, b)
        assert draft.tokens_of(st) == R.draft(ref, store)
    cap = draft.advance(draft.initial(), x, BLANK, capacity=3)
    assert len(cap["tokens"]) == 3 and cap["n_closed"] == ref[1] > 3


def test_ahead_and_seconds():
    toks = [(A, 0, 3, 0.9), (B, 6, 6, 0.5), (C, 10, 12, 0.7)]
    assert draft.ahead(toks, 0) == toks and draft.ahead(toks, 6) == toks[1:] and draft.ahead(toks, 7) == toks[2:]
    assert draft.ahead(toks, 13) == [] and draft.ahead(draft.token_dicts(toks), 7) == draft.token_dicts(toks[2:])
    clock = FeatureClock(400, 160)
    clock.call(16000, False)
    d = draft.token_dicts(toks[:1], clock, 4, 16000, names={A: "x"})[0]
    assert d["token"] == "x" and d["id"] == A and d["conf"] == 0.9
    assert (d["start"], d["end"]) == (clock.frame_span(0, 4)[0] / 16000, clock.frame_span(3, 4)[1] / 16000)


# ---- the Python engine on the spec backend ---------------------------------------------------------------------------
CHUNK, N_CHUNKS = 10240, 8


def _spec_batch(model, n_streams=2, **kw):
    from oracle.kernel_spec import SpecBackend
    return make_batch(model, "TINY", SpecBackend(), n_streams, max_frames=400, max_tokens=300, pcm_capacity=1 << 18, **kw)


def _pcm16(audio):
    return np.clip(np.round(audio * 32767.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module", params=MODELS)
def probe(request):
    """one run of stream 0 (what the server feeds: int16 audio scaled back; non-final chunks, then a final one), the RAW
    rows the engine handed its recurrence recorded, and the contract's state and store after every chunk"""
    from speechcatcher_amd import engine
    model = request.param
    pcm = _pcm16(synth.synth_audio(5, CHUNK * N_CHUNKS))
    audio = scale_server_pcm(pcm)
    rows, real = [], draft.advance

    def recorder(state, x, *a, **kw):
        rows.append(np.array(x, np.float32))
        return real(state, x, *a, **kw)

    sb = _spec_batch(model)
    sb.set_draft(True)
    engine.draft_mod.advance = recorder
    try:
        T = []
        for k in range(N_CHUNKS):
            sb.push([(0, audio[k * CHUNK:(k + 1) * CHUNK], k == N_CHUNKS - 1)])
            T.append(int(sb.st[0].T_enc))
    finally:
        engine.draft_mod.advance = real
    table = np.concatenate(rows)
    blank = sb.cfg.blank_id
    assert table.shape == (T[-1], sb.cfg.vocab_size) and T[-1] > 64
    path_mix(model, table, blank)                                   # all tokens / all blanks / a mix of both
    snaps = {}
    for t in sorted(set(T)):
        st, store = R.scan_table(table[:t], blank)
        snaps[t] = (st, store)
    assert snaps[T[-1]][0][1] >= 8 or model == "blanks"
    return {"model": model, "pcm": pcm, "audio": audio, "T": T, "table": table, "blank": blank, "snaps": snaps,
            "cfg": sb.cfg}


def _want(p, k):
    """(state, draft) of the contract over the frames the stream had after chunk k"""
    st, store = p["snaps"][p["T"][k]]
    return st, R.draft(st, store)


def _state_of(sb, s=0):
    d = sb.draft([s])
    return tuple(int(d[k][0]) for k in R.FIELDS[:6]) + (float(d["open_conf"][0]),)


def test_engine_draft_equals_the_contract_on_the_rows_it_projected(probe):
    p = probe
    sb = _spec_batch(p["model"], strict_reference=False)
    with pytest.raises(Exception):
        sb.draft([0])                                               # off by default
    with pytest.raises(Exception):
        sb.draft_tokens(0)
    sb.set_draft(True)
    assert _state_of(sb) == R.INITIAL and sb.draft_tokens(0) == []
    for k in range(N_CHUNKS):
        sb.push([(0, p["audio"][k * CHUNK:(k + 1) * CHUNK], k == N_CHUNKS - 1)])
        st, toks = _want(p, k)
        assert _state_of(sb) == st, k
        assert np.asarray(sb.draft_tokens(0)).tobytes() == np.asarray(toks, np.float64).tobytes(), k
    assert _state_of(sb, 1) == R.INITIAL                            # the idle stream
    sb.reset(0)
    assert _state_of(sb) == R.INITIAL and sb.draft_tokens(0) == []
    sb.set_draft(False)
    with pytest.raises(Exception):
        sb.draft([0])


def test_the_draft_does_not_change_the_hypotheses(probe):
    a, b = _spec_batch(probe["model"]), _spec_batch(probe["model"])
    b.set_draft(True)
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


def test_scheduler_replies_carry_draft_and_ahead_read_before_the_reset_after_a_final(probe):
    p = probe
    sb = _spec_batch(p["model"], strict_reference=False)
    sch = StreamScheduler(sb, None, result_format="espnet", draft=True)
    sid = sch.open()
    cfg = p["cfg"]
    for k in range(N_CHUNKS):
        sch.feed(sid, p["audio"][k * CHUNK:(k + 1) * CHUNK], is_final=k == N_CHUNKS - 1)
        res = sch.step()[sid]
        assert isinstance(res, DraftResults) and isinstance(res, SpottingResults) and isinstance(res, list)
        _, toks = _want(p, k)
        assert [(d["id"], d["start"], d["end"], d["conf"]) for d in res.draft] == toks, k
        clock = _clock(p, k)
        for d in res.draft:                                                           # seconds: the frames' sample spans
            assert d["start_s"] == clock.frame_span(d["start"], cfg.subsample)[0] / cfg.sample_rate
            assert d["end_s"] == clock.frame_span(d["end"], cfg.subsample)[1] / cfg.sample_rate
            assert 0.0 <= d["start_s"] < d["end_s"] <= (k + 1) * CHUNK / 16000 + 0.05
        pos = res[0][3] if res else []
        h = pos[-1] if pos else 0
        assert res.ahead == [d for d in res.draft if d["start"] >= h], k
        assert res.detections is None and res.activity is None
    assert len(res.draft) == len(_want(p, N_CHUNKS - 1)[1])                            # the final reply's draft was read
    assert _state_of(sb) == R.INITIAL                                                  # ... before the reset
    if p["model"] != "blanks":
        assert len(res.draft) >= 8
    # the next utterance of the session starts over: the same audio, the same draft
    sch.feed(sid, p["audio"][:CHUNK], is_final=False)
    assert [(d["id"], d["start"], d["end"]) for d in sch.step()[sid].draft] == _ids(_want(p, 0)[1])
    # with the other options on, one reply carries all
    both = StreamScheduler(_spec_batch(p["model"]), None, result_format="espnet", draft=True, activity=True)
    sid = both.open()
    both.feed(sid, p["audio"][:CHUNK])
    res = both.step()[sid]
    assert res.activity["n_frames"] == p["T"][0] and len(res.draft) == len(_want(p, 0)[1])
    # without the option: plain replies
    plain = StreamScheduler(_spec_batch(p["model"]), None, result_format="espnet")
    sid = plain.open()
    plain.feed(sid, p["audio"][:CHUNK])
    assert not hasattr(plain.step()[sid], "draft")


def test_server_loop_puts_ahead_fields_on_partials_only(probe):
    p = probe
    cfg = p["cfg"]
    names = [f"▁t{i}" for i in range(cfg.vocab_size)]

    def run(**kw):
        sch = StreamScheduler(_spec_batch(p["model"]), names, result_format="espnet")
        loop = ServerLoop(sch, vosk_output_format=True, finalize_update_iters=100, max_partial_iters=1000, **kw)
        sid = loop.connect()
        out = []
        for k in range(N_CHUNKS - 1):
            loop.submit(sid, p["pcm"][k * CHUNK:(k + 1) * CHUNK])
            out.append(loop.step()[sid])
        loop.submit(sid, '{"eof" : 1}')
        out.append(loop.step()[sid])
        return out

    replies, off, plain = run(draft_partials=True), run(draft_partials=False), run()
    assert json.dumps(off, sort_keys=True) == json.dumps(plain, sort_keys=True)         # False changes nothing
    n_ahead = 0
    for k in range(N_CHUNKS - 1):
        assert len(replies[k]) == len(plain[k]) == 1
        r = replies[k][0]
        assert sorted(r) == ["ahead", "ahead_result", "partial"] and r["partial"] == plain[k][0]["partial"]
        assert r["ahead"] == "".join(w["word"] for w in r["ahead_result"]).strip()
        _, toks = _want(p, k)
        clock = _clock(p, k)
        tail = toks[len(toks) - len(r["ahead_result"]):]                               # the ahead tokens end the draft
        assert r["ahead_result"] == [
            {"word": names[t[0]].replace("▁", " "), "start": round(clock.frame_span(t[1], cfg.subsample)[0] / cfg.sample_rate, 3),
             "end": round(clock.frame_span(t[2], cfg.subsample)[1] / cfg.sample_rate, 3), "conf": t[3]} for t in tail]
        n_ahead += len(tail)
    assert n_ahead >= 8 or p["model"] == "blanks"
    assert replies[-1] == plain[-1] and "ahead" not in replies[-1][0]                  # finals unchanged
    with pytest.raises(ValueError):
        ServerLoop(StreamScheduler(_spec_batch(p["model"]), None, result_format="espnet"), strict_reference=True,
                   draft_partials=True)
