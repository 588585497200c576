"""CTC speech activity on the CPU: the numpy contract (tests/ctc_activity_ref.py) against independent formulations, the
endpointing rules, and the Python lock-step engine / scheduler / server loop on the spec backend."""
import numpy as np
import pytest
import torch

import ctc_activity_ref as R
from activity_helpers import make_batch, pick_threshold
from speechcatcher_amd import synth
from speechcatcher_amd.activity import FIELDS, INITIAL, advance
from speechcatcher_amd.scheduler import ActivityResults, StreamScheduler
from speechcatcher_amd.server_session import AcousticEndpointer, EndpointRules, ServerLoop, scale_server_pcm


def _table(seed, T, V, scale=4.0):
    rng = np.random.RandomState(seed)
    return (rng.randn(T, V) * scale).astype(np.float32)


# ---- the contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 63, 1024])
def test_p_blank_equals_float64_log_softmax(V):
    x = _table(V, 37, V)
    x[3, : V // 2] = -np.inf                       # -inf entries are legal
    if V > 1:
        x[5, 0] = -np.inf                          # a blank of -inf: posterior 0
    x[7] = _table(99, 1, V)[0] * 1e30              # huge logits
    x[7][~np.isfinite(x[7])] = 1e30
    blank = 0
    want = torch.log_softmax(torch.from_numpy(x).double(), dim=1)[:, blank].exp().numpy()
    got = R.p_blank(x, blank)
    ok = ~np.isnan(want)                           # (row 3 at V = 1 is all -inf: torch gives NaN too)
    assert np.abs(got[ok] - want[ok]).max() <= 1e-12
    assert np.isnan(got[~ok]).all()
    if V > 1:
        assert got[5] == 0.0


def test_bad_rows():
    x = _table(1, 6, 16)
    x[1, 4] = np.nan
    x[2, 9] = np.inf
    x[3, :] = -np.inf
    x[4, 3] = -np.inf                               # legal
    pb = R.p_blank(x, 2)
    assert np.isnan(pb[[1, 2, 3]]).all() and not np.isnan(pb[[0, 4, 5]]).any()
    sil = R.silence(pb, 0.5)
    assert sil[[1, 2, 3]].all()                     # a bad frame is silence
    st = R.scan(R.INITIAL, pb, 2.0)                 # threshold above every posterior: every good frame is speech
    assert R.as_dict(st) == {"n_frames": 6, "n_speech": 3, "n_bad": 3, "first_speech": 0, "last_speech": 5,
                             "trail_silence": 0}


def _loop_scan(state, pb, thr):
    n, nsp, nbad, first, last, _ = state
    for p in pb:
        bad = p != p
        silence = bad or p > thr
        nbad += bad
        if not silence:
            nsp += 1
            first = n if first < 0 else first
            last = n
        n += 1
    return (n, nsp, nbad, first, last, n - 1 - last if last >= 0 else n)


@pytest.mark.parametrize("seed", range(6))
def test_scan_equals_a_per_frame_loop_and_splits(seed):
    rng = np.random.RandomState(seed)
    T = int(rng.randint(0, 200))
    pb = rng.rand(T)
    pb[rng.rand(T) < 0.1] = np.nan
    if seed == 0:
        pb[:] = 0.9                                 # all silence
    thr = 0.6
    want = _loop_scan(INITIAL, pb, thr)
    assert R.scan(R.INITIAL, pb, thr) == want
    assert advance(INITIAL, pb, thr) == want        # the engines' host-side scan is the same function
    for _ in range(20):                             # any split into consecutive spans, empty ones included
        cuts = np.sort(rng.randint(0, T + 1, size=int(rng.randint(0, 6))))
        cuts = np.concatenate([[0], cuts, cuts[-1:] if cuts.size else [0], [T]]).astype(int)
        st, states = R.INITIAL, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            st = R.scan(st, pb[a:b], thr)
            states.append(st)
            assert st == _loop_scan(INITIAL, pb[:b], thr)
        assert st == want
    assert R.scan(R.INITIAL, pb[:0], thr) == R.INITIAL
    assert tuple(R.FIELDS) == tuple(FIELDS)


# ---- endpointing rules ----------------------------------------------------------------------------------------------
def _act(n_frames, n_speech, last_speech):
    first = -1 if n_speech == 0 else 0
    return {"n_frames": n_frames, "n_speech": n_speech, "n_bad": 0, "first_speech": first, "last_speech": last_speech,
            "trail_silence": n_frames - 1 - last_speech if last_speech >= 0 else n_frames}


def test_rules_are_seconds_rounded_up_to_frames():
    assert [EndpointRules.frames(x) for x in (1.0, 5.0, 20.0, 0.04, 0.05, 0.0)] == [25, 125, 500, 1, 2, 0]
    ep = AcousticEndpointer()
    assert (ep.after_speech, ep.without_speech, ep.max_frames) == (25, 125, 500)


def test_each_rule_fires_at_its_frame_count_and_not_one_frame_earlier():
    ep = AcousticEndpointer(EndpointRules(silence_after_speech=1.0, silence_without_speech=5.0, max_utterance=20.0))
    assert not ep.decide()                                          # nothing observed yet
    # speech seen, then trailing silence: 24 frames do not fire, 25 do
    ep.observe(_act(40 + 24, 10, 39))
    assert not ep.decide()
    ep.observe(_act(40 + 25, 10, 39))
    assert ep.decide()
    assert not ep.decide()                                          # the history restarted with the finalisation
    # no speech at all: 124 frames do not fire, 125 do
    ep.observe(_act(124, 0, -1))
    assert not ep.decide()
    ep.observe(_act(125, 0, -1))
    assert ep.decide() and ep.last is None
    # speech going on: only the length bound
    ep.observe(_act(499, 499, 498))
    assert not ep.decide()
    ep.observe(_act(500, 500, 499))
    assert ep.decide()
    # a forced finalisation restarts the history as well
    ep.observe(_act(500, 500, 499))
    ep.reset()
    assert not ep.decide()
    # speech followed by less silence than the rule is not "no speech": rule 2 does not apply
    ep.observe(_act(200, 1, 180))
    assert not ep.decide()


# ---- the Python engine on the spec backend ---------------------------------------------------------------------------
CHUNK, N_CHUNKS = 10240, 8


def _spec_batch(n_streams=2, **kw):
    from oracle.kernel_spec import SpecBackend
    return make_batch("TINY", SpecBackend(), n_streams, max_frames=400, max_tokens=300, pcm_capacity=1 << 18, **kw)


@pytest.fixture(scope="module")
def probe():
    """one run of stream 0 (seeded audio, non-final chunks, then a final one): frames after every chunk, the engine's
    CTC table and the float64 reference of its blank posteriors"""
    sb = _spec_batch()
    sb.set_activity(True, 0.5)
    audio = synth.synth_audio(5, CHUNK * N_CHUNKS)
    T = []
    for k in range(N_CHUNKS):
        sb.push([(0, audio[k * CHUNK:(k + 1) * CHUNK], k == N_CHUNKS - 1)])
        T.append(int(sb.st[0].T_enc))
    table = sb.ctcx[:T[-1]].numpy().copy()
    ref = R.p_blank(table, sb.cfg.blank_id)
    thr, gap = pick_threshold(ref)
    assert gap > 1e-3
    return {"audio": audio, "T": T, "table": table, "ref": ref, "thr": thr, "track": sb.read_activity(0)}


def test_engine_activity_equals_the_reference_on_its_own_table(probe):
    sb = _spec_batch()
    with pytest.raises(Exception):
        sb.activity([0])                                            # off by default
    sb.set_activity(True, probe["thr"])
    assert sb.activity([0, 1])["n_frames"].tolist() == [0, 0] and sb.activity([1])["last_speech"].tolist() == [-1]
    audio = probe["audio"]
    seen = set()
    for k in range(N_CHUNKS):
        sb.push([(0, audio[k * CHUNK:(k + 1) * CHUNK], k == N_CHUNKS - 1)])
        got = {f: int(v[0]) for f, v in sb.activity([0]).items()}
        want = R.as_dict(R.scan(R.INITIAL, probe["ref"][:probe["T"][k]], probe["thr"]))
        assert got == want, (k, got, want)
        seen.add((want["n_speech"] > 0, want["trail_silence"] > 0))
    assert want["n_frames"] == probe["T"][-1] > 64 and 0 < want["n_speech"] < want["n_frames"]
    # the track: float64 posteriors of the raw rows against the table read back (first block log-softmaxed in fp32)
    track = sb.read_activity(0)
    assert track.shape == probe["ref"].shape and np.abs(track - probe["ref"]).max() <= 1e-5
    assert sb.activity([1])["n_frames"].tolist() == [0]             # the idle stream
    sb.reset(0)
    assert tuple(int(v[0]) for v in sb.activity([0]).values()) == INITIAL
    assert sb.read_activity(0).size == 0


def test_activity_does_not_change_the_hypotheses(probe):
    a, b = _spec_batch(), _spec_batch()
    b.set_activity(True, probe["thr"])
    audio = probe["audio"]
    for k in range(4):
        for sb in (a, b):
            sb.push([(0, audio[k * CHUNK:(k + 1) * CHUNK], k == 3)])
        assert a.hypotheses(0) == b.hypotheses(0)
    assert len(a.hypotheses(0)[0]["yseq"]) > 1


class _LoggingScheduler(StreamScheduler):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.finals = []

    def feed(self, sid, pcm, is_final=False, finalize_all=False):
        self.finals.append(bool(is_final))
        super().feed(sid, pcm, is_final, finalize_all)


def _pcm16(audio):
    return np.clip(np.round(audio * 32767.0), -32768, 32767).astype(np.int16)


def test_scheduler_replies_carry_the_activity_of_their_chunk(probe):
    sb = _spec_batch()
    sch = StreamScheduler(sb, None, result_format="espnet", activity=True, blank_threshold=probe["thr"])
    sid = sch.open()
    audio = probe["audio"]
    for k in range(N_CHUNKS):
        sch.feed(sid, audio[k * CHUNK:(k + 1) * CHUNK], is_final=k == N_CHUNKS - 1)
        res = sch.step()[sid]
        assert isinstance(res, ActivityResults) and isinstance(res, list)
        assert res.activity == R.as_dict(R.scan(R.INITIAL, probe["ref"][:probe["T"][k]], probe["thr"]))
    # ... read before the reset that follows a final
    assert res.activity["n_frames"] == probe["T"][-1] and sb.activity([0])["n_frames"].tolist() == [0]


def test_server_loop_finalises_at_the_chunk_the_reference_scan_predicts():
    n = 9
    pcm = [_pcm16(synth.synth_audio(5, CHUNK * n)[k * CHUNK:(k + 1) * CHUNK]) for k in range(n)]
    # the engine's table for this audio (what the server feeds: int16 -> float16 / 32767), all chunks non-final
    sb = _spec_batch()
    sb.set_activity(True, 0.5)
    T = []
    for k in range(n):
        sb.push([(0, scale_server_pcm(pcm[k]), False)])
        T.append(int(sb.st[0].T_enc))
    ref = R.p_blank(sb.ctcx[:T[-1]].numpy(), sb.cfg.blank_id)
    thr, gap = pick_threshold(ref)
    assert gap > 1e-3
    rules = EndpointRules(silence_after_speech=0.8, silence_without_speech=100.0, max_utterance=100.0)
    ep = AcousticEndpointer(rules)
    states = [R.as_dict(R.scan(R.INITIAL, ref[:t], thr)) for t in T]
    fires = [ep.fires(s) for s in states]
    want = fires.index(True) + 1                      # the chunk AFTER the first reply whose state fires is the final one
    assert 2 <= want < n - 1, (want, states)
    assert states[want - 1]["trail_silence"] >= 20 and not fires[want - 2]

    def run(acoustic):
        sch = _LoggingScheduler(_spec_batch(), None, result_format="espnet", activity=acoustic is not None,
                                blank_threshold=thr)
        loop = ServerLoop(sch, finalize_update_iters=100, max_partial_iters=1000, acoustic_endpointing=acoustic)
        sid = loop.connect()
        replies = []
        for k in range(n):
            loop.submit(sid, pcm[k])
            replies.extend(loop.step()[sid])
        return sch.finals, replies

    finals, replies = run(rules)
    assert finals[:want + 1] == [False] * want + [True], (finals, want)
    assert finals[want + 1] is False                  # the history restarted with the finalisation
    assert replies[want].endswith("\n") or replies[want] == ""
    # without the option: the text rule alone (silent here: 100 unchanged chunks), and the replies of today - the same
    # partials as the run with the option up to its acoustic final
    finals0, replies0 = run(None)
    assert finals0 == [False] * n
    assert replies0[:want] == replies[:want] and len(replies0) == n
    with pytest.raises(ValueError):
        ServerLoop(StreamScheduler(_spec_batch(), None, result_format="espnet"), strict_reference=True,
                   acoustic_endpointing=rules)
