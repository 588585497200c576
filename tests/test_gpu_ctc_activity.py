"""CTC speech activity on the GPU (csrc/activity.hip: sc_ctc_activity; csrc/streams.hip: sc_streams_set_activity /
sc_stream_activity / sc_streams_read_activity) against the float64 contract of tests/ctc_activity_ref.py: the kernel on
constructed tables, the stream level on the tiny and the XL synthetic model (lock-step, continuous batching at queue
depth 2, the Python engine over the HIP kernels), the option's effect on serving (none) and the server loop.

Measured on an MI355X (printed by the tests): kernel p_blank against the reference at most 6.7e-15 absolute
(bar 1e-12); stream-level track against the table read back at most 4.7e-08 (tiny) / 4.9e-08 (XL) (bar 1e-5)."""
import functools

import numpy as np
import pytest
import torch

import ctc_activity_ref as R
from activity_helpers import make_batch, packed_weights, pick_threshold
from speechcatcher_amd import synth

pytestmark = pytest.mark.gpu

THR = 0.8
SEEN = (100, 40, 3, 10, 90, 9)      # a carry-in state "speech seen" (the other one: None = nothing yet)


def _place(rng, T, V, blank, targets):
    """[T, V] fp32 table whose row t has a blank posterior of targets[t] (V >= 2): the other logits are random, the blank
    logit is log(p / (1 - p)) + logsumexp of the others"""
    x = (rng.standard_normal((T, V)) * 3).astype(np.float32)
    o = x.astype(np.float64)
    o[:, blank] = -np.inf
    m = o.max(1)
    lse = m + np.log(np.exp(o - m[:, None]).sum(1))
    p = np.asarray(targets, np.float64)
    x[:, blank] = (np.log(p) - np.log1p(-p) + lse).astype(np.float32)
    return x


def _targets(rng, T, speech):
    """posteriors at least 2e-3 away from THR: speech frames below it, silence frames above; the closest ones first"""
    speech = np.asarray(speech, bool)
    lo, hi = rng.uniform(0.01, THR - 2e-3, T), rng.uniform(THR + 2e-3, 0.999, T)
    lo[:4], hi[:4] = THR - 2e-3, THR + 2e-3
    return np.where(speech, lo, hi)


def _strided(x, pad=3):
    """the table on the device as a view with a row stride of V + pad floats (NaN between the rows: never read)"""
    T, V = x.shape
    buf = torch.full((T, V + pad), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :V] = torch.from_numpy(x).to("cuda:0")
    return buf[:, :V]


def _cases():
    rng = np.random.default_rng(11)
    cases = []   # (name, table [T, V] fp32, blank, t0, t1, carry-in)
    for V in (1, 63, 64, 65, 1024, 1500):
        T, blank = 140, (0 if V in (1, 1024) else int(rng.integers(0, V)))
        if V == 1:
            x = (rng.standard_normal((T, 1)) * 3).astype(np.float32)       # p_blank = 1: silence
        else:
            x = _place(rng, T, V, blank, _targets(rng, T, rng.random(T) < 0.5))
        for n in (0, 1, 63, 64, 65, 129):          # the ballot-word edges
            for carry in (None, SEEN):
                cases.append((f"V{V}_n{n}_{'seen' if carry else 'fresh'}", x, blank, 3, 3 + n, carry))
    V, T = 1024, 129
    pats = {"all_silence": np.zeros(T, bool), "all_speech": np.ones(T, bool), "first_only": np.arange(T) == 0,
            "last_only": np.arange(T) == T - 1}
    for name, sp in pats.items():
        x = _place(rng, T, V, 0, _targets(rng, T, sp))
        for carry in (None, SEEN):
            cases.append((f"{name}_{'seen' if carry else 'fresh'}", x, 0, 0, T, carry))
    for V in (65, 1024):                            # special rows
        T, blank = 70, 7
        x = _place(rng, T, V, blank, _targets(rng, T, rng.random(T) < 0.5))
        x[1, rng.random(V) < 0.5] = -np.inf         # -inf entries are legal ...
        x[1, blank] = 0.0
        x[2, blank] = -np.inf                       # ... a blank of -inf: posterior 0, speech
        x[3] = np.where(rng.random(V) < 0.5, 1e30, -1e30).astype(np.float32)   # logits of magnitude 1e30
        x[3, blank] = 1e30                          # ... the blank among the largest: silence
        x[4] = x[3]
        x[4, blank], x[4, (blank + 1) % V] = -1e30, 1e30   # ... the blank 2e30 below the largest: posterior 0, speech
        x[5] = -np.inf                              # bad: nothing but -inf
        x[6, V - 1] = np.nan                        # bad: a NaN (in the last, partial, lane stride)
        x[7, 0] = np.inf                            # bad: a +inf
        x[64, 5] = np.nan                           # bad frame in the second ballot word
        cases.append((f"special_V{V}", x, blank, 0, T, None))
        cases.append((f"special_V{V}_seen", x, blank, 0, T, SEEN))
    return cases


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


def _check(name, x, blank, t0, t1, carry, state, track, after, worst):
    pb = R.p_blank(x[t0:t1], blank)
    # threshold placement: no reference posterior closer than 1e-3 to the threshold, so no frame is left out of the
    # state comparison (share of excluded frames: zero)
    ok = ~np.isnan(pb)
    assert ok.all() or "special" in name
    assert np.abs(pb[ok] - THR).min(initial=1.0) >= 1e-3, name
    want = R.scan(carry if carry is not None else R.INITIAL, pb, THR)
    assert tuple(int(v) for v in state) == want, (name, state, want)
    assert tuple(int(v) for v in after) == want, name
    got = track[t0:t1]
    assert np.array_equal(np.isnan(got), np.isnan(pb)), name            # bad frames are NaN in both
    if ok.any():
        worst[0] = max(worst[0], float(np.abs(got[ok] - pb[ok]).max()))
        assert np.abs(got[ok] - pb[ok]).max() <= 1e-12, name
    assert (track[:t0] == -7.0).all() and (track[t1:] == -7.0).all(), name   # nothing outside the span is written


def test_kernel_equals_the_reference_on_constructed_tables(be):
    cases = _cases()
    dev = {}
    for c in cases:
        if id(c[1]) not in dev:
            dev[id(c[1])] = _strided(c[1])
            assert dev[id(c[1])].stride(0) > c[1].shape[1]
    jobs = [(dev[id(x)], blank, t0, t1, carry) for (_, x, blank, t0, t1, carry) in cases]
    state, tracks, after = be.ctc_activity(jobs, THR)            # ONE launch for all of them
    worst = [0.0]
    for k, (name, x, blank, t0, t1, carry) in enumerate(cases):
        _check(name, x, blank, t0, t1, carry, state[k], tracks[k], after[k], worst)
    print(f"\nsc_ctc_activity: {len(cases)} jobs, largest |p_blank - reference| = {worst[0]:.3e}")
    # the special rows do what the contract says
    name, x, blank = cases[-2][0], cases[-2][1], cases[-2][2]
    pb = tracks[len(cases) - 2]
    assert name == "special_V1024" and pb[2] == 0.0 and pb[3] > THR and pb[4] == 0.0
    assert np.isnan(pb[[5, 6, 7, 64]]).all() and int(state[len(cases) - 2][2]) == 4


def test_kernel_chained_spans_equal_one_span(be):
    rng = np.random.default_rng(5)
    V, spans = 1024, (1, 15, 16, 17, 64, 1)
    T = sum(spans)
    x = _place(rng, T, V, 0, _targets(rng, T, rng.random(T) < 0.4))
    x[20, 3] = np.nan
    tab = _strided(x)
    for carry in (None, SEEN):
        one, tr_one, _ = be.ctc_activity([(tab, 0, 0, T, carry)], THR)
        st, t0, tr = carry, 0, np.full(T, -7.0)
        for n in spans:
            s, trk, aft = be.ctc_activity([(tab, 0, t0, t0 + n, st)], THR)
            st = tuple(int(v) for v in s[0])
            assert st == tuple(int(v) for v in aft[0])
            assert st == R.scan(carry or R.INITIAL, R.p_blank(x[:t0 + n], 0), THR)
            tr[t0:t0 + n] = trk[0][t0:t0 + n]
            t0 += n
        assert st == tuple(int(v) for v in one[0])
        assert tr.tobytes() == tr_one[0].tobytes()                # the same bytes however the table was cut
    # an empty job table and argument errors: refused before anything is launched
    from speechcatcher_amd import _abi
    lib = _abi.load()
    assert lib.sc_ctc_activity(None, 0, None) == 0
    assert lib.sc_ctc_activity(None, 2, None) == -1 and lib.sc_ctc_activity(None, -1, None) == -1
    assert lib.sc_ctc_activity(tab.data_ptr(), _abi.ACTIVITY_MAX_JOBS + 1, None) == -1


# ---- stream level ----------------------------------------------------------------------------------------------------
CHUNK = 10240
N_CHUNKS = {"TINY": 8, "XL": 6}
KW = dict(max_frames=160, max_tokens=200, pcm_capacity=1 << 17)


@functools.lru_cache(maxsize=None)
def _weights(name):
    return packed_weights(name, "cuda:0")


@pytest.fixture(scope="module", params=["TINY", "XL"])
def probe(request):
    """per model, computed once: the weights, the audio of two streams, the frames after every chunk, the CTC table of
    the whole utterance read back from the C++ engine, its float64 reference posteriors and the threshold"""
    name = request.param
    n = N_CHUNKS[name]
    w = _weights(name)
    sb = make_batch(name, "native", 2, weights=w, **KW)
    sb.set_activity(True, 0.5)
    audio = [synth.synth_audio(5 + s, CHUNK * n - 1000 * s) for s in range(2)]
    T = [[], []]
    for k in range(n):
        sb.push([(s, audio[s][k * CHUNK:(k + 1) * CHUNK], k == n - 1) for s in range(2)])
        for s in range(2):
            T[s].append(int(sb.st[s].T_enc))
    table = [sb.read_ctc(s) for s in range(2)]
    ref = [R.p_blank(table[s], sb.cfg.blank_id) for s in range(2)]
    assert [len(r) for r in ref] == [T[0][-1], T[1][-1]]
    thr, gap = pick_threshold(np.concatenate(ref))
    assert gap > 1e-3, gap
    # every posterior of both streams is at least half that gap away from the threshold: nothing to exclude
    assert np.abs(np.concatenate(ref) - thr).min() >= 0.5e-3
    return {"name": name, "n": n, "w": w, "engine": sb.engine, "audio": audio, "T": T, "ref": ref, "thr": thr}


def _want(p, s, k):
    return R.as_dict(R.scan(R.INITIAL, p["ref"][s][:p["T"][s][k]], p["thr"]))


def _chunks(p, k):
    return [(s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == p["n"] - 1) for s in range(2)]


def _get(sb, s):
    return {f: int(v[0]) for f, v in sb.activity([s]).items()}


def test_lockstep_push_equals_the_reference_scan_of_the_table(probe):
    p = probe
    sb = make_batch(p["name"], "native", 2, weights=p["w"], engine=p["engine"], **KW)
    with pytest.raises(Exception):
        sb.activity([0])                                         # off by default
    sb.set_activity(True, p["thr"])
    assert _get(sb, 0) == R.as_dict(R.INITIAL)
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
        for s in range(2):
            assert _get(sb, s) == _want(p, s, k), (s, k)
    # more than one ballot word per stream; the threshold lies inside the posteriors of the two streams taken together
    w = [_want(p, s, p["n"] - 1) for s in range(2)]
    assert min(x["n_frames"] for x in w) > 64
    assert 0 < sum(x["n_speech"] for x in w) < sum(x["n_frames"] for x in w)
    worst = 0.0
    for s in range(2):
        track = sb.read_activity(s)
        assert track.shape == p["ref"][s].shape
        worst = max(worst, float(np.abs(track - p["ref"][s]).max()))
    print(f"\n{p['name']}: largest |track - p_blank of the table read back| = {worst:.3e}")
    assert worst <= 1e-5
    sb.reset(0)
    assert _get(sb, 0) == R.as_dict(R.INITIAL) and sb.read_activity(0).size == 0
    assert _get(sb, 1) == _want(p, 1, p["n"] - 1)                # the other stream keeps its state
    with pytest.raises(Exception):
        sb.set_activity(True, 1.5)
    sb.set_activity(False)
    with pytest.raises(Exception):
        sb.activity([0])


def test_continuous_queue_depth_2_gives_the_states_of_the_reported_chunks(probe):
    p = probe
    sb = make_batch(p["name"], "native", 2, weights=p["w"], engine=p["engine"], **KW)
    sb.set_queue_depth(2)
    sb.set_activity(True, p["thr"])
    nxt, rep = [0, 0], [0, 0]

    def feed(s):
        k = nxt[s]
        nxt[s] += 1
        return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == p["n"] - 1)

    sb.submit([feed(0), feed(1)])
    with pytest.raises(Exception):
        sb.set_activity(True, 0.5)                               # refused while chunks are outstanding
    sb.submit([feed(0), feed(1)])
    while sb.outstanding:
        done = sb.poll(1)
        for s in sorted(done):
            # the state of the chunk that was REPORTED, whatever is queued behind it
            assert _get(sb, s) == _want(p, s, rep[s]), (s, rep[s])
            assert sb.read_activity(s).shape[0] == p["T"][s][rep[s]]
            rep[s] += 1
        again = [feed(s) for s in sorted(done) if nxt[s] < p["n"]]
        if again:
            sb.submit(again)
    assert rep == [p["n"], p["n"]]


def test_python_engine_on_the_hip_backend_gives_the_same_states(probe):
    p = probe
    from speechcatcher_amd.hip_backend import HipBackend
    sb = make_batch(p["name"], HipBackend("cuda:0"), 2, weights=p["w"], **KW)
    sb.set_activity(True, p["thr"])
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
        for s in range(2):
            assert _get(sb, s) == _want(p, s, k), (s, k)
    assert np.abs(sb.read_activity(0) - p["ref"][0]).max() <= 1e-5


def test_activity_has_no_effect_on_serving():
    """XL streams under continuous batching (sc_submit / sc_poll, queue depth 2): hypotheses, positions and scores of every
    reply are bit-identical with the option on (and read after every reply) and off."""
    from test_engine_spec import make_batch as plain_batch
    S, chunk = 32, 10240
    lens = [chunk * (2 + (i * 5) % 3) + (i * 977) % 3000 for i in range(S)]
    audio = [synth.synth_audio(300 + i, n) for i, n in enumerate(lens)]

    def run(on):
        sb = plain_batch("XL", 1234, "meanstd", 5, True, n_streams=S, backend="native", max_frames=160, max_tokens=200,
                         pcm_capacity=1 << 17)
        sb.set_queue_depth(2)
        if on:
            sb.set_activity(True, 0.0005)          # (the plain synthetic model: blank posteriors around 1 / 1024)
        pos = [0] * S
        replies, frames = {}, 0

        def nxt(s):
            a, e = pos[s], min(pos[s] + chunk, lens[s])
            pos[s] = e
            return (s, audio[s][a:e], e >= lens[s])

        sb.submit([nxt(s) for s in range(S)])
        sb.submit([nxt(s) for s in range(S) if pos[s] < lens[s]])
        while sb.outstanding:
            ids = sorted(sb.poll(1))
            a = sb.hypotheses_arrays(ids)
            for i, s in enumerate(ids):
                replies.setdefault(s, []).append((a["ids"][i].tobytes(), a["xpos"][i].tobytes(), a["lens"][i].tobytes(),
                                                  a["score"][i].tobytes(), a["score_dec"][i].tobytes(),
                                                  a["score_ctc"][i].tobytes()))
            if on:
                act = sb.activity(ids)
                frames += int(act["n_frames"].sum())
                assert (act["n_bad"] == 0).all() and (act["n_speech"] <= act["n_frames"]).all()
            again = [nxt(s) for s in ids if pos[s] < lens[s]]
            if again:
                sb.submit(again)
        return replies, frames

    plain, _ = run(False)
    scanned, frames = run(True)
    assert frames > 0
    assert plain == scanned


def test_server_loop_on_the_native_engine_finalises_at_the_predicted_chunk():
    from speechcatcher_amd.scheduler import StreamScheduler
    from speechcatcher_amd.server_session import AcousticEndpointer, EndpointRules, ServerLoop, scale_server_pcm
    n, w = 9, _weights("TINY")
    a = synth.synth_audio(5, CHUNK * n)
    pcm = [np.clip(np.round(a[k * CHUNK:(k + 1) * CHUNK] * 32767.0), -32768, 32767).astype(np.int16) for k in range(n)]
    sb = make_batch("TINY", "native", 1, weights=w, **KW)
    T = []
    for k in range(n):                                           # what the server feeds, all chunks non-final
        sb.push([(0, scale_server_pcm(pcm[k]), False)])
        T.append(int(sb.st[0].T_enc))
    # the table of the last decode block: the frames of every chunk but the last, all a decision before chunk n - 1 needs
    ref = R.p_blank(sb.read_ctc(0), sb.cfg.blank_id)
    assert len(ref) >= T[-2]
    thr, gap = pick_threshold(ref)
    assert gap > 1e-3
    rules = EndpointRules(silence_after_speech=0.8, silence_without_speech=100.0, max_utterance=100.0)
    ep = AcousticEndpointer(rules)
    fires = [ep.fires(R.as_dict(R.scan(R.INITIAL, ref[:t], thr))) for t in T[:-1]]
    want = fires.index(True) + 1                                 # the chunk after the first reply whose state fires
    assert 2 <= want < n - 1
    finals = []

    class Sch(StreamScheduler):
        def feed(self, sid, pcm, is_final=False, finalize_all=False):
            finals.append(bool(is_final))
            super().feed(sid, pcm, is_final, finalize_all)

    sch = Sch(make_batch("TINY", "native", 1, weights=w, engine=sb.engine, **KW), None, result_format="espnet",
              activity=True, blank_threshold=thr)
    loop = ServerLoop(sch, finalize_update_iters=100, max_partial_iters=1000, acoustic_endpointing=rules)
    sid = loop.connect()
    for k in range(n):
        loop.submit(sid, pcm[k])
        while loop.pending():
            loop.step()
    assert finals[:want + 2] == [False] * want + [True, False], (finals, want)
