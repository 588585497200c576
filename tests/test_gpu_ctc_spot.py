"""CTC phrase spotting on the GPU (csrc/spot.hip: sc_ctc_spot; csrc/streams.hip: sc_streams_set_phrases /
sc_stream_set_phrase_mask / sc_stream_spot / sc_streams_read_spot_events) against the float64 contract of
tests/ctc_spot_ref.py: the kernel on constructed tables - every int32 and float64 bit pattern -, the stream level on the
tiny and the XL synthetic model (lock-step, continuous batching at queue depth 2, the Python engine over the HIP
kernels), and the option's effect on serving (none).

Measured on an MI355X (printed by the tests): kernel against the contract bit-equal in every case; stream
level scores against the contract on the table read back within 2.4e-07 (tiny) / 1.2e-07 (XL), bar 2.4e-06; the Python
engine over the HIP kernels bit-equal to the C++ engine (61 of 61 and 141 of 141 scores)."""
import functools

import numpy as np
import pytest
import torch

import ctc_spot_ref as R
from spot_helpers import make_batch, packed_weights, choose_floors, phrases_from_paths, plant_table, random_phrases, trace_end_values
from speechcatcher_amd import synth
from speechcatcher_amd.spotting import PhraseSet

pytestmark = pytest.mark.gpu

# |score - contract on the table read back| (its first block log-softmaxed in fp32).  Measured on an MI355X (printed by
# test_lockstep_push_...): 2.4e-07 (tiny) / 1.2e-07 (XL).  The bar is ten times the larger value.
SCORE_BAR = 2.4e-6


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


def _strided(x, pad=3):
    """the table on the device as a view with a row stride of V + pad floats (NaN between the rows: never read)"""
    T, V = x.shape
    buf = torch.full((T, V + pad), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :V] = torch.from_numpy(x).to("cuda:0")
    return buf[:, :V]


def _same(name, got, want):
    assert (got["n_frames"], got["n_events"]) == (want["n_frames"], want["n_events"]), \
        (name, got["n_frames"], got["n_events"], want["n_frames"], want["n_events"])
    assert got["values"].tobytes() == want["values"].tobytes(), name
    assert got["starts"].tobytes() == want["starts"].tobytes(), name
    assert R.events_bytes(got["events"]) == R.events_bytes(want["events"]), (name, got["events"][:4], want["events"][:4])
    k = len(want["events"])
    raw = got["raw_events"]
    assert (raw[:k, 3] == 0).all() and (raw[k:] == -7).all(), name   # reserved = 0; nothing behind the stored events


def _run(be, ps, floors, tab, x, blank, spans, name, mask=R.ALL):
    """every span (t0, t1) as a job that starts an utterance, and as a job that carries the contract's state over the rows
    [0, t0) in - ONE launch; both against the contract"""
    phrases = ps.phrases()
    jobs, want, names = [], [], []
    chains = {}   # (t0, carried) -> (state, frames scanned so far): the contract is chained from span end to span end
    for t0, t1 in sorted(spans, key=lambda s: (s[0], s[1])):
        carry = R.scan(R.initial(ps.P), x[:t0], blank, phrases, floors, mask)
        for start, key in ((R.initial(ps.P), "fresh"), (carry, "carried")):
            st, at = chains.get((t0, key), (start, t0))
            st = R.scan(st, x[at:t1], blank, phrases, floors, mask)
            chains[(t0, key)] = (st, t1)
            jobs.append((tab, blank, t0, t1, None if key == "fresh" else carry, mask))
            want.append(st)
            names.append(f"{name}[{t0},{t1}){key}")
    got, after = be.ctc_spot(jobs, ps.labels, ps.lens, floors)
    for k in range(len(jobs)):
        _same(names[k], got[k], want[k])
        assert tuple(after[k]) == (want[k]["n_frames"], want[k]["n_events"]), names[k]
    return want


SPANS = [(3, 3 + n) for n in (0, 1, 63, 64, 65, 129)]


@pytest.mark.parametrize("V,P", [(2, 1), (63, 16), (64, 17), (65, 64), (1024, 64), (1500, 17), (1024, 16)])
def test_kernel_equals_the_contract_bit_for_bit(be, V, P):
    rng = np.random.default_rng(V * 100 + P)
    blank = 0 if V in (2, 1024) else int(rng.integers(0, V))
    phrases = random_phrases(rng, P, V, blank, (1, 2, 31, 32, 3, 5))
    T = 140
    # occurrences: the first phrases of the set, one behind the other, then the short ones again near the tile edge
    plants, f = [], 4
    for p in range(min(P, 6)):
        if f + 2 * len(phrases[p]) < T:
            plants.append((f, phrases[p]))
            f += 2 * len(phrases[p]) - 1 + int(rng.integers(0, 3))
    x, _ = plant_table(rng, T, V, blank, plants)
    floors = np.asarray([-2.0 * len(y) for y in phrases])
    ps = PhraseSet(phrases, floors, V, blank)
    tab = _strided(x)
    assert tab.stride(0) > V
    want = _run(be, ps, floors, tab, x, blank, SPANS, f"V{V}_P{P}")
    full = R.scan(R.initial(P), x, blank, phrases, floors)
    assert full["n_events"] >= 1, "the planted phrases must fire"
    assert any(w["n_events"] for w in want)
    # masks with holes: disabled phrases keep their states (carried) / stay at the utterance's start (fresh)
    if P > 1:
        mask = int(rng.integers(1, 1 << 62)) & ~0b10 | 1
        _run(be, ps, floors, tab, x, blank, [(0, 70), (3, 132)], f"V{V}_P{P}_mask", mask)


def test_kernel_special_rows_repeats_and_fire_patterns(be):
    rng = np.random.default_rng(77)
    V, blank, T = 65, 7, 140
    a, b, c = 3, 11, 64
    phrases = [[a], [b, b], [a, b, c], [a], [c, c, c, a], [b]]      # phrases 0 and 3 are the same: they fire together
    floors = np.asarray([-0.5, -3.0, -4.0, -0.5, -6.0, -1e9])        # phrase 5 fires on every good frame: > 64 events
    plants = [(5, [b, b]), (20, [a, b, c]), (30, [c, c, c, a]), (63, [a]), (64, [a]), (90, [a, b, c]), (100, [b, b])]
    x, ends = plant_table(rng, T, V, blank, plants)
    x[91] = np.nan                                  # a bad row in the middle of an occurrence: it does not complete
    x[40, 2] = np.inf                               # bad: a +inf
    x[41] = -np.inf                                 # bad: nothing but -inf
    x[50, rng.random(V) < 0.5] = -np.inf            # -inf entries are legal ...
    x[50, blank] = 0.0
    x[101, b] = -np.inf                             # ... also at a label of a phrase under way (-inf value, start -1)
    x[110] = np.where(rng.random(V) < 0.5, 1e30, -1e30).astype(np.float32)   # logits of magnitude 1e30
    x[110, a] = 1e30
    x[111] = x[110]
    ps = PhraseSet(phrases, floors, V, blank)
    tab = _strided(x)
    _run(be, ps, floors, tab, x, blank, [(0, T), (0, 65), (63, 65), (60, 129)], "special")
    quiet = R.ALL & ~(1 << 5)                       # ... and without the phrase that fills the event store
    _run(be, ps, floors, tab, x, blank, [(0, T), (0, 65), (63, 65)], "special_quiet", quiet)
    full = R.scan(R.initial(len(phrases)), x, blank, phrases, floors)
    ev = R.scan(R.initial(len(phrases)), x, blank, phrases, floors, quiet)["events"]
    # what the contract says about this table (so the bit comparison above covered these situations)
    assert [(e[0], e[1]) for e in ev if e[1] in (0, 3) and e[0] in (63, 64)] == [(63, 0), (63, 3), (64, 0), (64, 3)]
    assert (ends[1], 2, 20) in [e[:3] for e in ev]              # a b c fires at its planted end with its planted start
    assert not any(e[1] == 2 and 90 <= e[0] <= 95 for e in ev)  # the occurrence the NaN row cut
    assert full["n_events"] > R.MAX_EVENTS == len(full["events"])
    # an adjacent repeat needs its blank: b b planted WITHOUT the blank does not fire phrase 1
    y, _ = plant_table(rng, 12, V, blank, [])
    y[4, b] += 14.0
    y[5, b] += 14.0
    one = R.scan(R.initial(2), y, blank, [[b, b], [b]], np.asarray([-3.0, -0.5]))
    assert [e[1] for e in one["events"]] == [1, 1]
    ps2 = PhraseSet([[b, b], [b]], [-3.0, -0.5], V, blank)
    _run(be, ps2, np.asarray([-3.0, -0.5]), _strided(y), y, blank, [(0, 12)], "repeat_without_blank")


def test_kernel_chained_spans_equal_one_span(be):
    rng = np.random.default_rng(5)
    V, blank = 1024, 0
    spans = (1, 15, 0, 16, 17, 64, 0, 1, 70)
    T = sum(spans)
    phrases = random_phrases(rng, 17, V, blank, (1, 2, 4, 32, 31))
    plants = [(2, phrases[1]), (10, phrases[2]), (30, phrases[3]), (100, phrases[4]), (150, phrases[0]), (170, phrases[2])]
    x, _ = plant_table(rng, T, V, blank, plants)
    x[25, 3] = np.nan
    floors = np.asarray([-2.0 * len(y) for y in phrases])
    ps = PhraseSet(phrases, floors, V, blank)
    tab = _strided(x)
    one, _ = be.ctc_spot([(tab, blank, 0, T, None, R.ALL)], ps.labels, ps.lens, floors)
    want = R.scan(R.initial(ps.P), x, blank, phrases, floors)
    _same("one span", one[0], want)
    assert want["n_events"] >= 5
    st, t0 = None, 0
    for n in spans:
        got, after = be.ctc_spot([(tab, blank, t0, t0 + n, st, R.ALL)], ps.labels, ps.lens, floors)
        st = {k: got[0][k] for k in ("n_frames", "n_events", "values", "starts", "events")}
        t0 += n
        _same(f"chained to {t0}", got[0], R.scan(R.initial(ps.P), x[:t0], blank, phrases, floors))
        assert tuple(after[0]) == (st["n_frames"], st["n_events"])
    _same("chained", got[0], want)


def test_malformed_jobs_write_nothing_and_argument_errors_launch_nothing(be):
    rng = np.random.default_rng(9)
    V, blank = 64, 0
    phrases = [[5, 6], [7]]
    floors = np.asarray([-4.0, -2.0])
    ps = PhraseSet(phrases, floors, V, blank)
    x, _ = plant_table(rng, 20, V, blank, [(3, [5, 6])])
    tab = _strided(x)

    def field(name, value):
        return lambda k, j: setattr(j, name, value) if k == 1 else None

    tweaks = [field("table", None), field("labels", None), field("lens", None), field("floors", None),
              field("counters", None), field("values", None), field("starts", None), field("events", None),
              field("V", 0), field("blank", V), field("blank", -1), field("t0", -1), field("t1", 0), field("stride", V - 1),
              field("P", 0), field("P", 65)]
    sets = [(ps.labels, np.asarray([2, 0], np.int32)), (ps.labels, np.asarray([33, 1], np.int32)),
            (np.where(ps.labels == 6, blank, ps.labels), ps.lens), (np.where(ps.labels == 6, V, ps.labels), ps.lens),
            (np.where(ps.labels == 7, -1, ps.labels), ps.lens)]
    want = R.scan(R.initial(2), x[1:20], blank, phrases, floors)
    for i, tw in enumerate(tweaks + [None] * len(sets)):
        labels, lens = (ps.labels, ps.lens) if tw is not None else sets[i - len(tweaks)]
        got, after = be.ctc_spot([(tab, blank, 1, 20, None, R.ALL)] * 3, labels, lens, floors, tweak=tw)
        for k in ((1,) if tw is not None else (0, 1, 2)):     # the malformed job(s): nothing written
            assert (got[k]["n_frames"], got[k]["n_events"]) == (-7, -7) and tuple(after[k]) == (-7, -7), i
            assert (got[k]["values"] == -7.0).all() and (got[k]["starts"] == -7).all() and (got[k]["raw_events"] == -7).all(), i
        if tw is not None:                                     # its neighbours in the same launch are served
            _same(f"neighbour {i}", got[0], want)
            _same(f"neighbour {i}", got[2], want)
    from speechcatcher_amd import _abi
    lib = _abi.load()
    assert lib.sc_ctc_spot(None, 0, None) == 0
    assert lib.sc_ctc_spot(None, 2, None) == -1 and lib.sc_ctc_spot(None, -1, None) == -1
    assert lib.sc_ctc_spot(tab.data_ptr(), _abi.SPOT_MAX_JOBS + 1, None) == -1


# ---- stream level ----------------------------------------------------------------------------------------------------
CHUNK = 10240
SHAPE = {"TINY": (2, 8), "XL": (8, 6)}      # streams, chunks
N_PHRASES = 16
KW = dict(max_frames=160, max_tokens=200, pcm_capacity=1 << 17)


@functools.lru_cache(maxsize=None)
def _weights(name):
    return packed_weights(name, "cuda:0")


@pytest.fixture(scope="module", params=["TINY", "XL"])
def probe(request):
    """per model, computed once: the weights, the audio, the frames after every chunk, the CTC tables read back from the
    C++ engine, phrases from their collapsed arg-max paths, floors in the widest gaps of the phrases' end-state values
    and the contract's run over the tables"""
    name = request.param
    S, n = SHAPE[name]
    w = _weights(name)
    sb = make_batch(name, "native", S, weights=w, **KW)
    audio = [synth.synth_audio(5 + s, CHUNK * n - 1000 * s) for s in range(S)]
    T = [[] for _ in range(S)]
    for k in range(n):
        sb.push([(s, audio[s][k * CHUNK:(k + 1) * CHUNK], k == n - 1) for s in range(S)])
        for s in range(S):
            T[s].append(int(sb.st[s].T_enc))
    table = [sb.read_ctc(s) for s in range(S)]
    assert [len(t) for t in table] == [t[-1] for t in T]
    blank = sb.cfg.blank_id
    # (no one-token phrases: such a phrase fires on every frame its token leads, the event store overflows)
    phrases = phrases_from_paths(table, blank, 2 * N_PHRASES, lengths=(2, 3, 4, 5))
    phrases, floors = choose_floors(table, blank, phrases, N_PHRASES)
    # the condition: with these floors no end-state value of any frame of any stream lies within 1e-3 of its floor
    ref, snaps, closest = [], [], np.inf
    for s in range(S):
        st, v, sn = trace_end_values(table[s], blank, phrases, floors, snap_at=set(T[s]))
        ref.append(st)
        snaps.append(sn)
        for p in range(N_PHRASES):
            closest = min(closest, np.abs(np.asarray(v[p]) - floors[p]).min(initial=np.inf))
    assert closest >= 1e-3, closest
    assert sum(st["n_events"] for st in ref) >= N_PHRASES // 2
    return {"name": name, "S": S, "n": n, "w": w, "engine": sb.engine, "audio": audio, "T": T, "table": table,
            "blank": blank, "phrases": phrases, "floors": floors, "ref": ref, "snaps": snaps}


def _chunks(p, k):
    return [(s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == p["n"] - 1) for s in range(p["S"])]


def _snapshot(sb, s):
    c = sb.spot([s])
    return int(c["n_frames"][0]), int(c["n_events"][0]), sb.spot_events(s)


def _want(p, s, k):
    """the contract's state over the frames stream s had after chunk k"""
    return p["snaps"][s][p["T"][s][k]]


@pytest.fixture(scope="module")
def pushed(probe):
    """the lock-step run with the option on: (n_frames, n_events, events) of every stream after every chunk, and the
    state blocks at the end"""
    p = probe
    sb = make_batch(p["name"], "native", p["S"], weights=p["w"], engine=p["engine"], **KW)
    with pytest.raises(Exception):
        sb.spot([0])                                             # off by default
    sb.set_phrases(p["phrases"], p["floors"])
    assert _snapshot(sb, 0) == (0, 0, [])
    snaps = []
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
        snaps.append([_snapshot(sb, s) for s in range(p["S"])])
    states = [sb.read_spot_state(s) for s in range(p["S"])]
    return {"sb": sb, "snaps": snaps, "states": states}


def test_lockstep_push_equals_the_contract_on_the_table_read_back(probe, pushed):
    p, worst = probe, 0.0
    for k in range(p["n"]):
        for s in range(p["S"]):
            nf, ne, ev = pushed["snaps"][k][s]
            want = _want(p, s, k)
            assert nf == p["T"][s][k] == want["n_frames"] and ne == want["n_events"], (s, k)
            assert [(e[1], e[2], e[0]) for e in ev] == [(e[1], e[2], e[0]) for e in want["events"]], (s, k)
            worst = max([worst] + [abs(a[3] - b[3]) for a, b in zip(ev, want["events"])])
    print(f"\n{p['name']}: largest |score - contract on the table read back| = {worst:.3e}")
    assert worst <= SCORE_BAR
    sb = pushed["sb"]
    sb.reset(0)
    assert _snapshot(sb, 0) == (0, 0, [])
    assert _snapshot(sb, 1) == pushed["snaps"][-1][1]           # the other stream keeps its state
    with pytest.raises(Exception):
        sb.set_phrases([[p["blank"]]])                           # the blank is no label
    with pytest.raises(Exception):
        sb.set_phrases([[sb.cfg.vocab_size]])
    sb.set_phrases([])
    with pytest.raises(Exception):
        sb.spot([0])


def test_continuous_queue_depth_2_is_bit_identical_to_push(probe, pushed):
    p = probe
    S, n = p["S"], p["n"]
    sb = make_batch(p["name"], "native", S, weights=p["w"], engine=p["engine"], **KW)
    sb.set_queue_depth(2)
    sb.set_phrases(p["phrases"], p["floors"])
    nxt, rep = [0] * S, [0] * S

    def feed(s):
        k = nxt[s]
        nxt[s] += 1
        return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == n - 1)

    sb.submit([feed(s) for s in range(S)])
    with pytest.raises(Exception):
        sb.set_phrases(p["phrases"], p["floors"])                # refused while chunks are outstanding
    sb.submit([feed(s) for s in range(S)])
    while sb.outstanding:
        done = sb.poll(1)
        for s in sorted(done):
            nf, ne, ev = _snapshot(sb, s)                        # of the chunk that was REPORTED
            wf, we, wev = pushed["snaps"][rep[s]][s]
            assert (nf, ne) == (wf, we) and R.events_bytes(ev) == R.events_bytes(wev), (s, rep[s])
            rep[s] += 1
        again = [feed(s) for s in sorted(done) if nxt[s] < n]
        if again:
            sb.submit(again)
    assert rep == [n] * S
    for s in range(S):
        v, st = sb.read_spot_state(s)
        assert v.tobytes() == pushed["states"][s][0].tobytes() and st.tobytes() == pushed["states"][s][1].tobytes(), s


def test_python_engine_on_the_hip_backend_gives_the_same_events(probe, pushed):
    p = probe
    from speechcatcher_amd.hip_backend import HipBackend
    sb = make_batch(p["name"], HipBackend("cuda:0"), p["S"], weights=p["w"], **KW)
    sb.set_phrases(p["phrases"], p["floors"])
    worst, same_bits, total = 0.0, 0, 0
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
        for s in range(p["S"]):
            nf, ne, ev = _snapshot(sb, s)
            wf, we, wev = pushed["snaps"][k][s]
            assert (nf, ne) == (wf, we), (s, k)
            assert [e[:3] for e in ev] == [e[:3] for e in wev], (s, k)
            if k == p["n"] - 1:
                worst = max([worst] + [abs(a[3] - b[3]) for a, b in zip(ev, wev)])
                same_bits += sum(np.float64(a[3]).tobytes() == np.float64(b[3]).tobytes() for a, b in zip(ev, wev))
                total += len(ev)
    print(f"\n{p['name']}: Python engine over the HIP kernels against the C++ engine: {same_bits} of {total} scores "
          f"bit-equal, largest difference {worst:.3e}")
    assert worst <= SCORE_BAR


def test_mask_disables_phrases_per_stream(probe, pushed):
    p = probe
    sb = make_batch(p["name"], "native", p["S"], weights=p["w"], engine=p["engine"], **KW)
    sb.set_phrases(p["phrases"], p["floors"])
    fired = sorted({e[1] for e in pushed["snaps"][-1][0][2]})
    assert fired, "stream 0 must have events"
    off = fired[0]
    sb.set_phrase_mask(0, R.ALL & ~(1 << off))
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
    nf, ne, ev0 = _snapshot(sb, 0)
    # phrases do not see each other: the run without the phrase is the full run with its events taken out
    full = pushed["snaps"][-1][0]
    assert full[1] <= R.MAX_EVENTS, "the event store of stream 0 must not overflow for this comparison"
    assert R.events_bytes(ev0) == R.events_bytes([e for e in full[2] if e[1] != off]) and ne == len(ev0) < full[1]
    assert _snapshot(sb, 1) == pushed["snaps"][-1][1]           # the other stream: every phrase


def test_spotting_has_no_effect_on_serving():
    """XL, 8 streams of 6 chunks under continuous batching (queue depth 2): hypotheses, positions and scores of every
    reply are bit-identical with the option on (and read after every reply) and off."""
    from test_engine_spec import make_batch as plain_batch
    S, chunk, n = 8, 10240, 6
    lens = [chunk * n - 977 * i for i in range(S)]
    audio = [synth.synth_audio(300 + i, m) for i, m in enumerate(lens)]

    def run(on):
        sb = plain_batch("XL", 1234, "meanstd", 5, True, n_streams=S, backend="native", max_frames=160, max_tokens=200,
                         pcm_capacity=1 << 17)
        sb.set_queue_depth(2)
        if on:
            rng = np.random.default_rng(3)
            sb.set_phrases(random_phrases(rng, 16, sb.cfg.vocab_size, sb.cfg.blank_id, (1, 2, 3, 8)))
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
                frames += int(sb.spot(ids)["n_frames"].sum())
                for s in ids:
                    sb.spot_events(s)
            again = [nxt(s) for s in ids if pos[s] < lens[s]]
            if again:
                sb.submit(again)
        return replies, frames

    plain, _ = run(False)
    scanned, frames = run(True)
    assert frames > 0
    assert plain == scanned
