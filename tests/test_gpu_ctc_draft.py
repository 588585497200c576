"""CTC draft transcript on the GPU (csrc/draft.hip: sc_ctc_draft; csrc/streams.hip: sc_streams_set_draft /
sc_stream_draft / sc_streams_read_draft) against the float64 contract of tests/ctc_draft_ref.py: the kernel on
constructed tables - every int32 equal, conf within 1e-12 -, the stream level on the tiny and the XL synthetic model
(lock-step, continuous batching at queue depth 2, the Python engine over the HIP kernels), and the option's effect on
serving (none).

Measured on an MI355X (printed by the tests): kernel against the contract, largest |conf - contract|
2.6e-15 (bar 1e-12); stream level conf against the posteriors of the table read back within 8.0e-11 (tiny) / 9.4e-11
(XL), bar 1e-5; the Python engine over the HIP kernels within 1.9e-17 of the C++ engine; smallest gap between a row's
best entry and its runner-up on the tables read back 1.1e-3 (tiny) / 3.3e-4 (XL), condition 1e-4."""
import functools

import numpy as np
import pytest
import torch

import ctc_draft_ref as R
from draft_helpers import MODELS, make_batch, packed_weights, path_mix
from speechcatcher_amd import synth

pytestmark = pytest.mark.gpu

# |conf - contract| on the same fp32 rows: the bar 8d set for the same float64 sum in another order (measured there: 6.7e-15)
CONF_BAR = 1e-12
# |conf - posterior of the row read back| (its first block log-softmaxed in fp32): 8d's bar for the same comparison
READBACK_BAR = 1e-5
# the condition of the comparison with the table read back: every row's best entry this far above its runner-up, so that
# the in-place fp32 log-softmax cannot create a tie
MIN_GAP = 1e-4
TILE = 256   # DR_TILE of csrc/draft.hip
A, B, C = 1, 5, 9


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


def _runs(rng, T, choices, longest):
    labels = []
    while len(labels) < T:
        labels += [choices[int(rng.integers(len(choices)))]] * int(rng.integers(1, longest + 1))
    return labels[:T]


def _table(labels, V, rng, lead=4.0):
    """one row per label: unit noise, the label's entry ahead by `lead`; None: a bad row (NaN, +inf or all -inf in turn)"""
    x = rng.standard_normal((len(labels), V)).astype(np.float32)
    for t, lab in enumerate(labels):
        if lab is None:
            if t % 3 == 0:
                x[t, int(rng.integers(V))] = np.nan
            elif t % 3 == 1:
                x[t, int(rng.integers(V))] = np.inf
            else:
                x[t] = -np.inf
        else:
            x[t, lab] = x[t].max() + np.float32(lead)
    return x


def _state_dict(st, store):
    d = R.as_dict(st)
    d["tokens"] = list(store)
    return d


WORST = {"conf": 0.0}


def _same(name, got, after, want, wstore, cap, sentinels=True):
    """every int32 of state and store equal, conf within CONF_BAR, the second copy the same bytes, nothing written behind
    min(n_closed, capacity)"""
    ints = tuple(got[f] for f in R.FIELDS[:6])
    assert ints == tuple(want[:6]), (name, ints, want)
    assert abs(got["open_conf"] - want[6]) <= CONF_BAR, (name, got["open_conf"], want[6])
    assert after[:6] == ints and np.float64(after[6]).tobytes() == np.float64(got["open_conf"]).tobytes(), (name, after)
    k = min(want[1], cap)
    assert len(wstore) == k and len(got["tokens"]) == k, (name, len(got["tokens"]), k)
    assert [t[:3] for t in got["tokens"]] == [t[:3] for t in wstore], name
    err = max([abs(got["open_conf"] - want[6])] + [abs(a[3] - b[3]) for a, b in zip(got["tokens"], wstore)])
    assert err <= CONF_BAR, (name, err)
    WORST["conf"] = max(WORST["conf"], err)
    raw = got["raw_tokens"]
    assert (raw[:k, 3] == 0).all(), name                             # reserved = 0
    if sentinels:
        assert (raw[k:] == -7).all(), name                           # nothing behind the stored tokens


def _run(be, x, blank, spans, name, cap=None, tab=None):
    """every span (t0, t1) as a job that starts an utterance, and as a job that carries the contract's state and store
    over the rows [0, t0) in - ONE launch; both against the contract"""
    tab = _strided(x) if tab is None else tab
    cap = len(x) + 1 if cap is None else cap
    lab, p = R.rows(x, blank)
    jobs, want = [], []
    for t0, t1 in spans:
        store = []
        st = R.scan(R.INITIAL, lab[t0:t1], p[t0:t1], blank, store, cap)
        jobs.append((tab, blank, t0, t1, None, cap))
        want.append((st, store))
        store = []
        carry = R.scan(R.INITIAL, lab[:t0], p[:t0], blank, store, cap)
        carried = _state_dict(carry, store)
        st = R.scan(carry, lab[t0:t1], p[t0:t1], blank, store, cap)
        jobs.append((tab, blank, t0, t1, carried, cap))
        want.append((st, store))
    got, after = be.ctc_draft(jobs)
    for i, (g, a, (st, store)) in enumerate(zip(got, after, want)):
        _same(f"{name} span {spans[i // 2]} {'carried' if i % 2 else 'restart'}", g, a, st, store, cap)
    return got


SPANS = [(0, 0), (0, 1), (0, 63), (0, 64), (0, 65), (0, 129), (0, TILE - 1), (0, TILE), (0, TILE + 1), (7, 7), (1, 2),
         (40, 300), (63, 65), (TILE - 1, TILE + 1), (TILE, 300), (300, 300)]


# ---- the kernel against the contract ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1024, 1500])
def test_kernel_equals_the_contract_at_every_width_and_span(be, V):
    rng = np.random.default_rng(V)
    blank = 0
    toks = [v for v in (A, B, C, V - 1, V // 2) if 0 < v < V]
    labels = _runs(rng, 300, [blank, None] + 3 * toks, 4)
    x = _table(labels, V, rng)
    lab, _ = R.rows(x, blank)
    assert (lab == R.BAD).sum() >= 10 and (lab == blank).sum() >= 10 and (V == 1 or (lab > 0).sum() >= 100)
    _run(be, x, blank, SPANS, f"V={V}")
    if V > 2:                                                         # another blank than 0: the last id
        _run(be, x, V - 1, SPANS[3:9], f"V={V} blank={V - 1}")
    print(f"\nV={V}: largest |conf - contract| so far {WORST['conf']:.3e}")


def test_runs_across_batch_tile_and_span_boundaries_chained_spans_equal_one_span(be):
    rng = np.random.default_rng(1)
    V, blank, T = 65, 0, 700
    labels = _runs(rng, T, [blank, A, B, A, C, None], 40)
    labels[60:70] = [B] * 10                                          # across the first 64-frame batch
    labels[250:262] = [C] * 12                                        # across the first tile
    labels[262:270] = [blank] * 8
    labels[299:300], labels[300:420], labels[420:421] = [blank], [B] * 120, [blank]   # longer than a batch, one token
    labels[500:530] = [A] * 30                                        # across a span boundary (and the second tile)
    x = _table(labels, V, rng)
    tab = _strided(x)
    lab, p = R.rows(x, blank)
    one_store = []
    one = R.scan(R.INITIAL, lab, p, blank, one_store, T)
    assert one[1] >= 8 and max(t[2] - t[1] for t in one_store) >= 64
    _run(be, x, blank, [(0, T), (60, 70), (250, 262), (200, 700)], "long runs", tab=tab)
    cuts = [0, 0, 10, 64, 64, 65, 200, 256, 300, 512, 515, 515, 700]
    state = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        (state,), (after,) = be.ctc_draft([(tab, blank, a, b, state, T)])
        store = []
        want = R.scan(R.INITIAL, lab[:b], p[:b], blank, store, T)
        _same(f"chain [{a}, {b})", state, after, want, store, T)
    _same("chain end", state, after, one, one_store, T)


def test_a_carried_open_token_on_the_first_frame_and_restart(be):
    rng = np.random.default_rng(2)
    V, blank = 64, 0
    carried = {"n_frames": 10, "n_closed": 2, "n_bad": 1, "open_id": A, "open_start": 7, "open_end": 9, "open_conf": 0.25,
               "tokens": [(B, 0, 1, 0.5), (C, 3, 4, 0.625)]}
    first = {"continued": [A, A, blank], "continued to the end": [A, A, A], "closed by a blank": [blank, A, A],
             "closed by another label": [B, B, A], "closed by a bad row": [None, A, blank], "one frame": [A],
             "one blank": [blank]}
    jobs, want = [], []
    for name, labels in first.items():
        x = _table(labels, V, rng)
        lab, p = R.rows(x, blank)
        store = list(carried["tokens"])
        st = R.scan(tuple(carried[f] for f in R.FIELDS), lab, p, blank, store, 16)
        jobs.append((_strided(x), blank, 0, len(labels), carried, 16))
        want.append((name, st, store))
    got, after = be.ctc_draft(jobs)
    for g, a, (name, st, store) in zip(got, after, want):
        _same(name, g, a, st, store, 16)
    assert got[0]["tokens"][2][:3] == (A, 7, 11) and got[0]["tokens"][2][3] >= 0.25 and got[0]["n_closed"] == 3
    assert (got[1]["open_start"], got[1]["open_end"]) == (7, 12) and got[1]["open_conf"] >= 0.25
    # restart: the stored state is ignored
    x = _table([A, A, blank, B], V, rng)
    lab, p = R.rows(x, blank)
    store = []
    st = R.scan(R.INITIAL, lab, p, blank, store, 16)

    def restart(k, j):
        j.restart = 1

    got, after = be.ctc_draft([(_strided(x), blank, 0, 4, carried, 16)], tweak=restart)
    _same("restart", got[0], after[0], st, store, 16, sentinels=False)
    # an empty span rewrites the state unchanged (and with restart: the initial state)
    got, after = be.ctc_draft([(_strided(x), blank, 2, 2, carried, 16), (_strided(x), blank, 2, 2, None, 16)])
    _same("empty", got[0], after[0], tuple(carried[f] for f in R.FIELDS), carried["tokens"], 16)
    _same("empty restart", got[1], after[1], R.INITIAL, [], 16)


def test_ties_take_the_lowest_index(be):
    V = 200
    rows, blanks = [], (0, 70)

    def row(hot, rest=-3.0):
        x = np.full(V, rest, np.float32)
        for k, v in hot.items():
            x[k] = v
        return x

    for v in (3, 64, 100, 135):
        rows.append(row({v: 2.0, v + 64: 2.0}))                       # the same lane of the row pass: (v, v + 64)
    rows.append(row({V - 1: 1.0, 17: 1.0}))                           # a tie with the last entry
    rows.append(row({V - 1: 1.0}))                                    # the last entry alone
    rows.append(row({V - 1: 1.0, V - 2: 1.0}))
    rows.append(row({0: 1.0, 6: 1.0}))                                # blank 0 against a token: the blank
    rows.append(row({70: 1.0, 6: 1.0}))                               # blank 70 against a lower token: the token
    rows.append(row({70: 1.0, 90: 1.0}))                              # blank 70 against a higher token: the blank
    rows.append(row({}, rest=0.5))                                    # all equal: index 0
    rows.append(row({k: 4.0 for k in range(5, V, 7)}))                # many maxima over all lanes
    x = np.stack(rows)
    lab, _ = R.rows(x, 0)
    assert lab.tolist() == [3, 64, 100, 135, 17, V - 1, V - 2, 0, 6, 70, 0, 5]
    for blank in blanks:
        _run(be, x, blank, [(0, len(x)), (4, 9), (7, 10)], f"ties blank={blank}")


def test_minus_inf_entries_huge_logits_and_bad_rows_inside_a_run(be):
    rng = np.random.default_rng(4)
    V, blank = 130, 0
    x = _table([A] * 12 + [B] * 6 + [blank] + [C] * 5, V, rng)
    x[1, 10:90] = -np.inf                                             # -inf entries beside finite ones: no fault
    x[2, :] = -np.inf
    x[2, A] = 0.0                                                     # one finite entry: p = 1
    x[3, :] = -1e30
    x[3, A] = x[3, 77] = 1e30                                         # logits of 1e30, tied: p = 1 for the lower one
    x[4, :] = 1e30
    x[4, A] = np.float32(1.0000001e30)
    x[6, 40] = np.nan                                                 # bad rows inside the run of A
    x[8, 41] = np.inf
    x[10, :] = -np.inf
    x[14, A] = np.nan                                                 # ... and inside the run of B
    lab, p = R.rows(x, blank)
    assert lab[:12].tolist() == [A, A, A, A, A, A, R.BAD, A, R.BAD, A, R.BAD, A] and p[2] == p[3] == p[4] == 1.0
    got = _run(be, x, blank, [(0, len(x)), (3, 5), (5, 16)], "inf")
    assert got[0]["n_bad"] == 4 and [t[:3] for t in got[0]["tokens"]][:2] == [(A, 0, 5), (A, 7, 7)]
    assert got[0]["tokens"][0][3] == 1.0


def test_all_blank_and_no_blank_tables(be):
    rng = np.random.default_rng(5)
    V, blank = 67, 3
    x = _table([blank] * 200, V, rng)
    got = _run(be, x, blank, [(0, 200), (0, 64), (10, 150)], "all blank")
    assert got[0]["n_closed"] == 0 and got[0]["open_id"] == -1 and got[0]["tokens"] == []
    x = _table(_runs(rng, 300, [A, B, C, 66], 3), V, rng)
    got = _run(be, x, blank, [(0, 300), (0, 64), (10, 150)], "no blank")
    assert got[0]["n_closed"] >= 90 and got[0]["open_id"] >= 0
    x = _table([A if t % 2 else B for t in range(200)], V, rng)       # a new token on every frame: 64 runs per batch
    got = _run(be, x, blank, [(0, 200), (1, 129)], "every frame")
    assert got[0]["n_closed"] == 199


def test_a_capacity_of_4_with_6_tokens_counts_and_writes_nothing_behind_it(be):
    rng = np.random.default_rng(6)
    V, blank = 67, 0
    x = _table([A, blank, B, blank, C, C, blank, A, None, B, B, blank, C, blank], V, rng)
    got = _run(be, x, blank, [(0, 14), (3, 14), (9, 14)], "capacity 4", cap=4)
    assert got[0]["n_closed"] == 6 and len(got[0]["tokens"]) == 4 and (got[0]["raw_tokens"][4:] == -7).all()
    got = _run(be, x, blank, [(0, 14)], "capacity 0", cap=0)
    assert got[0]["n_closed"] == 6 and (got[0]["raw_tokens"] == -7).all()


def test_nan_rows_outside_the_span_are_not_read(be):
    rng = np.random.default_rng(7)
    V, blank = 65, 0
    x = _table(_runs(rng, 120, [blank, A, B, C], 5), V, rng)
    poisoned = np.full_like(x, np.nan)
    poisoned[20:90] = x[20:90]
    tab = _strided(poisoned)
    lab, p = R.rows(x, blank)
    store = []
    want = R.scan(R.INITIAL, lab[20:90], p[20:90], blank, store, 200)
    got, after = be.ctc_draft([(tab, blank, 20, 90, None, 200)])
    _same("poison", got[0], after[0], want, store, 200)
    assert got[0]["n_bad"] == 0


def test_a_malformed_job_writes_nothing_while_its_neighbours_are_served(be):
    rng = np.random.default_rng(8)
    V, blank = 65, 0
    x = _table(_runs(rng, 100, [blank, A, B, C], 5), V, rng)
    tab = _strided(x)
    lab, p = R.rows(x, blank)
    store = []
    want = R.scan(R.INITIAL, lab, p, blank, store, 128)

    def setter(**kw):
        def tweak(k, j):
            if k == 1:
                for f, v in kw.items():
                    setattr(j, f, v)
        return tweak

    bad = [dict(table=None), dict(state=None), dict(tokens=None), dict(V=0), dict(blank=-1), dict(blank=V), dict(t0=-1),
           dict(t0=50, t1=49), dict(stride=V - 1), dict(capacity=-1), None]
    for i, kw in enumerate(bad):
        got, after = be.ctc_draft([(tab, blank, 0, 100, None, 128)] * 3, tweak=setter(**kw) if kw else None)
        if kw is not None:
            assert all(got[1][f] == -7 for f in R.FIELDS[:6]) and (got[1]["raw_tokens"] == -7).all(), kw
            if "state" not in kw:                                    # (the second copy of a job without a state: untouched too)
                assert after[1][:6] == (-7,) * 6, kw
        for k in (0, 2) if kw is not None else (0, 1, 2):            # its neighbours in the same launch are served
            _same(f"neighbour {i}.{k}", got[k], after[k], want, store, 128)
    from speechcatcher_amd import _abi
    lib = _abi.load()
    assert lib.sc_ctc_draft(None, 0, None) == 0
    assert lib.sc_ctc_draft(None, 2, None) == -1 and lib.sc_ctc_draft(None, -1, None) == -1
    assert lib.sc_ctc_draft(tab.data_ptr(), _abi.DRAFT_MAX_JOBS + 1, None) == -1


# ---- stream level ----------------------------------------------------------------------------------------------------
CHUNK = 10240
SHAPE = {"TINY": (2, 8), "XL": (8, 6)}      # streams, chunks
# audio seeds per stream slot: picked on the CPU spec engine so that with each of the three models every CTC row's best
# entry lies at least 3e-4 above its runner-up, raw and after an fp32 log-softmax, and no arg-max moves under it
SEEDS = {"TINY": [7, 10], "XL": [5, 6, 7, 8, 9, 10, 11, 12]}
KW = dict(max_frames=160, max_tokens=200, pcm_capacity=1 << 17)


@functools.lru_cache(maxsize=None)
def _weights(model, name):
    return packed_weights(model, name, "cuda:0")


def _snapshot(sb, s):
    d = sb.draft([s])
    return tuple(int(d[k][0]) for k in R.FIELDS[:6]) + (float(d["open_conf"][0]),), sb.draft_tokens(s)


def _bits(snap):
    st, toks = snap
    return st[:6], np.asarray([st[6]] + [v for t in toks for v in t], np.float64).tobytes()


@pytest.fixture(scope="module", params=[(n, m) for n in ("TINY", "XL") for m in MODELS], ids=lambda p: f"{p[0]}-{p[1]}")
def probe(request):
    """per model, computed once: the weights, the audio, the lock-step run of the C++ engine with the option on - state
    and draft of every stream after every chunk -, the CTC tables read back and the contract's run over them"""
    name, model = request.param
    S, n = SHAPE[name]
    w = _weights(model, name)
    sb = make_batch(model, name, "native", S, weights=w, **KW)
    with pytest.raises(Exception):
        sb.draft([0])                                                 # off by default
    with pytest.raises(Exception):
        sb.draft_tokens(0)
    sb.set_draft(True)
    assert _snapshot(sb, 0) == (R.INITIAL, [])
    audio = [synth.synth_audio(SEEDS[name][s], CHUNK * n - 1000 * s) for s in range(S)]
    T, snaps = [[] for _ in range(S)], []
    for k in range(n):
        sb.push([(s, audio[s][k * CHUNK:(k + 1) * CHUNK], k == n - 1) for s in range(S)])
        for s in range(S):
            T[s].append(int(sb.st[s].T_enc))
        snaps.append([_snapshot(sb, s) for s in range(S)])
    table = [sb.read_ctc(s) for s in range(S)]
    assert [len(t) for t in table] == [t[-1] for t in T]
    blank = sb.cfg.blank_id
    return {"name": name, "model": model, "S": S, "n": n, "w": w, "engine": sb.engine, "audio": audio, "T": T,
            "table": table, "blank": blank, "snaps": snaps, "sb": sb}


def _chunks(p, k):
    return [(s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == p["n"] - 1) for s in range(p["S"])]


def test_lockstep_push_equals_the_contract_on_the_table_read_back(probe):
    p, worst, gap, n_tok = probe, 0.0, np.inf, 0
    for s in range(p["S"]):                                          # the condition, before anything is compared
        srt = np.sort(p["table"][s], 1)
        gap = min(gap, float((srt[:, -1] - srt[:, -2]).min()))
        path_mix(p["model"], p["table"][s], p["blank"])
    print(f"\n{p['name']}-{p['model']}: smallest gap between a row's best entry and its runner-up {gap:.3e}")
    assert gap >= MIN_GAP
    for s in range(p["S"]):
        lab, post = R.rows(p["table"][s], p["blank"])
        for k in range(p["n"]):
            t = p["T"][s][k]
            store = []
            want = R.scan(R.INITIAL, lab[:t], post[:t], p["blank"], store, 1 << 30)
            st, toks = p["snaps"][k][s]
            assert st[:6] == want[:6], (s, k, st, want)
            assert [x[:3] for x in toks] == [x[:3] for x in R.draft(want, store)], (s, k)
            worst = max([worst, abs(st[6] - want[6])] + [abs(a[3] - b[3]) for a, b in zip(toks, R.draft(want, store))])
        n_tok += len(toks)
    print(f"{p['name']}-{p['model']}: {n_tok} draft tokens; largest |conf - posterior of the table read back| = {worst:.3e}")
    assert worst <= READBACK_BAR
    assert n_tok >= 8 * p["S"] or p["model"] == "blanks"
    sb = p["sb"]
    sb.reset(0)
    assert _snapshot(sb, 0) == (R.INITIAL, [])
    assert _snapshot(sb, 1) == p["snaps"][-1][1]                     # the other stream keeps its state
    sb.set_draft(False)
    with pytest.raises(Exception):
        sb.draft([0])


def test_continuous_queue_depth_2_is_bit_identical_to_push(probe):
    p = probe
    S, n = p["S"], p["n"]
    sb = make_batch(p["model"], p["name"], "native", S, weights=p["w"], engine=p["engine"], **KW)
    sb.set_queue_depth(2)
    sb.set_draft(True)
    nxt, rep, queued_behind = [0] * S, [0] * S, 0

    def feed(s):
        k = nxt[s]
        nxt[s] += 1
        return (s, p["audio"][s][k * CHUNK:(k + 1) * CHUNK], k == n - 1)

    sb.submit([feed(s) for s in range(S)])
    with pytest.raises(Exception):
        sb.set_draft(True)                                           # refused while chunks are outstanding
    sb.submit([feed(s) for s in range(S)])
    while sb.outstanding:
        done = sb.poll(1)
        for s in sorted(done):
            queued_behind += nxt[s] > rep[s] + 1                     # a later chunk of the stream is at the engine:
            got = _snapshot(sb, s)                                   # the state of the chunk that was REPORTED
            assert _bits(got) == _bits(p["snaps"][rep[s]][s]), (s, rep[s])
            rep[s] += 1
        again = [feed(s) for s in sorted(done) if nxt[s] < n]
        if again:
            sb.submit(again)
    assert rep == [n] * S and queued_behind >= S


def test_python_engine_on_the_hip_backend_gives_the_same_draft(probe):
    p = probe
    from speechcatcher_amd.hip_backend import HipBackend
    sb = make_batch(p["model"], p["name"], HipBackend("cuda:0"), p["S"], weights=p["w"], **KW)
    sb.set_draft(True)
    worst = 0.0
    for k in range(p["n"]):
        sb.push(_chunks(p, k))
        for s in range(p["S"]):
            st, toks = _snapshot(sb, s)
            wst, wtoks = p["snaps"][k][s]
            assert st[:6] == wst[:6], (s, k)
            assert [t[:3] for t in toks] == [t[:3] for t in wtoks], (s, k)
            worst = max([worst, abs(st[6] - wst[6])] + [abs(a[3] - b[3]) for a, b in zip(toks, wtoks)])
    print(f"\n{p['name']}-{p['model']}: Python engine over the HIP kernels against the C++ engine: largest |conf| "
          f"difference {worst:.3e}")
    assert worst <= CONF_BAR


def test_the_draft_has_no_effect_on_serving():
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
            sb.set_draft(True)
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
                frames += int(sb.draft(ids)["n_frames"].sum())
                for s in ids:
                    sb.draft_tokens(s)
            again = [nxt(s) for s in ids if pos[s] < lens[s]]
            if again:
                sb.submit(again)
        return replies, frames

    plain, _ = run(False)
    scanned, frames = run(True)
    assert frames > 0
    assert plain == scanned
