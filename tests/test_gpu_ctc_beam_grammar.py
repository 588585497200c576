"""Grammar-constrained CTC prefix beam search on the GPU (csrc/ctc_beam_grammar.hip: sc_ctc_beam_grammar) against the
float64 contract of tests/ctc_beam_grammar_ref.py on constructed tables and grammars: every int32 and every g equal -
entry order, node, last, len, parent, the counters, every stored node record, the sentinels behind the store -, pb / pnb
within 64 n_frames 2^-53 max(1, |want|) (the bar of tests/test_gpu_ctc_beam.py: the device functions are the same) and
-inf exactly; chained spans bit for bit the one-span run; the free grammar the bytes of sc_ctc_beam.

The integers can only be equal where no prune decision is a near-tie: every case first asserts, on the CPU from the
contract alone, that every gap between consecutive kept totals and between the B-th and the (B+1)-th is exactly 0 or at
least MIN_GAP = 1e-6; no case is skipped for it - the seeds are picked so that it holds.

Measured on an MI355X (printed by the tests): largest |pb, pnb - contract| 4.5e-13 at 300 frames = 0.0036 of
the bar; smallest non-zero prune gap of the parametrised cases 4.6e-6."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_grammar_ref as G
import ctc_beam_ref as R
from speechcatcher_amd import grammar

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-6
TILE = 256   # GB_TILE of csrc/ctc_beam_grammar.hip
NEG = -np.inf
BAR = lambda n_frames, want: 64.0 * max(n_frames, 1) * 2.0 ** -53 * max(1.0, abs(want))   # noqa: E731
T = 300
CUTS = [0, 17, 256, 300]


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


@functools.lru_cache(maxsize=None)
def _device_grammar(blob):
    from speechcatcher_amd import _abi
    from speechcatcher_amd.hip_backend import DeviceGrammar
    return DeviceGrammar(_abi.load(), blob)


def _strided(x, pad=3):
    """the table on the device as a view with a row stride of V + pad floats (NaN between the rows: never read)"""
    n, V = x.shape
    buf = torch.full((n, V + pad), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :V] = torch.from_numpy(x).to("cuda:0")
    return buf[:, :V]


def _spoken(rng, n, V, gr, blank=0, longest=3, lead=(1.0, 3.0), stray=0.15):
    """label runs of 1..longest frames that WALK the grammar (a blank run now and then, a stray label outside it with
    probability ``stray``) with a lead over unit noise: the menu's phrases are spoken, merges, repeats and stays occur"""
    x = rng.standard_normal((n, V)).astype(np.float32)
    t, g = 0, gr.start_state
    while t < n:
        arcs = gr.arcs(g)
        u = rng.random()
        if u < 0.3 or (not arcs and u < 0.8):
            lab = blank
        elif u < 0.3 + stray or not arcs:
            lab = int(rng.integers(V))
        else:
            lab, g = arcs[int(rng.integers(len(arcs)))]
        for _ in range(int(rng.integers(1, longest + 1))):
            if t < n:
                x[t, lab] = x[t].max() + np.float32(rng.uniform(*lead))
                t += 1
    return x


class Trace:
    """the contract's run over a whole table, the state and the store's length after every frame"""

    def __init__(self, x, blank, B, C, blob, cap=None):
        self.x, self.blank, self.B, self.C, self.blob = x, blank, B, C, blob
        self.gr = grammar.Grammar(blob)
        self.cap = 1 + B * len(x) if cap is None else cap
        self.rows = G.rows(x)
        self.gaps, self.store = [], []
        state = G.scan(G.initial(self.gr), [], self.store, self.cap, B, C, self.gr, blank)
        self.snaps = [(state, len(self.store))]
        for row in self.rows:
            state = G.scan(state, [row], self.store, self.cap, B, C, self.gr, blank, self.gaps)
            self.snaps.append((state, len(self.store)))

    def condition(self, name):
        near = [g for g in self.gaps if g != 0.0 and not g >= MIN_GAP]
        assert not near, (name, min(near))
        return min([g for g in self.gaps if g != 0.0], default=np.inf)

    def at(self, t):
        state, k = self.snaps[t]
        return state, self.store[:k]

    def carried(self, t):
        """the state after t frames as the dict the backend takes"""
        state, store = self.at(t)
        return {"n_frames": state[0], "n_bad": state[1], "n_nodes": state[2], "entries": list(state[3]),
                "nodes": list(store), "g": list(state[4])}


WORST = {"ratio": 0.0, "abs": 0.0}


def _same(name, got, after, want, wstore, cap):
    """every int32 of state, g and store equal, pb / pnb within the bar, the second copies the same bytes, nothing
    written behind min(n_nodes, capacity)"""
    n, nbad, nn, ent, gs = want
    assert (got["n_frames"], got["n_bad"], got["n_nodes"]) == (n, nbad, nn), (name, got["n_frames"], got["n_bad"],
                                                                             got["n_nodes"], want[:3])
    assert [e[:4] for e in got["entries"]] == [e[:4] for e in ent], (name, [e[:4] for e in got["entries"]],
                                                                     [e[:4] for e in ent])
    assert got["g"] == list(gs), (name, got["g"], gs)
    for g, w in zip(got["entries"], ent):
        for a, b in zip(g[4:], w[4:]):
            if b == NEG or a == NEG:
                assert a == b, (name, g, w)
            else:
                err = abs(a - b)
                assert err <= BAR(n, b), (name, a, b, err, BAR(n, b))
                WORST["ratio"] = max(WORST["ratio"], err / BAR(n, b))
                WORST["abs"] = max(WORST["abs"], err)
    raw = got["raw_state"]
    assert int(raw["i"][3]) == len(ent), name
    for r in range(len(ent), 16):                                    # the unused slots
        assert tuple(raw["e"][r]["i"]) == R.EMPTY_ENTRY[:4] and tuple(raw["e"][r]["p"]) == (NEG, NEG), (name, r)
        assert int(got["raw_gr"]["g"][r]) == 0, (name, r)
    assert after[0].tobytes() == raw.tobytes() and after[1].tobytes() == got["raw_gr"].tobytes(), name
    k = min(nn, cap)
    assert len(wstore) == k and got["nodes"] == list(wstore), (name, got["nodes"][:5], list(wstore)[:5])
    assert (got["raw_nodes"][:k, 3] == 0).all(), name                # reserved = 0
    assert (got["raw_nodes"][k:] == -7).all(), name                  # nothing behind the stored nodes


def _ints(rec):
    return np.frombuffer(rec.tobytes(), np.int32)


def _bits(got):
    return got["raw_state"].tobytes(), got["raw_gr"].tobytes(), got["raw_nodes"].tobytes()


def _run(be, tr, name, spans, chain=CUTS):
    """every span (t0, t1) as a job that carries the contract's state and store over the rows [0, t0) in - ONE launch -
    against the contract; then the spans of ``chain`` fed one after another: bit for bit the one-span run"""
    tab = _strided(tr.x)
    dg = _device_grammar(tr.blob)
    jobs = [(tab, tr.blank, t0, t1, None if t0 == 0 else tr.carried(t0), tr.cap, tr.B, tr.C) for t0, t1 in spans]
    got, after = be.ctc_beam_grammar(jobs, dg)
    for (t0, t1), g, a in zip(spans, got, after):
        st, store = tr.at(t1)
        _same(f"{name} span ({t0}, {t1})", g, a, st, store, tr.cap)
    if chain:
        assert spans[0] == (0, chain[-1])
        state = None
        for a, b in zip(chain[:-1], chain[1:]):
            (state,), (aft,) = be.ctc_beam_grammar([(tab, tr.blank, a, b, state, tr.cap, tr.B, tr.C)], dg)
            st, store = tr.at(b)
            _same(f"{name} chain [{a}, {b})", state, aft, st, store, tr.cap)
        assert _bits(state) == _bits(got[0]), name
    return got


def _menu(rng, V, blank, count=40):
    """``count`` distinct phrases of 1 to 6 tokens (as many as V allows), one of them a prefix of another"""
    toks = [t for t in range(V) if t != blank]
    seen = set()
    for k in range(1, 7):                                            # V = 2: the runs of its one token
        if len(toks) == 1:
            seen.add(tuple(toks * k))
    tries = 0
    while len(seen) < count and len(toks) > 1 and tries < 10000:
        tries += 1
        seen.add(tuple(int(rng.choice(toks)) for _ in range(int(rng.integers(1, 7)))))
    out = sorted(seen)
    long = max(out, key=len)
    if len(long) > 1:
        out.append(long[:-1])                                        # (a duplicate is dropped by the compiler)
    return [list(p) for p in out]


# seeds per (V, B, C) at which the condition holds (picked on the CPU)
SEEDS = {}


@functools.lru_cache(maxsize=None)
def _trace(V, B, C):
    rng = np.random.default_rng(SEEDS.get((V, B, C), 1000 * V + 16 * B + C))
    blob = grammar.compile(_menu(rng, V, 0), V, 0, loop=True)
    return Trace(_spoken(rng, T, V, grammar.Grammar(blob)), 0, B, C, blob)


# ---- the kernel against the contract ----------------------------------------------------------------------------------
@pytest.mark.parametrize("BC", [(1, 1), (2, 3), (8, 8), (16, 16)], ids=lambda bc: f"B{bc[0]}C{bc[1]}")
@pytest.mark.parametrize("V", [2, 17, 65, 1024, 1500])
def test_kernel_equals_the_contract_on_a_looped_menu_at_every_width_beam_and_cut(be, V, BC):
    B, C = BC
    tr = _trace(V, B, C)
    name = f"V={V} B={B} C={C}"
    gap = tr.condition(name)
    final = tr.at(T)[0]
    assert final[0] == T and final[2] > 20
    _run(be, tr, name, [(0, T), (0, 17), (17, 256), (256, T), (40, T), (TILE - 1, TILE + 1), (7, 7), (T, T)])
    print(f"\n{name}: {tr.gr.n_states} states, start state {len(tr.gr.arcs(0))} arcs; smallest non-zero gap {gap:.2e}; "
          f"largest |pb, pnb - contract| so far {WORST['abs']:.3e} = {WORST['ratio']:.4f} of the bar")


def test_one_linear_phrase_and_a_state_without_arcs(be):
    rng = np.random.default_rng(21)
    V = 40
    for loop, seed in ((False, 0), (True, 1)):
        blob = grammar.compile([[5, 9, 9, 31]], V, 0, loop=loop)
        gr = grammar.Grammar(blob)
        x = _spoken(rng, 80, V, gr)
        tr = Trace(x, 0, 8, 8, blob)
        name = f"linear loop={loop}"
        tr.condition(name)
        got = _run(be, tr, name, [(0, 80), (0, 17), (17, 80)], chain=[0, 17, 64, 80])
        if not loop:                                                 # the phrase was spoken: its end state only stays
            ends = [g for g in got[0]["g"] if gr.accepts(g)]
            assert ends and gr.arcs(ends[0]) == []
        assert len(got[0]["entries"]) <= 5 if not loop else True     # at most the phrase's five prefixes


@pytest.mark.parametrize("V,deg", [(67, 63), (67, 64), (67, 65), (67, 66), (1024, 63), (1024, 64), (1024, 65), (1024, 1023),
                                   (1500, 1499)])
def test_wide_states_at_the_lane_stride_edges(be, V, deg):
    """every state has ``deg`` out-arcs: the single-token phrases of the first ``deg`` tokens, looped"""
    rng = np.random.default_rng(31 * V + deg)
    blob = grammar.compile([[t] for t in range(1, deg + 1)], V, 0, loop=True)
    gr = grammar.Grammar(blob)
    assert [len(gr.arcs(g)) for g in range(gr.n_states)] == [deg] * gr.n_states
    x = _spoken(rng, 40, V, gr, stray=0.4)
    x[:, deg] = x[:, 1]                                              # the last arc ties the first
    if deg + 1 < V:
        x[:, deg + 1] = x.max(1) + np.float32(5.0)                   # the loudest token lies just outside the grammar
    tr = Trace(x, 0, 8, 8, blob)
    tr.condition(f"deg {deg}")
    got = _run(be, tr, f"V={V} deg={deg}", [(0, 40), (0, 17), (17, 40)], chain=[0, 17, 40])
    assert all(1 <= e[1] <= deg for e in got[0]["entries"] if e[1] >= 0)


def test_ties_among_arc_tokens_minus_inf_arcs_minus_inf_blanks_and_bad_rows(be):
    rng = np.random.default_rng(41)
    V, blank = 130, 0
    blob = grammar.compile(_menu(rng, V, blank), V, blank)
    gr = grammar.Grammar(blob)
    y = _spoken(rng, 90, V // 2, grammar.Grammar(grammar.compile(_menu(rng, V // 2, blank, 20), V // 2, blank)))
    x = np.concatenate([y, y], 1)                                    # every value of a row occurs twice: ties everywhere
    for B, C in ((8, 5), (16, 16), (3, 1)):
        tr = Trace(x, blank, B, C, blob)
        tr.condition(f"twins B={B} C={C}")
        _run(be, tr, f"twins B={B} C={C}", [(0, 90), (0, 17), (17, 90)], chain=[0, 17, 64, 90])
    z = _spoken(rng, 90, V, gr)
    z[5:30, blank] = NEG                                             # the stays live on their pnb alone
    start = [t for t, _ in gr.arcs(gr.start_state)]
    z[31, start] = NEG                                               # every arc token of the start state at -inf
    z[32, 1:] = NEG                                                  # ... of every state: the blank alone
    z[33, :] = NEG
    z[33, start[0]] = 0.0                                            # one finite entry, an arc of the start state
    z[40, 40] = np.nan                                               # bad rows: NaN, +inf, all -inf
    z[41, 41] = np.inf
    z[42, :] = NEG
    z[60, blank] = np.nan
    z[70, :] = -1e30
    z[70, start[0]] = z[70, start[-1]] = 1e30                        # logits of 1e30, tied
    tr = Trace(z, blank, 8, 8, blob)
    tr.condition("inf")
    got = _run(be, tr, "inf", [(0, 90), (5, 30), (30, 45), (39, 43), (60, 61)], chain=[0, 33, 41, 42, 64, 90])
    assert got[0]["n_bad"] == 4


def test_a_small_node_store_counts_and_writes_nothing_behind_it(be):
    rng = np.random.default_rng(51)
    V = 40
    blob = grammar.compile(_menu(rng, V, 0), V, 0)
    x = _spoken(rng, 30, V, grammar.Grammar(blob))
    for cap in (0, 1, 7, 20):
        tr = Trace(x, 0, 4, 4, blob, cap=cap)
        tr.condition(f"capacity {cap}")
        got = _run(be, tr, f"capacity {cap}", [(0, 30), (0, 3), (3, 30)], chain=[0, 3, 30])
        assert got[0]["n_nodes"] > 20 and len(got[0]["nodes"]) == cap and (got[0]["raw_nodes"][cap:] == -7).all()


def test_restart_ignores_the_stored_state(be):
    rng = np.random.default_rng(52)
    V = 64
    blob = grammar.compile(_menu(rng, V, 0), V, 0)
    x = _spoken(rng, 40, V, grammar.Grammar(blob))
    tr = Trace(x, 0, 8, 8, blob)
    fresh = Trace(x[20:], 0, 8, 8, blob, cap=tr.cap)
    fresh.condition("restart")

    def restart(k, j):
        j.beam.restart = 1

    broken = dict(tr.carried(20), g=[-5] * 8)                        # (not looked at with restart)
    got, after = be.ctc_beam_grammar([(_strided(x), 0, 20, 40, broken, tr.cap, 8, 8)], _device_grammar(blob), tweak=restart)
    st, store = fresh.at(20)
    g = got[0]
    assert [e[:4] for e in g["entries"]] == [e[:4] for e in st[3]] and g["g"] == st[4] and g["n_frames"] == 20
    assert g["nodes"][:len(store)] == store


# ---- identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,B", [(2, 4), (5, 16), (17, 16), (17, 5)])
def test_the_free_grammar_gives_the_bytes_of_sc_ctc_beam(be, V, B):
    rng = np.random.default_rng(60 + V + B)
    for blank in (0, V - 1):
        free = grammar.free(V, blank)
        x = _spoken(rng, T, V, grammar.Grammar(free))
        x[7, blank] = NEG
        x[9, (blank + 1) % V] = NEG
        x[11, :] = NEG
        x[13, 0] = np.nan
        x[270, V - 1] = np.inf
        tab = _strided(x)
        plain = R.scan_table(x[:100], blank, B, 16, capacity=1 + B * T)
        carried = {"n_frames": plain[0][0], "n_bad": plain[0][1], "n_nodes": plain[0][2], "entries": list(plain[0][3]),
                   "nodes": list(plain[1]), "g": [0] * len(plain[0][3])}
        jobs = [(tab, blank, 0, T, None, 1 + B * T, B, 16), (tab, blank, 100, T, carried, 1 + B * T, B, 16),
                (tab, blank, 0, 40, None, 9, B, 16)]
        want, wafter = be.ctc_beam(jobs)
        got, after = be.ctc_beam_grammar(jobs, _device_grammar(free))
        for k, (w, wa, g, a) in enumerate(zip(want, wafter, got, after)):
            assert g["raw_state"].tobytes() == w["raw_state"].tobytes(), (V, B, blank, k)
            assert a[0].tobytes() == wa.tobytes() and g["raw_nodes"].tobytes() == w["raw_nodes"].tobytes(), (V, B, blank, k)
            assert (g["raw_gr"]["g"] == 0).all() and (a[1]["g"] == 0).all() and g["n_bad"] == (3 if k < 2 else 2)
            assert g["n_nodes"] > 1


def test_a_malformed_job_writes_nothing_while_its_neighbours_are_served(be):
    rng = np.random.default_rng(71)
    V = 65
    blob = grammar.compile(_menu(rng, V, 0), V, 0)
    gr = grammar.Grammar(blob)
    x = _spoken(rng, 50, V, gr)
    tab = _strided(x)
    tr = Trace(x, 0, 4, 4, blob)
    tr.condition("neighbours")
    dg = _device_grammar(blob)
    other_v = _device_grammar(grammar.compile([[1, 2]], V + 1, 0))
    other_blank = _device_grammar(grammar.compile([[1, 2]], V, 3))

    def setter(**kw):
        def tweak(k, j):
            if k == 1:
                for f, v in kw.items():
                    setattr(j if f in ("grammar", "gr_state", "gr_state_after") else j.beam, f, v)
        return tweak

    bad = [dict(grammar=None), dict(gr_state=None), dict(grammar=other_v.view), dict(grammar=other_blank.view),
           dict(table=None), dict(state=None), dict(nodes=None), dict(V=0), dict(blank=-1), dict(blank=V), dict(t0=-1),
           dict(t0=30, t1=29), dict(stride=V - 1), dict(capacity=-1), dict(B=0), dict(B=17), dict(C=0), dict(C=17), None]
    for i, kw in enumerate(bad):
        got, after = be.ctc_beam_grammar([(tab, 0, 0, 50, None, tr.cap, 4, 4)] * 3, dg, tweak=setter(**kw) if kw else None)
        if kw is not None:
            assert (_ints(got[1]["raw_state"]) == -7).all() and (got[1]["raw_nodes"] == -7).all(), kw
            assert (_ints(got[1]["raw_gr"]) == -7).all(), kw
            if "state" not in kw:
                assert (_ints(after[1][0]) == -7).all(), kw
            if "gr_state" not in kw:
                assert (_ints(after[1][1]) == -7).all(), kw
        for k in (0, 2) if kw is not None else (0, 1, 2):            # its neighbours in the same launch are served
            _same(f"neighbour {i}.{k}", got[k], after[k], *tr.at(50), tr.cap)
    # a stored entry count outside [0, 16], a stored g outside [0, n_states): nothing is written
    c20 = tr.carried(20)
    for broken in (dict(c20, n_entries=17), dict(c20, n_entries=-1), dict(c20, g=[gr.n_states] + c20["g"][1:]),
                   dict(c20, g=c20["g"][:-1] + [-1])):
        got, after = be.ctc_beam_grammar([(tab, 0, 20, 50, tr.carried(20), tr.cap, 4, 4), (tab, 0, 20, 50, broken, tr.cap, 4, 4)],
                                         dg)
        _same("carried", got[0], after[0], *tr.at(50), tr.cap)
        assert got[1]["n_frames"] == 20 and int(got[1]["raw_state"]["i"][3]) == broken.get("n_entries", len(c20["entries"]))
        assert list(got[1]["raw_gr"]["g"][:len(broken["g"])]) == broken["g"]
        assert got[1]["nodes"] == c20["nodes"] and (_ints(after[1][0]) == -7).all() and (_ints(after[1][1]) == -7).all()
    # a g out of range BEHIND the beam's B entries is not looked at: the state is cut to B first
    wide = Trace(x, 0, 8, 4, blob)
    wide.condition("wide")
    c = wide.carried(20)
    assert len(c["g"]) > 4
    cut = dict(c, g=c["g"][:4] + [gr.n_states + 7] * (len(c["g"]) - 4))
    store = list(wide.at(20)[1])
    gaps = []
    want = G.scan(wide.at(20)[0], wide.rows[20:50], store, wide.cap, 4, 4, gr, 0, gaps)
    assert not [g for g in gaps if g != 0.0 and not g >= MIN_GAP]
    got, after = be.ctc_beam_grammar([(tab, 0, 20, 50, cut, wide.cap, 4, 4)], dg)
    _same("cut", got[0], after[0], want, store, wide.cap)
    from speechcatcher_amd import _abi
    lib = _abi.load()
    assert lib.sc_ctc_beam_grammar(None, 0, None) == 0
    assert lib.sc_ctc_beam_grammar(None, 2, None) == -1 and lib.sc_ctc_beam_grammar(None, -1, None) == -1
    assert lib.sc_ctc_beam_grammar(tab.data_ptr(), _abi.BEAM_MAX_JOBS + 1, None) == -1


def test_two_grammars_in_one_launch_and_the_handles_host_copy(be):
    rng = np.random.default_rng(81)
    V = 50
    blobs = [grammar.compile(_menu(rng, V, 0, 12), V, 0), grammar.compile([[3, 4], [3]], V, 0, loop=False)]
    x = _spoken(rng, 60, V, grammar.Grammar(blobs[0]))
    traces = [Trace(x, 0, 8, 8, b) for b in blobs]
    for tr in traces:
        tr.condition("two")
    tab = _strided(x)
    got, after = be.ctc_beam_grammar([(tab, 0, 0, 60, None, tr.cap, 8, 8) for tr in traces],
                                     [_device_grammar(b) for b in blobs])
    for tr, g, a in zip(traces, got, after):
        _same("two", g, a, *tr.at(60), tr.cap)
    # the handle's host copy walks as speechcatcher_amd.grammar.Grammar does; destroy looks at the use count
    from speechcatcher_amd import _abi
    lib = _abi.load()
    dg, gr = be.grammar(blobs[0]), traces[0].gr
    for s in range(gr.n_states):
        assert dg.accepts(s) == gr.accepts(s)
        for t in range(V):
            assert dg.step(s, t) == gr.step(s, t)
    assert dg.step(-1, 1) == dg.step(gr.n_states, 1) == dg.step(0, V) == -1 and lib.sc_grammar_accepts(dg.handle, -1) == -1
    assert (dg.info.V, dg.info.blank, dg.info.n_states, dg.info.n_arcs, dg.info.start_state) == \
        (V, 0, gr.n_states, gr.n_arcs, gr.start_state)
    assert lib.sc_grammar_use(dg.handle, 1) == 1 and lib.sc_grammar_use(dg.handle, 1) == 2
    assert lib.sc_grammar_destroy(dg.handle) == -1 and b"in use" in lib.sc_last_error()
    assert lib.sc_grammar_use(dg.handle, -2) == 0 and lib.sc_grammar_use(dg.handle, -1) == -1
    dg.close()
    assert dg.handle is None
