"""CTC prefix beam search on the GPU (csrc/ctc_beam.hip: sc_ctc_beam, sc_ctc_beam_pack) against the float64 contract
of tests/ctc_beam_ref.py on constructed tables: every int32 equal - entry order, node, last, len, parent, the counters,
every stored node record, the sentinels behind the store -, pb / pnb within 64 n_frames 2^-53 max(1, |want|) and -inf
exactly; chained spans bit for bit the one-span run.

The integers can only be equal where no prune decision is a near-tie: every test first asserts, on the CPU from the
contract alone, that every gap between consecutive kept totals and between the B-th and the (B+1)-th is exactly 0 or
at least MIN_GAP = 1e-6 (more than 10^3 times the bar at 300 frames); no case is skipped for it - the seeds are picked
so that it holds.

Measured on an MI355X (printed by the tests): largest |pb, pnb - contract| 3.4e-13 at 300 frames and
values near -600 = 0.14 of the bar; smallest non-zero prune gap of the parametrised cases 7.5e-6."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_ref as R

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-6
TILE = 256   # BM_TILE of csrc/ctc_beam.hip
NEG = -np.inf
# a frame puts a value through at most eight rounded float64 operations, each within a few ulp on either side, and the
# errors add linearly in the log domain
BAR = lambda n_frames, want: 64.0 * max(n_frames, 1) * 2.0 ** -53 * max(1.0, abs(want))   # noqa: E731


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


def _structured(rng, T, V, longest=4, lead=(1.0, 3.0)):
    """label runs of 1..longest frames (the blank among the labels) with a lead of lead[0]..lead[1] over unit noise:
    merges, repeats across a blank and stays all occur"""
    x = rng.standard_normal((T, V)).astype(np.float32)
    t = 0
    while t < T:
        lab = int(rng.integers(V))
        for _ in range(int(rng.integers(1, longest + 1))):
            if t < T:
                x[t, lab] = x[t].max() + np.float32(rng.uniform(*lead))
                t += 1
    return x


class Trace:
    """the contract's run over a whole table, the state and the store's length after every frame"""

    def __init__(self, x, blank, B, C, cap=None):
        self.x, self.blank, self.B, self.C = x, blank, B, C
        self.cap = 1 + B * len(x) if cap is None else cap
        self.rows = R.rows(x, blank, C)
        self.gaps, self.store = [], []
        state = R.scan(R.initial(), [], self.store, self.cap, B)
        self.snaps = [(state, len(self.store))]
        for row in self.rows:
            state = R.scan(state, [row], self.store, self.cap, B, self.gaps)
            self.snaps.append((state, len(self.store)))

    def condition(self, name):
        near = [g for g in self.gaps if g != 0.0 and not g >= MIN_GAP]
        assert not near, (name, min(near))
        return min([g for g in self.gaps if g != 0.0], default=np.inf)

    def at(self, t):
        """(state, store) after t frames"""
        state, k = self.snaps[t]
        return state, self.store[:k]

    def carried(self, t):
        """the state after t frames as the dict the backend takes"""
        state, store = self.at(t)
        return {"n_frames": state[0], "n_bad": state[1], "n_nodes": state[2], "entries": list(state[3]),
                "nodes": list(store)}


WORST = {"ratio": 0.0, "abs": 0.0}


def _same(name, got, after, want, wstore, cap, sentinels=True):
    """every int32 of state and store equal, pb / pnb within the bar, the second copy the same bytes, nothing written
    behind min(n_nodes, capacity)"""
    n, nbad, nn, ent = want
    assert (got["n_frames"], got["n_bad"], got["n_nodes"]) == (n, nbad, nn), (name, got["n_frames"], got["n_bad"],
                                                                             got["n_nodes"], want[:3])
    assert [e[:4] for e in got["entries"]] == [e[:4] for e in ent], (name, [e[:4] for e in got["entries"]],
                                                                     [e[:4] for e in ent])
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
    for r in range(len(ent), 16):                                    # the unused slots: (-1, -1, 0, -1, -inf, -inf)
        assert tuple(raw["e"][r]["i"]) == R.EMPTY_ENTRY[:4] and tuple(raw["e"][r]["p"]) == (NEG, NEG), (name, r)
    assert after.tobytes() == raw.tobytes(), name
    k = min(nn, cap)
    assert len(wstore) == k and got["nodes"] == list(wstore), (name, got["nodes"][:5], list(wstore)[:5])
    assert (got["raw_nodes"][:k, 3] == 0).all(), name                # reserved = 0
    if sentinels:
        assert (got["raw_nodes"][k:] == -7).all(), name              # nothing behind the stored nodes


def _ints(rec):
    """a state record as its 132 int32 words"""
    return np.frombuffer(rec.tobytes(), np.int32)


def _bits(got):
    return got["raw_state"].tobytes(), got["raw_nodes"].tobytes()


CUTS = [0, 1, 15, 16, 17, 255, 256, 257, 300]


def _run(be, tr, name, spans, tab=None, chain=CUTS):
    """every span (t0, t1) as a job that carries the contract's state and store over the rows [0, t0) in - ONE launch -
    against the contract; then the spans of ``chain`` fed one after another: bit for bit the one-span run"""
    tab = _strided(tr.x) if tab is None else tab
    jobs = [(tab, tr.blank, t0, t1, None if t0 == 0 else tr.carried(t0), tr.cap, tr.B, tr.C) for t0, t1 in spans]
    got, after = be.ctc_beam(jobs)
    for (t0, t1), g, a in zip(spans, got, after):
        st, store = tr.at(t1)
        _same(f"{name} span ({t0}, {t1})", g, a, st, store, tr.cap)
    if chain:
        T = chain[-1]
        assert spans[0] == (0, T)
        state = None
        for a, b in zip(chain[:-1], chain[1:]):
            (state,), (aft,) = be.ctc_beam([(tab, tr.blank, a, b, state, tr.cap, tr.B, tr.C)])
            st, store = tr.at(b)
            _same(f"{name} chain [{a}, {b})", state, aft, st, store, tr.cap)
        assert _bits(state) == _bits(got[0]), name
    return got


# seeds per (V, B, C) at which the condition holds (structured tables; T = 300)
SEEDS = {(65, 16, 16): 1}


@functools.lru_cache(maxsize=None)
def _trace(V, B, C, T=300):
    rng = np.random.default_rng(SEEDS.get((V, B, C), 1000 * V + 16 * B + C))
    return Trace(_structured(rng, T, V), 0, B, C)


# ---- the kernel against the contract ----------------------------------------------------------------------------------
@pytest.mark.parametrize("BC", [(1, 1), (2, 3), (8, 8), (16, 16)], ids=lambda bc: f"B{bc[0]}C{bc[1]}")
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1024, 1500])
def test_kernel_equals_the_contract_at_every_width_beam_and_cut(be, V, BC):
    B, C = BC
    tr = _trace(V, B, C)
    name = f"V={V} B={B} C={C}"
    gap = tr.condition(name)
    final = tr.at(300)[0]
    assert final[0] == 300 and (V == 1 or final[2] > 20) and len(final[3]) == (B if V > 2 else min(B, len(final[3])))
    spans = [(0, 300)] + list(zip(CUTS[1:-1], CUTS[2:])) + [(40, 300), (TILE - 1, TILE + 1), (63, 65), (7, 7), (300, 300)]
    _run(be, tr, name, spans)
    print(f"\n{name}: smallest non-zero gap {gap:.2e}; largest |pb, pnb - contract| so far {WORST['abs']:.3e} = "
          f"{WORST['ratio']:.4f} of the bar")


def test_more_candidates_than_tokens_and_another_blank(be):
    rng = np.random.default_rng(11)
    for V, B, C, blank in ((5, 16, 16, 0), (5, 4, 16, 4), (9, 8, 8, 3), (2, 16, 16, 1), (130, 8, 5, 129), (1100, 4, 6, 1050)):
        tr = Trace(_structured(rng, 70, V), blank, B, C)
        name = f"V={V} B={B} C={C} blank={blank}"
        tr.condition(name)
        _run(be, tr, name, [(0, 70), (0, 1), (1, 64), (64, 70)], chain=[0, 1, 64, 70])


def test_exact_ties_through_duplicated_columns_and_at_the_last_candidate(be):
    """columns [20, 40) repeat columns [0, 20): every value of a row occurs twice - the blank ties token 20 (a stay
    against a new prefix), an odd C cuts a pair (the lower index is taken), and the twin prefixes tie all along (the lower
    token first, then the lower parent rank).  The gaps are exactly 0 or clear."""
    rng = np.random.default_rng(12)
    y = _structured(rng, 80, 20)
    x = np.concatenate([y, y], 1)
    for B, C in ((8, 5), (16, 16), (3, 3), (7, 1)):
        tr = Trace(x, 0, B, C)
        name = f"twins B={B} C={C}"
        tr.condition(name)
        assert sum(g == 0.0 for g in tr.gaps) >= 40
        _run(be, tr, name, [(0, 80), (0, 17), (17, 80)], chain=[0, 17, 64, 65, 80])
    # one column twice among distinct ones, the pair on either side of a lane boundary of the row pass
    z = _structured(rng, 80, 200)
    z[:, 131] = z[:, 3]
    z[:, 67] = z[:, 3]
    tr = Trace(z, 0, 8, 8)
    tr.condition("triplet")
    _run(be, tr, "triplet", [(0, 80)], chain=[0, 33, 80])


def test_minus_inf_blank_bad_rows_inside_a_run_and_all_blank_tables(be):
    rng = np.random.default_rng(13)
    V, blank = 130, 0
    x = _structured(rng, 90, V)
    x[5:30, blank] = NEG                                             # the stays live on their pnb alone
    x[31, 10:90] = NEG                                               # -inf entries beside finite ones
    x[33, :] = NEG
    x[33, 7] = 0.0                                                   # one finite entry, not the blank: lp = 0
    x[35, :] = NEG
    x[35, blank] = 2.0                                               # the blank alone: no candidate
    x[40, 40] = np.nan                                               # bad rows: NaN, +inf, all -inf
    x[41, 41] = np.inf
    x[42, :] = NEG
    x[60, blank] = np.nan
    x[70, :] = -1e30
    x[70, 9] = x[70, 77] = 1e30                                      # logits of 1e30, tied
    tr = Trace(x, blank, 8, 8)
    tr.condition("inf")
    got = _run(be, tr, "inf", [(0, 90), (5, 30), (30, 45), (39, 43), (60, 61)], chain=[0, 33, 41, 42, 64, 90])
    assert got[0]["n_bad"] == 4
    for B, C, seed in ((4, 4, 104), (16, 16, 108)):                  # (seeds at which the condition holds)
        y = _structured(np.random.default_rng(seed), 280, 67)
        y[:, 3] = y.max(1) + np.float32(6.0)                         # all blank: the empty prefix stays ahead
        tr = Trace(y, 3, B, C)
        tr.condition("all blank")
        got = _run(be, tr, "all blank", [(0, 280), (10, 270)], chain=[0, 256, 280])
        assert got[0]["entries"][0][:4] == (0, -1, 0, -1)
    tr = Trace(np.zeros((70, 1), np.float32), 0, 8, 8)               # V = 1: nothing but the blank
    got = _run(be, tr, "V=1", [(0, 70)], chain=[0, 64, 70])
    assert got[0]["entries"] == [(0, -1, 0, -1, 0.0, NEG)] and got[0]["n_nodes"] == 1


def test_restart_an_empty_span_and_a_state_wider_than_the_beam(be):
    rng = np.random.default_rng(14)
    V = 64
    x = _structured(rng, 40, V)
    tr = Trace(x, 0, 8, 8)
    tr.condition("restart")
    tab = _strided(x)
    fresh = Trace(x[20:], 0, 8, 8, cap=tr.cap)
    fresh.condition("restart, rows 20..40 from a fresh state")

    def restart(k, j):
        j.restart = 1

    got, after = be.ctc_beam([(tab, 0, 20, 40, tr.carried(20), tr.cap, 8, 8)], tweak=restart)
    _same("restart", got[0], after[0], *fresh.at(20), tr.cap, sentinels=False)
    # an empty span rewrites the state unchanged (with restart: the initial state and node 0)
    got, after = be.ctc_beam([(tab, 0, 9, 9, tr.carried(30), tr.cap, 8, 8), (tab, 0, 9, 9, None, tr.cap, 8, 8)])
    _same("empty", got[0], after[0], *tr.at(30), tr.cap)
    _same("empty restart", got[1], after[1], R.initial(), [R.ROOT], tr.cap)
    # a state of 8 entries handed to a beam of 3: cut to its first 3, then searched on
    small_store = list(tr.at(30)[1])
    gaps = []
    want = R.scan(tr.at(30)[0], tr.rows[30:40], small_store, tr.cap, 3, gaps)
    near = [g for g in gaps if g != 0.0 and not g >= MIN_GAP]        # the condition of the cut beam's own run
    assert not near and len(gaps) >= 20, (min(near), len(gaps))
    got, after = be.ctc_beam([(tab, 0, 30, 40, tr.carried(30), tr.cap, 3, 8), (tab, 0, 30, 30, tr.carried(30), tr.cap, 3, 8)])
    _same("cut", got[0], after[0], want, small_store, tr.cap)
    st30, store30 = tr.at(30)
    _same("cut empty", got[1], after[1], st30[:3] + (st30[3][:3],), store30, tr.cap)


def test_a_small_node_store_counts_and_writes_nothing_behind_it(be):
    rng = np.random.default_rng(15)
    x = _structured(rng, 30, 40)
    for cap in (0, 1, 7, 20):
        tr = Trace(x, 0, 4, 4, cap=cap)
        tr.condition(f"capacity {cap}")
        got = _run(be, tr, f"capacity {cap}", [(0, 30), (0, 3), (3, 30)], chain=[0, 3, 30])
        assert got[0]["n_nodes"] > 40 and len(got[0]["nodes"]) == cap and (got[0]["raw_nodes"][cap:] == -7).all()


def test_nan_rows_outside_the_span_are_not_read(be):
    rng = np.random.default_rng(16)
    x = _structured(rng, 120, 65)
    poisoned = np.full_like(x, np.nan)
    poisoned[20:90] = x[20:90]
    tr = Trace(x[20:90], 0, 8, 8)
    tr.condition("poison")
    got, after = be.ctc_beam([(_strided(poisoned), 0, 20, 90, None, tr.cap, 8, 8)])
    _same("poison", got[0], after[0], *tr.at(70), tr.cap)
    assert got[0]["n_bad"] == 0


def test_a_malformed_job_writes_nothing_while_its_neighbours_are_served(be):
    rng = np.random.default_rng(17)
    V = 65
    x = _structured(rng, 50, V)
    tab = _strided(x)
    tr = Trace(x, 0, 4, 4)
    tr.condition("neighbours")

    def setter(**kw):
        def tweak(k, j):
            if k == 1:
                for f, v in kw.items():
                    setattr(j, f, v)
        return tweak

    bad = [dict(table=None), dict(state=None), dict(nodes=None), dict(V=0), dict(blank=-1), dict(blank=V), dict(t0=-1),
           dict(t0=30, t1=29), dict(stride=V - 1), dict(capacity=-1), dict(B=0), dict(B=17), dict(C=0), dict(C=17), None]
    for i, kw in enumerate(bad):
        got, after = be.ctc_beam([(tab, 0, 0, 50, None, tr.cap, 4, 4)] * 3, tweak=setter(**kw) if kw else None)
        if kw is not None:
            assert (_ints(got[1]["raw_state"]) == -7).all() and (got[1]["raw_nodes"] == -7).all(), kw
            if "state" not in kw:                                    # (the second copy of a job without a state: untouched too)
                assert (_ints(after[1]) == -7).all(), kw
        for k in (0, 2) if kw is not None else (0, 1, 2):            # its neighbours in the same launch are served
            _same(f"neighbour {i}.{k}", got[k], after[k], *tr.at(50), tr.cap)
    # a stored entry count outside [0, 16]: nothing is written
    for count in (17, -1):
        broken = dict(tr.carried(20), n_entries=count)
        got, after = be.ctc_beam([(tab, 0, 20, 50, tr.carried(20), tr.cap, 4, 4), (tab, 0, 20, 50, broken, tr.cap, 4, 4)])
        _same("carried", got[0], after[0], *tr.at(50), tr.cap)
        assert (got[1]["n_frames"], int(got[1]["raw_state"]["i"][3])) == (20, count)
        assert got[1]["nodes"] == tr.carried(20)["nodes"] and (_ints(after[1]) == -7).all()
    from speechcatcher_amd import _abi
    lib = _abi.load()
    assert lib.sc_ctc_beam(None, 0, None) == 0
    assert lib.sc_ctc_beam(None, 2, None) == -1 and lib.sc_ctc_beam(None, -1, None) == -1
    assert lib.sc_ctc_beam(tab.data_ptr(), _abi.BEAM_MAX_JOBS + 1, None) == -1


def test_the_pack_launch_equals_the_contracts_backtrace(be):
    from speechcatcher_amd import _abi
    tr = _trace(65, 8, 8)
    jobs, want = [], []
    for t in (0, 1, 40, 300):
        st = tr.carried(t)
        for rank in range(9):
            jobs.append((st, rank, 200, None))
            want.append((st, rank))
    got = be.ctc_beam_pack(jobs)
    longest = 0
    for g, (st, rank) in zip(got, want):
        head, sc, ids, frames = g["raw"]
        assert (head[4:] == -7).all() and (sc[2:] == -7.0).all()
        if rank >= len(st["entries"]):
            assert (g["len"], g["status"], g["node"], g["last"]) == (-1, _abi.BEAM_PACK_NO_ENTRY, -1, -1)
            assert np.isnan(g["pb"]) and np.isnan(g["pnb"]) and (ids == -7).all() and (frames == -7).all()
            continue
        e = st["entries"][rank]
        wids, wframes = R.backtrace(e, st["nodes"])
        assert (g["len"], g["status"], g["node"], g["last"]) == (e[2], _abi.BEAM_PACK_OK, e[0], e[1])
        assert np.float64(g["pb"]).tobytes() == np.float64(e[4]).tobytes() and g["pnb"] == e[5]
        assert g["ids"] == wids and g["frames"] == wframes
        assert (ids[e[2]:] == -7).all() and (frames[e[2]:] == -7).all()
        longest = max(longest, e[2])
    assert longest >= 60
    # max_len smaller than the prefix: its first max_len tokens; a store cut short: broken; malformed: nothing written
    st = tr.carried(300)
    e = st["entries"][0]
    wids, wframes = R.backtrace(e, st["nodes"])

    def tweak(k, j):
        if k == 3:
            j.header = None
        if k == 4:
            j.max_len = -1

    got = be.ctc_beam_pack([(st, 0, 10, None), (st, 0, 0, None), (st, 0, 200, e[0]), (st, 0, 200, None),
                            (st, 0, 200, None), (st, -1, 200, None)], tweak=tweak)
    assert (got[0]["len"], got[0]["status"]) == (e[2], _abi.BEAM_PACK_TRUNCATED)
    assert got[0]["ids"] == wids[:10] and got[0]["frames"] == wframes[:10] and (got[0]["raw"][2][10:] == -7).all()
    assert (got[1]["len"], got[1]["status"]) == (e[2], _abi.BEAM_PACK_TRUNCATED) and (got[1]["raw"][2] == -7).all()
    assert (got[2]["len"], got[2]["status"], got[2]["node"]) == (-1, _abi.BEAM_PACK_BROKEN, e[0])
    for k in (3, 4):
        assert all((a == -7).all() for a in got[k]["raw"]), k
    assert got[5]["status"] == _abi.BEAM_PACK_NO_ENTRY
    lib = _abi.load()
    assert lib.sc_ctc_beam_pack(None, 0, None) == 0 and lib.sc_ctc_beam_pack(None, 2, None) == -1
