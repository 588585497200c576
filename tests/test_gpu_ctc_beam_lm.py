"""CTC prefix beam search with a fused n-gram model on the GPU (csrc/ctc_beam.hip: sc_ctc_beam_lm, sc_lm_create) against
the float64 contract of tests/ctc_beam_lm_ref.py: every int32 of state and store and every ctx equal, lm bit-equal (pure
float64 addition in a fixed order), pb / pnb within the bar of tests/test_gpu_ctc_beam.py (their arithmetic is 8j's);
chained spans bit for bit the one-span run; without a model, or with alpha = beta = 0, every bit of sc_ctc_beam.

The integers can only be equal where no prune decision is a near-tie: every case first asserts, on the CPU from the
contract alone, that every gap between consecutive kept FUSED totals and between the B-th and the (B+1)-th is exactly 0
or at least MIN_GAP = 1e-6; no case is skipped for it - the seeds were picked on the CPU so that it holds."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_ref as L
import ctc_beam_ref as R
import ngram_ref as NR
from speechcatcher_amd import ngram
from test_gpu_ctc_beam import BAR, MIN_GAP, TILE, _bits, _ints, _strided, _structured

pytestmark = pytest.mark.gpu

NEG = -np.inf


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


class Memo:
    """a packed model with its scores remembered, and how deep the lookups backed off"""

    def __init__(self, blob):
        self.blob, self.b = blob, ngram.Blob(blob)
        self.start_state, self.memo, self.depth = self.b.start_state, {}, [0] * 6

    def score(self, s, c):
        if (s, c) not in self.memo:
            d, at = 0, s
            while at != 0 and self.b.find(at, c) is None:
                d, at = d + 1, int(self.b.bo_state[at])
            self.memo[(s, c)] = self.b.score(s, c) + (d,)
        l, nx, d = self.memo[(s, c)]
        self.depth[d] += 1
        return l, nx


def _model(x, V, order, kind, load, seed):
    """an estimated model over the table's own labels: "dense" - the arg-max label sequence and random sentences over
    the tokens the table favours; "sparse" - the arg-max sequence alone, so that the beam's other candidates find no arc
    at any level and back off the whole chain"""
    rng = np.random.default_rng(seed)
    top = [int(v) for v in np.argmax(x, 1)]
    seq = [v for v in R.collapse(top, 0)]
    sents = [seq[k:k + 12] for k in range(0, len(seq), 12)]
    if kind == "dense" and V > 2:
        fav = sorted(set(seq)) or [1]
        sents += [[int(fav[i]) for i in rng.integers(0, len(fav), int(rng.integers(2, 9)))] for _ in range(150)]
    model = NR.estimate([s for s in sents if s], V, order)
    if load > 0.5:
        # the table comes out as full as ``load`` allows: the longest n-grams are dropped (longest first, so the model
        # stays closed under prefixes) until the arcs fill floor(load 2^k) slots of 2^k
        arcs = sorted((g for g in model if len(g) > 1), key=lambda g: (-len(g), g))
        k = 1
        while int(load * (2 << k)) <= len(arcs):
            k += 1
        for g in arcs[:max(0, len(arcs) - int(load * (1 << k)))]:
            del model[g]
    return Memo(ngram.pack(model, V, order, load=load))


class Trace:
    """the contract's run over a whole table, the state and the store's length after every frame"""

    def __init__(self, x, blank, B, C, lm, alpha, beta, cap=None):
        self.x, self.blank, self.B, self.C, self.lm, self.alpha, self.beta = x, blank, B, C, lm, alpha, beta
        self.cap = 1 + B * len(x) if cap is None else cap
        self.rows = R.rows(x, blank, C)
        self.gaps, self.store = [], []
        state = L.scan(L.initial(lm), [], self.store, self.cap, B, lm, alpha, beta)
        self.snaps = [(state, len(self.store))]
        for row in self.rows:
            state = L.scan(state, [row], self.store, self.cap, B, lm, alpha, beta, self.gaps)
            self.snaps.append((state, len(self.store)))

    def condition(self, name):
        near = [g for g in self.gaps if g != 0.0 and not g >= MIN_GAP]
        assert not near, (name, min(near))
        return min([g for g in self.gaps if g != 0.0], default=np.inf)

    def at(self, t):
        state, k = self.snaps[t]
        return state, self.store[:k]

    def carried(self, t):
        state, store = self.at(t)
        return {"n_frames": state[0], "n_bad": state[1], "n_nodes": state[2], "entries": list(state[3]),
                "nodes": list(store), "side": list(state[4])}


WORST = {"ratio": 0.0, "abs": 0.0}


def _same(name, got, after, want, wstore, cap):
    n, nbad, nn, ent, side = want
    assert (got["n_frames"], got["n_bad"], got["n_nodes"]) == (n, nbad, nn), (name, got["n_frames"], got["n_bad"],
                                                                             got["n_nodes"], want[:3])
    assert [e[:4] for e in got["entries"]] == [e[:4] for e in ent], (name, [e[:4] for e in got["entries"]],
                                                                     [e[:4] for e in ent])
    assert [s[1] for s in got["side"]] == [s[1] for s in side], (name, got["side"], side)
    assert np.asarray([s[0] for s in got["side"]], np.float64).tobytes() == \
        np.asarray([s[0] for s in side], np.float64).tobytes(), (name, got["side"], side)
    for g, w in zip(got["entries"], ent):
        for a, b in zip(g[4:], w[4:]):
            if b == NEG or a == NEG:
                assert a == b, (name, g, w)
            else:
                err = abs(a - b)
                assert err <= BAR(n, b), (name, a, b, err, BAR(n, b))
                WORST["ratio"] = max(WORST["ratio"], err / BAR(n, b))
                WORST["abs"] = max(WORST["abs"], err)
    raw, raw_lm = got["raw_state"], got["raw_lm"]
    assert int(raw["i"][3]) == len(ent), name
    for r in range(len(ent), 16):                                    # the unused slots
        assert tuple(raw["e"][r]["i"]) == R.EMPTY_ENTRY[:4] and tuple(raw["e"][r]["p"]) == (NEG, NEG), (name, r)
        assert (raw_lm["lm"][r], raw_lm["ctx"][r]) == (0.0, 0), (name, r)
    assert after[0].tobytes() == raw.tobytes() and after[1].tobytes() == raw_lm.tobytes(), name
    k = min(nn, cap)
    assert len(wstore) == k and got["nodes"] == list(wstore), (name, got["nodes"][:5], list(wstore)[:5])
    assert (got["raw_nodes"][:k, 3] == 0).all() and (got["raw_nodes"][k:] == -7).all(), name


def _run(be, dev, tr, name, spans, chain):
    tab = _strided(tr.x)
    jobs = [(tab, tr.blank, t0, t1, None if t0 == 0 else tr.carried(t0), tr.cap, tr.B, tr.C) for t0, t1 in spans]
    got, after = be.ctc_beam_lm(jobs, dev, tr.alpha, tr.beta)
    for (t0, t1), g, a in zip(spans, got, after):
        st, store = tr.at(t1)
        _same(f"{name} span ({t0}, {t1})", g, a, st, store, tr.cap)
    state = None
    for a, b in zip(chain[:-1], chain[1:]):
        (state,), (aft,) = be.ctc_beam_lm([(tab, tr.blank, a, b, state, tr.cap, tr.B, tr.C)], dev, tr.alpha, tr.beta)
        st, store = tr.at(b)
        _same(f"{name} chain [{a}, {b})", state, aft, st, store, tr.cap)
    assert spans[0] == (0, chain[-1])
    assert _bits(state) == _bits(got[0]) and state["raw_lm"].tobytes() == got[0]["raw_lm"].tobytes(), name
    return got


# per (B, C): the model's order; per V: how the model is made and packed.  (16, 16) holds 272 items, the fifth of a lane.
ORDER = {(1, 1): 1, (2, 3): 2, (8, 8): 4, (16, 16): 4}
MODEL = {2: ("dense", 0.5), 65: ("dense", 0.5), 1024: ("dense", 0.95), 1500: ("sparse", 0.5)}
WEIGHTS = {(1, 1): (0.5, 0.0), (2, 3): (0.3, 0.5), (8, 8): (0.5, 0.3), (16, 16): (0.8, -0.2)}
# seeds per (V, B, C) at which the condition holds, found on the CPU (default: 1000 V + 16 B + C)
SEEDS = {(1500, 16, 16): 1}


@functools.lru_cache(maxsize=None)
def _case(V, B, C, T=300):
    seed = SEEDS.get((V, B, C), 1000 * V + 16 * B + C)
    x = _structured(np.random.default_rng(seed), T, V)
    kind, load = MODEL[V]
    order = min(ORDER[(B, C)], 2) if V == 2 else ORDER[(B, C)]
    lm = _model(x, V, order, kind, load, seed)
    return Trace(x, 0, B, C, lm, *WEIGHTS[(B, C)]), lm


@pytest.mark.parametrize("BC", [(1, 1), (2, 3), (8, 8), (16, 16)], ids=lambda bc: f"B{bc[0]}C{bc[1]}")
@pytest.mark.parametrize("V", [2, 65, 1024, 1500])
def test_kernel_equals_the_contract_at_every_width_beam_order_and_load(be, V, BC):
    B, C = BC
    tr, lm = _case(V, B, C)
    name = f"V={V} B={B} C={C} order={lm.b.order}"
    gap = tr.condition(name)
    final = tr.at(300)[0]
    assert final[0] == 300 and final[2] > 20 and (V == 2 or len(final[3]) == B)
    if V == 1500 and lm.b.order == 4:
        assert lm.depth[3] > 1000, lm.depth                          # the whole backoff chain is walked, often
    if V == 1024:
        assert lm.b.order == 1 or lm.b.n_arcs > 0.93 * lm.b.n_slots   # packed at load 0.95: long probe runs
    dev = be.language_model(lm.blob)
    _run(be, dev, tr, name, [(0, 300), (40, 300), (TILE - 1, TILE + 1), (7, 7)], chain=[0, 17, TILE, 300])
    dev.close()
    print(f"\n{name}: {lm.b.n_states} states, {lm.b.n_arcs} arcs in {lm.b.n_slots} slots, lookups by backoff depth "
          f"{lm.depth[:5]}; smallest non-zero gap {gap:.2e}; largest |pb, pnb - contract| so far {WORST['abs']:.3e} = "
          f"{WORST['ratio']:.4f} of the bar")


def test_the_model_changes_the_result():
    """(what the cases above compare is not the plain search under another name)"""
    tr, lm = _case(65, 8, 8)
    plain, _ = R.scan_table(tr.x, 0, 8, 8)
    assert [e[:4] for e in plain[3]] != [e[:4] for e in tr.at(300)[0][3]]


@pytest.mark.parametrize("V,B,C", [(65, 8, 8), (1024, 16, 16), (1500, 2, 3)])
def test_without_a_model_or_with_zero_weights_every_bit_of_the_plain_launch(be, V, B, C):
    tr, lm = _case(V, B, C)
    tab = _strided(tr.x)
    cap = tr.cap
    plain_tr = R.scan_table(tr.x[:40], 0, B, C)                      # a carried state of the PLAIN search
    carried = {"n_frames": 40, "n_bad": 0, "n_nodes": plain_tr[0][2], "entries": list(plain_tr[0][3]),
               "nodes": list(plain_tr[1])}
    jobs = [(tab, 0, 0, 300, None, cap, B, C), (tab, 0, 40, 300, carried, cap, B, C), (tab, 0, 0, 17, None, cap, B, C)]
    want, want_after = be.ctc_beam(jobs)
    dev = be.language_model(lm.blob)
    # the model's side of a carried state: what the fused run itself left after the same 40 rows
    (head,), _ = be.ctc_beam_lm([(tab, 0, 0, 40, None, cap, B, C)], dev, 0.0, 0.0)
    assert _bits(head)[0] == be.ctc_beam([(tab, 0, 0, 40, None, cap, B, C)])[0][0]["raw_state"].tobytes()
    fjobs = [jobs[0], jobs[1][:4] + (dict(carried, side=head["side"]),) + jobs[1][5:], jobs[2]]
    for what, (model, a, b) in {"no model": (None, 0.7, 0.3), "zero weights": (dev, 0.0, 0.0)}.items():
        got, after = be.ctc_beam_lm(fjobs, model, a, b)
        for k in range(len(jobs)):
            assert _bits(got[k]) == _bits(want[k]), (what, k)
            assert after[k][0].tobytes() == want_after[k].tobytes(), (what, k)
            if model is None:                                        # lm_state is neither read nor written
                assert (_ints(got[k]["raw_lm"]) == -7).all() == (k != 1) and (_ints(after[k][1]) == -7).all(), (what, k)
    dev.close()


def test_a_malformed_job_writes_nothing_while_its_neighbours_are_served(be):
    tr, lm = _case(65, 2, 3)
    tab = _strided(tr.x)
    dev = be.language_model(lm.blob)
    other = _model(tr.x[:, :64], 64, 2, "dense", 0.5, 3)
    dev64 = be.language_model(other.blob)                            # a model over 64 tokens for a table of 65

    def setter(**kw):
        def tweak(k, j):
            if k == 1:
                for f, v in kw.items():
                    setattr(j, f, v)
        return tweak

    bad = [dict(lm=dev64.view), dict(lm_state=None), dict(alpha=float("nan")), dict(beta=float("inf")), None]
    for i, kw in enumerate(bad):
        got, after = be.ctc_beam_lm([(tab, 0, 0, 50, None, tr.cap, 2, 3)] * 3, dev, tr.alpha, tr.beta,
                                    tweak=setter(**kw) if kw else None)
        if kw is not None:
            assert (_ints(got[1]["raw_state"]) == -7).all() and (got[1]["raw_nodes"] == -7).all(), kw
            assert (_ints(got[1]["raw_lm"]) == -7).all(), kw
            assert (_ints(after[1][0]) == -7).all() and (_ints(after[1][1]) == -7).all(), kw
        for k in (0, 2) if kw is not None else (0, 1, 2):
            _same(f"neighbour {i}.{k}", got[k], after[k], *tr.at(50), tr.cap)
    # a stored ctx outside the model's states: nothing is written
    broken = dict(tr.carried(20))
    broken["side"] = [(s[0], lm.b.n_states) for s in broken["side"]]
    got, after = be.ctc_beam_lm([(tab, 0, 20, 50, tr.carried(20), tr.cap, 2, 3), (tab, 0, 20, 50, broken, tr.cap, 2, 3)],
                                dev, tr.alpha, tr.beta)
    _same("carried", got[0], after[0], *tr.at(50), tr.cap)
    assert got[1]["n_frames"] == 20 and (_ints(after[1][0]) == -7).all() and (_ints(after[1][1]) == -7).all()
    from speechcatcher_amd import _abi
    lib = _abi.load()
    assert lib.sc_ctc_beam_lm(None, 0, None) == 0
    assert lib.sc_ctc_beam_lm(None, 2, None) == -1 and lib.sc_ctc_beam_lm(None, -1, None) == -1
    assert lib.sc_ctc_beam_lm(tab.data_ptr(), _abi.BEAM_MAX_JOBS + 1, None) == -1
    dev.close()
    dev64.close()


def test_a_blob_that_fails_validation_is_refused_and_allocates_nothing(be):
    tr, lm = _case(65, 2, 3)
    from speechcatcher_amd import _abi
    bad = bytearray(lm.blob)
    bad[-8:-4] = (lm.b.n_states).to_bytes(4, "little")                # the last slot's next out of range, used or not ...
    bad[-24:-16] = ((1 << 32) | 1).to_bytes(8, "little")              # ... under a key
    for blob in (bytes(bad), lm.blob[:-1], b""):
        with pytest.raises(_abi.ScasrError, match="language model blob"):
            be.language_model(blob)
