"""N-gram rescoring of n-best lists on the GPU (csrc/lm_rescore.hip: sc_lm_rescore) against the float64 contract of
tests/lm_rescore_ref.py: EVERY output bit for bit - float64 as uint64, every int32 (the arithmetic is exact lookups and
additions in one fixed order; there is no tolerance).  The shapes are the smallest at which the kernel can go wrong:
label counts 0, 1, order - 1, order and 63, 64, 65, 130 (a tile of 64 and its carry) mixed within one list, 1, 2, 5 and
16 rows (more rows than the workgroup has waves), orders 1, 2, 3, 5, vocabularies 2, 65, 1024, a table packed at load
0.95, a model whose lookups back off the whole chain.  For every model the packer made no row may carry
SC_RESCORE_SERIAL (the speculate-and-verify path provably ran); a blob the validator accepts whose next fields are
inconsistent must send rows to the serial fallback and still give the contract's bits."""
import functools
import struct

import numpy as np
import pytest
import torch

import lm_rescore_ref as RS
from speechcatcher_amd import _abi, ngram

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from speechcatcher_amd.hip_backend import HipBackend
    return HipBackend("cuda:0", use_graphs=False)


class Memo:
    """a packed model with its scores remembered, and how deep the lookups backed off"""

    def __init__(self, blob):
        self.blob, self.b = bytes(blob), ngram.Blob(bytes(blob))
        self.V, self.order, self.n_states, self.start_state = self.b.V, self.b.order, self.b.n_states, self.b.start_state
        self.memo, self.depth = {}, [0] * 6

    def score(self, s, c):
        if (s, c) not in self.memo:
            d, at = 0, s
            while at != 0 and self.b.find(at, c) is None:
                d, at = d + 1, int(self.b.bo_state[at])
            self.memo[(s, c)] = self.b.score(s, c) + (d,)
        l, nx, d = self.memo[(s, c)]
        self.depth[d] += 1
        return l, nx


def _sentences(rng, V, n, length):
    return [[int(v) for v in rng.integers(0, V, length)] for _ in range(n)]


def _model_of(sents, V, order, rng, load=0.5, bos=None):
    """every n-gram of the sentences up to ``order`` with random values (closed under prefixes and suffixes), a unigram
    for every token but - above 2 tokens - the last; at a load above 0.5 the longest n-grams are dropped until the arcs
    fill floor(load 2^k) slots of 2^k"""
    val = lambda: (float(-rng.uniform(0.1, 6.0)), float(-rng.uniform(0.0, 2.0)))     # noqa: E731
    model = {(w,): val() for w in range(V - 1 if V > 2 else V)}
    for s in sents:
        for n in range(2, order + 1):
            for k in range(len(s) - n + 1):
                g = tuple(s[k:k + n])
                if all(t < (V - 1 if V > 2 else V) for t in g) and g not in model:
                    model[g] = val()
    if load > 0.5:
        arcs = sorted((g for g in model if len(g) > 1), key=lambda g: (-len(g), g))
        k = 1
        while int(load * (2 << k)) <= len(arcs):
            k += 1
        for g in arcs[:max(0, len(arcs) - int(load * (1 << k)))]:
            del model[g]
    return Memo(ngram.pack(model, V, order, load=load, bos=bos))


def _rows(rng, sents, V, n, width, swap):
    """n rows of ``width`` tokens read off the sentences' stream, a share ``swap`` of them replaced at random"""
    stream = np.asarray([t for s in sents for t in s] * (2 + width // 8), np.int32)
    out = np.zeros((n, width), np.int32)
    for h in range(n):
        a = int(rng.integers(0, len(stream) - width))
        out[h] = stream[a:a + width]
        hit = rng.random(width) < swap
        out[h, hit] = rng.integers(0, V, int(hit.sum()))
    return out


# kind: (sentences, their length, share of swapped tokens, load)
KINDS = {"dense": (40, 30, 0.15, 0.5), "full": (60, 30, 0.15, 0.95), "sparse": (1, 60, 0.25, 0.5)}
MODELS = [(2, 1, "dense", None), (2, 2, "dense", 1), (65, 2, "dense", 7), (65, 3, "dense", None), (65, 5, "dense", 3),
          (65, 5, "sparse", None), (1024, 3, "full", None), (1024, 5, "dense", 11), (1024, 1, "dense", None)]
STRIP = 1     # the token the rows may end in


@functools.lru_cache(maxsize=None)
def _case(V, order, kind, bos):
    """(model, jobs as dicts of host arrays, the contract's outputs) - computed once, shared by the tests"""
    seed = 1000 * V + 10 * order + len(kind)
    rng = np.random.default_rng(seed)
    ns, sl, swap, load = KINDS[kind]
    sents = _sentences(rng, V if kind != "sparse" else V - 1, ns, sl)
    lm = _model_of(sents, V, order, rng, load, bos)
    counts = [0, 1, max(order - 1, 0), order, 63, 64, 65, 130]
    jobs = []
    for k, n in enumerate([1, 2, 5, 16, 16, 5, 2, 1]):
        skip = k % 2
        m = [counts[(h * 3 + k) % 8] for h in range(n)]                 # 3 is coprime to 8: 16 rows hold every count twice
        if n == 1:
            m = [130 if k == 0 else counts[2]]
        ends = [bool((h + k) % 3 == 0) for h in range(n)]               # the row ends in STRIP (behind its labels)
        lens = [skip + m[h] + int(ends[h]) for h in range(n)]
        L = max(lens) + (k % 3)
        rows = _rows(rng, sents, V, n, L + 2, swap)
        for h in range(n):
            if ends[h]:
                rows[h, lens[h] - 1] = STRIP
        uniform = n == 2 and k == 6                                     # one list without lens: L for every row
        if uniform:
            L, lens = lens[0], None
        jobs.append({"rows": rows, "scores": rng.uniform(-60.0, -1.0, n), "lens": lens, "L": L, "skip": skip,
                     "strip": STRIP if k % 4 != 3 else -1,             # -1: the trailing token is a label (strip missed)
                     "state0": -1 if k % 3 else int(rng.integers(0, lm.n_states)),
                     "lm_eos": -1 if k % 2 == 0 else (V - 2 if V > 2 else 0),
                     "alpha": float(rng.uniform(0.1, 1.0)), "beta": float(rng.uniform(-0.5, 0.5)), "tok": k % 4 != 1})
    # a list with a bad token, a non-finite total and an exact tie
    rows = _rows(rng, sents, V, 5, 12, swap)
    rows[1, 5] = V
    rows[4] = rows[0]
    jobs.append({"rows": rows, "scores": np.asarray([-3.0, -1.0, np.nan, -np.inf, -3.0]), "lens": [10, 10, 10, 9, 10],
                 "L": 10, "skip": 1, "strip": -1, "state0": -1, "lm_eos": -1, "alpha": 0.5, "beta": 0.25, "tok": True})
    want = [RS.rescore(lm, j["rows"], j["scores"], j["lens"], j["L"], j["skip"], j["strip"], j["state0"], j["lm_eos"],
                       j["alpha"], j["beta"]) for j in jobs]
    return lm, jobs, want


def _device(jobs, flags=0):
    out = []
    for j in jobs:
        buf = torch.full((j["rows"].shape[0], j["rows"].shape[1] + 3), -9, dtype=torch.int32, device="cuda:0")
        buf[:, :j["rows"].shape[1]] = torch.from_numpy(j["rows"]).to("cuda:0")
        out.append(dict(j, rows=buf[:, :j["rows"].shape[1]], scores=torch.from_numpy(np.asarray(j["scores"])).to("cuda:0"),
                        flags=flags))
    return out


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(name, got, want, job, serial):
    n = job["rows"].shape[0]
    for key in ("lm", "eos_lm", "fused"):
        assert (_u64(got[key]) == _u64(want[key])).all(), (name, key, got[key], want[key])
    for key in ("end_state", "order"):
        assert (got[key] == want[key]).all(), (name, key, got[key], want[key])
    assert ((got["status"] & ~RS.SERIAL) == want["status"]).all(), (name, got["status"], want["status"])
    assert ((got["status"] & RS.SERIAL) == (RS.SERIAL if serial else 0)).all(), (name, got["status"])
    if job["tok"]:
        for h in range(n):
            m = int(want["m"][h])
            assert (_u64(got["tok_lm"][h, :m]) == _u64(want["tok_lm"][h])).all(), (name, h)
            assert (got["tok_lm"][h, m:] == -7.0).all(), (name, h)
    else:
        assert got["tok_lm"] is None
    raw = got["raw"]
    assert (raw["f64"][:, n:] == -7.0).all() and (raw["i32"][:, n:] == -7).all(), name
    w = got["tok_lm"].size if job["tok"] else 0
    assert (raw["tok"][w:] == -7.0).all(), name


@pytest.mark.parametrize("V,order,kind,bos", MODELS, ids=lambda v: str(v))
def test_kernel_equals_the_contract_bit_for_bit_on_both_paths(be, V, order, kind, bos):
    lm, jobs, want = _case(V, order, kind, bos)
    name = f"V={V} order={order} {kind}"
    assert lm.order == order and (bos is None or order == 1 or lm.start_state != 0)
    if kind == "full":
        assert lm.b.n_arcs > 0.93 * lm.b.n_slots                        # packed at load 0.95: long probe runs
    if kind == "sparse":
        assert lm.depth[order - 1] > 50, lm.depth                        # the whole backoff chain is walked, often
    elif order > 1 and V > 2:
        assert lm.depth[0] > 200 and sum(lm.depth[1:]) > 50, lm.depth    # arcs found at the full context, and backoffs
    assert any(w["eos_lm"].any() for w in want) and any((w["status"] & RS.BAD_TOKEN).any() for w in want)
    dev = be.language_model(lm.blob)
    fast = be.lm_rescore(_device(jobs), dev)
    for k, (g, w, j) in enumerate(zip(fast, want, jobs)):
        _same(f"{name} job {k}", g, w, j, serial=False)                  # NO row of a packed model leaves the fast path
    slow = be.lm_rescore(_device(jobs, flags=_abi.RESCORE_FORCE_SERIAL), dev)
    for k, (g, w, j) in enumerate(zip(slow, want, jobs)):
        _same(f"{name} job {k} forced serial", g, w, j, serial=True)
    dev.close()
    print(f"\n{name}: {lm.n_states} states, {lm.b.n_arcs} arcs in {lm.b.n_slots} slots, lookups by backoff depth "
          f"{lm.depth[:5]}")


def test_a_validated_but_inconsistent_blob_takes_the_fallback_and_keeps_the_contract(be):
    lm, jobs, _ = _case(65, 3, "dense", None)
    b = lm.b
    blob = bytearray(lm.blob)
    rng = np.random.default_rng(3)
    slots_at = len(blob) - 24 * b.n_slots
    root_next_at = slots_at - ((4 * b.V + 7) & ~7)
    used = [k for k in range(b.n_slots) if int(b.slots[k]["key"]) != ngram.EMPTY]
    for k in rng.choice(used, 40, replace=False):                        # arcs that lead somewhere else ...
        struct.pack_into("<i", blob, slots_at + 24 * int(k) + 16, int(rng.integers(0, b.n_states)))
    for v in rng.choice(b.V - 1, 6, replace=False):                      # ... and unigrams
        struct.pack_into("<i", blob, root_next_at + 4 * int(v), int(rng.integers(1, b.n_states)))
    bent = Memo(blob)
    dev = be.language_model(bent.blob)                                   # lm_blob.h accepts it: every field is in range
    jobs = [j for j in jobs if j["rows"].shape[0] in (5, 16)]
    want = [RS.rescore(bent, j["rows"], j["scores"], j["lens"], j["L"], j["skip"], j["strip"], j["state0"], j["lm_eos"],
                       j["alpha"], j["beta"]) for j in jobs]
    # on the CPU: the rows on which some window guess is not the state of the sequential walk
    expect = []
    for j, w in zip(jobs, want):
        off = []
        for h in range(j["rows"].shape[0]):
            if w["status"][h] & RS.BAD_TOKEN:
                off.append(False)
                continue
            y = RS.labels(j["rows"][h], j["L"] if j["lens"] is None else j["lens"][h], j["skip"], j["strip"])
            s, miss = (bent.start_state if j["state0"] < 0 else j["state0"]), False
            for t in range(len(y)):
                miss = miss or RS.window_guess(bent, y, t, j["state0"]) != s
                s = bent.score(s, y[t])[1]
            off.append(miss)
        expect.append(off)
    assert sum(map(sum, expect)) >= 3 and any(not all(e) for e in expect)
    got = be.lm_rescore(_device(jobs), dev)
    n_serial = 0
    for k, (g, w, j, off) in enumerate(zip(got, want, jobs, expect)):
        # a mismatch behind the last label's score cannot show: a row is serial only if a guess it USES is wrong
        serial = (g["status"] & RS.SERIAL) != 0
        assert (serial == np.asarray(off)).all(), (k, serial, off)
        n_serial += int(serial.sum())
        g = dict(g, status=g["status"] & ~RS.SERIAL)
        _same(f"bent job {k}", g, w, j, serial=False)
    assert n_serial >= 3
    dev.close()


def test_a_malformed_job_writes_nothing_while_its_neighbours_are_served(be):
    lm, jobs, want = _case(65, 3, "dense", None)
    k5 = next(k for k, j in enumerate(jobs) if j["rows"].shape[0] == 5 and j["tok"] and j["lens"] is not None)
    job, w = jobs[k5], want[k5]
    other = _model_of(_sentences(np.random.default_rng(1), 64, 5, 10), 64, 2, np.random.default_rng(2))
    dev, dev64 = be.language_model(lm.blob), be.language_model(other.blob)
    null = ("model", "yseq", "score", "lm", "eos_lm", "fused", "end_state", "order", "status")
    bad = [{f: None} for f in null] + [
        dict(n_hyp=0), dict(n_hyp=17), dict(L=-1), dict(row_stride=job["L"] - 1), dict(score_stride=0), dict(skip=-1),
        dict(strip=-2), dict(tok_stride=job["L"] - job["skip"] - 1), dict(V=64), dict(model=dev64.view),
        dict(state0=lm.n_states), dict(state0=-2), dict(lm_eos=65), dict(lm_eos=-2), dict(alpha=float("nan")),
        dict(beta=float("inf")), dict(flags=2)]

    def tweak(k, j):
        if 0 < k <= len(bad):
            for f, v in bad[k - 1].items():
                setattr(j, f, v)

    got = be.lm_rescore(_device([job] * (len(bad) + 2)), dev, tweak=tweak)
    for k, g in enumerate(got):
        if 0 < k <= len(bad):
            raw = g["raw"]
            assert (raw["f64"] == -7.0).all() and (raw["i32"] == -7).all() and (raw["tok"] == -7.0).all(), bad[k - 1]
        else:
            _same(f"neighbour {k}", g, w, job, serial=False)
    lib = _abi.load()
    assert lib.sc_lm_rescore(None, 0, None) == 0
    assert lib.sc_lm_rescore(None, 2, None) == -1 and b"null job table" in lib.sc_last_error()
    assert lib.sc_lm_rescore(None, -1, None) == -1 and b"negative" in lib.sc_last_error()
    assert lib.sc_lm_rescore(dev.view, _abi.RESCORE_MAX_JOBS + 1, None) == -1 and b"SC_RESCORE_MAX_JOBS" in lib.sc_last_error()
    dev.close()
    dev64.close()
