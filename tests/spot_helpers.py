"""Shared by the phrase-spotting tests: constructed CTC tables with planted phrases, random phrase sets, and the choice
of phrases and floors from a table of the engine."""
import numpy as np

import ctc_spot_ref as R
from speechcatcher_amd import synth
from speechcatcher_amd.config import SearchConfig
from speechcatcher_amd.weights import PackedWeights
from helpers import CFGS


def packed_weights(cfg_name, device, seed=1234):
    """the seeded synthetic model as it is: its CTC arg-max path is tokens, not blanks - phrases can be cut from it"""
    cfg = CFGS[cfg_name]
    mean, std = synth.stats_to_mean_std(synth.make_stats(cfg, kind="meanstd"))
    return PackedWeights(synth.make_state_dict(cfg, seed), cfg, device, mean, std)


def make_batch(cfg_name, backend, n_streams, beam=3, device="cpu", weights=None, **kw):
    """backend: "native" = the C++ engine, else a backend object for the Python engine"""
    w = weights if weights is not None else packed_weights(cfg_name, device)
    sc = SearchConfig(beam_size=beam, use_bbd=True)
    if isinstance(backend, str) and backend == "native":
        from speechcatcher_amd.native import NativeStreamBatch
        return NativeStreamBatch(w, n_streams, sc, **kw)
    from speechcatcher_amd.engine import StreamBatch
    return StreamBatch(w, backend, n_streams, sc, **kw)


def ctc_path(y, blank):
    """the shortest frame-label path that spells y: one frame per token, a blank between adjacent repeats"""
    path = []
    for i, t in enumerate(y):
        if i and y[i - 1] == t:
            path.append(blank)
        path.append(int(t))
    return path


def plant_table(rng, T, V, blank, plants, noise=1.0, blank_bias=8.0, hi=14.0):
    """[T, V] fp32 table: unit noise, the blank ahead by `blank_bias` everywhere, and for every (start, y) in `plants` the
    labels of ctc_path(y) ahead by `hi` on the frames from `start` on.  Returns (table, [end frame of each plant])."""
    x = (rng.standard_normal((T, V)) * noise).astype(np.float32)
    x[:, blank] += np.float32(blank_bias)
    ends = []
    for start, y in plants:
        path = ctc_path(y, blank)
        assert start + len(path) <= T
        for f, lab in enumerate(path):
            x[start + f, lab] += np.float32(hi)
        ends.append(start + len(path) - 1)
    return x, ends


def random_phrases(rng, P, V, blank, lengths):
    """P phrases whose lengths cycle through `lengths`; about a third of the joints are adjacent repeats"""
    labels = [v for v in range(V) if v != blank]
    out = []
    for p in range(P):
        L = lengths[p % len(lengths)]
        y = [int(rng.choice(labels))]
        while len(y) < L:
            y.append(y[-1] if rng.random() < 0.33 else int(rng.choice(labels)))
        out.append(y)
    return out


def trace_end_values(table, blank, phrases, floors, mask=R.ALL, snap_at=()):
    """the contract run over `table` from the start of an utterance, frame by frame -> (state, [P] lists of the FINITE
    end-state values of every frame, taken before the fire decision, {t: the state after t frames} for t in snap_at)"""
    P = len(phrases)
    vals = [[] for _ in range(P)]
    st = R.initial(P)
    snaps = {0: st} if 0 in snap_at else {}
    never = np.full(P, np.inf)
    for t in range(len(table)):
        nxt = R.scan(st, table[t:t + 1], blank, phrases, floors, mask)
        # (a phrase that fired has its states at -inf: its end value was the score - recomputed without the floors)
        seen = nxt if nxt["n_events"] == st["n_events"] else R.scan(st, table[t:t + 1], blank, phrases, never, mask)
        for p in range(P):
            v = seen["values"][p, 2 * len(phrases[p]) - 2]
            if np.isfinite(v) and (mask >> p) & 1:
                vals[p].append(float(v))
        st = nxt
        if t + 1 in snap_at:
            snaps[t + 1] = st
    return st, vals, snaps


def gap_floors(values, top=16):
    """candidate floors of a phrase, best first: the midpoints of the gaps between consecutive values among the `top`
    largest DISTINCT end-state values (0.0, a perfect path, included), widest gap first.  The seeded synthetic models'
    rows are nearly flat - the maximum lies about 1.8 nats above the median, runners-up within 0.1 -, so the values are
    dense and the widest gap of ALL of them lies deep in the tail, where a phrase would fire on every other frame; among
    the best few it separates the occurrences from the near misses."""
    v = np.unique(np.asarray([0.0] + [x for x in values if x <= 0.0]))[::-1][:top]
    if v.size < 2:
        return [-1.0]
    d = -np.diff(v)
    return [float(0.5 * (v[i] + v[i + 1])) for i in np.argsort(-d, kind="stable")]


def choose_floors(tables, blank, phrases, n=None, margin=1.5e-3):
    """(phrases, floors): per phrase (phrases do not see each other) the floor in the widest gap of gap_floors - over the
    end-state values of all the tables with a floor of 0 - with which the contract's run keeps every end-state value of
    every frame at least `margin` away from the floor (a floor moves the fires, and with them the values behind them).
    A phrase without such a floor is left out; the first n (default: all given) that have one are returned."""
    n = len(phrases) if n is None else n
    kept, floors = [], []
    for y in phrases:
        vals = sum((trace_end_values(t, blank, [y], np.zeros(1))[1][0] for t in tables), [])
        for f in gap_floors(vals):
            got = sum((trace_end_values(t, blank, [y], np.asarray([f]))[1][0] for t in tables), [])
            if np.abs(np.asarray(got) - f).min(initial=np.inf) >= margin:
                kept.append(y)
                floors.append(f)
                break
        if len(kept) == n:
            break
    assert len(kept) == n, f"only {len(kept)} of {n} phrases have a floor with a margin of {margin}"
    return kept, np.asarray(floors)


def phrases_from_paths(tables, blank, n_phrases, lengths=(1, 2, 3, 4)):
    """phrases cut from the collapsed arg-max paths of the tables (round robin over the tables, spread over each path)"""
    paths = [[c[0] for c in R.collapse(np.argmax(t, 1), blank)] for t in tables]
    out, k = [], 0
    while len(out) < n_phrases and k < 50 * n_phrases:
        path = paths[k % len(paths)]
        L = lengths[k % len(lengths)]
        if len(path) >= L:
            i = (k * 7) % (len(path) - L + 1)
            y = path[i:i + L]
            if y not in out:
                out.append(y)
        k += 1
    assert len(out) == n_phrases, "the arg-max paths are too short to cut the phrases from"
    return out
