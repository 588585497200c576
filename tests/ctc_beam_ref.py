"""Contract of the CTC prefix beam search (csrc/ctc_beam.hip, sc_ctc_beam / sc_ctc_beam_pack), numpy
float64.

State of a stream over its utterance:
    n_frames, n_bad, n_nodes (int32) and up to B entries, best first, each
    (node, last, len, parent, pb, pnb): node = id of the prefix in the stream's prefix tree (0: the empty prefix), last =
    its last token (-1: none), len = its length, parent = the node of the prefix without its last token (-1: none),
    pb / pnb = float64 log probability of the prefix with the path ending in blank / in last.
    The initial state is the one entry (0, -1, 0, -1, 0.0, -inf) with n_nodes = 1.
The tree is a store of (parent, token, frame) records, node k of the utterance at slot k ((-1, -1, -1) at slot 0), never
touched once stored; a node at or beyond the store's capacity is counted, not written.

Parameters 1 <= B <= 16 (entries kept), 1 <= C <= 16 (candidate tokens per frame).  A state that holds more than B
entries is cut to its first B before the first frame.  Frames are numbered in the order they are scanned.  For frame n
with the fp32 row x[0..V):
    a row that holds a NaN or +inf, or nothing but -inf, is BAD (the rule of ctc_draft_ref): n_bad += 1, n_frames += 1,
    nothing else changes.
    lse = m + log(sum_v exp(x[v] - m)), x promoted to float64, v ascending (ctc_activity_ref);  lp(v) = x[v] - lse.
    candidates: the C non-blank tokens with the largest x, compared as fp32, the lowest index among ties; tokens at -inf
    are left out; fewer than C when V - 1 < C.
    lae(a, b) = max + log1p(exp(min - max)); the other argument when one is -inf.
    for entry i:  tot_i = lae(pb_i, pnb_i)
        stay        pb'_i = tot_i + lp(blank);  pnb'_i = pnb_i + lp(last_i) if last_i is a candidate, else -inf
        extension by candidate c:  ext = (pb_i if c == last_i else tot_i) + lp(c).  If an entry j of the beam has
                    parent_j == node_i and last_j == c (the prefix is in the beam already; at most one such term per j),
                    pnb'_j = lae(pnb'_j, ext); else a new prefix with (pb, pnb) = (-inf, ext).
    keep the B best by total = lae(pb', pnb'), those at -inf dropped; order: total descending, stays before new
    prefixes, lower rank i (a stay's own, a new prefix's parent's), lower token.  Kept new prefixes get the node ids
    n_nodes, n_nodes + 1, ... in that order, with the record (node_i, c, n).
scan(state, span) -> state; any split of a table into consecutive spans (empty ones included) gives the bits of the
one-span scan: the per-frame operations are the same.
"""
import numpy as np

import ctc_row_ref as row_ref

MAX_B = MAX_C = 16
NEG = -np.inf
ENTRY_FIELDS = ("node", "last", "len", "parent", "pb", "pnb")
EMPTY_ENTRY = (-1, -1, 0, -1, NEG, NEG)      # what the unused slots of a state hold
ROOT = (-1, -1, -1)                           # node 0


def initial():
    """(n_frames, n_bad, n_nodes, entries)"""
    return (0, 0, 1, [(0, -1, 0, -1, 0.0, NEG)])


def lae(a: float, b: float) -> float:
    if a == NEG:
        return b
    if b == NEG:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return float(hi + np.log1p(np.exp(lo - hi)))


def rows(table, blank: int, C: int):
    """per row of table [T, V] fp32: None for a bad row, else (candidate ids, their lp, lp(blank))"""
    x32 = np.asarray(table, np.float32)
    out = []
    for r32 in x32:
        if row_ref.is_bad(r32):
            out.append(None)
            continue
        row = r32.astype(np.float64)
        lse = row_ref.lse(r32)
        order = np.argsort(-r32, kind="stable")            # descending, the lowest index first among equals
        cand = [int(v) for v in order if v != blank and r32[v] > NEG][:C]
        out.append((cand, [float(row[v] - lse) for v in cand], float(row[blank] - lse)))
    return out


def step(state, row, store: list, capacity: int, B: int):
    """one frame: state + one element of rows() -> (the new state, every finite item (total, kind, i, token) in order;
    None for a bad row); the records of new nodes are appended to ``store`` while it holds fewer than ``capacity``"""
    n, nbad, nn, ent = state
    if row is None:
        return (n + 1, nbad + 1, nn, ent), None
    cand, lpc, lpb = row
    lp = dict(zip(cand, lpc))
    tot = [lae(e[4], e[5]) for e in ent]
    pb2 = [tot[i] + lpb for i in range(len(ent))]
    pnb2 = [e[5] + lp[e[1]] if e[1] in lp else NEG for e in ent]
    fresh = []
    for i, e in enumerate(ent):
        for c in cand:
            ext = (e[4] if c == e[1] else tot[i]) + lp[c]
            js = [j for j, f in enumerate(ent) if f[3] == e[0] and f[1] == c]
            assert len(js) <= 1
            if js:
                pnb2[js[0]] = lae(pnb2[js[0]], ext)
            else:
                fresh.append((ext, 1, i, c))
    items = [(lae(pb2[i], pnb2[i]), 0, i, -1) for i in range(len(ent))] + fresh
    items = sorted((it for it in items if it[0] > NEG), key=lambda it: (-it[0], it[1], it[2], it[3]))
    new = []
    for total, kind, i, c in items[:B]:
        e = ent[i]
        if kind == 0:
            new.append((e[0], e[1], e[2], e[3], pb2[i], pnb2[i]))
        else:
            if nn < capacity:
                assert len(store) == nn
                store.append((e[0], c, n))
            new.append((nn, c, e[2] + 1, e[0], NEG, total))
            nn += 1
    return (n + 1, nbad, nn, new), items


def scan(state, rws, store: list, capacity: int, B: int, gaps: list = None):
    """state + a span of rows() -> the new state.  ``gaps``: if a list, every gap between consecutive kept totals and
    between the B-th and the (B+1)-th of every frame is appended (the condition of an integer comparison)."""
    n, nbad, nn, ent = state
    state = (n, nbad, nn, list(ent[:B]))
    if nn >= 1 and not store and capacity > 0:
        store.append(ROOT)
    for row in rws:
        state, items = step(state, row, store, capacity, B)
        if gaps is not None and items is not None:
            tots = [it[0] for it in items[:B + 1]]
            gaps.extend(a - b for a, b in zip(tots[:-1], tots[1:]))
    return state


def scan_table(table, blank: int, B: int, C: int, state=None, store=None, capacity: int = 1 << 30, gaps: list = None):
    """(state after the rows of ``table``, the node store)"""
    store = [] if store is None else store
    return scan(initial() if state is None else state, rows(table, blank, C), store, capacity, B, gaps), store


def total(entry) -> float:
    return lae(entry[4], entry[5])


def backtrace(entry, store):
    """(token ids, first-emission frames) of an entry's prefix, in order; None when a node of its chain is not stored"""
    ids, frames, node = [], [], entry[0]
    for _ in range(entry[2]):
        if not 0 < node < len(store):
            return None
        parent, tok, frame = store[node]
        ids.append(tok)
        frames.append(frame)
        node = parent
    return ids[::-1], frames[::-1]


def collapse(path, blank: int):
    out, prev = [], blank
    for k in path:
        if k != blank and k != prev:
            out.append(k)
        prev = k
    return tuple(out)
