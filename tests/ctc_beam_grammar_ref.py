"""Contract of the grammar-constrained CTC prefix beam search (csrc/ctc_beam_grammar.hip, sc_ctc_beam_grammar;
DESIGN.md 8m), numpy float64, built ON tests/ctc_beam_ref.py.  Unchanged from that contract: the row rule (bad rows, lse,
lp), lae, the merge rule, the prune order and its ties, the node records and the chained-span property.

A grammar is a deterministic automaton over the token ids (speechcatcher_amd.grammar.Grammar: arcs(g) -> [(token, next)]
ascending by token, start_state).  State: ctc_beam_ref's (n_frames, n_bad, n_nodes, entries) and, beside entry i, g_i:
the automaton's state after its prefix.  The initial entry has start_state; the unused slots of a stored state hold 0.
Three things differ from ctc_beam_ref:
  1. candidates are per entry: entry i's are the C out-arc tokens of g_i with the largest x, compared as fp32, the lowest
     token among ties; tokens at -inf are left out; fewer than C when the state has fewer arcs - a state without arcs only
     stays.  Two entries in the same state have the same candidates.
  2. the stay's repeat term is unconditional: pnb'_i = pnb_i + lp(last_i), lp(v) = (double)x[v] - lse for ANY v; -inf
     when x[last_i] is -inf (and for the empty prefix, which has no last token).  ctc_beam_ref drops the term when last_i
     is no candidate of the frame; with per-entry candidates that would end every accepted phrase, whose last token is
     seldom an out-arc of the state it led to.
  3. a new prefix made from entry i by c gets g = next(g_i, c); a stay keeps g; an extension that merges leaves the
     target's g alone - the automaton is deterministic, so the same prefix has the same state (asserted here).
With the free grammar (one state, a self-loop on every non-blank token) and V - 1 <= C every non-blank token that is not
at -inf is a candidate, rule 2 coincides with ctc_beam_ref's, and the states and node stores are that contract's, exactly.
"""
import numpy as np

import ctc_beam_ref as R
import ctc_row_ref as row_ref

NEG = R.NEG


def initial(gr):
    return R.initial() + ([int(gr.start_state)],)


def rows(table):
    """per row of table [T, V] fp32: None for a bad row, else (the fp32 row, its lse)"""
    out = []
    for r32 in np.asarray(table, np.float32):
        out.append(None if row_ref.is_bad(r32) else (r32, row_ref.lse(r32)))
    return out


def candidates(gr, g: int, r32, C: int):
    """[(token, next)] of state g on the row: the C out-arcs with the largest x as fp32, the lowest token among ties"""
    arcs = [(t, n) for t, n in gr.arcs(g) if r32[t] > NEG]
    return sorted(arcs, key=lambda a: (-r32[a[0]], a[0]))[:C]


def step(state, row, store: list, capacity: int, B: int, C: int, gr, blank: int):
    """one frame, as ctc_beam_ref.step: -> (the new state, every finite item (total, kind, i, token) in order; None for a
    bad row)"""
    n, nbad, nn, ent, gs = state
    if row is None:
        return (n + 1, nbad + 1, nn, ent, gs), None
    r32, lse = row
    lp = lambda v: float(np.float64(r32[v]) - lse)   # noqa: E731
    lpb = lp(blank)
    cand = {}
    for g in gs:
        if g not in cand:
            cand[g] = candidates(gr, g, r32, C)
    tot = [R.lae(e[4], e[5]) for e in ent]
    pb2 = [tot[i] + lpb for i in range(len(ent))]
    pnb2 = [e[5] + lp(e[1]) if e[1] >= 0 else NEG for e in ent]
    fresh = []
    for i, e in enumerate(ent):
        for c, nxt in cand[gs[i]]:
            ext = (e[4] if c == e[1] else tot[i]) + lp(c)
            js = [j for j, f in enumerate(ent) if f[3] == e[0] and f[1] == c]
            assert len(js) <= 1
            if js:
                pnb2[js[0]] = R.lae(pnb2[js[0]], ext)
                assert gs[js[0]] == nxt, (i, c, nxt, gs[js[0]])      # the same prefix has the same state
            else:
                fresh.append((ext, 1, i, c, nxt))
    items = [(R.lae(pb2[i], pnb2[i]), 0, i, -1, gs[i]) for i in range(len(ent))] + fresh
    items = sorted((it for it in items if it[0] > NEG), key=lambda it: (-it[0], it[1], it[2], it[3]))
    new, ngs = [], []
    for total, kind, i, c, g2 in items[:B]:
        e = ent[i]
        if kind == 0:
            new.append((e[0], e[1], e[2], e[3], pb2[i], pnb2[i]))
        else:
            if nn < capacity:
                assert len(store) == nn
                store.append((e[0], c, n))
            new.append((nn, c, e[2] + 1, e[0], NEG, total))
            nn += 1
        ngs.append(g2)
    return (n + 1, nbad, nn, new, ngs), [it[:4] for it in items]


def scan(state, rws, store: list, capacity: int, B: int, C: int, gr, blank: int, gaps: list = None):
    """state + a span of rows() -> the new state.  ``gaps``: as ctc_beam_ref.scan"""
    n, nbad, nn, ent, gs = state
    state = (n, nbad, nn, list(ent[:B]), list(gs[:B]))
    if nn >= 1 and not store and capacity > 0:
        store.append(R.ROOT)
    for row in rws:
        state, items = step(state, row, store, capacity, B, C, gr, blank)
        if gaps is not None and items is not None:
            tots = [it[0] for it in items[:B + 1]]
            gaps.extend(a - b for a, b in zip(tots[:-1], tots[1:]))
    return state


def scan_table(table, blank: int, B: int, C: int, gr, state=None, store=None, capacity: int = 1 << 30, gaps: list = None):
    """(state after the rows of ``table``, the node store)"""
    store = [] if store is None else store
    return scan(initial(gr) if state is None else state, rows(table), store, capacity, B, C, gr, blank, gaps), store
