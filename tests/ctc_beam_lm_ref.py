"""Contract of the CTC prefix beam search with an n-gram language model fused in (csrc/ctc_beam.hip, sc_ctc_beam_lm;
DESIGN.md 8k), numpy float64, built ON tests/ctc_beam_ref.py: its rows, candidates, stays, extensions and merges are that
contract's, and pb / pnb stay the pure CTC prefix probabilities.

State: ctc_beam_ref's (n_frames, n_bad, n_nodes, entries) and, beside entry i, side[i] = (lm_i, ctx_i): the raw sum of the
model's score() values along the entry's prefix and the automaton's state after it.  The initial entry has
(0.0, start_state).
    a new prefix made from entry i by candidate c:  (l, s') = score(ctx_i, c);  lm = lm_i + l;  ctx = s'
    a stay keeps (lm, ctx); an extension that merges into an entry of the beam leaves that entry's alone - the same
    prefix has the same values (asserted here)
    keep the B best by fused = total + w,  w = alpha * lm + beta * len, each product and sum rounded on its own; those
    whose total is -inf dropped; order: fused descending, then ctc_beam_ref's (stays first, lower rank, lower token)
The candidates are the C best by their fp32 acoustic values: the model does not choose them.  alpha = beta = 0 gives every
bit of ctc_beam_ref.  ``lm`` is anything with score(s, c) -> (logp, next) and start_state (speechcatcher_amd.ngram.Blob).
"""
import ctc_beam_ref as R

NEG = R.NEG


def initial(lm):
    return R.initial() + ([(0.0, int(lm.start_state))],)


def weight(alpha: float, beta: float, lm_sum: float, length: int) -> float:
    return float(float(alpha * lm_sum) + float(beta * float(length)))


def step(state, row, store: list, capacity: int, B: int, lm, alpha: float, beta: float):
    """one frame, as ctc_beam_ref.step: -> (the new state, every finite item (fused, kind, i, token) in order; None for a
    bad row)"""
    n, nbad, nn, ent, side = state
    if row is None:
        return (n + 1, nbad + 1, nn, ent, side), None
    cand, lpc, lpb = row
    lp = dict(zip(cand, lpc))
    tot = [R.lae(e[4], e[5]) for e in ent]
    pb2 = [tot[i] + lpb for i in range(len(ent))]
    pnb2 = [e[5] + lp[e[1]] if e[1] in lp else NEG for e in ent]
    fresh = []
    for i, e in enumerate(ent):
        for c in cand:
            ext = (e[4] if c == e[1] else tot[i]) + lp[c]
            js = [j for j, f in enumerate(ent) if f[3] == e[0] and f[1] == c]
            assert len(js) <= 1
            if js:
                pnb2[js[0]] = R.lae(pnb2[js[0]], ext)
                l, s2 = lm.score(side[i][1], c)                      # the same prefix has the same values
                assert (float(side[i][0] + l), s2) == side[js[0]], (side[i], c, side[js[0]])
            else:
                fresh.append((ext, 1, i, c))
    items = []
    for i, e in enumerate(ent):
        t = R.lae(pb2[i], pnb2[i])
        items.append((float(t + weight(alpha, beta, side[i][0], e[2])), 0, i, -1, t, side[i]))
    for ext, _, i, c in fresh:
        if ext > NEG:
            l, s2 = lm.score(side[i][1], c)
            lm2 = float(side[i][0] + l)
            items.append((float(ext + weight(alpha, beta, lm2, ent[i][2] + 1)), 1, i, c, ext, (lm2, s2)))
    items = sorted((it for it in items if it[4] > NEG), key=lambda it: (-it[0], it[1], it[2], it[3]))
    new, nside = [], []
    for fused, kind, i, c, t, sd in items[:B]:
        e = ent[i]
        if kind == 0:
            new.append((e[0], e[1], e[2], e[3], pb2[i], pnb2[i]))
        else:
            if nn < capacity:
                assert len(store) == nn
                store.append((e[0], c, n))
            new.append((nn, c, e[2] + 1, e[0], NEG, t))
            nn += 1
        nside.append(sd)
    return (n + 1, nbad, nn, new, nside), [it[:4] for it in items]


def scan(state, rws, store: list, capacity: int, B: int, lm, alpha: float, beta: float, gaps: list = None):
    """state + a span of ctc_beam_ref.rows() -> the new state.  ``gaps``: if a list, every gap between consecutive kept
    FUSED totals and between the B-th and the (B+1)-th of every frame is appended."""
    n, nbad, nn, ent, side = state
    state = (n, nbad, nn, list(ent[:B]), list(side[:B]))
    if nn >= 1 and not store and capacity > 0:
        store.append(R.ROOT)
    for row in rws:
        state, items = step(state, row, store, capacity, B, lm, alpha, beta)
        if gaps is not None and items is not None:
            f = [it[0] for it in items[:B + 1]]
            gaps.extend(a - b for a, b in zip(f[:-1], f[1:]))
    return state


def scan_table(table, blank: int, B: int, C: int, lm, alpha: float, beta: float, state=None, store=None,
               capacity: int = 1 << 30, gaps: list = None):
    """(state after the rows of ``table``, the node store)"""
    store = [] if store is None else store
    return scan(initial(lm) if state is None else state, R.rows(table, blank, C), store, capacity, B, lm, alpha, beta,
                gaps), store


def fused(entry, side, alpha: float, beta: float) -> float:
    return float(R.total(entry) + weight(alpha, beta, side[0], entry[2]))
