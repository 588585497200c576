"""Contract of n-gram rescoring of n-best lists (csrc/lm_rescore.hip, sc_lm_rescore), numpy float64, built on
speechcatcher_amd.ngram.Blob.score - THE sequential walk of the automaton, the same score() and the same float64 addition
order as the fused beam of 8k (tests/ctc_beam_lm_ref.py).

A job is one list: n_hyp <= 16 rows of token ids, a total score per row, a per-row length lens[h] or one length L for all
rows, and
    skip      leading tokens that are no labels (1 for <sos>)
    strip     a token id or -1: ONE trailing token equal to it is no label (as sc_align_hyps drops a trailing <eos>)
    state0    the automaton's state before the first label; -1: the model's start_state
    lm_eos    the id that stands for </s> in the model; -1: no end term
    alpha, beta
Per row h, with the labels y_0 .. y_{m-1}:
    s_0 = state0;  (l_t, s_{t+1}) = score(s_t, y_t);  tok_lm[t] = l_t
    lm = ((0.0 + l_0) + l_1) + ...     ascending t (what an 8k beam entry carries)
    end_state = s_m
    eos_lm = score(s_m, lm_eos)[0], 0.0 without an end term
    lm_total = lm + eos_lm
    fused = score + (alpha * lm_total + beta * m)      every product and sum rounded on its own; a NaN is THE quiet NaN
    order[r] = the row at rank r: fused descending, ties to the lower row
A row whose score or fused is not finite carries NONFINITE in status[h]; a row with a label outside [0, V) - or with a
lens[h] outside [0, L] - carries BAD_TOKEN: lm = eos_lm = 0.0, every tok_lm 0.0, end_state -1, fused NaN.  Both kinds rank
behind all other rows, in row order among themselves.  SERIAL in a status says which path of the kernel walked the row; it
is no part of the contract's values.

``lm`` is anything with score(s, c) -> (logp, next), start_state, V and n_states (speechcatcher_amd.ngram.Blob)."""
import math

import numpy as np

NONFINITE, BAD_TOKEN, SERIAL = 1, 2, 4      # SC_RESCORE_* status bits
FORCE_SERIAL = 1                            # SC_RESCORE_FORCE_SERIAL (flags)
MAX_HYPS = 16
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]


def labels(row, length: int, skip: int, strip: int):
    a, e = skip, length
    if e > a and strip >= 0 and int(row[e - 1]) == strip:
        e -= 1
    return [int(v) for v in row[a:max(a, e)]]


def walk(lm, y, state0: int = -1):
    """the sequential walk: (tok_lm, lm, end_state)"""
    s = lm.start_state if state0 < 0 else state0
    tok, acc = [], 0.0
    for c in y:
        l, s = lm.score(s, c)
        tok.append(l)
        acc = float(acc + l)
    return tok, acc, s


def window_guess(lm, y, t: int, state0: int = -1):
    """phase A of the kernel: the state before label t from the last order - 1 labels alone (from state 0), or from
    state0 over all the labels before t when there are fewer than order - 1"""
    k = lm.order - 1
    if t < k:
        s, a = (lm.start_state if state0 < 0 else state0), 0
    else:
        s, a = 0, t - k
    for c in y[a:t]:
        s = lm.score(s, c)[1]
    return s


def fuse(score: float, alpha: float, beta: float, lm_total: float, m: int) -> float:
    with np.errstate(all="ignore"):
        f = float(np.float64(score) + (np.float64(alpha) * np.float64(lm_total) + np.float64(beta) * np.float64(m)))
    return float(QNAN) if math.isnan(f) else f


def rank(fused, status):
    """order[r]: the sound rows by fused descending (ties: the lower row), then the others in row order"""
    bad = [bool(s & (NONFINITE | BAD_TOKEN)) for s in status]
    return sorted(range(len(fused)), key=lambda h: (1, 0.0, h) if bad[h] else (0, -fused[h], h))


def rescore(lm, rows, scores, lens=None, L=None, skip=1, strip=-1, state0=-1, lm_eos=-1, alpha=0.0, beta=0.0):
    """-> dict: lm, eos_lm, fused (float64 [n]), end_state, order, status (int32 [n]), tok_lm (list of float64 arrays),
    m (label counts)"""
    n = len(rows)
    assert 1 <= n <= MAX_HYPS
    out = {k: np.zeros(n, np.float64) for k in ("lm", "eos_lm", "fused")}
    out.update({k: np.zeros(n, np.int32) for k in ("end_state", "status", "m")})
    out["tok_lm"] = []
    for h in range(n):
        length = int(L if lens is None else lens[h])
        sc = float(scores[h])
        ok = L is None or 0 <= length <= L
        y = labels(rows[h], length, skip, strip) if ok else []
        if not ok or any(not 0 <= c < lm.V for c in y):
            out["status"][h] = BAD_TOKEN | (0 if math.isfinite(sc) else NONFINITE)
            out["fused"][h], out["end_state"][h], out["m"][h] = QNAN, -1, len(y)
            out["tok_lm"].append(np.zeros(len(y), np.float64))
            continue
        tok, acc, s = walk(lm, y, state0)
        eos = lm.score(s, lm_eos)[0] if lm_eos >= 0 else 0.0
        f = fuse(sc, alpha, beta, float(acc + eos), len(y))
        out["lm"][h], out["eos_lm"][h], out["fused"][h], out["end_state"][h], out["m"][h] = acc, eos, f, s, len(y)
        out["status"][h] = 0 if math.isfinite(sc) and math.isfinite(f) else NONFINITE
        out["tok_lm"].append(np.asarray(tok, np.float64))
    out["order"] = np.asarray(rank(out["fused"].tolist(), out["status"].tolist()), np.int32)
    return out
