"""Contract of the CTC token alternates (csrc/alternates.hip, sc_ctc_alternates), numpy float64.

One job: a table x[T][V] of fp32 rows, the blank id b, L labels y[k], L spans [start[k], end[k]) (int32) and K with
1 <= K <= MAX_K.  Per span k, checked in this order:
    NO_SPAN (1)   start < 0, end <= start or end > T.  No row is read.
    BAD_ROW (2)   a row of the span is bad by the rule of ctc_activity_ref / ctc_spot_ref / ctc_draft_ref: a NaN or +inf,
                  or nothing but -inf.  Bad rows outside the span do not matter.
    OK (0)        S[v] = ((x[start][v] + x[start+1][v]) + ...), promoted to float64 and added in ascending frame order, for
                  every v (-inf entries give -inf; a NaN cannot arise because bad rows are excluded).  Only float64 adds of
                  promoted fp32 values occur: any implementation that adds in this order has the same bits.
                  Candidates: every v in [0, V) with v != b, ordered by S descending, then v ascending.
                  alt_ids[k][j]  the j-th candidate for j < min(K, V - 1), -1 behind them
                  alt_logp[k][j] (S[v] - sum_t lse_t) / (end - start), lse_t = m + log(sum_v exp(x[v] - m)) - the formula
                                 of ctc_activity_ref taken as written, v ascending - summed in frame order; -inf in the
                                 unused slots
                  own_rank[k]    the candidates strictly ahead of y[k] in that order (0: the token is the acoustic best of
                                 its own frames); -1 when y[k] is outside [0, V) or equals b - the rest of the span is
                                 still computed
On a status other than OK: ids -1, logp -inf, own_rank -1.  Outputs past L are never written.
A per-row constant cancels inside a span: raw logits and rows log-softmaxed in place give the same order, except where fp32
rounding creates ties.
"""
import numpy as np

from ctc_row_ref import is_bad as row_is_bad, lse as row_lse   # (fp32 rows)

OK, NO_SPAN, BAD_ROW = 0, 1, 2
MAX_K = 8


def span_sums(x32, start: int, end: int) -> np.ndarray:
    """S[v] over the rows [start, end): float64 adds of the promoted fp32 values in ascending frame order"""
    S = x32[start].astype(np.float64)
    for t in range(start + 1, end):
        S = S + x32[t].astype(np.float64)
    return S


def order(S, blank: int) -> np.ndarray:
    """the candidates (every v but the blank) by S descending, then v ascending"""
    V = S.shape[0]
    cand = np.array([v for v in range(V) if v != blank], np.int64)
    if cand.size == 0:
        return cand
    # a stable sort of -S keeps v ascending among equal sums (-inf sums included: -(-inf) = +inf sorts last)
    return cand[np.argsort(-S[cand], kind="stable")]


def alternates(table, blank: int, labels, start, end, K: int):
    """-> (alt_ids int32 [L, K], alt_logp float64 [L, K], own_rank int32 [L], status int32 [L])"""
    assert 1 <= K <= MAX_K
    x32 = np.asarray(table, np.float32)
    T, V = x32.shape
    labels, start, end = (np.asarray(a, np.int64).reshape(-1) for a in (labels, start, end))
    L = labels.shape[0]
    assert start.shape[0] == L and end.shape[0] == L
    ids = np.full((L, K), -1, np.int32)
    logp = np.full((L, K), -np.inf, np.float64)
    rank = np.full(L, -1, np.int32)
    status = np.zeros(L, np.int32)
    for k in range(L):
        a, e = int(start[k]), int(end[k])
        if a < 0 or e <= a or e > T:
            status[k] = NO_SPAN
            continue
        if any(row_is_bad(x32[t]) for t in range(a, e)):
            status[k] = BAD_ROW
            continue
        S = span_sums(x32, a, e)
        lse = 0.0
        for t in range(a, e):
            lse = lse + row_lse(x32[t])
        o = order(S, blank)
        n = min(K, o.shape[0])
        ids[k, :n] = o[:n]
        logp[k, :n] = (S[o[:n]] - lse) / float(e - a)
        y = int(labels[k])
        if 0 <= y < V and y != blank:
            rank[k] = int(np.nonzero(o == y)[0][0])
    return ids, logp, rank, status
