"""float32 numpy statement of the CTC forced-alignment contract (include/scasr.h, csrc/align.hip): the GPU kernel
must give the same status, the same path (token frames) and the same fp32 path score, bit for bit."""
import numpy as np

OK, INFEASIBLE, NONFINITE, BAD_INPUT = 0, 1, 2, 3
MAX_L = 1023


def state_labels(y, blank):
    """label of each of the 2L+1 states (blank, y0, blank, y1, ..., blank)"""
    lab = np.full(2 * len(y) + 1, blank, np.int64)
    lab[1::2] = y
    return lab


def skip_allowed(y):
    """state s may come from s-2: a label state whose label differs from the previous one"""
    S = 2 * len(y) + 1
    sk = np.zeros(S, bool)
    for i in range(1, len(y)):
        sk[2 * i + 1] = y[i] != y[i - 1]
    return sk


def status_of(e, y, blank):
    T, V = e.shape
    y = np.asarray(y, np.int64)
    L = len(y)
    if L > MAX_L or not 0 <= blank < V or np.any((y < 0) | (y >= V) | (y == blank)):
        return BAD_INPUT
    if not np.all(np.isfinite(e[:T])):
        return NONFINITE
    reps = int(np.sum(y[1:] == y[:-1])) if L > 1 else 0
    return INFEASIBLE if T < L + reps else OK


def viterbi(e, y, blank):
    """-> (status, path [T] of states, path_score float32).  e: float32 [T, V]."""
    e = np.asarray(e, np.float32)
    y = np.asarray(y, np.int64)
    st = status_of(e, y, blank)
    T = e.shape[0]
    if st != OK:
        return st, None, np.float32(-np.inf)
    if T == 0:
        return OK, np.zeros(0, np.int64), np.float32(0.0)
    S = 2 * len(y) + 1
    lab, sk = state_labels(y, blank), skip_allowed(y)
    ninf = np.float32(-np.inf)
    d = np.full(S, ninf, np.float32)
    d[0] = 0.0                                     # virtual frame -1: paths start in state 0 or 1
    bp = np.zeros((T, S), np.int8)
    for t in range(T):
        c1 = np.concatenate(([ninf], d[:-1]))
        c2 = np.concatenate(([ninf, ninf], d[:-2]))[:S]
        best = d.copy()
        ch = np.zeros(S, np.int8)
        m = c1 > best                               # later candidates take over only if strictly greater
        best[m], ch[m] = c1[m], 1
        m = sk & (c2 > best)
        best[m], ch[m] = c2[m], 2
        d = (best + e[t, lab]).astype(np.float32)   # one fp32 add per frame
        bp[t] = ch
    s = S - 1
    if S >= 2 and not d[S - 1] > d[S - 2]:
        s = S - 2
    score = d[s]
    path = np.zeros(T, np.int64)
    path[T - 1] = s
    for t in range(T - 1, 0, -1):
        s -= int(bp[t, s])
        path[t - 1] = s
    return OK, path, np.float32(score)


def spans(path, L):
    """token i occupies the frames of state 2i+1 -> start [L], end [L] (exclusive)"""
    start, end = np.full(L, -1, np.int64), np.full(L, -1, np.int64)
    for t, s in enumerate(path):
        if s & 1:
            i = s >> 1
            if start[i] < 0:
                start[i] = t
            end[i] = t + 1
    return start, end


def logsumexp_rows(e):
    e = np.asarray(e, np.float64)
    m = e.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(e - m).sum(axis=1, keepdims=True)))[:, 0]


def align(e, y, blank):
    """the whole contract: {"status", "start", "end", "logp_mean", "path_score"} (start / end / logp_mean None unless OK)"""
    e = np.asarray(e, np.float32)
    st, path, score = viterbi(e, y, blank)
    if st != OK:
        return {"status": st, "start": None, "end": None, "logp_mean": None, "path_score": score, "path": None}
    L = len(y)
    start, end = spans(path, L)
    lse = logsumexp_rows(e) if e.shape[0] else np.zeros(0)
    lp = np.array([np.mean(e[start[i]:end[i], y[i]].astype(np.float64) - lse[start[i]:end[i]]) for i in range(L)])
    return {"status": st, "start": start, "end": end, "logp_mean": lp, "path_score": score, "path": path}


def brute_force(e, y, blank):
    """every CTC path of the 2L+1 states -> (best fp32 score, the path the tie rule picks).  Tie rule (exact on tables
    whose sums are exact): among the best paths, the final state 2L-1 before 2L, then going back frame by frame the
    smallest step (stay, then s-1, then s-2)."""
    e = np.asarray(e, np.float32)
    T = e.shape[0]
    S = 2 * len(y) + 1
    lab, sk = state_labels(y, blank), skip_allowed(y)
    best = None

    def rec(t, s, acc, path):
        nonlocal best
        acc = np.float32(acc + e[t, lab[s]])
        path = path + [s]
        if t == T - 1:
            if s < S - 2:
                return
            steps = [path[k] - path[k - 1] for k in range(T - 1, 0, -1)]
            key = (-float(acc), 0 if s == S - 2 else 1, steps)
            if best is None or key < best[0]:
                best = (key, acc, list(path))
            return
        for c in (0, 1, 2):
            n = s + c
            if n >= S or (c == 2 and not sk[n]):
                continue
            rec(t + 1, n, acc, path)

    for s0 in (0, 1):
        if s0 < S:
            rec(0, s0, np.float32(0.0), [])
    if best is None:
        return None, None
    return best[1], np.array(best[2])
