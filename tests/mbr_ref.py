"""Contract of consensus finals (csrc/mbr.hip, sc_mbr), numpy float64: the minimum-Bayes-risk row of an
n-best list under the edit distance, and a pivot-based confusion network with the list's mass per slot.

A job is one list: n_hyp <= 16 rows of token ids with a per-row length lens[h] or one length L for all rows, ``skip``
leading tokens that are no labels, ONE trailing token equal to ``strip`` (-1: none) that is no label either - the
layout of tests/lm_rescore_ref.py - and per row a ``weight`` or a ``score``.  The labels of row h are y_h[0 .. m_h).

    status[h]   BAD_TOKEN   a label outside [0, V), or a lens[h] outside [0, L]
                TOO_LONG    m_h > MAX_LEN
                NONFINITE   a weight that is NaN, infinite or negative; a score that is NaN or +inf, or whose scaled
                            value z_h (below) is (-inf is a legal score: its weight is 0)
                a row with any of these is OUT: dist -1 in its row and column, risk THE quiet NaN, weight 0.0
                NO_PIVOT    on every row when the list has no pivot (below)
    w[h]        ``weight`` given: the values themselves.  Otherwise over the rows that are in
                z_h = scale * score[h] (-inf for a score of -inf, whatever the scale), M = max z, e_h = exp(z_h - M),
                Z = ((0 + e_0) + e_1) + ... ascending, w_h = e_h / Z; M = -inf: w_h = 1 / n_in
    dist[h][j]  Levenshtein distance of y_h and y_j, unit costs
    risk[h]     ((0.0 + w_0 dist[h][0]) + w_1 dist[h][1]) + ... ascending j over the rows that are in, every product and
                sum rounded on its own
    order[r]    rows by ascending risk, ties to the lower row, rows that are out last in row order
    header      {P, m_P, n_in, 0}: P = order[0] (pivot = -1) or the named row; P = -1, m_P = 0 when no row is in or the
                named row is out
    slots[j][t] row j (in) aligned against the pivot: D the full table of (y_P, y_j), walked back from (m_P, m_j) -
                diagonal if i > 0 and j > 0 and D[i][j] == D[i-1][j-1] + (y_P[i-1] != y_j[j-1]): slot i-1 <- y_j[j-1];
                otherwise up if i > 0 and D[i][j] == D[i-1][j] + 1: slot i-1 <- -1 (epsilon); otherwise left: row j has
                an insertion in gap i (the gap before the pivot's position i; gap m_P is the end).  A row that is out has
                -2 in every slot.
    conf[t]     sum over j ascending (rows in) of w_j where slots[j][t] == y_P[t]
    alt_tok[t], alt_mass[t]  among the symbols other than y_P[t] in column t (rows in; a token id or -1) the one with the
                largest mass - the same kind of sum -, ties to the lower symbol; -2 and 0.0 when there is none
    gap_mass[g] g in [0, m_P]: the mass of the rows (in) with at least one insertion in gap g

The distances are computed in the row-scan form the kernel uses (dist_rowscan: the in-row dependency as a prefix
minimum); a full table is built only for the backtraces."""
import math

import numpy as np

NONFINITE, BAD_TOKEN, TOO_LONG, NO_PIVOT = 1, 2, 4, 8      # SC_MBR_* status bits
OUT = NONFINITE | BAD_TOKEN | TOO_LONG
MAX_HYPS, MAX_LEN = 16, 1024
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]
_BIG = 1 << 28


def labels(row, length: int, skip: int, strip: int):
    a, e = skip, length
    if e > a and strip >= 0 and int(row[e - 1]) == strip:
        e -= 1
    return np.asarray(row[a:max(a, e)], np.int64)


def table_plain(a, b):
    """the textbook table, cell by cell (what the row-scan form is checked against)"""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return np.asarray(D, np.int64).reshape(len(a) + 1, len(b) + 1)


def _next_row(prev, i, ai, b, idx):
    t = prev + 1
    if len(b):
        t[1:] = np.minimum(t[1:], prev[:-1] + (b != ai))
    t[0] = i
    return idx + np.minimum.accumulate(t - idx)


def table_rowscan(a, b):
    """every row of the table from the one before: t[j] = min(prev[j] + 1, prev[j-1] + cost), cur[j] = j + min_{k<=j} (t[k] - k)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    D = np.empty((len(a) + 1, len(b) + 1), np.int64)
    D[0] = idx
    for i in range(1, len(a) + 1):
        D[i] = _next_row(D[i - 1], i, a[i - 1], b, idx)
    return D


def dist_rowscan(a, b) -> int:
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    cur = idx
    for i in range(1, len(a) + 1):
        cur = _next_row(cur, i, a[i - 1], b, idx)
    return int(cur[-1])


def backtrace(p, y, D=None):
    """-> (slots [m_P], gaps: the gap of every insertion in walk order) of row y against the pivot p"""
    D = table_rowscan(p, y) if D is None else D
    i, j = len(p), len(y)
    slots, gaps = np.full(len(p), -2, np.int64), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (p[i - 1] != y[j - 1]):
            slots[i - 1] = y[j - 1]
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            slots[i - 1] = -1
            i -= 1
        else:
            gaps.append(i)
            j -= 1
    return slots, gaps


def weights_of(scores, scale, inn):
    """the scaled softmax over the rows that are in"""
    w = np.zeros(len(scores), np.float64)
    if not inn:
        return w
    with np.errstate(all="ignore"):
        z = {h: (-math.inf if scores[h] == -math.inf else float(np.float64(scale) * np.float64(scores[h]))) for h in inn}
    M = max(z.values())
    if M == -math.inf:
        for h in inn:
            w[h] = float(np.float64(1.0) / np.float64(len(inn)))
        return w
    e = {h: float(np.exp(np.float64(z[h] - M))) for h in inn}
    Z = 0.0
    for h in inn:
        Z = float(Z + e[h])
    for h in inn:
        w[h] = float(np.float64(e[h]) / np.float64(Z))
    return w


def mass_sum(w, rows):
    acc = 0.0
    for j in rows:        # ascending
        acc = float(acc + w[j])
    return acc


def mbr(rows, weight=None, score=None, lens=None, L=None, skip=0, strip=-1, V=1 << 30, scale=1.0, pivot=-1, max_len=MAX_LEN, memo=None):
    """-> dict: status, order (int32 [n]), weight, risk (float64 [n]), dist (int32 [16][16], -7 where nothing is written),
    header (int32 [4]), slots (int32 [n][m_P]), conf, alt_mass (float64 [m_P]), alt_tok (int32 [m_P]), gap_mass (float64
    [m_P + 1]; empty without a pivot), y (the label arrays), ins (per row the gaps of its insertions).  ``memo``: a dict
    that remembers distances by the rows' labels (two evaluations of one list share them)"""
    n = len(rows)
    assert 1 <= n <= MAX_HYPS and (weight is None) != (score is None) and -1 <= pivot < n
    assert math.isfinite(scale) and scale >= 0
    ys, status = [], np.zeros(n, np.int32)
    for h in range(n):
        length = int(L if lens is None else lens[h])
        ok = L is None or 0 <= length <= L
        y = labels(rows[h], length, skip, strip) if ok else np.zeros(0, np.int64)
        if not ok or np.any((y < 0) | (y >= V)):
            status[h] |= BAD_TOKEN
        if len(y) > max_len:
            status[h] |= TOO_LONG
        if weight is not None:
            v = float(weight[h])
            if not math.isfinite(v) or v < 0:
                status[h] |= NONFINITE
        else:
            v = float(score[h])
            with np.errstate(all="ignore"):
                z = -math.inf if v == -math.inf else float(np.float64(scale) * np.float64(v))
            if math.isnan(v) or v == math.inf or math.isnan(z) or z == math.inf:
                status[h] |= NONFINITE
        ys.append(y)
    inn = [h for h in range(n) if not status[h] & OUT]
    if weight is not None:
        w = np.asarray([float(weight[h]) if h in inn else 0.0 for h in range(n)], np.float64)
    else:
        w = weights_of([float(s) for s in score], scale, inn)
    dist = np.full((MAX_HYPS, MAX_HYPS), -7, np.int32)
    dist[:n, :n] = -1
    for a, h in enumerate(inn):
        dist[h, h] = 0
        for g in inn[a + 1:]:
            key = (ys[h].tobytes(), ys[g].tobytes())
            if memo is None or key not in memo:
                d = dist_rowscan(ys[h], ys[g])
                if memo is not None:
                    memo[key] = d
            dist[h, g] = dist[g, h] = d if memo is None else memo[key]
    risk = np.full(n, QNAN, np.float64)
    for h in inn:
        acc = 0.0
        for j in inn:
            acc = float(acc + float(np.float64(w[j]) * np.float64(dist[h, j])))
        risk[h] = acc
    order = sorted(inn, key=lambda h: (risk[h], h)) + [h for h in range(n) if h not in inn]
    P = -1
    if inn:
        P = order[0] if pivot < 0 else (pivot if pivot in inn else -1)
    if P < 0:
        status |= NO_PIVOT
    mP = len(ys[P]) if P >= 0 else 0
    out = {"status": status, "order": np.asarray(order, np.int32), "weight": w, "risk": risk, "dist": dist,
           "header": np.asarray([P, mP, len(inn), 0], np.int32), "y": ys, "n_in": len(inn), "P": P,
           "slots": np.full((n, mP), -2, np.int32), "ins": [[] for _ in range(n)],
           "conf": np.zeros(mP, np.float64), "alt_mass": np.zeros(mP, np.float64), "alt_tok": np.full(mP, -2, np.int32),
           "gap_mass": np.zeros(mP + 1 if P >= 0 else 0, np.float64)}
    if P < 0:
        return out
    p = ys[P]
    for j in inn:
        s, gaps = backtrace(p, ys[j])
        out["slots"][j] = s
        out["ins"][j] = gaps
    for t in range(mP):
        col = {}
        for j in inn:
            col.setdefault(int(out["slots"][j, t]), []).append(j)
        out["conf"][t] = mass_sum(w, col.get(int(p[t]), []))
        best = None
        for sym in sorted(col):
            if sym == int(p[t]):
                continue
            m = mass_sum(w, col[sym])
            if best is None or m > best[1]:
                best = (sym, m)
        if best is not None:
            out["alt_tok"][t], out["alt_mass"][t] = best
    for g in range(mP + 1):
        out["gap_mass"][g] = mass_sum(w, [j for j in inn if g in out["ins"][j]])
    return out


def family(rng, n, length, V, rate=0.15):
    """n rows as mutated copies of one base row of ``length`` labels: substitutions, deletions and insertions at ``rate``"""
    base = rng.integers(0, V, length)
    rows = []
    for _ in range(n):
        y = []
        for c in base:
            r = rng.random()
            if r < rate / 3:
                continue
            if r < 2 * rate / 3:
                y.append(int(rng.integers(0, V)))
                continue
            y.append(int(c))
            if r > 1 - rate / 3:
                y.append(int(rng.integers(0, V)))
        rows.append(np.asarray(y, np.int64))
    return rows
