"""Contract of the CTC draft transcript (csrc/draft.hip, sc_ctc_draft), numpy float64.

Per row x[0..V) of the fp32 CTC table and the blank id b:
    a row that holds a NaN or +inf, or nothing but -inf, is a BAD frame (the rule of ctc_activity_ref / ctc_spot_ref);
    else k = argmax_v x[v] on the fp32 values, the LOWEST index among ties, and
    p = exp(x[k] - lse) with x promoted to float64, m = max_v x[v], lse = m + log(sum_v exp(x[v] - m)) (v ascending) -
    the formula of ctc_activity_ref.p_blank taken as written (logits around 1e30 give p = 1).
A per-row constant cancels: raw logits and log-softmaxed rows give the same labels unless fp32 rounding creates a tie.

Greedy collapse.  Frames are numbered in the order they are scanned.  State of a stream over its utterance:
    n_frames, n_closed, n_bad, open_id, open_start, open_end (int32; -1: no open token), open_conf (float64; 0.0: none)
For frame n:
    bad row or k == b    the open token, if any, is closed (a bad row also counts in n_bad)
    k == open_id         open_end = n, open_conf = max(open_conf, p)
    otherwise            the open token, if any, is closed; a new one opens: (k, n, n, p)
Closed = appended to the stream's token store at slot n_closed (counted, not written, at or beyond the capacity), then
n_closed += 1; a stored token is never touched again.  A token is (id, start, end, conf), frames both inclusive.  The
draft of a state is its stored tokens followed by the open token, if any.  scan(state, span) -> state; any split of a
table into consecutive spans (empty ones included) gives the state and store of the one-span scan.
"""
import numpy as np

import ctc_row_ref as row_ref

FIELDS = ("n_frames", "n_closed", "n_bad", "open_id", "open_start", "open_end", "open_conf")
INITIAL = (0, 0, 0, -1, -1, -1, 0.0)
BAD = -2   # label of a bad row


def rows(table, blank: int = 0):
    """(labels int32 [T]: the arg-max, BAD for a bad row; p float64 [T]: its posterior, NaN for a bad row) of the rows of
    table [T, V] fp32"""
    x32 = np.asarray(table, np.float32)
    T = x32.shape[0]
    lab, p = np.full(T, BAD, np.int32), np.full(T, np.nan)
    for t in range(T):
        r32 = x32[t]
        if row_ref.is_bad(r32):
            continue
        k = int(np.argmax(r32))   # the first of equal maxima
        lab[t] = k
        p[t] = np.exp(np.float64(r32[k]) - row_ref.lse(r32))
    return lab, p


def scan(state, lab, p, blank: int, store: list, capacity: int):
    """state (FIELDS order) + labels and posteriors of a span of further frames -> the new state; tokens that close are
    appended to ``store`` (a list of (id, start, end, conf)) while it holds fewer than ``capacity``"""
    n, nc, nbad, oid, ost, oen = (int(v) for v in state[:6])
    ocf = float(state[6])

    def close():
        nonlocal nc, oid, ost, oen, ocf
        if oid >= 0:
            if nc < capacity:
                assert len(store) == nc
                store.append((oid, ost, oen, ocf))
            nc += 1
            oid, ost, oen, ocf = -1, -1, -1, 0.0

    for k, q in zip(np.asarray(lab).tolist(), np.asarray(p, np.float64).tolist()):
        if k == BAD or k == blank:
            close()
            nbad += k == BAD
        elif k == oid:
            oen, ocf = n, max(ocf, q)
        else:
            close()
            oid, ost, oen, ocf = k, n, n, q
        n += 1
    return (n, nc, nbad, oid, ost, oen, ocf)


def scan_table(table, blank: int, state=INITIAL, store=None, capacity: int = 1 << 30):
    """(state after the rows of ``table``, the token store)"""
    store = [] if store is None else store
    lab, p = rows(table, blank)
    return scan(state, lab, p, blank, store, capacity), store


def draft(state, store):
    """the stored tokens followed by the open token, if any"""
    out = list(store)
    if int(state[3]) >= 0:
        out.append((int(state[3]), int(state[4]), int(state[5]), float(state[6])))
    return out


def as_dict(state):
    d = {k: int(v) for k, v in zip(FIELDS[:6], state)}
    d["open_conf"] = float(state[6])
    return d
