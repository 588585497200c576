"""Contract of the CTC phrase-spotting scan (csrc/spot.hip, sc_ctc_spot), numpy float64.

A phrase set holds P <= 64 phrases; phrase p is a label sequence y[0..L), 1 <= L <= 32, labels in [0, V) and not the
blank, with a floor min_score <= 0.  A phrase has S = 2L - 1 states: state 2i is token y[i], state 2i + 1 the blank
between y[i] and y[i + 1].  Each state holds a float64 value and an int32 start; -inf / -1 at the start of an utterance
(and in the unused entries [S, 64) of the state block, always).

For frame n (numbered in the order the frames are scanned) with row x of the fp32 table, promoted to float64:
  * the row is BAD if it holds a NaN or +inf, or nothing but -inf: every state of every enabled phrase becomes
    -inf / -1, nothing fires;
  * else m = max_v x[v], e(s) = x[label(s)] - m, and for every state s, from the values of the PREVIOUS frame, the
    candidates are compared in this order, a later one taking over only if it is strictly greater:
        1. stay V[s];  2. V[s-1] (s >= 1);  3. V[s-2] (s even, s >= 2, y[s/2] != y[s/2-1]);
        4. s == 0 only: a fresh start, value 0.0, start n
    new V[s] = best + e(s), new start = the winner's start (-1 when the new value is -inf).
  * with E = 2L - 2: the phrase fires iff the new V[E] >= min_score; event (end = n, phrase = p, start = start[E],
    score = V[E]); then all states of that phrase become -inf / -1.
Events of a stream are ordered by (end, phrase); the first MAX_EVENTS of an utterance are stored, n_events counts all.
A 64-bit mask enables phrases; a disabled phrase's states are not touched.
scan(state, span) -> state; any split of a table into consecutive spans (empty ones included) gives the states and
events of the one-span scan.
"""
import numpy as np

from ctc_row_ref import is_bad

MAX_EVENTS = 64
MAX_PHRASES = 64
MAX_LEN = 32
N_STATES = 64          # entries per phrase in the state block (2 * MAX_LEN - 1 used at most)
ALL = (1 << 64) - 1


def initial(P: int):
    return {"n_frames": 0, "n_events": 0, "values": np.full((P, N_STATES), -np.inf, np.float64),
            "starts": np.full((P, N_STATES), -1, np.int32), "events": []}


def copy_state(st):
    return {"n_frames": st["n_frames"], "n_events": st["n_events"], "values": st["values"].copy(),
            "starts": st["starts"].copy(), "events": list(st["events"])}


def check_phrases(phrases, floors, V: int, blank: int):
    assert 1 <= len(phrases) <= MAX_PHRASES and len(floors) == len(phrases)
    for y, f in zip(phrases, floors):
        assert 1 <= len(y) <= MAX_LEN and all(0 <= int(t) < V and int(t) != blank for t in y)
        assert f <= 0


def scan(state, table, blank: int, phrases, floors, mask: int = ALL):
    """state + the rows [T, V] of a span of further frames -> the new state (the argument is left unchanged)"""
    x = np.asarray(table).astype(np.float64)
    st = copy_state(state)
    P = len(phrases)
    NEG = -np.inf
    for t in range(x.shape[0]):
        row, n = x[t], st["n_frames"]
        bad = is_bad(row)
        m = None if bad else row.max()
        for p in range(P):                      # phrase ascending: the events of one frame are ordered by phrase
            if not (mask >> p) & 1:
                continue
            y = [int(v) for v in phrases[p]]
            L = len(y)
            S, E = 2 * L - 1, 2 * L - 2
            Vv, stt = st["values"][p], st["starts"][p]
            if bad:
                Vv[:S], stt[:S] = NEG, -1
                continue
            nv, ns = np.full(S, NEG), np.full(S, -1, np.int32)
            for s in range(S):
                best, bs = Vv[s], stt[s]
                if s >= 1 and Vv[s - 1] > best:
                    best, bs = Vv[s - 1], stt[s - 1]
                if s % 2 == 0 and s >= 2 and y[s // 2] != y[s // 2 - 1] and Vv[s - 2] > best:
                    best, bs = Vv[s - 2], stt[s - 2]
                if s == 0 and 0.0 > best:
                    best, bs = 0.0, n
                lab = y[s // 2] if s % 2 == 0 else blank
                v = best + (row[lab] - m)
                nv[s], ns[s] = v, (-1 if v == NEG else bs)
            if nv[E] >= floors[p]:
                if st["n_events"] < MAX_EVENTS:
                    st["events"].append((n, p, int(ns[E]), float(nv[E])))
                st["n_events"] += 1
                nv[:], ns[:] = NEG, -1
            Vv[:S], stt[:S] = nv, ns
        st["n_frames"] = n + 1
    return st


def same(a, b) -> bool:
    """bit-for-bit equality of two states (counters, values, starts, stored events)"""
    return (a["n_frames"] == b["n_frames"] and a["n_events"] == b["n_events"]
            and a["values"].tobytes() == b["values"].tobytes() and a["starts"].tobytes() == b["starts"].tobytes()
            and events_bytes(a["events"]) == events_bytes(b["events"]))


def events_bytes(events) -> bytes:
    return b"".join(np.asarray(e[:3], np.int32).tobytes() + np.float64(e[3]).tobytes() for e in events)


def collapse(path, blank: int):
    """the CTC collapse of an arg-max path: repeats merged, blanks dropped -> [(label, first frame, last frame)]"""
    out, prev = [], None
    for t, v in enumerate(int(v) for v in path):
        if v != prev and v != blank:
            out.append([v, t, t])
        elif v == prev and v != blank:
            out[-1][2] = t
        prev = v
    return [tuple(o) for o in out]
