"""Acoustic speech activity from the CTC table: the host-side pieces shared by the engines.

A frame is silence iff its CTC row is bad (a NaN, a +inf, or nothing but -inf) or its blank posterior exceeds the
threshold.  The state of a stream over the frames scanned so far in its utterance is six integers, FIELDS."""
import numpy as np

FIELDS = ("n_frames", "n_speech", "n_bad", "first_speech", "last_speech", "trail_silence")
INITIAL = (0, 0, 0, -1, -1, 0)
FRAME_SECONDS = 0.04   # one encoder frame (subsampling 4 at a 10 ms hop)


def advance(state, p_blank, thr: float):
    """state (six ints, FIELDS order) + the float64 blank posteriors of a span of further frames -> the new state"""
    n, nsp, nbad, first, last, _ = (int(v) for v in state)
    for p in np.asarray(p_blank, np.float64):
        if p != p:
            nbad += 1
        elif not p > thr:
            nsp += 1
            if first < 0:
                first = n
            last = n
        n += 1
    return (n, nsp, nbad, first, last, n - 1 - last if last >= 0 else n)


def as_arrays(states):
    """a list of states -> {field: int32 array [n]}"""
    a = np.asarray(states, np.int32).reshape(-1, len(FIELDS))
    return {k: a[:, i].copy() for i, k in enumerate(FIELDS)}


def of_stream(act, i: int):
    """{field: int} of entry i of an ``activity()`` result"""
    return {k: int(act[k][i]) for k in FIELDS}
