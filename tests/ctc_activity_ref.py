"""Contract of the CTC speech-activity scan (csrc/activity.hip, sc_ctc_activity), numpy float64.

For a row x[0..V) of the fp32 CTC table, promoted to float64, and the blank id b:
    m = max_v x[v];  lse = m + log(sum_v exp(x[v] - m))  (v ascending);  p_blank = exp(x[b] - lse)
-inf entries contribute 0.  (The formula is taken as written: for logits beyond about 1e16 the term log(sum) is absorbed
when it is added to m, so rows that tie at such a maximum give exp(0) = 1 for each of the tied entries.)  A row that holds a NaN or +inf, or nothing but -inf, is a BAD frame: p_blank = NaN.
A frame is SILENCE iff it is bad or p_blank > thr, else SPEECH.

State of a stream over the frames scanned so far in its utterance (six int32):
    n_frames, n_speech, n_bad, first_speech, last_speech (-1: none), trail_silence
    trail_silence = n_frames - 1 - last_speech if last_speech >= 0 else n_frames
Frames are numbered in the order they are scanned.  scan(state, span) -> state; any split of a table into consecutive
spans (empty ones included) gives the states of the one-span scan.
"""
import numpy as np

import ctc_row_ref as row_ref

FIELDS = ("n_frames", "n_speech", "n_bad", "first_speech", "last_speech", "trail_silence")
INITIAL = (0, 0, 0, -1, -1, 0)


def p_blank(table, blank: int) -> np.ndarray:
    """[T] float64 blank posteriors of the rows of table [T, V] (any float dtype; promoted to float64)."""
    x = np.asarray(table).astype(np.float64)
    T = x.shape[0]
    out = np.full(T, np.nan)
    for t in range(T):
        row = x[t]
        if not row_ref.is_bad(row):
            out[t] = np.exp(row[blank] - row_ref.lse(row))
    return out


def silence(pb: np.ndarray, thr: float) -> np.ndarray:
    """bool [T]: bad (NaN) or p_blank > thr"""
    pb = np.asarray(pb, np.float64)
    bad = np.isnan(pb)
    with np.errstate(invalid="ignore"):
        return bad | (pb > thr)


def scan(state, pb: np.ndarray, thr: float):
    """state (six ints, FIELDS order) + the p_blank values of a span of further frames -> the new state"""
    n, nsp, nbad, first, last, _ = (int(v) for v in state)
    pb = np.asarray(pb, np.float64)
    k = pb.shape[0]
    if k:
        bad = np.isnan(pb)
        sp = ~silence(pb, thr)
        idx = np.nonzero(sp)[0]
        if idx.size:
            if first < 0:
                first = n + int(idx[0])
            last = n + int(idx[-1])
        nsp += int(sp.sum())
        nbad += int(bad.sum())
        n += k
    trail = n - 1 - last if last >= 0 else n
    return (n, nsp, nbad, first, last, trail)


def scan_table(table, blank: int, thr: float, state=INITIAL):
    """(state after the rows of `table`, their p_blank)"""
    pb = p_blank(table, blank)
    return scan(state, pb, thr), pb


def as_dict(state):
    return {k: int(v) for k, v in zip(FIELDS, state)}
