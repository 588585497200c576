"""Phrase spotting from the CTC table: the host-side pieces shared by the engines.

A phrase is a sequence of 1..32 token ids (no blank) with a floor ``min_score`` <= 0.  Every CTC frame advances, per
phrase, a best-path recurrence over the phrase's 2L - 1 states (tokens and the blanks between them) whose score is the
log-ratio of the phrase's path to the frame-wise best path; when the end state reaches the floor the phrase FIRES - an
event (phrase, start frame, end frame, score) - and re-arms.  Nothing here touches the search.  ``advance`` is the
recurrence of the Python engine (numpy float64, the same operations in the same order as csrc/spot.hip)."""
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import ctc_rows

MAX_PHRASES = 64
MAX_LEN = 32
N_STATES = 64
MAX_EVENTS = 64
ALL = (1 << 64) - 1
EVENT_FIELDS = ("phrase", "start", "end", "score")   # frames of 0.04 s, numbered from the utterance's first frame
SCORE_PER_TOKEN = -2.0   # default floor: two nats per token below the frame-wise best path (not tuned: DESIGN.md 8e)


def default_min_score(length: int) -> float:
    return SCORE_PER_TOKEN * int(length)


def phrase_ids(text: str, token_list: Sequence[str], space: str = "▁") -> List[int]:
    """Greedy longest-match tokenisation of ``text`` against ``token_list`` (sentencepiece-style pieces: a word starts
    with ``space``).  A convenience - a real tokenizer may cut differently; callers may pass ids directly, and several
    id sequences may stand for one phrase.  Raises ValueError where no piece matches."""
    s = "".join(space + w for w in text.split())
    index = {t: i for i, t in enumerate(token_list)}
    longest = max((len(t) for t in token_list), default=0)
    out, i = [], 0
    while i < len(s):
        for n in range(min(longest, len(s) - i), 0, -1):
            j = index.get(s[i:i + n])
            if j is not None:
                out.append(j)
                i += n
                break
        else:
            raise ValueError(f"no token matches {s[i:]!r}")
    return out


class PhraseSet:
    """labels [P, 32] int32 (unused entries 0), lens [P] int32, floors [P] float64 - the arrays of sc_streams_set_phrases"""

    def __init__(self, phrases: Sequence[Sequence[int]], min_scores: Optional[Sequence[float]] = None,
                 vocab_size: Optional[int] = None, blank: int = 0):
        P = len(phrases)
        if not 1 <= P <= MAX_PHRASES:
            raise ValueError(f"a phrase set holds 1..{MAX_PHRASES} phrases")
        if min_scores is None:
            min_scores = [default_min_score(len(y)) for y in phrases]
        if len(min_scores) != P:
            raise ValueError("one min_score per phrase")
        self.labels = np.zeros((P, MAX_LEN), np.int32)
        self.lens = np.zeros(P, np.int32)
        self.floors = np.asarray(min_scores, np.float64).copy()
        for p, y in enumerate(phrases):
            y = [int(t) for t in y]
            if not 1 <= len(y) <= MAX_LEN:
                raise ValueError(f"phrase {p}: 1..{MAX_LEN} tokens")
            if any(t == blank or t < 0 or (vocab_size is not None and t >= vocab_size) for t in y):
                raise ValueError(f"phrase {p}: a label outside the vocabulary or equal to the blank")
            if not self.floors[p] <= 0:
                raise ValueError(f"phrase {p}: min_score must be <= 0")
            self.labels[p, :len(y)] = y
            self.lens[p] = len(y)
        self.P = P
        # per phrase and state: the label whose emission the state takes (-1: the blank), and whether the skip is allowed
        s = np.arange(N_STATES)
        self.state_label = np.where(s % 2 == 0, self.labels[:, np.minimum(s // 2, MAX_LEN - 1)], -1)
        prev = self.labels[:, np.maximum(np.minimum(s // 2, MAX_LEN - 1) - 1, 0)]
        self.skip = (s % 2 == 0) & (s >= 2) & (self.labels[:, np.minimum(s // 2, MAX_LEN - 1)] != prev)
        self.used = s[None, :] < (2 * self.lens[:, None] - 1)

    def phrases(self) -> List[List[int]]:
        return [self.labels[p, :self.lens[p]].tolist() for p in range(self.P)]


def initial(P: int) -> dict:
    return {"n_frames": 0, "n_events": 0, "values": np.full((P, N_STATES), -np.inf, np.float64),
            "starts": np.full((P, N_STATES), -1, np.int32), "events": []}


def advance(state: dict, rows, blank: int, ps: PhraseSet, mask: int = ALL) -> dict:
    """state + the fp32 CTC rows [T, V] of a span of further frames -> the new state (in place, returned)"""
    x = np.asarray(rows).astype(np.float64)
    NEG = -np.inf
    on = np.asarray([(int(mask) >> p) & 1 for p in range(ps.P)], bool)
    used = ps.used & on[:, None]
    lab = np.where(ps.state_label < 0, blank, ps.state_label)
    E = 2 * ps.lens - 2
    pr = np.arange(ps.P)
    Vv, St = state["values"], state["starts"]
    for t in range(x.shape[0]):
        row, n = x[t], state["n_frames"]
        state["n_frames"] = n + 1
        if ctc_rows.is_bad(row):
            Vv[used], St[used] = NEG, -1
            continue
        e = row[lab] - row.max()
        best, bs = Vv.copy(), St.copy()
        up1, us1 = np.full_like(Vv, NEG), np.full_like(St, -1)
        up1[:, 1:], us1[:, 1:] = Vv[:, :-1], St[:, :-1]
        w = up1 > best
        best[w], bs[w] = up1[w], us1[w]
        up2, us2 = np.full_like(Vv, NEG), np.full_like(St, -1)
        up2[:, 2:], us2[:, 2:] = Vv[:, :-2], St[:, :-2]
        w = ps.skip & (up2 > best)
        best[w], bs[w] = up2[w], us2[w]
        w = 0.0 > best[:, 0]
        best[w, 0], bs[w, 0] = 0.0, n
        nv = best + e
        ns = np.where(nv == NEG, -1, bs).astype(np.int32)
        fv, fs = nv[pr, E], ns[pr, E]
        fire = on & (fv >= ps.floors)
        for p in np.nonzero(fire)[0]:
            if state["n_events"] < MAX_EVENTS:
                state["events"].append((n, int(p), int(fs[p]), float(fv[p])))
            state["n_events"] += 1
        nv[fire], ns[fire] = NEG, -1
        Vv[used], St[used] = nv[used], ns[used]
    return state


def event_dicts(events, clock=None, subsample: int = 4, sample_rate: int = 16000,
                names: Optional[Sequence] = None) -> List[dict]:
    """stored events (end, phrase, start, score) -> [{phrase, start, end, score}].  With ``clock`` (align.FeatureClock of
    the utterance) start / end are SECONDS of audio - where the first frame begins, where the last one ends -, else
    encoder frames (both inclusive).  ``names``: phrase index -> what ``phrase`` shows (default: the index)."""
    out = []
    for end, p, start, score in events:
        d = {"phrase": names[p] if names is not None else int(p), "start": int(start), "end": int(end),
             "score": float(score)}
        if clock is not None:
            d["start"] = clock.frame_span(int(start), subsample)[0] / sample_rate
            d["end"] = clock.frame_span(int(end), subsample)[1] / sample_rate
        out.append(d)
    return out
