"""CTC draft transcript (csrc/draft.hip, sc_ctc_draft): the collapsed arg-max path of the CTC rows - token
ids with frame times and a posterior -, known as soon as the encoder has emitted the frames, ahead of the blockwise
search.  This module is the recurrence in numpy float64 (the Python engine's side of it; tests/ctc_draft_ref.py is the
contract) and the host-side helpers.

A token is (id, start, end, conf): frames of the utterance, both inclusive, numbered in the order they were scanned;
conf is the largest arg-max posterior among its frames.  The state of a stream is the seven FIELDS plus the tokens that
have closed; its draft is those followed by the open token, if any.
"""
from typing import List, Optional, Sequence

import numpy as np

from . import ctc_rows

FIELDS = ("n_frames", "n_closed", "n_bad", "open_id", "open_start", "open_end", "open_conf")
TOKEN_FIELDS = ("id", "start", "end", "conf")
INITIAL = (0, 0, 0, -1, -1, -1, 0.0)


def initial() -> dict:
    d = dict(zip(FIELDS, INITIAL))
    d["tokens"] = []
    return d


def advance(state: dict, rows, blank: int, capacity: Optional[int] = None) -> dict:
    """state + the fp32 CTC rows [T, V] of a span of further frames -> the new state (in place, returned).  A token that
    closes is appended to state["tokens"] while those hold fewer than ``capacity`` (None: no limit)."""
    x32 = np.asarray(rows, np.float32)
    n, nc, nbad = state["n_frames"], state["n_closed"], state["n_bad"]
    oid, ost, oen, ocf = state["open_id"], state["open_start"], state["open_end"], state["open_conf"]
    toks = state["tokens"]
    for t in range(x32.shape[0]):
        r32 = x32[t]
        bad = ctc_rows.is_bad(r32)
        k = -1 if bad else int(np.argmax(r32))   # the lowest index among ties
        if bad or k == blank or k != oid:
            if oid >= 0:                          # the open token closes
                if capacity is None or nc < capacity:
                    toks.append((oid, ost, oen, ocf))
                nc += 1
                oid, ost, oen, ocf = -1, -1, -1, 0.0
        if bad:
            nbad += 1
        elif k != blank:
            p = float(np.exp(np.float64(r32[k]) - ctc_rows.lse(r32)))
            if k == oid:
                oen, ocf = n, max(ocf, p)
            else:
                oid, ost, oen, ocf = k, n, n, p
        n += 1
    state.update(n_frames=n, n_closed=nc, n_bad=nbad, open_id=oid, open_start=ost, open_end=oen, open_conf=ocf)
    return state


def tokens_of(state: dict) -> List[tuple]:
    """the draft of a state: its stored tokens followed by the open token, if any"""
    out = list(state["tokens"])
    if state["open_id"] >= 0:
        out.append((state["open_id"], state["open_start"], state["open_end"], state["open_conf"]))
    return out


def as_arrays(states: Sequence[dict]) -> dict:
    """{field: array [n]} of a list of states: int32, open_conf float64"""
    return {k: np.asarray([s[k] for s in states], np.float64 if k == "open_conf" else np.int32) for k in FIELDS}


def token_dicts(tokens, clock=None, subsample: int = 4, sample_rate: int = 16000,
                names: Optional[Sequence] = None) -> List[dict]:
    """tokens (id, start, end, conf) -> [{id, start, end, conf}].  With ``clock`` (align.FeatureClock of the utterance)
    start / end are SECONDS of audio - where the first frame begins, where the last one ends -, else encoder frames
    (both inclusive).  ``names``: token id -> "token" (e.g. the model's token list)."""
    out = []
    for tid, start, end, conf in tokens:
        d = {"id": int(tid), "start": int(start), "end": int(end), "conf": float(conf)}
        if names is not None:
            d["token"] = names[int(tid)]
        if clock is not None:
            d["start"] = clock.frame_span(int(start), subsample)[0] / sample_rate
            d["end"] = clock.frame_span(int(end), subsample)[1] / sample_rate
        out.append(d)
    return out


def ahead(tokens, horizon: int) -> list:
    """The tokens (tuples, or dicts whose "start" is in frames) whose start >= horizon (a frame position): with the
    frame position of the search's last token as the horizon, the part of the draft that lies behind what the search
    has already put out.  A heuristic for splicing, exact as a function; it does not claim which frames a token of the
    search covers."""
    return [t for t in tokens if int(t["start"] if isinstance(t, dict) else t[1]) >= int(horizon)]
