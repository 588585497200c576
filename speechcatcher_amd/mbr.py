"""Consensus finals (sc_mbr_hyps / sc_mbr_lists; csrc/mbr.hip): the host side of the scheduler's
``consensus`` option.  The lists are compared and the slot statistics summed on the GPU (NativeStreamBatch.mbr_hyps /
mbr_lists); here a list's entry of those calls becomes records - per token of the pivot {"id", "token", "consensus": the
share of the list's mass that has this token in this slot, "rival": {"id", "token", "mass"} the strongest other
occupant of the slot (id -1, token "": nothing here) where there is one} -, token slots are merged into word slots with
align.merge_words' grouping (a word's consensus is the minimum of its tokens'), and the Vosk word entries get the
consensus as their "conf"."""
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from .align import merge_words

MAX_HYPS, MAX_LEN = _abi.MBR_MAX_HYPS, _abi.MBR_MAX_LEN
NONFINITE, BAD_TOKEN, TOO_LONG, NO_PIVOT = _abi.MBR_NONFINITE, _abi.MBR_BAD_TOKEN, _abi.MBR_TOO_LONG, _abi.MBR_NO_PIVOT
MODES = (True, "confidence")

_ROWS = ("ids", "xpos", "lens", "score", "score_dec", "score_ctc", "lm", "fused", "am_rank")


def check_mode(mode):
    """the ``consensus`` option: None / False (off), True (the reply is the minimum-risk row) or "confidence" (the reply
    stays the first-ranked row; only the slot statistics are added)"""
    if mode is None or mode is False:
        return None
    if mode is True or mode == "confidence":
        return mode
    raise ValueError('consensus is True or "confidence"')


def labels(row: Sequence[int], length: int, eos: int) -> List[int]:
    """a hypothesis row of ``hypotheses_arrays`` without <sos> and without a trailing <eos>"""
    e = int(length)
    if e > 1 and int(row[e - 1]) == eos:
        e -= 1
    return [int(v) for v in row[1:max(1, e)]]


def token_records(entry: dict, pivot_labels: Sequence[int], names: Optional[Sequence[str]] = None) -> List[dict]:
    """one record per label of the pivot from a list's entry of mbr_hyps / mbr_lists"""
    name = lambda t: names[t] if names is not None and 0 <= t < len(names) else str(t)     # noqa: E731
    out = []
    for t, c in enumerate(pivot_labels):
        if t >= len(entry["conf"]):
            break
        rec = {"id": int(c), "token": name(int(c)), "consensus": float(entry["conf"][t])}
        alt = int(entry["alt_tok"][t])
        if alt >= -1:
            rec["rival"] = {"id": alt, "token": "" if alt < 0 else name(alt), "mass": float(entry["alt_mass"][t])}
        out.append(rec)
    return out


def word_slots(tokens: Sequence[str], records: Sequence[dict]) -> List[dict]:
    """token slots -> word slots with merge_words' grouping: {"word", "consensus": the minimum of its tokens', "rival":
    the rival of the token that decides that minimum, as text, where it has one, "tokens": the word's records}"""
    idx = list(range(len(tokens)))
    words = merge_words(tokens, idx, idx, [1.0] * len(tokens))
    out = []
    for w in words:
        recs = [records[k] for k in range(int(w["start"]), int(w["end"]) + 1) if k < len(records)]
        if not recs:
            continue
        low = min(recs, key=lambda r: r["consensus"])
        slot = {"word": w["word"], "consensus": low["consensus"], "tokens": recs}
        if "rival" in low:
            slot["rival"] = {"word": low["rival"]["token"].replace("▁", ""), "mass": low["rival"]["mass"]}
        out.append(slot)
    return out


def summary(entry: dict, am_rank: Optional[int] = None) -> dict:
    """the "mbr" record of a reply: the pivot's row in the list the consensus was taken over, its risk, and its rank in
    the list before any re-ranking (``am_rank``; default: the pivot's row)"""
    P = int(entry["pivot"])
    return {"pivot": P, "risk": float(entry["risk"][P]) if P >= 0 else None, "am_rank": P if am_rank is None else int(am_rank)}


def pivot_first(arrays: dict, i: int, P: int, nh: int):
    """move hypothesis ``P`` of row ``i`` of ``hypotheses_arrays`` to the front, the others keeping their order, in place.
    Returns the order: row q is now the former row order[q]."""
    order = np.asarray([P] + [r for r in range(nh) if r != P], np.int64)
    if P > 0:
        moved = {k: arrays[k][i, order] for k in _ROWS if k in arrays}
        for k, v in moved.items():
            arrays[k][i, :nh] = v
    return order


def vosk_words(words: List[dict], slots: Sequence[dict]) -> List[dict]:
    """Vosk word entries with the consensus as their "conf": the acoustic value moves to "am_conf", and an entry with a
    rival carries it.  Entries and slots correspond one to one (both come from merge_words' grouping of one token
    list); when they do not - tokens without an alignment were left out of the entries - the entries stay as they are."""
    if len(words) != len(slots):
        return words
    out = []
    for w, s in zip(words, slots):
        e = dict(w)
        e["am_conf"], e["conf"] = w["conf"], s["consensus"]
        if "rival" in s:
            e["rival"] = s["rival"]
        out.append(e)
    return out
