"""CTC prefix beam search (csrc/ctc_beam.hip, sc_ctc_beam / sc_ctc_beam_pack): an n-best list of token
prefixes with their CTC prefix probabilities, from the CTC rows every admission group projects - the cheap tier beside
the attention search, and what a decoder-free stream is served from.  The search itself runs on the GPU
(tests/ctc_beam_ref.py is its contract); this module holds the host-side helpers.

A state is {"n_frames", "n_bad", "n_nodes", "entries": [(node, last, len, parent, pb, pnb)] best first}; a hypothesis
is {"ids", "frames", "pb", "pnb"}: the tokens of an entry's prefix with the frames of the utterance at which each was
first emitted, numbered in the order they were scanned.
"""
from typing import List, Optional, Sequence

import numpy as np

from .alternates import nbest_posterior
from .align import merge_words

DEFAULT = (8, 8)   # (B, C): a parameter, not tuned
NEG = float("-inf")


def params(ctc_beam):
    """``ctc_beam`` as the scheduler and the CLI take it - None / 0 / False: off, True: DEFAULT, B, or (B, C) - ->
    (B, C) or None"""
    if ctc_beam is None or ctc_beam is False or ctc_beam == 0:
        return None
    if ctc_beam is True:
        return DEFAULT
    if isinstance(ctc_beam, (tuple, list)):
        B, C = (int(v) for v in ctc_beam)
    else:
        B, C = int(ctc_beam), DEFAULT[1]
    if not (1 <= B <= 16 and 1 <= C <= 16):
        raise ValueError(f"ctc_beam: beam and candidates must lie in [1, 16], got ({B}, {C})")
    return B, C


def initial() -> dict:
    return {"n_frames": 0, "n_bad": 0, "n_nodes": 1, "entries": [(0, -1, 0, -1, 0.0, NEG)]}


def total(pb: float, pnb: float) -> float:
    """log(exp(pb) + exp(pnb)): the log probability of a prefix"""
    if pb == NEG:
        return float(pnb)
    if pnb == NEG:
        return float(pb)
    hi, lo = (pb, pnb) if pb >= pnb else (pnb, pb)
    return float(hi + np.log1p(np.exp(lo - hi)))


def backtrace(entry, nodes):
    """(ids, frames) of an entry's prefix from the stored (parent, token, frame) records; None when a node of its chain
    is not among them"""
    ids, frames, node = [], [], int(entry[0])
    for _ in range(int(entry[2])):
        if not 0 < node < len(nodes):
            return None
        parent, tok, frame = nodes[node][:3]
        ids.append(int(tok))
        frames.append(int(frame))
        node = int(parent)
    return ids[::-1], frames[::-1]


def hyps_of(state: dict, nodes, nbest: int) -> List[dict]:
    """the first nbest entries of a state as hypotheses, walked on the host (the Python engine's side of sc_ctc_beam_hyps)"""
    out = []
    for e in state["entries"][:nbest]:
        bt = backtrace(e, nodes)
        if bt is None:
            break
        out.append({"ids": bt[0], "frames": bt[1], "pb": float(e[4]), "pnb": float(e[5])})
    return out


def token_dicts(hyp: dict, clock=None, subsample: int = 4, sample_rate: int = 16000,
                names: Optional[Sequence] = None) -> List[dict]:
    """a hypothesis -> [{id, start, end}]: a token runs from the frame of its first emission to the frame before the
    next token's (its own for the last one).  With ``clock`` (align.FeatureClock of the utterance) start / end are SECONDS
    of audio - where the first frame begins, where the last one ends -, else encoder frames (both inclusive).
    ``names``: token id -> "token" (e.g. the model's token list)."""
    ids, frames = hyp["ids"], hyp["frames"]
    out = []
    for k, (tid, start) in enumerate(zip(ids, frames)):
        end = max(int(start), int(frames[k + 1]) - 1) if k + 1 < len(frames) else int(start)
        d = {"id": int(tid), "start": int(start), "end": end}
        if names is not None:
            d["token"] = names[int(tid)]
        if clock is not None:
            d["start"] = clock.frame_span(int(start), subsample)[0] / sample_rate
            d["end"] = clock.frame_span(end, subsample)[1] / sample_rate
        out.append(d)
    return out


def text_of(ids: Sequence[int], names: Optional[Sequence] = None, boundary: str = "▁") -> str:
    """the SentencePiece tokens of a hypothesis as text (ids joined by spaces without a token list)"""
    if names is None:
        return " ".join(str(int(t)) for t in ids)
    return "".join(names[int(t)] for t in ids).replace(boundary, " ").strip()


def words_of(hyp: dict, names: Sequence, clock=None, subsample: int = 4, sample_rate: int = 16000) -> List[dict]:
    """the words of a hypothesis through align.merge_words, timed by the first emission of their tokens (conf 1.0: the
    search gives a probability per prefix, none per token)"""
    toks = token_dicts(hyp, clock, subsample, sample_rate, names)
    return merge_words([t["token"] for t in toks], [t["start"] for t in toks], [t["end"] for t in toks],
                       [1.0] * len(toks))


def nbest(hyps: Sequence[dict], names: Optional[Sequence] = None, clock=None, subsample: int = 4,
          sample_rate: int = 16000, side: Optional[dict] = None) -> List[dict]:
    """hypotheses (best first) -> the n-best list of a reply: {"text", "ids", "score" (the prefix's log probability),
    "conf" (its share of the listed mass, alternates.nbest_posterior of the totals), "tokens"}.  ``side`` (a language
    model is fused in, DESIGN.md 8k: {"lm", "fused"} of the same entries, NativeStreamBatch.ctc_beam_lm): every entry
    also carries "lm", the model's log probability of its tokens, "score" is the FUSED total the beam ranks by
    ("ctc_score": the prefix's own log probability), and "conf" comes from the fused totals."""
    totals = [total(h["pb"], h["pnb"]) for h in hyps]
    if side is None:
        confs = nbest_posterior(totals)
        return [{"text": text_of(h["ids"], names), "ids": list(h["ids"]), "score": t, "conf": c,
                 "tokens": token_dicts(h, clock, subsample, sample_rate, names)} for h, t, c in zip(hyps, totals, confs)]
    fused = [float(f) for f in side["fused"][:len(hyps)]]
    confs = nbest_posterior(fused)
    return [{"text": text_of(h["ids"], names), "ids": list(h["ids"]), "score": f, "ctc_score": t, "lm": float(l), "conf": c,
             "tokens": token_dicts(h, clock, subsample, sample_rate, names)}
            for h, t, f, l, c in zip(hyps, totals, fused, side["lm"], confs)]
