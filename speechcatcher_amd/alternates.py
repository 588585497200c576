"""Token alternates and n-best alternatives of a final result.

``NativeStreamBatch.alternates`` (sc_alternates_hyps) gives, for every token of a hypothesis, the K tokens with the largest
summed CTC emission over the token's aligned frames and the rank of the token itself among them.  This module turns those
arrays into per-token records, turns the total scores of an n-best list into posteriors, and formats both the way a Vosk
client expects them (``config.max_alternatives``).

A record: {"id", "token", "conf", "own_rank", "alternates": [{"id", "token", "conf"}, ...]} with conf = exp(mean CTC
log-posterior over the token's frames) - for the token itself the alignment's confidence, for an alternate the same
quantity of the other token over the SAME frames.  own_rank 0: the token is the acoustic best of its own frames.
"""
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from .align import merge_words

MAX_K = _abi.ALT_MAX_K


def nbest_posterior(scores: Sequence[float]) -> List[float]:
    """exp(score_i - logsumexp(scores)) in float64 over the listed hypotheses: what share of the list's probability mass
    each one holds ([] for an empty list; -inf scores get 0, a list of nothing but -inf is shared evenly)"""
    s = np.asarray(list(scores), np.float64)
    if s.size == 0:
        return []
    m = s.max()
    if m == -np.inf:
        return [1.0 / s.size] * s.size
    lse = m + np.log(np.sum(np.exp(s - m)))
    return [float(p) for p in np.exp(s - lse)]


def _name(token_list, t: int) -> str:
    return token_list[t] if token_list is not None and 0 <= t < len(token_list) else str(t)


def token_record(token_id: int, conf: Optional[float], own_rank: Optional[int], alt_ids, alt_logp, token_list=None) -> dict:
    """one record from the K slots of a span (alt_ids -1: an unused slot)"""
    alts = [{"id": int(v), "token": _name(token_list, int(v)), "conf": float(np.exp(lp))}
            for v, lp in zip(alt_ids, alt_logp) if int(v) >= 0]
    return {"id": int(token_id), "token": _name(token_list, int(token_id)), "conf": conf,
            "own_rank": own_rank, "alternates": alts}


def result_token_alternates(ys, is_final: bool, alt: dict, i: int, j: int, cfg, token_list=None) -> List[dict]:
    """the records of the tokens hyps_to_results returns for hypothesis yseq ``ys`` - one per entry of
    result_token_alignment's "token_ids", in that order - from row (i, j) of NativeStreamBatch.alternates.  A token without
    a label state of the alignment, of a hypothesis that could not be aligned, or whose span holds a bad row has conf
    None, own_rank None and no alternates."""
    ids = ys[1:] if is_final else ys[1:min(1, len(ys))]
    if ids and ids[-1] == 1023:
        ids = ids[:-1]
    n_lab = len(ys) - 1 - (1 if ys[-1] == cfg.eos_id else 0)
    ok = int(alt["status"][i, j]) == _abi.ALIGN_OK
    out = []
    for k, t in enumerate(ids):
        if t in (0, 1, 1023):
            continue
        if ok and k < n_lab and int(alt["span_status"][i, j, k]) == _abi.ALT_OK:
            rank = int(alt["own_rank"][i, j, k])
            out.append(token_record(t, float(np.exp(alt["logp_mean"][i, j, k])), rank if rank >= 0 else None,
                                    alt["alt_ids"][i, j, k], alt["alt_logp"][i, j, k], token_list))
        else:
            out.append(token_record(t, None, None, [], [], token_list))
    return out


# ---- Vosk formatting -------------------------------------------------------------------------------------------------
def word_token_groups(tokens: Sequence[str]) -> List[List[int]]:
    """indices of the tokens that make up each word of align.merge_words(tokens, ...), word by word"""
    idx = list(range(len(tokens)))
    return [list(range(int(w["start"]), int(w["end"]) + 1)) for w in merge_words(tokens, idx, idx, [1.0] * len(tokens))]


def attach_word_tokens(words: List[dict], tokens: Sequence[str], records: Sequence[dict]) -> List[dict]:
    """word entries of a Vosk result built by merge_words over ``tokens`` -> the same entries with "tokens": the records of
    each word's tokens (``records``: one per token)"""
    groups = word_token_groups(tokens)
    assert len(groups) == len(words)
    return [dict(w, tokens=[records[k] for k in g]) for w, g in zip(words, groups)]


def attach_entry_tokens(entries: List[dict], records: Sequence[dict]) -> List[dict]:
    """the classic Vosk result's entries, one per token -> the same entries with "tokens": [that token's record]"""
    return [dict(e, tokens=[r]) for e, r in zip(entries, records)]


def vosk_alternatives(texts: Sequence[str], scores: Sequence[float], results: Sequence[List[dict]]) -> dict:
    """the final message of a session with ``config.max_alternatives`` > 0: {"alternatives": [{"text", "confidence",
    "result": [word entries]}, ...]}, best first; confidence = nbest_posterior of the listed hypotheses' total scores"""
    conf = nbest_posterior(scores)
    return {"alternatives": [{"text": t, "confidence": c, "result": list(r)} for t, c, r in zip(texts, conf, results)]}


__all__ = ["MAX_K", "nbest_posterior", "token_record", "result_token_alternates", "word_token_groups",
           "attach_word_tokens", "attach_entry_tokens", "vosk_alternatives"]
