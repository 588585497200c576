"""Multi-stream scheduler: turns independent client sessions into batched
``StreamBatch.push`` calls (continuous batching across sessions, per-session
chunk order preserved).

This is the "next" row of SURVEY.md section 8(f) rank 1: it replaces the
reference server's pool of full model copies, one per websocket client
(``Speech2TextPool``, speechcatcher/speechcatcher_server.py:331-357) and its
per-session call ``self.speech2text(speech=data, is_final=...)`` (:270) by
slots of ONE weight replica whose chunk steps run batched on the GPU.  The
network side (websockets, ffmpeg, Vosk JSON) stays out of scope.

Parity note: the reference's output depends on the chunking of each stream, so
the scheduler never re-chunks: one chunk fed by a session is one engine call
for that stream, exactly as if the session owned a private Speech2TextStreaming.
"""
import hashlib
import math
import os
from collections import deque
from typing import Deque, Dict, List, Optional, Tuple

import numpy as np

from .engine import StreamBatch
from . import spotting
from .spotting import phrase_ids
from . import grammar as grammar_mod
from . import draft as draft_mod
from . import ctc_beam as beam_mod
from . import alternates as alternates_mod
from . import commit as commit_mod
from . import rescore as rescore_mod
from . import mbr as mbr_mod
from .activity import of_stream as activity_of_stream
from .align import FeatureClock
from . import pcm as pcm_mod
from .resample import OutputClock, check_input_rate
from .speech2text_streaming import hyps_to_results, result_token_alignment

EOS_ID = 1023   # hard-coded in the reference's result assembly (speech2text_streaming.py:474,500: SURVEY A4)


class ServerBusy(RuntimeError):
    """All stream slots are taken (the reference answers "Server busy",
    speechcatcher_server.py:365-368)."""


_FLOAT_INPUT = (pcm_mod.F32, 1, 0, pcm_mod.SCALE_FULL)   # mono float samples: the engine's default format


class AlignedResults(list):
    """the results of a final reply (a list, like every reply) and ``alignment``: result_token_alignment of its first
    result (None when it has none) - StreamScheduler(align_final=True).  With ``alternates=K`` the alignment also carries
    "alternates": the records of those tokens (speechcatcher_amd.alternates.result_token_alternates); with
    ``align_nbest`` > 1 also "nbest": result_token_alignment of each of the reply's first ``align_nbest`` results."""
    alignment: Optional[dict] = None
    # StreamScheduler(final_lm=...): per result of a re-ranked final {"score", "lm", "fused", "am_rank"}
    rescored: Optional[list] = None
    # StreamScheduler(consensus=...): of a final {"mbr": {"pivot", "risk", "am_rank"}, "tokens": a record per token of
    # the first result {"id", "token", "consensus", "rival"?} (speechcatcher_amd.mbr)}
    consensus: Optional[dict] = None


class ActivityResults(AlignedResults):
    """the results of a reply and ``activity``: {field: int} (speechcatcher_amd.activity.FIELDS) of the session's stream
    for that chunk - StreamScheduler(activity=True).  A final reply of a scheduler with ``align_final`` as well carries
    both attributes."""
    activity: Optional[dict] = None


class SpottingResults(ActivityResults):
    """the results of a reply and ``detections``: the phrase-spotting events of the session's stream that are new since
    the session's previous reply - StreamScheduler(phrases=...).  Each is {"phrase": index in the set, "start", "end":
    encoder frames of the utterance (both inclusive), "score", "start_s", "end_s": seconds of the utterance's audio}.
    ``alignment`` / ``activity`` are carried as well when those options are on."""
    detections: Optional[list] = None


class DraftResults(SpottingResults):
    """the results of a reply, ``draft``: the draft transcript of the session's stream for that chunk (the collapsed
    arg-max path of every CTC frame the encoder had emitted when the chunk was admitted) and ``ahead``: the part of it
    behind the search's last token - StreamScheduler(draft=True).  Each token is {"id", "start", "end": encoder frames
    of the utterance (both inclusive), "conf", "start_s", "end_s": seconds of the utterance's audio, "token": its text
    when the scheduler has a token list}.  ``ahead`` = speechcatcher_amd.draft.ahead(draft, h) with h the frame position
    the reply carries for its first result's last token (result_format "espnet"; 0 for an empty result and for the
    "native" format, which carries no positions): a heuristic for splicing.  ``alignment`` / ``activity`` /
    ``detections`` are carried as well when those options are on."""
    draft: Optional[list] = None
    ahead: Optional[list] = None


class LevelResults(DraftResults):
    """the results of a reply and ``level``: the input level of the session's stream up to and including that chunk
    ({field: int}, speechcatcher_amd.pcm.LEVEL_FIELDS; all zero for a session that feeds float samples) -
    StreamScheduler(input_level=True).  The attributes of the other options are carried as well when those are on."""
    level: Optional[dict] = None


class StableResults(LevelResults):
    """the results of a reply and ``stable``: {"committed": n, "tokens": ids, "stability": values} of the session's stream
    for that chunk - StreamScheduler(stable_partials=True).  ``tokens`` is the best live hypothesis (the <sos> first); its
    first n tokens are committed: every live hypothesis has them, so no later chunk of the utterance changes them, and n
    only grows.  ``stability`` holds one value per token behind them: the share of the beam's probability
    mass that agrees with the best hypothesis up to and including that token.  A final reply commits everything.  The
    attributes of the other options are carried as well when those are on."""
    stable: Optional[dict] = None


class CtcBeamResults(StableResults):
    """the results of a reply and ``ctc_nbest``: the n-best list of the CTC prefix beam search of the session's stream for
    that chunk, best first - StreamScheduler(ctc_beam=B) or ctc_beam=(B, C).  Each entry is {"text", "ids",
    "score": the prefix's log probability, "conf": its share of the listed mass, "tokens": [{"id", "start", "end":
    encoder frames of the utterance (both inclusive; a token runs from its first emission to the frame before the next
    token's), "start_s", "end_s": seconds of the utterance's audio, "token": its text when the scheduler has a token
    list}]}.  For a decoder-free session (``open(decoder="ctc")``) the reply's results ARE the beam's best.  The
    attributes of the other options are carried as well when those are on."""
    ctc_nbest: Optional[list] = None
    # a session with a grammar (open(grammar=...)): the entries of ``ctc_nbest`` carry "complete", the
    # grammar's accept flag; at a final they come complete entries first (each group in beam order), and
    # ``grammar_complete`` says whether the entry reported first is complete (None without a grammar)
    grammar_complete: Optional[bool] = None


class StreamScheduler:
    def __init__(self, batch: StreamBatch, token_list: Optional[List[str]] = None,
                 result_format: str = "native", reset_after_final: bool = True, reset_on_open: bool = True,
                 queue_depth: int = 1, align_final: bool = False, activity: bool = False, blank_threshold: float = 0.8,
                 phrases=None, min_scores=None, draft: bool = False, input_level: bool = False, alternates: int = 0,
                 align_nbest: int = 1, stable_partials: bool = False, ctc_beam=None, ctc_lm=None,
                 lm_weight: float = 0.5, word_bonus: float = 0.0, final_lm=None, final_lm_weight: float = 0.5,
                 final_word_bonus: float = 0.0, final_lm_eos: bool = False, attention_rescore=None, consensus=None,
                 consensus_scale: float = 1.0):
        """``queue_depth`` > 1 (C++ engine, ``pump``): up to that many queued chunks of a session are handed to the engine
        at a time (sc_streams_set_queue_depth) - for sessions whose audio is already there (files): the encoder stage of
        the next chunk runs beside the decoding of the current one.  Replies and their order per session do not change.

        ``reset_after_final`` / ``reset_on_open`` (default True): a finalised utterance and a newly opened
        session start from a reset stream - what the reference CLI does (speechcatcher.py:618-619).  The
        reference SERVER does neither (speechcatcher_server.py:270,364-397: no reset after is_final=True, models
        go back to the pool as they are); ``ServerLoop(strict_reference=True)`` switches both off to reproduce
        that.  What reset() itself leaves behind is the batch's ``strict_reference`` (StreamBatch.reset).

        ``align_final`` (C++ engine): every final reply is an ``AlignedResults`` whose ``alignment`` holds the token times and
        confidences of its first result (CTC forced alignment, NativeStreamBatch.align), taken before the stream is reset."""
        self.align_final = align_final
        # ``alternates`` = K > 0 (C++ engine; implies ``align_final``): the ``alignment`` of a final reply also carries
        # "alternates", the K acoustic alternates of every token of its first result, from ONE call in place of ``align``
        # (NativeStreamBatch.alternates).  ``align_nbest`` = N > 1: the final's alignment covers its first N results
        # ("nbest"; what ServerLoop(vosk_alternatives=N) formats)
        self.alternates, self.align_nbest = 0, max(1, int(align_nbest))
        # ``activity``: every reply (an exception aside) is an ``ActivityResults`` whose ``activity`` is the acoustic
        # speech / silence state of the session's stream for that chunk (batch.set_activity(True, blank_threshold)), read
        # before the stream is reset after a final
        self.activity = False
        # ``phrases`` (token-id sequences; ``min_scores``: their floors): every reply (an exception aside) is a
        # ``SpottingResults`` whose ``detections`` are the events new since the session's previous reply
        # (batch.set_phrases), read before the stream is reset after a final
        self.spotting = False
        # ``draft``: every reply (an exception aside) is a ``DraftResults`` (batch.set_draft), read before the stream is
        # reset after a final
        self.draft = False
        # ``ctc_beam``: (B, C) when on - every reply (an exception aside) is a ``CtcBeamResults`` (batch.set_ctc_beam),
        # read before the stream is reset after a final; sessions opened with decoder="ctc" are served from it alone
        self.ctc_beam = None
        # ``ctc_lm`` (needs ``ctc_beam``; C++ engine): the path of a packed n-gram model (speechcatcher_amd.ngram) or its
        # bytes - the beam keeps its entries by total + lm_weight * lm + word_bonus * len, the entries of
        # ``ctc_nbest`` gain "lm" and their "score" is that fused total.  (lm_weight, word_bonus) when on.
        self.ctc_lm = None
        # ``final_lm`` (C++ engine): the path of a packed n-gram model or its bytes - at a final of a FULL session the
        # n-best list is rescored on the GPU and re-ranked by fused = score + final_lm_weight * (lm + the </s> term with
        # ``final_lm_eos``) + final_word_bonus * labels (NativeStreamBatch.rescore_hyps): the reply's results
        # come in that order, its ``rescored`` holds {"score", "lm", "fused", "am_rank"} per result (result_format
        # "espnet": the hypothesis dicts carry them too), and the alignment / alternates belong to the results reported.
        # Partials are untouched; no hypothesis or score of the search changes.  (weight, bonus, eos) when on.
        # ``final_lm_eos`` with ``ctc_lm``: the final ``ctc_nbest`` of a decoder-free session is re-ranked with the </s>
        # term of the SAME model at the beam's weights (NativeStreamBatch.rescore_lists).
        self.final_lm = None
        self.final_lm_eos = bool(final_lm_eos)
        self._final_dev = self._ctc_blob = self._ctc_dev = None
        self._ctc_sessions = set()
        # ``attention_rescore`` (needs ``ctc_beam``; C++ engine): True or (w_att, w_ctc[, beta]) - sessions
        # opened with decoder="rescore" are decoder-free in the engine, their partials the beam's best as for "ctc"; at a
        # final the n-best list gets one teacher-forced pass of the attention decoder over the stream's encoder output and
        # is re-ranked by w_ctc * first pass + w_att * att + beta * labels (NativeStreamBatch.attention_rescore_beam, ONE
        # call for all such finals of a reply round).  (w_att, w_ctc, beta) when on; the default (1.0, 0.5, 0.0) are
        # parameters, not tuned.
        self.attention_rescore = None
        self._rescore_sessions = set()
        # ``consensus`` (C++ engine): True or "confidence" - at a final the rows of the n-best list are
        # compared on the GPU (NativeStreamBatch.mbr_hyps; mbr_lists for a list that ``final_lm`` / ``attention_rescore``
        # re-ranked and for the ``ctc_nbest`` of a decoder-free session - the totals are then the fused ones), ONE call for
        # all such finals of a reply round, with weights softmax(consensus_scale * total).  True: the reply's first
        # result is the minimum-Bayes-risk row under the edit distance.  "confidence": the first-ranked row stays first.
        # Both: the reply's ``consensus`` holds "mbr": {"pivot", "risk", "am_rank"} and "tokens", per token of the first
        # result its "consensus" - the share of the list's mass with that token in that slot - and the strongest "rival".
        # A grammar's "complete entries first" stays the outermost order.  Partials are untouched; the scale is a
        # parameter, not tuned.
        self.consensus = None
        self.consensus_scale = 1.0
        self._slot_dec: Dict[int, str] = {}
        # grammars (``open(grammar=...)``, ``set_grammar``; needs ``ctc_beam``; C++ engine): compiled grammars by the
        # SHA-256 of their blob, {"handle": the device copy, "uses": the slots that name it, "walk": its host walk} - a
        # thousand connections with one menu share one device copy, released when the last lets go of it
        self._gr_cache: Dict[str, dict] = {}
        self._slot_gr: Dict[int, Optional[str]] = {}
        # ``stable_partials``: every reply (an exception aside) is a ``StableResults``.  The scheduler owns one
        # commit.StablePrefix per session and asks the engine only for the tokens behind what that holds
        # (batch.hyps_delta: one call for all sessions of a reply round)
        self.stable_partials = False
        self._stable: Dict[int, commit_mod.StablePrefix] = {}
        self._spot_seen: Dict[int, int] = {}                  # per session: events of its utterance handed out so far
        self._clock: Dict[int, FeatureClock] = {}             # align_final: per session, the calls since its last reset
        self._fed: Dict[int, Deque[Tuple[int, bool]]] = {}   # ... and its fed chunks not reported yet (length, final)
        self.reset_after_final, self.reset_on_open = reset_after_final, reset_on_open
        self.batch = batch
        self.token_list = token_list
        self.result_format = result_format
        self._free: Deque[int] = deque(range(batch.S))
        self._slot_of: Dict[int, int] = {}
        self._queue: Dict[int, Deque[Tuple[np.ndarray, bool, bool]]] = {}
        # continuous batching: session -> its chunks at the engine, oldest first: (slot, final, finalize_all)
        self._in_flight: Dict[int, Deque[Tuple[int, bool, bool]]] = {}
        # replies that are ready but have not gone out yet, per session and oldest first: pump() hands out at most ONE
        # reply per session and call (its return value is {session: reply}); a second one of the same session (queue
        # depth > 1, or one collected inside close() of another session) waits here for the next call
        self._stash: Dict[int, Deque[list]] = {}
        self._slot_rate: Dict[int, int] = {}                  # input rate last set on a slot (absent: 16000)
        self._slot_fmt: Dict[int, tuple] = {}                 # input format last set on a slot (absent: float samples)
        self._fmt: Dict[int, tuple] = {}                      # per session with a wire format: (format, channels, channel, scale)
        self.input_level = bool(input_level)                  # replies carry the session's input level (LevelResults)
        self._rate: Dict[int, OutputClock] = {}               # per session: its rate and its count of 16 kHz samples
        self.queue_depth = 1
        if queue_depth > 1 and hasattr(batch, "set_queue_depth"):
            batch.set_queue_depth(queue_depth)
            self.queue_depth = queue_depth
        self._next_sid = 0
        if activity:
            self.enable_activity(blank_threshold)
        if phrases:
            self.enable_spotting(phrases, min_scores)
        if draft:
            self.enable_draft()
        if beam_mod.params(ctc_beam):
            self.enable_ctc_beam(*beam_mod.params(ctc_beam))
        if ctc_lm is not None:
            self.enable_ctc_lm(ctc_lm, lm_weight, word_bonus)
        if final_lm is not None:
            self.enable_final_lm(final_lm, final_lm_weight, final_word_bonus, final_lm_eos)
        elif self.final_lm_eos and not hasattr(batch, "rescore_lists"):
            raise NotImplementedError("the </s> term of finals is computed by the C++ engine (NativeStreamBatch."
                                      "rescore_lists); the Python lock-step engine has none")
        if attention_rescore is not None and attention_rescore is not False:
            self.enable_attention_rescore(attention_rescore)
        if alternates:
            self.enable_alternates(alternates)
        if stable_partials:
            self.enable_stable_partials()
        if consensus is not None and consensus is not False:
            self.enable_consensus(consensus, consensus_scale)

    def enable_activity(self, blank_threshold: float = 0.8):
        """switch the ``activity`` option on (only while no chunk is at the engine; every stream's state starts over)"""
        self.batch.set_activity(True, blank_threshold)
        self.activity = True

    def enable_spotting(self, phrases, min_scores=None):
        """switch the ``phrases`` option on (only while no chunk is at the engine; every stream's state starts over)"""
        self.batch.set_phrases(phrases, min_scores)
        self.spotting = True
        self._spot_seen.clear()

    def enable_draft(self):
        """switch the ``draft`` option on (only while no chunk is at the engine; every stream's state starts over)"""
        self.batch.set_draft(True)
        self.draft = True

    def enable_ctc_beam(self, beam: int = beam_mod.DEFAULT[0], candidates: int = beam_mod.DEFAULT[1]):
        """switch the ``ctc_beam`` option on (only while no chunk is at the engine; every stream's state starts over)"""
        if not hasattr(self.batch, "set_ctc_beam"):
            raise NotImplementedError("this batch has no CTC prefix beam search (set_ctc_beam)")
        self.batch.set_ctc_beam(int(beam), int(candidates))
        self.ctc_beam = (int(beam), int(candidates))

    def enable_ctc_lm(self, source, lm_weight: float = 0.5, word_bonus: float = 0.0):
        """fuse an n-gram model into the CTC beam (only while no chunk is at the engine; every stream's beam starts
        over).  ``source``: the path of a packed model or its bytes; None detaches it."""
        if self.ctc_beam is None:
            raise ValueError("ctc_lm needs the ctc_beam option (StreamScheduler(ctc_beam=...))")
        if not hasattr(self.batch, "set_ctc_beam_lm"):
            raise NotImplementedError("this batch has no language model fusion (set_ctc_beam_lm)")
        if source is None:
            self.batch.set_ctc_beam_lm(None)
            self.ctc_lm = self._ctc_blob = self._ctc_dev = None
            return
        from . import ngram
        blob = ngram.load(source)
        self.batch.set_ctc_beam_lm(blob, float(lm_weight), float(word_bonus))
        self.ctc_lm = (float(lm_weight), float(word_bonus))
        self._ctc_blob, self._ctc_dev = blob, None

    def enable_final_lm(self, source, lm_weight: float = 0.5, word_bonus: float = 0.0, eos: bool = False):
        """switch the ``final_lm`` option on: ``source`` is the path of a packed model or its bytes; None switches it
        off.  ``lm_weight`` / ``word_bonus`` are parameters, not tuned."""
        if source is None:
            self.final_lm = self._final_dev = None
            return
        if not hasattr(self.batch, "rescore_hyps"):
            raise NotImplementedError("n-gram rescoring of finals runs in the C++ engine (NativeStreamBatch.rescore_hyps); "
                                      "the Python lock-step engine has none")
        if self.batch.W > rescore_mod.MAX_HYPS:
            raise ValueError(f"final_lm rescores a list of at most {rescore_mod.MAX_HYPS} hypotheses "
                             f"(this batch has beam {self.batch.W})")
        if not (math.isfinite(lm_weight) and math.isfinite(word_bonus)):
            raise ValueError("final_lm_weight and final_word_bonus must be finite")
        from . import ngram
        self._final_dev = self.batch.language_model(ngram.load(source))
        self.final_lm = (float(lm_weight), float(word_bonus), bool(eos))
        self.final_lm_eos = bool(eos)

    def enable_consensus(self, mode=True, scale: float = 1.0):
        """switch the ``consensus`` option on: True or "confidence"; None / False switches it off"""
        mode = mbr_mod.check_mode(mode)
        if mode is None:
            self.consensus = None
            return
        wide = max(int(getattr(self.batch, "W", 0) or 0), self.ctc_beam[0] if self.ctc_beam is not None else 0)
        if wide < 2:
            raise ValueError("consensus compares the rows of an n-best list: it needs a beam_size of at least 2 "
                             "(or ctc_beam=B with B >= 2 for decoder-free sessions)")
        if not hasattr(self.batch, "mbr_hyps"):
            raise NotImplementedError("consensus finals run in the C++ engine (NativeStreamBatch.mbr_hyps / mbr_lists, "
                                      "sc_mbr_hyps / sc_mbr_lists); the Python lock-step engine has none")
        if not (math.isfinite(scale) and scale >= 0):
            raise ValueError("consensus_scale must be finite and not negative")
        self.consensus, self.consensus_scale = mode, float(scale)

    def _consensus_full(self, arrays: dict, row: dict, fins: list, perm: dict) -> Tuple[dict, dict]:
        """ONE call for the round's finals of FULL sessions -> ({slot: the reply's ``consensus``}, {slot: order}): with
        ``consensus=True`` the pivot's row of ``arrays`` is moved to the front (row q is then the engine's row order[q])"""
        pinned = self.consensus == "confidence"
        eos = self._eos_id
        if perm:   # re-ranked finals: the lists as they stand now, each with its fused totals (a slot that was not
            # re-ranked goes with the search's totals, in the same call)
            lists, vals = [], []
            for slot in fins:
                i = row[slot]
                nh = int(arrays["n_hyps"][i])
                lists.append([mbr_mod.labels(arrays["ids"][i, j], arrays["lens"][i, j], eos) for j in range(nh)])
                vals.append([float(v) for v in arrays["fused" if slot in perm else "score"][i, :nh]])
            got = dict(zip(fins, self.batch.mbr_lists(lists, vals, scale=self.consensus_scale,
                                                      pivots=[0 if li else -1 for li in lists] if pinned else None)))
        else:
            got = self.batch.mbr_hyps(fins, scale=self.consensus_scale, pivot_best=pinned, nbest=arrays["ids"].shape[1])
        out, orders = {}, {}
        for slot in fins:
            e, i = got[slot], row[slot]
            P, nh = int(e["pivot"]), len(e["order"])
            if P < 0:
                continue
            base = perm.get(slot)
            am = int(base[P]) if base is not None else P
            piv = mbr_mod.labels(arrays["ids"][i, P], arrays["lens"][i, P], eos)
            order = mbr_mod.pivot_first(arrays, i, P, nh)
            orders[slot] = order if base is None else np.asarray(base)[order]
            out[slot] = {"mbr": mbr_mod.summary(e, am), "tokens": mbr_mod.token_records(e, piv, self.token_list)}
        return out, orders

    def _consensus_ctc(self, out: dict, pending: list):
        """ONE call for the round's finals of decoder-free sessions, over their ``ctc_nbest`` as it stands (re-ranked or
        not; with a grammar over the group that leads the list, so "complete entries first" stays outermost); with
        ``consensus=True`` the pivot moves to the front of its group and the reply's results follow"""
        groups = []
        for sid, has_gr in pending:
            nb = out[sid].ctc_nbest
            g = len(nb)
            if has_gr:
                g = next((k for k, e in enumerate(nb) if e.get("complete") != nb[0].get("complete")), len(nb))
            groups.append(min(g, mbr_mod.MAX_HYPS))
        pinned = self.consensus == "confidence"
        got = self.batch.mbr_lists([[list(e["ids"]) for e in out[sid].ctc_nbest[:g]] for (sid, _), g in zip(pending, groups)],
                                   [[float(e["score"]) for e in out[sid].ctc_nbest[:g]] for (sid, _), g in zip(pending, groups)],
                                   scale=self.consensus_scale, pivots=[0] * len(pending) if pinned else None)
        for (sid, _), g, e in zip(pending, groups, got):
            old, P = out[sid], int(e["pivot"])
            if P < 0:
                continue
            nb = list(old.ctc_nbest)
            piv = nb[P]
            am = int(piv.get("am_rank", P))
            if P > 0:
                nb = [piv] + nb[:P] + nb[P + 1:]
                res = CtcBeamResults(self._ctc_results(nb))
                for k in ("alignment", "activity", "detections", "draft", "ahead", "level", "stable", "rescored",
                          "grammar_complete"):
                    setattr(res, k, getattr(old, k, None))
                res.ctc_nbest = nb
                if old.alignment is not None and len(res):
                    res.alignment = self._ctc_alignment(res)
                out[sid] = res
            names = None if self.token_list is None else self.token_list
            out[sid].consensus = {"mbr": mbr_mod.summary(e, am), "tokens": mbr_mod.token_records(e, piv["ids"], names)}

    def enable_attention_rescore(self, spec=True):
        """switch the ``attention_rescore`` option on: True, or (w_att, w_ctc[, beta]); None / False switches it off"""
        if spec is None or spec is False:
            self.attention_rescore = None
            return
        if self.ctc_beam is None:
            raise ValueError("attention_rescore needs the ctc_beam option (StreamScheduler(ctc_beam=...))")
        if not hasattr(self.batch, "attention_rescore_beam"):
            raise NotImplementedError("attention rescoring runs in the C++ engine (NativeStreamBatch.attention_rescore_beam, "
                                      "sc_attention_rescore_beam); the Python lock-step engine has none")
        w = (1.0, 0.5, 0.0) if spec is True else tuple(float(v) for v in spec)
        if len(w) == 2:
            w = w + (0.0,)
        if len(w) != 3 or not all(np.isfinite(v) for v in w):
            raise ValueError("attention_rescore is True or (w_att, w_ctc[, beta]), all finite")
        self.attention_rescore = w

    @property
    def _eos_id(self) -> int:
        return int(getattr(self.batch.cfg, "eos_id", EOS_ID))

    def enable_stable_partials(self):
        """switch the ``stable_partials`` option on (every session's tracker starts over)"""
        if self.batch.W > commit_mod.MAX_HYPS:
            raise ValueError(f"stable partials compare a beam of at most {commit_mod.MAX_HYPS} hypotheses "
                             f"(this batch has beam {self.batch.W})")
        self.stable_partials = True
        self._stable.clear()

    def enable_alternates(self, k: int):
        """switch the ``alternates`` option on (and ``align_final`` with it)"""
        if not hasattr(self.batch, "alternates"):
            raise NotImplementedError("token alternates are computed by the C++ engine (NativeStreamBatch.alternates); "
                                      "the Python lock-step engine has none")
        if not 1 <= int(k) <= alternates_mod.MAX_K:
            raise ValueError(f"alternates must be in [1, {alternates_mod.MAX_K}]")
        self.alternates = int(k)
        self.align_final = True

    @property
    def _clocked(self) -> bool:   # the options that need the sessions' feature clocks
        return self.align_final or self.spotting or self.draft or self.ctc_beam is not None

    # ---- session lifecycle -------------------------------------------------
    def open(self, sample_rate: int = 16000, format: int = pcm_mod.F32, channels: int = 1, channel: int = pcm_mod.MIX,
             scale: int = pcm_mod.SCALE_FULL, decoder: str = "full", grammar=None) -> int:
        """``decoder``: "full" - the attention search (the default) - or "ctc": a decoder-free session, served from the CTC
        prefix beam search alone (needs the ``ctc_beam`` option and the C++ engine; its replies carry the beam's best as
        their result; a slot goes back to "full" for a later session that does not ask).
        ``grammar`` (needs the ``ctc_beam`` option and the C++ engine): the session's CTC beam answers only from it - a
        compiled blob (speechcatcher_amd.grammar), the path of a .scgr file or of a text file with one phrase per line,
        or a list of phrases (lists of token ids, or strings tokenised by spotting.phrase_ids); see ``set_grammar``.
        ``sample_rate``: rate of the PCM this session feeds (speechcatcher_amd.resample: 8000..48000 Hz; the C++
        engine converts it to 16 kHz on the GPU).  A slot goes back to 16000 for a later session that does not ask.
        ``format`` / ``channels`` / ``channel`` / ``scale``: the wire format of what the session feeds
        (speechcatcher_amd.pcm; default: mono float samples in +-1).  With any other format ``feed`` takes the coded
        bytes, decoded by the engine (on the GPU in the C++ engine's staging step); a slot goes back to float samples
        for a later session that does not ask."""
        sample_rate = check_input_rate(sample_rate)
        fmt = self._check_format(format, channels, channel, scale)
        self._check_decoder(decoder)
        if not self._free:
            raise ServerBusy("Server busy: all stream slots are in use")
        gr_key = self._grammar_key(grammar) if grammar is not None else None
        slot = self._free[0]
        if self.reset_on_open:
            self.batch.reset(slot)
        try:
            self._set_slot_grammar(slot, gr_key)
        finally:
            if gr_key in self._gr_cache and self._gr_cache[gr_key]["uses"] == 0:   # (the set failed)
                self.batch.release_grammar(self._gr_cache.pop(gr_key)["handle"])
        self._set_slot_decoder(slot, "ctc" if decoder == "rescore" else decoder)   # (decoder-free in the engine)
        self._set_slot_rate(slot, sample_rate)
        self._set_slot_format(slot, fmt)
        self._free.popleft()
        sid = self._next_sid
        self._next_sid += 1
        self._slot_of[sid] = slot
        self._queue[sid] = deque()
        self._clock.pop(sid, None)
        self._fed.pop(sid, None)
        self._rate[sid] = OutputClock(sample_rate)
        self._spot_seen.pop(sid, None)
        self._stable.pop(sid, None)
        if fmt != _FLOAT_INPUT:
            self._fmt[sid] = fmt
        if decoder in ("ctc", "rescore"):
            self._ctc_sessions.add(sid)
        if decoder == "rescore":
            self._rescore_sessions.add(sid)
        return sid

    def _check_decoder(self, decoder):
        if decoder not in ("full", "ctc", "rescore"):
            raise ValueError(f'decoder must be "full", "ctc" or "rescore", got {decoder!r}')
        if decoder != "full" and self.ctc_beam is None:
            raise ValueError(f'decoder="{decoder}" needs the ctc_beam option (StreamScheduler(ctc_beam=...))')
        if decoder == "rescore" and self.attention_rescore is None:
            raise ValueError('decoder="rescore" needs the attention_rescore option (StreamScheduler(attention_rescore=...))')
        if decoder != "full" and self.alternates:
            raise ValueError(f'decoder="{decoder}": token alternates rank the frames of a forced alignment against a decode '
                             "block's rows, which a decoder-free session does not have")

    def set_decoder(self, sid: int, decoder: str):
        """Change the decoder of a session that has not fed any audio yet (the Vosk ``config`` message arrives after the
        connection is made).  ValueError for an unknown value, without the ``ctc_beam`` option, or once audio has been fed."""
        self._check_decoder(decoder)
        if decoder == self.decoder(sid):
            return
        if self._rate[sid].fed:
            raise ValueError("the decoder of a session can only be set before its first audio")
        self._set_slot_decoder(self._slot_of[sid], "ctc" if decoder == "rescore" else decoder)
        if decoder in ("ctc", "rescore"):
            self._ctc_sessions.add(sid)
        else:
            self._ctc_sessions.discard(sid)
        self._rescore_sessions.discard(sid)
        if decoder == "rescore":
            self._rescore_sessions.add(sid)
        else:
            self._rescore_sessions.discard(sid)

    def _set_slot_decoder(self, slot: int, decoder: str):
        if self._slot_dec.get(slot, "full") == decoder:
            return
        if not hasattr(self.batch, "set_decoder"):
            raise NotImplementedError('decoder="ctc": decoder-free streams are served by the C++ engine only')
        try:
            self.batch.set_decoder(slot, decoder)
        except RuntimeError as e:     # e.g. a slot that is never reset (strict_reference) and has audio buffered
            raise ValueError(f"decoder {decoder!r} cannot be set on this stream: {e}") from e
        self._slot_dec[slot] = decoder

    def decoder(self, sid: int) -> str:
        return "rescore" if sid in self._rescore_sessions else "ctc" if sid in self._ctc_sessions else "full"

    # ---- a grammar per session ------------------------------
    def _grammar_blob(self, source) -> bytes:
        """``source`` as ``open(grammar=...)`` takes it -> a compiled blob: the blob itself (bytes), the path of a .scgr
        file or of a text file with one phrase per line, or a list of phrases - each a list of token ids or a string,
        tokenised by spotting.phrase_ids against the scheduler's token list"""
        cfg = self.batch.cfg
        if isinstance(source, (bytes, bytearray, memoryview)):
            return bytes(source)
        if isinstance(source, (str, os.PathLike)):
            with open(source, "rb") as fh:
                data = fh.read()
            if data[:4] == b"SCGR":
                return data
            source = [ln.strip() for ln in data.decode("utf-8").splitlines() if ln.strip()]
        phrases = []
        for ph in source:
            if isinstance(ph, str):
                if self.token_list is None:
                    raise ValueError("grammar: phrases given as text need the scheduler's token list")
                ph = phrase_ids(ph, self.token_list)
            phrases.append([int(t) for t in ph])
        return grammar_mod.compile(phrases, cfg.vocab_size, cfg.blank_id)

    def _set_slot_grammar(self, slot: int, key):
        """the slot's grammar becomes the cached one ``key`` (None: none); the cache counts the slots that name an entry and
        frees the device copy with the last"""
        old = self._slot_gr.get(slot)
        if old == key:
            return
        if key is not None and not hasattr(self.batch, "set_stream_grammar"):
            raise NotImplementedError("grammar: this batch has no grammar-constrained CTC beam (set_stream_grammar)")
        try:
            self.batch.set_stream_grammar(slot, self._gr_cache[key]["handle"] if key is not None else None)
        except RuntimeError as e:     # e.g. a slot that is never reset (strict_reference) and has audio buffered
            raise ValueError(f"the grammar cannot be set on this stream: {e}") from e
        if key is not None:
            self._gr_cache[key]["uses"] += 1
        self._slot_gr[slot] = key
        if old is not None:
            entry = self._gr_cache[old]
            entry["uses"] -= 1
            if entry["uses"] == 0:
                self.batch.release_grammar(entry["handle"])
                del self._gr_cache[old]

    def _grammar_key(self, source):
        """the cache entry of ``source`` (compiled and uploaded when it is new), by the blob's SHA-256"""
        if self.ctc_beam is None:
            raise ValueError("grammar needs the ctc_beam option (StreamScheduler(ctc_beam=...))")
        if self.ctc_lm is not None:
            raise ValueError("grammar: a grammar and a fused language model (ctc_lm) together are not served")
        if not hasattr(self.batch, "grammar"):
            raise NotImplementedError("grammar: this batch has no grammar-constrained CTC beam (set_stream_grammar)")
        blob = self._grammar_blob(source)
        key = hashlib.sha256(blob).hexdigest()
        if key not in self._gr_cache:
            try:
                handle = self.batch.grammar(blob)
            except NotImplementedError:
                raise
            except RuntimeError as e:
                raise ValueError(f"grammar: {e}") from e
            self._gr_cache[key] = {"handle": handle, "uses": 0, "walk": grammar_mod.Grammar(blob)}
        return key

    def set_grammar(self, sid: int, source):
        """The grammar of a session that has not fed any audio yet (the Vosk ``config`` message arrives after the connection
        is made): its CTC beam answers only from it; None: none.  ``source``: see ``open``.  ValueError for phrases that
        cannot be compiled, without the ``ctc_beam`` option, with ``ctc_lm``, or once audio has been fed."""
        if self._rate[sid].fed:
            raise ValueError("the grammar of a session can only be set before its first audio")
        slot = self._slot_of[sid]
        if source is None:
            self._set_slot_grammar(slot, None)
            return
        key = self._grammar_key(source)
        try:
            self._set_slot_grammar(slot, key)
        finally:
            if key in self._gr_cache and self._gr_cache[key]["uses"] == 0:   # (the set failed: nobody names the new entry)
                self.batch.release_grammar(self._gr_cache.pop(key)["handle"])

    def grammar(self, sid: int):
        """the host walk (speechcatcher_amd.grammar.Grammar) of the session's grammar, None without one"""
        key = self._slot_gr.get(self._slot_of[sid])
        return self._gr_cache[key]["walk"] if key is not None else None

    @staticmethod
    def _check_format(format, channels, channel, scale) -> tuple:
        try:
            pcm_mod.check_args(format, channels, channel, scale)
        except (ValueError, TypeError) as e:
            raise ValueError(f"input format: {e}") from e
        fmt = (int(format), int(channels), int(channel), int(scale))
        return _FLOAT_INPUT if fmt[:2] == _FLOAT_INPUT[:2] else fmt

    def _set_slot_format(self, slot: int, fmt: tuple):
        if self._slot_fmt.get(slot, _FLOAT_INPUT) == fmt:
            return
        if not hasattr(self.batch, "set_input_format"):
            raise NotImplementedError(f"input format {fmt}: this batch takes mono float samples only")
        try:
            self.batch.set_input_format(slot, *fmt)
        except RuntimeError as e:     # e.g. a slot that is never reset (strict_reference) and has audio buffered
            raise ValueError(f"input format {fmt} cannot be set on this stream: {e}") from e
        self._slot_fmt[slot] = fmt

    def input_format(self, sid: int) -> tuple:
        return self._fmt.get(sid, _FLOAT_INPUT)

    def set_input_format(self, sid: int, format: int = pcm_mod.F32, channels: int = 1, channel: int = pcm_mod.MIX,
                         scale: int = pcm_mod.SCALE_FULL):
        """Change the wire format of a session that has not fed any audio yet (the Vosk ``config`` message arrives
        after the connection is made).  ValueError for a value out of range or once audio has been fed."""
        fmt = self._check_format(format, channels, channel, scale)
        if fmt == self.input_format(sid):
            return
        if self._rate[sid].fed:
            raise ValueError("the input format of a session can only be set before its first audio")
        self._set_slot_format(self._slot_of[sid], fmt)
        if fmt != _FLOAT_INPUT:
            self._fmt[sid] = fmt
        else:
            self._fmt.pop(sid, None)

    def _set_slot_rate(self, slot: int, rate: int):
        if self._slot_rate.get(slot, 16000) == rate:
            return
        if not hasattr(self.batch, "set_input_rate"):
            raise NotImplementedError(f"sample rate {rate}: this batch takes 16 kHz PCM only (the native engine converts)")
        try:
            self.batch.set_input_rate(slot, rate)
        except NotImplementedError:   # the Python lock-step engine: 16 kHz only
            raise
        except RuntimeError as e:     # e.g. a slot that is never reset (strict_reference) and has audio buffered
            raise ValueError(f"sample rate {rate} cannot be set on this stream: {e}") from e
        self._slot_rate[slot] = rate

    def sample_rate(self, sid: int) -> int:
        return self._rate[sid].rate

    def set_sample_rate(self, sid: int, sample_rate: int):
        """Change the rate of a session that has not fed any audio yet (the Vosk ``config`` message arrives after the
        connection is made).  ValueError for an unsupported rate or once audio has been fed."""
        sample_rate = check_input_rate(sample_rate)
        clock = self._rate[sid]
        if sample_rate == clock.rate:
            return
        if clock.fed:
            raise ValueError(f"the sample rate of a session can only be set before its first audio (it is {clock.rate})")
        self._set_slot_rate(self._slot_of[sid], sample_rate)
        self._rate[sid] = OutputClock(sample_rate)

    def close(self, sid: int):
        while sid in self._in_flight:        # its chunks must be reported before the slot can be reset;
            for k, v in self.pump(1, _collect=False, _feed=False).items():   # replies of OTHER sessions wait for their pump()
                if k != sid:
                    self._stash.setdefault(k, deque()).append(v)
        self._stash.pop(sid, None)
        slot = self._slot_of.pop(sid)
        self._queue.pop(sid)
        self._clock.pop(sid, None)
        self._fed.pop(sid, None)
        self._rate.pop(sid, None)
        self._fmt.pop(sid, None)
        self._spot_seen.pop(sid, None)
        self._stable.pop(sid, None)
        self._ctc_sessions.discard(sid)
        if self.reset_on_open:
            self.batch.reset(slot)
        if self._slot_gr.get(slot) is not None:   # the session's grammar goes with it (the cache frees it with its last user)
            try:
                self._set_slot_grammar(slot, None)
            except ValueError:                    # a slot that is never reset: it keeps the grammar until it is opened again
                pass
        self._free.append(slot)

    @property
    def n_active(self) -> int:
        return len(self._slot_of)

    # ---- data path -----------------------------------------------------------
    def feed(self, sid: int, pcm: np.ndarray, is_final: bool = False, finalize_all: bool = False):
        """Queue one chunk of a session (float PCM in +-1, like the reference API) at the session's sample rate; a
        session with a wire format (``open(format=...)``) feeds the coded bytes of whole sample frames instead: bytes,
        memoryview or an integer array."""
        fmt = self._fmt.get(sid)
        if fmt is None:
            self._queue[sid].append((np.asarray(pcm, dtype=np.float32), bool(is_final), bool(finalize_all)))
            n_in = int(np.shape(pcm)[0])
        else:
            raw = pcm_mod.as_bytes(pcm).copy()
            bpf = pcm_mod.bytes_per_frame(fmt[0], fmt[1])
            if raw.size % bpf:
                raise ValueError(f"{raw.size} bytes are not a whole number of {bpf}-byte sample frames")
            self._queue[sid].append((raw, bool(is_final), bool(finalize_all)))
            n_in = raw.size // bpf
        n16 = self._rate[sid].call(n_in, bool(is_final))   # the call in 16 kHz samples: the engine's clock
        if self._clocked:
            self._fed.setdefault(sid, deque()).append((n16, bool(is_final)))

    def pending(self) -> int:
        return sum(1 for sid, q in self._queue.items() if q or sid in self._in_flight or sid in self._stash)

    def _take_queued(self, skip=()):
        """the next queued chunk of every session that may hand one over: none at the engine (``skip`` = the sessions
        that have), or - queue depth > 1 - fewer than the depth and no final chunk among them"""
        items, meta = [], {}
        for sid, q in self._queue.items():
            fl = skip.get(sid) if isinstance(skip, dict) else (True if sid in skip else None)
            if fl is not None and (self.queue_depth <= 1 or len(fl) >= self.queue_depth or fl[-1][1]):
                continue
            if q:
                pcm, fin, fa = q.popleft()
                slot = self._slot_of[sid]
                items.append((slot, pcm, fin))
                meta[sid] = (slot, fin, fa)
        return items, meta

    def _results(self, has: dict, meta: Dict[int, Tuple[int, bool, bool]]) -> Dict[int, list]:
        """replies of the sessions in `meta` ({session: (slot, is_final, finalize_all)}) whose engine call returned
        `has[slot]`: ONE device round trip for the hypotheses of all of them (sc_get_hyps_batch)"""
        out: Dict[int, list] = {}
        want = [slot for (slot, _, _) in meta.values() if has[slot] is True]
        arrays = hyps = None
        if want:
            if hasattr(self.batch, "hypotheses_arrays"):
                arrays = self.batch.hypotheses_arrays(want)
                row = {slot: i for i, slot in enumerate(want)}
            else:
                hyps = {slot: self.batch.hypotheses(slot) for slot in want}
        perm = {}
        if self.final_lm is not None and arrays is not None:   # ONE launch and one copy back for the round's finals
            fins = [slot for sid, (slot, fin, _) in meta.items()
                    if fin and has[slot] is True and sid not in self._ctc_sessions]
            if fins:
                a, b, eos = self.final_lm
                got = self.batch.rescore_hyps(fins, self._final_dev, a, b, lm_eos=self._eos_id if eos else -1, final=fins,
                                              nbest=arrays["ids"].shape[1])
                for slot in fins:
                    perm[slot] = rescore_mod.rerank_arrays(arrays, row[slot], got[slot])
        cons, cperm, cons_ctc = {}, {}, []
        if self.consensus is not None and arrays is not None:   # ONE call and one copy back for the round's finals
            fins = [slot for sid, (slot, fin, _) in meta.items()
                    if fin and has[slot] is True and sid not in self._ctc_sessions]
            if fins:
                cons, cperm = self._consensus_full(arrays, row, fins, perm)
        act = act_row = None
        if self.activity:
            act_slots = [slot for (slot, _, _) in meta.values() if not isinstance(has[slot], Exception)]
            act_row = {slot: i for i, slot in enumerate(act_slots)}
            act = self.batch.activity(act_slots) if act_slots else None
        delta = None
        if self.stable_partials:
            ask = [(sid, slot) for sid, (slot, _, _) in meta.items() if not isinstance(has[slot], Exception)]
            if ask:
                held = [self._stable.setdefault(sid, commit_mod.StablePrefix()).next_from for sid, _ in ask]
                delta = self.batch.hyps_delta([slot for _, slot in ask], held,
                                              final=[slot for sid, slot in ask if meta[sid][1]])
        beams, sides = None, {}
        if self.ctc_beam is not None:   # ONE launch and one copy back for the round (sc_ctc_beam_hyps)
            ask = [slot for (slot, _, _) in meta.values() if not isinstance(has[slot], Exception)]
            beams = self.batch.ctc_beam_hyps(ask, self.ctc_beam[0]) if ask else {}
            if self.ctc_lm is not None and ask:   # the model's side of the same entries (host arithmetic, no launch)
                sides = dict(zip(ask, self.batch.ctc_beam_lm(ask, self.ctc_beam[0])))
        att = {}
        if self.attention_rescore is not None and beams is not None:   # ONE call and one copy back for the round's finals
            fins = [slot for sid, (slot, fin, _) in meta.items()
                    if fin and has[slot] is True and sid in self._rescore_sessions and beams.get(slot)]
            if fins:
                att = self.batch.attention_rescore_beam(fins, self.ctc_beam[0], *self.attention_rescore)
        for sid, (slot, fin, fa) in meta.items():
            if self._clocked and self._fed.get(sid):   # the stream's clock advances by the reported chunk
                n, f = self._fed[sid].popleft()
                cfg = self.batch.cfg
                self._clock.setdefault(sid, FeatureClock(cfg.win_length, cfg.hop_length)).call(n, f)
            if isinstance(has[slot], Exception):
                out[sid] = has[slot]          # the engine has reset the stream
                self._clock.pop(sid, None)
                self._spot_seen.pop(sid, None)
                self._stable.pop(sid, None)
                continue
            rescored = None
            if not has[slot]:
                out[sid] = []
            elif arrays is not None:
                kept = _select_hyps(arrays, row[slot], fin, fa)
                out[sid] = hyps_to_results(kept, fin, fa, self.token_list, self.result_format)
                if slot in perm:
                    rescored = [{k: h[k] for k in ("score", "lm", "fused", "am_rank")} for h in kept]
            else:
                out[sid] = hyps_to_results(hyps[slot], fin, fa, self.token_list, self.result_format)
            if fin and self.align_final and not isinstance(out[sid], Exception) and sid not in self._ctc_sessions:
                out[sid] = self._aligned(out[sid], arrays, row[slot] if arrays is not None and has[slot] is True else None,
                                         slot, fin, fa, self._clock.get(sid), cperm.get(slot, perm.get(slot)))
            if rescored is not None:
                if not isinstance(out[sid], AlignedResults):
                    out[sid] = AlignedResults(out[sid])
                out[sid].rescored = rescored
            if act is not None:
                res = ActivityResults(out[sid])
                res.alignment, res.rescored = getattr(out[sid], "alignment", None), getattr(out[sid], "rescored", None)
                res.activity = activity_of_stream(act, act_row[slot])
                out[sid] = res
            if self.spotting:
                res = SpottingResults(out[sid])
                res.alignment, res.rescored = getattr(out[sid], "alignment", None), getattr(out[sid], "rescored", None)
                res.activity = getattr(out[sid], "activity", None)
                res.detections = self._detections(sid, slot)
                out[sid] = res
            if self.draft:
                res = DraftResults(out[sid])
                for k in ("alignment", "activity", "detections", "rescored"):
                    setattr(res, k, getattr(out[sid], k, None))
                res.draft = self._draft_tokens(sid, slot)
                pos = out[sid][0][3] if out[sid] and len(out[sid][0]) > 3 else None
                res.ahead = draft_mod.ahead(res.draft, pos[-1] if pos else 0)
                out[sid] = res
            if self.input_level:
                res = LevelResults(out[sid])
                for k in ("alignment", "activity", "detections", "draft", "ahead", "rescored"):
                    setattr(res, k, getattr(out[sid], k, None))
                res.level = self.batch.input_level(slot) if hasattr(self.batch, "input_level") else pcm_mod.zero_level()
                out[sid] = res
            if delta is not None:
                res = StableResults(out[sid])
                for k in ("alignment", "activity", "detections", "draft", "ahead", "level", "rescored"):
                    setattr(res, k, getattr(out[sid], k, None))
                res.stable = self._stable[sid].update(delta[slot], final=fin).state()   # (a final starts the tracker over)
                out[sid] = res
            if beams is not None:
                nbest = self._ctc_nbest(sid, beams[slot], sides.get(slot))
                gr_key = self._slot_gr.get(slot)
                if gr_key is not None:   # the accept flags of the same entries (host arithmetic, no launch), read before
                    # the list is re-ordered
                    flags = self.batch.ctc_beam_hyps_grammar([slot], self.ctc_beam[0])[slot]
                    for e, (_, acc) in zip(nbest, flags):
                        e["complete"] = bool(acc)
                if slot in att and nbest:
                    nbest = self._attention_reranked(nbest, att[slot])
                if gr_key is not None and fin:   # a final: the complete entries first, each group in its order
                    nbest = [e for e in nbest if e["complete"]] + [e for e in nbest if not e["complete"]]
                if fin and self.final_lm_eos and self.ctc_lm is not None and sid in self._ctc_sessions and nbest:
                    nbest = self._ctc_end_term(nbest, after_attention=slot in att)
                # a decoder-free session: its results are the beam's entries, best first (a chunk the engine answers with
                # nothing stays [])
                free = sid in self._ctc_sessions
                res = CtcBeamResults(self._ctc_results(nbest) if free and has[slot] else out[sid])
                for k in ("alignment", "activity", "detections", "draft", "ahead", "level", "stable", "rescored"):
                    setattr(res, k, getattr(out[sid], k, None))
                res.ctc_nbest = nbest
                if gr_key is not None:
                    res.grammar_complete = bool(nbest and nbest[0]["complete"])
                if free and fin and self.align_final and len(res):
                    res.alignment = self._ctc_alignment(res)
                out[sid] = res
                if free and fin and self.consensus is not None and has[slot] and nbest and hasattr(self.batch, "mbr_lists"):
                    cons_ctc.append((sid, gr_key is not None))
            if slot in cons:
                if not isinstance(out[sid], AlignedResults):
                    out[sid] = AlignedResults(out[sid])
                out[sid].consensus = cons[slot]
            if fin and self.reset_after_final:
                self.batch.reset(slot)
                self._clock.pop(sid, None)
                self._spot_seen.pop(sid, None)
        if cons_ctc:
            self._consensus_ctc(out, cons_ctc)
        return out

    def _ctc_nbest(self, sid: int, hyps: list, side: Optional[dict] = None) -> list:
        """the n-best list of the session's beam (``hyps``: its entries as batch.ctc_beam_hyps gives them; ``side``: the
        language model's side of them when one is attached): frames, and seconds by the session's feature clock"""
        cfg = self.batch.cfg
        out = beam_mod.nbest(hyps, names=self.token_list, side=side)
        clock = self._clock.get(sid) or FeatureClock(cfg.win_length, cfg.hop_length)
        for entry, h in zip(out, hyps):
            secs = beam_mod.token_dicts(h, clock, cfg.subsample, cfg.sample_rate)
            for d, t in zip(entry["tokens"], secs):
                d["start_s"], d["end_s"] = t["start"], t["end"]
        return out

    def _attention_reranked(self, nbest: list, got: dict) -> list:
        """the final n-best list of a "rescore" session after the attention pass (``got``: its entry of
        batch.attention_rescore_beam): re-ordered; "att" the decoder's log probability of the entry's labels and <eos>,
        "ctc_score" its first-pass total, "am_rank" its rank in the beam, "score" the fused total, "conf" from the new
        totals"""
        out = []
        for r in got["order"][:len(nbest)]:
            r = int(r)
            if r >= len(nbest):
                continue
            e = dict(nbest[r])
            e.setdefault("ctc_score", e["score"])
            e["first_pass"], e["att"], e["am_rank"] = float(got["ctc_score"][r]), float(got["att"][r]), r
            e["score"] = float(got["fused"][r])
            out.append(e)
        for e, c in zip(out, alternates_mod.nbest_posterior([e["score"] for e in out])):
            e["conf"] = c
        return out

    def _ctc_end_term(self, nbest: list, after_attention: bool = False) -> list:
        """the final n-best list of a decoder-free session with the </s> term of the fused model: rescored as a
        caller-given list at the beam's weights (one launch), re-ranked; "score" is the fused total with the term,
        "eos_lm" the term, "am_rank" the entry's rank in the beam, "conf" from the new totals"""
        if self._ctc_dev is None:
            self._ctc_dev = self.batch.language_model(self._ctc_blob)
        a, b = self.ctc_lm
        got = self.batch.rescore_lists([[e["ids"] for e in nbest]], [[e["ctc_score"] for e in nbest]], self._ctc_dev, a, b,
                                       lm_eos=self._eos_id)[0]
        out = []
        if after_attention:   # the term is added to the attention-fused totals; ties keep the attention pass's order
            rows = [dict(e, score=float(e["score"] + a * float(got["eos_lm"][r])), eos_lm=float(got["eos_lm"][r]))
                    for r, e in enumerate(nbest)]
            finite = [e for e in rows if np.isfinite(e["score"])]
            out = sorted(finite, key=lambda e: -e["score"]) + [e for e in rows if not np.isfinite(e["score"])]
        for r in ([] if after_attention else got["order"]):
            e = dict(nbest[int(r)])
            e["score"], e["eos_lm"], e["am_rank"] = float(got["fused"][r]), float(got["eos_lm"][r]), int(r)
            out.append(e)
        for e, c in zip(out, alternates_mod.nbest_posterior([e["score"] for e in out])):
            e["conf"] = c
        return out

    def _ctc_results(self, nbest: list) -> list:
        """the beam's entries as the results of a reply, best first, in the scheduler's result format - the reply's text is
        the beam's best; no result while the best prefix is empty, and an empty prefix further down is left out"""
        if not nbest or not nbest[0]["ids"]:
            return []
        out = []
        for e in nbest:
            if not e["ids"]:
                continue
            toks = [t.get("token", str(t["id"])) for t in e["tokens"]]
            if self.result_format == "espnet":
                out.append((e["text"], toks, list(e["ids"]), [t["start"] for t in e["tokens"]], e))
            else:
                out.append((e["text"], toks, list(e["ids"])))
        return out

    def _ctc_alignment(self, res: list) -> dict:
        """``align_final`` for a decoder-free session: sc_align_tokens aligns against the rows of a stream's last decode
        block, which such a stream does not have, so the times are the prefix tree's - a token runs from the frame at
        which its prefix entered the beam to the frame before the next token's; conf 1.0 (the search gives a probability
        per prefix, none per token).  The shape of result_token_alignment, "nbest" with ``align_nbest`` > 1."""
        def one(entry):
            t = entry["tokens"]
            return {"token_ids": [d["id"] for d in t], "start_s": [d["start_s"] for d in t],
                    "end_s": [d["end_s"] for d in t], "conf": [1.0] * len(t), "source": "ctc_beam"}

        entries = [r[4] for r in res] if self.result_format == "espnet" else [e for e in res.ctc_nbest if e["ids"]]
        al = one(entries[0])
        if self.align_nbest > 1:
            al["nbest"] = [dict(al)] + [one(e) for e in entries[1:self.align_nbest]]
        return al

    def _draft_tokens(self, sid: int, slot: int) -> list:
        """the draft of the session's stream as token dicts: frames, and seconds by the session's feature clock"""
        cfg = self.batch.cfg
        toks = self.batch.draft_tokens(slot)
        out = draft_mod.token_dicts(toks, names=self.token_list)
        secs = draft_mod.token_dicts(toks, self._clock.get(sid) or FeatureClock(cfg.win_length, cfg.hop_length),
                                     cfg.subsample, cfg.sample_rate)
        for d, t in zip(out, secs):
            d["start_s"], d["end_s"] = t["start"], t["end"]
        return out

    def _detections(self, sid: int, slot: int) -> list:
        """the stored events of the session's utterance that have not gone out yet (each goes out once)"""
        seen = self._spot_seen.get(sid, 0)
        n = min(int(self.batch.spot([slot])["n_events"][0]), spotting.MAX_EVENTS)
        if n <= seen:
            return []
        cfg = self.batch.cfg
        new = self.batch.spot_events(slot)[seen:n]
        self._spot_seen[sid] = n
        out = spotting.event_dicts(new)
        secs = spotting.event_dicts(new, self._clock.get(sid) or FeatureClock(cfg.win_length, cfg.hop_length),
                                    cfg.subsample, cfg.sample_rate)
        for d, t in zip(out, secs):
            d["start_s"], d["end_s"] = t["start"], t["end"]
        return out

    def _aligned(self, res: list, arrays, i, slot: int, fin: bool, fa: bool, clock, perm=None) -> "AlignedResults":
        """``perm`` (a re-ranked final): row q of ``arrays`` is the engine's row perm[q] - the alignment is asked for a list
        wide enough to hold the rows reported and read at THEIR rows"""
        out = AlignedResults(res)
        if not res or arrays is None:
            return out
        # the hypothesis behind res[0]: the first one _select_hyps keeps
        # (with align_nbest > 1: the hypotheses behind res[:align_nbest], in the order _select_hyps keeps them)
        js = [j for j in range(int(arrays["n_hyps"][i]))
              if (fin and fa) or int(arrays["ids"][i, j, int(arrays["lens"][i, j]) - 1]) == EOS_ID][:self.align_nbest]
        ys = [arrays["ids"][i, q, :int(arrays["lens"][i, q])].tolist() for q in js]
        if perm is not None:
            js = [int(perm[q]) for q in js]
        j = js[0]
        if self.alternates:
            al = self.batch.alternates([slot], max(js) + 1, self.alternates)
        else:
            al = self.batch.align([slot], max(js) + 1)
        out.alignment = result_token_alignment(ys[0], fin, al, 0, j, self.batch.cfg, clock)
        if self.alternates:
            out.alignment["alternates"] = alternates_mod.result_token_alternates(ys[0], fin, al, 0, j, self.batch.cfg,
                                                                                 self.token_list)
        if self.align_nbest > 1:
            out.alignment["nbest"] = [dict(out.alignment)] + [
                result_token_alignment(y, fin, al, 0, q, self.batch.cfg, clock) for y, q in zip(ys[1:], js[1:])]
        return out

    def step(self) -> Dict[int, list]:
        """One batched chunk step over every session that has a chunk queued
        (at most one chunk per session: per-stream order is preserved).
        Returns {session: results} in the reference's tuple format; a final
        chunk resets the slot's stream state afterwards, like the reference
        callers do (speechcatcher.py:618-619).

        Fault isolation: a session whose chunk cannot be processed (capacity limit, or an input
        the reference itself raises on, e.g. a final chunk of <7 feature frames) gets the
        EXCEPTION OBJECT as its result and its stream is reset; the other sessions of the step
        are decoded as if it had not been there (in the reference an exception ends only that
        client's handler: every client owns a model instance)."""
        items, meta = self._take_queued()
        if not items:
            return {}
        has = self.batch.push(items, isolate_faults=True)
        return self._results(has, meta)

    # ---- continuous batching ------------------------------------------------------
    def pump(self, min_done: int = 1, _collect: bool = True, _feed: bool = True) -> Dict[int, list]:
        """Continuous batching (C++ engine: sc_submit / sc_poll).  Hands the engine the next queued chunk of every
        session that has none in flight - ONE admission group - and then lets it decode until at least ``min_done``
        replies are ready.  A session's reply is delivered when ITS decode blocks are done: sessions that finish
        early are fed again by the next pump() while the stragglers of this group are still decoding, so the streams
        leave lock-step and every decode iteration runs with (nearly) all of them.  Per session the calls and their
        results are those of ``step()`` (the reference's session loop: call, reply, next call -
        speechcatcher_server.py:359-397).  Returns {session: results} of the replies that became ready."""
        if not hasattr(self.batch, "submit"):
            return self.step()                      # the Python engine has no resumable decode loop any more
        for _ in range(self.queue_depth if _feed else 0):     # one chunk per session and submit call
            items, meta = self._take_queued(skip=self._in_flight)
            if not items:
                break
            self.batch.submit(items)
            for sid, m in meta.items():
                self._in_flight.setdefault(sid, deque()).append(m)
        n_ready = len(self._stash) if _collect else 0           # sessions with a reply waiting from an earlier call
        new: Dict[int, list] = {}
        if self._in_flight and n_ready < min_done:
            has = self.batch.poll(max(1, min(min_done - n_ready, len(self._in_flight))), isolate_faults=True)
            sid_of = {fl[0][0]: sid for sid, fl in self._in_flight.items()}
            done = {}
            for slot in has:                       # one reply per session and poll: that of its OLDEST chunk at the engine
                sid = sid_of[slot]
                done[sid] = self._in_flight[sid].popleft()
                if not self._in_flight[sid]:
                    del self._in_flight[sid]
            new = self._results(has, done)
        if not _collect:
            return new                             # close(): the caller parks them
        for sid, res in new.items():               # behind what the session already has waiting: replies stay in order
            self._stash.setdefault(sid, deque()).append(res)
        out: Dict[int, list] = {}
        for sid in list(self._stash):
            out[sid] = self._stash[sid].popleft()
            if not self._stash[sid]:
                del self._stash[sid]
        return out

    @property
    def n_in_flight(self) -> int:
        return len(self._in_flight)

    def drain(self) -> Dict[int, list]:
        """Run steps until every queue is empty; returns the LAST result of each session.  On the C++ engine through the
        continuous path (``pump``: sc_submit / sc_poll) - per session the same calls and replies as ``step``."""
        last: Dict[int, list] = {}
        cont = hasattr(self.batch, "submit")
        while self.pending():
            for sid, res in (self.pump() if (cont or self._in_flight or self._stash) else self.step()).items():
                if isinstance(res, Exception):
                    raise res
                last[sid] = res
        return last


def _select_hyps(a: dict, i: int, is_final: bool, finalize_all: bool) -> List[dict]:
    out = _select_plain(a, i, is_final, finalize_all)
    if "am_rank" in a and int(a["am_rank"][i, 0]) >= 0:   # a re-ranked final (rescore.rerank_arrays)
        for h in out:
            j = h.pop("_row")
            h["lm"], h["fused"], h["am_rank"] = float(a["lm"][i, j]), float(a["fused"][i, j]), int(a["am_rank"][i, j])
    else:
        for h in out:
            del h["_row"]
    return out


def _select_plain(a: dict, i: int, is_final: bool, finalize_all: bool) -> List[dict]:
    """hypothesis dicts of row i of ``hypotheses_arrays`` - only those the reference's result assembly looks at
    (speech2text_streaming.py:469-476: without finalize_all only hypotheses that end in <eos>), so that a partial
    reply does not turn W x L token ids into Python lists"""
    out = []
    for j in range(int(a["n_hyps"][i])):
        L = int(a["lens"][i, j])
        if not (is_final and finalize_all) and int(a["ids"][i, j, L - 1]) != EOS_ID:
            continue
        out.append({"yseq": a["ids"][i, j, :L].tolist(), "score": float(a["score"][i, j]),
                    "score_dec": float(a["score_dec"][i, j]), "score_ctc": float(a["score_ctc"][i, j]),
                    "xpos": a["xpos"][i, j, :L].tolist(), "_row": j})
    return out


def recognize_segments(batch: StreamBatch, speech: np.ndarray, segments: List[Tuple[int, int]],
                       chunk_length: int = 8192, token_list: Optional[List[str]] = None,
                       frames_per_second: float = 24.0, finalize_all_last_only: bool = False,
                       queue_depth: int = 1, token_alignment: bool = False, token_alternates: int = 0,
                       ctc_beam=None, ctc_only: bool = False, ctc_lm=None, lm_weight: float = 0.5,
                       word_bonus: float = 0.0, rescore_lm=None, rescore_weight: float = 0.5,
                       rescore_bonus: float = 0.0, ctc_grammar=None, attention_rescore=None, consensus=None) -> List[dict]:
    """Decode the (start, end) sample ranges of one recording as PARALLEL streams
    of one batch instead of the reference's process pool over segments
    (speechcatcher/speechcatcher.py:474-497, chunk loop :574-592; SURVEY 8(f)
    rank 2).  Every segment is fed in ``chunk_length`` pieces, the last one with
    is_final=finalize_all=True.  Token timestamps follow the reference's
    convention: encoder-frame position / 24.0 s + segment start
    (speechcatcher.py:48,509-536).  ``token_alignment`` (C++ engine): every segment also gets ``token_start`` /
    ``token_end`` / ``token_conf`` per token, from a CTC forced alignment of its result (seconds of the recording; None
    for a token without one).  ``token_alternates`` = K > 0 (implies ``token_alignment``): also ``token_alternates``,
    one record per token with its K acoustic alternates (speechcatcher_amd.alternates).  ``ctc_beam`` = B or (B, C): every
    segment also gets ``ctc_nbest``, the n-best list of the CTC prefix beam search over it ({"text", "score", "conf"} per
    entry, best first).  ``ctc_only`` (implies ``ctc_beam``, default (8, 8)): the segments are decoder-free
    streams - text, tokens and token_timestamps are the beam's best, token_start / token_end the prefix tree's frames; not
    with ``token_alternates``.  ``ctc_lm`` (needs ``ctc_beam`` or ``ctc_only``): a packed n-gram model fused into that
    search with ``lm_weight`` / ``word_bonus``; the entries of ``ctc_nbest`` then carry "lm" too and their
    "score" is the fused total.  ``rescore_lm`` (C++ engine; not with ``ctc_only``): a packed n-gram model the final n-best
    list of every segment is rescored with and re-ranked by, </s> term included, at ``rescore_weight`` / ``rescore_bonus``
    (the scheduler's ``final_lm`` option): the segment's text is the fused best, "score" stays its search
    score, "lm_score" / "fused_score" / "am_rank" say what the model added and which row of the search's list it was.
    ``ctc_grammar`` (needs ``ctc_beam`` or ``ctc_only``; not with ``ctc_lm``): every segment's CTC beam answers only from
    this grammar (``StreamScheduler.open(grammar=...)``); the entries of ``ctc_nbest`` carry "complete".
    ``consensus`` (C++ engine): True or "confidence" - the scheduler's option of that name: with True a
    segment's text is the minimum-Bayes-risk row of its final n-best list; with both a segment gets ``token_consensus``
    (per token the share of the list's mass behind it), ``token_rival`` (per token {"id", "token", "mass"} or None) and
    ``mbr`` ([{"pivot", "risk", "am_rank"}])."""
    token_alignment = token_alignment or token_alternates > 0
    if rescore_lm is not None and ctc_only:
        raise ValueError("rescore_lm re-ranks the n-best list of the attention decoder's search: not with ctc_only "
                         "(fuse the model into the CTC beam with ctc_lm)")
    if ctc_lm is not None and not (ctc_only or beam_mod.params(ctc_beam)):
        raise ValueError("ctc_lm: the model is fused into the CTC prefix beam search - it needs ctc_beam or ctc_only")
    if ctc_grammar is not None and not (ctc_only or beam_mod.params(ctc_beam)):
        raise ValueError("ctc_grammar: the grammar constrains the CTC prefix beam search - it needs ctc_beam or ctc_only")
    if ctc_grammar is not None and ctc_lm is not None:
        raise ValueError("ctc_grammar: a grammar and a fused language model (ctc_lm) together are not served")
    if ctc_only and token_alternates:
        raise ValueError("ctc_only: token alternates rank the frames of a forced alignment against a decode block's rows, "
                         "which a decoder-free stream does not have")
    # ``attention_rescore`` (only with ``ctc_only``): True or (w_att, w_ctc[, beta]) - every segment is a "rescore" session,
    # its final ``ctc_nbest`` re-ranked by one pass of the attention decoder (the scheduler's option)
    if attention_rescore is not None and attention_rescore is not False and not ctc_only:
        raise ValueError("attention_rescore re-ranks the n-best list of a decoder-free segment: it needs ctc_only")
    if ctc_only and not beam_mod.params(ctc_beam):
        ctc_beam = beam_mod.DEFAULT
    # queue_depth > 1 (C++ engine): that many chunks of a segment at the engine - the audio is all there.  Measured: worth
    # +6..12 % when the search is decode-heavy (no block-boundary detection, <= 32 segments), nothing to -8 % with
    # detection on (the CLI's default), hence off by default
    sch = StreamScheduler(batch, token_list, result_format="espnet", queue_depth=queue_depth, align_final=token_alignment,
                          alternates=token_alternates, ctc_beam=ctc_beam, ctc_lm=ctc_lm, lm_weight=lm_weight,
                          word_bonus=word_bonus, final_lm=rescore_lm, final_lm_weight=rescore_weight,
                          final_word_bonus=rescore_bonus, final_lm_eos=rescore_lm is not None,
                          attention_rescore=attention_rescore, consensus=consensus)
    free = "rescore" if sch.attention_rescore is not None else "ctc"
    out: List[Optional[dict]] = [None] * len(segments)
    todo = list(enumerate(segments))
    sid_to_seg: Dict[int, int] = {}
    while todo or sch.n_active:
        while todo and sch._free:
            idx, (a, b) = todo.pop(0)
            sid = sch.open(decoder=free if ctc_only else "full", **({} if ctc_grammar is None else {"grammar": ctc_grammar}))
            sid_to_seg[sid] = idx
            seg = speech[a:b]
            for pos in range(0, len(seg), chunk_length):
                end = min(pos + chunk_length, len(seg))
                last = end >= len(seg)
                # the reference CLI passes finalize_all only with the very last chunk of the
                # recording (speechcatcher.py:586): earlier segments then return only beams that
                # ended in <eos> (A5); the default here returns the best beam of every segment
                fa = last and (not finalize_all_last_only or idx == len(segments) - 1)
                sch.feed(sid, seg[pos:end], is_final=last, finalize_all=fa)
        # (C++ engine: continuous batching - a segment that is answered gets its next chunk while the others decode)
        for sid, res in sch.pump().items():
            if isinstance(res, Exception):
                raise res
            if not sch._queue[sid] and sid not in sch._in_flight and sid not in sch._stash:    # the final chunk's reply
                idx = sid_to_seg.pop(sid)
                start_s = segments[idx][0] / 16000.0
                if res:
                    text, toks, ids, pos, hyp = res[0]
                    out[idx] = {"text": text, "tokens": toks, "token_ids": ids,
                                "token_timestamps": [start_s + p / frames_per_second for p in pos],
                                "score": hyp["score"], "start": start_s}
                    if "fused" in hyp:
                        out[idx].update(lm_score=hyp["lm"], fused_score=hyp["fused"], am_rank=hyp["am_rank"])
                else:
                    out[idx] = {"text": "", "tokens": [], "token_ids": [], "token_timestamps": [],
                                "score": 0.0, "start": start_s}
                if sch.ctc_beam is not None:   # (a list of one n-best per segment: paragraphs append them)
                    out[idx]["ctc_nbest"] = [[{k: e[k] for k in ("text", "score", "conf", "lm", "ctc_score", "complete") if k in e}
                                              for e in (getattr(res, "ctc_nbest", None) or [])]]
                cons = getattr(res, "consensus", None)
                if sch.consensus is not None:   # (a list of one record per segment: paragraphs append them)
                    n = len(out[idx]["tokens"])
                    recs = cons["tokens"] if cons is not None and len(cons["tokens"]) == n else None
                    out[idx]["token_consensus"] = [None] * n if recs is None else [r["consensus"] for r in recs]
                    out[idx]["token_rival"] = [None] * n if recs is None else [r.get("rival") for r in recs]
                    out[idx]["mbr"] = [cons["mbr"]] if cons is not None else [None]
                if token_alignment:
                    al = getattr(res, "alignment", None) if res else None
                    n = len(out[idx]["tokens"])
                    if al is None:
                        al = {"start_s": [None] * n, "end_s": [None] * n, "conf": [None] * n}
                    out[idx]["token_start"] = [None if a is None else start_s + a for a in al["start_s"]]
                    out[idx]["token_end"] = [None if b is None else start_s + b for b in al["end_s"]]
                    out[idx]["token_conf"] = list(al["conf"])
                    if token_alternates:
                        recs = al.get("alternates")
                        if recs is None:   # no alignment: records without alternates
                            recs = [alternates_mod.token_record(t, None, None, [], [], token_list)
                                    for t in out[idx]["token_ids"]]
                        out[idx]["token_alternates"] = list(recs)
                sch.close(sid)
    return out  # type: ignore[return-value]
