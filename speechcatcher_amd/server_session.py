"""Server-side sessions on top of the batched scheduler: the per-client logic
of the reference's websocket server (SpeechRecognitionSession,
speechcatcher/speechcatcher_server.py:205-328) without its one-model-copy-per-
client pool - on-the-fly endpointing, Vosk-style JSON replies, eof / reset
control messages, the server's int16 -> float16/32767 input scaling (SURVEY
A10) - driven by ONE ``StreamScheduler`` so that the chunk steps of all
connected clients run as one batch on the GPU.

SURVEY.md section 8(f) rank 1.  The network layer (websockets, ffmpeg
transcoding of webm/mp3 input) stays out of scope: a transport hands
``ServerLoop.submit`` the messages it received and sends back what
``ServerLoop.step`` returns.

Differences to the reference, on purpose:
* token timestamps of final Vosk results are real (encoder frame of the token
  / 24 s, the CLI's convention speechcatcher.py:48) instead of the placeholder
  ``idx * 0.1`` (speechcatcher_server.py:309-311);
* after a finalised utterance, and for every new connection, the stream is reset
  (the native decoder of the reference keeps its finished state after
  ``is_final=True`` - the espnet decoder it replaced reset itself - so the reference
  server goes on decoding into a finalised stream, and a model returned to the pool
  hands its hypotheses to the next client).  ``ServerLoop(strict_reference=True)``
  switches this off and reproduces the reference server call for call;
* only 16 kHz s16le / int16 input (what Vosk clients send); other container
  formats need the transport to transcode first.
"""
import json
import math
from collections import deque
from dataclasses import dataclass
from typing import Deque, Dict, List, Optional, Union

import numpy as np

from .activity import FRAME_SECONDS
from .align import merge_words
from . import mbr as mbr_mod
from . import alternates as alternates_mod
from . import pcm as pcm_mod
from .scheduler import ServerBusy, StreamScheduler
from .speech2text_streaming import TEXT_SKIP_IDS

Message = Union[str, bytes, np.ndarray]
FRAMES_PER_SECOND = 24.0   # speechcatcher.py:48


class Endpointer:
    """On-the-fly endpointing of one session (speechcatcher_server.py:252-268):
    an utterance is finalised when the best partial has had the same length for
    ``finalize_update_iters`` consecutive chunks, or after more than
    ``max_iters`` chunks; the history restarts after every finalisation."""

    def __init__(self, finalize_update_iters: int = 6, max_iters: int = 42):
        self.finalize_update_iters = finalize_update_iters
        self.max_iters = max_iters
        self.n_best_lens: List[int] = []

    def decide(self) -> bool:
        """Called BEFORE a chunk is decoded: finalise this chunk?"""
        n = len(self.n_best_lens)
        if n < self.finalize_update_iters:
            return False
        if n > self.max_iters:
            self.n_best_lens = []
            return True
        tail = self.n_best_lens[-self.finalize_update_iters:]
        if all(x == self.n_best_lens[-1] for x in tail):
            self.n_best_lens = []
            return True
        return False

    def observe(self, partial_len: int):
        """Called after a NON-final chunk that produced a result."""
        self.n_best_lens.append(partial_len)


@dataclass
class EndpointRules:
    """Acoustic endpointing rules in SECONDS of audio (ServerLoop(acoustic_endpointing=...)); an encoder frame is
    0.04 s, a rule of x seconds is ceil(x / 0.04) frames.  Conventional defaults, not tuned on the shipped models."""
    silence_after_speech: float = 1.0     # finalise when speech has been seen and this much silence has followed it
    silence_without_speech: float = 5.0   # ... when nothing but silence has come in for this long
    max_utterance: float = 20.0           # ... whatever has been said, after this long

    @staticmethod
    def frames(seconds: float) -> int:
        return int(math.ceil(round(seconds / FRAME_SECONDS, 6)))


class AcousticEndpointer:
    """Acoustic endpointing of one session: finalise after N ms of silence, from the speech / silence state of the
    session's stream (the ``activity`` of its replies: speechcatcher_amd.activity.FIELDS) instead of "the text did not
    grow".  Same protocol as ``Endpointer``: ``decide`` before a chunk, ``observe`` after every non-final reply; the
    history restarts after every finalisation (``reset``)."""

    def __init__(self, rules: Optional[EndpointRules] = None):
        self.rules = rules or EndpointRules()
        self.after_speech = EndpointRules.frames(self.rules.silence_after_speech)
        self.without_speech = EndpointRules.frames(self.rules.silence_without_speech)
        self.max_frames = EndpointRules.frames(self.rules.max_utterance)
        self.last: Optional[dict] = None

    def fires(self, a: dict) -> bool:
        return ((a["n_speech"] > 0 and a["trail_silence"] >= self.after_speech)
                or (a["n_speech"] == 0 and a["n_frames"] >= self.without_speech)
                or a["n_frames"] >= self.max_frames)

    def decide(self) -> bool:
        """Called BEFORE a chunk is decoded: finalise this chunk?"""
        if self.last is None or not self.fires(self.last):
            return False
        self.reset()
        return True

    def observe(self, activity: dict):
        """Called after every NON-final reply with its ``activity``."""
        self.last = dict(activity)

    def reset(self):
        self.last = None


def spotting_set(spotting: dict):
    """{name: ids or [ids, ...]} -> (phrases: list of id sequences, names: the name each stands for).  Several id
    sequences may stand for one phrase (other tokenisations of it)."""
    phrases, names = [], []
    for name, ids in spotting.items():
        seqs = ids if len(ids) and isinstance(ids[0], (list, tuple, np.ndarray)) else [ids]
        for y in seqs:
            phrases.append([int(t) for t in y])
            names.append(name)
    return phrases, names


def spotted_message(detections, names) -> dict:
    """{"spotted": [{"phrase", "start", "end", "score"}]}: the phrase's name, start / end in seconds of the utterance"""
    return {"spotted": [{"phrase": names[d["phrase"]], "start": round(d["start_s"], 3), "end": round(d["end_s"], 3),
                         "score": d["score"]} for d in detections]}


def vosk_partial(text: str) -> dict:
    return {"partial": text}


def vosk_partial_ahead(text: str, ahead: list) -> dict:
    """a partial with the draft tokens that lie behind the search's last token (DraftResults.ahead): their text, and one
    entry per token with start / end in seconds of the utterance and conf = its arg-max posterior"""
    words = [{"word": str(d.get("token", d["id"])).replace("▁", " "), "start": round(d["start_s"], 3),
              "end": round(d["end_s"], 3), "conf": d["conf"]} for d in ahead]
    if ahead and "token" in ahead[0]:
        text_ahead = "".join(d["token"] for d in ahead).replace("▁", " ").strip()
    else:
        text_ahead = " ".join(str(d["id"]) for d in ahead)
    return {"partial": text, "ahead": text_ahead, "ahead_result": words}


def vosk_result(tokens: List[str], token_pos: Optional[List[int]] = None) -> dict:
    """Final result in Vosk style (speechcatcher_server.py:298-328): one entry
    per output token (not per word), "▁" is the sentencepiece space."""
    words, text = [], ""
    for idx, tok in enumerate(tokens):
        start = token_pos[idx] / FRAMES_PER_SECOND if token_pos is not None and idx < len(token_pos) else idx * 0.1
        words.append({"conf": 1.0, "start": start, "end": start + 1.0 / FRAMES_PER_SECOND,
                      "word": tok.replace("▁", " ")})
        text += tok
    return {"result": words, "text": text.replace("▁", " ").strip()}


def vosk_result_aligned(tokens: List[str], alignment: dict) -> dict:
    """Final result with CTC forced-alignment times (ServerLoop(vosk_alignment=True)): one entry per WORD -
    SentencePiece tokens merged at "▁" - with the aligned start / end of its tokens (seconds of the stream) and
    conf = the product of their confidences; tokens without an alignment are left out of the words."""
    keep = [k for k in range(len(tokens)) if alignment["start_s"][k] is not None]
    words = merge_words([tokens[k] for k in keep], [alignment["start_s"][k] for k in keep],
                        [alignment["end_s"][k] for k in keep], [alignment["conf"][k] for k in keep])
    return {"result": [{"conf": w["conf"], "start": w["start"], "end": w["end"], "word": w["word"]} for w in words],
            "text": "".join(tokens).replace("▁", " ").strip()}


def _aligned_keep(alignment: dict) -> List[int]:
    return [k for k in range(len(alignment["start_s"])) if alignment["start_s"][k] is not None]


def vosk_words(tokens: List[str], token_pos, alignment: Optional[dict], aligned: bool, records=None) -> List[dict]:
    """the "result" entries of one hypothesis: vosk_result_aligned's words when ``aligned`` and it has an alignment, else
    vosk_result's entry per token; with ``records`` (one per token: speechcatcher_amd.alternates) every entry also carries
    "tokens", the records of the tokens it is made of"""
    if aligned and alignment is not None and any(a is not None for a in alignment["start_s"]):
        words = vosk_result_aligned(tokens, alignment)["result"]
        if records is not None:
            keep = _aligned_keep(alignment)
            words = alternates_mod.attach_word_tokens(words, [tokens[k] for k in keep], [records[k] for k in keep])
        return words
    words = vosk_result(tokens, token_pos)["result"]
    return alternates_mod.attach_entry_tokens(words, records) if records is not None else words


def scale_server_pcm(data: np.ndarray) -> np.ndarray:
    """int16 -> the float values the reference server feeds its model:
    ``astype(float16) / 32767.0`` (rounded to float16), then fp32."""
    return (data.astype(np.float16) / np.float16(32767.0)).astype(np.float32)


class _Session:
    def __init__(self, sid: int, vosk: bool, finalize_update_iters: int, max_partial_iters: int,
                 acoustic: Optional[EndpointRules] = None):
        self.sid = sid
        self.vosk = vosk
        self.endpointer = Endpointer(finalize_update_iters, max_partial_iters)
        self.acoustic = AcousticEndpointer(acoustic) if acoustic is not None else None
        self.inbox: Deque[Message] = deque()
        self.in_flight: Optional[dict] = None     # the chunk currently queued in the scheduler
        self.vosk_sample_rate = 16000
        self.wire = None                          # (format, channels, channel, scale): the session hands its bytes to the engine
        self.max_alternatives = 0                 # Vosk config.max_alternatives (ServerLoop(vosk_alternatives=N))
        self.stable_n = 0                         # ServerLoop(stable_partials=True): committed tokens put into text so far
        self.stable_text = ""                     # ... and their text (the "▁" of the pieces already turned into spaces)
        self.last = vosk_partial("") if vosk else ""


class ServerLoop:
    """Sessions of all connected clients over one ``StreamScheduler``."""

    def __init__(self, scheduler: StreamScheduler, vosk_output_format: bool = False,
                 finalize_update_iters: int = 6, max_partial_iters: int = 42, strict_reference: bool = False,
                 continuous: Optional[bool] = None, min_replies: int = 1, vosk_alignment: bool = False,
                 acoustic_endpointing: Optional[EndpointRules] = None, spotting: Optional[dict] = None,
                 spotting_min_scores: Optional[dict] = None, draft_partials: bool = False, raw_input: bool = False,
                 input_level: bool = False, vosk_alternatives: int = 0, token_alternates: int = 0,
                 stable_partials: bool = False, ctc_beam=None, ctc_lm=None, lm_weight: float = 0.5,
                 word_bonus: float = 0.0, rescore_lm=None, rescore_weight: float = 0.5, rescore_bonus: float = 0.0,
                 attention_rescore=None, consensus=None, consensus_scale: float = 1.0):
        """``strict_reference``: no stream reset after a finalised utterance nor between clients, exactly like
        ``recognize_ws`` / ``process_audio_chunk`` (speechcatcher_server.py:270,359-397); the default resets.
        ``continuous`` (default: on whenever the batch has the C++ engine's submit / poll - round 4; False forces one
        batched lock-step call per step): a step hands the engine the chunks of the sessions that are ready and returns as soon as
        ``min_replies`` replies are (``StreamScheduler.pump``): every client is answered when ITS chunk is decoded
        and may send the next one at once, instead of all clients waiting for the slowest stream of a batch -
        the reference's per-client handler loop (:359-397), same calls and replies per session.
        ``vosk_alignment`` (C++ engine, Vosk format): final results carry WORDS with times and confidences from a CTC
        forced alignment (vosk_result_aligned) instead of one entry per token at its block's frame with conf 1.0; a result
        whose hypothesis cannot be aligned (more tokens than its block has frames) keeps those default entries.
        ``acoustic_endpointing``: an utterance is also finalised when the acoustic rules fire (AcousticEndpointer: N ms of
        silence from the CTC blank posterior) - finalize = text endpointer or acoustic endpointer or forced.  Switches the
        scheduler's ``activity`` option on (blank threshold 0.8 unless the scheduler was built with another); needs the
        reset after a final, so not with ``strict_reference``.  None (default): the reference's rule alone.
        ``spotting``: {name: token ids, or a list of id sequences that all stand for the name} - phrase spotting from the
        CTC table (the scheduler's ``phrases`` option; floors: ``spotting_min_scores`` {name: min_score}, default -2.0
        per token).  When phrases were detected in the frames of a chunk, a {"spotted": [{"phrase", "start", "end",
        "score"}]} message (seconds of the utterance) goes out in front of that chunk's reply.  Counts the frames of an
        utterance from the reset after a final, so not with ``strict_reference``.  None (default): no such message.
        ``draft_partials`` (Vosk format): a partial becomes {"partial": text, "ahead": text of the draft tokens behind the
        search's last token, "ahead_result": [{"word", "start", "end", "conf"}]} (the scheduler's ``draft`` option:
        the greedy CTC transcript of the newest frames, which the blockwise search has not reached yet).  Finals are
        unchanged.  Counts the frames of an utterance from the reset after a final, so not with ``strict_reference``.
        False (default): partials as they are.
        ``raw_input``: plain s16le sessions hand their bytes to the engine as they arrive (wire format S16LE with
        pcm.SCALE_SERVER: the values of ``scale_server_pcm`` bit for bit, computed by the engine - on the GPU in the C++
        engine's staging step) instead of converting every message here.  Sessions whose Vosk ``config`` names a
        ``format`` ("s16le", "s24le", "u8", "mulaw", "alaw", "f32"), ``channels`` (1..8) or ``channel`` (an index, or
        "mix") always do.  False (default): today's host conversion.
        ``input_level`` (Vosk format): partial and final replies carry {"level": {frames, clipped, sum_abs, peak,
        full_scale}} - the input level of the utterance so far (the scheduler's ``input_level`` option; all zero for a
        session converted on the host).
        ``vosk_alternatives`` = N > 0 (C++ engine, Vosk format): a session whose Vosk ``config`` carries
        ``max_alternatives`` = m > 0 (values above N count as N) gets its finals as {"alternatives": [{"text",
        "confidence", "result": [word entries]}, ...]}: the results the final reply holds, best first and at most m,
        confidence = speechcatcher_amd.alternates.nbest_posterior of their total scores, word times from the forced
        alignment of each (one call for all of them; a hypothesis that cannot be aligned keeps an entry per token).  m = 0
        or the option off: today's message.
        ``token_alternates`` = K > 0 (C++ engine, Vosk format): the word entries of a final - of its first alternative, or
        of the classic result - carry "tokens": per token of the word {"id", "token", "conf", "own_rank", "alternates":
        [{"id", "token", "conf"}]}, the K tokens that fit the token's frames best acoustically (the scheduler's
        ``alternates`` option).
        ``stable_partials`` (Vosk format): a partial becomes {"partial": text, "stable": text of the committed tokens,
        "stability": [one value per token of the best hypothesis behind them]} (the scheduler's ``stable_partials``
        option): ``stable`` is what every live hypothesis of the beam begins with - no later chunk of the
        utterance changes it and it only grows -, ``stability`` the share of the beam's mass behind each open token.
        The session keeps the committed text and puts only the newly committed tokens into text.  Composes with
        ``draft_partials`` (the ``ahead`` keys stay).  Finals are unchanged.  False (default): partials as they are.
        ``ctc_beam`` = B or (B, C) (C++ engine, Vosk format): the scheduler's ``ctc_beam`` option.  A
        connection whose Vosk ``config`` carries ``"decoder": "ctc"`` before its first audio becomes a decoder-free session:
        its partials and finals are built from the beam's best, ``max_alternatives`` = m > 0 (at most B; no
        ``vosk_alternatives`` needed) from the beam's n-best with confidence = each entry's share of the listed mass, word
        times from the prefix tree's frames with ``vosk_alignment``.  The endpointing rules are unchanged and operate on that
        text.  ``"decoder": "full"`` goes back.  Counts the frames of an utterance from the reset after a final, so not with
        ``strict_reference``.  None (default): the key is refused.
        ``ctc_lm`` (needs ``ctc_beam``): the path of a packed n-gram model (speechcatcher_amd.ngram) or its bytes, fused
        into that search with ``lm_weight`` / ``word_bonus`` (the scheduler's ``ctc_lm`` option): the
        beam's best and its n-best are ranked by the fused totals, and the ``max_alternatives`` confidences of a
        decoder-free session are the entries' shares of the listed FUSED mass.
        ``rescore_lm`` (C++ engine): the path of a packed n-gram model or its bytes - the final n-best list of a FULL
        session is rescored on the GPU, </s> term included, and re-ranked by score + ``rescore_weight`` * lm +
        ``rescore_bonus`` * tokens (the scheduler's ``final_lm`` option): the final's text and the order of
        its ``alternatives`` come from that ranking, their confidences are nbest_posterior of the FUSED totals, and the
        word times belong to the hypotheses reported.  Partials are unchanged."""
        if rescore_lm is not None:
            scheduler.enable_final_lm(rescore_lm, rescore_weight, rescore_bonus, eos=True)
        from . import ctc_beam as beam_mod
        if ctc_lm is not None and not (beam_mod.params(ctc_beam) or scheduler.ctc_beam is not None):
            raise ValueError("ctc_lm needs the ctc_beam option")
        if beam_mod.params(ctc_beam):
            if strict_reference:
                raise ValueError("the CTC prefix beam search counts the frames of an utterance from the reset after a final: "
                                 "not with strict_reference")
            if scheduler.ctc_beam is None:
                scheduler.enable_ctc_beam(*beam_mod.params(ctc_beam))
        if ctc_lm is not None:
            scheduler.enable_ctc_lm(ctc_lm, lm_weight, word_bonus)
        # ``attention_rescore`` = True or (w_att, w_ctc[, beta]) (needs ``ctc_beam``): the scheduler's option of that name
        #  - a connection whose Vosk ``config`` carries ``"decoder": "rescore"`` before its first audio is
        # decoder-free until its final, whose n-best list the attention decoder re-ranks; ``max_alternatives`` come from
        # the re-ranked list
        if attention_rescore is not None and attention_rescore is not False:
            scheduler.enable_attention_rescore(attention_rescore)
        # ``consensus`` = True or "confidence" (C++ engine): the scheduler's option of that name.  In the Vosk
        # format the entries of a final's "result" (of its first alternative) carry the consensus mass as "conf" - the
        # share of the n-best list's mass that agrees on the word, the minimum over its tokens -, the acoustic value as
        # "am_conf", and "rival" {"word", "mass"} where the list has a strongest other reading; with True the final also
        # carries "mbr" {"pivot", "risk", "am_rank"}.  Off by default: nothing changes.
        self.consensus = None
        if consensus is not None and consensus is not False:
            scheduler.enable_consensus(consensus, consensus_scale)
            self.consensus = scheduler.consensus
        self.stable_partials = bool(stable_partials) and vosk_output_format
        if self.stable_partials and not scheduler.stable_partials:
            scheduler.enable_stable_partials()
        self.vosk_alternatives = int(vosk_alternatives) if vosk_output_format else 0
        self.token_alternates = int(token_alternates) if vosk_output_format else 0
        if self.vosk_alternatives < 0:
            raise ValueError("vosk_alternatives must be >= 0")
        if self.token_alternates:
            scheduler.enable_alternates(self.token_alternates)
        if self.vosk_alternatives:
            if not hasattr(scheduler.batch, "align"):
                raise NotImplementedError("n-best alternatives take their word times from the C++ engine's forced alignment")
            scheduler.align_final = True
            scheduler.align_nbest = max(scheduler.align_nbest, self.vosk_alternatives)
        self.raw_input = bool(raw_input)
        self.input_level = bool(input_level)
        if input_level:
            scheduler.input_level = True
        self.draft_partials = False
        if draft_partials:
            if strict_reference:
                raise ValueError("draft partials count the frames of an utterance from the reset after a final: "
                                 "not with strict_reference")
            if not scheduler.draft:
                scheduler.enable_draft()
            self.draft_partials = True
        self.spot_names = None
        if spotting:
            if strict_reference:
                raise ValueError("phrase spotting counts the frames of an utterance from the reset after a final: "
                                 "not with strict_reference")
            phrases, self.spot_names = spotting_set(spotting)
            floors = None
            if spotting_min_scores is not None:
                floors = [float(spotting_min_scores.get(n, -2.0 * len(y))) for y, n in zip(phrases, self.spot_names)]
            scheduler.enable_spotting(phrases, floors)
        if acoustic_endpointing is not None:
            if strict_reference:
                raise ValueError("acoustic endpointing counts the frames of an utterance from the reset after a final: "
                                 "not with strict_reference")
            if not scheduler.activity:
                scheduler.enable_activity()
        self.acoustic_rules = acoustic_endpointing
        assert scheduler.result_format == "espnet", "sessions need token positions: result_format='espnet'"
        if strict_reference:
            scheduler.reset_after_final = scheduler.reset_on_open = False
        self.sch = scheduler
        if continuous is None:
            continuous = hasattr(scheduler.batch, "submit")
        self.continuous, self.min_replies = continuous, min_replies
        self.vosk = vosk_output_format
        self.vosk_alignment = vosk_alignment and vosk_output_format
        if self.vosk_alignment:
            scheduler.align_final = True
            if scheduler.ctc_beam is not None:   # the alternatives of a decoder-free session: every entry's tree frames
                scheduler.align_nbest = max(scheduler.align_nbest, scheduler.ctc_beam[0])
        self.fui, self.mpi = finalize_update_iters, max_partial_iters
        self.sessions: Dict[int, _Session] = {}

    # ---- connection lifecycle (recognize_ws, speechcatcher_server.py:359-397) ----
    def connect(self) -> int:
        """Raises ServerBusy when every stream slot is taken ("Server busy,
        please try again later.", :366)."""
        if self.raw_input:
            wire = (pcm_mod.S16LE, 1, 0, pcm_mod.SCALE_SERVER)
            sid = self.sch.open(format=wire[0], channels=wire[1], channel=wire[2], scale=wire[3])
        else:
            wire, sid = None, self.sch.open()
        self.sessions[sid] = _Session(sid, self.vosk, self.fui, self.mpi, self.acoustic_rules)
        self.sessions[sid].wire = wire
        return sid

    def disconnect(self, sid: int):
        self.sessions.pop(sid)
        self.sch.close(sid)

    def submit(self, sid: int, message: Message):
        """Queue one message of a client (audio bytes / int16 array, or a control string)."""
        self.sessions[sid].inbox.append(message)

    # ---- one batched step -------------------------------------------------------
    def step(self) -> Dict[int, List[Union[str, dict]]]:
        """Feeds at most one audio chunk per session into the batch (the
        endpointing decision of chunk k needs the result of chunk k-1), runs one
        batched chunk step and returns the replies per session, in order.  An Exception instance
        among a session's replies means: that client's message could not be processed (its stream
        has been reset) - close that connection; no other session is affected."""
        replies: Dict[int, List[Union[str, dict]]] = {}
        for ses in self.sessions.values():
            while ses.inbox and ses.in_flight is None:
                try:
                    immediate = self._start(ses, ses.inbox.popleft())
                except (TypeError, NotImplementedError, ValueError) as exc:
                    replies.setdefault(ses.sid, []).append(exc)     # this client only
                    continue
                if immediate is not None:
                    replies.setdefault(ses.sid, []).append(self._reply(ses, immediate))
        for sid, results in (self.sch.pump(self.min_replies) if self.continuous else self.sch.step()).items():
            ses = self.sessions[sid]
            if isinstance(results, Exception):
                # the client's handler dies with the exception in the reference (recognize_ws has no except for
                # it): the transport closes this connection; every other session is untouched
                ses.in_flight = None
                ses.endpointer.n_best_lens = []
                ses.stable_n, ses.stable_text = 0, ""
                if ses.acoustic is not None:
                    ses.acoustic.reset()
                replies.setdefault(sid, []).append(results)
                continue
            if self.spot_names is not None and getattr(results, "detections", None):
                replies.setdefault(sid, []).append(spotted_message(results.detections, self.spot_names))
            reply = self._reply(ses, self._finish(ses, results))
            if self.input_level and isinstance(reply, dict):
                reply = dict(reply, level=dict(getattr(results, "level", None) or pcm_mod.zero_level()))
            replies.setdefault(sid, []).append(reply)
        return replies

    def pending(self) -> bool:
        return any(s.inbox or s.in_flight for s in self.sessions.values())

    # ---- process_audio_chunk, split around the batched model call (:205-296) ----
    def _start(self, ses: _Session, message: Message):
        forced = False
        if isinstance(message, str):
            if not ses.vosk:
                return ""
            if message in ('{"eof" : 1}', '{"reset" : 1}'):
                forced = True
                data = np.zeros(1000, dtype=np.int16)
                if ses.wire is not None:
                    data = pcm_mod.silence(ses.wire[0], ses.wire[1], 1000)
            else:
                try:
                    cfg = json.loads(message).get("config", {})
                    rate = cfg.get("sample_rate", ses.vosk_sample_rate)
                    wire = self._config_format(ses, cfg)
                    if not isinstance(cfg, dict):
                        raise AttributeError("config")
                    decoder = cfg.get("decoder", self.sch.decoder(ses.sid))
                    if decoder not in ("full", "ctc", "rescore"):
                        raise ValueError(f'decoder must be "full", "ctc" or "rescore", got {decoder!r}')
                    max_alt = self._config_alternatives(ses, cfg, decoder)
                    phrases, unk = self._config_phrases(cfg, decoder)
                except (AttributeError, json.JSONDecodeError):
                    return vosk_partial("")
                # honoured for every rate the engine converts (8000..48000 Hz: speechcatcher_amd.resample) and every
                # wire format it decodes (speechcatcher_amd.pcm), before the session's first audio; ValueError
                # otherwise - this client's error reply (step)
                # - and both or neither: a rate whose format is refused does not stay
                if phrases is not None:   # the session answers only from this list (StreamScheduler.set_grammar); it is
                    self.sch.set_grammar(ses.sid, phrases)   # refused where the decoder would be: nothing has changed then
                self.sch.set_decoder(ses.sid, decoder)   # (the first of the three: a refusal leaves nothing changed)
                old_rate = self.sch.sample_rate(ses.sid)
                self.sch.set_sample_rate(ses.sid, rate)
                if wire is not None:
                    try:
                        self.sch.set_input_format(ses.sid, *wire)
                    except (ValueError, NotImplementedError):
                        self.sch.set_sample_rate(ses.sid, old_rate)
                        raise
                    ses.wire = wire
                ses.vosk_sample_rate = int(rate)
                ses.max_alternatives = max_alt
                if unk:   # no garbage model: the entry is left out of the grammar, and the reply says so
                    return dict(vosk_partial(""), ignored=["[unk]"])
                return vosk_partial("")
        elif ses.wire is not None:                          # the session's bytes go to the engine as they are
            if isinstance(message, np.ndarray) and message.dtype.kind not in "iu" and not (
                    ses.wire[0] == pcm_mod.F32 and message.dtype == np.float32):
                raise TypeError("audio arrays must hold the session's coded samples (an integer dtype)")
            data = pcm_mod.as_bytes(message)
        elif isinstance(message, np.ndarray):
            if message.dtype != np.int16:
                raise TypeError("audio arrays must be int16 PCM")
            data = message
        else:
            data = np.frombuffer(message, dtype="<i2")      # s16le at the session's sample rate
        if data.size == 0:
            return vosk_partial("") if ses.vosk else ""
        finalize = ses.endpointer.decide()
        if ses.acoustic is not None:
            if ses.acoustic.decide() and not finalize:
                finalize = True
                ses.endpointer.n_best_lens = []   # a finalisation restarts both histories
        finalize = finalize or forced
        if finalize and ses.acoustic is not None:
            ses.acoustic.reset()
        self.sch.feed(ses.sid, data if ses.wire is not None else scale_server_pcm(data), is_final=finalize, finalize_all=False)
        ses.in_flight = {"finalize": finalize, "forced": forced}
        return None

    def _config_format(self, ses: _Session, cfg: dict):
        """the wire format a Vosk ``config`` asks for -> (format, channels, channel, scale), or None when it names none
        (the session stays as it is); ValueError for an unknown value.  SCALE_SERVER where the format takes it: the
        reference server's conversion."""
        if not any(k in cfg for k in ("format", "channels", "channel")):
            return None
        cur = ses.wire or (pcm_mod.S16LE, 1, 0, pcm_mod.SCALE_SERVER)
        name = cfg.get("format", pcm_mod.NAME_OF[cur[0]])
        if not isinstance(name, str) or name.lower() not in pcm_mod.FORMAT_NAMES:
            raise ValueError(f"unknown audio format {name!r} (one of {', '.join(pcm_mod.FORMAT_NAMES)})")
        fmt = pcm_mod.FORMAT_NAMES[name.lower()]
        channels = cfg.get("channels", cur[1])
        channel = cfg.get("channel", pcm_mod.MIX if "channels" in cfg else cur[2])
        if channel == "mix":
            channel = pcm_mod.MIX
        for what, v in (("channels", channels), ("channel", channel)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{what} must be an integer, got {v!r}")
        scale = pcm_mod.SCALE_SERVER if fmt in (pcm_mod.S16LE, pcm_mod.MULAW, pcm_mod.ALAW) else pcm_mod.SCALE_FULL
        pcm_mod.check_args(fmt, channels, channel, scale)
        return (fmt, channels, channel, scale)

    @staticmethod
    def _config_phrases(cfg: dict, decoder: str):
        """the ``phrase_list`` a Vosk ``config`` carries -> (its phrases without "[unk]" entries, whether one was left
        out); (None, False) when the message names none.  ValueError for anything but a list of strings with a phrase
        left, and on a connection that is not decoder-free: the grammar constrains the CTC beam, the blockwise search of
        a FULL session has none."""
        if "phrase_list" not in cfg:
            return None, False
        pl = cfg["phrase_list"]
        if decoder not in ("ctc", "rescore"):
            raise ValueError('phrase_list needs a decoder-free connection ("decoder": "ctc")')
        if not isinstance(pl, list) or not all(isinstance(p, str) for p in pl):
            raise ValueError("phrase_list must be a list of strings")
        phrases = [p for p in pl if p.strip() != "[unk]"]
        if not any(p.strip() for p in phrases):
            raise ValueError("phrase_list holds no phrase")
        return [p for p in phrases if p.strip()], len(phrases) != len(pl)

    def _config_alternatives(self, ses: _Session, cfg: dict, decoder: str = "full") -> int:
        """the ``max_alternatives`` a Vosk ``config`` asks for, at most ``vosk_alternatives`` - for a decoder-free session
        at most the beam's B - (the session's own when the message names none; 0 with the option off); ValueError for
        anything but a non-negative integer"""
        cap = self.sch.ctc_beam[0] if decoder in ("ctc", "rescore") and self.sch.ctc_beam else self.vosk_alternatives
        if "max_alternatives" not in cfg or not cap:
            return min(ses.max_alternatives, cap)
        m = cfg["max_alternatives"]
        if isinstance(m, bool) or not isinstance(m, int) or m < 0:
            raise ValueError(f"max_alternatives must be a non-negative integer, got {m!r}")
        return min(m, cap)

    def _final_message(self, ses: _Session, results: list) -> dict:
        """the Vosk final of a reply with results: the classic {"result", "text"}, or {"alternatives": [...]} for a
        session that asked for them; with ``token_alternates`` the first hypothesis' entries carry their token records.
        A session with a ``phrase_list``: the text is the best COMPLETE entry's (the scheduler lists those first); when
        none is complete the text is empty and the best entry's goes out under "incomplete"; alternatives carry
        "complete"."""
        msg = self._with_consensus(self._final_message_plain(ses, results), results)
        complete = getattr(results, "grammar_complete", None)
        if complete is None:
            return msg
        if "alternatives" in msg:
            for a, r in zip(msg["alternatives"], results):
                a["complete"] = bool(r[4].get("complete")) if len(r) > 4 and isinstance(r[4], dict) else bool(complete)
            return msg
        return msg if complete else {"result": [], "text": "", "incomplete": msg["text"]}

    def _with_consensus(self, msg: dict, results: list) -> dict:
        """``msg`` with the consensus mass in the word entries of the first result (ServerLoop(consensus=...))"""
        cons = getattr(results, "consensus", None)
        if self.consensus is None or cons is None:
            return msg
        tokens = results[0][1]
        recs = cons["tokens"]
        if len(recs) == len(tokens):
            first = msg["alternatives"][0] if "alternatives" in msg else msg
            words = first.get("result", [])
            slots = mbr_mod.word_slots(tokens, recs)
            if len(slots) != len(words) and len(words) == len(recs):   # an entry per token (no forced alignment)
                slots = [dict({"consensus": r["consensus"]}, **({"rival": {"word": r["rival"]["token"].replace("▁", ""),
                                                                          "mass": r["rival"]["mass"]}} if "rival" in r else {}))
                         for r in recs]
            first["result"] = mbr_mod.vosk_words(words, slots)
        if self.consensus is True:
            msg["mbr"] = dict(cons["mbr"])
        return msg

    def _final_message_plain(self, ses: _Session, results: list) -> dict:
        _text, tokens, _ids, pos, _hyp = results[0]
        al = getattr(results, "alignment", None)
        records = al.get("alternates") if self.token_alternates and al is not None else None
        if records is not None and len(records) != len(tokens):
            records = None
        free = self.sch.decoder(ses.sid) in ("ctc", "rescore")   # its results are the beam's entries, its alignment the tree's frames
        alts = ses.max_alternatives > 0 and (self.vosk_alternatives > 0 or free)
        aligned = self.vosk_alignment or (alts and not free)
        if alts:
            res = list(results[:ses.max_alternatives])
            nbest = (al or {}).get("nbest") or [al]
            texts, words = [], []
            for r, (_t, toks, _i, p, _h) in enumerate(res):
                texts.append("".join(toks).replace("▁", " ").strip())
                words.append(vosk_words(toks, p, nbest[r] if r < len(nbest) else None, aligned, records if r == 0 else None))
            # (a re-ranked final: the fused totals rank the list, so the confidences come from them)
            return alternates_mod.vosk_alternatives(texts, [r[4].get("fused", r[4]["score"]) for r in res], words)
        if records is None:   # today's message
            if self.vosk_alignment and al is not None and any(a is not None for a in al["start_s"]):
                return vosk_result_aligned(tokens, al)
            return vosk_result(tokens, pos)
        return {"result": vosk_words(tokens, pos, al, aligned, records), "text": "".join(tokens).replace("▁", " ").strip()}

    def _stable_keys(self, ses: _Session, results, message: dict, finalize: bool) -> dict:
        """``message`` with the "stable" and "stability" keys of a partial; a final starts the session's text over"""
        st = getattr(results, "stable", None)
        if finalize or st is None:
            ses.stable_n, ses.stable_text = 0, ""
            return message
        names = self.sch.token_list
        # hyps_to_results' selection: yseq without its first token (the <sos>), without the ids a transcript leaves out
        new = [t for t in st["tokens"][max(ses.stable_n, 1):st["committed"]] if t not in TEXT_SKIP_IDS]
        if names is not None:
            ses.stable_text += "".join(names[t] for t in new).replace("▁", " ")
        else:
            ses.stable_text += "".join(f" {t}" for t in new)
        ses.stable_n = st["committed"]
        return dict(message, stable=ses.stable_text.strip(), stability=[float(v) for v in st["stability"]])

    def _finish(self, ses: _Session, results: list):
        finalize = ses.in_flight["finalize"]
        out = self._finish_plain(ses, results)
        if not (ses.vosk and self.stable_partials):
            return out
        if finalize:
            if not out and isinstance(ses.last, dict) and "stable" in ses.last:
                # a final without a hypothesis repeats the partial alone
                ses.last = {k: v for k, v in ses.last.items() if k not in ("stable", "stability")}
            return self._stable_keys(ses, results, out, True)
        if not out:   # no hypothesis yet: the partial of the last reply (an empty one behind a final)
            out = vosk_partial(ses.last["partial"] if isinstance(ses.last, dict) and "partial" in ses.last else "")
        return self._stable_keys(ses, results, out, False)

    def _finish_plain(self, ses: _Session, results: list):
        info, ses.in_flight = ses.in_flight, None
        if info["forced"]:
            ses.endpointer.n_best_lens = []   # session.reset() after a client-forced finalize (:272-273)
        if ses.acoustic is not None and not info["finalize"]:
            ses.acoustic.observe(results.activity)
        if not results:
            if ses.vosk and self.draft_partials and not info["finalize"]:
                # no hypothesis yet: the partial of the last reply (an empty one behind a final), and the draft
                last = ses.last["partial"] if isinstance(ses.last, dict) and "partial" in ses.last else ""
                return vosk_partial_ahead(last, getattr(results, "ahead", None) or [])
            if self.draft_partials and isinstance(ses.last, dict) and "ahead" in ses.last:
                ses.last = vosk_partial(ses.last["partial"])   # a final without a hypothesis repeats the partial alone
            return ""
        text, tokens, _ids, pos, _hyp = results[0]
        if info["finalize"]:
            if len(text) >= 1:
                if text[-1] not in ".!?":
                    text += "."
                text += "\n"
            return self._final_message(ses, results) if ses.vosk else text
        ses.endpointer.observe(len(text))
        if ses.vosk and self.draft_partials:
            return vosk_partial_ahead(text, getattr(results, "ahead", None) or [])
        return vosk_partial(text) if ses.vosk else text

    @staticmethod
    def _reply(ses: _Session, transcription):
        """recognize_ws (:376-393): Vosk clients get an answer for every message; an
        empty transcription repeats the last one, a final result only once."""
        if transcription:
            ses.last = transcription
            return transcription
        if ses.vosk:
            if isinstance(ses.last, dict) and ("result" in ses.last or "alternatives" in ses.last):
                ses.last = vosk_partial("")
            return ses.last
        return transcription


class StepPacer:
    """WHEN to run the next batched step.  The reference answers every message with its own model call as it
    arrives (``recognize_ws``, speechcatcher_server.py:376-380); a batch needs a policy instead: run a step as
    soon as every connected session has a message waiting (a full batch), or when the oldest waiting message has
    waited ``max_wait_s`` (latency bound for the clients that did send), whichever comes first.  The transport
    calls ``submit`` for every received message and ``poll`` from its event loop."""

    def __init__(self, loop: ServerLoop, max_wait_s: float = 0.05, clock=None):
        import time
        self.loop = loop
        self.max_wait_s = max_wait_s
        self.clock = clock or time.monotonic
        self._stamps: Dict[int, Deque[float]] = {}

    def submit(self, sid: int, message: Message):
        self._stamps.setdefault(sid, deque()).append(self.clock())
        self.loop.submit(sid, message)

    def due(self) -> bool:
        sessions = self.loop.sessions
        waiting = [sid for sid, ses in sessions.items() if ses.inbox]
        if not waiting:
            return False
        if len(waiting) == len(sessions):
            return True
        oldest = min(self._stamps[sid][0] for sid in waiting if self._stamps.get(sid))
        return self.clock() - oldest >= self.max_wait_s

    def poll(self) -> Optional[Dict[int, List[Union[str, dict]]]]:
        """Runs one batched step if one is due and returns its replies (None otherwise)."""
        if not self.due():
            return None
        replies = self.loop.step()
        for sid in list(self._stamps):
            ses = self.loop.sessions.get(sid)
            if ses is None:                       # disconnected meanwhile
                del self._stamps[sid]
                continue
            st = self._stamps[sid]
            while len(st) > len(ses.inbox):       # messages the step consumed
                st.popleft()
        return replies


__all__ = ["Endpointer", "EndpointRules", "AcousticEndpointer", "ServerLoop", "StepPacer", "ServerBusy", "vosk_partial", "vosk_result", "vosk_result_aligned",
           "spotting_set", "spotted_message", "vosk_partial_ahead",
           "scale_server_pcm"]
