"""Long-recording segmentation and the file-level recognise loop on top of the
batched engine - SURVEY.md section 8(f) rank 2.

Replaces, for the native-decoder path, the reference CLI's
``segment_speech`` + process pool over segments
(speechcatcher/simple_endpointing.py:21-145, speechcatcher/speechcatcher.py:414-497,
574-592): recordings longer than a minute are cut at low-energy points into
~60 s segments, every segment is decoded as its own stream - here as PARALLEL
streams of one ``StreamBatch`` on the GPU instead of forked CPU processes.

* ``CutSearch`` restates the reference's beam search over cut points; pinned
  against the reference class on seeded energy curves (tests/golden/segmenter.json,
  tools/gen_golden_segmenter.py).
* ``log_fbank_energy`` restates ``python_speech_features.logfbank`` (third-party
  dependency of the reference, requirements.txt:10, unpinned version; absent in
  this image) from its published algorithm: pre-emphasis 0.97, 25 ms / 10 ms
  rectangular frames, 512-point power spectrum / NFFT, 26 triangular mel filters
  0..fs/2, log.  PARITY UNPINNED for this function (no fixture can be generated
  without the package); the cut search downstream of it is pinned.
* ``smoothed_negative_energy(backend="gpu")`` / ``segmentation="gpu"``: the same curve from the float64 kernels of
  csrc/segment.hip instead of the host pass (opt-in; DESIGN.md 8c, contract in tests/segment_ref.py).
* ``plan_segments`` mirrors the chunk-aligned finalize positions of
  speechcatcher.py:430-446; ``recognize_recording`` is the file-level loop.
"""
import math
from typing import List, Optional, Tuple

import numpy as np

from .scheduler import recognize_segments


# ---------------------------------------------------------------------------
# energy curve
# ---------------------------------------------------------------------------
def _mel_filterbank(nfilt: int, nfft: int, samplerate: int) -> np.ndarray:
    hz2mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)      # noqa: E731
    mel2hz = lambda mel: 700.0 * (10.0 ** (mel / 2595.0) - 1.0)  # noqa: E731
    melpoints = np.linspace(hz2mel(0.0), hz2mel(samplerate / 2.0), nfilt + 2)
    bins = np.floor((nfft + 1) * mel2hz(melpoints) / samplerate)
    fb = np.zeros((nfilt, nfft // 2 + 1))
    for j in range(nfilt):
        lo, mid, hi = int(bins[j]), int(bins[j + 1]), int(bins[j + 2])
        for i in range(lo, mid):
            fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(mid, hi):
            fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    return fb


def log_fbank_energy(data: np.ndarray, samplerate: int = 16000, winlen: float = 0.025, winstep: float = 0.01,
                     nfilt: int = 26, nfft: int = 512, preemph: float = 0.97) -> np.ndarray:
    """(n_frames, nfilt) log mel filterbank energies, 100 frames per second."""
    sig = np.asarray(data, dtype=np.float64)
    sig = np.append(sig[0], sig[1:] - preemph * sig[:-1])
    flen, fstep = int(round(winlen * samplerate)), int(round(winstep * samplerate))
    n = len(sig)
    nframes = 1 if n <= flen else 1 + int(math.ceil((1.0 * n - flen) / fstep))
    pad = np.concatenate([sig, np.zeros((nframes - 1) * fstep + flen - n)])
    idx = np.arange(flen)[None, :] + (np.arange(nframes) * fstep)[:, None]
    frames = pad[idx]
    pspec = (1.0 / nfft) * np.square(np.abs(np.fft.rfft(frames, nfft)))
    feat = pspec @ _mel_filterbank(nfilt, nfft, samplerate).T
    feat = np.where(feat == 0, np.finfo(float).eps, feat)
    return np.log(feat)


SEGMENTATION_BACKENDS = ("host", "gpu")


def _check_segmentation(backend: str) -> None:
    if backend not in SEGMENTATION_BACKENDS:
        raise ValueError(f"unknown segmentation backend {backend!r}: one of {SEGMENTATION_BACKENDS}")


def smoothed_negative_energy(data: np.ndarray, samplerate: int = 16000, backend: str = "host") -> np.ndarray:
    """simple_endpointing.py:81-84: summed log fbank / 10, Gaussian sigma = 20 frames, sign flipped
    (pauses become maxima).  ``backend="gpu"``: the same curve in float64 from the two kernels of csrc/segment.hip
    (hip_backend.segment_energy) - int16 samples at 16 kHz only."""
    _check_segmentation(backend)
    if backend == "gpu":
        if samplerate != 16000:
            raise ValueError(f"the GPU energy curve is 16 kHz only, got {samplerate} Hz (convert first: hip_backend.resample)")
        data = np.asarray(data)
        if data.dtype != np.int16:
            raise ValueError(f"the GPU energy curve takes int16 samples, got {data.dtype}")
        from .hip_backend import segment_energy
        return segment_energy(data, smoothed=True)
    from scipy.ndimage import gaussian_filter1d
    power = log_fbank_energy(data, samplerate).sum(axis=-1) / 10.0
    return gaussian_filter1d(power, sigma=20) * -1.0


# ---------------------------------------------------------------------------
# cut search (simple_endpointing.py:21-79)
# ---------------------------------------------------------------------------
class CutSearch:
    """Beam search over cut positions: a path is a list of cut frames; extending
    it by a segment of j frames (min_len <= j < max_lookahead, every ``step``)
    adds  w_len * f * (ideal - |ideal - j|) + w_energy * energy[cut]  with
    f = w_len / ideal (the length weight enters twice, as in the reference)."""

    def __init__(self, beam_size=10, ideal_segment_len=4000, max_lookahead=18000, min_len=2000, step=10,
                 len_reward_weight=1.0, energy_weight=1.0):
        self.beam_size, self.ideal, self.max_lookahead = beam_size, ideal_segment_len, max_lookahead
        self.min_len, self.step = min_len, step
        self.w_len, self.w_energy = len_reward_weight, energy_weight
        self.factor = len_reward_weight / float(ideal_segment_len)

    def search(self, energy: np.ndarray, n_frames: int) -> List[Tuple[int, int]]:
        energy = np.asarray(energy, dtype=np.float64)
        paths: List[Tuple[List[int], float]] = [([0], 0.0)]
        while True:
            worst_in_beam = paths[-1][1]
            cand_scores, cand_src, cand_cut = [], [], []
            expand = False
            for pi, (cuts, score) in enumerate(paths):
                last = cuts[-1]
                j = np.arange(self.min_len, min(self.max_lookahead, n_frames - last - 1), self.step)
                if j.size == 0:
                    continue
                length_reward = self.factor * (self.ideal - np.abs(self.ideal - j.astype(np.float64)))
                new = score + ((self.w_len * length_reward) + (self.w_energy * energy[last + j]))
                keep = new > score
                if (new > worst_in_beam).any():
                    expand = True
                cand_scores.append(new[keep])
                cand_cut.append(last + j[keep] + 1)
                cand_src.append(np.full(int(keep.sum()), pi))
            if not cand_scores or not expand:
                break
            sc, cut, src = np.concatenate(cand_scores), np.concatenate(cand_cut), np.concatenate(cand_src)
            if sc.size == 0:
                break
            order = np.argsort(-sc, kind="stable")[: self.beam_size]   # ties keep generation order
            paths = [(paths[int(src[o])][0] + [int(cut[o])], float(sc[o])) for o in order]
        best = paths[0][0] if paths[0][0] != [0] else [0, n_frames]
        return list(zip(best[:-1], best[1:]))


def segment_speech(data: np.ndarray, samplerate: int = 16000, average_segment_length: float = 60.0,
                   max_segment_len_sec: float = 180, beam_size: int = 10, step: int = 10,
                   len_reward_weight: float = 12.0, energy_weight: float = 1.0,
                   segmentation: str = "host") -> List[Tuple[int, int]]:
    """simple_endpointing.py:81-145: (start, end) in 10 ms frames; no segment longer than max_segment_len_sec.
    ``segmentation``: where the energy curve is computed ("host", or "gpu": smoothed_negative_energy)."""
    _check_segmentation(segmentation)
    energy = smoothed_negative_energy(data, samplerate, backend=segmentation)
    search = CutSearch(beam_size=beam_size, ideal_segment_len=int(average_segment_length * 100), step=step,
                       len_reward_weight=len_reward_weight, energy_weight=energy_weight)
    return constrain_segments(search.search(energy, len(energy)), max_segment_len_sec)


def constrain_segments(segments, max_segment_len_sec: float = 180) -> List[Tuple[int, int]]:
    max_frames = int(max_segment_len_sec * 100)
    out = []
    for start, end in segments:
        while end - start > max_frames:
            out.append((start, start + max_frames))
            start += max_frames
        out.append((start, end))
    return out


# ---------------------------------------------------------------------------
# file-level loop (speechcatcher.py:414-497)
# ---------------------------------------------------------------------------
def plan_segments(n_samples: int, rate: int, segments: List[Tuple[int, int]], chunk_length: int = 8192):
    """Chunk-aligned sample ranges of the decode segments: the reference finalises
    at chunk index ceil((end_s * rate - chunk) / chunk) for every cut that leaves
    at least 10 s, segment k covers chunks (i_k, i_{k+1}]  (speechcatcher.py:430-446,
    574-586)."""
    n_frames = (n_samples / rate) * 100.0
    ends = [e for _, e in segments if e < n_frames - 1000.0]
    max_i = (n_samples // chunk_length) + 1
    idx = [-1] + [math.ceil((((f / 100.0) * rate) - chunk_length) / chunk_length) for f in ends] + [max_i]
    ranges = []
    for a, b in zip(idx[:-1], idx[1:]):
        lo, hi = (a + 1) * chunk_length, min((b + 1) * chunk_length, n_samples)
        if hi > lo:
            ranges.append((lo, hi))
    return ranges


def upper_case_first_letter(text: str) -> str:
    """speechcatcher.py:309-312"""
    return text[0].upper() + text[1:] if text and text[0].islower() else text


def is_completed(text: str) -> bool:
    """speechcatcher.py:316-317"""
    return text.endswith((".", "?", "!"))


def interpolate_repeating_positions(positions: List[float]) -> List[float]:
    """speechcatcher.py:323-352: inside a run of equal positions only the last element keeps
    the value, the others are spread linearly between the preceding value (0 before the first
    run) and it - several tokens emitted on the same encoder frame get increasing timestamps."""
    vals = [0.0] + [float(p) for p in positions]
    out: List[float] = []
    i = 0
    while i < len(vals):
        start = i
        while i < len(vals) and vals[i] == vals[start]:
            i += 1
        end = i - 1
        prev = 0.0 if start == 0 else vals[start - 1]
        n = end - start + 1
        out.extend(prev + (end - j) / n * (vals[start] - vals[start - 1]) for j in range(start, end))
        out.append(vals[end])
    return out[1:]


# --token-alignment, and with --token-alternates the per-token records (recognize_segments)
# ... and with --ctc-beam / --ctc-only the n-best list of every segment
# ... and with --consensus / --consensus-confidence the slot statistics of every segment
ALIGNMENT_KEYS = ("token_start", "token_end", "token_conf", "token_alternates", "ctc_nbest", "token_consensus", "token_rival",
                  "mbr")


def merge_paragraphs(segments: List[dict]) -> Tuple[str, List[dict]]:
    """speechcatcher.py:516-572: a segment starts a new paragraph (first letter capitalised)
    only if the previous segment's text ended a sentence; otherwise its text, tokens and
    timestamps are appended to the open paragraph."""
    if not segments:
        return "\n", []
    merged = [segments[0]["text"]]
    info = [dict(segments[0])]
    for prev, seg in zip(segments[:-1], segments[1:]):
        if is_completed(prev["text"]):
            text = upper_case_first_letter(seg["text"])
            merged.append(text)
            info.append(dict(seg, text=text))
        else:
            merged[-1] += " " + seg["text"]
            last = info[-1]
            last["end"] = seg["end"]
            last["text"] += " " + seg["text"]
            last["tokens"] = list(last["tokens"]) + list(seg["tokens"])
            last["token_timestamps"] = list(last["token_timestamps"]) + list(seg["token_timestamps"])
            for key in ALIGNMENT_KEYS:
                if key in last:
                    last[key] = list(last[key]) + list(seg[key])
    return "\n\n".join(merged) + "\n", info


def recognize_recording_segments(batch, raw_speech_data: np.ndarray, rate: int = 16000, chunk_length: int = 8192,
                                 token_list: Optional[List[str]] = None, reference_finalize: bool = False,
                                 average_segment_length: float = 60.0, token_alignment: bool = False,
                                 segmentation: str = "host", token_alternates: int = 0, ctc_beam=None,
                                 ctc_only: bool = False, ctc_lm=None, lm_weight: float = 0.5, word_bonus: float = 0.0,
                                 rescore_lm=None, rescore_weight: float = 0.5, rescore_bonus: float = 0.0,
                                 ctc_grammar=None, attention_rescore=None, consensus=None):
    """The segment loop of ``recognize`` (speechcatcher.py:414-497): int16 recording -> chunk-aligned sample
    ranges and the raw per-segment results of ``recognize_segments`` (before paragraph merging)."""
    assert rate == 16000
    _check_segmentation(segmentation)
    speech = np.asarray(raw_speech_data).astype(np.float32) / 32768.0
    segments = (segment_speech(raw_speech_data, rate, average_segment_length=average_segment_length,
                               segmentation=segmentation)
                if len(speech) > 60.0 * rate else [])
    ranges = plan_segments(len(speech), rate, segments, chunk_length)
    res = recognize_segments(batch, speech, ranges, chunk_length=chunk_length, token_list=token_list,
                             finalize_all_last_only=reference_finalize, token_alignment=token_alignment,
                             token_alternates=token_alternates, ctc_beam=ctc_beam, ctc_only=ctc_only,
                             ctc_lm=ctc_lm, lm_weight=lm_weight, word_bonus=word_bonus, rescore_lm=rescore_lm,
                             rescore_weight=rescore_weight, rescore_bonus=rescore_bonus,
                             **({} if ctc_grammar is None else {"ctc_grammar": ctc_grammar}), **({} if attention_rescore is None else {"attention_rescore": attention_rescore}),
                             **({} if consensus is None else {"consensus": consensus}))
    return ranges, res


def recognize_recording(batch, raw_speech_data: np.ndarray, rate: int = 16000, chunk_length: int = 8192,
                        token_list: Optional[List[str]] = None, reference_finalize: bool = False,
                        average_segment_length: float = 60.0, token_alignment: bool = False,
                        segmentation: str = "host", token_alternates: int = 0, ctc_beam=None,
                        ctc_only: bool = False, ctc_lm=None, lm_weight: float = 0.5,
                        word_bonus: float = 0.0, rescore_lm=None, rescore_weight: float = 0.5,
                        rescore_bonus: float = 0.0, ctc_grammar=None, attention_rescore=None,
                        consensus=None) -> Tuple[str, List[dict]]:
    """int16 recording -> (text, per-paragraph info).  Native-decoder input scaling
    /32768 in fp32 (speechcatcher.py:421); recordings over a minute are segmented;
    the segments run as parallel streams of ``batch`` (one slot = the reference CLI with one worker:
    serial segments on one model); paragraphs are merged like the CLI does.
    ``reference_finalize``: pass finalize_all only with the last chunk of the recording, as the
    reference CLI does.  ``token_alignment``: the paragraphs also carry ``token_start`` / ``token_end`` /
    ``token_conf`` (CTC forced alignment, next to ``token_timestamps``).  ``segmentation="gpu"``: the energy curve the
    cut search reads comes from the GPU (csrc/segment.hip) instead of the host pass.  ``token_alternates`` = K > 0
    (implies ``token_alignment``): they also carry ``token_alternates``, one record per token with its K acoustic alternates
    (speechcatcher_amd.alternates).  ``ctc_beam`` = B or (B, C): they also carry ``ctc_nbest``, per segment the n-best
    list of the CTC prefix beam search; ``ctc_only``: the segments are decoded by that search alone (recognize_segments);
    ``ctc_lm`` / ``lm_weight`` / ``word_bonus``: a packed n-gram model fused into it.
    ``rescore_lm`` / ``rescore_weight`` / ``rescore_bonus``: a packed n-gram model every segment's final n-best list is
    rescored with and re-ranked by (recognize_segments).  ``ctc_grammar``: a grammar every segment's CTC
    beam answers only from (recognize_segments).  ``attention_rescore`` (with ``ctc_only``): every segment's
    final ``ctc_nbest`` is re-ranked by one pass of the attention decoder (recognize_segments).
    ``consensus``: True or "confidence" - every segment's final n-best list is compared on the GPU; the paragraphs carry
    ``token_consensus`` / ``token_rival`` per token and ``mbr`` per segment (recognize_segments)."""
    ranges, res = recognize_recording_segments(batch, raw_speech_data, rate, chunk_length, token_list,
                                               reference_finalize, average_segment_length,
                                               token_alignment or token_alternates > 0, segmentation, token_alternates,
                                               ctc_beam, ctc_only, ctc_lm, lm_weight, word_bonus, rescore_lm,
                                               rescore_weight, rescore_bonus,
                                               **({} if ctc_grammar is None else {"ctc_grammar": ctc_grammar}), **({} if attention_rescore is None else {"attention_rescore": attention_rescore}),
                             **({} if consensus is None else {"consensus": consensus}))
    segs = [{"start": lo / rate, "end": hi / rate, "text": r["text"], "tokens": r["tokens"],
             "token_timestamps": r["token_timestamps"], **{k: r[k] for k in ALIGNMENT_KEYS if k in r}}
            for (lo, hi), r in zip(ranges, res)]
    return merge_paragraphs(segs)
