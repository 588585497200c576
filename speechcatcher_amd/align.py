"""Encoder frames of a CTC forced alignment (NativeStreamBatch.align / align_tokens) -> seconds.

The geometry comes from the model configuration, nothing is hard-coded:

* the frontend is an STFT with center=True: STFT frame j of a call is centred at sample ``hop * j`` of the waveform
  that call transforms (its carry-over + its chunk);
* the subsampling is two Conv2d layers with kernel 3 and stride 2 (``cfg.subsample`` = 4): encoder frame t is computed
  from the stream's feature frames ``4t ... 4t+6`` and stands for the ``subsample * hop`` samples (40 ms) centred on
  feature frame ``4t+3``.  The encoder's carry-over buffers emit every subsampled
  frame of the concatenated features exactly once, so this holds over all calls.

The FEATURE frames are not continuous in the audio: every call after the first keeps the last ``win - hop`` samples
(+ the remainder) of the previous one and drops its own first two STFT frames - frames the previous call did not keep
either (Appendix D item 1).  Each call boundary thus removes two hops (20 ms) from the feature sequence, and an index
-> time rule of a constant 40 ms per frame drifts by that much per call.  ``FeatureClock`` replays item 1 over the
stream's calls and gives every kept feature frame its centre sample; it also covers the quirk of the same item - a
middle call with at most 4 STFT frames returns nothing and its frames are lost.
"""
from typing import List, Sequence


class FeatureClock:
    """Centre sample of every feature frame a stream has produced since its last reset, from the lengths of its calls
    (``speech2text_streaming.py:300-400``)."""

    def __init__(self, win_length: int, hop_length: int):
        self.win, self.hop = win_length, hop_length
        self.centres: List[int] = []
        self._pos = 0          # stream sample of the carry-over's first sample
        self._buf = 0          # carry-over samples
        self._calls = 0

    def call(self, n_samples: int, is_final: bool):
        N, x0, first = self._buf + int(n_samples), self._pos, self._calls == 0
        self._calls += 1
        ov = self.win - self.hop
        if not is_final:
            if N <= self.win:
                self._buf = N
                return
            n, r = (N - ov) // self.hop, (N - ov) % self.hop
            if first:
                keep = range(0, n)
            else:
                keep = range(2, n) if n + 2 > 4 else range(0)   # a middle call of <= 4 STFT frames loses them
            self.centres += [x0 + self.hop * j for j in keep]
            self._pos, self._buf = x0 + N - ov - r, ov + r
        else:
            nf = 1 + max(N, self.win) // self.hop
            self.centres += [x0 + self.hop * j for j in range(0 if first else 2, nf)]
            self._pos, self._buf = x0 + N, 0

    def frame_span(self, t: int, subsample: int):
        """encoder frame t -> [first, last) sample of the stream it stands for"""
        f = subsample * t + subsample - 1
        c = self.centres[f] if f < len(self.centres) else \
            (self.centres[-1] if self.centres else 0) + self.hop * (f - len(self.centres) + 1)
        half = subsample * self.hop // 2
        return c - half, c + half

    def seconds(self, start_frames, end_frames, subsample: int, sample_rate: int, offset_s: float = 0.0):
        """token spans [start, end) in encoder frames -> (start seconds, end seconds) lists"""
        return ([offset_s + self.frame_span(int(a), subsample)[0] / sample_rate for a in start_frames],
                [offset_s + self.frame_span(int(b) - 1, subsample)[1] / sample_rate for b in end_frames])


def subsampled_frames(n_features: int) -> int:
    """encoder frames of n feature frames through the two k=3 s=2 convolutions (Appendix D item 2, final call)"""
    return ((n_features - 3) // 2 + 1 - 3) // 2 + 1


def frame_span_samples(t: int, hop_length: int, subsample: int):
    """encoder frame t -> [first, last) samples if the feature frames were continuous (a stream's first call; a
    stream fed as features) - FeatureClock for a stream fed as audio over several calls"""
    centre = hop_length * (subsample * t + subsample - 1)
    half = subsample * hop_length // 2
    return centre - half, centre + half


def frames_to_seconds(start_frames: Sequence[int], end_frames: Sequence[int], hop_length: int, subsample: int,
                      sample_rate: int, offset_s: float = 0.0):
    """token spans [start, end) in encoder frames -> (start seconds, end seconds) lists; ``offset_s``: the start of the
    segment in the recording (CLI segments)"""
    starts = [offset_s + frame_span_samples(int(a), hop_length, subsample)[0] / sample_rate for a in start_frames]
    ends = [offset_s + frame_span_samples(int(b) - 1, hop_length, subsample)[1] / sample_rate for b in end_frames]
    return starts, ends


def cfg_frames_to_seconds(cfg, start_frames, end_frames, offset_s: float = 0.0):
    """frames_to_seconds with the geometry of a model configuration (config.ModelConfig)"""
    return frames_to_seconds(start_frames, end_frames, cfg.hop_length, cfg.subsample, cfg.sample_rate, offset_s)


def merge_words(tokens: Sequence[str], starts: Sequence[float], ends: Sequence[float], confs: Sequence[float],
                boundary: str = "▁"):
    """SentencePiece tokens -> words: a token that begins with the word boundary mark starts a new word.  Each word:
    {"word", "start" (its first token's), "end" (its last token's), "conf" (product of its tokens' confidences)}."""
    words = []
    for tok, a, b, c in zip(tokens, starts, ends, confs):
        piece = tok.replace(boundary, "")
        if tok.startswith(boundary) or not words:
            if tok.startswith(boundary) and not piece:   # a lone boundary mark: the next token starts the word
                words.append({"word": "", "start": a, "end": b, "conf": float(c)})
                continue
            if words and words[-1]["word"] == "":
                w = words[-1]
                w["word"], w["end"], w["conf"] = piece, b, w["conf"] * float(c)
                continue
            words.append({"word": piece, "start": a, "end": b, "conf": float(c)})
        else:
            w = words[-1]
            w["word"] += piece
            w["end"] = b
            w["conf"] *= float(c)
    return [w for w in words if w["word"] != ""]
