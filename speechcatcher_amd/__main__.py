"""``python -m speechcatcher_amd <media.wav>`` - the file mode of the reference CLI on the MI355X engine.

Flags follow speechcatcher/speechcatcher.py:756-808 (``main``) and the file path of ``recognize_file`` /
``recognize`` (:358-400, :414-572): 16 kHz mono recording -> endpointing into segments (> 60 s) -> chunked
streaming decode of every segment (``--chunk-length`` samples per call, is_final on the last chunk of a segment,
reset() after it) -> paragraphs -> ``<input>.txt`` and ``<input>.json``.

Differences to the reference CLI, all on the host side: only ``--decoder native`` exists here; the device is a ROCm
GPU (no CPU path); ``-n`` is the number of parallel stream slots of ONE model replica instead of worker processes
(default 1 = the reference's behaviour on a GPU: segments decoded serially on one model, speechcatcher.py:823-825);
input must be a RIFF/WAVE file - 8 / 16 / 24-bit PCM, 32-bit float, A-law or mu-law, 1..8 channels
(speechcatcher_amd.pcm.read_wav) - at 16 kHz or at any rate the engine converts (8000..48000 Hz, speechcatcher_amd.resample).
Mono 16-bit files take the int16 samples as they are; anything else is decoded once, whole, on the GPU
(hip_backend.decode_recording); the recording is then resampled once on the GPU if need be and takes the 16 kHz int16
path.  A recording with more than one channel is refused, as it always was, unless ``--channel`` says what to decode:
``--channel N`` one channel, ``--channel mix`` the downmix of all (two speakers of a call on two channels are two
transcripts, not one: the choice is the caller's).  The ffmpeg conversion of other media, microphone mode and model
download are out of scope - pass a local model directory or a .scasr blob as ``-m``.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np


def read_wav_16k_mono(path, channel=None, device="cuda:0"):
    """A RIFF/WAVE recording -> (mono samples, rate).  Mono 16-bit PCM: its int16 samples, as they are.  Anything else the
    reader takes (speechcatcher_amd.pcm.read_wav): float32 samples in +-1 as a device tensor, decoded once, whole, on the
    GPU (hip_backend.decode_recording).  ``channel``: an index, or "mix" / pcm.MIX for the downmix; None refuses a
    recording with more than one channel."""
    from . import pcm
    from .resample import MAX_RATE, MIN_RATE, rate_params
    try:
        wav = pcm.read_wav(path)
    except ValueError as e:
        raise SystemExit(f"Error: {e} (the reference converts other media with ffmpeg first: ffmpeg -i in -ac 1 -ar 16000 "
                         "out.wav)")
    if rate_params(wav.sample_rate) is None:
        raise SystemExit(f"Error: '{path}' is at {wav.sample_rate} Hz; this entry point reads 16 kHz mono recordings, or WAV at "
                         f"{MIN_RATE}..{MAX_RATE} Hz which it resamples")
    if channel == "mix":
        channel = pcm.MIX
    if channel is None and wav.channels > 1:
        raise SystemExit(f"Error: '{path}' has {wav.channels} channels; this entry point reads 16 kHz mono recordings (or mono "
                         f"at {MIN_RATE}..{MAX_RATE} Hz) unless --channel N or --channel mix says which part of a multichannel "
                         "recording to decode")
    if channel is not None and not pcm.MIX <= int(channel) < wav.channels:
        raise SystemExit(f"Error: --channel {channel}: '{path}' has {wav.channels} channel(s)")
    if wav.format == pcm.S16LE and wav.channels == 1:
        return np.frombuffer(wav.data, dtype="<i2"), wav.sample_rate
    from .hip_backend import decode_recording
    x, _level = decode_recording(wav.data, wav.format, wav.channels, 0 if channel is None else int(channel),
                                 pcm.SCALE_FULL, device)
    return x, wav.sample_rate


def to_16k(raw, rate, device="cuda:0"):
    """recording at ``rate`` (int16, or float32 in +-1 from read_wav_16k_mono) -> int16 at 16 kHz: resampled once, whole,
    on the GPU (hip_backend.resample) if need be"""
    if rate == 16000 and isinstance(raw, np.ndarray) and raw.dtype == np.int16:
        return raw
    if isinstance(raw, np.ndarray):
        raw = raw.astype(np.float32) / 32768.0
    if rate != 16000:
        from .hip_backend import resample
        raw = resample(raw, rate, device)
    y = raw.cpu().numpy() if not isinstance(raw, np.ndarray) else raw
    return np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)


def recognize_file(speech2text, media_path, output_file="", quiet=True, progress=True, num_slots=1, chunk_length=8192,
                   token_alignment=False, segmentation="host", channel=None, token_alternates=0, ctc_beam=0,
                   ctc_only=False, ctc_lm=None, lm_weight=0.5, word_bonus=0.0, rescore_lm=None, rescore_weight=0.5,
                   rescore_bonus=0.0, ctc_grammar=None, attention_rescore=None, consensus=None):
    """speechcatcher.py:358-400: recording -> text + paragraphs JSON next to the input.  ``token_alignment``: the
    paragraphs also get token_start / token_end (seconds) and token_conf from a CTC forced alignment of each segment.
    ``segmentation``: "host" or "gpu" - where the energy curve for the cut points of a recording over 60 s is computed.
    ``channel``: what to decode of a multichannel recording - an index, or "mix" (None: such a recording is refused).
    ``token_alternates`` = K > 0 (implies ``token_alignment``): the paragraphs also get token_alternates, one record per
    token with its K acoustic alternates over the token's frames.  ``ctc_beam`` = B > 0: the paragraphs also get ctc_nbest,
    per segment the n-best list of the CTC prefix beam search; ``ctc_only``: the segments are decoded by that search alone,
    with no attention decoder step (B = 8 unless ``ctc_beam`` says otherwise; not with ``token_alternates``).  ``ctc_lm``:
    the path of a packed n-gram model (python -m speechcatcher_amd.ngram) fused into that search with ``lm_weight`` and
    ``word_bonus`` (needs ``ctc_beam`` or ``ctc_only``).  ``rescore_lm``: the path of a packed n-gram model the final
    n-best list of every segment is rescored with and re-ranked by, at ``rescore_weight`` / ``rescore_bonus`` (not with
    ``ctc_only``).  ``ctc_grammar``: the path of a compiled grammar (python -m speechcatcher_amd.grammar) or of a text file
    with one phrase per line - the CTC beam answers only from it (needs ``ctc_beam`` or ``ctc_only``; not with ``ctc_lm``).
    ``consensus``: True - every segment's text is the minimum-Bayes-risk row of its final n-best list - or "confidence" -
    the text stays the search's; both: the paragraphs get token_consensus / token_rival per token and mbr per segment
    (needs a beam of at least 2)."""
    if ctc_grammar and not (ctc_only or int(ctc_beam)):
        raise SystemExit("Error: --ctc-grammar constrains the CTC prefix beam search: it needs --ctc-beam or --ctc-only")
    if ctc_grammar and ctc_lm:
        raise SystemExit("Error: --ctc-grammar and --ctc-lm together are not served")
    if ctc_grammar and not os.path.isfile(ctc_grammar):
        raise SystemExit(f"Error: --ctc-grammar: '{ctc_grammar}' does not exist or is not a file")
    if consensus and max(int(getattr(speech2text, "beam_size", 0) or 0), int(ctc_beam), 8 if ctc_only else 0) < 2:
        raise SystemExit("Error: --consensus compares the rows of an n-best list: it needs --beamsize of at least 2")
    if attention_rescore is not None and not ctc_only:
        raise SystemExit("Error: --attention-rescore re-ranks the n-best list of a decoder-free segment: it needs --ctc-only")
    if rescore_lm and ctc_only:
        raise SystemExit("Error: --rescore-lm re-ranks the n-best list of the attention decoder's search: not with --ctc-only")
    if rescore_lm and not os.path.isfile(rescore_lm):
        raise SystemExit(f"Error: --rescore-lm: '{rescore_lm}' does not exist or is not a file")
    if ctc_lm and not (ctc_only or int(ctc_beam)):
        raise SystemExit("Error: --ctc-lm is fused into the CTC prefix beam search: it needs --ctc-beam or --ctc-only")
    if ctc_lm and not os.path.isfile(ctc_lm):
        raise SystemExit(f"Error: --ctc-lm: '{ctc_lm}' does not exist or is not a file")
    if ctc_only and token_alternates:
        raise SystemExit("Error: --ctc-only has no forced alignment to rank token alternates in: not with --token-alternates")
    if not 0 <= int(ctc_beam) <= 16:
        raise SystemExit("Error: --ctc-beam must lie in [1, 16]")
    from .config import SearchConfig
    from .native import NativeStreamBatch
    from .segmenter import recognize_recording
    raw, rate = read_wav_16k_mono(media_path, channel, speech2text.device)
    raw, rate = to_16k(raw, rate, speech2text.device), 16000
    seconds = len(raw) / float(rate)
    # capacities for the longest segment the endpointer may produce (it cuts at <= 180 s: simple_endpointing)
    seg_s = min(seconds, 200.0) + 2.0
    batch = NativeStreamBatch(speech2text.weights, max(1, num_slots),
                              SearchConfig(beam_size=speech2text.beam_size, ctc_weight=speech2text.ctc_weight,
                                           use_bbd=speech2text.use_bbd),
                              max_frames=int(seg_s * 25) + 64, max_tokens=min(2048, int(seg_s * 12) + 64),
                              pcm_capacity=max(1 << 20, int(seg_s * rate) + chunk_length),
                              max_chunk_samples=max(chunk_length, 32768), engine=speech2text.batch.engine)
    # finalize_all only with the very last chunk of the recording, like the reference CLI (speechcatcher.py:586)
    text, info = recognize_recording(batch, raw, rate, chunk_length=chunk_length, token_list=speech2text.token_list,
                                     reference_finalize=True, token_alignment=token_alignment,
                                     segmentation=segmentation, token_alternates=token_alternates,
                                     ctc_beam=int(ctc_beam) or None, ctc_only=ctc_only, ctc_lm=ctc_lm or None,
                                     lm_weight=float(lm_weight), word_bonus=float(word_bonus),
                                     rescore_lm=rescore_lm or None, rescore_weight=float(rescore_weight),
                                     rescore_bonus=float(rescore_bonus),
                                     **({"ctc_grammar": ctc_grammar} if ctc_grammar else {}),
                                     **({} if attention_rescore is None else {"attention_rescore": (float(attention_rescore), 0.5)}),
                                     **({"consensus": consensus} if consensus else {}))
    out_txt, out_json = (output_file or media_path) + ".txt", (output_file or media_path) + ".json"
    with open(out_txt, "w") as f:
        f.write(text)
    complete = {"complete_text": text, "paragraphs": info}
    with open(out_json, "w") as f:
        f.write(json.dumps(complete, indent=4))
    if not quiet:
        sys.stdout.write(text)
    print(f"Wrote transcription to {out_txt} and {out_json}.")
    return complete


def make_parser():
    p = argparse.ArgumentParser(prog="python -m speechcatcher_amd",
                                description="Decode speech with speechcatcher models on an MI355X (native decoder path).")
    p.add_argument("-l", "--live-transcription", dest="live", action="store_true",
                   help="(not available here: microphone mode is host I/O of the reference CLI)")
    p.add_argument("-m", "--model", dest="model", default="de_streaming_transformer_xl",
                   help="model tag (needs espnet_model_zoo, like the reference), a local model directory, or a .scasr blob")
    p.add_argument("-d", "--device", dest="device", default="cuda", help="'cuda' (there is no CPU path)")
    p.add_argument("-b", "--beamsize", dest="beamsize", type=int, default=5, help="beam size for the decoder")
    p.add_argument("--decoder", dest="decoder", choices=["native", "espnet"], default="native",
                   help="only 'native' is implemented")
    p.add_argument("--fp16", dest="fp16", action="store_true",
                   help="accepted like the reference does: the native decoder stays fp32 (speechcatcher.py:205-210)")
    p.add_argument("--disable-bbd", dest="disable_bbd", action="store_true", help="disable block boundary detection")
    p.add_argument("--quiet", dest="quiet", action="store_true")
    p.add_argument("--no-progress", dest="no_progress", action="store_true")
    p.add_argument("--num-threads", dest="num_threads", type=int, default=1, help="(host threads: unused on the GPU path)")
    p.add_argument("--cache-dir", dest="cache_dir", default="~/.cache/espnet")
    p.add_argument("-n", "--num-processes", dest="num_processes", type=int, default=-1,
                   help="parallel stream slots for the segments of a long recording (-1: 1, the reference's GPU behaviour)")
    p.add_argument("--chunk-length", dest="chunk_length", type=int, default=8192,
                   help="raw audio samples per streaming call (default 8192)")
    p.add_argument("--log-level", dest="log_level", default="ERROR", choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"])
    p.add_argument("--show-ffmpeg-output", dest="show_ffmpeg_output", action="store_true", help="(unused: no ffmpeg step)")
    p.add_argument("--token-alignment", dest="token_alignment", action="store_true",
                   help="add token_start / token_end / token_conf to the .json: token times at 40 ms resolution and a per-token "
                        "confidence from a CTC forced alignment on the GPU (token_timestamps stay as they are)")
    p.add_argument("--token-alternates", dest="token_alternates", type=int, default=0, metavar="K",
                   help="add token_alternates to the .json: per token the K (1..8) tokens that fit its frames best acoustically, "
                        "each with a confidence, and the rank of the token itself among them (implies --token-alignment)")
    p.add_argument("--ctc-beam", dest="ctc_beam", type=int, default=0, metavar="B",
                   help="add ctc_nbest to the .json: per segment the B (1..16) best transcripts of a CTC prefix beam search over "
                        "the encoder's CTC output, each with its log probability and its share of the listed mass")
    p.add_argument("--ctc-only", dest="ctc_only", action="store_true",
                   help="decode with the CTC prefix beam search alone: no attention decoder step, the transcript is the beam's "
                        "best (B = 8 unless --ctc-beam says otherwise; not with --token-alternates)")
    p.add_argument("--ctc-lm", dest="ctc_lm", default="", metavar="FILE",
                   help="fuse a backoff n-gram language model into the CTC prefix beam search (needs --ctc-beam or --ctc-only): "
                        "a file packed by `python -m speechcatcher_amd.ngram in.arpa tokens.txt out.sclm`")
    p.add_argument("--ctc-grammar", dest="ctc_grammar", default="", metavar="FILE",
                   help="answer only from a list: the CTC prefix beam search is constrained to the phrases of FILE and their "
                        "concatenations (needs --ctc-beam or --ctc-only; not with --ctc-lm): a grammar compiled by `python -m "
                        "speechcatcher_amd.grammar phrases.txt tokens.txt out.scgr`, or a text file with one phrase per line")
    p.add_argument("--lm-weight", dest="lm_weight", type=float, default=0.5, metavar="A",
                   help="weight of the model's log probability in the beam's ranking (default 0.5; a parameter, not tuned)")
    p.add_argument("--word-bonus", dest="word_bonus", type=float, default=0.0, metavar="B",
                   help="bonus per token of a prefix in the beam's ranking (default 0)")
    p.add_argument("--rescore-lm", dest="rescore_lm", default="", metavar="FILE",
                   help="rescore the final n-best list of every segment with a backoff n-gram language model on the GPU and "
                        "report the fused best (a file packed by `python -m speechcatcher_amd.ngram`; not with --ctc-only)")
    p.add_argument("--rescore-weight", dest="rescore_weight", type=float, default=0.5, metavar="A",
                   help="weight of the model's log probability, </s> included, in the re-ranking (default 0.5; a parameter, "
                        "not tuned)")
    p.add_argument("--rescore-bonus", dest="rescore_bonus", type=float, default=0.0, metavar="B",
                   help="bonus per token of a hypothesis in the re-ranking (default 0)")
    p.add_argument("--attention-rescore", dest="attention_rescore", type=float, nargs="?", const=1.0, default=None, metavar="W_ATT",
                   help="with --ctc-only: re-rank every segment's final n-best list by one teacher-forced pass of the attention "
                        "decoder over the segment's encoder output, fused = 0.5 * ctc + W_ATT * att (default 1.0; parameters, not "
                        "tuned); the segment .json carries the re-ranked ctc_nbest")
    p.add_argument("--consensus", dest="consensus", action="store_const", const=True, default=None,
                   help="report the minimum-Bayes-risk row of every segment's final n-best list under the edit distance "
                        "instead of the best-scored one, and add token_consensus / token_rival / mbr to the .json: per token "
                        "the share of the list's mass that agrees on it and its strongest rival (needs --beamsize >= 2)")
    p.add_argument("--consensus-confidence", dest="consensus", action="store_const", const="confidence",
                   help="as --consensus, but the transcript stays the best-scored row: only the statistics are added")
    p.add_argument("--segmentation", dest="segmentation", choices=["host", "gpu"], default="host",
                   help="where the energy curve for the cut points of a recording over 60 s is computed: 'host' (numpy, the "
                        "default) or 'gpu' (float64 kernels; the same cuts, without the host pass over the whole recording)")
    p.add_argument("--channel", dest="channel", type=lambda v: "mix" if v == "mix" else int(v), default=None,
                   help="what to decode of a recording with more than one channel: a channel index from 0, or 'mix' for the "
                        "downmix of all channels (without it such a recording is refused)")
    p.add_argument("inputfile", nargs="?", default="",
                   help="input recording: WAV, 8 / 16 / 24-bit PCM, 32-bit float, A-law or mu-law, 1..8 channels, 16 kHz or "
                        "8000..48000 Hz.  The recording is quantised to 16 bits before it is decoded: 24-bit and float input "
                        "lose what lies below that")
    return p


def main(argv=None):
    p = make_parser()
    args = p.parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level))
    if args.decoder != "native":
        raise SystemExit("Error: only --decoder native is implemented by speechcatcher_amd")
    if args.live:
        raise SystemExit("Error: live transcription (microphone) is not part of this package")
    if args.inputfile == "":
        p.print_help()
        return 0
    if not os.path.isfile(args.inputfile):
        print(f"Error: Input file '{args.inputfile}' does not exist or is not a valid file.")
        return -1
    from .speech2text_streaming import load_model
    speech2text = load_model(tag=args.model, device=args.device, beam_size=args.beamsize, quiet=args.quiet,
                             cache_dir=args.cache_dir, decoder_impl=args.decoder, fp16=args.fp16,
                             use_bbd=not args.disable_bbd)
    recognize_file(speech2text, args.inputfile, quiet=args.quiet or not args.no_progress, progress=not args.no_progress,
                   num_slots=1 if args.num_processes < 1 else args.num_processes, chunk_length=args.chunk_length,
                   token_alignment=args.token_alignment or args.token_alternates > 0, segmentation=args.segmentation,
                   channel=args.channel, token_alternates=args.token_alternates, ctc_beam=args.ctc_beam,
                   ctc_only=args.ctc_only, ctc_lm=args.ctc_lm or None, lm_weight=args.lm_weight, word_bonus=args.word_bonus,
                   rescore_lm=args.rescore_lm or None, rescore_weight=args.rescore_weight, rescore_bonus=args.rescore_bonus,
                   **({"ctc_grammar": args.ctc_grammar} if args.ctc_grammar else {}),
                   **({} if args.attention_rescore is None else {"attention_rescore": args.attention_rescore}),
                   **({"consensus": args.consensus} if args.consensus else {}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
