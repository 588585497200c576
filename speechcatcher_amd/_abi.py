"""ctypes binding of libscasr.so (the C ABI declared in include/scasr.h).

cffi is not installed in the target image, so the
"thin C-ABI cffi layer" of the north star is ctypes in ABI mode; the binding
is plain C, nothing torch-specific crosses it.

The library is built in-tree (speechcatcher_amd/libscasr.so) by
``build()`` / ``__graft_entry__.build()``; loading fails LOUDLY when it is
missing - there is no CPU fallback in the product path.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libscasr.so"
CSRC = HERE / "csrc"

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int32)
c_double_p = C.POINTER(C.c_double)
vp = C.c_void_p


class EncLayer(C.Structure):
    _fields_ = [(n, vp) for n in ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo",
                                  "ln2_g", "ln2_b", "w1", "b1", "w2", "b2", "w1_p", "w2_p",
                                  "wqkv_p", "wo_p", "w1_h", "w2_h", "wqkv_h", "wo_h", "w1_s", "w2_s",
                                  "wqkv_s", "wo_s")]


class DecLayer(C.Structure):
    _fields_ = [(n, vp) for n in ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo",
                                  "ln2_g", "ln2_b", "wq", "bq", "wo2", "bo2",
                                  "ln3_g", "ln3_b", "w1", "b1", "w2", "b2",
                                  "wo_p", "wq_p", "wo2_p", "w1_p", "w2_p", "wqkv_q", "wqkv_pp", "wq_pp", "wo_pp", "wo2_pp", "w1_h", "w2_h",
                                  "w1_s", "w2_s", "wqkv_pph", "wq_pph", "wo_pph", "wo2_pph")]


class Search(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ("S", "W", "K", "V", "d", "H", "F", "n_layers", "TCAP", "LCAP",
                                  "blank", "eos", "sos")]
        + [(n, C.c_float) for n in ("w_dec", "w_ctc", "ln_eps")]
        + [(n, vp) for n in ("ctrl", "flags", "ctcx", "ckv", "skv", "yseq", "xpos", "anc", "score",
                             "sc_dec", "sc_ctc", "ctc_r", "ctc_s", "ctc_rnew", "dx", "dxn", "dqkv",
                             "datt", "dq", "dffh", "logits", "logp", "pre_ids", "psi", "psi_eos",
                             "cand_score", "cand_tok", "cand_ctc", "sel", "embed", "pe",
                             "dec_norm_g", "dec_norm_b", "out_w", "out_b", "layers", "rowmap")]
        + [("n_rows", C.c_int32), ("out_w_q", vp), ("ph1", vp), ("ph2", vp), ("ffn_part", vp),
           ("max_ffn_part", C.c_int32), ("tct", C.c_int32), ("ctcxT", vp), ("kv_half", C.c_int32), ("stat_rows", vp),
           ("out_w_qh", vp), ("act_half", C.c_int32), ("kv_rows", C.c_int32), ("kvflags", vp), ("ctc_rs", vp)]
    )


class Config(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("d_model", "enc_heads", "enc_layers", "dec_heads", "dec_layers", "ffn_dim",
                                           "vocab_size", "n_mels", "n_fft", "win_length", "hop_length", "sample_rate",
                                           "block_size", "hop_size", "look_ahead", "subsample", "conv_freq1",
                                           "conv_freq2", "blank_id", "sos_id", "eos_id", "pe_max_len", "mvn_mode")]
                + [("ln_eps", C.c_float)])


class NamedTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", vp), ("numel", C.c_int64), ("dtype", C.c_int32)]


class StreamOptions(C.Structure):
    _fields_ = [("n_streams", C.c_int32), ("beam_size", C.c_int32), ("ctc_weight", C.c_float), ("use_bbd", C.c_int32),
                ("max_frames", C.c_int32), ("max_tokens", C.c_int32), ("pcm_capacity", C.c_int32),
                ("max_chunk_samples", C.c_int32), ("strict_reference", C.c_int32), ("kv_half", C.c_int32),
                ("kv_pool_rows", C.c_int32)]


class AlignJob(C.Structure):
    """sc_ctc_align_job (include/scasr.h): one CTC forced alignment of sc_ctc_align"""
    _fields_ = ([(n, vp) for n in ("emis", "labels", "ws", "start", "end", "logp_mean", "path_score", "status")]
                + [("stride", C.c_int64)] + [(n, C.c_int32) for n in ("T", "L", "V", "blank")])


class ActivityJob(C.Structure):
    """sc_ctc_activity_job (include/scasr.h): one span of CTC rows scanned by sc_ctc_activity"""
    _fields_ = ([(n, vp) for n in ("table", "state", "track", "state_after")] + [("stride", C.c_int64), ("thr", C.c_double)]
                + [(n, C.c_int32) for n in ("V", "blank", "t0", "t1", "restart", "reserved")])


class Activity(C.Structure):
    """sc_activity_t (include/scasr.h)"""
    _fields_ = [(n, C.c_int32) for n in ("n_frames", "n_speech", "n_bad", "first_speech", "last_speech", "trail_silence")]


ACTIVITY_FIELDS = tuple(n for n, _ in Activity._fields_)
ACTIVITY_MAX_JOBS = 65535


class SpotEvent(C.Structure):
    """sc_spot_event (include/scasr.h)"""
    _fields_ = [(n, C.c_int32) for n in ("end", "phrase", "start", "reserved")] + [("score", C.c_double)]


class Spot(C.Structure):
    """sc_spot_t (include/scasr.h)"""
    _fields_ = [("n_frames", C.c_int32), ("n_events", C.c_int32)]


class SpotJob(C.Structure):
    """sc_ctc_spot_job (include/scasr.h): one span of CTC rows scanned by sc_ctc_spot"""
    _fields_ = ([(n, vp) for n in ("table", "labels", "lens", "floors", "counters", "values", "starts", "events",
                                   "state_after")] + [("stride", C.c_int64), ("mask", C.c_uint64)]
                + [(n, C.c_int32) for n in ("V", "blank", "t0", "t1", "restart", "P")])


SPOT_MAX_PHRASES, SPOT_MAX_LEN, SPOT_STATES, SPOT_MAX_EVENTS, SPOT_MAX_JOBS = 64, 32, 64, 64, 65535



class Draft(C.Structure):
    """sc_draft_t (include/scasr.h)"""
    _fields_ = ([(n, C.c_int32) for n in ("n_frames", "n_closed", "n_bad", "open_id", "open_start", "open_end")]
                + [("open_conf", C.c_double)])


class DraftToken(C.Structure):
    """sc_draft_token (include/scasr.h)"""
    _fields_ = [(n, C.c_int32) for n in ("id", "start", "end", "reserved")] + [("conf", C.c_double)]


class DraftJob(C.Structure):
    """sc_ctc_draft_job (include/scasr.h): one span of CTC rows scanned by sc_ctc_draft"""
    _fields_ = ([(n, vp) for n in ("table", "state", "tokens", "state_after")] + [("stride", C.c_int64)]
                + [(n, C.c_int32) for n in ("V", "blank", "t0", "t1", "restart", "capacity")])


DRAFT_FIELDS = tuple(n for n, _ in Draft._fields_)
DRAFT_MAX_JOBS = 65535

BEAM_MAX, BEAM_MAX_JOBS = 16, 65535
# SC_BEAM_PACK_* of include/scasr.h
BEAM_PACK_OK, BEAM_PACK_NO_ENTRY, BEAM_PACK_TRUNCATED, BEAM_PACK_BROKEN = 0, 1, 2, 3
# SC_DECODER_* of include/scasr.h
DECODER_FULL, DECODER_NONE = 0, 1


class BeamEntry(C.Structure):
    """sc_beam_entry (include/scasr.h)"""
    _fields_ = [(n, C.c_int32) for n in ("node", "last", "len", "parent")] + [("pb", C.c_double), ("pnb", C.c_double)]


class Beam(C.Structure):
    """sc_beam_t (include/scasr.h)"""
    _fields_ = [(n, C.c_int32) for n in ("n_frames", "n_bad", "n_nodes", "n_entries")] + [("e", BeamEntry * BEAM_MAX)]


class BeamNode(C.Structure):
    """sc_beam_node (include/scasr.h)"""
    _fields_ = [(n, C.c_int32) for n in ("parent", "token", "frame", "reserved")]


class BeamJob(C.Structure):
    """sc_ctc_beam_job (include/scasr.h): one span of CTC rows searched by sc_ctc_beam"""
    _fields_ = ([(n, vp) for n in ("table", "state", "nodes", "state_after")] + [("stride", C.c_int64)]
                + [(n, C.c_int32) for n in ("V", "blank", "t0", "t1", "restart", "capacity", "B", "C")])


class BeamLm(C.Structure):
    """sc_beam_lm_t (include/scasr.h): beside the entries of a sc_beam_t, the model's sum along each prefix and the
    automaton's state after it"""
    _fields_ = [("lm", C.c_double * BEAM_MAX), ("ctx", C.c_int32 * BEAM_MAX)]


class BeamLmJob(C.Structure):
    """sc_ctc_beam_lm_job (include/scasr.h): a sc_ctc_beam_job with a language model fused in"""
    _fields_ = [("beam", BeamJob), ("lm", vp), ("lm_state", vp), ("lm_state_after", vp), ("alpha", C.c_double),
                ("beta", C.c_double)]


class LmHeader(C.Structure):
    """sc_lm_header (include/scasr.h): the first bytes of a language model blob (speechcatcher_amd/ngram.py packs it)"""
    _fields_ = [(n, C.c_int32) for n in ("magic", "version", "V", "order", "n_states", "n_arcs", "n_slots", "start_state")]


class LmSlot(C.Structure):
    """sc_lm_slot (include/scasr.h): one slot of the arc hash table"""
    _fields_ = [("key", C.c_uint64), ("logp", C.c_double), ("next", C.c_int32), ("reserved", C.c_int32)]


class LmView(C.Structure):
    """sc_lm_view (include/scasr.h): the automaton as the kernel reads it"""
    _fields_ = ([(n, vp) for n in ("backoff", "bo_state", "root_logp", "root_next", "slots")]
                + [(n, C.c_int32) for n in ("V", "order", "n_states", "n_slots", "start_state", "shift")])


LM_MAX_ORDER, LM_MAGIC, LM_VERSION = 5, 0x4D4C4353, 1


class GrammarHeader(C.Structure):
    """sc_grammar_header (include/scasr.h): the first bytes of a grammar blob (speechcatcher_amd/grammar.py compiles it)"""
    _fields_ = [(n, C.c_int32) for n in ("magic", "version", "V", "blank", "n_states", "n_arcs", "start_state", "reserved")]


class GrammarView(C.Structure):
    """sc_grammar_view (include/scasr.h): the automaton as the kernel reads it"""
    _fields_ = ([(n, vp) for n in ("arc_off", "arc_tok", "arc_next", "accept")]
                + [(n, C.c_int32) for n in ("V", "blank", "n_states", "n_arcs", "start_state", "reserved")])


class BeamGr(C.Structure):
    """sc_beam_gr_t (include/scasr.h): beside the entries of a sc_beam_t, the grammar's state after each prefix"""
    _fields_ = [("g", C.c_int32 * BEAM_MAX)]


class BeamGrJob(C.Structure):
    """sc_ctc_beam_gr_job (include/scasr.h): a sc_ctc_beam_job whose candidates a grammar chooses"""
    _fields_ = [("beam", BeamJob), ("grammar", vp), ("gr_state", vp), ("gr_state_after", vp)]


GRAMMAR_MAGIC, GRAMMAR_VERSION, GRAMMAR_MAX_STATES, GRAMMAR_MAX_ARCS = 0x52474353, 1, 1 << 20, 1 << 24


class RescoreJob(C.Structure):
    """sc_lm_rescore_job (include/scasr.h): one n-best list rescored by sc_lm_rescore"""
    _fields_ = ([(n, vp) for n in ("model", "yseq", "score", "lens", "lm", "eos_lm", "fused", "end_state", "order",
                                   "status", "tok_lm")]
                + [(n, C.c_int64) for n in ("row_stride", "score_stride", "tok_stride")]
                + [("alpha", C.c_double), ("beta", C.c_double)]
                + [(n, C.c_int32) for n in ("n_hyp", "L", "skip", "strip", "state0", "lm_eos", "V", "flags")])


# SC_RESCORE_* of include/scasr.h
RESCORE_MAX_HYPS, RESCORE_MAX_JOBS, RESCORE_FORCE_SERIAL = 16, 65535, 1
RESCORE_NONFINITE, RESCORE_BAD_TOKEN, RESCORE_SERIAL = 1, 2, 4


class MbrJob(C.Structure):
    """sc_mbr_job (include/scasr.h): one n-best list whose consensus sc_mbr computes"""
    _fields_ = ([(n, vp) for n in ("yseq", "score", "weight", "lens", "weight_out", "risk", "dist", "order", "status",
                                   "header", "conf", "alt_mass", "gap_mass", "alt_tok", "slots")]
                + [(n, C.c_int64) for n in ("row_stride", "score_stride", "slot_stride")]
                + [("scale", C.c_double)]
                + [(n, C.c_int32) for n in ("n_hyp", "L", "skip", "strip", "V", "pivot", "flags", "reserved")])


# SC_MBR_* of include/scasr.h
MBR_MAX_HYPS, MBR_MAX_LEN, MBR_MAX_JOBS = 16, 1024, 65535
MBR_NONFINITE, MBR_BAD_TOKEN, MBR_TOO_LONG, MBR_NO_PIVOT = 1, 2, 4, 8


class SeqAttnJob(C.Structure):
    """sc_seq_attn_job (include/scasr.h): the attention of one sequence in sc_seq_attention"""
    _fields_ = ([(n, vp) for n in ("q", "k", "v", "o")]
                + [(n, C.c_int64) for n in ("q_stride", "k_stride", "v_stride", "o_stride")]
                + [(n, C.c_int32) for n in ("Lq", "Lk", "H", "causal")])


class DecRescoreJob(C.Structure):
    """sc_dec_rescore_job (include/scasr.h): one n-best list rescored by the attention decoder in sc_dec_rescore"""
    _fields_ = ([(n, vp) for n in ("E", "yseq", "score", "lens", "wkv", "bkv", "att", "fused", "order", "status", "tok_att")]
                + [(n, C.c_int64) for n in ("e_stride", "row_stride", "score_stride", "tok_stride")]
                + [(n, C.c_double) for n in ("w_att", "w_ctc", "beta")]
                + [(n, C.c_int32) for n in ("n_hyp", "L", "T", "pe_rows")])


# SC_ATT_* / SC_SEQ_ATTN_* of include/scasr.h
ATT_MAX_HYPS, ATT_MAX_JOBS, SEQ_ATTN_MAX_JOBS = 16, 65535, 1 << 24
ATT_NONFINITE, ATT_BAD_TOKEN, ATT_TOO_LONG, ATT_NO_FRAMES = 1, 2, 4, 8
ERR_CAPACITY, ERR_UNSUPPORTED = -3, -5


class BeamPackJob(C.Structure):
    """sc_ctc_beam_pack_job (include/scasr.h): one entry of a beam state walked up its parent chain"""
    _fields_ = ([(n, vp) for n in ("state", "nodes", "ids", "frames", "header", "scores")]
                + [(n, C.c_int32) for n in ("capacity", "rank", "max_len", "reserved")])


class AltJob(C.Structure):
    """sc_ctc_alt_job (include/scasr.h): the token spans of one label sequence ranked by sc_ctc_alternates"""
    _fields_ = ([(n, vp) for n in ("emis", "labels", "start", "end", "alt_ids", "alt_logp", "own_rank", "status")]
                + [("stride", C.c_int64)] + [(n, C.c_int32) for n in ("T", "V", "blank", "L")])


# SC_ALT_* of include/scasr.h
ALT_OK, ALT_NO_SPAN, ALT_BAD_ROW = 0, 1, 2
ALT_MAX_K, ALT_MAX_JOBS = 8, 65535


class CommitJob(C.Structure):
    """sc_hyp_commit_job (include/scasr.h): the live beam of one stream handed to sc_hyp_commit"""
    _fields_ = ([(n, vp) for n in ("yseq", "xpos", "score", "score_dec", "score_ctc", "header", "agree", "ids", "pos",
                                   "stability", "totals")]
                + [("row_stride", C.c_int64), ("score_stride", C.c_int64)]
                + [(n, C.c_int32) for n in ("n_hyp", "L", "frm", "flags")])


# SC_COMMIT_* of include/scasr.h
COMMIT_MAX_HYPS, COMMIT_FINAL, COMMIT_NONFINITE, COMMIT_MAX_JOBS = 16, 1, 1, 65535


class InputLevel(C.Structure):
    """sc_input_level_t (include/scasr.h)"""
    _fields_ = ([(n, C.c_int64) for n in ("frames", "clipped", "sum_abs")]
                + [(n, C.c_int32) for n in ("peak", "full_scale")])


class PcmJob(C.Structure):
    """sc_pcm_job (include/scasr.h): one chunk of coded audio decoded by sc_pcm_decode"""
    _fields_ = ([(n, vp) for n in ("src", "dst", "level", "level_after")] + [("offset", C.c_int64)]
                + [(n, C.c_int32) for n in ("format", "channels", "channel", "scale", "n", "restart")])


LEVEL_FIELDS = tuple(n for n, _ in InputLevel._fields_)
PCM_MAX_JOBS = 65535

# SC_ALIGN_* of include/scasr.h
ALIGN_OK, ALIGN_INFEASIBLE, ALIGN_NONFINITE, ALIGN_BAD_INPUT = 0, 1, 2, 3
ALIGN_MAX_L = 1023
# SC_MAX_VOCAB of include/scasr.h: largest vocabulary the search kernels serve (LDS of sc_fuse_topw's full path)
MAX_VOCAB = 8192


class StreamInfo(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("enc_frames", "processed_block", "process_idx", "n_hyp", "hyp_len",
                                           "pcm_buffered", "frontend_started")] + [("decode_steps", C.c_int64)])


_SIGS = {
    "sc_last_error": (C.c_char_p, []),
    "sc_version": (C.c_int, []),
    "sc_gemm": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                          C.c_int, C.c_int, vp]),
    "sc_gemm_ln": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.c_int, C.c_int, vp, vp, C.c_float, vp, C.c_int, vp]),
    "sc_proj_ln_proj": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_float, vp, C.c_int,
                                  vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp]),
    "sc_proj_ln_proj_supported": (C.c_int, [C.c_int]),
    "sc_pack_panel_weight": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "sc_pack_lane_weight": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "sc_ffn_ln": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp]),
    "sc_ffn_ln_h": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp]),
    "sc_ffn_ln_s": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp]),
    "sc_ffn_ln_proj_s": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp,
                                   vp, vp, vp, C.c_int, vp]),
    "sc_ffn_ln_proj_h": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp,
                                   vp, vp, vp, C.c_int, vp]),
    "sc_ffn_ln_supported": (C.c_int, [C.c_int, C.c_int]),
    "sc_rowtile_proj": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_float, vp, vp, C.c_int, vp, vp,
                                  C.c_int, vp, vp, vp, vp]),
    "sc_rowtile_proj_h": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_float, vp, vp, C.c_int, vp, vp,
                                    C.c_int, vp, vp, vp, vp]),
    "sc_rowtile_proj_s": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_float, vp, vp, C.c_int, vp, vp,
                                    C.c_int, vp, vp, vp, vp]),
    "sc_rowtile_proj_supported": (C.c_int, [C.c_int, C.c_int]),
    "sc_workspace_bytes": (C.c_size_t, [vp]),
    "sc_ffn_ln_proj": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp,
                                 vp, vp, vp, C.c_int, vp]),
    "sc_graph_capture_begin": (C.c_int, [vp]),
    "sc_graph_capture_end": (C.c_int, [vp, C.POINTER(vp)]),
    "sc_graph_launch": (C.c_int, [vp, vp]),
    "sc_graph_destroy": (C.c_int, [vp]),
    "sc_set_workspace": (C.c_int, [vp, C.c_size_t]),
    "sc_set_stream_workspace": (C.c_int, [vp, vp, C.c_size_t]),
    "sc_prof_collect_kinds": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_longlong), C.c_int]),
    "sc_prof_enable": (C.c_int, [C.c_int]),
    "sc_prof_collect": (C.c_int, [c_double_p, c_double_p, C.POINTER(C.c_longlong)]),
    "sc_prof_collect2": (C.c_int, [c_double_p, c_double_p, c_double_p, C.POINTER(C.c_longlong)]),
    "sc_prof_event_overhead_ms": (C.c_double, [vp]),
    "sc_layernorm": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_float, vp]),
    "sc_copy_rows": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "sc_log_softmax_rows": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "sc_logmel": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int,
                            C.c_int, C.c_int, C.c_int, vp, vp]),
    "sc_conv1": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
    "sc_block_pack": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "sc_ctx_handoff": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp]),
    "sc_enc_attention": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "sc_encoder_layers": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp,
                                    vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "sc_glu_dwconv_bn_swish": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp,
                                         C.c_float, vp, vp]),
    "sc_relpos_attention": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "sc_relpos_attention_masked": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "sc_ctc_extend_state": (C.c_int, [vp, vp]),
    "sc_dec_embed": (C.c_int, [vp, vp]),
    "sc_kv_rows_to_half": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "sc_dec_self_attn": (C.c_int, [vp, C.c_int, vp]),
    "sc_dec_cross_attn": (C.c_int, [vp, C.c_int, vp]),
    "sc_decoder_layers": (C.c_int, [vp, vp]),
    "sc_logsoftmax_topk": (C.c_int, [vp, vp]),
    "sc_ctc_prefix_scan": (C.c_int, [vp, vp]),
    "sc_fuse_topw": (C.c_int, [vp, vp]),
    "sc_beam_prune": (C.c_int, [vp, vp]),
    "sc_ctc_gather_state": (C.c_int, [vp, vp]),
    "sc_ctc_gather_state_split": (C.c_int, [vp, C.c_int, vp]),
    "sc_decode_step": (C.c_int, [vp, vp]),
    "sc_decode_step_ex": (C.c_int, [vp, C.c_int, vp]),
    "sc_ctc_prefix_scan_split": (C.c_int, [vp, C.c_int, vp]),
    "sc_dec_layer_fused_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sc_dec_layer_self": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp]),
    "sc_dec_layer_cross": (C.c_int, [vp, C.c_int, vp, vp, vp]),
    "sc_dec_layer_ffn": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_int), vp]),
    "sc_dec_output_logits": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
    "sc_streams_kv_rows": (C.c_int, [vp]),
    "sc_dec_layer_stream_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "sc_dec_layer_stream": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]),
    "sc_dec_layer_reduce_ln": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
    "sc_dec_layer_ffn_xn": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int), vp]),
    # stream-level API
    "sc_engine_create": (C.c_int, [C.POINTER(Config), C.POINTER(NamedTensor), C.c_int, C.c_int, C.POINTER(vp)]),
    "sc_engine_load": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(vp)]),
    "sc_engine_config": (C.c_int, [vp, C.POINTER(Config)]),
    "sc_engine_destroy": (None, [vp]),
    "sc_streams_create": (C.c_int, [vp, C.POINTER(StreamOptions), C.POINTER(vp)]),
    "sc_streams_destroy": (None, [vp]),
    "sc_push": (C.c_int, [vp, c_int_p, C.POINTER(vp), c_int_p, C.POINTER(C.c_uint8), C.c_int, c_int_p]),
    "sc_push_features": (C.c_int, [vp, c_int_p, C.POINTER(vp), c_int_p, C.POINTER(C.c_uint8), C.c_int, c_int_p]),
    "sc_get_hyps": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_double_p, c_double_p,
                              c_double_p]),
    "sc_get_hyps_batch": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p,
                                    c_double_p, c_double_p, c_double_p]),
    "sc_submit": (C.c_int, [vp, c_int_p, C.POINTER(vp), c_int_p, C.POINTER(C.c_uint8), C.c_int]),
    "sc_poll": (C.c_int, [vp, C.c_int, C.c_int, c_int_p, c_int_p]),
    "sc_streams_outstanding": (C.c_int, [vp]),
    "sc_streams_set_encoder_batch": (C.c_int, [vp, C.c_int]),
    "sc_streams_set_queue_depth": (C.c_int, [vp, C.c_int]),
    "sc_stream_last_error": (C.c_char_p, [vp, C.c_int]),
    "sc_reset": (C.c_int, [vp, C.c_int]),
    "sc_stream_info": (C.c_int, [vp, C.c_int, C.POINTER(StreamInfo)]),
    "sc_streams_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "sc_streams_capture_stats": (C.c_int, [vp, C.POINTER(C.c_long), c_double_p]),
    "sc_streams_set_graphs": (C.c_int, [vp, C.c_int]),
    "sc_marker": (C.c_int, [C.c_int, vp]),
    "sc_streams_host_times": (C.c_int, [vp, c_double_p, c_double_p]),
    "sc_streams_bucket_times": (C.c_int, [vp, c_double_p, C.POINTER(C.c_long)]),
    "sc_streams_take_xattn_rows": (C.c_long, [vp]),
    "sc_streams_take_xattn_rows_by_kernel": (C.c_int, [vp, vp]),
    "sc_streams_take_attn_counters": (C.c_int, [vp, vp]),
    "sc_streams_hip_stream": (vp, [vp]),
    "sc_streams_pcm": (vp, [vp, C.POINTER(C.c_long)]),
    "sc_streams_write_pcm": (C.c_int, [vp, C.c_int, C.c_long, vp, C.c_long]),
    "sc_streams_read_pcm_buffer": (C.c_long, [vp, C.c_int, vp, C.c_long]),
    "sc_streams_read_enc": (C.c_int, [vp, C.c_int, vp, C.c_int]),
    # CTC forced alignment (align.hip, streams.hip)
    "sc_ctc_align_ws_bytes": (C.c_size_t, [C.c_int]),
    "sc_ctc_align": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]),
    "sc_align_hyps": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_float_p, c_double_p,
                                c_int_p, c_int_p]),
    "sc_align_tokens": (C.c_int, [vp, C.c_int, c_int_p, C.c_int, c_int_p, c_int_p, c_float_p, c_double_p, c_int_p]),
    "sc_streams_read_ctc": (C.c_int, [vp, C.c_int, vp, C.c_int]),
    # CTC token alternates (alternates.hip, streams.hip)
    "sc_ctc_alternates": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]),
    "sc_alternates_hyps": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_float_p,
                                     c_double_p, c_int_p, c_int_p, c_double_p, c_int_p, c_int_p, c_int_p]),
    # stable partials (commit.hip, streams.hip)
    "sc_hyp_commit": (C.c_int, [vp, C.c_int, vp]),
    "sc_get_hyps_delta": (C.c_int, [vp, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p,
                                    c_int_p, c_double_p, c_double_p, c_int_p]),
    # CTC speech activity (activity.hip, streams.hip)
    "sc_ctc_activity": (C.c_int, [vp, C.c_int, vp]),
    "sc_streams_set_activity": (C.c_int, [vp, C.c_int, C.c_double]),
    "sc_stream_activity": (C.c_int, [vp, C.c_int, C.POINTER(Activity)]),
    "sc_streams_read_activity": (C.c_int, [vp, C.c_int, vp, C.c_int]),
    # CTC phrase spotting (spot.hip, streams.hip)
    "sc_ctc_spot": (C.c_int, [vp, C.c_int, vp]),
    "sc_streams_set_phrases": (C.c_int, [vp, vp, vp, vp, C.c_int]),
    "sc_stream_set_phrase_mask": (C.c_int, [vp, C.c_int, C.c_uint64]),
    "sc_stream_spot": (C.c_int, [vp, C.c_int, C.POINTER(Spot)]),
    "sc_streams_read_spot_events": (C.c_int, [vp, C.c_int, vp, C.c_int]),
    "sc_streams_read_spot_state": (C.c_int, [vp, C.c_int, vp, vp]),
    # CTC draft transcript (draft.hip, streams.hip)
    "sc_ctc_draft": (C.c_int, [vp, C.c_int, vp]),
    "sc_streams_set_draft": (C.c_int, [vp, C.c_int]),
    "sc_stream_draft": (C.c_int, [vp, C.c_int, C.POINTER(Draft)]),
    "sc_streams_read_draft": (C.c_int, [vp, C.c_int, vp, C.c_int]),
    # CTC prefix beam search (ctc_beam.hip, streams.hip)
    "sc_ctc_beam": (C.c_int, [vp, C.c_int, vp]),
    "sc_ctc_beam_pack": (C.c_int, [vp, C.c_int, vp]),
    "sc_ctc_beam_lm": (C.c_int, [vp, C.c_int, vp]),
    "sc_lm_create": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "sc_lm_destroy": (None, [vp]),
    "sc_lm_device_view": (C.c_int, [vp, C.POINTER(vp), C.POINTER(LmView)]),
    "sc_streams_set_ctc_beam": (C.c_int, [vp, C.c_int, C.c_int]),
    "sc_stream_ctc_beam": (C.c_int, [vp, C.c_int, C.POINTER(Beam)]),
    "sc_ctc_beam_hyps": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "sc_streams_set_ctc_beam_lm": (C.c_int, [vp, vp, C.c_double, C.c_double]),
    "sc_stream_ctc_beam_lm": (C.c_int, [vp, C.c_int, C.POINTER(BeamLm)]),
    "sc_ctc_beam_hyps_lm": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, vp, vp]),
    # grammar-constrained CTC prefix beam (ctc_beam_grammar.hip)
    "sc_ctc_beam_grammar": (C.c_int, [vp, C.c_int, vp]),
    "sc_grammar_create": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "sc_grammar_destroy": (C.c_int, [vp]),
    "sc_grammar_device_view": (C.c_int, [vp, C.POINTER(vp), C.POINTER(GrammarView)]),
    "sc_grammar_use": (C.c_int, [vp, C.c_int]),
    "sc_grammar_step": (C.c_int, [vp, C.c_int, C.c_int]),
    "sc_grammar_accepts": (C.c_int, [vp, C.c_int]),
    "sc_stream_set_grammar": (C.c_int, [vp, C.c_int, vp]),
    "sc_stream_ctc_beam_grammar": (C.c_int, [vp, C.c_int, C.POINTER(BeamGr)]),
    "sc_ctc_beam_hyps_grammar": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, c_int_p, c_int_p]),
    # n-gram rescoring of n-best lists (lm_rescore.hip, streams.hip)
    "sc_lm_rescore": (C.c_int, [vp, C.c_int, vp]),
    "sc_rescore_hyps": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, vp, C.c_double, C.c_double, C.c_int, c_int_p, vp, vp,
                                  vp, vp, vp, c_int_p]),
    "sc_lm_rescore_lists": (C.c_int, [vp, vp, vp, vp, vp, c_int_p, C.c_int, C.c_int, C.c_int, vp, C.c_double,
                                      C.c_double, C.c_int, vp, vp, vp, vp, vp, vp]),
    # consensus of n-best lists (mbr.hip, stream_readback.hip)
    "sc_mbr_ws_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sc_mbr": (C.c_int, [vp, C.c_int, vp, C.c_size_t, vp]),
    "sc_mbr_hyps": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                              vp, c_int_p]),
    "sc_mbr_lists": (C.c_int, [vp, vp, vp, vp, C.c_int, c_int_p, vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp,
                               vp, vp, vp, vp, vp, vp]),
    "sc_streams_set_mbr_ws": (C.c_int, [vp, C.c_size_t]),
    "sc_streams_mbr_ws": (C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    # attention rescoring of n-best lists (dec_rescore.hip)
    "sc_seq_attention": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "sc_dec_rescore_ws_bytes": (C.c_size_t, [vp, C.c_long, C.c_long, C.c_int, C.c_int]),
    "sc_dec_rescore": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, vp]),
    "sc_attention_rescore_beam": (C.c_int, [vp, c_int_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp,
                                            vp, c_int_p]),
    "sc_attention_rescore_lists": (C.c_int, [vp, c_int_p, C.c_int, vp, vp, vp, c_int_p, C.c_int, C.c_int, C.c_double,
                                             C.c_double, C.c_double, vp, vp, vp, vp]),
    "sc_streams_set_attention_rescore_ws": (C.c_int, [vp, C.c_size_t]),
    "sc_streams_attention_rescore_ws": (C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "sc_stream_set_decoder": (C.c_int, [vp, C.c_int, C.c_int]),
    "sc_stream_decoder": (C.c_int, [vp, C.c_int]),
    "sc_streams_read_ctc_projected": (C.c_int, [vp, C.c_int, vp, C.c_int]),
    # wire-format audio in (pcm.hip)
    "sc_pcm_decode": (C.c_int, [vp, C.c_int, vp]),
    "sc_pcm_bytes_per_frame": (C.c_int, [C.c_int, C.c_int]),
    "sc_stream_set_input_format": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sc_stream_input_format": (C.c_int, [vp, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p]),
    "sc_push_raw": (C.c_int, [vp, c_int_p, C.POINTER(vp), c_int_p, C.POINTER(C.c_uint8), C.c_int, c_int_p]),
    "sc_submit_raw": (C.c_int, [vp, c_int_p, C.POINTER(vp), c_int_p, C.POINTER(C.c_uint8), C.c_int]),
    "sc_stream_input_level": (C.c_int, [vp, C.c_int, C.POINTER(InputLevel)]),
    # sample-rate conversion (resample.hip, streams.hip)
    "sc_resample_design": (C.c_int, [C.c_int, c_int_p, c_int_p, c_int_p, c_float_p]),
    "sc_resample_out_count": (C.c_long, [C.c_int, C.c_long, C.c_int]),
    "sc_resample": (C.c_long, [vp, C.c_long, C.c_int, vp, C.c_long, vp]),
    "sc_stream_set_input_rate": (C.c_int, [vp, C.c_int, C.c_int]),
    "sc_stream_input_rate": (C.c_int, [vp, C.c_int]),
    "sc_stage_bench": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_double_p]),
    # energy curve of a long recording (segment.hip)
    "sc_segment_frame_count": (C.c_long, [C.c_long]),
    "sc_segment_design": (C.c_int, [c_double_p, c_double_p]),
    "sc_segment_energy": (C.c_long, [vp, C.c_long, C.c_int, vp, C.c_long, vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGS.keys())

# revision of include/scasr.h these ctypes mirrors were written against (SC_ABI_VERSION): a library built from another
# revision would be handed mis-laid-out structs
ABI_VERSION = 12

_lib = None


class ScasrError(RuntimeError):
    pass


def build(verbose: bool = False) -> Path:
    """Compile every HIP source for gfx950 into speechcatcher_amd/libscasr.so."""
    cmd = ["make", "-C", str(CSRC), "-j4"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise ScasrError("building libscasr.so failed")
    return LIB_PATH


def load():
    """Load the library; raise if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7; import it FIRST so that libscasr
    # binds to the same HIP runtime instance (two runtimes in one process do
    # not see each other's device / streams).
    import torch  # noqa: F401
    lib_path = LIB_PATH
    # A/B runs of library VARIANTS (tools/ab_libs.sh, tools/build_variant.sh): honoured only with the test hooks on - a
    # production process always loads the in-tree product build (the variants used to be copied over it)
    if os.environ.get("SC_TEST_HOOKS") == "1" and os.environ.get("SC_LIB_VARIANT"):
        lib_path = Path(os.environ["SC_LIB_VARIANT"]).resolve()
    if not lib_path.exists():
        raise ScasrError(
            f"{lib_path} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback for the product path.")
    lib = C.CDLL(str(lib_path))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.sc_version()
    if got != ABI_VERSION:
        raise ScasrError(f"{lib_path} was built from ABI revision {got} of include/scasr.h, this binding is revision "
                         f"{ABI_VERSION}: rebuild the library (`python -c 'import __graft_entry__ as g; g.build()'`)")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().sc_last_error()
        raise ScasrError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
