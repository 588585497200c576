// Internal header of the stream-level C ABI: the state of an engine and of a stream handle, shared by the engine
// (streams.hip) and the read-back services (stream_readback.hip).  Not installed; include/scasr.h is the interface.
// The types live in the named namespace sc_state, not in an anonymous one: sc_streams has members of these types and is
// seen from two translation units, where anonymous-namespace members would make it two different types.  The namespace is
// hidden, so nothing of it is exported from libscasr.so.
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "common.h"
#include "handover.h"
#include "resample.h"

struct sc_streams;
#pragma GCC visibility push(hidden)
namespace sc_state {

#define HIP_TRY(call)                                                              \
  do {                                                                             \
    hipError_t e__ = (call);                                                       \
    if (e__ != hipSuccess) {                                                       \
      sc_set_error("%s: %s failed: %s", __func__, #call, hipGetErrorString(e__));  \
      return SC_ERR_LAUNCH;                                                        \
    }                                                                              \
  } while (0)
#define RC_TRY(call)                 \
  do {                               \
    int rc__ = (call);               \
    if (rc__ != SC_OK) return rc__;  \
  } while (0)

struct Tensor {
  void *ptr = nullptr;
  int64_t numel = 0;
  int dtype = 0;  // 0 f32, 1 f64, 2 f16
  bool owned = false;
};

struct StreamFault {
  int stream;
  int code;  // SC_ERR_CAPACITY / SC_ERR_INPUT
  std::string msg;
};

// host mirror of one stream's scalar state (engine.py: StreamState)
struct St {
  bool fe_started = false;
  long pcm_start = 0, pcm_end = 0;
  bool enc_started = false;
  int fpp = 0, nfeat = 0, upp = 0, nsub = 0;
  bool has_sub = false;
  int n_blocks = 0;
  bool has_addin = false, has_ctx = false;
  int short_pos = 0;
  int T_enc = 0, processed_block = 0, process_idx = 0;
  bool prev_valid = false, started = false;
  int cur = 0, L = 1, nhyp = 1;
  bool has_ctc = false;
  int T_ctc = 0, T_kv = 0, output_index = 0;
  // encoder frames whose CTC rows / cross-attention K|V rows have been projected (by the encoder stage that
  // emitted them); after a strict reset() T_proj restarts at the stale table's extent (scorers.py:342-350)
  int T_proj = 0, T_projkv = 0;
  long n_steps_total = 0;
  int T_hyp = 0;   // frames [0, T_hyp) of the decode block the live hypotheses come from (sc_align_hyps)
  // sample-rate conversion (resample.hip): coefficient table of the stream's input rate (-1: 16 kHz, no conversion), input
  // samples taken and 16 kHz samples produced in this utterance, history row the next launch reads (it writes the other)
  int rs_tab = -1, rs_par = 0;
  long rs_in = 0, rs_out = 0;
  // wire format of the stream's input (pcm.hip): SC_PCM_F32 with one channel is the float path - no decode launch
  int in_fmt = SC_PCM_F32, in_ch = 1, in_sel = 0, in_scale = SC_PCM_SCALE_FULL;
  bool coded() const { return in_fmt != SC_PCM_F32 || in_ch != 1; }
  // SC_DECODER_NONE (sc_stream_set_decoder): admission queues no decode block and lists no cross-attention K|V rows
  bool no_dec = false;
};

// a decode block of the schedule (beam_search.py:590-634): the T frames [0, T) it presents to the scorers, whether
// it is the final block, and the encoder group whose frames it sees (0: only frames that were there before)
// ... and the chunk (Job::seq of its stream) that queued it
struct Blk { int T; bool fin; long gen; long job; };

// the block a stream is inside (the loop state of _decode_one_block, beam_search.py:655-838)
struct Run {
  bool inblk = false, live = false, took = false, pvalid = false, has = false, hasp = false, fin = false;
  int cur = 0, L = 1, nhyp = 1, nhp = 1, pidx = 0, T = 0, Tc = 0, out = 0;
  long nsteps = 0;
  long job = 0;   // Job::seq of the chunk the block belongs to
};

// The side states (handover.h; DESIGN.md section 5, "Side states"): the payload each option hands over with a chunk, with
// its value before anything of the utterance has been scanned.  A Job carries a handover::Pending of each.
// Acoustic activity (sc_streams_set_activity; activity.hip): the state over every frame the encoder had emitted for the
// utterance when the chunk was admitted.  T: rows of the CTC table the state covers (the track's extent).
struct ActState {
  int32_t v[6] = {0, 0, 0, -1, -1, 0};
  int T = 0;
};
// Phrase spotting (sc_streams_set_phrases; spot.hip): the counters (n_frames, n_events).  The events themselves stay on the
// device: the utterance's event k is at slot k, so the first n_events of them are final whatever later groups append.
struct SpotState {
  int32_t v[2] = {0, 0};
};
// Draft transcript (sc_streams_set_draft; draft.hip): the greedy state.  The tokens stay on the device: the utterance's
// token k is at slot k and is never touched once stored, so the first n_closed of them are final whatever later groups
// append; the open token travels in the state.
struct DraftState {
  sc_draft_t d = {0, 0, 0, -1, -1, -1, 0.0};
};
// CTC prefix beam search (sc_streams_set_ctc_beam; ctc_beam.hip): the beam - counters and entries.  The prefix tree stays
// on the device: the utterance's node k is at slot k and is never touched once stored, so the chains of a reported state's
// entries are final whatever later groups append.
// With a language model attached (sc_streams_set_ctc_beam_lm) the model's side of the entries travels with them: all
// zero without one, and before the first group of an utterance (the readers put the model's start state there).
// A stream with a grammar (sc_stream_set_grammar) carries the automaton's states beside its entries in the same way.
struct BeamState {
  sc_beam_t d;
  sc_beam_lm_t lm{};
  sc_beam_gr_t gr{};
  BeamState() {
    d.n_frames = 0; d.n_bad = 0; d.n_nodes = 1; d.n_entries = 1;
    for (sc_beam_entry &e : d.e) e = sc_beam_entry{-1, -1, 0, -1, -INFINITY, -INFINITY};
    d.e[0] = sc_beam_entry{0, -1, 0, -1, 0.0, -INFINITY};
  }
  explicit BeamState(const sc_beam_t &v) : d(v) {}
  BeamState(const sc_beam_t &v, const sc_beam_lm_t &l) : d(v), lm(l) {}
  BeamState(const sc_beam_t &v, const sc_beam_gr_t &g) : d(v), gr(g) {}
};
// Input level (sc_stream_set_input_format; pcm.hip): the cumulative level, all zero at first.  Its launch belongs to a
// STAGING slot (it runs in the admission's staging step, not in an encoder group), so its key is a ticket that names the
// decode job, and slots are collected in any order.
using LevelState = sc_input_level_t;

// the options that scan the CTC rows of an encoder group, in launch order (EncGroup::Span::opt)
enum { OPT_ACT, OPT_SPOT, OPT_DRAFT, OPT_BEAM, N_OPT };

// a stream's outstanding chunk (sc_push / sc_submit): open until it has been reported.  With a queue depth > 1
// (sc_streams_set_queue_depth) further chunks of the stream wait behind it (sc_streams::ahead), in order.
struct Job {
  bool open = false;
  int has_out = 0;   // 1: the call produced output, 0: the reference's early `return []`
  int fault = 0;     // SC_ERR_*: the chunk failed, the stream is reset when it is reported
  long seq = 0;      // per-stream sequence number of the chunk (tags its decode blocks)
  bool fin = false;  // is_final chunk: nothing may be queued behind it
  bool dropped = false;   // failed only because an EARLIER chunk of the stream failed (the reset has happened by then)
  bool started = false;   // St::started right after THIS chunk's admission (a later admission may set it before this one is reported)
  handover::Pending<ActState> act;       // sc_streams_set_activity: the activity state that belongs to this chunk
  handover::Pending<SpotState> spot;     // sc_streams_set_phrases: the spotting counters that belong to this chunk
  handover::Pending<DraftState> draft;   // sc_streams_set_draft: the draft state that belongs to this chunk
  handover::Pending<BeamState> beam;     // sc_streams_set_ctc_beam: the beam that belongs to this chunk
  handover::Pending<LevelState> level;   // sc_stream_set_input_format: the input level up to and including this chunk
};

// hypotheses of a stream's last complete chunk, copied aside when later chunks of the stream may go on decoding
// (queue depth > 1): what sc_get_hyps_batch returns for the stream until the next sc_poll call
struct Snap {
  bool valid = false, reported = false;
  long seq = 0;
  int L = 1, nhyp = 0;
  int T = 0;   // St::T_hyp of the copied hypotheses
};

template <typename T>
int dalloc(T **p, size_t n) {
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  HIP_TRY(hipMalloc((void **)p, bytes));
  HIP_TRY(hipMemset(*p, 0, bytes));
  // (a fill of device memory may return before it has run, and the engine's streams are not ordered behind the null
  // stream: without the wait the zeros can land on what a first launch has already written there)
  HIP_TRY(hipStreamSynchronize(nullptr));
  return SC_OK;
}

// A grow-only scratch area: a device buffer and a pinned host buffer of the same size.  reserve() keeps what is there
// when it is large enough; otherwise it waits for `stream` (whatever still reads the old buffers runs there), frees and
// allocates geometrically: few reallocations (a hipFree may stall the device).  The contents do not survive a growth.
struct Scratch {
  char *dev = nullptr, *host = nullptr;
  size_t cap = 0;
  ~Scratch() { release(); }
  void release() {
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr;
    cap = 0;
  }
  int reserve(size_t need, hipStream_t stream) {
    if (need <= cap) return SC_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    const size_t want = std::max(need, 2 * cap);
    release();
    HIP_TRY(hipMalloc((void **)&dev, want));
    HIP_TRY(hipHostMalloc((void **)&host, want));
    cap = want;
    return SC_OK;
  }
};

// The hypotheses a stream reports (sc_get_hyps_batch and every read-back call that speaks of "the stream's hypotheses"):
// the snapshot taken at queue depth > 1 if there is one, otherwise the live rows at St::cur.  nh is NOT clamped to a
// caller's nbest (0: the stream has not started); row is the first hypothesis' row of the tables the pointers lie in;
// T: frames of the decode block the hypotheses come from (Snap::T, St::T_hyp).
struct HypSrc {
  bool snap = false;
  int nh = 0, L = 1, T = 0;
  const int32_t *yseq = nullptr, *xpos = nullptr;
  const double *score = nullptr, *score_dec = nullptr, *score_ctc = nullptr;
  int score_stride = 1;
  size_t row = 0;
};

// the names the read-back services (stream_readback.hip) and the engine (streams.hip) share beside the types
int wait_group(sc_streams *b, long gen);   // streams.hip: host-blocking wait for the encoder group `gen`
int beam_ready(sc_streams *b, int s);      // streams.hip: the beam state of the stream's last reported chunk is complete
int hyp_source(const sc_streams *b, int s, HypSrc *h);                  // stream_readback.hip; fails inside a decode block
int listed_once(const sc_streams *b, int s, std::vector<char> &listed); // stream_readback.hip; listed: [S], zero at first
}  // namespace sc_state
#pragma GCC visibility pop
using namespace sc_state;

struct sc_engine {
  sc_config cfg{};
  int device = 0;
  std::map<std::string, Tensor> t;
  std::vector<sc_enc_layer> enc;
  std::vector<sc_dec_layer> dec;
  std::vector<const float *> wkv, bkv;
  float *wkv_all = nullptr, *bkv_all = nullptr;   // the layers' K|V weights [Ld * 2d][d] and biases one behind the other (project_rows)

  const float *f(const std::string &name, bool required = true) const {
    auto it = t.find(name);
    if (it == t.end()) {
      if (required) sc_set_error("sc_engine: tensor '%s' is missing", name.c_str());
      return nullptr;
    }
    return (const float *)it->second.ptr;
  }
  ~sc_engine() {
    for (auto &kv : t)
      if (kv.second.owned && kv.second.ptr) (void)hipFree(kv.second.ptr);
    if (wkv_all) (void)hipFree(wkv_all);
    if (bkv_all) (void)hipFree(bkv_all);
  }
};

struct EncPlan {
  std::vector<int32_t> conv_jobs, a_rows, lin_dst, feat_src, feat_dst, blk_jobs, sjobs, emit_src, emit_dst, sub_src,
      sub_dst;
  struct Short { int s, ubase, U, pe_pos, dst_T; };
  std::vector<Short> shorts;
  int n_conv = 0, max_t1 = 0;
};

// One admission group: the frontend + encoder launches of the chunks admitted together, planned (host state already
// advanced) and issued on the encoder stream either at once (sc_submit) or when the decode loop has thinned out
// (sc_push).  `ev` completes when the group's encoder output, CTC rows and cross-attention K|V rows are in place.
struct EncGroup {
  long gen = 0;
  bool launched = false, features = false;
  bool open = false;                         // sc_submit: later admissions may still be merged into this (unlaunched) group
  bool deferred = false;                     // sc_submit: issued when it is full or when a decode block needs its frames
  int slot = 0;                              // job-table arena slot
  int stage_slot = -1;                       // pinned staging slot holding the admission's host input (-1: none)
  std::vector<long long> copy_jobs;          // [n][3] staging offset, destination offset, count (floats)
  std::vector<sc_rs_job> rs_jobs;            // chunks of the streams whose input rate is not 16000: converted, not copied
  size_t stage_floats = 0;
  // coded chunks (streams with an input format): their bytes go to the slot's byte region, ONE sc_pcm_decode launch writes
  // the float spans reserved for them before the scatter / conversion launch reads those; pcm_spans[i] belongs to pcm_jobs[i]
  struct PcmSpan { int s; bool fin; };
  std::vector<sc_pcm_job> pcm_jobs;
  std::vector<PcmSpan> pcm_spans;
  size_t stage_bytes = 0;
  bool stage_filled = false;                 // the host wrote floats into the slot (false: the float copy is skipped)
  std::vector<int32_t> fe_jobs;
  int n_fe = 0, max_keep = 0;
  EncPlan P;
  std::vector<int32_t> ctc_rows, kv_src, kv_dst;   // eager projections of the frames the group emits
  // side-state options (activity, spotting, draft, beam): per stream the span [t0, t1) of ctc_rows that every option which is on
  // scans, one job each and in this order in every option's launch; mask: the stream's enabled phrases (spotting);
  // opt[o]: the span as option o planned it (every span of a group carries the same options)
  struct Span {
    int s = 0, t0 = 0, t1 = 0;
    uint64_t mask = 0;
    const sc_grammar_view *grammar = nullptr;   // (beam) the device view of the stream's grammar when the span was planned
    handover::Plan opt[N_OPT];
  };
  std::vector<Span> spans;
  bool same_rows = true;
  std::vector<int> streams;                  // streams with work in this group (each at most once)
  bool empty() const { return !n_fe && !P.n_conv; }
};

constexpr int N_ARENA = 8;   // job-table arena slots = encoder groups that can be in flight
constexpr int N_STAGE = 4;   // pinned staging slots for host input (a slot is free again when its H2D copy is done)
constexpr int N_RING = 4;    // block-start tables (ctrl rows, log-softmax row lists): pinned ring

struct sc_streams {
  sc_engine *eng = nullptr;
  sc_config cfg{};
  int S = 0, W = 0, K = 0, TCAP = 0, LCAP = 0, FCAP = 0, UCAP = 0, max_feat_new = 0, max_t1 = 0, max_t2 = 0,
      max_blocks = 0, max_chunk = 0, max_length = 500;
  long PCAP = 0;
  bool use_bbd = false, strict = true;
  hipStream_t stream = nullptr;
  // Encoder side on its OWN HIP stream: frontend + encoder of a chunk do not feed the decode blocks whose frames
  // were already there before the chunk (the block schedule runs one hop behind the encoder), so both
  // are in flight together: the encoder's kernels run in the gaps of the decode chain (between a step's last kernel
  // and the next step's first - the host reads the stop flags there) and behind its thin iterations.  Kernel traces
  // (tools/rocpd_busy.py) show the kernels of the two streams ALTERNATING, not sharing CUs: 1.5 % of the wall time
  // has both running - every kernel of the path fills the registers or the LDS of the CUs it occupies.
  // `es` is the stream the current phase launches into.
  hipStream_t stream_enc = nullptr, es = nullptr;
  hipEvent_t ev_iter[2] = {nullptr, nullptr};   // end of decode iteration k (k & 1)
  int32_t *ring_dev = nullptr;                  // device view of flags_host [S]: the prune kernel stores the stop flags there
  int32_t *rm_host[2] = {nullptr, nullptr};     // pinned rowmap images (double-buffered: one may still be in a copy queue)
  int rm_idx = 0;
  bool rm_dirty = false;                        // rm_host[rm_idx] differs from the device rowmap
  // T-parallel CTC scan: frames to walk >= scan_split_min (tools: and bucket streams <= scan_split_streams, 0 = any).  1024
  // (round 5; 256 with a 48-stream bucket limit until round 4): WHICH form a stream's scan takes must depend on that
  // stream alone (bit-reproducible serving), and with every stream of a full bucket in it the T-parallel form costs more
  // than the sequential walk (3181 against 3258 audio-s/s at 390 frames to walk, profiles/r05_ab_scan_logits.txt) - it is
  // for the long tables of CLI segments (T = 4500: 61 against 588 us per step)
  int scan_split_min = 1024, scan_split_streams = 0;
  bool scan_long = false;                       // this step: a live stream has >= scan_split_min frames to walk
  // (round 5) the T-parallel kernel is part of a step whenever ONE live stream has a table long enough for it - whatever the
  // size of the bucket: which form a stream's scan takes must depend on that stream alone (bit-reproducible serving);
  // scan_split_streams (tools) restores the old bucket limit for A/B runs
  int step_split_min() const { return (scan_long && (scan_split_streams <= 0 || n_rows_step <= scan_split_streams * W)) ? scan_split_min : 0; }
  int graph_key() const { return n_rows_step * 2 + (step_split_min() > 0 ? 1 : 0); }
  int enc_start_thr = 0;         // sc_push: launch the planned encoder group when at most this many streams are still decoding
  int enc_batch_min = 0;         // sc_submit: launch the open encoder group when it holds this many streams (sc_streams_set_encoder_batch)
  int gemm_flags = 0;            // SC_GEMM_SPLIT16 when the engine carries split-precision copies of the PROJECTIONS (wqkv_s): the tiled
                                 // GEMMs of the encoder stage (conv2, subsampling Linear, CTC / cross-K|V projections) in the same form
                                 // (weights.py checks the range of their operands at load time)
  void *ws = nullptr, *ws_enc = nullptr;
  std::vector<void *> owned, owned_host;
  // device buffers
  float *pcm = nullptr, *featbuf = nullptr, *subbuf = nullptr, *prev_addin = nullptr, *past_ctx = nullptr, *enc = nullptr,
        *c1 = nullptr, *c2 = nullptr, *xblk = nullptr, *ws_xn = nullptr, *ws_qkv = nullptr, *ws_att = nullptr,
        *ws_ffh = nullptr;
  int32_t *jobs_ctx = nullptr, *ctrlmap = nullptr;
  float *kv_stage = nullptr;   // kv_half: fp32 staging [dec_layers][kv_stage_rows][2d] of the K|V projections
  int kv_stage_rows = 0;
  sc_search sb{};
  // pinned host
  int32_t *ctrlmap_host = nullptr, *flags_host = nullptr;
  // ---- job tables of the encoder groups: N_ARENA slots of one pinned / one device arena --------------------------
  int32_t *arena_host = nullptr, *arena_dev = nullptr;
  size_t slot_cap = 0, arena_off = 0;
  int cur_slot = 0;
  hipEvent_t ev_group[N_ARENA] = {nullptr};
  long slot_gen[N_ARENA] = {0};   // group that owns the slot (0: free)
  // ---- block-start tables (decode side) ------------------------------------------------------------------------------
  int32_t *bs_host = nullptr, *bs_dev = nullptr;   // [N_RING][S*8 + S*block_size]: ctrl rows, then log-softmax rows
  size_t bs_cap = 0;
  int bs_i = 0;
  // ---- host input staging (sc_push / sc_submit with host pointers): one H2D copy + one scatter launch per group ----
  float *stage_host = nullptr, *stage_dev = nullptr;
  size_t stage_cap = 0;           // floats per slot
  hipEvent_t ev_stage[N_STAGE] = {nullptr};
  bool stage_busy[N_STAGE] = {false};
  int stage_next = 0;
  long long *cjobs_host = nullptr, *cjobs_dev = nullptr;   // [N_STAGE][S*3] scatter jobs of a staging slot
  // ---- sample-rate conversion of the streams whose input rate is not 16000 (resample.hip; one launch per admission) ----
  sc_rs_job *rsjobs_host = nullptr, *rsjobs_dev = nullptr;   // [N_STAGE][S] jobs of a staging slot
  float *rs_hist = nullptr;       // [2][S][SC_RS_HIST] last K - 1 input samples of every stream, flipped per call
  sc_rs_tabs rs_tabs{};           // coefficient tables of the rates set on this handle (designed when a rate is first set)
  int rs_rate[SC_RS_MAX_TABS] = {0};
  int n_rs_tabs = 0;
  // ---- wire-format input (sc_stream_set_input_format; pcm.hip): everything below is allocated when a format is first set ----
  uint8_t *stageb_host = nullptr, *stageb_dev = nullptr;   // [N_STAGE][stageb_cap] byte region of a staging slot
  size_t stageb_cap = 0;          // bytes per slot = the float slot's bytes
  sc_pcm_job *pcmjobs_host = nullptr, *pcmjobs_dev = nullptr;             // [N_STAGE][S] decode jobs of a staging slot
  sc_input_level_t *lvl_state = nullptr;                                  // device [S]: the running level of every stream
  sc_input_level_t *lvl_out_host = nullptr, *lvl_out_dev = nullptr;       // [N_STAGE][S] host-mapped: the jobs' levels-after
  struct LvlSpan { int s; long epoch, ticket; };
  std::vector<LvlSpan> stage_lvl[N_STAGE];   // the decode jobs of the slot's latest admission, until their levels are collected
  handover::Track<LevelState> lvl;           // keyed by ticket: `pending` is the stream's latest job not collected yet
  long lvl_ticket = 0;
  // ---- batched hypothesis read-back (sc_get_hyps_batch): pack kernel -> one D2H into pinned memory -------------------
  int32_t *pack_dev = nullptr, *pack_host = nullptr, *pjobs_host = nullptr, *pjobs_dev = nullptr;
  size_t pack_cap = 0;            // int32 elements
  // ---- stable partials (sc_get_hyps_delta): job table and packed outputs, one job per stream; allocated on the first call ----
  sc_hyp_commit_job *cmjobs_host = nullptr, *cmjobs_dev = nullptr;   // [S]
  int32_t *cm_dev = nullptr, *cm_host = nullptr;
  size_t cm_cap = 0;              // int32 elements
  // ---- scratch area of the read-back services (stream_readback.hip): job tables, inputs, outputs, workspaces ---------------
  // ONE area serves sc_rescore_hyps / sc_lm_rescore_lists, sc_align_hyps / sc_alternates_hyps / sc_align_tokens,
  // sc_ctc_beam_hyps, sc_attention_rescore_beam / _lists and sc_mbr_hyps / _lists, each with a layout of its own from offset 0.  That is sound
  // because every one of them reserves what it needs, fills the pinned half, makes its round trip on stream_rb, ends in a
  // host synchronise (on failure too) and copies its results to the caller's arrays before it returns: nothing is kept in
  // the area between two calls, and the handle serves one call at a time.  Allocated by the first such call.
  // (pack_* and cm_* stay apart: sc_align_hyps calls sc_get_hyps_batch and then aligns, and their fixed capacity is what
  // "exceed the read-back buffer" refuses.)
  Scratch rb;
  // ---- acoustic activity (sc_streams_set_activity): everything below is allocated when the option is first switched on ----
  bool act_on = false;
  double act_thr = 0.8;
  int32_t *act_state = nullptr;   // device [S][6]: the running state of every stream (advanced group by group, encoder stream)
  double *act_track = nullptr;    // device [S][TCAP]: p_blank per CTC row
  sc_ctc_activity_job *act_jobs_host = nullptr, *act_jobs_dev = nullptr;   // [N_ARENA][S]: the job table of a group's launch
  int32_t *act_out_host = nullptr, *act_out_dev = nullptr;                 // [N_ARENA][S][6] host-mapped: the jobs' states-after
  handover::Track<ActState> act;  // keyed by encoder group: `known` is the state after the latest RETIRED group that scanned the stream
  // ---- phrase spotting (sc_streams_set_phrases): everything below is allocated when a phrase set is first given ----------
  bool spot_on = false;
  int spot_P = 0;
  int32_t *spot_labels = nullptr, *spot_lens = nullptr;   // device [64][32], [64]: the phrase set
  double *spot_floors = nullptr;                          // device [64]
  int32_t *spot_counters = nullptr;   // device [S][2]: n_frames, n_events of every stream (advanced group by group)
  double *spot_values = nullptr;      // device [S][64][64]
  int32_t *spot_starts = nullptr;     // device [S][64][64]
  sc_spot_event *spot_events = nullptr;   // device [S][SC_SPOT_MAX_EVENTS]
  sc_ctc_spot_job *spot_jobs_host = nullptr, *spot_jobs_dev = nullptr;   // [N_ARENA][S]: the job table of a group's launch
  int32_t *spot_out_host = nullptr, *spot_out_dev = nullptr;             // [N_ARENA][S][2] host-mapped: the jobs' counters-after
  handover::Track<SpotState> spot;             // keyed by encoder group, as act
  std::vector<uint64_t> spot_mask;             // per stream: enabled phrases
  // ---- draft transcript (sc_streams_set_draft): everything below is allocated when the option is first switched on --------
  bool draft_on = false;
  sc_draft_t *draft_state = nullptr;        // device [S]: the running state of every stream (advanced group by group)
  sc_draft_token *draft_tokens = nullptr;   // device [S][TCAP]: a frame opens at most one token, so the store cannot overflow
  sc_ctc_draft_job *draft_jobs_host = nullptr, *draft_jobs_dev = nullptr;   // [N_ARENA][S]: the job table of a group's launch
  sc_draft_t *draft_out_host = nullptr, *draft_out_dev = nullptr;           // [N_ARENA][S] host-mapped: the jobs' states-after
  handover::Track<DraftState> draft;              // keyed by encoder group, as act
  // ---- CTC prefix beam search (sc_streams_set_ctc_beam): everything below is allocated when the option is first switched on ----
  bool beam_on = false;
  int beam_B = 0, beam_C = 0;
  int beam_nodes_B = 0;                     // the B the node store was sized for
  sc_beam_t *beam_state = nullptr;          // device [S]: the running state of every stream (advanced group by group)
  sc_beam_node *beam_nodes = nullptr;       // device [S][1 + beam_nodes_B * TCAP]: a frame adds at most B nodes, so the store cannot overflow
  sc_ctc_beam_job *beam_jobs_host = nullptr, *beam_jobs_dev = nullptr;   // [N_ARENA][S]: the job table of a group's launch
  sc_beam_t *beam_out_host = nullptr, *beam_out_dev = nullptr;           // [N_ARENA][S] host-mapped: the jobs' states-after
  handover::Track<BeamState> beam;          // keyed by encoder group, as act
  // language model fused into the beam (sc_streams_set_ctc_beam_lm): allocated when a model is first attached
  const sc_lm *beam_lm = nullptr;           // the caller's model (NULL: none - the group launches sc_ctc_beam as before)
  const sc_lm_view *beam_lm_view = nullptr; // its device view
  sc_lm_view beam_lm_info{};                // ... and a host copy of it
  double beam_alpha = 0.0, beam_beta = 0.0;
  sc_beam_lm_t *beam_lm_state = nullptr;    // device [S], beside beam_state
  sc_ctc_beam_lm_job *beam_lm_jobs_host = nullptr, *beam_lm_jobs_dev = nullptr;   // [N_ARENA][S]
  sc_beam_lm_t *beam_lm_out_host = nullptr, *beam_lm_out_dev = nullptr;           // [N_ARENA][S] host-mapped, beside beam_out
  // grammars (sc_stream_set_grammar): a menu belongs to a stream.  Allocated when a grammar is first set on the handle.
  std::vector<sc_grammar *> beam_gr;         // [S] the stream's grammar (NULL: none); the handle holds one use of each
  int beam_gr_n = 0;                         // streams with a grammar
  sc_beam_gr_t *beam_gr_state = nullptr;    // device [S], beside beam_state
  sc_ctc_beam_gr_job *beam_gr_jobs_host = nullptr, *beam_gr_jobs_dev = nullptr;   // [N_ARENA][S]
  sc_beam_gr_t *beam_gr_out_host = nullptr, *beam_gr_out_dev = nullptr;           // [N_ARENA][S] host-mapped, beside beam_out
  // ---- attention rescoring (sc_attention_rescore_beam / _lists): everything below is allocated by the first call ----
  char *ar_ws = nullptr;                        // workspace of sc_dec_rescore: what a call needs, at most ar_ws_limit bytes
  size_t ar_ws_bytes = 0, ar_ws_limit = SC_ATT_WS_DEFAULT_BYTES;
  void *ar_splitk = nullptr;                    // split-K workspace of the read-back stream (the fused feed-forward's partial sums)
  // ---- consensus of n-best lists (sc_mbr_hyps / sc_mbr_lists): allocated by the first call ---------------------------
  char *mbr_ws = nullptr;                       // direction workspace of sc_mbr: what a call needs, at most mbr_ws_limit bytes
  size_t mbr_ws_bytes = 0, mbr_ws_limit = SC_MBR_WS_DEFAULT_BYTES;
  size_t beam_ncap() const { return 1 + (size_t)beam_nodes_B * TCAP; }
  // ---- tick engine -----------------------------------------------------------------------------------------------------
  std::vector<St> st;
  std::vector<Run> run;
  std::vector<std::deque<Blk>> bq;
  std::vector<Job> job;                    // the OLDEST outstanding chunk of a stream (reported next)
  std::vector<std::deque<Job>> ahead;      // chunks queued behind it (queue_depth > 1)
  std::vector<long> job_seq;               // sequence number of the stream's latest chunk
  int queue_depth = 1;                     // outstanding chunks a stream may have (sc_streams_set_queue_depth)
  std::vector<Snap> snap;
  std::vector<long> done_at;               // sc_poll: order in which the streams' oldest chunks became complete (0: not yet)
  long done_counter = 0;
  int32_t *snap_yseq = nullptr, *snap_xpos = nullptr;   // [S*W][LCAP]
  double *snap_score = nullptr;                         // [S*W][3]
  hipEvent_t ev_snap = nullptr;
  std::vector<std::string> fault_msg;
  std::vector<long> enc_gen;       // group of the stream's latest encoder stage
  std::deque<EncGroup *> groups;   // planned or in flight, oldest first
  long gen_next = 1, gen_done = 0, gen_ordered = 0;   // groups: issued, known complete, main stream ordered behind
  int n_open = 0;                  // outstanding chunks
  long iter = 0;
  bool inflight = false;           // a decode step has been enqueued and not collected yet (between two sc_poll calls)
  std::vector<int> tick_active;    // ... for these streams
  std::chrono::steady_clock::time_point tick_t0, tick_t1;
  hipStream_t stream_rb = nullptr; // hypothesis read-back (sc_get_hyps_batch) beside an enqueued decode step
  bool poisoned = false;           // a call failed half-way: device and host state may disagree
  std::vector<int> rowmap_key;
  int row_bucket = 1, n_rows_step = 0;
  bool decode_prepared = false;
  std::map<int, hipGraphExec_t> dec_graphs;
  std::map<std::vector<long>, hipGraphExec_t> enc_graphs;
  long dec_steps = 0, dec_blocks = 0, enc_calls = 0, xattn_rows[3] = {0, 0, 0};   // [0] flash kernels, [1] head-parallel layer kernels, [2] stream-resident layer kernel
  long sattn_pos[3] = {0, 0, 0};           // token positions the self-attention covered (sum of L over steps, streams, layers)
  unsigned long long *stat_rows = nullptr; // device [3]: distinct self-attention K|V rows read (sc_search.stat_rows)
  double t_launch = 0, t_wait = 0;               // seconds in the step loop: issuing, waiting for the flags
  double t_bucket[17] = {0};                     // ... by compaction bucket (n_rows_step / (row_bucket*W))
  long n_bucket[17] = {0};
  bool use_graphs = true;
  long n_enc_captures = 0;        // encoder-layer graphs captured (one per group shape) and the host time that took
  double t_enc_capture = 0;

  ~sc_streams() {
    for (auto &g : dec_graphs) (void)hipGraphExecDestroy(g.second);
    for (auto &g : enc_graphs) (void)hipGraphExecDestroy(g.second);
    if (stream) (void)sc_set_stream_workspace(stream, nullptr, 0);
    if (stream_enc) {
      (void)sc_set_stream_workspace(stream_enc, nullptr, 0);
      (void)hipStreamDestroy(stream_enc);
    }
    for (int i = 0; i < 2; ++i)
      if (ev_iter[i]) (void)hipEventDestroy(ev_iter[i]);
    for (int i = 0; i < N_ARENA; ++i)
      if (ev_group[i]) (void)hipEventDestroy(ev_group[i]);
    for (int i = 0; i < N_STAGE; ++i)
      if (ev_stage[i]) (void)hipEventDestroy(ev_stage[i]);
    if (ev_snap) (void)hipEventDestroy(ev_snap);
    for (EncGroup *g : groups) delete g;
    for (void *p : owned) (void)hipFree(p);
    for (void *p : owned_host) (void)hipHostFree(p);
    if (stream_rb && ar_splitk) (void)sc_set_stream_workspace(stream_rb, nullptr, 0);
    if (stream_rb) (void)hipStreamDestroy(stream_rb);
    if (stream) (void)hipStreamDestroy(stream);
    if (ar_ws) (void)hipFree(ar_ws);
    if (mbr_ws) (void)hipFree(mbr_ws);
    if (ar_splitk) (void)hipFree(ar_splitk);
    if (beam_nodes) (void)hipFree(beam_nodes);
    for (sc_grammar *g : beam_gr)   // (the streams are synchronised: nothing reads a grammar any more)
      if (g) (void)sc_grammar_use(g, -1);
  }

  template <typename T>
  int alloc(T **p, size_t n) {
    RC_TRY(dalloc(p, n));
    owned.push_back(*p);
    return SC_OK;
  }
  template <typename T>
  int halloc(T **p, size_t n) {   // pinned, device-visible
    HIP_TRY(hipHostMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    owned_host.push_back(*p);
    memset(*p, 0, std::max<size_t>(n, 1) * sizeof(T));
    return SC_OK;
  }
  template <typename T>
  int halloc_mapped(T **host, T **dev, size_t n, const char *who, const char *what) {   // ... and its device view
    RC_TRY(halloc(host, n));
    void *dv = nullptr;
    if (hipHostGetDevicePointer(&dv, *host, 0) != hipSuccess || !dv) {
      sc_set_error("%s: the pinned %s are not visible to the device", who, what);
      return SC_ERR_LAUNCH;
    }
    *dev = (T *)dv;
    return SC_OK;
  }
  int32_t *ctrl_host() { return ctrlmap_host; }              // [S][8]
  int32_t *rowmap_host() { return rm_host[rm_idx]; }          // [S*W]

  // host int table -> device (slot `cur_slot` of the pinned arena, async copy on the encoder-side stream; the launches
  // that read it are ordered behind the copy; a slot is recycled when its group's event has completed)
  int itensor(const std::vector<int32_t> &a, const int32_t **out) {
    const size_t n = a.size();
    if (arena_off + n > slot_cap) {
      sc_set_error("job-table arena exhausted (%zu + %zu of %zu entries)", arena_off, n, slot_cap);
      return SC_ERR_ARG;
    }
    const size_t off = (size_t)cur_slot * slot_cap + arena_off;
    arena_off += (n + 63) & ~size_t(63);
    if (n) {
      memcpy(arena_host + off, a.data(), n * sizeof(int32_t));
      HIP_TRY(hipMemcpyAsync(arena_dev + off, arena_host + off, n * sizeof(int32_t), hipMemcpyHostToDevice, es));
    }
    *out = arena_dev + off;
    return SC_OK;
  }
};

#define SC_API_BEGIN try {
#define SC_API_END                                                            \
  } catch (const std::bad_alloc &) {                                         \
    sc_set_error("%s: out of host memory", __func__);                        \
    return SC_ERR_ARG;                                                       \
  } catch (const std::exception &ex) {                                       \
    sc_set_error("%s: %s", __func__, ex.what());                             \
    return SC_ERR_ARG;                                                       \
  } catch (...) {                                                            \
    sc_set_error("%s: unexpected exception", __func__);                      \
    return SC_ERR_ARG;                                                       \
  }
