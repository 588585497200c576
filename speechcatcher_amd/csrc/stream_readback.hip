// Read-back services of the stream-level C ABI (include/scasr.h): the calls that report something about the hypotheses or
// the beam of idle streams - stable partials, n-gram rescoring, CTC alignment and alternates, the CTC beam's read-outs,
// attention rescoring.  They read the engine's state (streams.hip; the types are in streams_state.h) and change none of
// it.  Each one is the same five steps ("Read-back calls"): check the list (listed_once), find what
// each stream reports (hyp_source, or the reported beam state), lay a job table, inputs and outputs out in the handle's
// scratch area (Scratch, sc_streams::rb), make ONE round trip on the read-back stream (area_run) and copy the outputs to
// the caller's arrays.  sc_get_hyps_batch, the first of the kind, stays with the engine and its pack kernel.
#include "streams_state.h"

// ---- which hypotheses a stream reports, and which streams a call may list ------------------------------------------------
int sc_state::hyp_source(const sc_streams *b, int s, HypSrc *h) {
  const Snap &sn = b->snap[s];
  h->snap = sn.valid;
  if (sn.valid) {   // queue depth > 1: the copy taken when the stream's last reported chunk completed
    h->row = (size_t)s * b->W;
    h->nh = sn.nhyp; h->L = sn.L; h->T = sn.T;
    h->yseq = b->snap_yseq + h->row * b->LCAP;
    h->xpos = b->snap_xpos + h->row * b->LCAP;
    h->score = b->snap_score + h->row * 3;   // {total, dec, ctc} triples
    h->score_dec = h->score + 1;
    h->score_ctc = h->score + 2;
    h->score_stride = 3;
    return SC_OK;
  }
  SC_CHECK_ARG(!b->run[s].inblk && b->bq[s].empty(), "stream is inside a decode block (its chunk has not been reported yet)");
  const St &st = b->st[s];
  h->row = ((size_t)st.cur * b->S + s) * b->W;
  h->nh = st.started ? st.nhyp : 0; h->L = st.L; h->T = st.T_hyp;
  h->yseq = b->sb.yseq + h->row * b->LCAP;
  h->xpos = b->sb.xpos + h->row * b->LCAP;
  h->score = b->sb.score + h->row;
  h->score_dec = b->sb.sc_dec + h->row;
  h->score_ctc = b->sb.sc_ctc + h->row;
  h->score_stride = 1;
  return SC_OK;
}

// stream s of a call's list: in range, and not listed before (the job tables hold one entry per stream or hypothesis row)
int sc_state::listed_once(const sc_streams *b, int s, std::vector<char> &listed) {
  SC_CHECK_ARG(s >= 0 && s < b->S, "stream out of range");
  SC_CHECK_ARG(!listed[s], "a stream is listed twice");
  listed[s] = 1;
  return SC_OK;
}

namespace {

// The round trip of a read-back call: ONE upload, the launches, ONE copy back, all on the read-back stream - a decode step
// of OTHER streams may be in flight on the batch's stream (sc_poll); the listed streams' last steps have been collected
// (host-synchronised) by then.  wait_snap: something the launches read lies in a snapshot, and the copies are written on
// the batch's stream.  Synchronised when it returns, on failure too: nothing of this call may still read the pinned side
// when the next call fills it.
template <typename Launch>
int round_trip(sc_streams *b, void *up_dev, const void *up_host, size_t upload_bytes, bool wait_snap, Launch launch,
               void *out_host, const void *out_dev, size_t out_bytes) {
  const int rc = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(up_dev, up_host, upload_bytes, hipMemcpyHostToDevice, b->stream_rb));
    if (wait_snap) HIP_TRY(hipStreamWaitEvent(b->stream_rb, b->ev_snap, 0));
    RC_TRY(launch());
    HIP_TRY(hipMemcpyAsync(out_host, out_dev, out_bytes, hipMemcpyDeviceToHost, b->stream_rb));
    HIP_TRY(hipStreamSynchronize(b->stream_rb));
    return SC_OK;
  }();
  if (rc != SC_OK) (void)hipStreamSynchronize(b->stream_rb);
  return rc;
}

// ... on the scratch area: [0, upload_bytes) of its pinned half goes up, [out_off, out_off + out_bytes) comes back to it
template <typename Launch>
int area_run(sc_streams *b, size_t upload_bytes, bool wait_snap, Launch launch, size_t out_off, size_t out_bytes) {
  Scratch &a = b->rb;
  return round_trip(b, a.dev, a.host, upload_bytes, wait_snap, launch, a.host + out_off, a.dev + out_off, out_bytes);
}

// A job's fixed-slot output block - [slots] doubles per pointer of `d`, then [slots] int32 per pointer of `q` - to the
// caller's arrays at element `at` (row i of [n][nbest]), nh entries each; a NULL array is not wanted.
void slots_out(const char *out, size_t slots, size_t at, int nh, std::initializer_list<double *> d,
               std::initializer_list<int32_t *> q) {
  const double *sd = (const double *)out;
  const int32_t *sq = (const int32_t *)(sd + d.size() * slots);
  for (double *p : d) {
    if (p) memcpy(p + at, sd, nh * sizeof(double));
    sd += slots;
  }
  for (int32_t *p : q) {
    if (p) memcpy(p + at, sq, nh * sizeof(int32_t));
    sq += slots;
  }
}

constexpr int CM_FIXED = 4 + SC_COMMIT_MAX_HYPS + 6;   // sc_get_hyps_delta, int32 per job: header, agree, three float64 totals

}  // namespace

// ---- stable partials ----------------------------------------------------------------------------------
// The committed prefix of the listed streams' live beams and the tails of their best hypotheses behind from[i]: ONE
// job-table upload, ONE sc_hyp_commit launch, ONE copy back, all on the read-back stream as sc_get_hyps_batch does it.  A
// job's outputs lie packed at an even int32 offset of cm_dev: [header: 4][agree: SC_COMMIT_MAX_HYPS][totals: 3 doubles]
// [stability: t doubles][ids: t][positions: t] with t = L - from.  Reads the engine's state, changes none.
extern "C" int sc_get_hyps_delta(sc_streams *b, const int *stream_ids, int n, const int *from, const int *final,
                                 int max_tail, int32_t *L_out, int32_t *commit, int32_t *n_hyps, int32_t *ids,
                                 int32_t *xpos, double *stability, double *scores, int32_t *status) {
  SC_CHECK_ARG(b && stream_ids && from && n >= 0 && max_tail >= 0, "bad arguments");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  SC_CHECK_ARG(n <= b->S, "more streams listed than the batch has");
  if (!b->cmjobs_host) {   // the first call (the last of the four allocations marks them done): a handle that never asks holds none
    b->cm_cap = (size_t)b->S * (4 * (size_t)b->LCAP + CM_FIXED + 2);
    RC_TRY(b->alloc(&b->cm_dev, b->cm_cap));
    RC_TRY(b->alloc(&b->cmjobs_dev, (size_t)b->S));
    RC_TRY(b->halloc(&b->cm_host, b->cm_cap));
    RC_TRY(b->halloc(&b->cmjobs_host, (size_t)b->S));
  }
  std::vector<char> listed(b->S, 0);
  std::vector<int> job_of(n, -1);
  std::vector<size_t> offs;
  size_t off = 0;
  int m = 0;
  bool from_snapshot = false;
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    RC_TRY(listed_once(b, s, listed));
    HypSrc h;
    RC_TRY(hyp_source(b, s, &h));
    const int nh = h.nh, L = h.L;   // every live hypothesis, not the first nbest of them
    from_snapshot = from_snapshot || (h.snap && nh > 0);
    if (nh == 0) {
      SC_CHECK_ARG(from[i] == 0, "from is beyond the hypotheses");
      continue;
    }
    SC_CHECK_ARG(nh <= SC_COMMIT_MAX_HYPS, "more than SC_COMMIT_MAX_HYPS live hypotheses");
    SC_CHECK_ARG(from[i] >= 0 && from[i] <= L, "from is beyond the hypotheses");
    const int t = L - from[i];
    SC_CHECK_ARG(t <= max_tail, "max_tail is smaller than the tail");
    sc_hyp_commit_job &j = b->cmjobs_host[m];
    int32_t *o = b->cm_dev + off;
    j.yseq = h.yseq;
    j.xpos = h.xpos;
    j.score = h.score;
    j.score_dec = h.score_dec;
    j.score_ctc = h.score_ctc;
    j.score_stride = h.score_stride;
    j.header = o;
    j.agree = o + 4;
    j.totals = (double *)(o + 4 + SC_COMMIT_MAX_HYPS);
    j.stability = j.totals + 3;
    j.ids = o + CM_FIXED + 2 * (size_t)t;
    j.pos = j.ids + t;
    j.row_stride = b->LCAP;
    j.n_hyp = nh; j.L = L; j.from = from[i];
    j.flags = (final && final[i]) ? SC_COMMIT_FINAL : 0;
    job_of[i] = m++;
    offs.push_back(off);
    off += ((size_t)CM_FIXED + 4 * (size_t)t + 1) & ~(size_t)1;
  }
  SC_CHECK_ARG(off <= b->cm_cap, "tails exceed the read-back buffer");
  if (m > 0)   // (on its own fixed-size buffers, not on the scratch area: the capacity refusal above is behaviour)
    RC_TRY(round_trip(b, b->cmjobs_dev, b->cmjobs_host, (size_t)m * sizeof(sc_hyp_commit_job), from_snapshot,
                      [&]() { return sc_hyp_commit(b->cmjobs_dev, m, b->stream_rb); }, b->cm_host, b->cm_dev,
                      off * sizeof(int32_t)));
  for (int i = 0; i < n; ++i) {
    const int k = job_of[i];
    if (k < 0) {
      if (L_out) L_out[i] = 0;
      if (commit) commit[i] = 0;
      if (n_hyps) n_hyps[i] = 0;
      if (status) status[i] = 0;
      if (scores) scores[3 * i] = scores[3 * i + 1] = scores[3 * i + 2] = 0.0;
      continue;
    }
    const int32_t *src = b->cm_host + offs[k];
    const size_t t = (size_t)(b->cmjobs_host[k].L - from[i]);
    if (L_out) L_out[i] = src[0];
    if (commit) commit[i] = src[1];
    if (n_hyps) n_hyps[i] = src[2];
    if (status) status[i] = src[3];
    const double *d = (const double *)(src + 4 + SC_COMMIT_MAX_HYPS);
    if (scores) memcpy(scores + 3 * (size_t)i, d, 3 * sizeof(double));
    if (stability) memcpy(stability + (size_t)i * max_tail, d + 3, t * sizeof(double));
    if (ids) memcpy(ids + (size_t)i * max_tail, src + CM_FIXED + 2 * t, t * 4);
    if (xpos) memcpy(xpos + (size_t)i * max_tail, src + CM_FIXED + 3 * t, t * 4);
  }
  return SC_OK;
  SC_API_END
}

// ---- n-gram rescoring of n-best lists ---------------------------------------------------------------
// The scratch area holds [job table][inputs of caller-given lists][outputs]: what lies before the outputs goes up in ONE
// copy, ONE sc_lm_rescore launch, the outputs come back in ONE copy, all on the read-back stream.  A job's outputs:
// fused, lm, eos_lm [16] doubles, then end_state, order, status [16] int32.
namespace {
constexpr size_t RS_OUT = (size_t)SC_RESCORE_MAX_HYPS * (3 * sizeof(double) + 3 * sizeof(int32_t));

void rs_outputs(sc_lm_rescore_job &j, char *out) {
  j.fused = (double *)out;
  j.lm = j.fused + SC_RESCORE_MAX_HYPS;
  j.eos_lm = j.lm + SC_RESCORE_MAX_HYPS;
  j.end_state = (int32_t *)(j.eos_lm + SC_RESCORE_MAX_HYPS);
  j.order = j.end_state + SC_RESCORE_MAX_HYPS;
  j.status = j.order + SC_RESCORE_MAX_HYPS;
  j.tok_lm = nullptr;
  j.tok_stride = 0;
}

// the m jobs at the head of the area, with whatever else lies before o_out, go up; the outputs [o_out, o_out + m RS_OUT) come back
int rs_run(sc_streams *b, size_t o_out, int m, bool from_snapshot) {
  return area_run(b, o_out, from_snapshot,
                  [&]() { return sc_lm_rescore((const sc_lm_rescore_job *)b->rb.dev, m, b->stream_rb); }, o_out, (size_t)m * RS_OUT);
}

// the outputs of job k -> row i of the caller's [n][nbest] arrays (nh entries each), in the order rs_outputs laid them out
void rs_copy_out(const sc_streams *b, size_t o_out, int k, size_t i, int nbest, int nh, int32_t *order, double *fused,
                 double *lm_sum, double *eos_lm, int32_t *status, int32_t *end_state) {
  slots_out(b->rb.host + o_out + (size_t)k * RS_OUT, SC_RESCORE_MAX_HYPS, i * (size_t)nbest, nh, {fused, lm_sum, eos_lm},
            {end_state, order, status});
}

int rs_model(const sc_lm *lm, double alpha, double beta, int lm_eos, const sc_lm_view **view, sc_lm_view *info) {
  SC_CHECK_ARG(std::isfinite(alpha) && std::isfinite(beta), "alpha and beta must be finite");
  RC_TRY(sc_lm_device_view(lm, view, info));
  SC_CHECK_ARG(*view, "the model has no device view");
  SC_CHECK_ARG(lm_eos >= -1 && lm_eos < info->V, "lm_eos is outside the model's vocabulary");
  return SC_OK;
}
}  // namespace

// The hypotheses sc_get_hyps_batch would return (same rules: the snapshot with a queue depth > 1, an error for a stream
// inside a decode block or listed twice), rescored: labels without <sos> and without a trailing <eos>.  Reads the
// engine's state, changes none, keeps none of its own; synchronised before it returns.
extern "C" int sc_rescore_hyps(sc_streams *b, const int *stream_ids, int n, int nbest, const sc_lm *lm, double alpha,
                               double beta, int lm_eos, const int *final, int32_t *order, double *fused, double *lm_sum,
                               double *eos_lm, int32_t *status, int *n_hyps) {
  SC_CHECK_ARG(b && stream_ids && lm && n_hyps && n >= 0 && nbest >= 0 && nbest <= SC_RESCORE_MAX_HYPS, "bad arguments");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  SC_CHECK_ARG(n <= b->S, "more streams listed than the batch has");
  sc_lm_view info;
  const sc_lm_view *view = nullptr;
  RC_TRY(rs_model(lm, alpha, beta, lm_eos, &view, &info));
  SC_CHECK_ARG(info.V == b->cfg.vocab_size, "the model's vocabulary size is not the batch's");
  const size_t o_out = (size_t)std::max(n, 1) * sizeof(sc_lm_rescore_job);
  RC_TRY(b->rb.reserve(o_out + (size_t)std::max(n, 1) * RS_OUT, b->stream_rb));
  sc_lm_rescore_job *jobs = (sc_lm_rescore_job *)b->rb.host;
  std::vector<char> listed(b->S, 0);
  std::vector<int> job_of(n, -1);
  int m = 0;
  bool from_snapshot = false;
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    RC_TRY(listed_once(b, s, listed));
    HypSrc h;
    RC_TRY(hyp_source(b, s, &h));
    const int nh = std::min(nbest, h.nh);
    from_snapshot = from_snapshot || (h.snap && nh > 0);
    n_hyps[i] = nh;
    if (nh == 0) continue;
    sc_lm_rescore_job j{};
    j.yseq = h.yseq;
    j.score = h.score;
    j.score_stride = h.score_stride;
    j.model = view;
    j.lens = nullptr;
    rs_outputs(j, b->rb.dev + o_out + (size_t)m * RS_OUT);
    j.row_stride = b->LCAP;
    j.alpha = alpha; j.beta = beta;
    j.n_hyp = nh; j.L = h.L; j.skip = 1; j.strip = b->cfg.eos_id; j.state0 = -1;
    j.lm_eos = (final && final[i]) ? lm_eos : -1;
    j.V = info.V; j.flags = 0;
    jobs[m] = j;
    job_of[i] = m++;
  }
  if (m > 0) RC_TRY(rs_run(b, o_out, m, from_snapshot));
  for (int i = 0; i < n; ++i)
    if (job_of[i] >= 0)
      rs_copy_out(b, o_out, job_of[i], (size_t)i, nbest, n_hyps[i], order, fused, lm_sum, eos_lm, status, nullptr);
  return SC_OK;
  SC_API_END
}

// The same launch for caller-given lists: list i has list_sizes[i] <= nbest rows, row r its lens[i][r] LABELS
// ids[i][r][0 .. lens) (nothing skipped, nothing stripped) and its total scores[i][r]; state0[i] is the automaton's state
// before the first label (-1, or state0 == NULL: the model's start_state).  How a decoder-free stream's final gets its
// </s> term (the ids and totals of sc_ctc_beam_hyps), and how any list from elsewhere is rescored.
extern "C" int sc_lm_rescore_lists(sc_streams *b, const sc_lm *lm, const int32_t *ids, const int32_t *lens,
                                   const double *scores, const int *list_sizes, int n, int nbest, int max_len,
                                   const int32_t *state0, double alpha, double beta, int lm_eos, int32_t *order,
                                   double *fused, double *lm_sum, double *eos_lm, int32_t *status, int32_t *end_state) {
  SC_CHECK_ARG(b && lm && lens && scores && list_sizes && n >= 0 && n <= SC_RESCORE_MAX_JOBS && nbest >= 0 &&
               nbest <= SC_RESCORE_MAX_HYPS && max_len >= 0 && (ids || max_len == 0), "bad arguments");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  sc_lm_view info;
  const sc_lm_view *view = nullptr;
  RC_TRY(rs_model(lm, alpha, beta, lm_eos, &view, &info));
  const size_t rows = (size_t)n * nbest;
  const size_t o_sc = (size_t)std::max(n, 1) * sizeof(sc_lm_rescore_job), o_len = o_sc + rows * sizeof(double),
               o_ids = o_len + ((rows * sizeof(int32_t) + 7) & ~(size_t)7),
               o_out = o_ids + ((rows * max_len * sizeof(int32_t) + 7) & ~(size_t)7);
  for (int i = 0; i < n; ++i) {
    SC_CHECK_ARG(list_sizes[i] >= 0 && list_sizes[i] <= nbest, "a list size outside [0, nbest]");
    SC_CHECK_ARG(!state0 || (state0[i] >= -1 && state0[i] < info.n_states), "a state0 outside the model's states");
  }
  RC_TRY(b->rb.reserve(o_out + (size_t)std::max(n, 1) * RS_OUT, b->stream_rb));
  sc_lm_rescore_job *jobs = (sc_lm_rescore_job *)b->rb.host;
  memcpy(b->rb.host + o_sc, scores, rows * sizeof(double));
  memcpy(b->rb.host + o_len, lens, rows * sizeof(int32_t));
  if (rows * max_len) memcpy(b->rb.host + o_ids, ids, rows * max_len * sizeof(int32_t));
  std::vector<int> job_of(n, -1);
  int m = 0;
  for (int i = 0; i < n; ++i) {
    if (list_sizes[i] == 0) continue;
    sc_lm_rescore_job j{};
    j.model = view;
    j.yseq = (const int32_t *)(b->rb.dev + o_ids) + (size_t)i * nbest * max_len;
    j.score = (const double *)(b->rb.dev + o_sc) + (size_t)i * nbest;
    j.lens = (const int32_t *)(b->rb.dev + o_len) + (size_t)i * nbest;
    rs_outputs(j, b->rb.dev + o_out + (size_t)m * RS_OUT);
    j.row_stride = max_len; j.score_stride = 1;
    j.alpha = alpha; j.beta = beta;
    j.n_hyp = list_sizes[i]; j.L = max_len; j.skip = 0; j.strip = -1; j.state0 = state0 ? state0[i] : -1;
    j.lm_eos = lm_eos; j.V = info.V; j.flags = 0;
    jobs[m] = j;
    job_of[i] = m++;
  }
  if (m > 0) RC_TRY(rs_run(b, o_out, m, false));
  for (int i = 0; i < n; ++i)
    if (job_of[i] >= 0)
      rs_copy_out(b, o_out, job_of[i], (size_t)i, nbest, list_sizes[i], order, fused, lm_sum, eos_lm, status, end_state);
  return SC_OK;
  SC_API_END
}

// ---- consensus of n-best lists ------------------------------------------------------------------------
// The scratch area holds [job table][inputs of caller-given lists][outputs]: what lies before the outputs goes up in ONE
// copy, the launches of sc_mbr, the outputs come back in ONE copy, all on the read-back stream.  A job's outputs, for a
// call whose rows have at most `cap` labels: weight, risk [16], conf, alt_mass [cap], gap_mass [cap + 1] doubles, then
// order, status [16], header [4], dist [256], alt_tok [cap] int32.  The direction workspace is the handle's own
// allocation (mbr_ws): as large as a call needs, never beyond mbr_ws_limit; beyond it the jobs run in slabs of whole
// lists, one sc_mbr call each, in stream order on the one workspace.
namespace {
constexpr int MB_H = SC_MBR_MAX_HYPS;

struct MbrLayout {
  int cap;   // labels a row of the call has at most, clamped to SC_MBR_MAX_LEN
  size_t doubles() const { return 2 * MB_H + 3 * (size_t)cap + 1; }
  size_t ints() const { return 2 * MB_H + 4 + MB_H * MB_H + (size_t)cap; }
  size_t bytes() const { return (doubles() * sizeof(double) + ints() * sizeof(int32_t) + 7) & ~(size_t)7; }
};

void mb_outputs(sc_mbr_job &j, const MbrLayout &lay, char *out) {
  j.weight_out = (double *)out;
  j.risk = j.weight_out + MB_H;
  j.conf = j.risk + MB_H;
  j.alt_mass = j.conf + lay.cap;
  j.gap_mass = j.alt_mass + lay.cap;
  j.order = (int32_t *)(j.gap_mass + lay.cap + 1);
  j.status = j.order + MB_H;
  j.header = j.status + MB_H;
  j.dist = j.header + 4;
  j.alt_tok = j.dist + MB_H * MB_H;
  j.slots = nullptr;
  j.slot_stride = 0;
}

int mb_workspace(sc_streams *b, size_t need) {
  const size_t want = std::min((need + 255) & ~(size_t)255, b->mbr_ws_limit & ~(size_t)255);
  if (want <= b->mbr_ws_bytes) return SC_OK;
  HIP_TRY(hipStreamSynchronize(b->stream_rb));
  if (b->mbr_ws) (void)hipFree(b->mbr_ws);
  b->mbr_ws = nullptr;
  b->mbr_ws_bytes = 0;
  HIP_TRY(hipMalloc((void **)&b->mbr_ws, want));
  b->mbr_ws_bytes = want;
  return SC_OK;
}

// the m jobs at the head of the area (job k's rows have at most caps[k] labels), with whatever else lies before o_out, go
// up; the jobs run in slabs that fit the workspace; the outputs [o_out, o_out + m lay.bytes()) come back
int mb_run(sc_streams *b, size_t o_out, const MbrLayout &lay, const std::vector<int> &caps, bool from_snapshot) {
  const int m = (int)caps.size();
  std::vector<std::pair<int, int>> slabs;   // [first, count)
  size_t need = 0;
  for (int a = 0; a < m;) {
    int cnt = 1, cap = caps[a];
    while (a + cnt < m && sc_mbr_ws_bytes(cnt + 1, std::max(cap, caps[a + cnt])) <= (b->mbr_ws_limit & ~(size_t)255)) {
      cap = std::max(cap, caps[a + cnt]);
      ++cnt;
    }
    need = std::max(need, sc_mbr_ws_bytes(cnt, cap));
    slabs.emplace_back(a, cnt);
    a += cnt;
  }
  RC_TRY(mb_workspace(b, need));
  return area_run(b, o_out, from_snapshot, [&]() -> int {
    for (const auto &sl : slabs)
      RC_TRY(sc_mbr((const sc_mbr_job *)b->rb.dev + sl.first, sl.second, b->mbr_ws, b->mbr_ws_bytes, b->stream_rb));
    return SC_OK;
  }, o_out, (size_t)m * lay.bytes());
}

struct MbrOut {
  int32_t *order; double *risk, *weight; int32_t *status, *header, *dist; double *conf; int32_t *alt_tok; double *alt_mass, *gap_mass;
};

// the outputs of job k (nh rows) -> entry i of the caller's arrays; k < 0: the list was empty
void mb_copy_out(const sc_streams *b, size_t o_out, const MbrLayout &lay, int k, size_t i, int nbest, int max_len, int nh,
                 const MbrOut &o) {
  if (k < 0) {
    if (o.header) { int32_t *h = o.header + 4 * i; h[0] = -1; h[1] = h[2] = h[3] = 0; }
    return;
  }
  const char *src = b->rb.host + o_out + (size_t)k * lay.bytes();
  const double *d = (const double *)src;
  const int32_t *q = (const int32_t *)(d + lay.doubles());
  const int mp = std::max(0, std::min(q[2 * MB_H + 1], lay.cap));
  const bool has_pivot = q[2 * MB_H] >= 0;
  if (o.weight) memcpy(o.weight + i * nbest, d, nh * sizeof(double));
  if (o.risk) memcpy(o.risk + i * nbest, d + MB_H, nh * sizeof(double));
  if (o.conf) memcpy(o.conf + i * max_len, d + 2 * MB_H, mp * sizeof(double));
  if (o.alt_mass) memcpy(o.alt_mass + i * max_len, d + 2 * MB_H + lay.cap, mp * sizeof(double));
  if (o.gap_mass && has_pivot) memcpy(o.gap_mass + i * ((size_t)max_len + 1), d + 2 * MB_H + 2 * (size_t)lay.cap, (mp + 1) * sizeof(double));
  if (o.order) memcpy(o.order + i * nbest, q, nh * sizeof(int32_t));
  if (o.status) memcpy(o.status + i * nbest, q + MB_H, nh * sizeof(int32_t));
  if (o.header) memcpy(o.header + 4 * i, q + 2 * MB_H, 4 * sizeof(int32_t));
  if (o.dist) memcpy(o.dist + i * MB_H * MB_H, q + 2 * MB_H + 4, MB_H * MB_H * sizeof(int32_t));
  if (o.alt_tok) memcpy(o.alt_tok + i * max_len, q + 2 * MB_H + 4 + MB_H * MB_H, mp * sizeof(int32_t));
}
}  // namespace

extern "C" int sc_streams_set_mbr_ws(sc_streams *b, size_t max_bytes) {
  SC_CHECK_ARG(b && max_bytes >= SC_MBR_WS_MIN_BYTES, "a workspace limit of at least SC_MBR_WS_MIN_BYTES");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  b->mbr_ws_limit = max_bytes;
  if (b->mbr_ws_bytes > max_bytes) {   // the next call allocates within the new limit
    HIP_TRY(hipStreamSynchronize(b->stream_rb));
    (void)hipFree(b->mbr_ws);
    b->mbr_ws = nullptr;
    b->mbr_ws_bytes = 0;
  }
  return SC_OK;
  SC_API_END
}

extern "C" int sc_streams_mbr_ws(const sc_streams *b, size_t *limit, size_t *allocated) {
  SC_CHECK_ARG(b, "null");
  if (limit) *limit = b->mbr_ws_limit;
  if (allocated) *allocated = b->mbr_ws_bytes;
  return SC_OK;
}

extern "C" int sc_mbr_hyps(sc_streams *b, const int *stream_ids, int n, int nbest, double scale, int pivot_best, int max_len,
                           int32_t *order, double *risk, double *weight, int32_t *status, int32_t *header, int32_t *dist,
                           double *conf, int32_t *alt_tok, double *alt_mass, double *gap_mass, int *n_hyps) {
  SC_CHECK_ARG(b && stream_ids && n_hyps && n >= 0 && nbest >= 0 && nbest <= SC_MBR_MAX_HYPS && max_len >= 0, "bad arguments");
  SC_CHECK_ARG(std::isfinite(scale) && scale >= 0.0, "scale must be finite and not negative");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  SC_CHECK_ARG(n <= b->S, "more streams listed than the batch has");
  const MbrLayout lay{std::min(max_len, SC_MBR_MAX_LEN)};
  const size_t o_out = (size_t)std::max(n, 1) * sizeof(sc_mbr_job);
  RC_TRY(b->rb.reserve(o_out + (size_t)std::max(n, 1) * lay.bytes(), b->stream_rb));
  sc_mbr_job *jobs = (sc_mbr_job *)b->rb.host;
  std::vector<char> listed(b->S, 0);
  std::vector<int> job_of(n, -1), caps;
  bool from_snapshot = false;
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    RC_TRY(listed_once(b, s, listed));
    HypSrc h;
    RC_TRY(hyp_source(b, s, &h));
    const int nh = std::min(nbest, h.nh);
    from_snapshot = from_snapshot || (h.snap && nh > 0);
    n_hyps[i] = nh;
    if (nh == 0) continue;
    const int cap = std::min(std::max(0, h.L - 1), SC_MBR_MAX_LEN);
    SC_CHECK_ARG(cap <= max_len, "max_len is smaller than the hypotheses");
    sc_mbr_job j{};
    j.yseq = h.yseq;
    j.score = h.score;
    j.score_stride = h.score_stride;
    mb_outputs(j, lay, b->rb.dev + o_out + caps.size() * lay.bytes());
    j.row_stride = b->LCAP;
    j.scale = scale;
    j.n_hyp = nh; j.L = h.L; j.skip = 1; j.strip = b->cfg.eos_id; j.V = b->cfg.vocab_size;
    j.pivot = pivot_best ? 0 : -1;
    jobs[caps.size()] = j;
    job_of[i] = (int)caps.size();
    caps.push_back(cap);
  }
  if (!caps.empty()) RC_TRY(mb_run(b, o_out, lay, caps, from_snapshot));
  const MbrOut o{order, risk, weight, status, header, dist, conf, alt_tok, alt_mass, gap_mass};
  for (int i = 0; i < n; ++i) mb_copy_out(b, o_out, lay, job_of[i], (size_t)i, nbest, max_len, n_hyps[i], o);
  return SC_OK;
  SC_API_END
}

extern "C" int sc_mbr_lists(sc_streams *b, const int32_t *ids, const int32_t *lens, const double *values, int are_weights,
                            const int *list_sizes, const int32_t *pivot, int n, int nbest, int max_len, double scale,
                            int32_t *order, double *risk, double *weight, int32_t *status, int32_t *header, int32_t *dist,
                            double *conf, int32_t *alt_tok, double *alt_mass, double *gap_mass) {
  SC_CHECK_ARG(b && lens && values && list_sizes && n >= 0 && n <= SC_MBR_MAX_JOBS && nbest >= 0 && nbest <= SC_MBR_MAX_HYPS &&
               max_len >= 0 && (ids || max_len == 0), "bad arguments");
  SC_CHECK_ARG(std::isfinite(scale) && scale >= 0.0, "scale must be finite and not negative");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  for (int i = 0; i < n; ++i) {
    SC_CHECK_ARG(list_sizes[i] >= 0 && list_sizes[i] <= nbest, "a list size outside [0, nbest]");
    SC_CHECK_ARG(!pivot || (pivot[i] >= -1 && pivot[i] < std::max(list_sizes[i], 1)), "a pivot outside [-1, list size)");
  }
  const MbrLayout lay{std::min(max_len, SC_MBR_MAX_LEN)};
  const size_t rows = (size_t)n * nbest;
  const size_t o_val = (size_t)std::max(n, 1) * sizeof(sc_mbr_job), o_len = o_val + rows * sizeof(double),
               o_ids = o_len + ((rows * sizeof(int32_t) + 7) & ~(size_t)7),
               o_out = o_ids + ((rows * max_len * sizeof(int32_t) + 7) & ~(size_t)7);
  RC_TRY(b->rb.reserve(o_out + (size_t)std::max(n, 1) * lay.bytes(), b->stream_rb));
  sc_mbr_job *jobs = (sc_mbr_job *)b->rb.host;
  memcpy(b->rb.host + o_val, values, rows * sizeof(double));
  memcpy(b->rb.host + o_len, lens, rows * sizeof(int32_t));
  if (rows * max_len) memcpy(b->rb.host + o_ids, ids, rows * max_len * sizeof(int32_t));
  std::vector<int> job_of(n, -1), caps;
  for (int i = 0; i < n; ++i) {
    if (list_sizes[i] == 0) continue;
    sc_mbr_job j{};
    j.yseq = (const int32_t *)(b->rb.dev + o_ids) + (size_t)i * nbest * max_len;
    const double *v = (const double *)(b->rb.dev + o_val) + (size_t)i * nbest;
    if (are_weights) j.weight = v; else j.score = v;
    j.score_stride = 1;
    j.lens = (const int32_t *)(b->rb.dev + o_len) + (size_t)i * nbest;
    mb_outputs(j, lay, b->rb.dev + o_out + caps.size() * lay.bytes());
    j.row_stride = max_len;
    j.scale = scale;
    j.n_hyp = list_sizes[i]; j.L = max_len; j.skip = 0; j.strip = -1; j.V = b->cfg.vocab_size;
    j.pivot = pivot ? pivot[i] : -1;
    jobs[caps.size()] = j;
    job_of[i] = (int)caps.size();
    caps.push_back(lay.cap);
  }
  if (!caps.empty()) RC_TRY(mb_run(b, o_out, lay, caps, false));
  const MbrOut o{order, risk, weight, status, header, dist, conf, alt_tok, alt_mass, gap_mass};
  for (int i = 0; i < n; ++i) mb_copy_out(b, o_out, lay, job_of[i], (size_t)i, nbest, max_len, list_sizes[i], o);
  return SC_OK;
  SC_API_END
}

// ---- CTC forced alignment ------------------------------------------------------------------------------------------
// One sc_ctc_align launch pair on the read-back stream for a list of (stream, frames, labels) requests; outputs back to
// the host.  The scratch area holds [job table][labels][outputs: start, end | logp_mean | path_score, status][workspaces]
// (the workspaces are used on the device only).
struct AlignReq { int s, T; std::vector<int32_t> y; };
struct AlignOut {   // a request's outputs where the copy back left them in the area's pinned half: read before the next call
  size_t L;
  const int32_t *start, *end;
  const float *lp;
  float score;
  int32_t status;
  // alt_K > 0 (sc_alternates_hyps): [L][K] ids and logp, [L] own_rank and span status
  const int32_t *alt_ids, *own_rank, *span_status;
  const double *alt_logp;
};

static size_t al_round(size_t x) { return (x + 255) & ~(size_t)255; }

// alt_K > 0: ONE sc_ctc_alternates launch behind them reads start / end where the alignment left them on the device; its
// job table travels in the same upload (behind the labels), its outputs come back in the same copy (behind the
// alignment's: [alt_logp: doubles][alt_ids | own_rank | span status]).  The alignment's launches, areas and bits are the
// same with and without it.
static int run_align(sc_streams *b, const std::vector<AlignReq> &reqs, bool after_snap, std::vector<AlignOut> &out,
                     int alt_K = 0) {
  const int n = (int)reqs.size();
  out.assign(n, AlignOut());
  if (n == 0) return SC_OK;
  int max_T = 0, max_L = 0;
  size_t n_lab = 0;
  for (const AlignReq &r : reqs) {
    max_T = std::max(max_T, r.T);
    max_L = std::max(max_L, (int)r.y.size());
    n_lab += r.y.size();
  }
  SC_CHECK_ARG(max_L <= SC_ALIGN_MAX_L, "a label sequence is longer than SC_ALIGN_MAX_L");
  const size_t o_lab = al_round((size_t)n * sizeof(sc_ctc_align_job));
  const size_t K = (size_t)alt_K;
  const size_t o_alt = o_lab + al_round(n_lab * 4);   // the alternates' job table (empty without them)
  const size_t o_out = o_alt + (alt_K ? al_round((size_t)n * sizeof(sc_ctc_alt_job)) : 0);
  const size_t n_alw = 3 * n_lab + 2 * (size_t)n;   // start, end, logp_mean per label; path_score, status per job
  const size_t o_altout = (n_alw * 4 + 7) & ~(size_t)7;   // (bytes behind o_out; doubles first)
  const size_t n_outb = alt_K ? o_altout + n_lab * K * 8 + (n_lab * K + 2 * n_lab) * 4 : n_alw * 4;
  size_t o_ws = o_out + al_round(n_outb), total = o_ws;
  for (const AlignReq &r : reqs) total += al_round(sc_ctc_align_ws_bytes(r.T));
  RC_TRY(b->rb.reserve(total, b->stream_rb));
  char *D = b->rb.dev, *H = b->rb.host;
  memset(H, 0, o_out);   // (the gaps between the tables: what goes up does not depend on the call before)
  sc_ctc_align_job *J = (sc_ctc_align_job *)H;
  int32_t *lab = (int32_t *)(H + o_lab);
  int32_t *od = (int32_t *)(D + o_out);
  const int V = b->cfg.vocab_size;
  size_t li = 0, wo = o_ws;
  for (int k = 0; k < n; ++k) {
    const AlignReq &r = reqs[k];
    const int L = (int)r.y.size();
    if (L) memcpy(lab + li, r.y.data(), (size_t)L * 4);
    sc_ctc_align_job &j = J[k];
    j.emis = b->sb.ctcx + (size_t)r.s * b->TCAP * V;
    j.labels = (const int32_t *)(D + o_lab) + li;
    j.ws = D + wo;
    j.start = od + 3 * li;
    j.end = od + 3 * li + L;
    j.logp_mean = (float *)(od + 3 * li + 2 * L);
    j.path_score = (float *)(od + 3 * n_lab + 2 * k);
    j.status = od + 3 * n_lab + 2 * k + 1;
    j.stride = V;
    j.T = r.T; j.L = L; j.V = V; j.blank = b->cfg.blank_id;
    if (alt_K) {
      sc_ctc_alt_job &a = ((sc_ctc_alt_job *)(H + o_alt))[k];
      char *ao = D + o_out + o_altout;
      a.emis = j.emis;
      a.labels = j.labels;
      a.start = j.start;
      a.end = j.end;
      a.alt_logp = (double *)ao + li * K;
      int32_t *ai = (int32_t *)(ao + n_lab * K * 8);
      a.alt_ids = ai + li * K;
      a.own_rank = ai + n_lab * K + li;
      a.status = ai + n_lab * K + n_lab + li;
      a.stride = V;
      a.T = r.T; a.V = V; a.blank = b->cfg.blank_id; a.L = L;
    }
    li += L;
    wo += al_round(sc_ctc_align_ws_bytes(r.T));
  }
  RC_TRY(area_run(b, o_out, after_snap, [&]() -> int {
    RC_TRY(sc_ctc_align((const sc_ctc_align_job *)D, n, max_T, max_L, b->stream_rb));
    if (alt_K) RC_TRY(sc_ctc_alternates((const sc_ctc_alt_job *)(D + o_alt), n, max_L, alt_K, b->stream_rb));
    return SC_OK;
  }, o_out, n_outb));
  const int32_t *res = (const int32_t *)(H + o_out);
  const char *ro = (const char *)res + o_altout;
  const int32_t *ri = (const int32_t *)(ro + n_lab * K * 8);
  li = 0;
  for (int k = 0; k < n; ++k) {
    AlignOut &o = out[k];
    const size_t L = o.L = reqs[k].y.size();
    o.start = res + 3 * li;
    o.end = o.start + L;
    o.lp = (const float *)(o.end + L);
    memcpy(&o.score, res + 3 * n_lab + 2 * k, 4);
    o.status = res[3 * n_lab + 2 * k + 1];
    o.alt_logp = (const double *)ro + li * K;
    o.alt_ids = ri + li * K;
    o.own_rank = ri + n_lab * K + li;
    o.span_status = ri + n_lab * K + n_lab + li;
    li += L;
  }
  return SC_OK;
}

// sc_align_hyps (K == 0) and sc_alternates_hyps (K > 0): the same requests, the same alignment
static int align_hyps(sc_streams *b, const int *stream_ids, int n, int nbest, int max_len, int K, int32_t *start,
                      int32_t *end, float *logp_mean, double *path_score, int *status, int32_t *alt_ids, double *alt_logp,
                      int32_t *own_rank, int32_t *span_status, int *n_hyps) {
  SC_CHECK_ARG(b && stream_ids && n_hyps && n >= 0 && nbest >= 0 && max_len >= 0, "bad arguments");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  if (n == 0 || nbest == 0) {
    for (int i = 0; i < n; ++i) n_hyps[i] = 0;
    return SC_OK;
  }
  const int LC = b->LCAP;
  std::vector<int32_t> ids((size_t)n * nbest * LC);
  std::vector<int> lens((size_t)n * nbest);
  RC_TRY(sc_get_hyps_batch(b, stream_ids, n, nbest, LC, ids.data(), nullptr, lens.data(), n_hyps, nullptr, nullptr, nullptr));
  std::vector<AlignReq> reqs;
  bool any_snap = false;
  for (int i = 0; i < n; ++i) {
    HypSrc src;   // (the frames of the hypotheses sc_get_hyps_batch has just reported)
    RC_TRY(hyp_source(b, stream_ids[i], &src));
    const int T = src.T;
    any_snap |= src.snap && n_hyps[i] > 0;
    for (int h = 0; h < n_hyps[i]; ++h) {
      const size_t o = (size_t)i * nbest + h;
      const int32_t *y = ids.data() + o * LC;
      int a = 1, e = lens[o];                                  // without <sos> ...
      if (e > a && y[e - 1] == b->cfg.eos_id) --e;             // ... and without a trailing <eos>
      AlignReq r{stream_ids[i], T, std::vector<int32_t>(y + a, y + std::max(a, e))};
      SC_CHECK_ARG((int)r.y.size() <= max_len || (!start && !end && !logp_mean && !alt_ids && !alt_logp && !own_rank && !span_status),
                   "max_len is smaller than the hypotheses");
      reqs.push_back(std::move(r));
    }
  }
  std::vector<AlignOut> out;
  RC_TRY(run_align(b, reqs, any_snap, out, K));
  int k = 0;
  for (int i = 0; i < n; ++i)
    for (int h = 0; h < n_hyps[i]; ++h, ++k) {
      const size_t o = (size_t)i * nbest + h;
      const AlignOut &a = out[k];
      const size_t L = a.L;
      if (start) memcpy(start + o * max_len, a.start, L * 4);
      if (end) memcpy(end + o * max_len, a.end, L * 4);
      if (logp_mean) memcpy(logp_mean + o * max_len, a.lp, L * 4);
      if (path_score) path_score[o] = a.score;
      if (status) status[o] = a.status;
      if (K) {
        if (alt_ids) memcpy(alt_ids + o * max_len * K, a.alt_ids, L * K * 4);
        if (alt_logp) memcpy(alt_logp + o * max_len * K, a.alt_logp, L * K * 8);
        if (own_rank) memcpy(own_rank + o * max_len, a.own_rank, L * 4);
        if (span_status) memcpy(span_status + o * max_len, a.span_status, L * 4);
      }
    }
  return SC_OK;
  SC_API_END
}

extern "C" int sc_align_hyps(sc_streams *b, const int *stream_ids, int n, int nbest, int max_len, int32_t *start,
                             int32_t *end, float *logp_mean, double *path_score, int *status, int *n_hyps) {
  return align_hyps(b, stream_ids, n, nbest, max_len, 0, start, end, logp_mean, path_score, status, nullptr, nullptr,
                    nullptr, nullptr, n_hyps);
}

extern "C" int sc_alternates_hyps(sc_streams *b, const int *stream_ids, int n, int nbest, int max_len, int K,
                                  int32_t *start, int32_t *end, float *logp_mean, double *path_score, int *status,
                                  int32_t *alt_ids, double *alt_logp, int32_t *own_rank, int32_t *span_status, int *n_hyps) {
  SC_CHECK_ARG(K >= 1 && K <= SC_ALT_MAX_K, "K outside [1, SC_ALT_MAX_K]");
  return align_hyps(b, stream_ids, n, nbest, max_len, K, start, end, logp_mean, path_score, status, alt_ids, alt_logp,
                    own_rank, span_status, n_hyps);
}

extern "C" int sc_align_tokens(sc_streams *b, int stream, const int32_t *ids, int L, int32_t *start, int32_t *end,
                               float *logp_mean, double *path_score, int *status) {
  SC_CHECK_ARG(b && stream >= 0 && stream < b->S && L >= 0 && (L == 0 || ids), "bad arguments");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  HypSrc src;   // the frames of the hypotheses sc_get_hyps_batch reports for the stream
  RC_TRY(hyp_source(b, stream, &src));
  std::vector<AlignReq> reqs{AlignReq{stream, src.T, std::vector<int32_t>(ids, ids + L)}};
  std::vector<AlignOut> out;
  RC_TRY(run_align(b, reqs, src.snap && src.nh > 0, out));
  const AlignOut &a = out[0];
  if (start) memcpy(start, a.start, (size_t)L * 4);
  if (end) memcpy(end, a.end, (size_t)L * 4);
  if (logp_mean) memcpy(logp_mean, a.lp, (size_t)L * 4);
  if (path_score) *path_score = a.score;
  if (status) *status = a.status;
  return SC_OK;
  SC_API_END
}

// ---- read-outs of the CTC prefix beam ------------------------------------------------------------------------
namespace {

// First-pass total of entry r of a reported beam state: lae(pb, pnb), with a language model attached
// + (alpha * lm + beta * len) - in this association (the build does not contract): sc_ctc_beam_hyps_lm reports it as
// `fused`, sc_attention_rescore_beam takes it as the entry's first-pass score, and the two are the same bits.
double beam_entry_total(const sc_streams *b, const BeamState &v, int r) {
  const sc_beam_entry &e = v.d.e[r];
  const double hi = std::max(e.pb, e.pnb), lo = std::min(e.pb, e.pnb);
  const double total = lo == -INFINITY ? hi : hi + log1p(exp(lo - hi));
  if (!b->beam_lm) return total;
  const double wa = b->beam_alpha * v.lm.lm[r], wb = b->beam_beta * (double)e.len;
  return total + (wa + wb);
}

// The sc_ctc_beam_pack jobs of the first nbest entries of the listed streams' reported beams, into the scratch area: the
// states [n] at offset 0 and the jobs [n][nbest] at o_jobs of its pinned half (both go up); a job's ids / frames
// [max_len], header [4] and scores [2] at slot k = i * nbest + r of the device regions at the given offsets.
void fill_beam_pack_jobs(sc_streams *b, const int *stream_ids, int n, int nbest, int max_len, size_t o_jobs, size_t o_ids,
                         size_t o_frames, size_t o_head, size_t o_sc) {
  sc_beam_t *st_host = (sc_beam_t *)b->rb.host;
  sc_ctc_beam_pack_job *jobs = (sc_ctc_beam_pack_job *)(b->rb.host + o_jobs);
  char *D = b->rb.dev;
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    st_host[i] = b->beam.rep[s].v.d;
    for (int r = 0; r < nbest; ++r) {
      const size_t k = (size_t)i * nbest + r;
      sc_ctc_beam_pack_job &j = jobs[k];
      j.state = (const sc_beam_t *)D + i;
      j.nodes = b->beam_nodes + (size_t)s * b->beam_ncap();
      j.ids = (int32_t *)(D + o_ids) + k * max_len;
      j.frames = (int32_t *)(D + o_frames) + k * max_len;
      j.header = (int32_t *)(D + o_head) + k * 4;
      j.scores = (double *)(D + o_sc) + k * 2;
      j.capacity = (int32_t)b->beam_ncap(); j.rank = r; j.max_len = max_len; j.reserved = 0;
    }
  }
}

}  // namespace

// beside sc_ctc_beam_hyps' scores: lm [n][nbest] and fused [n][nbest] = lae(pb, pnb) + (alpha * lm + beta * len) of the
// same entries (NaN where the state has no such entry); host arithmetic on the reported states, no launch.  Either may
// be NULL.
extern "C" int sc_ctc_beam_hyps_lm(sc_streams *b, const int *stream_ids, int n, int nbest, double *lm, double *fused) {
  SC_CHECK_ARG(b && stream_ids && n >= 0 && nbest >= 0 && nbest <= SC_BEAM_MAX, "bad arguments");
  SC_API_BEGIN
  SC_CHECK_ARG(b->beam_on && b->beam_lm, "no language model is attached (sc_streams_set_ctc_beam_lm)");
  SC_CHECK_ARG(n <= b->S, "more streams listed than the batch has");
  HIP_TRY(hipSetDevice(b->eng->device));
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    SC_CHECK_ARG(s >= 0 && s < b->S, "stream out of range");
    RC_TRY(beam_ready(b, s));
    const BeamState &v = b->beam.rep[s].v;
    for (int r = 0; r < nbest; ++r) {
      const size_t k = (size_t)i * nbest + r;
      double l = NAN, f = NAN;
      if (r < v.d.n_entries) {
        l = v.lm.lm[r];
        f = beam_entry_total(b, v, r);
      }
      if (lm) lm[k] = l;
      if (fused) fused[k] = f;
    }
  }
  return SC_OK;
  SC_API_END
}

// beside sc_ctc_beam_hyps: g [n][nbest], the grammar's state after each entry's prefix, and accept [n][nbest], its accept
// flag; -1 where the state has no such entry or the stream has no grammar.  Host arithmetic on the reported states and the
// grammars' host copies, no launch.  Either may be NULL.
extern "C" int sc_ctc_beam_hyps_grammar(sc_streams *b, const int *stream_ids, int n, int nbest, int32_t *g, int32_t *accept) {
  SC_CHECK_ARG(b && stream_ids && n >= 0 && nbest >= 0 && nbest <= SC_BEAM_MAX, "bad arguments");
  SC_API_BEGIN
  SC_CHECK_ARG(b->beam_on, "the beam option is off (sc_streams_set_ctc_beam)");
  SC_CHECK_ARG(n <= b->S, "more streams listed than the batch has");
  HIP_TRY(hipSetDevice(b->eng->device));
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    SC_CHECK_ARG(s >= 0 && s < b->S, "stream out of range");
    RC_TRY(beam_ready(b, s));
    const BeamState &v = b->beam.rep[s].v;
    const sc_grammar *gr = b->beam_gr_n ? b->beam_gr[s] : nullptr;
    sc_grammar_view info{};
    if (gr) RC_TRY(sc_grammar_device_view(gr, nullptr, &info));
    for (int r = 0; r < nbest; ++r) {
      const size_t k = (size_t)i * nbest + r;
      int32_t st = -1;
      if (gr && r < v.d.n_entries) st = v.d.n_frames == 0 ? info.start_state : v.gr.g[r];
      if (g) g[k] = st;
      if (accept) accept[k] = st < 0 ? -1 : sc_grammar_accepts(gr, st);
    }
  }
  return SC_OK;
  SC_API_END
}

// The first nbest entries of the listed streams' reported beams as token sequences: the states and ONE job table go up,
// ONE sc_ctc_beam_pack launch walks the chains, ONE copy comes back, all on the read-back stream as sc_get_hyps_batch
// does it.  header [n][nbest][4] (len, SC_BEAM_PACK_* status, node, last), ids / frames [n][nbest][max_len], scores
// [n][nbest][2] (pb, pnb); any of ids / frames / scores may be NULL.
extern "C" int sc_ctc_beam_hyps(sc_streams *b, const int *stream_ids, int n, int nbest, int max_len, int32_t *header,
                                int32_t *ids, int32_t *frames, double *scores) {
  SC_CHECK_ARG(b && stream_ids && header && n >= 0 && nbest >= 0 && nbest <= SC_BEAM_MAX && max_len >= 0, "bad arguments");
  SC_API_BEGIN
  SC_CHECK_ARG(b->beam_on, "the beam option is off (sc_streams_set_ctc_beam)");
  SC_CHECK_ARG(n <= b->S, "more streams listed than the batch has");
  HIP_TRY(hipSetDevice(b->eng->device));
  const size_t m = (size_t)n * nbest;
  if (m == 0) return SC_OK;
  SC_CHECK_ARG(m <= SC_BEAM_MAX_JOBS, "more than SC_BEAM_MAX_JOBS entries asked for");
  std::vector<char> listed(b->S, 0);
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    RC_TRY(listed_once(b, s, listed));
    RC_TRY(beam_ready(b, s));
  }
  // [states: n][jobs: m] go up; [scores: m][2] doubles, [header: m][4], [ids: m][max_len], [frames: m][max_len] come back
  const size_t o_jobs = (size_t)n * sizeof(sc_beam_t), o_sc = o_jobs + m * sizeof(sc_ctc_beam_pack_job),
               o_head = o_sc + m * 2 * sizeof(double), o_ids = o_head + m * 4 * sizeof(int32_t),
               o_frames = o_ids + m * max_len * sizeof(int32_t), need = o_frames + m * max_len * sizeof(int32_t);
  RC_TRY(b->rb.reserve(need, b->stream_rb));
  fill_beam_pack_jobs(b, stream_ids, n, nbest, max_len, o_jobs, o_ids, o_frames, o_head, o_sc);
  // (the groups that stored the nodes of these states have been retired; later groups write behind them)
  RC_TRY(area_run(b, o_sc, false, [&]() {
    return sc_ctc_beam_pack((const sc_ctc_beam_pack_job *)(b->rb.dev + o_jobs), (int)m, b->stream_rb);
  }, o_sc, need - o_sc));
  const char *H = b->rb.host;
  memcpy(header, H + o_head, m * 4 * sizeof(int32_t));
  if (scores) memcpy(scores, H + o_sc, m * 2 * sizeof(double));
  // (only [0, min(len, max_len)) of a row is written by the launch: the rest of the caller's rows is left as it is)
  for (size_t k = 0; k < m; ++k) {
    const int32_t *h = (const int32_t *)(H + o_head) + k * 4;
    const size_t L = (size_t)std::max(0, std::min(h[0], max_len));
    if (ids) memcpy(ids + k * max_len, (const int32_t *)(H + o_ids) + k * max_len, L * sizeof(int32_t));
    if (frames) memcpy(frames + k * max_len, (const int32_t *)(H + o_frames) + k * max_len, L * sizeof(int32_t));
  }
  return SC_OK;
  SC_API_END
}

// ---- attention rescoring of n-best lists at finals (dec_rescore.hip) ------------------------------------
// The lists' rows are scored by ONE sc_dec_rescore call against the listed streams' encoder rows enc[s][0 .. T_enc), on
// the read-back stream, with ONE copy back; nothing of the engine is written.  The scratch area holds [inputs][outputs]; a
// job's outputs: att, fused [16] doubles, then order, status [16] int32.  The workspace is allocated by the first call, as
// large as the call needs and never beyond ar_ws_limit (sc_streams_set_attention_rescore_ws): a call that needs more
// runs in slabs of whole streams, with the same bits.
namespace {
constexpr size_t AR_OUT = (size_t)SC_ATT_MAX_HYPS * (2 * sizeof(double) + 2 * sizeof(int32_t));
constexpr size_t AR_SPLITK = (size_t)32 << 20;

size_t ar_up(size_t x) { return (x + 255) & ~(size_t)255; }

int ar_workspace(sc_streams *b, size_t need) {
  if (!b->ar_splitk) {   // the read-back stream gets split-K storage of its own: the dense launchers never share partial sums
    HIP_TRY(hipMalloc(&b->ar_splitk, AR_SPLITK));
    RC_TRY(sc_set_stream_workspace(b->stream_rb, b->ar_splitk, AR_SPLITK));
  }
  const size_t want = std::min(ar_up(need), b->ar_ws_limit & ~(size_t)255);
  if (want <= b->ar_ws_bytes) return SC_OK;
  HIP_TRY(hipStreamSynchronize(b->stream_rb));
  if (b->ar_ws) (void)hipFree(b->ar_ws);
  b->ar_ws = nullptr;
  b->ar_ws_bytes = 0;
  HIP_TRY(hipMalloc((void **)&b->ar_ws, want));
  b->ar_ws_bytes = want;
  return SC_OK;
}

// the layers' cross-attention K|V weights one behind the other, as sc_dec_rescore takes them
int ar_weights(const sc_streams *b, const float **wkv, const float **bkv) {
  const sc_engine *e = b->eng;
  if (e->wkv_all && e->bkv_all) { *wkv = e->wkv_all; *bkv = e->bkv_all; return SC_OK; }
  if (b->cfg.dec_layers == 1) { *wkv = e->wkv[0]; *bkv = e->bkv[0]; return SC_OK; }
  sc_set_error("attention rescoring: the engine holds no contiguous copy of the cross-attention K|V weights");
  return SC_ERR_UNSUPPORTED;
}

// a listed stream: idle (its chunks reported), its encoder rows complete
int ar_stream(sc_streams *b, int s) {
  SC_CHECK_ARG(s >= 0 && s < b->S, "stream out of range");
  SC_CHECK_ARG(!b->job[s].open && b->ahead[s].empty(), "the stream has a chunk outstanding (sc_poll reports it first)");
  return wait_group(b, b->enc_gen[s]);
}

void ar_job(const sc_streams *b, sc_dec_rescore_job &j, int s, const float *wkv, const float *bkv, double w_att, double w_ctc,
            double beta, char *out) {
  j.E = b->enc + (size_t)s * b->TCAP * b->cfg.d_model;
  j.e_stride = b->cfg.d_model;
  j.T = b->st[s].T_enc;
  j.wkv = wkv; j.bkv = bkv;
  j.att = (double *)out;
  j.fused = j.att + SC_ATT_MAX_HYPS;
  j.order = (int32_t *)(j.fused + SC_ATT_MAX_HYPS);
  j.status = j.order + SC_ATT_MAX_HYPS;
  j.tok_att = nullptr; j.tok_stride = 0;
  j.score_stride = 1;
  j.w_att = w_att; j.w_ctc = w_ctc; j.beta = beta;
  j.pe_rows = b->cfg.pe_max_len;
}

// what lies before `up` of the area goes up, `before` is launched, the jobs run, their outputs come back
template <typename Before>
int ar_run(sc_streams *b, const std::vector<sc_dec_rescore_job> &jobs, size_t up, size_t o_out, Before before) {
  long rows = 0, enc_rows = 0;
  int seqs = 0;
  for (const sc_dec_rescore_job &j : jobs) { rows += (long)j.n_hyp * (j.L + 1); enc_rows += j.T; seqs += j.n_hyp; }
  RC_TRY(ar_workspace(b, sc_dec_rescore_ws_bytes(&b->sb, rows, enc_rows, seqs, (int)jobs.size())));
  return area_run(b, up, false, [&]() -> int {
    RC_TRY(before());
    return sc_dec_rescore(jobs.data(), (int)jobs.size(), &b->sb, b->ar_ws, b->ar_ws_bytes, b->stream_rb);
  }, o_out, jobs.size() * AR_OUT);
}

// the outputs of job k -> row i of the caller's [n][nbest] arrays (nh entries each), in the order ar_job laid them out
void ar_copy_out(const sc_streams *b, size_t o_out, int k, size_t i, int nbest, int nh, int32_t *order, double *fused,
                 double *att, int32_t *status) {
  slots_out(b->rb.host + o_out + (size_t)k * AR_OUT, SC_ATT_MAX_HYPS, i * (size_t)nbest, nh, {att, fused}, {order, status});
}

int ar_weights_ok(double w_att, double w_ctc, double beta) {
  SC_CHECK_ARG(std::isfinite(w_att) && std::isfinite(w_ctc) && std::isfinite(beta), "w_att, w_ctc and beta must be finite");
  return SC_OK;
}
}  // namespace

extern "C" int sc_streams_set_attention_rescore_ws(sc_streams *b, size_t max_bytes) {
  SC_CHECK_ARG(b && max_bytes >= ((size_t)1 << 20), "a workspace limit of at least 1 MiB");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  b->ar_ws_limit = max_bytes;
  if (b->ar_ws_bytes > max_bytes) {   // the next call allocates within the new limit
    HIP_TRY(hipStreamSynchronize(b->stream_rb));
    (void)hipFree(b->ar_ws);
    b->ar_ws = nullptr;
    b->ar_ws_bytes = 0;
  }
  return SC_OK;
  SC_API_END
}

extern "C" int sc_streams_attention_rescore_ws(const sc_streams *b, size_t *limit, size_t *allocated) {
  SC_CHECK_ARG(b, "null");
  if (limit) *limit = b->ar_ws_limit;
  if (allocated) *allocated = b->ar_ws_bytes;
  return SC_OK;
}

extern "C" int sc_attention_rescore_lists(sc_streams *b, const int *stream_ids, int n, const int32_t *ids, const int32_t *lens,
                                          const double *scores, const int *list_sizes, int nbest, int max_len, double w_att,
                                          double w_ctc, double beta, int32_t *order, double *fused, double *att,
                                          int32_t *status) {
  SC_CHECK_ARG(b && stream_ids && lens && scores && list_sizes && n >= 0 && n <= SC_ATT_MAX_JOBS && nbest >= 0 &&
               nbest <= SC_ATT_MAX_HYPS && max_len >= 0 && max_len < 65535 && (ids || max_len == 0), "bad arguments");
  SC_API_BEGIN
  HIP_TRY(hipSetDevice(b->eng->device));
  RC_TRY(ar_weights_ok(w_att, w_ctc, beta));
  const float *wkv = nullptr, *bkv = nullptr;
  RC_TRY(ar_weights(b, &wkv, &bkv));
  for (int i = 0; i < n; ++i) {
    SC_CHECK_ARG(list_sizes[i] >= 0 && list_sizes[i] <= nbest, "a list size outside [0, nbest]");
    RC_TRY(ar_stream(b, stream_ids[i]));
  }
  const size_t rows = (size_t)n * nbest;
  const size_t o_len = ar_up(rows * sizeof(double)), o_ids = o_len + ar_up(rows * sizeof(int32_t)),
               o_out = o_ids + ar_up(rows * max_len * sizeof(int32_t));
  RC_TRY(b->rb.reserve(o_out + (size_t)std::max(n, 1) * AR_OUT, b->stream_rb));
  memcpy(b->rb.host, scores, rows * sizeof(double));
  memcpy(b->rb.host + o_len, lens, rows * sizeof(int32_t));
  if (rows * max_len) memcpy(b->rb.host + o_ids, ids, rows * max_len * sizeof(int32_t));
  std::vector<sc_dec_rescore_job> jobs;
  std::vector<int> job_of(n, -1);
  for (int i = 0; i < n; ++i) {
    if (list_sizes[i] == 0) continue;
    sc_dec_rescore_job j{};
    ar_job(b, j, stream_ids[i], wkv, bkv, w_att, w_ctc, beta, b->rb.dev + o_out + jobs.size() * AR_OUT);
    j.yseq = (const int32_t *)(b->rb.dev + o_ids) + (size_t)i * nbest * max_len;
    j.score = (const double *)b->rb.dev + (size_t)i * nbest;
    j.lens = (const int32_t *)(b->rb.dev + o_len) + (size_t)i * nbest;
    j.row_stride = max_len;
    j.n_hyp = list_sizes[i]; j.L = max_len;
    job_of[i] = (int)jobs.size();
    jobs.push_back(j);
  }
  if (!jobs.empty()) RC_TRY(ar_run(b, jobs, o_out, o_out, []() { return SC_OK; }));
  for (int i = 0; i < n; ++i)
    if (job_of[i] >= 0)
      ar_copy_out(b, o_out, job_of[i], (size_t)i, nbest, list_sizes[i], order, fused, att, status);
  return SC_OK;
  SC_API_END
}

// The first nbest entries of the listed streams' REPORTED beam states - the entries sc_ctc_beam_hyps returns -, packed on
// the device by sc_ctc_beam_pack; their first-pass scores are the entries' totals lae(pb, pnb), with a language model
// attached the fused totals sc_ctc_beam_hyps_lm reports.  ctc_score [n][nbest] receives them.
extern "C" int sc_attention_rescore_beam(sc_streams *b, const int *stream_ids, int n, int nbest, double w_att, double w_ctc,
                                         double beta, int32_t *order, double *fused, double *att, double *ctc_score,
                                         int32_t *status, int *n_hyps) {
  SC_CHECK_ARG(b && stream_ids && n_hyps && n >= 0 && nbest >= 0 && nbest <= SC_ATT_MAX_HYPS, "bad arguments");
  SC_API_BEGIN
  SC_CHECK_ARG(b->beam_on, "the beam option is off (sc_streams_set_ctc_beam)");
  SC_CHECK_ARG(n <= b->S, "more streams listed than the batch has");
  HIP_TRY(hipSetDevice(b->eng->device));
  RC_TRY(ar_weights_ok(w_att, w_ctc, beta));
  const float *wkv = nullptr, *bkv = nullptr;
  RC_TRY(ar_weights(b, &wkv, &bkv));
  std::vector<char> listed(b->S, 0);
  int max_len = 0;
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    RC_TRY(ar_stream(b, s));
    RC_TRY(listed_once(b, s, listed));
    RC_TRY(beam_ready(b, s));
    const sc_beam_t &d = b->beam.rep[s].v.d;
    n_hyps[i] = std::max(0, std::min(nbest, d.n_entries));
    for (int r = 0; r < n_hyps[i]; ++r) max_len = std::max(max_len, d.e[r].len);
  }
  SC_CHECK_ARG(max_len < 65535, "an entry too long");
  const size_t m = (size_t)n * nbest;
  if (m == 0) return SC_OK;
  // [states: n][pack jobs: m][scores: m][lens: m] go up; [ids, frames: m][max_len], [pack header: m][4], [pack scores: m][2] stay on
  // the device; [outputs] come back
  const size_t o_pj = ar_up((size_t)n * sizeof(sc_beam_t)), o_sc = o_pj + ar_up(m * sizeof(sc_ctc_beam_pack_job)),
               o_len = o_sc + ar_up(m * sizeof(double)), o_ids = o_len + ar_up(m * sizeof(int32_t)),
               o_frames = o_ids + ar_up(m * max_len * sizeof(int32_t)), o_head = o_frames + ar_up(m * max_len * sizeof(int32_t)),
               o_psc = o_head + ar_up(m * 4 * sizeof(int32_t)),
               o_out = o_psc + ar_up(m * 2 * sizeof(double));
  RC_TRY(b->rb.reserve(o_out + (size_t)n * AR_OUT, b->stream_rb));
  fill_beam_pack_jobs(b, stream_ids, n, nbest, max_len, o_pj, o_ids, o_frames, o_head, o_psc);
  double *sc_host = (double *)(b->rb.host + o_sc);
  int32_t *len_host = (int32_t *)(b->rb.host + o_len);
  std::vector<sc_dec_rescore_job> jobs;
  std::vector<int> job_of(n, -1);
  for (int i = 0; i < n; ++i) {
    const int s = stream_ids[i];
    const BeamState &v = b->beam.rep[s].v;
    for (int r = 0; r < nbest; ++r) {
      const size_t k = (size_t)i * nbest + r;
      const bool has = r < n_hyps[i];
      sc_host[k] = has ? beam_entry_total(b, v, r) : NAN;
      len_host[k] = has ? v.d.e[r].len : 0;
      if (ctc_score) ctc_score[k] = sc_host[k];
    }
    if (n_hyps[i] == 0) continue;
    sc_dec_rescore_job j{};
    ar_job(b, j, s, wkv, bkv, w_att, w_ctc, beta, b->rb.dev + o_out + jobs.size() * AR_OUT);
    j.yseq = (const int32_t *)(b->rb.dev + o_ids) + (size_t)i * nbest * max_len;
    j.score = (const double *)(b->rb.dev + o_sc) + (size_t)i * nbest;
    j.lens = (const int32_t *)(b->rb.dev + o_len) + (size_t)i * nbest;
    j.row_stride = max_len;
    j.n_hyp = n_hyps[i]; j.L = max_len;
    job_of[i] = (int)jobs.size();
    jobs.push_back(j);
  }
  if (!jobs.empty())
    RC_TRY(ar_run(b, jobs, o_ids, o_out, [&]() -> int {
      if (max_len == 0) return SC_OK;   // every entry is the empty prefix: there is nothing to pack
      return sc_ctc_beam_pack((const sc_ctc_beam_pack_job *)(b->rb.dev + o_pj), (int)m, b->stream_rb);
    }));
  for (int i = 0; i < n; ++i)
    if (job_of[i] >= 0)
      ar_copy_out(b, o_out, job_of[i], (size_t)i, nbest, n_hyps[i], order, fused, att, status);
  return SC_OK;
  SC_API_END
}
