// Stable partials (sc_hyp_commit): the committed prefix of a stream's live beam - what all its hypotheses share, which no
// later chunk can change - the share of the beam's mass behind every token after it, and the tail of the best hypothesis
// a caller does not hold yet.  tests/hyp_commit_ref.py is the contract.
//
// One launch per call, one workgroup of CM_WAVES = 4 wave64 per job:
//   compare   threads stride over the token positions [0, L); each keeps, per hypothesis h >= 1, the first position at
//             which row h differs from row 0 in a register (positions ascend per thread, so the first hit is its lowest;
//             a hypothesis that has one is not loaded again by that thread)
//   reduce    a min butterfly per wave, then a min over the waves' values in LDS: agree[h]
//   weigh     the scores are loaded one per thread beside the compare pass; thread 0: w[h] = exp(score[h] - largest finite
//             score) and Z in float64, ascending h, as the contract adds
//   write     header, agree, and for the positions [from, L) the ids and positions of row 0 and
//             stability = (sum over ascending h with agree[h] > i of w[h]) / Z - every thread the same order
// No atomics; every output has one writer; plain vector stores.  Nothing at or behind L of a row is read.
#include "common.h"

namespace {

constexpr int CM_WAVES = 4;
constexpr int CM_THREADS = CM_WAVES * 64;
constexpr int CM_H = SC_COMMIT_MAX_HYPS;

__device__ __forceinline__ bool cm_finite(double x) { return fabs(x) < INFINITY; }   // false for a NaN

__global__ __launch_bounds__(CM_THREADS) void hyp_commit_kernel(const sc_hyp_commit_job *__restrict__ jobs) {
  __shared__ int s_first[CM_WAVES][CM_H];
  __shared__ int s_agree[CM_H];
  __shared__ double s_w[CM_H];
  __shared__ double s_score[CM_H];
  __shared__ double s_z;
  __shared__ int s_status;
  const sc_hyp_commit_job j = jobs[blockIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = j.n_hyp, L = j.L;
  // a malformed job writes nothing (the host-side entry point cannot see the device table)
  if (!j.yseq || !j.xpos || !j.score || !j.score_dec || !j.score_ctc || !j.header || !j.agree || !j.ids || !j.pos ||
      !j.stability || !j.totals || n < 1 || n > CM_H || L < 0 || j.from < 0 || j.from > L || j.row_stride < L ||
      j.score_stride < 1)
    return;

  // the scores are under way while the rows are compared (one load per thread, not a serial chain in thread 0)
  if (tid < n) s_score[tid] = j.score[(size_t)tid * (size_t)j.score_stride];
  int first[CM_H];
#pragma unroll
  for (int h = 0; h < CM_H; ++h) first[h] = L;
  for (int i = tid; i < L; i += CM_THREADS) {
    const int y0 = j.yseq[i];
#pragma unroll
    for (int h = 1; h < CM_H; ++h)
      if (h < n && first[h] == L && j.yseq[(size_t)h * (size_t)j.row_stride + i] != y0) first[h] = i;
  }
#pragma unroll
  for (int h = 1; h < CM_H; ++h) {
    if (h < n) {   // (workgroup-uniform)
      int v = first[h];
      for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
      if (lane == 0) s_first[wave][h] = v;
    }
  }
  __syncthreads();
  if (tid < CM_H) {
    int v = L;
    if (tid >= 1 && tid < n)
      for (int w = 0; w < CM_WAVES; ++w) v = min(v, s_first[w][tid]);
    s_agree[tid] = v;
  }
  if (tid == 0) {
    double m = -INFINITY;
    bool any = false, all = true;
    for (int h = 0; h < n; ++h) {
      const double s = s_score[h];
      if (cm_finite(s)) {
        any = true;
        m = fmax(m, s);
      } else {
        all = false;
      }
    }
    double z = 0.0;
    for (int h = 0; h < n; ++h) {
      const double s = s_score[h];
      const double w = !any ? 1.0 : (cm_finite(s) ? exp(s - m) : 0.0);
      s_w[h] = w;
      z = z + w;
    }
    s_z = z;
    s_status = all ? 0 : SC_COMMIT_NONFINITE;
  }
  __syncthreads();

  const bool fin = (j.flags & SC_COMMIT_FINAL) != 0;
  if (tid < n) j.agree[tid] = s_agree[tid];
  if (tid == 0) {
    int commit = L;
    if (!fin)
      for (int h = 1; h < n; ++h) commit = min(commit, s_agree[h]);
    j.header[0] = L;
    j.header[1] = commit;
    j.header[2] = n;
    j.header[3] = s_status;
    j.totals[0] = s_score[0];
    j.totals[1] = j.score_dec[0];
    j.totals[2] = j.score_ctc[0];
  }
  const double z = s_z;
  for (int i = j.from + tid; i < L; i += CM_THREADS) {
    const int k = i - j.from;
    j.ids[k] = j.yseq[i];
    j.pos[k] = j.xpos[i];
    double st = 1.0;
    if (!fin) {
      double a = 0.0;
      for (int h = 0; h < n; ++h)
        if (s_agree[h] > i) a = a + s_w[h];
      st = a / z;
    }
    j.stability[k] = st;
  }
}

}  // namespace

extern "C" int sc_hyp_commit(const sc_hyp_commit_job *jobs, int n_jobs, void *stream) {
  SC_CHECK_ARG(n_jobs >= 0, "negative job count");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_COMMIT_MAX_JOBS, "more than SC_COMMIT_MAX_JOBS jobs");
  if (n_jobs == 0) return SC_OK;
  hyp_commit_kernel<<<n_jobs, CM_THREADS, 0, (hipStream_t)stream>>>(jobs);
  SC_CHECK_LAUNCH();
  return SC_OK;
}
