// N-gram rescoring of n-best lists (sc_lm_rescore): per row of a list the model's sum along its labels, an </s> term, the
// fused total and the list's new order.  tests/lm_rescore_ref.py is the contract, every output bit for bit.
//
// One launch per call, one workgroup of RS_WAVES wave64 per job; wave w walks the rows w, w + RS_WAVES, ...
// The sequential walk s_{t+1} = next(s_t, y_t) is a chain of dependent hash lookups, so a row is walked in tiles of 64
// labels, one lane per label, in a speculate-and-verify form that is exact for EVERY blob lm_blob.h accepts:
//   guess    lane t guesses s_t: from state 0 over the order - 1 labels before t (from state0 over all of them when there
//            are fewer) - at most order - 1 lookups, all lanes of the tile at once
//   score    (l_t, s') = score(guess_t, y_t): the lookup the row needs anyway
//   verify   s' of lane t - 1 == guess_t for every lane of the tile (shuffle; the last state of the tile before is carried
//            in a register; guess_0 = state0 is given).  When every check of a row holds, induction over t gives: every
//            guess is the state of the sequential walk, hence every l_t its value - whatever the blob's next fields say.
//   sum      the l_t of a tile go through LDS and are added in ascending t, every lane the same chain (no tree)
//   fallback a row with any mismatch is walked label by label by lane 0 and carries SC_RESCORE_SERIAL in its status; so
//            does every row of a job with SC_RESCORE_FORCE_SERIAL
// The ranks are a count over the at most 16 fused values behind one barrier.  No atomics; every output of a row is written
// by the wave that walks it, order[] by one thread per rank; plain vector stores.  The model and the rows are only read;
// of a row nothing but [0, lens[h]) is read.
#include "lm_score.h"

namespace {

constexpr int RS_WAVES = 8;   // latency-bound: two waves per SIMD hide each other's lookups; 16 rows take two rounds
constexpr int RS_THREADS = RS_WAVES * 64;
constexpr int RS_H = SC_RESCORE_MAX_HYPS;

__device__ __forceinline__ void rs_wave_sync() {   // LDS written by some lanes of the wave is read by others behind this
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool rs_finite(double x) { return fabs(x) < INFINITY; }   // false for a NaN

__global__ __launch_bounds__(RS_THREADS) void lm_rescore_kernel(const sc_lm_rescore_job *__restrict__ jobs) {
  __shared__ double s_l[RS_WAVES][64];
  __shared__ double s_fused[RS_H];
  __shared__ int s_status[RS_H];
  const sc_lm_rescore_job j = jobs[blockIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = j.n_hyp, L = j.L;
  // a malformed job writes nothing (the host-side entry point cannot see the device table); uniform over the workgroup
  if (!j.model || !j.yseq || !j.score || !j.lm || !j.eos_lm || !j.fused || !j.end_state || !j.order || !j.status ||
      n < 1 || n > RS_H || L < 0 || j.row_stride < L || j.score_stride < 1 || j.skip < 0 || j.strip < -1 ||
      (j.tok_lm && j.tok_stride < (int64_t)max(0, L - j.skip)) || !rs_finite(j.alpha) || !rs_finite(j.beta) ||
      (j.flags & ~SC_RESCORE_FORCE_SERIAL) != 0)
    return;
  const sc_lm_view lv = *j.model;
  if (lv.V != j.V || j.state0 < -1 || j.state0 >= lv.n_states || j.lm_eos < -1 || j.lm_eos >= lv.V) return;
  const int state0 = j.state0 < 0 ? lv.start_state : j.state0;
  const int K = lv.order - 1;
  const bool force = (j.flags & SC_RESCORE_FORCE_SERIAL) != 0;

  for (int h = wave; h < n; h += RS_WAVES) {   // (wave-uniform from here to the end of the loop body)
    const int len = j.lens ? j.lens[h] : L;
    const double score = j.score[(size_t)h * (size_t)j.score_stride];
    const int32_t *row = j.yseq + (size_t)h * (size_t)j.row_stride;
    bool bad = len < 0 || len > L;
    int e = bad ? 0 : len;
    if (e > j.skip && j.strip >= 0 && row[e - 1] == j.strip) --e;
    const int m = max(0, e - j.skip);
    const int32_t *y = row + j.skip;   // only y[0, m) is read
    double *tok = j.tok_lm ? j.tok_lm + (size_t)h * (size_t)j.tok_stride : nullptr;

    bool mine = false;
    for (int t = lane; t < m; t += 64) {
      const int c = y[t];
      mine = mine || c < 0 || c >= lv.V;
    }
    bad = bad || __ballot(mine) != 0;

    double lm = 0.0, eos = 0.0, fused = __longlong_as_double(0x7FF8000000000000ll);
    int end = -1, status = force ? SC_RESCORE_SERIAL : 0;
    if (bad) {
      status |= SC_RESCORE_BAD_TOKEN;
      if (tok)
        for (int t = lane; t < m; t += 64) tok[t] = 0.0;
    } else {
      bool serial = force;
      if (!serial) {
        int carry = state0;
        for (int base = 0; base < m; base += 64) {
          const int t = base + lane;
          const bool act = t < m;
          int g = 0, nx = 0;
          double l = 0.0;
          if (act) {
            int k = 0;
            if (t < K) g = state0; else k = t - K;
            for (; k < t; ++k) g = lm_advance(lv, g, y[k]);
            lm_score(lv, g, y[t], l, nx);
          }
          const int up = __shfl_up(nx, 1);
          if (__ballot(act && (lane == 0 ? carry : up) != g) != 0) {
            serial = true;
            break;
          }
          if (act && tok) tok[t] = l;
          s_l[wave][lane] = l;
          rs_wave_sync();
          const int cnt = min(64, m - base);
          for (int k = 0; k < cnt; ++k) lm = lm + s_l[wave][k];
          rs_wave_sync();   // (the next tile overwrites the buffer)
          carry = __shfl(nx, cnt - 1);
        }
        end = carry;
      }
      if (serial) {
        status |= SC_RESCORE_SERIAL;
        // what the tiles before the mismatch stored to tok has landed before lane 0 stores there again
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        double acc = 0.0;
        int s = state0;
        if (lane == 0)
          for (int t = 0; t < m; ++t) {
            double l;
            int nx;
            lm_score(lv, s, y[t], l, nx);
            if (tok) tok[t] = l;
            acc = acc + l;
            s = nx;
          }
        lm = __shfl(acc, 0);
        end = __shfl(s, 0);
      }
      if (j.lm_eos >= 0) {
        int nx;
        lm_score(lv, end, j.lm_eos, eos, nx);
      }
      const double w = __dadd_rn(__dmul_rn(j.alpha, __dadd_rn(lm, eos)), __dmul_rn(j.beta, (double)m));
      const double f = __dadd_rn(score, w);
      if (f == f) fused = f;
      if (!rs_finite(f)) status |= SC_RESCORE_NONFINITE;
    }
    if (!rs_finite(score)) status |= SC_RESCORE_NONFINITE;
    if (lane == 0) {
      j.lm[h] = lm;
      j.eos_lm[h] = eos;
      j.fused[h] = fused;
      j.end_state[h] = end;
      j.status[h] = status;
      s_fused[h] = fused;
      s_status[h] = status;
    }
  }
  __syncthreads();
  if (tid < n) {
    const bool bad_h = (s_status[tid] & (SC_RESCORE_NONFINITE | SC_RESCORE_BAD_TOKEN)) != 0;
    const double f_h = s_fused[tid];
    int rank = 0;
    for (int g = 0; g < n; ++g) {
      if (g == tid) continue;
      const bool bad_g = (s_status[g] & (SC_RESCORE_NONFINITE | SC_RESCORE_BAD_TOKEN)) != 0;
      const double f_g = s_fused[g];
      const bool ahead = bad_g != bad_h ? bad_h : (bad_h ? g < tid : (f_g > f_h || (f_g == f_h && g < tid)));
      rank += ahead ? 1 : 0;
    }
    j.order[rank] = tid;
  }
}

}  // namespace

extern "C" int sc_lm_rescore(const sc_lm_rescore_job *jobs, int n_jobs, void *stream) {
  SC_CHECK_ARG(n_jobs >= 0, "negative job count");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_RESCORE_MAX_JOBS, "more than SC_RESCORE_MAX_JOBS jobs");
  if (n_jobs == 0) return SC_OK;
  lm_rescore_kernel<<<n_jobs, RS_THREADS, 0, (hipStream_t)stream>>>(jobs);
  SC_CHECK_LAUNCH();
  return SC_OK;
}
