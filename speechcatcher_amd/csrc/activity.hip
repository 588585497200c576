// CTC speech activity (sc_ctc_activity): per-frame blank posterior of the rows of a CTC table and the running
// speech / silence state of a stream over them.  tests/ctc_activity_ref.py is the contract.
//
// One launch per call, one workgroup of ACT_WAVES = 16 wave64 per job, the job's span [t0, t1) in tiles of ACT_TILE frames:
//   row pass   the waves take the tile's rows in turn.  Lanes stride over V with an online (max, sum of exp(x - max)) in
//              float64; the wave combines them in one fixed order (xor butterfly), lane 0 writes
//              p_blank = exp(x[blank] - lse) to the stream's track and to LDS.  NaN for a bad row (a NaN, a +inf, or
//              nothing but -inf).
//   scan pass  wave 0 walks the tile 64 frames at a time: __ballot gives the speech and the bad mask, their popcounts
//              and first / last set bits update the state, which the wave keeps in registers across tiles.
// No atomics; every output has one writer (lane 0 of one wave); plain vector stores.  The table is only read.
#include "common.h"

namespace {

constexpr int ACT_WAVES = 16;   // a group's jobs hold about 16 rows each: one row per wave
constexpr int ACT_UNROLL = 8;
constexpr int ACT_TILE = 256;   // frames whose p_blank the workgroup holds in LDS between the two passes

__device__ __forceinline__ double wave_max_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// p_blank of one row, computed by one wave (every lane returns it)
__device__ __forceinline__ double row_p_blank(const float *__restrict__ row, int V, int blank, int lane) {
  double m = -INFINITY, s = 0.0;
  bool bad = false;
  // ACT_UNROLL values per lane at a time: their loads are in flight together, the running sum is rescaled at most once
  // per batch (to the batch's maximum) and the batch's terms are added in ascending v
  for (int v0 = lane; v0 < V; v0 += 64 * ACT_UNROLL) {
    double x[ACT_UNROLL];
#pragma unroll
    for (int k = 0; k < ACT_UNROLL; ++k) {
      const int v = v0 + 64 * k;
      x[k] = v < V ? (double)row[v] : -INFINITY;
    }
    double cm = x[0];
#pragma unroll
    for (int k = 0; k < ACT_UNROLL; ++k) {
      bad |= (x[k] != x[k]) || x[k] == INFINITY;
      cm = fmax(cm, x[k]);
    }
    if (cm > m) {
      s = m == -INFINITY ? 0.0 : s * exp(m - cm);
      m = cm;
    }
    if (m > -INFINITY) {   // (a -inf entry adds exp(-inf) = 0; a bad row's sum is never used)
#pragma unroll
      for (int k = 0; k < ACT_UNROLL; ++k) s += exp(x[k] - m);
    }
  }
  const bool any_bad = __any(bad);
  const double M = wave_max_f64(m);
  if (any_bad || M == -INFINITY) return NAN;   // (wave-uniform)
  const double sum = wave_sum_f64(m == -INFINITY ? 0.0 : s * exp(m - M));
  return exp((double)row[blank] - (M + log(sum)));
}

__global__ __launch_bounds__(ACT_WAVES * 64) void ctc_activity_kernel(const sc_ctc_activity_job *__restrict__ jobs) {
  __shared__ double pb[ACT_TILE];
  const sc_ctc_activity_job j = jobs[blockIdx.x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // a malformed job writes nothing (the host-side entry point cannot see the device table)
  if (!j.table || !j.state || j.V < 1 || j.blank < 0 || j.blank >= j.V || j.t0 < 0 || j.t1 < j.t0) return;

  int n = 0, n_speech = 0, n_bad = 0, first = -1, last = -1;
  if (wave == 0 && !j.restart) {
    n = j.state[0]; n_speech = j.state[1]; n_bad = j.state[2]; first = j.state[3]; last = j.state[4];
  }
  for (int tb = j.t0; tb < j.t1; tb += ACT_TILE) {
    const int nt = min(ACT_TILE, j.t1 - tb);
    for (int i = wave; i < nt; i += ACT_WAVES) {
      const double p = row_p_blank(j.table + (size_t)(tb + i) * (size_t)j.stride, j.V, j.blank, lane);
      if (lane == 0) {
        pb[i] = p;
        if (j.track) j.track[tb + i] = p;
      }
    }
    __syncthreads();
    if (wave == 0) {
      for (int base = 0; base < nt; base += 64) {
        const int i = base + lane;
        const bool valid = i < nt;
        const double p = valid ? pb[i] : 0.0;
        const bool bad = valid && (p != p);
        const bool speech = valid && !bad && !(p > j.thr);
        const unsigned long long msp = __ballot(speech), mbad = __ballot(bad);
        if (msp) {
          if (first < 0) first = n + (__ffsll((long long)msp) - 1);
          last = n + (63 - __clzll((long long)msp));
        }
        n_speech += __popcll(msp);
        n_bad += __popcll(mbad);
        n += min(64, nt - base);
      }
    }
    __syncthreads();   // the tile is free for the next row pass
  }
  if (wave == 0 && lane == 0) {
    const int trail = last >= 0 ? n - 1 - last : n;
    j.state[0] = n; j.state[1] = n_speech; j.state[2] = n_bad; j.state[3] = first; j.state[4] = last; j.state[5] = trail;
    if (j.state_after) {
      int32_t *o = j.state_after;
      o[0] = n; o[1] = n_speech; o[2] = n_bad; o[3] = first; o[4] = last; o[5] = trail;
    }
  }
}

}  // namespace

extern "C" int sc_ctc_activity(const sc_ctc_activity_job *jobs, int n_jobs, void *stream) {
  SC_CHECK_ARG(n_jobs >= 0, "negative job count");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_ACTIVITY_MAX_JOBS, "more than SC_ACTIVITY_MAX_JOBS jobs");
  if (n_jobs == 0) return SC_OK;
  ctc_activity_kernel<<<n_jobs, ACT_WAVES * 64, 0, (hipStream_t)stream>>>(jobs);
  SC_CHECK_LAUNCH();
  return SC_OK;
}
