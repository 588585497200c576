// What the scanners of the CTC table share (activity.hip, spot.hip, draft.hip, ctc_beam.hip; the bad-value test also
// alternates.hip): the row pass of one wave, the check of a job's common fields, and the entry points' launch path.
// tests/ctc_row_ref.py is the contract of a row.
//
// A row x[0..V) of the fp32 table is BAD when it holds a NaN or a +inf, or nothing but -inf.  Otherwise, with x promoted
// to float64, lse = M + log(sum_v exp(x[v] - M)), M = max_v x[v].  One wave computes it: lane l takes v = l, l + 64, ...
// in batches of UNROLL values with an online (max, sum of exp(x - max)); the 64 lanes are combined by xor butterflies in
// one fixed order.  UNROLL fixes where a lane's running sum is rescaled and so the bits of lse: a kernel keeps its own.
#pragma once
#include "common.h"

__device__ __forceinline__ bool ctc_bad_value(float x) { return (x != x) || x == INFINITY; }

__device__ __forceinline__ double wave_max_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// a lane's share of a row: m = its maximum so far, s = the sum of exp(x - m) over its values so far
struct CtcRowAcc {
  double m = -INFINITY, s = 0.0;
  bool bad = false;
};

// One batch: the values v0, v0 + 64, ... (UNROLL of them; -inf behind V).  Their loads are in flight together, the
// running sum is rescaled at most once per batch (to the batch's maximum) and the batch's terms are added in ascending v.
// Before the sum moves the caller sees the batch: see(xf, vmax, rose) with the fp32 values, the v of the FIRST of the
// batch's maxima, and whether the lane's running maximum rises with this batch (a lane sees its v ascending, so taking
// vmax only when `rose` keeps the lowest index of the row's maximum).
template <int UNROLL, class See>
__device__ __forceinline__ void ctc_row_batch(CtcRowAcc &a, const float *__restrict__ row, int V, int v0, See &&see) {
  float xf[UNROLL];
  double x[UNROLL];
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    const int v = v0 + 64 * k;
    xf[k] = v < V ? row[v] : -INFINITY;
    x[k] = (double)xf[k];
  }
  double cm = x[0];
  int ck = 0;
#pragma unroll
  for (int k = 0; k < UNROLL; ++k) {
    a.bad |= ctc_bad_value(xf[k]);
    if (x[k] > cm) { cm = x[k]; ck = k; }
  }
  const bool rose = cm > a.m;
  see(xf, v0 + 64 * ck, rose);
  if (rose) {
    a.s = a.m == -INFINITY ? 0.0 : a.s * exp(a.m - cm);
    a.m = cm;
  }
  if (a.m > -INFINITY) {   // (a -inf entry adds exp(-inf) = 0; a bad row's sum is never used)
#pragma unroll
    for (int k = 0; k < UNROLL; ++k) a.s += exp(x[k] - a.m);
  }
}

// the whole row, batch after batch
template <int UNROLL, class See>
__device__ __forceinline__ CtcRowAcc ctc_row_pass(const float *__restrict__ row, int V, int lane, See &&see) {
  CtcRowAcc a;
  for (int v0 = lane; v0 < V; v0 += 64 * UNROLL) ctc_row_batch<UNROLL>(a, row, V, v0, see);
  return a;
}

// The wave's result from its lanes' shares, the same in every lane: bad, or the maximum M and lse.  The overload with M
// is for a caller whose own butterfly has the wave's maximum already (draft.hip: together with its arg-max).
struct CtcRowLse {
  bool bad;
  double M, lse;
};
__device__ __forceinline__ CtcRowLse ctc_row_combine(const CtcRowAcc &a, double M) {
  if (__any(a.bad) || M == -INFINITY) return {true, M, NAN};   // (wave-uniform)
  const double sum = wave_sum_f64(a.m == -INFINITY ? 0.0 : a.s * exp(a.m - M));
  return {false, M, M + log(sum)};
}
__device__ __forceinline__ CtcRowLse ctc_row_combine(const CtcRowAcc &a) { return ctc_row_combine(a, wave_max_f64(a.m)); }

// The fields every scanner's job has.  A malformed job writes nothing (the host-side entry point cannot see the device
// table); each kernel adds the conditions on the fields of its own.
template <class Job>
__device__ __forceinline__ bool ctc_job_ok(const Job &j) {
  return j.table && j.V >= 1 && j.blank >= 0 && j.blank < j.V && j.t0 >= 0 && j.t1 >= j.t0;
}

// Behind the sc_ctc_* entry points: the checks of the job table, then launch().  `fn` is the entry point's name and
// `too_many` its text for a count above max_jobs.
template <class Launch>
static inline int ctc_launch_jobs(const char *fn, const void *jobs, int n_jobs, int max_jobs, const char *too_many,
                                  Launch &&launch) {
  const char *wrong = n_jobs < 0 ? "negative job count" : n_jobs != 0 && !jobs ? "null job table" : n_jobs > max_jobs ? too_many : nullptr;
  if (wrong) {
    sc_set_error("%s: %s", fn, wrong);
    return SC_ERR_ARG;
  }
  if (n_jobs == 0) return SC_OK;
  launch();
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    sc_set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
    return SC_ERR_LAUNCH;
  }
  return SC_OK;
}
