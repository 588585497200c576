// CTC token alternates (sc_ctc_alternates): for every token span of a label sequence over a CTC table, the K tokens with
// the largest summed emission over the span's frames, their mean log-posterior, and the rank of the span's own label.
// tests/ctc_alt_ref.py is the contract.
//
// One launch per call, one workgroup of 256 threads per (job, span); a workgroup whose span index is >= the job's L
// leaves at once, and the span is checked before any row is read.
//   row walk   thread `tid` owns the vocabulary entries tid + 256 i, i < NV (NV = 8 / 16 / 32 by the job's V), and keeps
//              their float64 sums S in registers.  The span's rows are taken in ascending frame order with coalesced loads
//              (for NV = 8 / 16 the next row is in flight while the current one is summed): S += (double)x is the
//              contract's sum bit for bit.  Per frame a wave takes the max of its values (fp32 butterfly) and the float64
//              sum of exp(x - max) in one fixed order; lane 0 leaves the pair in LDS.  No barrier inside a tile of
//              ALT_TILE frames.  The instantiation is chosen inside the kernel: V lives in the device table.
//   lse        after a tile, wave 0 merges the four pairs of each frame (lane = frame) into lse_t and adds the lse_t to
//              the running sum in frame order (readlane by readlane).  A frame whose maximum is -inf is a bad row; NaN
//              and +inf are flagged by the thread that loaded them and reduced with the barrier.
//   top-K      K rounds of a block arg-max under (S descending, v ascending): thread-local over the entries not yet
//              taken, wave butterfly, four pairs in LDS, every thread reads the winner.  own_rank is a block count.
// No atomics; every output has one writer (thread 0); plain vector stores.  Table, labels and spans are only read.
#include "ctc_row.h"

namespace {

constexpr int ALT_THREADS = 256;
constexpr int ALT_WAVES = ALT_THREADS / 64;
constexpr int ALT_TILE = 64;   // frames whose per-wave (max, sum) pairs the workgroup holds in LDS between two merges
constexpr int ALT_NONE = 0x7fffffff;

struct AltShared {
  float pm[ALT_TILE][ALT_WAVES];    // per frame and wave: max of the wave's values
  double ps[ALT_TILE][ALT_WAVES];   //                     sum of exp(x - that max)
  double bs[ALT_WAVES];             // arg-max round: best S of each wave ...
  int bv[ALT_WAVES];                // ... and its v (ALT_NONE: the wave has no candidate left)
  int cnt[ALT_WAVES];
  double own_s;                     // S[y] of the span's own label
  double sum_lse;
  int neg_row;                      // a row of the span holds nothing but -inf
};

__device__ __forceinline__ void alt_sentinels(const sc_ctc_alt_job &j, int k, int K, int st) {
  if (threadIdx.x == 0) {
    for (int q = 0; q < K; ++q) {
      j.alt_ids[(size_t)k * K + q] = -1;
      j.alt_logp[(size_t)k * K + q] = -INFINITY;
    }
    j.own_rank[k] = -1;
    j.status[k] = st;
  }
}

// (a, av) is ahead of (b, bv) in the candidates' order
__device__ __forceinline__ bool alt_ahead(double a, int av, double b, int bv) {
  if (av == ALT_NONE) return false;
  if (bv == ALT_NONE) return true;
  return a > b || (a == b && av < bv);
}

template <int NV>
__device__ __forceinline__ void alt_span(const sc_ctc_alt_job &j, int k, int K, int s, int e, int y, AltShared &sh) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int V = j.V;
  const int nv = (V - tid + ALT_THREADS - 1) / ALT_THREADS;   // entries this thread owns (<= NV; 0 when tid >= V)
  const size_t ld = (size_t)j.stride;
  double S[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) S[i] = 0.0;
  bool bad = false;
  double sum_lse = 0.0;   // (wave 0, every lane the same)
  bool neg_row = false;

  constexpr bool PF = NV <= 16;   // the next row is loaded while this one is summed (NV = 32: 32 loads in flight as it is)
  float xn[PF ? NV : 1];
  if (PF) {
    const float *row = j.emis + (size_t)s * ld;
#pragma unroll
    for (int i = 0; i < NV; ++i) xn[PF ? i : 0] = i < nv ? row[tid + ALT_THREADS * i] : -INFINITY;
  }
  for (int tb = s; tb < e; tb += ALT_TILE) {
    const int nt = min(ALT_TILE, e - tb);
    for (int f = 0; f < nt; ++f) {
      const float *row = j.emis + (size_t)(tb + f) * ld;
      float x[NV];
      if (PF) {
#pragma unroll
        for (int i = 0; i < NV; ++i) x[i] = xn[PF ? i : 0];
        if (tb + f + 1 < e) {
#pragma unroll
          for (int i = 0; i < NV; ++i) xn[PF ? i : 0] = i < nv ? row[ld + tid + ALT_THREADS * i] : -INFINITY;
        }
      } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) x[i] = i < nv ? row[tid + ALT_THREADS * i] : -INFINITY;
      }
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (i < nv) {
          bad |= ctc_bad_value(x[i]);
          S[i] += (double)x[i];
          m = fmaxf(m, x[i]);
        }
      }
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      // sum of exp(x - max) over the thread's entries, v ascending: from the registers for NV = 8 (a span of one or two
      // frames is a chain of memory round trips, and this saves two per frame); for NV = 16 / 32 a rolled loop over the
      // row just loaded (it is in the cache), so that the float64 exp stands once in the code and its temporaries do
      // not multiply with NV.  The same adds in the same order either way
      double p = 0.0;
      if (m > -INFINITY) {   // (wave-uniform; a -inf entry adds exp(-inf) = 0, a bad row's sum is never used)
        const double md = (double)m;
        if (NV <= 8) {
#pragma unroll
          for (int i = 0; i < NV; ++i)
            if (i < nv) p += exp((double)x[i] - md);
        } else {
#pragma unroll 2
          for (int v = tid; v < V; v += ALT_THREADS) p += exp((double)row[v] - md);
        }
      }
      for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
      if (lane == 0) {
        sh.pm[f][wave] = m;
        sh.ps[f][wave] = p;
      }
    }
    __syncthreads();
    if (wave == 0) {
      double lse = 0.0;
      bool neg = false;
      if (lane < nt) {
        float M = sh.pm[lane][0];
#pragma unroll
        for (int w = 1; w < ALT_WAVES; ++w) M = fmaxf(M, sh.pm[lane][w]);
        if (M == -INFINITY) {
          neg = true;
        } else {
          double sum = 0.0;
#pragma unroll
          for (int w = 0; w < ALT_WAVES; ++w) {
            const float mw = sh.pm[lane][w];
            if (mw > -INFINITY) sum += sh.ps[lane][w] * exp((double)mw - (double)M);
          }
          lse = (double)M + log(sum);
        }
      }
      neg_row |= __any(neg) != 0;
      for (int f = 0; f < nt; ++f) sum_lse += __shfl(lse, f);
    }
    __syncthreads();   // the tile is free for the next frames
  }
  if (tid == 0) {
    sh.sum_lse = sum_lse;
    sh.neg_row = neg_row ? 1 : 0;
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);   // (also publishes sum_lse / neg_row)
  if (any_bad || sh.neg_row) {
    alt_sentinels(j, k, K, SC_ALT_BAD_ROW);
    return;
  }
  const double inv_n = (double)(e - s);
  const double total_lse = sh.sum_lse;

  // ---- own label: S[y] to LDS, then the candidates strictly ahead of it ------------------------------------------------
  const bool own_ok = y >= 0 && y < V && y != j.blank;
  if (own_ok && (y & (ALT_THREADS - 1)) == tid) {
    const int iy = y / ALT_THREADS;
    double v = S[0];
#pragma unroll
    for (int i = 1; i < NV; ++i)
      if (i == iy) v = S[i];
    sh.own_s = v;
  }
  __syncthreads();
  int ahead = 0;
  if (own_ok) {
    const double sy = sh.own_s;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + ALT_THREADS * i;
      if (i < nv && v != j.blank && v != y && (S[i] > sy || (S[i] == sy && v < y))) ++ahead;
    }
  }
  for (int o = 32; o > 0; o >>= 1) ahead += __shfl_xor(ahead, o);
  if (lane == 0) sh.cnt[wave] = ahead;

  // ---- top-K: K rounds of a block arg-max over the entries not yet taken -----------------------------------------------
  uint32_t taken = 0;   // bit i: entry tid + 256 i has been given out
  for (int q = 0; q < K; ++q) {
    double bs = -INFINITY;
    int bv = ALT_NONE;
#pragma unroll
    for (int i = 0; i < NV; ++i) {   // v ascending: only a strictly greater S takes over
      const int v = tid + ALT_THREADS * i;
      if (i < nv && v != j.blank && !((taken >> i) & 1u) && (bv == ALT_NONE || S[i] > bs)) {
        bs = S[i];
        bv = v;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o);
      const int ov = __shfl_xor(bv, o);
      if (alt_ahead(os, ov, bs, bv)) { bs = os; bv = ov; }
    }
    if (lane == 0) {
      sh.bs[wave] = bs;
      sh.bv[wave] = bv;
    }
    __syncthreads();
    bs = sh.bs[0];
    bv = sh.bv[0];
#pragma unroll
    for (int w = 1; w < ALT_WAVES; ++w)
      if (alt_ahead(sh.bs[w], sh.bv[w], bs, bv)) { bs = sh.bs[w]; bv = sh.bv[w]; }
    if (bv != ALT_NONE && (bv & (ALT_THREADS - 1)) == tid) taken |= 1u << (bv / ALT_THREADS);
    if (tid == 0) {
      j.alt_ids[(size_t)k * K + q] = bv == ALT_NONE ? -1 : bv;
      j.alt_logp[(size_t)k * K + q] = bv == ALT_NONE ? -INFINITY : (bs - total_lse) / inv_n;
    }
    __syncthreads();   // sh.bs / sh.bv are free for the next round
  }
  if (tid == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < ALT_WAVES; ++w) c += sh.cnt[w];
    j.own_rank[k] = own_ok ? c : -1;
    j.status[k] = SC_ALT_OK;
  }
}

// grid (max_L, n_jobs): workgroup (k, job) serves span k of the job
__global__ __launch_bounds__(ALT_THREADS) void ctc_alternates_kernel(const sc_ctc_alt_job *__restrict__ jobs, int K) {
  __shared__ AltShared sh;
  const sc_ctc_alt_job j = jobs[blockIdx.y];
  const int k = blockIdx.x;
  if (k >= j.L) return;
  // a malformed job writes nothing (the host-side entry point cannot see the device table)
  if (!j.emis || !j.labels || !j.start || !j.end || !j.alt_ids || !j.alt_logp || !j.own_rank || !j.status || j.V < 1 ||
      j.V > SC_MAX_VOCAB || j.blank < 0 || j.blank >= j.V || j.T < 0 || j.L > (int)gridDim.x || j.stride < j.V)
    return;
  const int s = j.start[k], e = j.end[k], y = j.labels[k];   // (one round trip for the three)
  if (s < 0 || e <= s || e > j.T) {
    alt_sentinels(j, k, K, SC_ALT_NO_SPAN);
    return;
  }
  if (j.V <= 8 * ALT_THREADS) alt_span<8>(j, k, K, s, e, y, sh);
  else if (j.V <= 16 * ALT_THREADS) alt_span<16>(j, k, K, s, e, y, sh);
  else alt_span<32>(j, k, K, s, e, y, sh);
}

}  // namespace

extern "C" int sc_ctc_alternates(const sc_ctc_alt_job *jobs, int n_jobs, int max_L, int K, void *stream) {
  SC_CHECK_ARG(n_jobs >= 0 && max_L >= 0, "bad arguments");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_ALT_MAX_JOBS, "more than SC_ALT_MAX_JOBS jobs");
  SC_CHECK_ARG(max_L <= SC_ALIGN_MAX_L, "labels longer than SC_ALIGN_MAX_L");
  SC_CHECK_ARG(K >= 1 && K <= SC_ALT_MAX_K, "K outside [1, SC_ALT_MAX_K]");
  if (n_jobs == 0 || max_L == 0) return SC_OK;
  ctc_alternates_kernel<<<dim3(max_L, n_jobs), ALT_THREADS, 0, (hipStream_t)stream>>>(jobs, K);
  SC_CHECK_LAUNCH();
  return SC_OK;
}
