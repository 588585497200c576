// CTC Viterbi forced alignment (sc_ctc_align): token spans over the encoder frames and a per-token confidence, from the
// CTC emission table the beam search scored its hypotheses against (sc_search.ctcx).  tests/ctc_align_ref.py is the
// contract this file reproduces bit for bit (the path and its fp32 score).
//
// Two launches per call, both on the caller's stream:
//   row_lse_kernel    one wave per emission row: lse_t = log sum_v exp e[t][v] (NaN when the row holds a non-finite
//                     value), written into the job's workspace.  Wide and bandwidth-bound: every row is read once.
//   ctc_align_kernel  one wave64 per job, no barrier inside the frame loop.  Lane l holds the NPL states
//                     [l*NPL, (l+1)*NPL) of the 2L+1 (blank, y0, blank, ..., blank) in VGPRs; s-1 and s-2 of its first
//                     two states come from lane l-1 by two __shfl_up.  The emissions e[t][label(s)] are gathered PF
//                     frames ahead (L2 latency).  Backpointers take 2 bits per state: one dword per lane and frame for
//                     NPL <= 16, two for NPL = 32, stored coalesced ([t][word][64 lanes]).  The backtrace walks tiles of 64
//                     frames: the wave loads the few lanes' words the path can touch in those frames into LDS and lane 0
//                     walks them there.  Last, lane per frame: the token spans and lp(t, y) = e[t][y] - lse_t, summed per
//                     token in frame order.
// The table is only read.
#include "common.h"

namespace {

constexpr int AL_PF = 4;          // frames of emissions in flight ahead of the recurrence
constexpr int AL_TILE = 64;       // frames per backtrace tile
constexpr int AL_TILE_W = 68;     // dwords per tile row in LDS (>= the columns x words any NPL can touch in 64 frames)

__device__ __forceinline__ size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace of one job: [lse / lp: T floats][path: T int32][backpointers: T x 2 x 64 dwords]
__device__ __forceinline__ float *ws_lse(const sc_ctc_align_job &j) { return (float *)j.ws; }
__device__ __forceinline__ int32_t *ws_path(const sc_ctc_align_job &j) { return (int32_t *)((char *)j.ws + align256((size_t)j.T * 4)); }
__device__ __forceinline__ uint32_t *ws_bp(const sc_ctc_align_job &j) {
  return (uint32_t *)((char *)j.ws + 2 * align256((size_t)j.T * 4));
}

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// grid (ceil(max_T / 4), n_jobs), 256 threads: wave w of block x handles row 4x + w of job y
__global__ __launch_bounds__(256) void row_lse_kernel(const sc_ctc_align_job *__restrict__ jobs) {
  const sc_ctc_align_job j = jobs[blockIdx.y];
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= j.T) return;
  const float *row = j.emis + (size_t)t * j.stride;
  // per lane: online (max, sum of exp(x - max)); any non-finite value poisons the row
  float m = -INFINITY, s = 0.f;
  bool bad = false;
  for (int v = lane; v < j.V; v += 64) {
    const float x = row[v];
    bad |= !isfinite(x);
    if (x > m) {
      s = s * expf(m - x) + 1.f;
      m = x;
    } else {
      s += expf(x - m);
    }
  }
  const float M = wave_max(bad ? INFINITY : m);
  float part = (m == -INFINITY) ? 0.f : s * expf(m - M);
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  const bool any_bad = __any(bad);
  if (lane == 0) ws_lse(j)[t] = any_bad ? NAN : M + logf(part);
}

template <int NPL>
__global__ __launch_bounds__(64) void ctc_align_kernel(const sc_ctc_align_job *__restrict__ jobs) {
  constexpr int NL = NPL / 2;                // label states per lane (states alternate blank, label: NPL is even)
  constexpr int NW = NPL > 16 ? 2 : 1;       // backpointer dwords per lane and frame
  __shared__ uint32_t tile[AL_TILE][AL_TILE_W];
  __shared__ int32_t tpath[AL_TILE];
  __shared__ int32_t sh_s;
  const sc_ctc_align_job j = jobs[blockIdx.x];
  const int lane = threadIdx.x;
  const int T = j.T, L = j.L, S = 2 * L + 1;
  const float *lse = ws_lse(j);

  // ---- status: bad arguments, non-finite rows, infeasible ----------------------------------------------------------
  int st = SC_ALIGN_OK;
  if (T < 0 || L < 0 || S > 64 * NPL || j.V <= 0 || j.blank < 0 || j.blank >= j.V) st = SC_ALIGN_BAD_INPUT;
  if (st == SC_ALIGN_OK) {
    bool badlab = false;
    int reps = 0;
    for (int i = lane; i < L; i += 64) {
      const int y = j.labels[i];
      badlab |= (y < 0 || y >= j.V || y == j.blank);
      reps += (i > 0 && y == j.labels[i - 1]);
    }
    bool nonfin = false;
    for (int t = lane; t < T; t += 64) nonfin |= !isfinite(lse[t]);
    for (int o = 32; o > 0; o >>= 1) reps += __shfl_xor(reps, o);
    if (__any(badlab)) st = SC_ALIGN_BAD_INPUT;
    else if (__any(nonfin)) st = SC_ALIGN_NONFINITE;
    else if (T < L + reps) st = SC_ALIGN_INFEASIBLE;
  }
  if (st != SC_ALIGN_OK || T == 0) {
    for (int i = lane; i < L; i += 64) {
      j.start[i] = -1;
      j.end[i] = -1;
      j.logp_mean[i] = NAN;
    }
    if (lane == 0) {
      *j.status = st;
      *j.path_score = st == SC_ALIGN_OK ? 0.f : -INFINITY;
    }
    return;
  }

  // ---- forward recurrence ---------------------------------------------------------------------------------------------
  const int s0 = lane * NPL;
  int lab[NL];
  uint32_t skip = 0, valid = 0;   // bit k: state s0+k may take s-2 / exists
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int s = s0 + k;
    if (s < S) valid |= 1u << k;
    if ((k & 1) && s < S) {
      const int i = s >> 1;
      if (i > 0 && j.labels[i] != j.labels[i - 1]) skip |= 1u << k;
    }
  }
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    const int i = (s0 >> 1) + q;
    lab[q] = i < L ? j.labels[i] : j.blank;
  }
  float d[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) d[k] = -INFINITY;
  if (lane == 0) d[0] = 0.f;   // virtual frame -1: every path starts at state 0 or 1 of frame 0

  const float *E = j.emis;
  const size_t ld = (size_t)j.stride;
  float eb[AL_PF], el[AL_PF][NL];
#pragma unroll
  for (int p = 0; p < AL_PF; ++p) {
    const float *row = E + (size_t)min(p, T - 1) * ld;
    eb[p] = row[j.blank];
#pragma unroll
    for (int q = 0; q < NL; ++q) el[p][q] = row[lab[q]];
  }
  uint32_t *bp = ws_bp(j);
  for (int t0 = 0; t0 < T; t0 += AL_PF) {
#pragma unroll
    for (int p = 0; p < AL_PF; ++p) {
      const int t = t0 + p;
      if (t < T) {
        const float up1 = __shfl_up(d[NPL - 1], 1), up2 = __shfl_up(d[NPL - 2], 1);
        const float in1 = lane == 0 ? -INFINITY : up1, in2 = lane == 0 ? -INFINITY : up2;
        uint32_t w[NW];
#pragma unroll
        for (int q = 0; q < NW; ++q) w[q] = 0;
        // downwards: d[k-1], d[k-2] are still frame t-1's when state k is updated
#pragma unroll
        for (int k = NPL - 1; k >= 0; --k) {
          const float c1 = k >= 1 ? d[k - 1] : in1;
          const float c2 = k >= 2 ? d[k - 2] : (k == 1 ? in1 : in2);
          float best = d[k];
          uint32_t ch = 0;
          if (c1 > best) { best = c1; ch = 1; }
          if ((k & 1) && ((skip >> k) & 1) && c2 > best) { best = c2; ch = 2; }
          const float e = (k & 1) ? el[p][k >> 1] : eb[p];
          d[k] = ((valid >> k) & 1) ? best + e : -INFINITY;
          w[k >> 4] |= ch << (2 * (k & 15));
        }
#pragma unroll
        for (int q = 0; q < NW; ++q) bp[((size_t)t * 2 + q) * 64 + lane] = w[q];
      }
      const float *row = E + (size_t)min(t + AL_PF, T - 1) * ld;
      eb[p] = row[j.blank];
#pragma unroll
      for (int q = 0; q < NL; ++q) el[p][q] = row[lab[q]];
    }
  }

  // ---- final state: S-1 (trailing blank) replaces S-2 only if strictly greater ----------------------------------------
  auto state_value = [&](int s) {
    float v = d[0];
#pragma unroll
    for (int k = 1; k < NPL; ++k)
      if (k == s % NPL) v = d[k];
    return __shfl(v, s / NPL);
  };
  int s = S - 1;
  float score = state_value(S - 1);
  if (S >= 2) {
    const float a = state_value(S - 2);
    if (!(score > a)) { score = a; s = S - 2; }
  }

  // ---- backtrace by tiles of 64 frames --------------------------------------------------------------------------------
  int32_t *path = ws_path(j);
  __syncthreads();   // the backpointer stores of every lane are visible to the tile loads
  for (int thi = T - 1; thi >= 0; thi -= AL_TILE) {
    const int tlo = max(0, thi - (AL_TILE - 1)), nf = thi - tlo + 1;
    const int clo = max(0, s - 2 * (nf - 1)) / NPL, ncol = s / NPL - clo + 1, nwd = ncol * NW;
    for (int idx = lane; idx < nf * nwd; idx += 64) {
      const int f = idx / nwd, r = idx - f * nwd;
      tile[f][r] = bp[((size_t)(tlo + f) * 2 + (r % NW)) * 64 + clo + r / NW];
    }
    __syncthreads();
    if (lane == 0) {
      for (int t = thi; t >= tlo; --t) {
        tpath[t - tlo] = s;
        if (t > 0) {
          const int k = s % NPL, c = s / NPL - clo;
          const uint32_t ch = (tile[t - tlo][c * NW + (k >> 4)] >> (2 * (k & 15))) & 3u;
          s -= min((int)ch, s);
        }
      }
      sh_s = s;
    }
    __syncthreads();
    s = sh_s;
    if (lane < nf) path[tlo + lane] = tpath[lane];
    __syncthreads();
  }

  // ---- token spans and lp(t, y) = e[t][y] - lse_t, then the per-token means in frame order -----------------------------
  float *lp = ws_lse(j);   // lse_t is replaced by lp of frame t (each lane reads and writes its own frames)
  for (int t = lane; t < T; t += 64) {
    const int sc = path[t];
    if (sc & 1) {
      const int i = sc >> 1;
      lp[t] = E[(size_t)t * ld + j.labels[i]] - lse[t];
      if (t == 0 || path[t - 1] != sc) j.start[i] = t;
      if (t == T - 1 || path[t + 1] != sc) j.end[i] = t + 1;
    }
  }
  __syncthreads();
  for (int i = lane; i < L; i += 64) {
    const int a = j.start[i], b = j.end[i];
    float acc = 0.f;
    for (int t = a; t < b; ++t) acc += lp[t];
    j.logp_mean[i] = acc / (float)(b - a);
  }
  if (lane == 0) {
    *j.status = SC_ALIGN_OK;
    *j.path_score = score;
  }
}

}  // namespace

extern "C" size_t sc_ctc_align_ws_bytes(int T) {
  const size_t t = T > 0 ? (size_t)T : 0;
  return 2 * ((t * 4 + 255) & ~(size_t)255) + t * 2 * 64 * 4;
}

extern "C" int sc_ctc_align(const sc_ctc_align_job *jobs, int n_jobs, int max_T, int max_L, void *stream) {
  SC_CHECK_ARG(n_jobs >= 0 && max_T >= 0 && max_L >= 0, "bad arguments");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(max_L <= SC_ALIGN_MAX_L, "labels longer than SC_ALIGN_MAX_L");
  if (n_jobs == 0) return SC_OK;
  hipStream_t st = (hipStream_t)stream;
  if (max_T > 0) {
    row_lse_kernel<<<dim3(cdiv(max_T, 4), n_jobs), 256, 0, st>>>(jobs);
    SC_CHECK_LAUNCH();
  }
  const int spl = cdiv(2 * max_L + 1, 64);
  if (spl <= 2) ctc_align_kernel<2><<<n_jobs, 64, 0, st>>>(jobs);
  else if (spl <= 4) ctc_align_kernel<4><<<n_jobs, 64, 0, st>>>(jobs);
  else if (spl <= 8) ctc_align_kernel<8><<<n_jobs, 64, 0, st>>>(jobs);
  else if (spl <= 16) ctc_align_kernel<16><<<n_jobs, 64, 0, st>>>(jobs);
  else ctc_align_kernel<32><<<n_jobs, 64, 0, st>>>(jobs);
  SC_CHECK_LAUNCH();
  return SC_OK;
}
