// Sample-rate conversion to 16 kHz (sc_resample_design / sc_resample_out_count / sc_resample, and the launch the stream
// engine issues per admission for the streams whose input rate is not 16000: streams.hip stage_copy).  DESIGN.md 8b is
// the contract; tests/resample_ref.py restates it in numpy and this file reproduces it bit for bit.
//
// Rational polyphase FIR, Kaiser-windowed sinc:
//   g = gcd(rate, 16000), L = 16000 / g, M = rate / g          output m sits at input time m * M / L
//   fc = 0.94 min(1, L / M), W = 24 / fc, Wc = ceil(W), K = 2 Wc
//   h(x) = fc sinc(fc x) I0(10 sqrt(1 - (x / W)^2)) / I0(10) for |x| <= W, else 0
//   coef[p][k] = h((k - Wc + 1) - p / L), every phase row divided by its float64 sum, rounded to f32
//   y[m] = sum_k coef[p][k] x[n0 - Wc + 1 + k],  n0 = (m M) div L, p = (m M) mod L,  x = 0 outside the signal
// fp32 in ONE order: four partial sums over k = 0, 1, 2, 3 (mod 4), each in ascending k, every product rounded before it
// is added (no fma: -ffp-contract=off), combined as (s0 + s1) + (s2 + s3).  y[m] is a function of m and the signal alone:
// neither the call nor the tile it is computed in enters.
//
// resample_kernel: grid (tiles of outputs, jobs), 256 threads.  A workgroup brings the input span of its tile (the stream's
// history, then the staged input, zeros outside) into LDS once; what a tile is depends on the job's table:
//   L <= 4 (48000, 32000, 24000, 12000, 8000: the whole table is at most 4 x 154 floats and lives in LDS too): 256
//          consecutive outputs, one per thread;
//   L > 4  (44100: 160 phases of 142 taps, 91 KB; 22050; 11025): four periods of L outputs.  The outputs m, m + L, m + 2L,
//          m + 3L share their phase row and their inputs are M apart, so a thread reads its row from the device table
//          (L2-resident) ONCE and accumulates the four outputs from it in registers.  Measured against one output per thread
//          with a row read per output (128 chunks of 640 ms): 47 against 120 us at 44100, 23 / 78 at 22050, 18 / 68 at 11025.
// The workgroup of tile 0 also leaves the last K - 1 input samples of the stream (zeros before its start) as the next
// call's history, in the OTHER of the stream's two history rows: no workgroup reads what another one writes.
#include <algorithm>
#include <map>
#include <mutex>
#include <numeric>
#include <utility>
#include <vector>

#include "common.h"
#include "resample.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 256;                            // L <= RS_LDS_L: outputs per workgroup, one per thread
constexpr int RS_SPAN = 3 * RS_TILE + SC_RS_HIST;       // ... floats of its input span: M / L <= 3 (48 kHz), K <= 154 < SC_RS_HIST
constexpr int RS_LDS_L = 4;                             // tables of at most this many phases are staged in LDS
constexpr int RS_LDS_COEF = RS_LDS_L * SC_RS_HIST;
constexpr int RS_PER = 4;                               // L > RS_LDS_L: periods of L outputs per workgroup

// x[g] of a job's stream: g counts the stream's input samples from its start
__device__ __forceinline__ float rs_sample(const sc_rs_job &j, int K, const float *__restrict__ src,
                                           const float *__restrict__ hist_in, long long g) {
  if (g < 0 || g >= j.n_before + j.n_in) return 0.f;    // before the start; behind the end (the flush of a final call)
  if (g >= j.n_before) return src[j.src_off + (g - j.n_before)];
  const long long h = g - (j.n_before - (K - 1));       // the K - 1 samples before this call
  return h >= 0 ? hist_in[h] : 0.f;
}

// the canonical order over one phase row c and the K samples under it, for R outputs whose samples are `step` apart
template <int R>
__device__ __forceinline__ void rs_dot(const float *__restrict__ c, const float *x, int step, int K, float (&y)[R]) {
  float s[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) s[r][0] = s[r][1] = s[r][2] = s[r][3] = 0.f;
  int k = 0;
  for (; k + 3 < K; k += 4) {
    const float c0 = c[k], c1 = c[k + 1], c2 = c[k + 2], c3 = c[k + 3];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s[r][0] += c0 * x[r * step + k];
      s[r][1] += c1 * x[r * step + k + 1];
      s[r][2] += c2 * x[r * step + k + 2];
      s[r][3] += c3 * x[r * step + k + 3];
    }
  }
  if (k < K) {   // K is even: two taps are left when K % 4 == 2
    const float c0 = c[k], c1 = c[k + 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s[r][0] += c0 * x[r * step + k];
      s[r][1] += c1 * x[r * step + k + 1];
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) y[r] = (s[r][0] + s[r][1]) + (s[r][2] + s[r][3]);
}

// LDS of a launch (floats): what the largest of its tables needs
__host__ __device__ inline int rs_lds_floats(int L, int M, int Wc) {
  return L <= RS_LDS_L ? RS_SPAN + RS_LDS_COEF : RS_PER * M + 2 * Wc + 2;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(sc_rs_tabs tabs, sc_rs_job one, const sc_rs_job *__restrict__ jobs,
                                                              const float *__restrict__ src, float *__restrict__ dst,
                                                              float *__restrict__ hist, int S) {
  extern __shared__ float xs[];
  const sc_rs_job j = jobs ? jobs[blockIdx.y] : one;
  const int L = tabs.L[j.tab], M = tabs.M[j.tab], Wc = tabs.Wc[j.tab], K = 2 * Wc;
  const float *__restrict__ coef = tabs.coef[j.tab];
  const float *hist_in = hist ? hist + ((size_t)j.par * S + j.stream) * SC_RS_HIST : nullptr;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && hist) {   // next call's history: the last K - 1 samples the stream has taken
    float *hist_out = hist + ((size_t)(1 - j.par) * S + j.stream) * SC_RS_HIST;
    if (tid < K - 1) hist_out[tid] = rs_sample(j, K, src, hist_in, j.n_before + j.n_in - (K - 1) + tid);
  }
  const int tile = L <= RS_LDS_L ? RS_TILE : RS_PER * L;
  const long long ta = (long long)blockIdx.x * tile;
  if (ta >= j.n_out) return;
  const long long ma = j.m0 + ta;
  const int nt = (int)(j.n_out - ta < tile ? j.n_out - ta : tile);
  const long long lo = (ma * M) / L - Wc + 1;
  if (L <= RS_LDS_L) {
    float *cs = xs + RS_SPAN;
    const int span = (int)(((ma + nt - 1) * M) / L + Wc - lo + 1);   // <= (RS_TILE - 1) * 3 + 1 + K <= RS_SPAN
    for (int i = tid; i < span; i += RS_THREADS) xs[i] = rs_sample(j, K, src, hist_in, lo + i);
    for (int i = tid; i < L * K; i += RS_THREADS) cs[i] = coef[i];
    __syncthreads();
    if (tid >= nt) return;
    const long long mm = (ma + tid) * M;
    float y[1];
    rs_dot<1>(cs + (int)(mm % L) * K, xs + (int)(mm / L - Wc + 1 - lo), 0, K, y);
    dst[j.dst_off + ta + tid] = y[0];
    return;
  }
  // the span of RS_PER periods: slot i < L starts at most M samples in, its last output (RS_PER - 1) * M further on
  const int size = RS_PER * M + K + 2;
  for (int i = tid; i < size; i += RS_THREADS) xs[i] = rs_sample(j, K, src, hist_in, lo + i);
  __syncthreads();
  for (int i = tid; i < L && i < nt; i += RS_THREADS) {
    const long long mm = (ma + i) * M;
    float y[RS_PER];
    rs_dot<RS_PER>(coef + (size_t)(mm % L) * K, xs + (int)(mm / L - Wc + 1 - lo), M, K, y);
#pragma unroll
    for (int r = 0; r < RS_PER; ++r)
      if (i + r * L < nt) dst[j.dst_off + ta + i + r * L] = y[r];
  }
}

double bessel_i0(double x) {   // power series: every term positive, 60 terms reach 1e-17 relative for x <= 10
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 60; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
  }
  return sum;
}

// tables uploaded for sc_resample: one per (device, rate), kept for the life of the process
std::mutex rs_cache_mutex;
std::map<std::pair<int, int>, float *> rs_cache;

}  // namespace

bool sc_rs_params(int rate, int *L, int *M, int *Wc) {
  if (rate < 8000 || rate > 48000) return false;
  const int g = std::gcd(rate, 16000);
  const int l = 16000 / g, m = rate / g;
  if (l > 640) return false;
  const double fc = 0.94 * std::min(1.0, (double)l / (double)m), W = 24.0 / fc;
  *L = l;
  *M = m;
  *Wc = (int)std::ceil(W);
  return true;
}

long sc_rs_out_count(int L, int M, int Wc, long n_in_total, bool is_final) {
  const long n = is_final ? n_in_total : n_in_total - Wc;
  return n <= 0 ? 0 : (n * L + M - 1) / M;
}

long long sc_rs_tiles(const sc_rs_tabs &tabs, int tab, long long n_out) {
  const int tile = tabs.L[tab] <= RS_LDS_L ? RS_TILE : RS_PER * tabs.L[tab];
  return std::max<long long>(1, (n_out + tile - 1) / tile);
}

int sc_rs_launch(const sc_rs_tabs &tabs, const sc_rs_job *one, const sc_rs_job *jobs_dev, int n_jobs, long long tiles,
                 const float *src, float *dst, float *hist, int S, hipStream_t st) {
  if (n_jobs <= 0) return SC_OK;
  SC_CHECK_ARG(tiles >= 1 && tiles <= 0x7fffffffLL && n_jobs <= 65535, "too many tiles / jobs for one launch");
  int lds = 0;
  for (int t = 0; t < SC_RS_MAX_TABS; ++t)
    if (tabs.coef[t]) lds = std::max(lds, rs_lds_floats(tabs.L[t], tabs.M[t], tabs.Wc[t]));
  // (at most 4 x 1920 + 156 floats = 31 KB: L <= 640 and M <= 3 L)
  resample_kernel<<<dim3((unsigned)tiles, (unsigned)n_jobs), RS_THREADS, lds * sizeof(float), st>>>(
      tabs, one ? *one : sc_rs_job{}, jobs_dev, src, dst, hist, S);
  SC_CHECK_LAUNCH();
  return SC_OK;
}

extern "C" int sc_resample_design(int rate, int *L, int *M, int *half_width, float *coef) {
  int l, m, wc;
  if (!sc_rs_params(rate, &l, &m, &wc)) {
    sc_set_error("sc_resample_design: unsupported input rate %d (supported: 8000..48000 Hz with 16000 / gcd(rate, 16000) <= 640)", rate);
    return SC_ERR_ARG;
  }
  if (L) *L = l;
  if (M) *M = m;
  if (half_width) *half_width = wc;
  if (!coef) return SC_OK;
  const int K = 2 * wc;
  const double fc = 0.94 * std::min(1.0, (double)l / (double)m), W = 24.0 / fc, i0b = bessel_i0(10.0);
  std::vector<double> row(K);
  for (int p = 0; p < l; ++p) {
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
      const double x = (double)(k - wc + 1) - (double)p / (double)l;
      double h = 0.0;
      if (std::fabs(x) <= W) {
        const double a = M_PI * fc * x, r = x / W;
        const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
        h = fc * sinc * bessel_i0(10.0 * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
      }
      row[k] = h;
      sum += h;
    }
    for (int k = 0; k < K; ++k) coef[(size_t)p * K + k] = (float)(row[k] / sum);
  }
  return SC_OK;
}

extern "C" long sc_resample_out_count(int rate, long n_in_total, int is_final) {
  int l, m, wc;
  if (!sc_rs_params(rate, &l, &m, &wc) || n_in_total < 0) {
    sc_set_error("sc_resample_out_count: unsupported input rate %d or a negative count", rate);
    return SC_ERR_ARG;
  }
  return sc_rs_out_count(l, m, wc, n_in_total, is_final != 0);
}

extern "C" long sc_resample(const float *x_dev, long n_in, int rate, float *y_dev, long y_cap, void *stream) {
  int l, m, wc;
  if (!sc_rs_params(rate, &l, &m, &wc) || n_in < 0 || (n_in > 0 && !x_dev)) {
    sc_set_error("sc_resample: unsupported input rate %d (supported: 8000..48000 Hz with 16000 / gcd(rate, 16000) <= 640), "
                 "a negative count or a null input", rate);
    return SC_ERR_ARG;
  }
  const long n_out = sc_rs_out_count(l, m, wc, n_in, true);
  if (n_out > y_cap || (n_out > 0 && !y_dev)) {
    sc_set_error("sc_resample: the output holds %ld samples, %ld are produced", y_cap, n_out);
    return SC_ERR_ARG;
  }
  if (n_out == 0) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    sc_set_error("sc_resample: no HIP device");
    return SC_ERR_LAUNCH;
  }
  sc_rs_tabs tabs{};
  {
    std::lock_guard<std::mutex> lock(rs_cache_mutex);
    float *&tab = rs_cache[{dev, rate}];
    if (!tab) {
      std::vector<float> host((size_t)l * 2 * wc);
      (void)sc_resample_design(rate, nullptr, nullptr, nullptr, host.data());
      float *d = nullptr;
      if (hipMalloc((void **)&d, host.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        if (d) (void)hipFree(d);
        sc_set_error("sc_resample: uploading the coefficient table failed");
        return SC_ERR_LAUNCH;
      }
      tab = d;
    }
    tabs.coef[0] = tab;
  }
  tabs.L[0] = l; tabs.M[0] = m; tabs.Wc[0] = wc;
  sc_rs_job one{};
  one.n_in = n_in;
  one.n_out = n_out;
  const int rc = sc_rs_launch(tabs, &one, nullptr, 1, sc_rs_tiles(tabs, 0, n_out), x_dev, y_dev, nullptr, 0, (hipStream_t)stream);
  return rc == SC_OK ? n_out : rc;
}
