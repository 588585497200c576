// Energy curve of a long recording for the cut search of file mode (sc_segment_frame_count / sc_segment_design /
// sc_segment_energy).  DESIGN.md 8c is the contract; tests/segment_ref.py restates it in numpy.  For int16 x[0..n) at 16 kHz:
//   s[0] = x[0], s[i] = x[i] - 0.97 x[i-1]                        (on the int16 values)
//   F = 1 if n <= 400 else 1 + ceil((n - 400) / 160)              frames of 400 samples every 160, zeros behind the end
//   P_f[k] = |rfft_512(frame f, zero padded)[k]|^2 / 512,  E_f[j] = sum_k P_f[k] fb[j][k] (26 triangular mel filters),
//   E_f[j] == 0 -> 2^-52,  p[f] = (sum_j log E_f[j]) / 10
//   y[f] = - sum_{d = -80..80} w[d] p[refl(f + d)],  w[d] = exp(-d^2 / 800) / sum,  refl: i mod 2F, then 2F-1-i if >= F
// Float64 throughout, no fma (-ffp-contract=off), every sum in ONE order (k, j and d ascending), one writer per output: a
// value is a function of the signal and its frame index alone.
//
// seg_energy_kernel: 256 threads own SEG_TILE consecutive frames.  Their sample span (plus the sample before it) is brought
//   into LDS as int16 once; per frame the pre-emphasised samples go bit-reversed into a 512-point complex radix-2 FFT in
//   LDS (one butterfly per thread and stage, twiddles from a table in LDS) - ONE real frame per transform: packing two
//   frames into one would leak rounding noise of a loud frame into a silent neighbour, whose exact zeros the eps rule
//   needs.  The power spectra of the tile stay in LDS; then one thread per (frame, filter) sums its filter's bins (the
//   nonzero weights are packed, a bin feeds at most two filters), applies the zero rule and log, and one thread per frame
//   adds the 26 logs.
// seg_smooth_kernel: SM_TILE outputs per workgroup; the tile and its 80-frame halos come into LDS through refl (any F >= 1),
//   then 161 taps per thread.
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "common.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_TILE = 8;                              // frames per workgroup of seg_energy_kernel
constexpr int SEG_WIN = 400, SEG_HOP = 160, SEG_NFFT = 512, SEG_LOG2N = 9, SEG_BINS = SEG_NFFT / 2 + 1, SEG_NFILT = 26;
constexpr int SEG_SPAN = (SEG_TILE - 1) * SEG_HOP + SEG_WIN;   // samples under a tile
constexpr int SEG_WTS = 512;                             // packed nonzero filter weights: bins[26] + bins[27] - bins[1] <= 512
constexpr int SM_TILE = 256;                             // outputs per workgroup of seg_smooth_kernel, one per thread
constexpr int SM_HALO = 80, SM_TAPS = 2 * SM_HALO + 1;
constexpr double SEG_PREEMPH = 0.97;
constexpr double SEG_EPS = 2.220446049250313e-16;

static_assert(SEG_NFFT / 2 == SEG_THREADS, "one butterfly per thread");
static_assert(SEG_TILE * SEG_NFILT <= SEG_THREADS && SM_TILE == SEG_THREADS, "one thread per (frame, filter) / output");

struct SegTab {                  // designed on the host in double, one copy per device
  double tw[SEG_NFFT];           // exp(-2 pi i j / 512), j < 256: (cos, -sin) pairs
  double gauss[SM_TAPS];
  double wts[SEG_WTS];           // filter j: fb[j][lo[j] .. hi[j]) at wts[off[j] ..]
  int lo[SEG_NFILT], hi[SEG_NFILT], off[SEG_NFILT];
};

__global__ __launch_bounds__(SEG_THREADS) void seg_energy_kernel(const int16_t *__restrict__ pcm, long n, long F,
                                                                 const SegTab *__restrict__ tab, double *__restrict__ p) {
  __shared__ double re[SEG_NFFT], im[SEG_NFFT], tw[SEG_NFFT], wts[SEG_WTS];
  __shared__ double pw[SEG_TILE][SEG_BINS], le[SEG_TILE][SEG_NFILT];
  __shared__ int flo[SEG_NFILT], fhi[SEG_NFILT], foff[SEG_NFILT];
  __shared__ short xs[SEG_SPAN + 1];                     // xs[i] = x[t0 - 1 + i], 0 outside the signal
  const int tid = threadIdx.x;
  const long f0 = (long)blockIdx.x * SEG_TILE;
  if (f0 >= F) return;
  const int nf = (int)(F - f0 < SEG_TILE ? F - f0 : SEG_TILE);
  const long t0 = f0 * SEG_HOP;
  for (int i = tid; i < SEG_SPAN + 1; i += SEG_THREADS) {
    const long g = t0 - 1 + i;
    xs[i] = (g >= 0 && g < n) ? pcm[g] : (short)0;
  }
  for (int i = tid; i < SEG_NFFT; i += SEG_THREADS) tw[i] = tab->tw[i];
  for (int i = tid; i < SEG_WTS; i += SEG_THREADS) wts[i] = tab->wts[i];
  if (tid < SEG_NFILT) {
    flo[tid] = tab->lo[tid];
    fhi[tid] = tab->hi[tid];
    foff[tid] = tab->off[tid];
  }
  __syncthreads();
  for (int fi = 0; fi < nf; ++fi) {
    for (int i = tid; i < SEG_NFFT; i += SEG_THREADS) {
      double v = 0.0;
      const long g = t0 + (long)fi * SEG_HOP + i;
      if (i < SEG_WIN && g < n) {                        // zeros behind the end are appended AFTER the pre-emphasis
        const double a = (double)xs[fi * SEG_HOP + i + 1], b = (double)xs[fi * SEG_HOP + i];
        v = g == 0 ? a : a - SEG_PREEMPH * b;            // x[-1] is absent: s[0] = x[0]
      }
      const int rev = (int)(__brev((unsigned)i) >> (32 - SEG_LOG2N));
      re[rev] = v;
      im[rev] = 0.0;
    }
    __syncthreads();
    for (int sft = 1; sft <= SEG_LOG2N; ++sft) {
      const int hm = 1 << (sft - 1), j = tid & (hm - 1);
      const int i0 = ((tid >> (sft - 1)) << sft) + j, i1 = i0 + hm;
      const int t = j << (SEG_LOG2N - sft);
      const double wr = tw[2 * t], wi = tw[2 * t + 1];
      const double xr = re[i1], xi = im[i1];
      const double vr = xr * wr - xi * wi, vi = xr * wi + xi * wr;
      const double ur = re[i0], ui = im[i0];
      re[i0] = ur + vr;
      im[i0] = ui + vi;
      re[i1] = ur - vr;
      im[i1] = ui - vi;
      __syncthreads();
    }
    for (int k = tid; k < SEG_BINS; k += SEG_THREADS) pw[fi][k] = (re[k] * re[k] + im[k] * im[k]) * (1.0 / SEG_NFFT);
    __syncthreads();
  }
  if (tid < nf * SEG_NFILT) {
    const int fi = tid / SEG_NFILT, j = tid % SEG_NFILT;
    const int lo = flo[j], hi = fhi[j], off = foff[j];
    double e = 0.0;
    for (int k = lo; k < hi; ++k) e += pw[fi][k] * wts[off + k - lo];
    le[fi][j] = log(e == 0.0 ? SEG_EPS : e);
  }
  __syncthreads();
  if (tid < nf) {
    double s = 0.0;
    for (int j = 0; j < SEG_NFILT; ++j) s += le[tid][j];
    p[f0 + tid] = s / 10.0;
  }
}

__device__ __forceinline__ long seg_refl(long i, long F) {
  const long m = 2 * F;
  long r = i % m;
  if (r < 0) r += m;
  return r >= F ? m - 1 - r : r;
}

__global__ __launch_bounds__(SEG_THREADS) void seg_smooth_kernel(const double *__restrict__ p, long F,
                                                                 const SegTab *__restrict__ tab, double *__restrict__ y) {
  __shared__ double ps[SM_TILE + 2 * SM_HALO], w[SM_TAPS];
  const int tid = threadIdx.x;
  const long f0 = (long)blockIdx.x * SM_TILE;
  if (f0 >= F) return;
  for (int i = tid; i < SM_TILE + 2 * SM_HALO; i += SEG_THREADS) ps[i] = p[seg_refl(f0 - SM_HALO + i, F)];
  for (int i = tid; i < SM_TAPS; i += SEG_THREADS) w[i] = tab->gauss[i];
  __syncthreads();
  if (f0 + tid >= F) return;
  double acc = 0.0;
  for (int d = 0; d < SM_TAPS; ++d) acc += w[d] * ps[tid + d];
  y[f0 + tid] = -acc;
}

// integer bin edges floor(513 mel2hz(m_i) / 16000) of the 26 + 2 mel points between 0 and 8000 Hz
void seg_bin_edges(int (&bins)[SEG_NFILT + 2]) {
  const double lo = 2595.0 * std::log10(1.0 + 0.0 / 700.0), hi = 2595.0 * std::log10(1.0 + 8000.0 / 700.0);
  const double step = (hi - lo) / (double)(SEG_NFILT + 1);
  for (int i = 0; i < SEG_NFILT + 2; ++i) {
    const double mel = i == SEG_NFILT + 1 ? hi : (double)i * step + lo;
    const double hz = 700.0 * (std::pow(10.0, mel / 2595.0) - 1.0);
    bins[i] = (int)std::floor((double)(SEG_NFFT + 1) * hz / 16000.0);
  }
}

struct SegDev { SegTab *tab = nullptr; double *ws = nullptr; long ws_cap = 0; };
std::mutex seg_mutex;
std::map<int, SegDev> seg_devs;

}  // namespace

extern "C" long sc_segment_frame_count(long n_samples) {
  if (n_samples < 1) {
    sc_set_error("sc_segment_frame_count: %ld samples (at least one is needed)", n_samples);
    return SC_ERR_ARG;
  }
  return n_samples <= SEG_WIN ? 1 : 1 + (n_samples - SEG_WIN + SEG_HOP - 1) / SEG_HOP;
}

extern "C" int sc_segment_design(double *fb, double *gauss) {
  if (fb) {
    int bins[SEG_NFILT + 2];
    seg_bin_edges(bins);
    for (int i = 0; i < SEG_NFILT * SEG_BINS; ++i) fb[i] = 0.0;
    for (int j = 0; j < SEG_NFILT; ++j) {
      const int lo = bins[j], mid = bins[j + 1], hi = bins[j + 2];
      for (int i = lo; i < mid; ++i) fb[j * SEG_BINS + i] = (double)(i - lo) / (double)(mid - lo);
      for (int i = mid; i < hi; ++i) fb[j * SEG_BINS + i] = (double)(hi - i) / (double)(hi - mid);
    }
  }
  if (gauss) {
    long double sum = 0.0L;
    for (int d = -SM_HALO; d <= SM_HALO; ++d) {
      gauss[d + SM_HALO] = std::exp(-(double)(d * d) / 800.0);
      sum += (long double)gauss[d + SM_HALO];
    }
    for (int i = 0; i < SM_TAPS; ++i) gauss[i] = gauss[i] / (double)sum;
  }
  return SC_OK;
}

extern "C" long sc_segment_energy(const int16_t *pcm_dev, long n_samples, int smoothed, double *out_dev, long out_cap,
                                  void *stream) {
  SC_CHECK_ARG(pcm_dev && out_dev, "null pointer");
  SC_CHECK_ARG(n_samples >= 1, "at least one sample is needed");
  const long F = sc_segment_frame_count(n_samples);
  if (F > out_cap) {
    sc_set_error("sc_segment_energy: the output holds %ld frames, %ld are produced", out_cap, F);
    return SC_ERR_ARG;
  }
  SC_CHECK_ARG((F + SEG_TILE - 1) / SEG_TILE <= 0x7fffffffL, "too many frames for one launch");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    sc_set_error("sc_segment_energy: no HIP device");
    return SC_ERR_LAUNCH;
  }
  const SegTab *tab = nullptr;
  double *raw = out_dev;
  {
    std::lock_guard<std::mutex> lock(seg_mutex);
    SegDev &sd = seg_devs[dev];
    if (!sd.tab) {
      std::vector<double> fb((size_t)SEG_NFILT * SEG_BINS);
      std::vector<SegTab> host(1);
      SegTab &t = host[0];
      (void)sc_segment_design(fb.data(), t.gauss);
      for (int j = 0; j < SEG_NFFT / 2; ++j) {
        const double a = 2.0 * M_PI * (double)j / (double)SEG_NFFT;
        t.tw[2 * j] = std::cos(a);
        t.tw[2 * j + 1] = -std::sin(a);
      }
      int bins[SEG_NFILT + 2], off = 0;
      seg_bin_edges(bins);
      for (int i = 0; i < SEG_WTS; ++i) t.wts[i] = 0.0;
      for (int j = 0; j < SEG_NFILT; ++j) {
        t.lo[j] = bins[j];
        t.hi[j] = bins[j + 2];
        t.off[j] = off;
        if (bins[j] < 0 || bins[j + 2] > SEG_BINS || bins[j + 2] < bins[j] || off + (bins[j + 2] - bins[j]) > SEG_WTS) {
          sc_set_error("sc_segment_energy: the filter table does not fit its packed form");
          return SC_ERR_ARG;
        }
        for (int k = bins[j]; k < bins[j + 2]; ++k) t.wts[off++] = fb[(size_t)j * SEG_BINS + k];
      }
      SegTab *d = nullptr;
      if (hipMalloc((void **)&d, sizeof(SegTab)) != hipSuccess ||
          hipMemcpy(d, &t, sizeof(SegTab), hipMemcpyHostToDevice) != hipSuccess) {
        if (d) (void)hipFree(d);
        sc_set_error("sc_segment_energy: uploading the tables failed");
        return SC_ERR_LAUNCH;
      }
      sd.tab = d;
    }
    tab = sd.tab;
    if (smoothed) {
      if (F > sd.ws_cap) {   // geometric: few reallocations (a hipFree waits for the device)
        const long cap = F > 2 * sd.ws_cap ? F : 2 * sd.ws_cap;
        if (sd.ws) (void)hipFree(sd.ws);
        sd.ws = nullptr;
        sd.ws_cap = 0;
        if (hipMalloc((void **)&sd.ws, (size_t)cap * sizeof(double)) != hipSuccess) {
          sd.ws = nullptr;
          sc_set_error("sc_segment_energy: no memory for the raw curve of %ld frames", cap);
          return SC_ERR_LAUNCH;
        }
        sd.ws_cap = cap;
      }
      raw = sd.ws;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  seg_energy_kernel<<<(unsigned)((F + SEG_TILE - 1) / SEG_TILE), SEG_THREADS, 0, st>>>(pcm_dev, n_samples, F, tab, raw);
  SC_CHECK_LAUNCH();
  if (smoothed) {
    seg_smooth_kernel<<<(unsigned)((F + SM_TILE - 1) / SM_TILE), SEG_THREADS, 0, st>>>(raw, F, tab, out_dev);
    SC_CHECK_LAUNCH();
  }
  return F;
}
