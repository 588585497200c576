// Wire-format audio in (sc_pcm_decode): interleaved s16 / s24 / u8 / G.711 / f32 codes at any byte address -> mono fp32
// samples, with the running input level of a stream over them.  tests/pcm_ref.py is the contract.
//
// One launch per call, one workgroup of PCM_THREADS = 256 threads per job; the workgroup walks the job's n frames in tiles
// of 256, thread = frame.  A frame's codes are assembled from BYTE loads, which are legal at any address (packed s24, odd
// offsets); s16 and f32 frames on a naturally aligned address take one load per code instead.  The integer formats keep
// m exact in int32 (at most 8 x 2^23), divide in float64 and round to fp32 once; the level (all integer, exact in any
// order) is kept per thread in registers, reduced across the wave by shuffles and across the four waves through LDS,
// and thread 0 is the only writer of the job's level and of its state-after copy.
// No atomics; every output has one writer; plain vector stores.  The source is only read.
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

constexpr int PCM_THREADS = 256;

__host__ __device__ __forceinline__ int pcm_code_bytes(int format) {
  return format == SC_PCM_F32 ? 4 : format == SC_PCM_S16LE ? 2 : format == SC_PCM_S24LE ? 3 : 1;
}
__host__ __device__ __forceinline__ int pcm_full_scale_bits(int format) {
  return format == SC_PCM_S24LE ? 23 : format == SC_PCM_U8 ? 7 : 15;
}

__device__ __forceinline__ int mulaw_value(unsigned b) {
  const unsigned u = ~b & 0xFFu;
  const int mag = (int)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u)) - 0x84;
  return (u & 0x80u) ? -mag : mag;
}
__device__ __forceinline__ int alaw_value(unsigned b) {
  const unsigned a = (b ^ 0x55u) & 0xFFu;
  const unsigned e = (a >> 4) & 7u;
  const int mag = e == 0 ? (int)(((a & 15u) << 4) + 8u) : (int)((((a & 15u) << 4) + 0x108u) << (e - 1u));
  return (a & 0x80u) ? mag : -mag;
}

// value of one integer code at p; *ext: it sits at its format's extreme
__device__ __forceinline__ int code_value(const uint8_t *__restrict__ p, int format, bool aligned, bool *ext) {
  int v;
  switch (format) {
    case SC_PCM_S16LE: {
      const unsigned w = aligned ? (unsigned)*reinterpret_cast<const uint16_t *>(p) : ((unsigned)p[0] | ((unsigned)p[1] << 8));
      v = (int)(int16_t)(uint16_t)w;
      *ext = v == -32768 || v == 32767;
      break;
    }
    case SC_PCM_S24LE: {
      const unsigned w = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
      v = (int)(w << 8) >> 8;   // sign extension of bit 23
      *ext = v == -8388608 || v == 8388607;
      break;
    }
    case SC_PCM_U8:
      v = (int)p[0] - 128;
      *ext = v == -128 || v == 127;
      break;
    case SC_PCM_MULAW:
      v = mulaw_value(p[0]);
      *ext = v == -32124 || v == 32124;
      break;
    default:   // SC_PCM_ALAW
      v = alaw_value(p[0]);
      *ext = v == -32256 || v == 32256;
      break;
  }
  return v;
}

__device__ __forceinline__ uint32_t f32_bits(const uint8_t *__restrict__ p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint32_t *>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_decode_kernel(const sc_pcm_job *__restrict__ jobs) {
  __shared__ long long red_sum[PCM_THREADS / 64], red_clip[PCM_THREADS / 64];
  __shared__ int red_peak[PCM_THREADS / 64];
  const sc_pcm_job j = jobs[blockIdx.x];
  // a malformed job writes nothing (the host-side entry point cannot see the device table)
  if (!j.src || !j.dst || !j.level || j.format < 0 || j.format >= SC_PCM_N_FORMATS || j.channels < 1 ||
      j.channels > SC_PCM_MAX_CHANNELS || j.channel < SC_PCM_MIX || j.channel >= j.channels || j.offset < 0 || j.n < 0)
    return;
  const bool b15 = j.format == SC_PCM_S16LE || j.format == SC_PCM_MULAW || j.format == SC_PCM_ALAW;
  if (!(j.scale == SC_PCM_SCALE_FULL || (j.scale == SC_PCM_SCALE_SERVER && b15))) return;

  const int cb = pcm_code_bytes(j.format), C = j.channels;
  const size_t bpf = (size_t)cb * (size_t)C;
  const uint8_t *__restrict__ base = static_cast<const uint8_t *>(j.src) + j.offset;
  // every code of the chunk is naturally aligned iff its first one is (the frame size is a multiple of the code size)
  const bool aligned = (reinterpret_cast<uintptr_t>(base) & (uintptr_t)(cb - 1)) == 0 && (cb == 2 || cb == 4);
  const bool mix = j.channel == SC_PCM_MIX;
  const int c_lo = mix ? 0 : j.channel, c_hi = mix ? C : j.channel + 1;
  const double div = mix ? (double)C : 1.0;

  long long t_sum = 0, t_clip = 0;
  int t_peak = 0;
  if (j.format == SC_PCM_F32) {
    for (int i = threadIdx.x; i < j.n; i += PCM_THREADS) {
      const uint8_t *f = base + (size_t)i * bpf;
      uint32_t bits;
      if (!mix) {
        bits = f32_bits(f + 4 * (size_t)j.channel, aligned);   // the selected channel's bits, NaNs included
      } else {
        float s = __uint_as_float(f32_bits(f, aligned));
        for (int c = 1; c < C; ++c) s = s + __uint_as_float(f32_bits(f + 4 * (size_t)c, aligned));
        const float r = (float)((double)s / div);
        bits = r != r ? 0x7fc00000u : __float_as_uint(r);
      }
      reinterpret_cast<uint32_t *>(j.dst)[i] = bits;
    }
  } else {
    const float unit = 1.0f / (float)(1 << pcm_full_scale_bits(j.format));   // 2^-B: the product below is exact
    for (int i = threadIdx.x; i < j.n; i += PCM_THREADS) {
      const uint8_t *f = base + (size_t)i * bpf;
      int m = 0;
      bool clip = false;
      for (int c = c_lo; c < c_hi; ++c) {
        bool ext;
        m += code_value(f + (size_t)c * cb, j.format, aligned, &ext);
        clip |= ext;
      }
      const float x = (float)((double)m / div);   // RN_fp32 of the exact quotient (53 >= 2 * 24 + 2: one rounding)
      j.dst[i] = j.scale == SC_PCM_SCALE_SERVER ? __half2float(__float2half_rn(x)) * unit : x * unit;
      const int a = m < 0 ? -m : m;
      t_sum += a;
      t_peak = max(t_peak, a);
      t_clip += clip ? 1 : 0;
    }
  }

  // the level: per wave by shuffles, across the waves through LDS, one writer
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  t_sum = wave_sum_i64(t_sum);
  t_clip = wave_sum_i64(t_clip);
  t_peak = wave_max_i32(t_peak);
  if (lane == 0) {
    red_sum[wave] = t_sum;
    red_clip[wave] = t_clip;
    red_peak[wave] = t_peak;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sc_input_level_t o = {0, 0, 0, 0, 0};
    if (!j.restart) o = *j.level;
    if (j.format == SC_PCM_F32) {
      o.full_scale = 0;
    } else {
      o.frames += j.n;
      for (int w = 0; w < PCM_THREADS / 64; ++w) {
        o.sum_abs += red_sum[w];
        o.clipped += red_clip[w];
        o.peak = max(o.peak, red_peak[w]);
      }
      o.full_scale = (mix ? C : 1) << pcm_full_scale_bits(j.format);
    }
    *j.level = o;
    if (j.level_after) *j.level_after = o;
  }
}

}  // namespace

extern "C" int sc_pcm_bytes_per_frame(int format, int channels) {
  SC_CHECK_ARG(format >= 0 && format < SC_PCM_N_FORMATS, "format out of range");
  SC_CHECK_ARG(channels >= 1 && channels <= SC_PCM_MAX_CHANNELS, "channels outside 1..8");
  return pcm_code_bytes(format) * channels;
}

extern "C" int sc_pcm_decode(const sc_pcm_job *jobs, int n_jobs, void *stream) {
  SC_CHECK_ARG(n_jobs >= 0, "negative job count");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_PCM_MAX_JOBS, "more than SC_PCM_MAX_JOBS jobs");
  if (n_jobs == 0) return SC_OK;
  pcm_decode_kernel<<<n_jobs, PCM_THREADS, 0, (hipStream_t)stream>>>(jobs);
  SC_CHECK_LAUNCH();
  return SC_OK;
}
