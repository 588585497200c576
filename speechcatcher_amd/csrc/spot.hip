// CTC phrase spotting (sc_ctc_spot): per-stream keyword detection from the rows of a CTC table.  For every enabled phrase a
// best-path recurrence over its 2L - 1 states (tokens and the blanks between them) whose score is the log-ratio of the
// phrase's path to the frame-wise best path; the phrase fires when its end state reaches its floor, and re-arms.
// tests/ctc_spot_ref.py is the contract; this kernel reproduces it bit for bit: a maximum, float64 adds
// and subtractions of promoted fp32 values, comparisons.
//
// One launch per call, one workgroup of SPOT_WAVES = 16 wave64 per job, the job's span [t0, t1) in tiles of SPOT_TILE frames:
//   pass 1  the waves take the tile's rows in turn: fp32 row maximum and bad flag (the rule of ctc_row.h) -> LDS
//   pass 2  wave w takes the enabled phrases w, w + 16, ...; lane = state.  SPOT_BATCH frames at a time: every lane
//           first issues the emission gathers x[t][label(lane)] of the batch (in flight together), then the serial frame
//           loop with shuffles from lanes - 1 and - 2; the fire decision is broadcast from the end state's lane.  A fire
//           goes to the phrase's LDS slot of that frame.
//   pass 3  wave 0, lane = phrase, merges the tile's fires frame by frame: a ballot and a prefix popcount give every
//           firing lane its own event slot - events ordered by (end, phrase).
// No atomics; every output has one writer; plain vector stores.  The table is only read.
#include "ctc_row.h"

namespace {

constexpr int SPOT_WAVES = 16;
constexpr int SPOT_TILE = 64;    // frames per tile: one bit each in a phrase's 64-bit fire mask
constexpr int SPOT_BATCH = 16;   // frames whose emission gathers are in flight together (a group's jobs hold about 16 rows)
constexpr int SPOT_P = SC_SPOT_MAX_PHRASES, SPOT_L = SC_SPOT_MAX_LEN, SPOT_S = SC_SPOT_STATES;

__device__ __forceinline__ bool spot_job_ok(const sc_ctc_spot_job &j) {
  return ctc_job_ok(j) && j.labels && j.lens && j.floors && j.counters && j.values && j.starts && j.events && j.P >= 1 &&
         j.P <= SPOT_P && j.stride >= j.V;
}

__global__ __launch_bounds__(SPOT_WAVES * 64) void ctc_spot_kernel(const sc_ctc_spot_job *__restrict__ jobs) {
  __shared__ float row_max[SPOT_TILE];
  __shared__ int row_bad[SPOT_TILE];
  __shared__ unsigned long long fire_mask[SPOT_P];   // per phrase: the tile's frames at which it fired
  __shared__ double fire_score[SPOT_TILE][SPOT_P];
  __shared__ int fire_start[SPOT_TILE][SPOT_P];
  const sc_ctc_spot_job j = jobs[blockIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // a malformed job writes nothing (the host-side entry point cannot see the device table); the phrase set belongs to
  // the job: a length outside [1, 32] or a label outside the vocabulary or equal to the blank makes it malformed
  if (!spot_job_ok(j)) return;   // (uniform)
  int wrong = 0;
  for (int i = tid; i < j.P * SPOT_L; i += SPOT_WAVES * 64) {
    const int L = j.lens[i / SPOT_L];
    if (L < 1 || L > SPOT_L) wrong = 1;
    else if (i % SPOT_L < L) {
      const int y = j.labels[i];
      wrong |= y < 0 || y >= j.V || y == j.blank;
    }
  }
  if (__syncthreads_or(wrong)) return;

  if (j.restart) {   // the span starts an utterance: every state of the set is -inf / -1
    for (int i = tid; i < j.P * SPOT_S; i += SPOT_WAVES * 64) {
      j.values[i] = -INFINITY;
      j.starts[i] = -1;
    }
    __syncthreads();
  }
  const int n0 = j.restart ? 0 : j.counters[0];
  int n_events = j.restart ? 0 : j.counters[1];

  for (int tb = j.t0; tb < j.t1; tb += SPOT_TILE) {
    const int nt = min(SPOT_TILE, j.t1 - tb);
    const int nb = n0 + (tb - j.t0);   // number of the tile's first frame
    // ---- pass 1: row maxima and bad flags ----
    if (tid < SPOT_P) fire_mask[tid] = 0ull;
    for (int i = wave; i < nt; i += SPOT_WAVES) {
      const float *__restrict__ row = j.table + (size_t)(tb + i) * (size_t)j.stride;
      float m = -INFINITY;
      bool bad = false;
      for (int v = lane; v < j.V; v += 64) {
        const float x = row[v];
        bad |= ctc_bad_value(x);
        m = fmaxf(m, x);   // (a NaN is skipped here and caught by the flag)
      }
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      const bool any_bad = __any(bad) || m == -INFINITY;
      if (lane == 0) {
        row_max[i] = m;
        row_bad[i] = any_bad ? 1 : 0;
      }
    }
    __syncthreads();
    // ---- pass 2: the recurrence, one wave per phrase, lane = state ----
    for (int p = wave; p < j.P; p += SPOT_WAVES) {
      if (!((j.mask >> p) & 1ull)) continue;   // a disabled phrase's states are not touched
      const int L = j.lens[p], S = 2 * L - 1, E = 2 * L - 2;
      const bool used = lane < S;
      const int tok = j.labels[p * SPOT_L + min(lane >> 1, L - 1)];
      const int lab = (used && !(lane & 1)) ? tok : j.blank;
      const int tok_prev = j.labels[p * SPOT_L + max(min(lane >> 1, L - 1) - 1, 0)];
      const bool skip = used && !(lane & 1) && lane >= 2 && tok != tok_prev;
      const double floor_p = j.floors[p];
      double v = used ? j.values[p * SPOT_S + lane] : -INFINITY;
      int st = used ? j.starts[p * SPOT_S + lane] : -1;
      unsigned long long fm = 0ull;
      for (int f0 = 0; f0 < nt; f0 += SPOT_BATCH) {
        float x[SPOT_BATCH];
#pragma unroll
        for (int k = 0; k < SPOT_BATCH; ++k) {
          const int f = min(f0 + k, nt - 1);   // (the batch's tail re-reads the tile's last row: in bounds, unused)
          x[k] = j.table[(size_t)(tb + f) * (size_t)j.stride + lab];
        }
#pragma unroll
        for (int k = 0; k < SPOT_BATCH; ++k) {
          const int f = f0 + k;
          if (f >= nt) break;   // (uniform)
          if (row_bad[f]) {     // (uniform) a bad frame: every state -inf / -1, nothing fires
            v = -INFINITY;
            st = -1;
            continue;
          }
          const double e = (double)x[k] - (double)row_max[f];
          const double u1 = __shfl_up(v, 1), u2 = __shfl_up(v, 2);
          const int s1 = __shfl_up(st, 1), s2 = __shfl_up(st, 2);
          double best = v;
          int bs = st;
          if (lane >= 1 && u1 > best) { best = u1; bs = s1; }
          if (skip && u2 > best) { best = u2; bs = s2; }
          if (lane == 0 && 0.0 > best) { best = 0.0; bs = nb + f; }
          double nv = used ? best + e : -INFINITY;
          int ns = nv == -INFINITY ? -1 : bs;
          const double fv = __shfl(nv, E);
          const int fs = __shfl(ns, E);
          if (fv >= floor_p) {   // (uniform) the phrase fires and re-arms
            if (lane == E) {
              fire_score[f][p] = fv;
              fire_start[f][p] = fs;
            }
            fm |= 1ull << f;
            nv = -INFINITY;
            ns = -1;
          }
          v = nv;
          st = ns;
        }
      }
      j.values[p * SPOT_S + lane] = v;   // (the unused entries [S, 64) are -inf / -1)
      j.starts[p * SPOT_S + lane] = st;
      if (lane == 0) fire_mask[p] = fm;
    }
    __syncthreads();
    // ---- pass 3: the tile's events in (end, phrase) order ----
    if (wave == 0) {
      const unsigned long long fm = fire_mask[lane];
      unsigned long long any = fm;
      for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o);
      while (any) {   // (uniform)
        const int f = __ffsll((long long)any) - 1;
        any &= any - 1ull;
        const bool fired = (fm >> f) & 1ull;
        const unsigned long long b = __ballot(fired);
        const int slot = n_events + __popcll(b & ((1ull << lane) - 1ull));
        if (fired && slot < SC_SPOT_MAX_EVENTS) {
          sc_spot_event ev;
          ev.end = nb + f;
          ev.phrase = lane;
          ev.start = fire_start[f][lane];
          ev.reserved = 0;
          ev.score = fire_score[f][lane];
          j.events[slot] = ev;
        }
        n_events += __popcll(b);
      }
    }
    __syncthreads();   // the tile's LDS is free for the next tile
  }
  if (wave == 0 && lane == 0) {
    const int n = n0 + (j.t1 - j.t0);
    j.counters[0] = n;
    j.counters[1] = n_events;
    if (j.state_after) {
      j.state_after[0] = n;
      j.state_after[1] = n_events;
    }
  }
}

}  // namespace

extern "C" int sc_ctc_spot(const sc_ctc_spot_job *jobs, int n_jobs, void *stream) {
  return ctc_launch_jobs(__func__, jobs, n_jobs, SC_SPOT_MAX_JOBS, "more than SC_SPOT_MAX_JOBS jobs",
                         [&] { ctc_spot_kernel<<<n_jobs, SPOT_WAVES * 64, 0, (hipStream_t)stream>>>(jobs); });
}
