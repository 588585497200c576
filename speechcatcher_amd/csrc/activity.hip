// CTC speech activity (sc_ctc_activity): per-frame blank posterior of the rows of a CTC table and the running
// speech / silence state of a stream over them.  tests/ctc_activity_ref.py is the contract.
//
// One launch per call, one workgroup of ACT_WAVES = 16 wave64 per job, the job's span [t0, t1) in tiles of ACT_TILE frames:
//   row pass   the waves take the tile's rows in turn, each by the row pass of ctc_row.h; lane 0 writes
//              p_blank = exp(x[blank] - lse) to the stream's track and to LDS.  NaN for a bad row.
//   scan pass  wave 0 walks the tile 64 frames at a time: __ballot gives the speech and the bad mask, their popcounts
//              and first / last set bits update the state, which the wave keeps in registers across tiles.
// No atomics; every output has one writer (lane 0 of one wave); plain vector stores.  The table is only read.
#include "ctc_row.h"

namespace {

constexpr int ACT_WAVES = 16;   // a group's jobs hold about 16 rows each: one row per wave
constexpr int ACT_UNROLL = 8;
constexpr int ACT_TILE = 256;   // frames whose p_blank the workgroup holds in LDS between the two passes

// p_blank of one row, computed by one wave (every lane returns it)
__device__ __forceinline__ double row_p_blank(const float *__restrict__ row, int V, int blank, int lane) {
  const CtcRowLse r = ctc_row_combine(ctc_row_pass<ACT_UNROLL>(row, V, lane, [](const float (&)[ACT_UNROLL], int, bool) {}));
  return r.bad ? NAN : exp((double)row[blank] - r.lse);
}

__global__ __launch_bounds__(ACT_WAVES * 64) void ctc_activity_kernel(const sc_ctc_activity_job *__restrict__ jobs) {
  __shared__ double pb[ACT_TILE];
  const sc_ctc_activity_job j = jobs[blockIdx.x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (!ctc_job_ok(j) || !j.state) return;   // (a malformed job writes nothing)

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
  return ctc_launch_jobs(__func__, jobs, n_jobs, SC_ACTIVITY_MAX_JOBS, "more than SC_ACTIVITY_MAX_JOBS jobs",
                         [&] { ctc_activity_kernel<<<n_jobs, ACT_WAVES * 64, 0, (hipStream_t)stream>>>(jobs); });
}
