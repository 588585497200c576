// CTC draft transcript (sc_ctc_draft): the collapsed arg-max path of the rows of a CTC table - token ids with frame times
// and a posterior - and the running greedy state of a stream over them.  tests/ctc_draft_ref.py is the contract
// (DESIGN.md 8f).
//
// One launch per call, one workgroup of DR_WAVES = 16 wave64 per job, the job's span [t0, t1) in tiles of DR_TILE frames:
//   row pass   the waves take the tile's rows in turn, each by the row pass of ctc_row.h with the lane's lowest arg-max
//              index kept beside it; the wave's maximum comes from an xor butterfly whose arg-max merge prefers the
//              lower index on equal maxima, so the label is exact in any order.  Lane 0 writes the label (DR_BAD for
//              a bad row) and p = exp(x[k] - lse) to LDS.
//   scan pass  wave 0 walks the tile 64 frames at a time, lane = frame.  The previous frame's label comes from __shfl_up
//              (lane 0: the carried open token); __ballot of "opens a token" and "continues the previous frame's token"
//              gives every run's slot (popcount), start and end (first unset continue bit above it); a segmented max
//              over the run gives its conf.  A run that ends inside the batch is stored by its first lane, the carried
//              token by lane 0; the run that reaches the last frame stays open in registers across batches and tiles.
// No atomics; every output has one writer; plain vector stores.  The table is only read.
#include "ctc_row.h"

namespace {

constexpr int DR_WAVES = 16;   // a group's jobs hold about 16 rows each: one row per wave
constexpr int DR_UNROLL = 8;
constexpr int DR_TILE = 256;   // frames whose label and posterior the workgroup holds in LDS between the two passes
constexpr int DR_BAD = -2;     // label of a bad row (-1: a blank or bad frame as the scan's "no token")

// label and posterior of one row, computed by one wave (every lane returns them); label DR_BAD: a bad row
__device__ __forceinline__ int row_best(const float *__restrict__ row, int V, int lane, double *p_out) {
  int K = 0x7fffffff;   // the lane's lowest arg-max index
  const CtcRowAcc a = ctc_row_pass<DR_UNROLL>(row, V, lane, [&](const float (&)[DR_UNROLL], int vmax, bool rose) {
    if (rose) K = vmax;
  });
  double M = a.m;
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(M, o);
    const int ok = __shfl_xor(K, o);
    if (om > M || (om == M && ok < K)) { M = om; K = ok; }
  }
  const CtcRowLse r = ctc_row_combine(a, M);
  *p_out = r.bad ? NAN : exp(M - r.lse);   // x[K] == M
  return r.bad ? DR_BAD : K;
}

__device__ __forceinline__ void put_token(sc_draft_token *t, int id, int start, int end, double conf) {
  t->id = id; t->start = start; t->end = end; t->reserved = 0; t->conf = conf;
}

__global__ __launch_bounds__(DR_WAVES * 64) void ctc_draft_kernel(const sc_ctc_draft_job *__restrict__ jobs) {
  __shared__ double pp[DR_TILE];
  __shared__ int lab[DR_TILE];
  const sc_ctc_draft_job j = jobs[blockIdx.x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (!ctc_job_ok(j) || !j.state || j.stride < j.V || j.capacity < 0 || (j.capacity > 0 && !j.tokens))
    return;   // (a malformed job writes nothing)

  // the state, wave-uniform in wave 0's registers
  int n = 0, n_closed = 0, n_bad = 0, oid = -1, ost = -1, oen = -1;
  double ocf = 0.0;
  if (wave == 0 && !j.restart) {
    n = j.state->n_frames; n_closed = j.state->n_closed; n_bad = j.state->n_bad;
    oid = j.state->open_id; ost = j.state->open_start; oen = j.state->open_end; ocf = j.state->open_conf;
  }
  for (int tb = j.t0; tb < j.t1; tb += DR_TILE) {
    const int nt = min(DR_TILE, j.t1 - tb);
    for (int i = wave; i < nt; i += DR_WAVES) {
      double p;
      const int k = row_best(j.table + (size_t)(tb + i) * (size_t)j.stride, j.V, lane, &p);
      if (lane == 0) {
        lab[i] = k;
        pp[i] = p;
      }
    }
    __syncthreads();
    if (wave == 0) {
      for (int base = 0; base < nt; base += 64) {
        const int nv = min(64, nt - base);   // (< 64 only in the span's last batch: the lanes behind it break every run)
        const bool valid = lane < nv;
        const int k = valid ? lab[base + lane] : DR_BAD;
        const double p = valid ? pp[base + lane] : 0.0;
        const bool bad = valid && k == DR_BAD;
        const bool tok = valid && !bad && k != j.blank;
        const int cur = tok ? k : -1;   // the token this frame belongs to; -1: none
        int prev = __shfl_up(cur, 1);
        if (lane == 0) prev = oid;
        const bool cont = tok && cur == prev;
        const bool opens = tok && !cont;
        const unsigned long long mo = __ballot(opens), mc = __ballot(cont), mbad = __ballot(bad);
        // e: the last lane of the run this lane belongs to = the lane below the first non-continuing lane above it
        const unsigned long long above = lane == 63 ? 0ull : (~mc & (~0ull << (lane + 1)));
        const int e = above ? __ffsll((long long)above) - 2 : 63;
        // conf: max of p over [lane, e] (suffix scan bounded by the run's end)
        double c = tok ? p : 0.0;
        for (int d = 1; d < 64; d <<= 1) {
          const double o = __shfl_down(c, d);
          if (tok && lane + d <= e) c = fmax(c, o);
        }
        // the carried token: continued by the first `lead` lanes, closed when the batch goes on behind them
        const int lead = ~mc ? __ffsll((long long)~mc) - 1 : 64;
        const double c0 = __shfl(c, 0);
        int carried_closed = 0;
        if (oid >= 0) {
          if (lead > 0) {
            oen = n + lead - 1;
            ocf = fmax(ocf, c0);
          }
          if (lead < nv) {
            if (lane == 0 && n_closed < j.capacity) put_token(j.tokens + n_closed, oid, ost, oen, ocf);
            carried_closed = 1;
            oid = ost = oen = -1;
            ocf = 0.0;
          }
        }
        // runs opened in this batch: every earlier one has closed before the next opens, so slot = tokens before it
        if (opens && e < nv - 1) {
          const int slot = n_closed + carried_closed + __popcll(mo & ((1ull << lane) - 1ull));
          if (slot < j.capacity) put_token(j.tokens + slot, k, n + lane, n + e, c);
        }
        int opened = __popcll(mo);
        if (mo) {
          const int ls = 63 - __clzll((long long)mo);   // the last run opened: still open iff it reaches the last frame
          const int le = __shfl(e, ls);
          if (le == nv - 1) {
            oid = __shfl(k, ls);
            ost = n + ls;
            oen = n + le;
            ocf = __shfl(c, ls);
            opened -= 1;
          }
        }
        n_closed += carried_closed + opened;
        n_bad += __popcll(mbad);
        n += nv;
      }
    }
    __syncthreads();   // the tile is free for the next row pass
  }
  if (wave == 0 && lane == 0) {
    sc_draft_t o;
    o.n_frames = n; o.n_closed = n_closed; o.n_bad = n_bad; o.open_id = oid; o.open_start = ost; o.open_end = oen;
    o.open_conf = ocf;
    *j.state = o;
    if (j.state_after) *j.state_after = o;
  }
}

}  // namespace

extern "C" int sc_ctc_draft(const sc_ctc_draft_job *jobs, int n_jobs, void *stream) {
  return ctc_launch_jobs(__func__, jobs, n_jobs, SC_DRAFT_MAX_JOBS, "more than SC_DRAFT_MAX_JOBS jobs",
                         [&] { ctc_draft_kernel<<<n_jobs, DR_WAVES * 64, 0, (hipStream_t)stream>>>(jobs); });
}
