// Consensus of n-best lists (sc_mbr): pairwise edit distances, the minimum-Bayes-risk row, and the rows aligned against
// that pivot with the list's mass per slot.  tests/mbr_ref.py is the contract: with weights given every
// output bit for bit; with scores only exp() separates the two evaluations.
//
// The table of an edit distance is walked row by row by ONE wave that holds the columns in registers, lane l the columns
// [l C, (l + 1) C) with C = ceil((m + 1) / 64).  The in-row dependency is a prefix minimum:
//   t[j] = min(prev[j] + 1, prev[j-1] + cost(i, j));   cur[j] = j + min_{k <= j} (t[k] - k)
// so a row of the table is a serial pass over the lane's C columns, one 6-step wave scan (shuffles) and a second pass: no
// LDS round trip.  The pivot-side labels come in tiles of 64 (one coalesced load) and are broadcast by readlane.
// Three launches, no host synchronisation:
//   mbr_pairs   block (0, job): validation, weights, status, the diagonal of dist.  Block (1 + p, job): pair p = (h, g),
//               h < g, validates its two rows itself and writes dist[h][g] and dist[g][h].
//   mbr_risk    one wave per job: risk, order, the pivot, header.
//   mbr_align   one workgroup of 16 waves per job, wave j the row j: the table of (y_P, y_j) again, a 2-bit direction per
//               cell evaluated forward by the contract's rule into the workspace (4 cells a byte, byte b of table row i
//               of lane l at ((i - 1) DB + b) 64 + l: a wave's store is 64 consecutive bytes), the walk back by lane 0
//               (slots, gap marks), a barrier, then the column pass over the slots, one thread per column.
// No atomics; one writer per output; plain vector stores; the inputs are only read.  A malformed job writes nothing: all
// three kernels evaluate the same predicate (mbr_ok) before anything else.
#include "common.h"

namespace {

constexpr int MB_H = SC_MBR_MAX_HYPS;
constexpr int MB_PAIRS = MB_H * (MB_H - 1) / 2;
constexpr int MB_CMAX = (SC_MBR_MAX_LEN + 1 + 63) / 64;   // columns a lane holds at most (17)
constexpr int MB_BIG = 1 << 28;

__host__ __device__ inline size_t mb_up(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ inline int mb_cap(int L, int skip) {
  const int c = L - skip;
  return c < 0 ? 0 : (c > SC_MBR_MAX_LEN ? SC_MBR_MAX_LEN : c);
}
// direction bytes per lane and table row for rows of at most m labels
__host__ __device__ inline int mb_db(int m) { return (((m + 1 + 63) / 64) + 3) / 4; }
// a job's share of the workspace: [dir: 16 rows][cap table rows][DB][64] | [slots: 16][cap] int32 | [gap marks: 16][cap + 1]
__host__ __device__ inline size_t mb_dir_row_bytes(int cap) { return mb_up((size_t)cap * mb_db(cap) * 64); }
__host__ __device__ inline size_t mb_job_bytes(int cap) {
  return MB_H * mb_dir_row_bytes(cap) + mb_up((size_t)MB_H * cap * sizeof(int32_t)) + mb_up((size_t)MB_H * (cap + 1));
}

__device__ __forceinline__ bool mb_finite(double x) { return fabs(x) < INFINITY; }   // false for a NaN
__device__ __forceinline__ double mb_qnan() { return __longlong_as_double(0x7FF8000000000000ll); }

// uniform over the launch's threads of a job
__device__ bool mbr_ok(const sc_mbr_job &j, size_t share) {
  if (!j.yseq || (j.score == nullptr) == (j.weight == nullptr) || !j.weight_out || !j.risk || !j.dist || !j.order ||
      !j.status || !j.header || !j.conf || !j.alt_mass || !j.gap_mass || !j.alt_tok)
    return false;
  if (j.n_hyp < 1 || j.n_hyp > MB_H || j.L < 0 || j.row_stride < j.L || (j.score && j.score_stride < 1) || j.skip < 0 ||
      j.strip < -1 || j.V < 1 || !mb_finite(j.scale) || j.scale < 0.0 || j.pivot < -1 || j.pivot >= j.n_hyp ||
      j.flags != 0 || j.reserved != 0)
    return false;
  const int cap = mb_cap(j.L, j.skip);
  if (j.slots && j.slot_stride < cap) return false;
  return share >= mb_job_bytes(cap);
}

// the labels of row h: y[0, m).  false: lens[h] is a bad one (m = 0)
__device__ __forceinline__ bool mb_row(const sc_mbr_job &j, int h, const int32_t *&y, int &m) {
  const int len = j.lens ? j.lens[h] : j.L;
  const int32_t *row = j.yseq + (size_t)h * (size_t)j.row_stride;
  y = row + j.skip;
  m = 0;
  if (len < 0 || len > j.L) return false;
  int e = len;
  if (e > j.skip && j.strip >= 0 && row[e - 1] == j.strip) --e;
  m = max(0, e - j.skip);
  return true;
}

// status bits of row h that put it out, and the value z it enters the weights with (its weight itself when weights are
// given); by a whole wave
__device__ int mb_row_status(const sc_mbr_job &j, int h, int lane, double &z) {
  const int32_t *y;
  int m;
  int st = mb_row(j, h, y, m) ? 0 : SC_MBR_BAD_TOKEN;
  bool mine = false;
  for (int t = lane; t < m; t += 64) {
    const int c = y[t];
    mine = mine || c < 0 || c >= j.V;
  }
  if (__ballot(mine) != 0) st |= SC_MBR_BAD_TOKEN;
  if (m > SC_MBR_MAX_LEN) st |= SC_MBR_TOO_LONG;
  if (j.weight) {
    z = j.weight[h];
    if (!mb_finite(z) || z < 0.0) st |= SC_MBR_NONFINITE;
  } else {
    const double s = j.score[(size_t)h * (size_t)j.score_stride];
    z = s == -INFINITY ? -INFINITY : __dmul_rn(j.scale, s);
    if (s != s || s == INFINITY || z != z || z == INFINITY) st |= SC_MBR_NONFINITE;
  }
  return st;
}

template <int CM>
__device__ __forceinline__ int mb_pick(const int (&v)[CM], int c) {   // v[c] without a dynamic register index
  int r = 0;
#pragma unroll
  for (int k = 0; k < CM; ++k) r = k == c ? v[k] : r;
  return r;
}

// The table of (a[0, ma), b[0, mb)) by one wave, CM >= C columns a lane.  DIR: the direction bits of the table rows
// 1 .. ma go to dir (layout above, DB bytes a lane and row).  Returns D[ma][mb] in every lane.
template <int CM, bool DIR>
__device__ int mb_table(const int32_t *a, int ma, const int32_t *b, int mb, int lane, uint8_t *dir, int DB) {
  const int C = (mb + 1 + 63) / 64;
  const int j0 = lane * C;
  int prev[CM], yb[CM], t[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    const int jj = j0 + c;
    const bool in = c < C && jj <= mb;
    prev[c] = in ? jj : MB_BIG;
    yb[c] = (in && jj >= 1) ? b[jj - 1] : -1;
  }
  int tile = 0;
  for (int i = 1; i <= ma; ++i) {
    if (((i - 1) & 63) == 0) tile = (i - 1 + lane) < ma ? a[i - 1 + lane] : -1;
    const int ai = __builtin_amdgcn_readlane(tile, (i - 1) & 63);
    int left = __shfl_up(mb_pick(prev, C - 1), 1);   // D[i-1][j0 - 1]
    const int left0 = left;
    int run = MB_BIG;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < C) {
        const int jj = j0 + c;
        int v;
        if (jj == 0) v = i;
        else if (jj > mb) v = MB_BIG;
        else v = min(prev[c] + 1, left + (yb[c] != ai ? 1 : 0));
        left = prev[c];
        run = min(run, v - jj);
        t[c] = run;   // min over the lane's columns up to c of t - column
      }
    }
    int scan = run;   // inclusive prefix minimum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(scan, d);
      if (lane >= d) scan = min(scan, o);
    }
    int carry = __shfl_up(scan, 1);
    if (lane == 0) carry = MB_BIG;
    uint32_t bits = 0;
    left = left0;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < C) {
        const int jj = j0 + c;
        const int cur = jj > mb ? MB_BIG : jj + min(carry, t[c]);
        if (DIR) {
          int code = 2;
          if (jj == 0) code = 1;
          else if (jj <= mb) {
            if (cur == left + (yb[c] != ai ? 1 : 0)) code = 0;
            else if (cur == prev[c] + 1) code = 1;
          }
          bits |= (uint32_t)code << ((c & 3) * 2);
          if ((c & 3) == 3 || c == C - 1) {
            dir[((size_t)(i - 1) * DB + (c >> 2)) * 64 + lane] = (uint8_t)bits;
            bits = 0;
          }
        }
        left = prev[c];
        prev[c] = cur;
      }
    }
  }
  return __shfl(mb_pick(prev, mb % C), mb / C);
}

template <bool DIR>
__device__ int mb_table_any(const int32_t *a, int ma, const int32_t *b, int mb, int lane, uint8_t *dir, int DB) {
  const int C = (mb + 1 + 63) / 64;   // wave-uniform
  if (C <= 1) return mb_table<1, DIR>(a, ma, b, mb, lane, dir, DB);
  if (C <= 2) return mb_table<2, DIR>(a, ma, b, mb, lane, dir, DB);
  if (C <= 4) return mb_table<4, DIR>(a, ma, b, mb, lane, dir, DB);
  if (C <= 8) return mb_table<8, DIR>(a, ma, b, mb, lane, dir, DB);
  return mb_table<MB_CMAX, DIR>(a, ma, b, mb, lane, dir, DB);
}

__global__ __launch_bounds__(64) void mbr_pairs_kernel(const sc_mbr_job *__restrict__ jobs, size_t share) {
  const sc_mbr_job j = jobs[blockIdx.y];
  if (!mbr_ok(j, share)) return;
  const int lane = threadIdx.x, n = j.n_hyp;
  if (blockIdx.x == 0) {
    __shared__ int s_st[MB_H];
    __shared__ double s_z[MB_H];
    for (int h = 0; h < n; ++h) {
      double z;
      const int st = mb_row_status(j, h, lane, z);
      if (lane == 0) { s_st[h] = st; s_z[h] = z; }
    }
    __syncthreads();
    if (lane == 0) {   // at most 16 values: one thread, the contract's order
      int n_in = 0;
      double M = -INFINITY;
      for (int h = 0; h < n; ++h)
        if (!s_st[h]) { ++n_in; M = fmax(M, s_z[h]); }
      const bool pivot_out = n_in == 0 || (j.pivot >= 0 && s_st[j.pivot] != 0);
      double e[MB_H], Z = 0.0;
      if (!j.weight) {
        for (int h = 0; h < n; ++h) {
          e[h] = 0.0;
          if (s_st[h]) continue;
          e[h] = M == -INFINITY ? 1.0 : exp(__dsub_rn(s_z[h], M));
          Z = __dadd_rn(Z, e[h]);
        }
        if (M == -INFINITY) Z = (double)n_in;
      }
      for (int h = 0; h < n; ++h) {
        const bool in = !s_st[h];
        j.weight_out[h] = !in ? 0.0 : (j.weight ? s_z[h] : __ddiv_rn(e[h], Z));
        j.status[h] = s_st[h] | (pivot_out ? SC_MBR_NO_PIVOT : 0);
        j.dist[h * MB_H + h] = in ? 0 : -1;
      }
    }
    return;
  }
  // pair p -> (h, g), h < g
  int p = blockIdx.x - 1, h = 0;
  while (p >= MB_H - 1 - h) { p -= MB_H - 1 - h; ++h; }
  const int g = h + 1 + p;
  if (g >= n) return;
  double z;
  const bool out = (mb_row_status(j, h, lane, z) | mb_row_status(j, g, lane, z)) != 0;
  int d = -1;
  if (!out) {
    const int32_t *ya, *yb;
    int ma, mb;
    mb_row(j, h, ya, ma);
    mb_row(j, g, yb, mb);
    d = mb_table_any<false>(ya, ma, yb, mb, lane, nullptr, 0);
  }
  if (lane == 0) {
    j.dist[h * MB_H + g] = d;
    j.dist[g * MB_H + h] = d;
  }
}

__global__ __launch_bounds__(64) void mbr_risk_kernel(const sc_mbr_job *__restrict__ jobs, size_t share) {
  __shared__ double s_risk[MB_H];
  __shared__ int s_out[MB_H];
  const sc_mbr_job j = jobs[blockIdx.x];
  if (!mbr_ok(j, share)) return;
  const int h = threadIdx.x, n = j.n_hyp;
  bool out = true;
  double r = mb_qnan();
  if (h < n) {
    out = j.dist[h * MB_H + h] < 0;
    if (!out) {
      r = 0.0;
      for (int k = 0; k < n; ++k) {
        const int d = j.dist[h * MB_H + k];
        if (d >= 0) r = __dadd_rn(r, __dmul_rn(j.weight_out[k], (double)d));
      }
    }
    j.risk[h] = r;
    s_risk[h] = r;
    s_out[h] = out ? 1 : 0;
  }
  __syncthreads();
  if (h < n) {
    int rank = 0;
    for (int g = 0; g < n; ++g) {
      if (g == h) continue;
      const bool out_g = s_out[g] != 0;
      const double r_g = s_risk[g];
      const bool ahead = out_g != out ? out : (out ? g < h : (r_g < r || (r_g == r && g < h)));
      rank += ahead ? 1 : 0;
    }
    j.order[rank] = h;
    int n_in = 0;
    for (int g = 0; g < n; ++g) n_in += s_out[g] ? 0 : 1;
    // the pivot: this row when it is first (or named) and in
    const bool named = j.pivot >= 0;
    if (n_in == 0 || (named && s_out[j.pivot])) {
      if (h == 0) { j.header[0] = -1; j.header[1] = 0; j.header[2] = n_in; j.header[3] = 0; }
    } else if (named ? h == j.pivot : rank == 0) {
      const int32_t *y;
      int m;
      mb_row(j, h, y, m);
      j.header[0] = h; j.header[1] = m; j.header[2] = n_in; j.header[3] = 0;
    }
  }
}

__global__ __launch_bounds__(MB_H * 64) void mbr_align_kernel(const sc_mbr_job *__restrict__ jobs, char *ws, size_t share) {
  const sc_mbr_job j = jobs[blockIdx.x];
  if (!mbr_ok(j, share)) return;
  const int P = j.header[0];
  if (P < 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = j.n_hyp;
  const int cap = mb_cap(j.L, j.skip);
  char *base = ws + (size_t)blockIdx.x * share;
  int32_t *ws_slots = (int32_t *)(base + MB_H * mb_dir_row_bytes(cap));
  uint8_t *ws_gap = (uint8_t *)ws_slots + mb_up((size_t)MB_H * cap * sizeof(int32_t));
  const int64_t sstride = j.slots ? j.slot_stride : (int64_t)cap;
  int32_t *slots = j.slots ? j.slots : ws_slots;
  const int32_t *yp;
  int mp;
  mb_row(j, P, yp, mp);

  if (wave < n) {   // (wave-uniform)
    const int r = wave;
    int32_t *srow = slots + (size_t)r * (size_t)sstride;
    uint8_t *grow = ws_gap + (size_t)r * (cap + 1);
    const bool in = j.dist[r * MB_H + r] == 0;
    for (int g = lane; g <= mp; g += 64) grow[g] = 0;
    if (!in) {
      for (int t = lane; t < mp; t += 64) srow[t] = -2;
    } else {
      const int32_t *y;
      int m;
      mb_row(j, r, y, m);
      uint8_t *dir = (uint8_t *)base + (size_t)r * mb_dir_row_bytes(cap);
      const int DB = mb_db(m), C = (m + 1 + 63) / 64;
      mb_table_any<true>(yp, mp, y, m, lane, dir, DB);
      // the direction bytes and the cleared gap marks of the other lanes have landed before lane 0 reads and writes there
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (lane == 0) {
        int i = mp, k = m;
        while (i > 0 || k > 0) {
          int code;
          if (i == 0) code = 2;
          else if (k == 0) code = 1;
          else {
            const int l = k / C, c = k - l * C;
            code = (dir[((size_t)(i - 1) * DB + (c >> 2)) * 64 + l] >> ((c & 3) * 2)) & 3;
          }
          if (code == 0) { srow[i - 1] = y[k - 1]; --i; --k; }
          else if (code == 1) { srow[i - 1] = -1; --i; }
          else { grow[i] = 1; --k; }
        }
      }
    }
  }
  __syncthreads();   // (also makes the waves' global stores visible within the workgroup)

  __shared__ double s_w[MB_H];
  __shared__ int s_in[MB_H];
  if (tid < MB_H) {
    const bool in = tid < n && j.dist[tid * MB_H + tid] == 0;
    s_in[tid] = in ? 1 : 0;
    s_w[tid] = in ? j.weight_out[tid] : 0.0;
  }
  __syncthreads();
  for (int t = tid; t <= mp; t += MB_H * 64) {
    double gm = 0.0;
    for (int r = 0; r < n; ++r)
      if (s_in[r] && ws_gap[(size_t)r * (cap + 1) + t]) gm = __dadd_rn(gm, s_w[r]);
    j.gap_mass[t] = gm;
    if (t == mp) break;
    const int own = yp[t];
    int sy[MB_H];   // the column; -3: the row is out (no symbol is below -1)
#pragma unroll
    for (int r = 0; r < MB_H; ++r) sy[r] = (r < n && s_in[r]) ? slots[(size_t)r * (size_t)sstride + t] : -3;
    double conf = 0.0, best_m = 0.0;
    int best = -2;
#pragma unroll
    for (int r = 0; r < MB_H; ++r) {
      const int sym = sy[r];
      if (sym == -3) continue;
      if (sym == own) { conf = __dadd_rn(conf, s_w[r]); continue; }
      bool first = true;
#pragma unroll
      for (int q = 0; q < r; ++q) first = first && sy[q] != sym;
      if (!first) continue;
      double m = 0.0;
#pragma unroll
      for (int q = r; q < MB_H; ++q)
        if (sy[q] == sym) m = __dadd_rn(m, s_w[q]);
      if (best == -2 || m > best_m || (m == best_m && sym < best)) { best = sym; best_m = m; }
    }
    j.conf[t] = conf;
    j.alt_tok[t] = best;
    j.alt_mass[t] = best_m;
  }
}

}  // namespace

extern "C" size_t sc_mbr_ws_bytes(int n_jobs, int max_len) {
  if (n_jobs < 0 || n_jobs > SC_MBR_MAX_JOBS || max_len < 0) return 0;
  return (size_t)n_jobs * mb_job_bytes(mb_cap(max_len, 0));
}

extern "C" int sc_mbr(const sc_mbr_job *jobs, int n_jobs, void *ws, size_t ws_bytes, void *stream) {
  SC_CHECK_ARG(n_jobs >= 0, "negative job count");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_MBR_MAX_JOBS, "more than SC_MBR_MAX_JOBS jobs");
  SC_CHECK_ARG(n_jobs == 0 || ws, "null workspace");
  if (n_jobs == 0) return SC_OK;
  const size_t share = (ws_bytes / (size_t)n_jobs) & ~(size_t)255;
  hipStream_t st = (hipStream_t)stream;
  mbr_pairs_kernel<<<dim3(1 + MB_PAIRS, n_jobs), 64, 0, st>>>(jobs, share);
  SC_CHECK_LAUNCH();
  mbr_risk_kernel<<<n_jobs, 64, 0, st>>>(jobs, share);
  SC_CHECK_LAUNCH();
  mbr_align_kernel<<<n_jobs, MB_H * 64, 0, st>>>(jobs, (char *)ws, share);
  SC_CHECK_LAUNCH();
  return SC_OK;
}
