// Attention rescoring of n-best lists: attention of whole token sequences (sc_seq_attention) and one
// teacher-forced pass of the attention decoder over the rows of n-best lists (sc_dec_rescore).  tests/dec_rescore_ref.py
// is the contract.
//
// seq_attention_kernel<DK, CAUSAL>: one wave per (sequence, head, tile of 16 queries).  The wave keeps its 16 x DK query
// tile in registers in the A-operand layout of v_mfma_f32_16x16x4_f32 and walks the keys in tiles of 16 from key 0:
//   stage   the tile's K and V rows through LDS, 16 bytes per lane; a row at or beyond the walk's end (Lk, or the end of
//           the query tile when causal) is not read: zeros are staged
//   S       = Q K^T, DK / 4 MFMAs; acc[j] of lane (r, kk) = q(row 4 kk + j) . k(key r)
//   softmax online, in the accumulator layout: a row's 16 scores sit in the 16 lanes of one lane group; a masked key is
//           SELECTED out of the maximum and gets the weight 0.0f, whatever its score's bits
//   O      += P V, P through LDS into the A-operand layout, 4 MFMAs per 16 output columns.  In the one tile of a causal
//           walk that holds masked keys with real rows (the diagonal tile: keys j > i that a LATER query of the tile
//           attends to) the product is formed on the VALU under the same select, so not even a NaN in such a row reaches
//           the queries before it.
// Tiles are fixed (query tile = i / 16, key tile = j / 16) and every sum of a row runs in one order, so the bits of an
// output row do not depend on Lq, on the other jobs or on the workgroup.  No atomics, one writer per output, plain stores.
//
// sc_dec_rescore packs the rows of all lists of a slab into one row table (list k, row h, position p at row
// row0[k] + h * (L_k + 1) + p; the positions behind a row's m_h + 1 are padding that is computed and never read) and runs
// the decoder's dense work over it with the library's launchers; what is per sequence - the lengths, the status, the
// job tables of the two attentions - is made ON THE DEVICE by dr_prep_kernel, because the lengths live there.
#include <algorithm>
#include <vector>

#include "ctc_row.h"

namespace {

typedef float drf32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void dr_wave_sync() {   // LDS written by some lanes of the wave is read by others behind this
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool dr_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <int DK, bool CAUSAL>
__global__ __launch_bounds__(64) void seq_attention_kernel(const sc_seq_attn_job *__restrict__ jobs, int max_Lq, int max_H) {
  constexpr int LK = DK + 1, LP = 17, NT = DK / 16, C4 = DK / 4;
  __shared__ float Ks[16 * LK];
  __shared__ __attribute__((aligned(16))) float Vs[16 * DK];
  __shared__ float Ps[16 * LP];
  const sc_seq_attn_job j = jobs[blockIdx.x];
  const int head = blockIdx.y, q0 = 16 * (int)blockIdx.z;
  // a malformed job writes nothing (the host-side entry point cannot see the device table); uniform over the workgroup
  if (!j.q || !j.k || !j.v || !j.o || !dr_aligned16(j.q) || !dr_aligned16(j.k) || !dr_aligned16(j.v) || j.Lq < 0 ||
      j.Lq > max_Lq || j.H < 1 || j.H > max_H || (j.causal != 0 && j.causal != 1) || (j.Lq > 0 && j.Lk < 1))
    return;
  const int64_t w = (int64_t)j.H * DK;
  if (j.q_stride < w || j.k_stride < w || j.v_stride < w || j.o_stride < w || ((j.q_stride | j.k_stride | j.v_stride) & 3))
    return;
  if ((j.causal != 0) != CAUSAL || head >= j.H || q0 >= j.Lq) return;

  const int lane = threadIdx.x, r = lane & 15, kk = lane >> 4;
  const int Lq = j.Lq, Lk = j.Lk;
  float qa[C4];   // A operand of S: row q0 + r, element 4 s + kk
  {
    const bool ok = q0 + r < Lq;
    const float *qrow = j.q + (int64_t)(ok ? q0 + r : 0) * j.q_stride + head * DK;
#pragma unroll
    for (int s = 0; s < C4; ++s) qa[s] = ok ? qrow[4 * s + kk] : 0.f;
  }
  drf32x4 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o[t] = drf32x4{0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) { m[jj] = -INFINITY; l[jj] = 0.f; }
  const float scale = sqrtf((float)DK);
  const int kend = CAUSAL ? min(Lk, q0 + 16) : Lk;   // keys at or beyond it are masked for every query of the tile

  for (int k0 = 0; k0 < kend; k0 += 16) {
    for (int e = lane; e < 16 * C4; e += 64) {
      const int row = e / C4, c4 = e % C4;
      float4 k4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = k4;
      if (k0 + row < kend) {
        k4 = reinterpret_cast<const float4 *>(j.k + (int64_t)(k0 + row) * j.k_stride + head * DK)[c4];
        v4 = reinterpret_cast<const float4 *>(j.v + (int64_t)(k0 + row) * j.v_stride + head * DK)[c4];
      }
      float *kd = Ks + row * LK + 4 * c4;
      kd[0] = k4.x; kd[1] = k4.y; kd[2] = k4.z; kd[3] = k4.w;
      reinterpret_cast<float4 *>(Vs)[row * C4 + c4] = v4;
    }
    dr_wave_sync();
    drf32x4 sacc = drf32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < C4; ++s) sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s], Ks[r * LK + 4 * s + kk], sacc, 0, 0, 0);
    // sacc[jj] = q(row q0 + 4 kk + jj) . k(key k0 + r)
    const int key = k0 + r;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int i = q0 + 4 * kk + jj;
      const bool masked = key >= Lk || (CAUSAL && key > i);
      const float sc = masked ? -INFINITY : sacc[jj] / scale;
      float tm = sc;
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) tm = fmaxf(tm, __shfl_xor(tm, x, 16));
      // key 0 is masked for no query and lies in the first tile: from there on the running maximum is a finite number
      // (or the NaN of a row whose own scores hold one)
      const float mn = fmaxf(m[jj], tm);
      const float alpha = m[jj] == -INFINITY ? 0.f : expf(m[jj] - mn);
      const float p = masked ? 0.f : expf(sc - mn);
      float ps = p;
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) ps += __shfl_xor(ps, x, 16);
      l[jj] = l[jj] * alpha + ps;
      m[jj] = mn;
#pragma unroll
      for (int t = 0; t < NT; ++t) o[t][jj] *= alpha;
      Ps[(4 * kk + jj) * LP + r] = p;
    }
    dr_wave_sync();
    if (CAUSAL && k0 == q0) {   // the diagonal tile (wave-uniform): keys j > i carry rows of later queries
      for (int k = 0; k < 16; ++k) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float v = Vs[k * DK + 16 * t + r];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const float pv = fmaf(Ps[(4 * kk + jj) * LP + k], v, o[t][jj]);
            o[t][jj] = k <= 4 * kk + jj ? pv : o[t][jj];
          }
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float a = Ps[r * LP + 4 * s + kk];
#pragma unroll
        for (int t = 0; t < NT; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Vs[(4 * s + kk) * DK + 16 * t + r], o[t], 0, 0, 0);
      }
    }
    dr_wave_sync();   // (the next tile overwrites the buffers)
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int i = q0 + 4 * kk + jj;
    if (i >= Lq) continue;
    float *orow = j.o + (int64_t)i * j.o_stride + head * DK;
#pragma unroll
    for (int t = 0; t < NT; ++t) orow[16 * t + r] = o[t][jj] / l[jj];
  }
}

template <int DK>
void seq_attention_launch(const sc_seq_attn_job *jobs, int n_jobs, int max_Lq, int max_H, int forms, hipStream_t st) {
  const dim3 grid((unsigned)n_jobs, (unsigned)max_H, (unsigned)cdiv(max_Lq, 16));
  if (forms & 1) seq_attention_kernel<DK, false><<<grid, 64, 0, st>>>(jobs, max_Lq, max_H);
  if (forms & 2) seq_attention_kernel<DK, true><<<grid, 64, 0, st>>>(jobs, max_Lq, max_H);
}

// ---- the glue of sc_dec_rescore ------------------------------------------------------------------------------------
struct DrModel {   // what the glue kernels read of the model
  const float *embed, *pe;
  int32_t V, d, H, n_layers, LCAP, sos, eos;
};
struct DrJob {   // a list of the slab: the caller's job and where its rows are
  sc_dec_rescore_job job;
  int32_t row0, enc0, seq0, pad;   // first packed token row, first packed encoder row, first sequence
};
struct DrSeq { int32_t job, h; };   // (index into the slab's DrJob table, row of the list)
struct DrBufs {
  const DrJob *jobs;
  const DrSeq *seqs;
  int32_t *seq_m, *seq_status;   // [n_seqs] labels of the row (0 for a row with a status), its SC_ATT_* bits so far
  sc_seq_attn_job *self_tab, *cross_tab;   // [n_seqs], [n_layers][n_seqs]
  float *x, *qkv, *q, *att, *epk, *ckv, *logits;
  double *tok;   // [rows]
  int64_t ckv_layer_stride;   // floats between the K|V rows of two layers
  int32_t n_seqs;
};

__device__ __forceinline__ bool dr_finite(double x) { return fabs(x) < INFINITY; }   // false for a NaN

// one wave per sequence: its length and status, and its jobs for the two attentions
__global__ __launch_bounds__(64) void dr_prep_kernel(DrBufs b, DrModel md) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const DrSeq sq = b.seqs[s];
  const DrJob &dj = b.jobs[sq.job];
  const sc_dec_rescore_job &j = dj.job;
  const int len = j.lens ? j.lens[sq.h] : j.L;
  int status = j.T == 0 ? SC_ATT_NO_FRAMES : 0;
  int m = 0;
  if (len < 0 || len > j.L) {
    status |= SC_ATT_BAD_TOKEN;
  } else {
    m = len;
    if (m + 1 > j.pe_rows || m + 1 > md.LCAP) status |= SC_ATT_TOO_LONG;
    const int32_t *y = j.yseq + (int64_t)sq.h * j.row_stride;
    bool mine = false;
    for (int t = lane; t < m; t += 64) {
      const int c = y[t];
      mine = mine || c < 0 || c >= md.V;
    }
    if (__ballot(mine) != 0) status |= SC_ATT_BAD_TOKEN;
  }
  if (status) m = 0;
  const int cap = j.L + 1, Lq = status ? 0 : m + 1;
  const int64_t row = dj.row0 + (int64_t)sq.h * cap;
  if (lane == 0) {
    b.seq_m[s] = m;
    b.seq_status[s] = status;
    sc_seq_attn_job a;
    a.q = b.qkv + row * 3 * md.d;
    a.k = a.q + md.d;
    a.v = a.q + 2 * md.d;
    a.o = b.att + row * md.d;
    a.q_stride = a.k_stride = a.v_stride = 3 * md.d;
    a.o_stride = md.d;
    a.Lq = Lq; a.Lk = Lq; a.H = md.H; a.causal = 1;
    b.self_tab[s] = a;
  }
  for (int li = lane; li < md.n_layers; li += 64) {
    sc_seq_attn_job a;
    a.q = b.q + row * md.d;
    a.k = b.ckv + li * b.ckv_layer_stride + (int64_t)dj.enc0 * 2 * md.d;
    a.v = a.k + md.d;
    a.o = b.att + row * md.d;
    a.q_stride = a.o_stride = md.d;
    a.k_stride = a.v_stride = 2 * md.d;
    a.Lq = Lq; a.Lk = j.T; a.H = md.H; a.causal = 0;
    b.cross_tab[(int64_t)li * b.n_seqs + s] = a;
  }
}

// grid (sequence, position): x = embed[tok] * sqrt(d) + pe[pos] (positional_encoding.py:51-75) for the positions of a
// row, zeros for the padding behind them
__global__ __launch_bounds__(64) void dr_embed_kernel(DrBufs b, DrModel md, float sq_d) {
  const int s = blockIdx.x, pos = blockIdx.y;
  const DrSeq sq = b.seqs[s];
  const DrJob &dj = b.jobs[sq.job];
  const int cap = dj.job.L + 1;
  if (pos >= cap) return;
  const int m = b.seq_m[s];
  const bool live = b.seq_status[s] == 0 && pos <= m;
  float *x = b.x + (dj.row0 + (int64_t)sq.h * cap + pos) * md.d;
  int tok = 0;
  if (live) tok = pos == 0 ? md.sos : dj.job.yseq[(int64_t)sq.h * dj.job.row_stride + pos - 1];
  for (int c = threadIdx.x; c < md.d; c += 64)
    x[c] = live ? md.embed[(int64_t)tok * md.d + c] * sq_d + md.pe[(int64_t)pos * md.d + c] : 0.f;
}

// grid (list, encoder row): the lists' encoder rows one behind the other, d floats each
__global__ __launch_bounds__(64) void dr_gather_enc_kernel(DrBufs b, DrModel md) {
  const DrJob &dj = b.jobs[blockIdx.x];
  const int t = blockIdx.y;
  if (t >= dj.job.T) return;
  const float4 *src = reinterpret_cast<const float4 *>(dj.job.E + (int64_t)t * dj.job.e_stride);
  float4 *dst = reinterpret_cast<float4 *>(b.epk + (int64_t)(dj.enc0 + t) * md.d);
  for (int c = threadIdx.x; c < md.d / 4; c += 64) dst[c] = src[c];
}

// grid (sequence, position), one wave: lse of the logits row in float64 (ctc_row.h), tok = logit[target] - lse
__global__ __launch_bounds__(64) void dr_pick_kernel(DrBufs b, DrModel md) {
  const int s = blockIdx.x, pos = blockIdx.y, lane = threadIdx.x;
  const DrSeq sq = b.seqs[s];
  const DrJob &dj = b.jobs[sq.job];
  const sc_dec_rescore_job &j = dj.job;
  const int cap = j.L + 1;
  if (pos >= cap) return;
  const int m = b.seq_m[s];
  const bool dead = b.seq_status[s] != 0;
  const int64_t row = dj.row0 + (int64_t)sq.h * cap + pos;
  double *out = j.tok_att ? j.tok_att + (int64_t)sq.h * j.tok_stride + pos : nullptr;
  if (dead) {   // (wave-uniform) every entry of the row is 0.0
    if (lane == 0) {
      b.tok[row] = 0.0;
      if (out) *out = 0.0;
    }
    return;
  }
  if (pos > m) return;
  const float *lg = b.logits + row * md.V;
  const CtcRowAcc acc = ctc_row_pass<4>(lg, md.V, lane, [](const float *, int, bool) {});
  const CtcRowLse rl = ctc_row_combine(acc);
  if (lane == 0) {
    const int target = pos < m ? j.yseq[(int64_t)sq.h * j.row_stride + pos] : md.eos;
    const double v = (double)lg[target] - rl.lse;
    b.tok[row] = v;
    if (out) *out = v;
  }
}

// one workgroup per list: att, fused, status, order (lm_rescore.hip's last stage)
__global__ __launch_bounds__(64) void dr_final_kernel(DrBufs b) {
  __shared__ double s_fused[SC_ATT_MAX_HYPS];
  __shared__ int s_status[SC_ATT_MAX_HYPS];
  const DrJob &dj = b.jobs[blockIdx.x];
  const sc_dec_rescore_job &j = dj.job;
  const int h = threadIdx.x, n = j.n_hyp;
  if (h < n) {
    const int s = dj.seq0 + h, m = b.seq_m[s];
    int status = b.seq_status[s];
    const double score = j.score[(int64_t)h * j.score_stride];
    double att = 0.0, fused = __longlong_as_double(0x7FF8000000000000ll);
    if (!status) {
      const double *tok = b.tok + dj.row0 + (int64_t)h * (j.L + 1);
      for (int t = 0; t <= m; ++t) att = att + tok[t];
      const double f = __dadd_rn(__dadd_rn(__dmul_rn(j.w_ctc, score), __dmul_rn(j.w_att, att)), __dmul_rn(j.beta, (double)m));
      if (f == f) fused = f;
      if (!dr_finite(f)) status |= SC_ATT_NONFINITE;
    }
    if (!dr_finite(score)) status |= SC_ATT_NONFINITE;
    j.att[h] = att;
    j.fused[h] = fused;
    j.status[h] = status;
    s_fused[h] = fused;
    s_status[h] = status;
  }
  __syncthreads();
  if (h < n) {
    const bool bad_h = s_status[h] != 0;
    const double f_h = s_fused[h];
    int rank = 0;
    for (int g = 0; g < n; ++g) {
      if (g == h) continue;
      const bool bad_g = s_status[g] != 0;
      const double f_g = s_fused[g];
      const bool ahead = bad_g != bad_h ? bad_h : (bad_h ? g < h : (f_g > f_h || (f_g == f_h && g < h)));
      rank += ahead ? 1 : 0;
    }
    j.order[rank] = h;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
size_t dr_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

bool dr_ffn_fused(const sc_search &md, void *stream) {
  bool packed = true;
  for (int li = 0; li < md.n_layers; ++li) packed = packed && md.layers[li].w1_p && md.layers[li].w2_p;
  return packed && sc_ffn_ln_supported(md.d, md.F) &&
         sc_workspace_bytes(stream) >= (size_t)(md.F / 128) * 80 * md.d * sizeof(float);   // (search.hip: the same test)
}

// the slab's buffers one behind the other; `base` NULL: only the size
struct DrLayout {
  size_t jobs, seqs, seq_m, seq_status, self_tab, cross_tab, x, xn, qkv, q, att, ffh, epk, ckv, logits, tok, total;
};
DrLayout dr_layout(const sc_search &md, long rows, long enc_rows, int n_seqs, int n_jobs, bool ffh) {
  DrLayout L{};
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += dr_up(bytes); return o; };
  const size_t R = (size_t)rows, d = (size_t)md.d;
  L.jobs = take((size_t)n_jobs * sizeof(DrJob));
  L.seqs = take((size_t)n_seqs * sizeof(DrSeq));
  L.seq_m = take((size_t)n_seqs * sizeof(int32_t));
  L.seq_status = take((size_t)n_seqs * sizeof(int32_t));
  L.self_tab = take((size_t)n_seqs * sizeof(sc_seq_attn_job));
  L.cross_tab = take((size_t)n_seqs * md.n_layers * sizeof(sc_seq_attn_job));
  L.x = take(R * d * sizeof(float));
  L.xn = take(R * d * sizeof(float));
  L.qkv = take(R * 3 * d * sizeof(float));
  L.q = take(R * d * sizeof(float));
  L.att = take(R * d * sizeof(float));
  L.ffh = take(ffh ? R * (size_t)md.F * sizeof(float) : 0);
  L.epk = take((size_t)enc_rows * d * sizeof(float));
  L.ckv = take((size_t)enc_rows * md.n_layers * 2 * d * sizeof(float));
  L.logits = take(R * (size_t)md.V * sizeof(float));
  L.tok = take(R * sizeof(double));
  L.total = at;
  return L;
}

int dr_check_model(const sc_search *model) {
  SC_CHECK_ARG(model, "null model");
  const sc_search &md = *model;
  SC_CHECK_ARG(md.d > 0 && md.d % 32 == 0 && md.H > 0 && md.d % md.H == 0, "d must be a multiple of 32 and of H");
  const int dk = md.d / md.H;
  SC_CHECK_ARG(dk == 16 || dk == 32 || dk == 64, "head dim must be 16, 32 or 64");
  SC_CHECK_ARG(md.V > 1 && md.V <= SC_MAX_VOCAB && md.F > 0 && md.F % 32 == 0 && md.n_layers > 0 && md.LCAP > 0,
               "bad model dimensions");
  SC_CHECK_ARG(md.sos >= 0 && md.sos < md.V && md.eos >= 0 && md.eos < md.V, "sos / eos outside the vocabulary");
  bool have = md.layers && md.embed && md.pe && md.dec_norm_g && md.dec_norm_b && md.out_w && md.out_b;
  for (int li = 0; have && li < md.n_layers; ++li) {
    const sc_dec_layer &w = md.layers[li];
    have = w.ln1_g && w.ln1_b && w.wqkv && w.bqkv && w.wo && w.bo && w.ln2_g && w.ln2_b && w.wq && w.bq && w.wo2 && w.bo2 &&
           w.ln3_g && w.ln3_b && w.w1 && w.b1 && w.w2 && w.b2;
  }
  if (!have) {
    sc_set_error("sc_dec_rescore: the fp32 decoder weights are not resident");
    return SC_ERR_UNSUPPORTED;
  }
  return SC_OK;
}

long dr_job_rows(const sc_dec_rescore_job &j) { return (long)j.n_hyp * (j.L + 1); }

// the launches of one slab: lists [k0, k1) of the call
int dr_run_slab(const sc_dec_rescore_job *jobs, int k0, int k1, const sc_search &md, char *ws, bool fused, hipStream_t st) {
  static thread_local std::vector<char> host;   // the slab's tables, uploaded in one copy
  const int nj = k1 - k0;
  long rows = 0, enc_rows = 0;
  int n_seqs = 0, max_cap = 0, max_T = 0;
  for (int k = k0; k < k1; ++k) {
    rows += dr_job_rows(jobs[k]);
    enc_rows += jobs[k].T;
    n_seqs += jobs[k].n_hyp;
    max_cap = std::max(max_cap, jobs[k].L + 1);
    max_T = std::max(max_T, jobs[k].T);
  }
  const DrLayout lay = dr_layout(md, rows, enc_rows, n_seqs, nj, !fused);
  host.resize(lay.seqs + dr_up((size_t)n_seqs * sizeof(DrSeq)));
  DrJob *hj = (DrJob *)(host.data() + lay.jobs);
  DrSeq *hs = (DrSeq *)(host.data() + lay.seqs);
  {
    long r = 0, e = 0;
    int s = 0;
    for (int k = k0; k < k1; ++k) {
      DrJob &dj = hj[k - k0];
      dj.job = jobs[k];
      dj.row0 = (int32_t)r; dj.enc0 = (int32_t)e; dj.seq0 = s; dj.pad = 0;
      for (int h = 0; h < jobs[k].n_hyp; ++h) hs[s++] = DrSeq{k - k0, h};
      r += dr_job_rows(jobs[k]);
      e += jobs[k].T;
    }
  }
  // (a copy from pageable memory has left the host buffer when the call returns)
  if (hipMemcpyAsync(ws, host.data(), host.size(), hipMemcpyHostToDevice, st) != hipSuccess) {
    sc_set_error("sc_dec_rescore: uploading the job tables failed");
    return SC_ERR_LAUNCH;
  }
  const int d = md.d, F = md.F, V = md.V, Ld = md.n_layers, dk = d / md.H, R = (int)rows, TT = (int)enc_rows;
  DrBufs b{};
  b.jobs = (const DrJob *)(ws + lay.jobs);
  b.seqs = (const DrSeq *)(ws + lay.seqs);
  b.seq_m = (int32_t *)(ws + lay.seq_m);
  b.seq_status = (int32_t *)(ws + lay.seq_status);
  b.self_tab = (sc_seq_attn_job *)(ws + lay.self_tab);
  b.cross_tab = (sc_seq_attn_job *)(ws + lay.cross_tab);
  b.x = (float *)(ws + lay.x);
  b.qkv = (float *)(ws + lay.qkv);
  b.q = (float *)(ws + lay.q);
  b.att = (float *)(ws + lay.att);
  b.epk = (float *)(ws + lay.epk);
  b.ckv = (float *)(ws + lay.ckv);
  b.logits = (float *)(ws + lay.logits);
  b.tok = (double *)(ws + lay.tok);
  b.ckv_layer_stride = (int64_t)TT * 2 * d;
  b.n_seqs = n_seqs;
  float *xn = (float *)(ws + lay.xn), *ffh = (float *)(ws + lay.ffh);
  const DrModel dm{md.embed, md.pe, V, d, md.H, Ld, md.LCAP, md.sos, md.eos};
  int rc;

  dr_prep_kernel<<<n_seqs, 64, 0, st>>>(b, dm);
  dr_embed_kernel<<<dim3((unsigned)n_seqs, (unsigned)max_cap), 64, 0, st>>>(b, dm, sqrtf((float)d));
  // the rows behind a sequence's last position are never written by an attention: they are padding, kept finite
  if (hipMemsetAsync(b.att, 0, (size_t)R * d * sizeof(float), st) != hipSuccess) {
    sc_set_error("sc_dec_rescore: clearing the workspace failed");
    return SC_ERR_LAUNCH;
  }
  if (TT > 0) {   // cross-attention K|V of every layer from the lists' encoder rows
    dr_gather_enc_kernel<<<dim3((unsigned)nj, (unsigned)max_T), 64, 0, st>>>(b, dm);
    const float *wkv = jobs[k0].wkv, *bkv = jobs[k0].bkv;
    if (!((2 * d) % 128 == 0 && Ld > 1 &&
          sc_gemm_colblocks(b.epk, nullptr, d, wkv, bkv, b.ckv, nullptr, 2 * d, TT, Ld * 2 * d, d, 2 * d, (long)b.ckv_layer_stride,
                            0, st) == SC_OK))
      for (int li = 0; li < Ld; ++li)   // (the same k chain per element: the same bits)
        SC_TRY(sc_gemm(b.epk, nullptr, d, wkv + (size_t)li * 2 * d * d, bkv + (size_t)li * 2 * d, b.ckv + li * b.ckv_layer_stride,
                       nullptr, 2 * d, TT, 2 * d, d, 0, 0, st));
  }
  SC_TRY(sc_layernorm(b.x, nullptr, d, xn, nullptr, d, R, d, md.layers[0].ln1_g, md.layers[0].ln1_b, md.ln_eps, st));
  for (int li = 0; li < Ld; ++li) {
    const sc_dec_layer &w = md.layers[li];
    const bool last = li + 1 == Ld;
    const float *ng = last ? md.dec_norm_g : md.layers[li + 1].ln1_g, *nb = last ? md.dec_norm_b : md.layers[li + 1].ln1_b;
    SC_TRY(sc_gemm(xn, nullptr, d, w.wqkv, w.bqkv, b.qkv, nullptr, 3 * d, R, 3 * d, d, 0, 0, st));
    SC_TRY(sc_seq_attention(b.self_tab, n_seqs, dk, max_cap, md.H, 2, st));
    SC_TRY(sc_gemm_ln(b.att, nullptr, d, w.wo, w.bo, b.x, nullptr, d, R, d, d, SC_GEMM_RESIDUAL, 0, w.ln2_g, w.ln2_b, md.ln_eps,
                      xn, d, st));
    SC_TRY(sc_gemm(xn, nullptr, d, w.wq, w.bq, b.q, nullptr, d, R, d, d, 0, 0, st));
    if (TT > 0) SC_TRY(sc_seq_attention(b.cross_tab + (size_t)li * n_seqs, n_seqs, dk, max_cap, md.H, 1, st));
    SC_TRY(sc_gemm_ln(b.att, nullptr, d, w.wo2, w.bo2, b.x, nullptr, d, R, d, d, SC_GEMM_RESIDUAL, 0, w.ln3_g, w.ln3_b, md.ln_eps,
                      xn, d, st));
    if (fused) {
      SC_TRY(sc_ffn_ln(xn, nullptr, R, d, F, w.w1_p, w.b1, w.w2_p, w.b2, b.x, ng, nb, md.ln_eps, xn, st));
    } else {
      SC_TRY(sc_gemm(xn, nullptr, d, w.w1, w.b1, ffh, nullptr, F, R, F, d, SC_GEMM_RELU, 0, st));
      SC_TRY(sc_gemm_ln(ffh, nullptr, F, w.w2, w.b2, b.x, nullptr, d, R, d, F, SC_GEMM_RESIDUAL, 0, ng, nb, md.ln_eps, xn, d, st));
    }
  }
  SC_TRY(sc_gemm(xn, nullptr, d, md.out_w, md.out_b, b.logits, nullptr, V, R, V, d, 0, 0, st));
  dr_pick_kernel<<<dim3((unsigned)n_seqs, (unsigned)max_cap), 64, 0, st>>>(b, dm);
  dr_final_kernel<<<nj, 64, 0, st>>>(b);
  SC_CHECK_LAUNCH();
  return SC_OK;
}

}  // namespace

extern "C" int sc_seq_attention(const sc_seq_attn_job *jobs, int n_jobs, int dk, int max_Lq, int max_H, int forms,
                                void *stream) {
  SC_CHECK_ARG(n_jobs >= 0, "negative job count");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_SEQ_ATTN_MAX_JOBS, "more than SC_SEQ_ATTN_MAX_JOBS jobs");
  SC_CHECK_ARG(dk == 16 || dk == 32 || dk == 64, "head dim must be 16, 32 or 64");
  SC_CHECK_ARG(max_Lq >= 0 && max_Lq <= 16 * 65535 && max_H >= 1 && max_H <= 65535, "max_Lq or max_H out of range");
  SC_CHECK_ARG(forms >= 1 && forms <= 3, "forms must be 1, 2 or 3");
  if (n_jobs == 0 || max_Lq == 0) return SC_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dk == 16) seq_attention_launch<16>(jobs, n_jobs, max_Lq, max_H, forms, st);
  else if (dk == 32) seq_attention_launch<32>(jobs, n_jobs, max_Lq, max_H, forms, st);
  else seq_attention_launch<64>(jobs, n_jobs, max_Lq, max_H, forms, st);
  SC_CHECK_LAUNCH();
  return SC_OK;
}

extern "C" size_t sc_dec_rescore_ws_bytes(const sc_search *model, long rows, long enc_rows, int n_seqs, int n_jobs) {
  if (dr_check_model(model) != SC_OK || rows < 0 || enc_rows < 0 || n_seqs < 0 || n_jobs < 0) return 0;
  // (the hidden rows of the two-GEMM feed-forward are counted only where sc_ffn_ln does not cover the model)
  return dr_layout(*model, rows, enc_rows, n_seqs, n_jobs, !sc_ffn_ln_supported(model->d, model->F)).total;
}

extern "C" int sc_dec_rescore(const sc_dec_rescore_job *jobs, int n_jobs, const sc_search *model, void *ws, size_t ws_bytes,
                              void *stream) {
  SC_CHECK_ARG(n_jobs >= 0, "negative job count");
  SC_CHECK_ARG(n_jobs == 0 || jobs, "null job table");
  SC_CHECK_ARG(n_jobs <= SC_ATT_MAX_JOBS, "more than SC_ATT_MAX_JOBS jobs");
  int rc;
  SC_TRY(dr_check_model(model));
  if (n_jobs == 0) return SC_OK;
  SC_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0, "the workspace must be 256-byte aligned");
  const sc_search &md = *model;
  for (int k = 0; k < n_jobs; ++k) {
    const sc_dec_rescore_job &j = jobs[k];
    SC_CHECK_ARG(j.yseq && j.score && j.wkv && j.bkv && j.att && j.fused && j.order && j.status, "a job with a null pointer");
    SC_CHECK_ARG(j.n_hyp >= 1 && j.n_hyp <= SC_ATT_MAX_HYPS, "n_hyp outside [1, SC_ATT_MAX_HYPS]");
    SC_CHECK_ARG(j.L >= 0 && j.L < 65535 && j.T >= 0 && j.T <= 65535 && j.pe_rows >= 1, "L, T or pe_rows out of range");
    SC_CHECK_ARG(j.T == 0 || (j.E && ((uintptr_t)j.E & 15) == 0 && j.e_stride >= md.d && j.e_stride % 4 == 0),
                 "encoder rows: null, misaligned or a bad stride");
    SC_CHECK_ARG(j.row_stride >= j.L && j.score_stride >= 1 && (!j.tok_att || j.tok_stride >= j.L + 1), "a stride below its size");
    SC_CHECK_ARG(fabs(j.w_att) < INFINITY && fabs(j.w_ctc) < INFINITY && fabs(j.beta) < INFINITY, "a weight that is not finite");
    SC_CHECK_ARG(j.wkv == jobs[0].wkv && j.bkv == jobs[0].bkv, "wkv / bkv differ between the jobs of a call");
    SC_CHECK_ARG(((uintptr_t)j.wkv & 15) == 0 && ((uintptr_t)j.bkv & 15) == 0, "wkv / bkv misaligned");
  }
  // which feed-forward runs is a property of the model and of the stream's split-K workspace, never of the rows in flight
  const bool fused = dr_ffn_fused(md, stream);
  std::vector<int> cut{0};   // slabs of whole jobs, as many as fit
  {
    long rows = 0, enc_rows = 0;
    int n_seqs = 0;
    for (int k = 0; k < n_jobs; ++k) {
      const long r = dr_job_rows(jobs[k]);
      if (dr_layout(md, rows + r, enc_rows + jobs[k].T, n_seqs + jobs[k].n_hyp, k + 1 - cut.back(), !fused).total > ws_bytes ||
          rows + r > (1l << 30) / std::max(md.V, 3 * md.d)) {   // (row and element indices stay below 2^31)
        if (cut.back() == k) {
          sc_set_error("sc_dec_rescore: job %d alone needs %zu bytes of workspace, %zu given", k,
                       dr_layout(md, r, jobs[k].T, jobs[k].n_hyp, 1, !fused).total, ws_bytes);
          return SC_ERR_CAPACITY;
        }
        cut.push_back(k);
        rows = enc_rows = 0;
        n_seqs = 0;
        --k;   // the job opens the next slab
        continue;
      }
      rows += r; enc_rows += jobs[k].T; n_seqs += jobs[k].n_hyp;
    }
    cut.push_back(n_jobs);
  }
  for (size_t c = 0; c + 1 < cut.size(); ++c) SC_TRY(dr_run_slab(jobs, cut[c], cut[c + 1], md, (char *)ws, fused, (hipStream_t)stream));
  return SC_OK;
}
