// CTC prefix beam search (sc_ctc_beam, sc_ctc_beam_pack): an n-best list of token prefixes with their CTC prefix
// probabilities from the rows of a CTC table, and the running beam of a stream over them.  tests/ctc_beam_ref.py is the
// contract.
//
// One launch per call, one workgroup of BM_WAVES = 16 wave64 per job, the job's span [t0, t1) in tiles of BM_TILE frames:
//   row pass   the waves take the tile's rows in turn: lse by the row pass of ctc_row.h, whose first batches also fill a
//              lane's cache.  The C candidates come in C rounds: every lane's best entry that lies BEHIND the previous
//              round's winner in the order (x descending, index ascending), the wave's best of those by a butterfly
//              whose merge prefers the lower index on equal values - exact in any order, ties included.  A lane keeps
//              its first BM_CACHE entries in registers (V <= 1024: the whole row), the rounds read the rest again.
//              Lane 0 writes the candidate ids, their lp and lp(blank) to LDS; BM_BAD for a bad row.
//   beam pass  wave 0 walks the tile frame by frame, the beam in LDS (two buffers).  Lane j holds entry j for the stay
//              and looks its parent up among the <= 16 entries: the extension that merges into it is added to its pnb'
//              and stamped in a (parent, candidate) table.  The lanes then hold the ne (nc + 1) items (entry, stay or
//              candidate), up to BM_ITEMS each: total and tie key to LDS, rank = the items that precede it, counted over
//              all items (broadcast reads).  The items of rank < B are written to the other buffer at their rank; a
//              __ballot over the new prefixes numbers their nodes, one lane each stores its record.
// No atomics; every output has one writer; plain vector stores.  The table is only read.
//
// sc_ctc_beam_lm is the same kernel body with an n-gram model fused in (template <bool LM>; DESIGN.md 8k,
// tests/ctc_beam_lm_ref.py): beside the entries the beam carries (lm, ctx) in LDS; the lanes that hold the extension
// items look their arcs up in the backoff automaton - one round per backoff level, the first probes of a lane's items
// issued together so that their loads overlap -, and the items are ranked by total + (alpha * lm + beta * len).  The
// LM = false instantiation is the kernel without any of it.  sc_lm_create validates a model on the host (lm_blob.h)
// and uploads it once.
//
// ctc_beam_grammar.hip (sc_ctc_beam_grammar) writes lae, the entry constructors and the beam step a second
// time instead of sharing them with this file through a header: the register allocation of ctc_beam_kernel follows the
// shape of its source (8j, 8k), and this file stays as it is.
#include "ctc_row.h"
#include "lm_blob.h"

namespace {

constexpr int BM_WAVES = 16;   // a group's jobs hold about 16 rows each: one row per wave (8 waves - 256 registers a lane,
                               // no spill in the beam pass, two rows per wave - measured 6 % slower: DESIGN.md 8j)
constexpr int BM_UNROLL = 4;
constexpr int BM_TILE = 256;   // frames whose candidates the workgroup holds in LDS between the two passes
constexpr int BM_MAX = SC_BEAM_MAX;
constexpr int BM_CACHE = 16;   // entries of a row a lane keeps in registers for the candidate rounds
constexpr int BM_ITEMS = (BM_MAX * (BM_MAX + 1) + 63) / 64;   // items per lane
constexpr int BM_BAD = -1;     // candidate count of a bad row

__device__ __forceinline__ void wave_sync() {   // LDS written by some lanes of the wave is read by others behind this
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double lae(double a, double b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const double hi = a >= b ? a : b, lo = a >= b ? b : a;
  return hi + log1p(exp(lo - hi));
}

// candidates of one row, computed by one wave: their count (every lane returns it; BM_BAD: a bad row); lane 0 writes
// ids[0..count), lp[0..count) and *lp_blank
__device__ __forceinline__ int row_candidates(const float *__restrict__ row, int V, int blank, int C, int lane, int *ids,
                                              double *lp, double *lp_blank) {
  CtcRowAcc a;
  float xv[BM_CACHE];
#pragma unroll
  for (int k = 0; k < BM_CACHE; ++k) xv[k] = -INFINITY;
  // the row pass of ctc_row.h; the first BM_CACHE / BM_UNROLL batches also fill the cache.  (One lambda for both call
  // sites: with the batch step written out at each the launch measured 3 % slower)
  auto batch = [&](int v0, float *keep) {
    ctc_row_batch<BM_UNROLL>(a, row, V, v0, [&](const float (&xf)[BM_UNROLL], int, bool) {
#pragma unroll
      for (int k = 0; k < BM_UNROLL; ++k)
        if (keep) keep[k] = v0 + 64 * k == blank ? -INFINITY : xf[k];   // (the blank is no candidate: -inf in the cache)
    });
  };
#pragma unroll
  for (int b = 0; b < BM_CACHE / BM_UNROLL; ++b)
    if (lane + 64 * BM_UNROLL * b < V) batch(lane + 64 * BM_UNROLL * b, xv + BM_UNROLL * b);
  for (int v0 = lane + 64 * BM_CACHE; v0 < V; v0 += 64 * BM_UNROLL) batch(v0, nullptr);
  const CtcRowLse rl = ctc_row_combine(a);
  if (rl.bad) return BM_BAD;   // (wave-uniform)
  const double lse = rl.lse;
  if (lane == 0) *lp_blank = (double)row[blank] - lse;
  // round r: the best entry behind (pv, pi), the winner of round r - 1, in the order (x descending, index ascending)
  float pv = INFINITY;
  int pi = -1, nc = 0;
  for (int r = 0; r < C; ++r) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    // a lane sees its v ascending, so "strictly greater" keeps the lowest index
#pragma unroll
    for (int k = 0; k < BM_CACHE; ++k) {
      const int v = lane + 64 * k;
      const float x = xv[k];
      if ((x < pv || (x == pv && v > pi)) && x > bv) { bv = x; bi = v; }
    }
    for (int v = lane + 64 * BM_CACHE; v < V; v += 64) {
      const float x = row[v];
      if (v != blank && (x < pv || (x == pv && v > pi)) && x > bv) { bv = x; bi = v; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) break;   // (wave-uniform) nothing finite is left
    if (lane == 0) {
      ids[r] = bi;
      lp[r] = (double)bv - lse;
    }
    pv = bv;
    pi = bi;
    nc = r + 1;
  }
  return nc;
}

__device__ __forceinline__ sc_beam_entry empty_entry() {
  sc_beam_entry e;
  e.node = -1; e.last = -1; e.len = 0; e.parent = -1; e.pb = -INFINITY; e.pnb = -INFINITY;
  return e;
}

template <bool LM> struct BeamJobOf { using type = sc_ctc_beam_job; };
template <> struct BeamJobOf<true> { using type = sc_ctc_beam_lm_job; };
__device__ __forceinline__ const sc_ctc_beam_job &beam_of(const sc_ctc_beam_job &j) { return j; }
__device__ __forceinline__ const sc_ctc_beam_job &beam_of(const sc_ctc_beam_lm_job &j) { return j.beam; }

template <bool LM>
__global__ __launch_bounds__(BM_WAVES * 64) void ctc_beam_kernel(const typename BeamJobOf<LM>::type *__restrict__ jobs) {
  __shared__ double clp[BM_TILE][BM_MAX];
  __shared__ int cid[BM_TILE][BM_MAX];
  __shared__ double blp[BM_TILE];
  __shared__ int cn[BM_TILE];
  __shared__ sc_beam_entry ent[2][BM_MAX];
  __shared__ double s_tot[BM_MAX], s_total2[BM_MAX], s_pb2[BM_MAX], s_pnb2[BM_MAX];
  __shared__ double it_tot[BM_MAX * (BM_MAX + 1)];
  __shared__ unsigned long long it_key[BM_MAX * (BM_MAX + 1)];
  __shared__ int mrg[BM_MAX * BM_MAX];
  __shared__ double e_lm[LM ? 2 : 1][LM ? BM_MAX : 1];   // (LM) beside ent[p][i]: the model's sum along the prefix ...
  __shared__ int e_ctx[LM ? 2 : 1][LM ? BM_MAX : 1];     // ... and the automaton's state after it
  const sc_ctc_beam_job j = beam_of(jobs[blockIdx.x]);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (!ctc_job_ok(j) || !j.state || j.stride < j.V || j.capacity < 0 || (j.capacity > 0 && !j.nodes) || j.B < 1 ||
      j.B > BM_MAX || j.C < 1 || j.C > BM_MAX)
    return;   // (a malformed job writes nothing)
  int stored = 1;
  if (!j.restart) {
    stored = j.state->n_entries;   // (every thread reads it: the decision is uniform over the workgroup)
    if (stored < 0 || stored > BM_MAX) return;
  }
  // (LM) the model's side of the job; fuse: a model is attached (uniform over the workgroup)
  sc_lm_view lv{};
  sc_beam_lm_t *lm_state = nullptr, *lm_state_after = nullptr;
  double alpha = 0.0, beta = 0.0;
  bool fuse = false;
  if constexpr (LM) {
    const sc_ctc_beam_lm_job &jl = jobs[blockIdx.x];
    if (jl.lm) {
      lv = *jl.lm;
      lm_state = jl.lm_state; lm_state_after = jl.lm_state_after; alpha = jl.alpha; beta = jl.beta;
      fuse = true;
      if (!lm_state || lv.V != j.V || !(fabs(alpha) < INFINITY) || !(fabs(beta) < INFINITY)) return;
      if (!j.restart)
        for (int k = 0; k < min(stored, j.B); ++k)
          if (lm_state->ctx[k] < 0 || lm_state->ctx[k] >= lv.n_states) return;
    }
  }
  __syncthreads();   // every wave has read the count before wave 0 may rewrite it (an empty span has no other barrier)

  // the state: counters wave-uniform in wave 0's registers, the entries in ent[p]
  int n = 0, n_bad = 0, n_nodes = 1, ne = min(stored, j.B), p = 0, f = 0;
  if (wave == 0) {
    if (!j.restart) {
      n = j.state->n_frames; n_bad = j.state->n_bad; n_nodes = j.state->n_nodes;
      if (lane < ne) ent[0][lane] = j.state->e[lane];
      if constexpr (LM)
        if (fuse && lane < ne) { e_lm[0][lane] = lm_state->lm[lane]; e_ctx[0][lane] = lm_state->ctx[lane]; }
    } else {
      if (lane == 0) {
        sc_beam_entry e = empty_entry();
        e.node = 0; e.pb = 0.0;
        ent[0][0] = e;
        if (j.capacity > 0) {
          sc_beam_node r;
          r.parent = -1; r.token = -1; r.frame = -1; r.reserved = 0;
          j.nodes[0] = r;
        }
        if constexpr (LM)
          if (fuse) { e_lm[0][0] = 0.0; e_ctx[0][0] = lv.start_state; }
      }
    }
    for (int k = lane; k < BM_MAX * BM_MAX; k += 64) mrg[k] = 0;
    wave_sync();
  }
  for (int tb = j.t0; tb < j.t1; tb += BM_TILE) {
    const int nt = min(BM_TILE, j.t1 - tb);
    for (int i = wave; i < nt; i += BM_WAVES) {
      const int c = row_candidates(j.table + (size_t)(tb + i) * (size_t)j.stride, j.V, j.blank, j.C, lane, cid[i], clp[i],
                                   &blp[i]);
      if (lane == 0) cn[i] = c;
    }
    __syncthreads();
    if (wave == 0) {
      for (int i = 0; i < nt; ++i, ++n) {
        const int nc = cn[i];
        if (nc == BM_BAD) {   // (wave-uniform)
          ++n_bad;
          continue;
        }
        ++f;
        const double lpb = blp[i];
        // ---- the stay of entry `lane`, and the extension that merges into it
        sc_beam_entry me = empty_entry();
        int kk = -1;
        double lpl = 0.0, tot = -INFINITY;
        if (lane < ne) {
          me = ent[p][lane];
          for (int k = 0; k < nc; ++k)
            if (cid[i][k] == me.last) kk = k;
          if (kk >= 0) lpl = clp[i][kk];
          tot = lae(me.pb, me.pnb);
          s_tot[lane] = tot;
        }
        wave_sync();
        if (lane < ne) {
          const double pb2 = tot + lpb;
          double pnb2 = kk >= 0 ? me.pnb + lpl : -INFINITY;
          if (kk >= 0 && me.parent >= 0) {
            for (int ii = 0; ii < ne; ++ii) {
              if (ent[p][ii].node == me.parent) {   // (node ids are unique in a beam: at most one)
                const double ext = (me.last == ent[p][ii].last ? ent[p][ii].pb : s_tot[ii]) + lpl;
                pnb2 = lae(pnb2, ext);
                mrg[ii * BM_MAX + kk] = f;
              }
            }
          }
          s_pb2[lane] = pb2;
          s_pnb2[lane] = pnb2;
          s_total2[lane] = lae(pb2, pnb2);
        }
        wave_sync();
        // ---- the items: total and tie key (stay / new prefix, rank of the entry, token)
        const int per = nc + 1, M = ne * per;
        double my_t[BM_ITEMS];
        unsigned long long my_k[BM_ITEMS];
        int cnt[BM_ITEMS];
        double my_raw[LM ? BM_ITEMS : 1], my_lm[LM ? BM_ITEMS : 1];   // (LM) the item's pure total, its lm and ctx
        int my_ctx[LM ? BM_ITEMS : 1];
#pragma unroll
        for (int q = 0; q < BM_ITEMS; ++q) {
          const int s = lane + 64 * q;
          my_t[q] = -INFINITY;
          my_k[q] = 0ull;
          cnt[q] = 0;
          if (s < M) {
            const int ii = s / per, k = s - ii * per;
            if (k == 0) {
              my_t[q] = s_total2[ii];
              my_k[q] = (unsigned long long)ii << 32;
            } else {
              const int c = cid[i][k - 1];
              if (mrg[ii * BM_MAX + k - 1] != f) my_t[q] = (c == ent[p][ii].last ? ent[p][ii].pb : s_tot[ii]) + clp[i][k - 1];
              my_k[q] = ((unsigned long long)(BM_MAX + ii) << 32) | (unsigned)c;
            }
            if (!LM || !fuse) it_tot[s] = my_t[q];
            it_key[s] = my_k[q];
          }
        }
        if constexpr (LM) {
#pragma unroll
          for (int q = 0; q < BM_ITEMS; ++q) my_raw[q] = my_t[q];
          if (fuse) {
            // ---- the arcs of the new prefixes: score(ctx of the entry, candidate), every item of the lane at once
            int st[BM_ITEMS], tk[BM_ITEMS], len[BM_ITEMS];
            double acc[BM_ITEMS];
            bool todo[BM_ITEMS];
#pragma unroll
            for (int q = 0; q < BM_ITEMS; ++q) {
              const int s = lane + 64 * q;
              st[q] = 0; tk[q] = 0; len[q] = 0; acc[q] = 0.0; todo[q] = false; my_lm[q] = 0.0; my_ctx[q] = 0;
              if (s < M) {
                const int ii = s / per, k = s - ii * per;
                my_lm[q] = e_lm[p][ii];
                my_ctx[q] = e_ctx[p][ii];
                len[q] = ent[p][ii].len + (k > 0 ? 1 : 0);
                if (k > 0 && my_raw[q] > -INFINITY) {
                  todo[q] = true;
                  st[q] = my_ctx[q];
                  tk[q] = cid[i][k - 1];
                }
              }
            }
            const unsigned mask = (unsigned)lv.n_slots - 1u;
            for (int lvl = 0; lvl < SC_LM_MAX_ORDER; ++lvl) {   // (a validated model backs off SC_LM_MAX_ORDER - 1 times at most)
              bool any = false;
#pragma unroll
              for (int q = 0; q < BM_ITEMS; ++q) any = any || todo[q];
              if (!__ballot(any)) break;   // (wave-uniform)
              unsigned long long key[BM_ITEMS];
              unsigned at[BM_ITEMS];
              sc_lm_slot sl[BM_ITEMS];
#pragma unroll
              for (int q = 0; q < BM_ITEMS; ++q) {   // the first probe of every item: independent loads
                key[q] = ((unsigned long long)(unsigned)st[q] << 32) | (unsigned)tk[q];
                at[q] = todo[q] && st[q] != 0 ? (unsigned)((key[q] * SC_LM_HASH_MUL) >> lv.shift) & mask : 0u;
                sl[q] = lv.slots[at[q]];
              }
#pragma unroll
              for (int q = 0; q < BM_ITEMS; ++q) {
                if (!todo[q]) continue;
                double l;
                int nx;
                if (st[q] == 0) {
                  l = acc[q] + lv.root_logp[tk[q]];
                  nx = lv.root_next[tk[q]];
                } else {
                  for (int n = 0; sl[q].key != key[q] && sl[q].key != SC_LM_EMPTY && n < lv.n_slots; ++n) {
                    at[q] = (at[q] + 1u) & mask;
                    sl[q] = lv.slots[at[q]];
                  }
                  if (sl[q].key != key[q]) {   // no arc: back off
                    acc[q] = acc[q] + lv.backoff[st[q]];
                    st[q] = lv.bo_state[st[q]];
                    continue;
                  }
                  l = acc[q] + sl[q].logp;
                  nx = sl[q].next;
                }
                my_lm[q] = my_lm[q] + l;
                my_ctx[q] = nx;
                todo[q] = false;
              }
            }
            // ---- fused = total + (alpha * lm + beta * len): every product and sum rounded on its own
#pragma unroll
            for (int q = 0; q < BM_ITEMS; ++q) {
              const int s = lane + 64 * q;
              if (s < M) {
                const double w = __dadd_rn(__dmul_rn(alpha, my_lm[q]), __dmul_rn(beta, (double)len[q]));
                my_t[q] = __dadd_rn(my_raw[q], w);
                it_tot[s] = my_t[q];
              }
            }
          }
        }
        wave_sync();
        // ---- rank = the items that precede it: total descending, then the key ascending
        for (int s2 = 0; s2 < M; ++s2) {
          const double t2 = it_tot[s2];
          const unsigned long long k2 = it_key[s2];
#pragma unroll
          for (int q = 0; q < BM_ITEMS; ++q) cnt[q] += (t2 > my_t[q] || (t2 == my_t[q] && k2 < my_k[q])) ? 1 : 0;
        }
        int finite = 0;
#pragma unroll
        for (int q = 0; q < BM_ITEMS; ++q) {
          const bool live = (LM ? my_raw[q] : my_t[q]) > -INFINITY;
          finite += __popcll(__ballot(live));
          if (live && cnt[q] < j.B) {
            const int s = lane + 64 * q, ii = s / per, k = s - ii * per;
            const sc_beam_entry src = ent[p][ii];
            sc_beam_entry e;
            if (k == 0) {
              e = src;
              e.pb = s_pb2[ii];
              e.pnb = s_pnb2[ii];
            } else {
              e.node = -1;   // numbered below
              e.last = cid[i][k - 1];
              e.len = src.len + 1;
              e.parent = src.node;
              e.pb = -INFINITY;
              e.pnb = LM ? my_raw[q] : my_t[q];
            }
            ent[p ^ 1][cnt[q]] = e;
            if constexpr (LM)
              if (fuse) { e_lm[p ^ 1][cnt[q]] = my_lm[q]; e_ctx[p ^ 1][cnt[q]] = my_ctx[q]; }
          }
        }
        wave_sync();
        ne = min(j.B, finite);
        p ^= 1;
        // ---- the new prefixes become nodes, in rank order
        const bool fresh = lane < ne && ent[p][lane].node < 0;
        const unsigned long long mf = __ballot(fresh);
        if (fresh) {
          const int id = n_nodes + __popcll(mf & ((1ull << lane) - 1ull));
          ent[p][lane].node = id;
          if (id < j.capacity) {
            sc_beam_node r;
            r.parent = ent[p][lane].parent; r.token = ent[p][lane].last; r.frame = n; r.reserved = 0;
            j.nodes[id] = r;
          }
        }
        n_nodes += __popcll(mf);
        wave_sync();
      }
    }
    __syncthreads();   // the tile is free for the next row pass
  }
  if (wave == 0) {
    if (lane < BM_MAX) {
      const sc_beam_entry e = lane < ne ? ent[p][lane] : empty_entry();
      j.state->e[lane] = e;
      if (j.state_after) j.state_after->e[lane] = e;
      if constexpr (LM)
        if (fuse) {
          const double l = lane < ne ? e_lm[p][lane] : 0.0;
          const int c = lane < ne ? e_ctx[p][lane] : 0;
          lm_state->lm[lane] = l; lm_state->ctx[lane] = c;
          if (lm_state_after) { lm_state_after->lm[lane] = l; lm_state_after->ctx[lane] = c; }
        }
    }
    if (lane == 0) {
      j.state->n_frames = n; j.state->n_bad = n_bad; j.state->n_nodes = n_nodes; j.state->n_entries = ne;
      if (j.state_after) {
        j.state_after->n_frames = n; j.state_after->n_bad = n_bad; j.state_after->n_nodes = n_nodes;
        j.state_after->n_entries = ne;
      }
    }
  }
}

constexpr int PK_THREADS = 64;

__global__ __launch_bounds__(PK_THREADS) void ctc_beam_pack_kernel(const sc_ctc_beam_pack_job *__restrict__ jobs, int n_jobs) {
  const int k = blockIdx.x * PK_THREADS + threadIdx.x;
  if (k >= n_jobs) return;
  const sc_ctc_beam_pack_job j = jobs[k];
  if (!j.state || !j.header || !j.scores || j.capacity < 0 || j.max_len < 0 || (j.max_len > 0 && (!j.ids || !j.frames)) ||
      (j.capacity > 0 && !j.nodes))
    return;
  const int ne = j.state->n_entries, nn = j.state->n_nodes;
  if (j.rank < 0 || j.rank >= ne || j.rank >= BM_MAX) {
    j.header[0] = -1; j.header[1] = SC_BEAM_PACK_NO_ENTRY; j.header[2] = -1; j.header[3] = -1;
    j.scores[0] = NAN; j.scores[1] = NAN;
    return;
  }
  const sc_beam_entry e = j.state->e[j.rank];
  const int stored = min(nn, j.capacity);
  int node = e.node, status = e.len > j.max_len ? SC_BEAM_PACK_TRUNCATED : SC_BEAM_PACK_OK;
  if (e.len < 0) status = SC_BEAM_PACK_BROKEN;
  for (int pos = e.len - 1; pos >= 0 && status != SC_BEAM_PACK_BROKEN; --pos) {
    if (node < 1 || node >= stored) {
      status = SC_BEAM_PACK_BROKEN;
      break;
    }
    const sc_beam_node r = j.nodes[node];
    if (pos < j.max_len) {
      j.ids[pos] = r.token;
      j.frames[pos] = r.frame;
    }
    node = r.parent;
  }
  if (status != SC_BEAM_PACK_BROKEN && node != 0) status = SC_BEAM_PACK_BROKEN;
  j.header[0] = status == SC_BEAM_PACK_BROKEN ? -1 : e.len;
  j.header[1] = status; j.header[2] = e.node; j.header[3] = e.last;
  j.scores[0] = e.pb; j.scores[1] = e.pnb;
}

}  // namespace

extern "C" int sc_ctc_beam(const sc_ctc_beam_job *jobs, int n_jobs, void *stream) {
  return ctc_launch_jobs(__func__, jobs, n_jobs, SC_BEAM_MAX_JOBS, "more than SC_BEAM_MAX_JOBS jobs",
                         [&] { ctc_beam_kernel<false><<<n_jobs, BM_WAVES * 64, 0, (hipStream_t)stream>>>(jobs); });
}

extern "C" int sc_ctc_beam_lm(const sc_ctc_beam_lm_job *jobs, int n_jobs, void *stream) {
  return ctc_launch_jobs(__func__, jobs, n_jobs, SC_BEAM_MAX_JOBS, "more than SC_BEAM_MAX_JOBS jobs",
                         [&] { ctc_beam_kernel<true><<<n_jobs, BM_WAVES * 64, 0, (hipStream_t)stream>>>(jobs); });
}

// the model on the device: the blob as it was packed, and the view whose pointers lead into it
struct sc_lm {
  unsigned char *blob = nullptr;
  sc_lm_view *view = nullptr;
  sc_lm_view host{};   // (the same device pointers)
};

extern "C" int sc_lm_create(const void *blob, size_t bytes, sc_lm **out) {
  SC_CHECK_ARG(out, "null out");
  *out = nullptr;
  lm_blob::Layout L;
  const char *wrong = lm_blob::validate(blob, bytes, &L);
  if (wrong) {
    sc_set_error("%s: not a sound language model blob: %s", __func__, wrong);
    return SC_ERR_ARG;
  }
  sc_lm *lm = new sc_lm();
  if (hipMalloc((void **)&lm->blob, bytes) != hipSuccess || hipMalloc((void **)&lm->view, sizeof(sc_lm_view)) != hipSuccess) {
    sc_set_error("%s: out of device memory (%zu bytes)", __func__, bytes);
    sc_lm_destroy(lm);
    return SC_ERR_LAUNCH;
  }
  sc_lm_view &v = lm->host;
  v.backoff = (const double *)(lm->blob + L.backoff);
  v.bo_state = (const int32_t *)(lm->blob + L.bo_state);
  v.root_logp = (const double *)(lm->blob + L.root_logp);
  v.root_next = (const int32_t *)(lm->blob + L.root_next);
  v.slots = (const sc_lm_slot *)(lm->blob + L.slots);
  v.V = L.h.V; v.order = L.h.order; v.n_states = L.h.n_states; v.n_slots = L.h.n_slots; v.start_state = L.h.start_state;
  v.shift = L.shift;
  if (hipMemcpy(lm->blob, blob, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(lm->view, &v, sizeof v, hipMemcpyHostToDevice) != hipSuccess) {
    sc_set_error("%s: upload failed", __func__);
    sc_lm_destroy(lm);
    return SC_ERR_LAUNCH;
  }
  *out = lm;
  return SC_OK;
}

extern "C" void sc_lm_destroy(sc_lm *lm) {
  if (!lm) return;
  if (lm->blob) (void)hipFree(lm->blob);
  if (lm->view) (void)hipFree(lm->view);
  delete lm;
}

extern "C" int sc_lm_device_view(const sc_lm *lm, const sc_lm_view **device, sc_lm_view *host) {
  SC_CHECK_ARG(lm, "null model");
  if (device) *device = lm->view;
  if (host) *host = lm->host;
  return SC_OK;
}

extern "C" int sc_ctc_beam_pack(const sc_ctc_beam_pack_job *jobs, int n_jobs, void *stream) {
  return ctc_launch_jobs(__func__, jobs, n_jobs, SC_BEAM_MAX_JOBS, "more than SC_BEAM_MAX_JOBS jobs", [&] {
    ctc_beam_pack_kernel<<<cdiv(n_jobs, PK_THREADS), PK_THREADS, 0, (hipStream_t)stream>>>(jobs, n_jobs);
  });
}
