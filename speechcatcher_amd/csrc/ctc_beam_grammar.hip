// Grammar-constrained CTC prefix beam search (sc_ctc_beam_grammar) and the grammar handle (sc_grammar_*): the beam of
// ctc_beam.hip with a deterministic automaton over token ids, carried per entry, that CHOOSES the candidates.
// tests/ctc_beam_grammar_ref.py is the contract, built on tests/ctc_beam_ref.py.
//
// One launch per call, one workgroup of GB_WAVES = 16 wave64 per job, the job's span [t0, t1) in tiles of GB_TILE frames:
//   row pass   the waves take the tile's rows in turn: the row pass of ctc_row.h in the batches of ctc_beam.hip (the same
//              bits of lse).  Per frame only the bad flag, lse and lp(blank) go to LDS: the candidates depend on the
//              entry's state and cannot come from here.
//   selection  per frame, wave w picks the candidates of entry w - unless an entry before it is in the same state, whose
//              list it then shares: its lanes stride over the out-arcs of g_w and gather x[arc_tok] from the table row;
//              C rounds of ctc_beam.hip's selection (a lane's best behind the previous winner, the wave butterfly that
//              prefers the lower index).  Tokens ascend within a state, so the lowest arc index is the lowest token, and
//              the winning arc's index gives `next` with no lookup.  A lane keeps its first GB_CACHE values in registers
//              (a state of up to 64 GB_CACHE = 1024 arcs: all of them), the rounds read the rest again.
//   beam pass  wave 0 steps the beam as in ctc_beam.hip; the items of entry i are its stay and the candidates of ITS
//              list, the stay's repeat term reads x[last] from the row, a new prefix takes the arc's next state.
// Two workgroup barriers per frame (entries -> selection -> beam step).  No atomics; every output has one writer; plain
// vector stores.  The table and the grammar are only read.
//
// lae, the entry constructors and the beam step are written here a second time and not shared with ctc_beam.hip through
// a header: that kernel's register allocation is sensitive to the shape of its source, so its file
// stays as it is.
#include <vector>

#include "ctc_row.h"
#include "grammar_blob.h"

namespace {

constexpr int GB_WAVES = 16;
constexpr int GB_UNROLL = 4;   // the batches of ctc_beam.hip's row pass: the same bits of lse
constexpr int GB_TILE = 256;   // frames whose (bad, lse, lp(blank)) the workgroup holds in LDS between the passes
constexpr int GB_MAX = SC_BEAM_MAX;
constexpr int GB_CACHE = 16;   // arc values a lane keeps in registers for the candidate rounds (a state of up to 1024 arcs: all)
constexpr int GB_SLOTS = GB_MAX * (GB_MAX + 1);   // item slots: (entry, stay or candidate k)
constexpr int GB_ITEMS = (GB_SLOTS + 63) / 64;    // items per lane

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

__device__ __forceinline__ sc_beam_entry empty_entry() {
  sc_beam_entry e;
  e.node = -1; e.last = -1; e.len = 0; e.parent = -1; e.pb = -INFINITY; e.pnb = -INFINITY;
  return e;
}

// the candidates of state g on one row, computed by one wave: their count (every lane returns it); lane 0 writes
// tok[0..count), nx[0..count), lp[0..count)
__device__ __forceinline__ int state_candidates(const sc_grammar_view &gv, int g, const float *__restrict__ row, double lse,
                                                int C, int lane, int *tok, int *nx, double *lp) {
  const int a0 = gv.arc_off[g], deg = gv.arc_off[g + 1] - a0;
  float xv[GB_CACHE];
#pragma unroll
  for (int k = 0; k < GB_CACHE; ++k) {
    const int a = lane + 64 * k;
    xv[k] = a < deg ? row[gv.arc_tok[a0 + a]] : -INFINITY;
  }
  // round r: the best arc behind (pv, pi), the winner of round r - 1, in the order (x descending, arc index ascending)
  float pv = INFINITY;
  int pi = -1, nc = 0;
  for (int r = 0; r < C; ++r) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    // a lane sees its arcs ascending, so "strictly greater" keeps the lowest index
#pragma unroll
    for (int k = 0; k < GB_CACHE; ++k) {
      const int a = lane + 64 * k;
      const float x = xv[k];
      if ((x < pv || (x == pv && a > pi)) && x > bv) { bv = x; bi = a; }
    }
    for (int a = lane + 64 * GB_CACHE; a < deg; a += 64) {
      const float x = row[gv.arc_tok[a0 + a]];
      if ((x < pv || (x == pv && a > pi)) && x > bv) { bv = x; bi = a; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) break;   // (wave-uniform) nothing finite is left
    if (lane == 0) {
      tok[r] = gv.arc_tok[a0 + bi];
      nx[r] = gv.arc_next[a0 + bi];
      lp[r] = (double)bv - lse;
    }
    pv = bv;
    pi = bi;
    nc = r + 1;
  }
  return nc;
}

__global__ __launch_bounds__(GB_WAVES * 64) void ctc_beam_grammar_kernel(const sc_ctc_beam_gr_job *__restrict__ jobs) {
  __shared__ double t_lse[GB_TILE], t_lpb[GB_TILE];
  __shared__ int t_bad[GB_TILE];
  __shared__ double c_lp[GB_MAX][GB_MAX];   // the candidate lists: list w belongs to entry w when c_src[w] == w
  __shared__ int c_tok[GB_MAX][GB_MAX], c_nx[GB_MAX][GB_MAX], c_n[GB_MAX], c_src[GB_MAX];
  __shared__ sc_beam_entry ent[2][GB_MAX];
  __shared__ int e_g[2][GB_MAX];            // beside ent[p][i]: the automaton's state after the prefix
  __shared__ int s_ne;                      // entries of ent[p]: what the selection of the next frame serves
  __shared__ double s_tot[GB_MAX], s_total2[GB_MAX], s_pb2[GB_MAX], s_pnb2[GB_MAX];
  __shared__ double it_tot[GB_SLOTS];
  __shared__ unsigned long long it_key[GB_SLOTS];
  __shared__ int mrg[GB_MAX * GB_MAX];
  const sc_ctc_beam_gr_job &jg = jobs[blockIdx.x];
  const sc_ctc_beam_job j = jg.beam;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (!ctc_job_ok(j) || !j.state || j.stride < j.V || j.capacity < 0 || (j.capacity > 0 && !j.nodes) || j.B < 1 ||
      j.B > GB_MAX || j.C < 1 || j.C > GB_MAX)
    return;   // (a malformed job writes nothing)
  sc_beam_gr_t *const gr_state = jg.gr_state, *const gr_state_after = jg.gr_state_after;
  if (!jg.grammar || !gr_state) return;
  const sc_grammar_view gv = *jg.grammar;
  if (gv.V != j.V || gv.blank != j.blank) return;
  int stored = 1;
  if (!j.restart) {
    stored = j.state->n_entries;   // (every thread reads it: the decision is uniform over the workgroup)
    if (stored < 0 || stored > GB_MAX) return;
    for (int k = 0; k < min(stored, j.B); ++k)
      if (gr_state->g[k] < 0 || gr_state->g[k] >= gv.n_states) return;
  }
  __syncthreads();   // every wave has read the stored state before wave 0 may rewrite it (an empty span has no other barrier)

  // the state: counters wave-uniform in wave 0's registers, the entries in ent[p], e_g[p]; every wave follows p
  int n = 0, n_bad = 0, n_nodes = 1, ne = min(stored, j.B), p = 0, f = 0;
  if (wave == 0) {
    if (!j.restart) {
      n = j.state->n_frames; n_bad = j.state->n_bad; n_nodes = j.state->n_nodes;
      if (lane < ne) { ent[0][lane] = j.state->e[lane]; e_g[0][lane] = gr_state->g[lane]; }
    } else {
      if (lane == 0) {
        sc_beam_entry e = empty_entry();
        e.node = 0; e.pb = 0.0;
        ent[0][0] = e;
        e_g[0][0] = gv.start_state;
        if (j.capacity > 0) {
          sc_beam_node r;
          r.parent = -1; r.token = -1; r.frame = -1; r.reserved = 0;
          j.nodes[0] = r;
        }
      }
    }
    if (lane == 0) s_ne = ne;
    for (int k = lane; k < GB_MAX * GB_MAX; k += 64) mrg[k] = 0;
  }
  for (int tb = j.t0; tb < j.t1; tb += GB_TILE) {
    const int nt = min(GB_TILE, j.t1 - tb);
    for (int i = wave; i < nt; i += GB_WAVES) {
      const float *row = j.table + (size_t)(tb + i) * (size_t)j.stride;
      const CtcRowLse rl = ctc_row_combine(ctc_row_pass<GB_UNROLL>(row, j.V, lane, [](const float (&)[GB_UNROLL], int, bool) {}));
      if (lane == 0) {
        t_bad[i] = rl.bad ? 1 : 0;
        t_lse[i] = rl.lse;
        t_lpb[i] = rl.bad ? 0.0 : (double)row[j.blank] - rl.lse;
      }
    }
    __syncthreads();   // the tile's rows are summed; (first tile) wave 0 has laid the state out
    for (int i = 0; i < nt; ++i) {
      if (t_bad[i]) {   // (uniform over the workgroup)
        ++n;
        ++n_bad;
        continue;
      }
      const float *row = j.table + (size_t)(tb + i) * (size_t)j.stride;
      const double lse = t_lse[i];
      // ---- selection: wave w serves entry w, unless an earlier entry is in the same state
      const int ne_all = s_ne;
      if (wave < ne_all) {
        const int g = e_g[p][wave];
        int src = wave;
        for (int k = wave - 1; k >= 0; --k)
          if (e_g[p][k] == g) src = k;
        int nc = 0;
        if (src == wave) nc = state_candidates(gv, g, row, lse, j.C, lane, c_tok[wave], c_nx[wave], c_lp[wave]);
        if (lane == 0) {
          c_src[wave] = src;
          c_n[wave] = nc;
        }
      }
      __syncthreads();   // the lists are written
      if (wave == 0) {
        ++f;
        const double lpb = t_lpb[i];
        // ---- the stay of entry `lane`, and the extension that merges into it
        sc_beam_entry me = empty_entry();
        double lpl = -INFINITY, tot = -INFINITY;
        if (lane < ne) {
          me = ent[p][lane];
          if (me.last >= 0 && me.last < j.V) lpl = (double)row[me.last] - lse;   // (a stored last outside the row: as -inf)
          tot = lae(me.pb, me.pnb);
          s_tot[lane] = tot;
        }
        wave_sync();
        if (lane < ne) {
          const double pb2 = tot + lpb;
          double pnb2 = me.last >= 0 ? me.pnb + lpl : -INFINITY;   // (lpl = -inf: -inf)
          if (me.parent >= 0) {
            for (int ii = 0; ii < ne; ++ii) {
              if (ent[p][ii].node == me.parent) {   // (node ids are unique in a beam: at most one)
                const int ls = c_src[ii], ln = c_n[ls];
                int kk = -1;
                for (int k = 0; k < ln; ++k)
                  if (c_tok[ls][k] == me.last) kk = k;
                if (kk >= 0) {
                  const double ext = (me.last == ent[p][ii].last ? ent[p][ii].pb : s_tot[ii]) + c_lp[ls][kk];
                  pnb2 = lae(pnb2, ext);
                  mrg[ii * GB_MAX + kk] = f;
                }
              }
            }
          }
          s_pb2[lane] = pb2;
          s_pnb2[lane] = pnb2;
          s_total2[lane] = lae(pb2, pnb2);
        }
        wave_sync();
        // ---- the items: slot s = entry * (C + 1) + (0: the stay, k: candidate k - 1 of the entry's list); total and tie
        // key (stay / new prefix, rank of the entry, token).  A slot without a candidate is an item at -inf.
        const int per = j.C + 1, M = ne * per;
        double my_t[GB_ITEMS];
        unsigned long long my_k[GB_ITEMS];
        int cnt[GB_ITEMS];
#pragma unroll
        for (int q = 0; q < GB_ITEMS; ++q) {
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
              const int ls = c_src[ii];
              if (k - 1 < c_n[ls]) {
                const int c = c_tok[ls][k - 1];
                if (mrg[ii * GB_MAX + k - 1] != f) my_t[q] = (c == ent[p][ii].last ? ent[p][ii].pb : s_tot[ii]) + c_lp[ls][k - 1];
                my_k[q] = ((unsigned long long)(GB_MAX + ii) << 32) | (unsigned)c;
              }
            }
            it_tot[s] = my_t[q];
            it_key[s] = my_k[q];
          }
        }
        wave_sync();
        // ---- rank = the items that precede it: total descending, then the key ascending
        for (int s2 = 0; s2 < M; ++s2) {
          const double t2 = it_tot[s2];
          const unsigned long long k2 = it_key[s2];
#pragma unroll
          for (int q = 0; q < GB_ITEMS; ++q) cnt[q] += (t2 > my_t[q] || (t2 == my_t[q] && k2 < my_k[q])) ? 1 : 0;
        }
        int finite = 0;
#pragma unroll
        for (int q = 0; q < GB_ITEMS; ++q) {
          const bool live = my_t[q] > -INFINITY;
          finite += __popcll(__ballot(live));
          if (live && cnt[q] < j.B) {
            const int s = lane + 64 * q, ii = s / per, k = s - ii * per;
            const sc_beam_entry src = ent[p][ii];
            sc_beam_entry e;
            int g2 = e_g[p][ii];
            if (k == 0) {
              e = src;
              e.pb = s_pb2[ii];
              e.pnb = s_pnb2[ii];
            } else {
              const int ls = c_src[ii];
              e.node = -1;   // numbered below
              e.last = c_tok[ls][k - 1];
              e.len = src.len + 1;
              e.parent = src.node;
              e.pb = -INFINITY;
              e.pnb = my_t[q];
              g2 = c_nx[ls][k - 1];
            }
            ent[p ^ 1][cnt[q]] = e;
            e_g[p ^ 1][cnt[q]] = g2;
          }
        }
        wave_sync();
        ne = min(j.B, finite);
        // ---- the new prefixes become nodes, in rank order
        const bool fresh = lane < ne && ent[p ^ 1][lane].node < 0;
        const unsigned long long mf = __ballot(fresh);
        if (fresh) {
          const int id = n_nodes + __popcll(mf & ((1ull << lane) - 1ull));
          ent[p ^ 1][lane].node = id;
          if (id >= 0 && id < j.capacity) {
            sc_beam_node r;
            r.parent = ent[p ^ 1][lane].parent; r.token = ent[p ^ 1][lane].last; r.frame = n; r.reserved = 0;
            j.nodes[id] = r;
          }
        }
        n_nodes += __popcll(mf);
        if (lane == 0) s_ne = ne;
      }
      ++n;
      p ^= 1;
      __syncthreads();   // the new entries are laid out; the lists are free
    }
    __syncthreads();   // the tile is free for the next row pass (its last frames may be bad rows: no barrier of their own)
  }
  __syncthreads();   // (an empty span: wave 0's layout of the state is behind no other barrier)
  if (wave == 0) {
    if (lane < GB_MAX) {
      const sc_beam_entry e = lane < ne ? ent[p][lane] : empty_entry();
      const int g = lane < ne ? e_g[p][lane] : 0;
      j.state->e[lane] = e;
      gr_state->g[lane] = g;
      if (j.state_after) j.state_after->e[lane] = e;
      if (gr_state_after) gr_state_after->g[lane] = g;
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

}  // namespace

extern "C" int sc_ctc_beam_grammar(const sc_ctc_beam_gr_job *jobs, int n_jobs, void *stream) {
  return ctc_launch_jobs(__func__, jobs, n_jobs, SC_BEAM_MAX_JOBS, "more than SC_BEAM_MAX_JOBS jobs",
                         [&] { ctc_beam_grammar_kernel<<<n_jobs, GB_WAVES * 64, 0, (hipStream_t)stream>>>(jobs); });
}

// the grammar on the device - the blob as it was compiled, and the view whose pointers lead into it - and a host copy of
// its arrays for the readers that walk it without a launch
struct sc_grammar {
  unsigned char *blob = nullptr;
  sc_grammar_view *view = nullptr;
  sc_grammar_view host{};   // (the same device pointers)
  std::vector<int32_t> arc_off, arc_tok, arc_next, accept;
  int uses = 0;
};

static void grammar_free(sc_grammar *g) {
  if (g->blob) (void)hipFree(g->blob);
  if (g->view) (void)hipFree(g->view);
  delete g;
}

extern "C" int sc_grammar_create(const void *blob, size_t bytes, sc_grammar **out) {
  SC_CHECK_ARG(out, "null out");
  *out = nullptr;
  grammar_blob::Layout L;
  const char *wrong = grammar_blob::validate(blob, bytes, &L);
  if (wrong) {
    sc_set_error("%s: not a sound grammar blob: %s", __func__, wrong);
    return SC_ERR_ARG;
  }
  sc_grammar *g = new sc_grammar();
  if (hipMalloc((void **)&g->blob, bytes) != hipSuccess || hipMalloc((void **)&g->view, sizeof(sc_grammar_view)) != hipSuccess) {
    sc_set_error("%s: out of device memory (%zu bytes)", __func__, bytes);
    grammar_free(g);
    return SC_ERR_LAUNCH;
  }
  const unsigned char *p = (const unsigned char *)blob;
  const size_t ns = (size_t)L.h.n_states, na = (size_t)L.h.n_arcs;
  auto copy = [&](std::vector<int32_t> &v, size_t off, size_t count) {
    v.resize(count);
    if (count) memcpy(v.data(), p + off, 4 * count);
  };
  copy(g->arc_off, L.arc_off, ns + 1);
  copy(g->arc_tok, L.arc_tok, na);
  copy(g->arc_next, L.arc_next, na);
  copy(g->accept, L.accept, ns);
  sc_grammar_view &v = g->host;
  v.arc_off = (const int32_t *)(g->blob + L.arc_off);
  v.arc_tok = (const int32_t *)(g->blob + L.arc_tok);
  v.arc_next = (const int32_t *)(g->blob + L.arc_next);
  v.accept = (const int32_t *)(g->blob + L.accept);
  v.V = L.h.V; v.blank = L.h.blank; v.n_states = L.h.n_states; v.n_arcs = L.h.n_arcs; v.start_state = L.h.start_state;
  v.reserved = 0;
  if (hipMemcpy(g->blob, blob, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(g->view, &v, sizeof v, hipMemcpyHostToDevice) != hipSuccess) {
    sc_set_error("%s: upload failed", __func__);
    grammar_free(g);
    return SC_ERR_LAUNCH;
  }
  *out = g;
  return SC_OK;
}

extern "C" int sc_grammar_destroy(sc_grammar *g) {
  if (!g) return SC_OK;
  SC_CHECK_ARG(g->uses == 0, "the grammar is still in use");
  grammar_free(g);
  return SC_OK;
}

extern "C" int sc_grammar_device_view(const sc_grammar *g, const sc_grammar_view **device, sc_grammar_view *host) {
  SC_CHECK_ARG(g, "null grammar");
  if (device) *device = g->view;
  if (host) *host = g->host;
  return SC_OK;
}

extern "C" int sc_grammar_use(sc_grammar *g, int delta) {
  SC_CHECK_ARG(g, "null grammar");
  SC_CHECK_ARG(g->uses + delta >= 0, "the use count would fall below 0");
  g->uses += delta;
  return g->uses;
}

extern "C" int sc_grammar_step(const sc_grammar *g, int state, int token) {
  if (!g || state < 0 || state >= g->host.n_states) return -1;
  int lo = g->arc_off[state], hi = g->arc_off[state + 1];
  while (lo < hi) {   // (tokens ascend within a state)
    const int mid = lo + (hi - lo) / 2;
    if (g->arc_tok[mid] < token) lo = mid + 1; else hi = mid;
  }
  return lo < g->arc_off[state + 1] && g->arc_tok[lo] == token ? g->arc_next[lo] : -1;
}

extern "C" int sc_grammar_accepts(const sc_grammar *g, int state) {
  if (!g || state < 0 || state >= g->host.n_states) return -1;
  return g->accept[state];
}
