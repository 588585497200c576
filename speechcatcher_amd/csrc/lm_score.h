// score() of the backoff automaton on the device (include/scasr.h, "n-gram language model"): ONE (state, token) lookup as
// a straight function, for code that walks token sequences (lm_rescore.hip).
//
// ctc_beam.hip does NOT use this header and keeps its own interleaved form of the same lookup: there every lane issues
// the first probes of all its items together, a shape fitted to that kernel's register budget (DESIGN.md 8k records how
// sensitive it is).  Both must give the bits of speechcatcher_amd/ngram.py's Blob.score; tests/test_gpu_lm_rescore.py and
// tests/test_gpu_ctc_beam_lm.py hold each to it.
//
// Relies on exactly what lm_blob.h validates: s in [0, n_states) stays there along bo_state and next; the slot index is
// masked, a probe run is capped at n_slots and the backoff levels at SC_LM_MAX_ORDER (a validated model needs fewer).
// The caller guarantees 0 <= c < V and 0 <= s < n_states.
#pragma once
#include "common.h"

__device__ __forceinline__ void lm_score(const sc_lm_view &lv, int s, int c, double &l, int &next) {
  const unsigned mask = (unsigned)lv.n_slots - 1u;
  double acc = 0.0;
  for (int lvl = 0; lvl < SC_LM_MAX_ORDER && s != 0; ++lvl) {
    const unsigned long long key = ((unsigned long long)(unsigned)s << 32) | (unsigned)c;
    unsigned at = (unsigned)((key * SC_LM_HASH_MUL) >> lv.shift) & mask;
    unsigned long long k = lv.slots[at].key;
    for (int n = 0; k != key && k != SC_LM_EMPTY && n < lv.n_slots; ++n) {
      at = (at + 1u) & mask;
      k = lv.slots[at].key;
    }
    if (k == key) {
      l = acc + lv.slots[at].logp;
      next = lv.slots[at].next;
      return;
    }
    acc = acc + lv.backoff[s];   // no arc: back off
    s = lv.bo_state[s];
  }
  l = acc + lv.root_logp[c];
  next = lv.root_next[c];
}

// the state after (s, c) alone
__device__ __forceinline__ int lm_advance(const sc_lm_view &lv, int s, int c) {
  double l;
  int next;
  lm_score(lv, s, c, l, next);
  return next;
}
