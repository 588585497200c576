// Validation of a language model blob (include/scasr.h, "n-gram language model") before any byte of it
// reaches the device: the kernel follows bo_state, next and the probe runs without a bound of its own beyond what is
// checked here.
//
// Plain C++17 and nothing of the engine or of HIP: tests/host/lm_blob_check.cpp drives this file alone with a host compiler.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/scasr.h"

namespace lm_blob {

// where the sections of a blob lie, in bytes from its start
struct Layout {
  sc_lm_header h{};
  size_t backoff = 0, bo_state = 0, root_logp = 0, root_next = 0, slots = 0, bytes = 0;
  int shift = 0;   // 64 - log2 n_slots
};

inline size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

inline uint64_t home(uint64_t key, int shift) { return (key * SC_LM_HASH_MUL) >> shift; }

// nullptr: the blob is sound and *out describes it; else what is wrong with it.  Reads nothing outside [blob, blob + bytes).
inline const char *validate(const void *blob, size_t bytes, Layout *out) {
  if (!blob) return "null blob";
  if (bytes < sizeof(sc_lm_header)) return "shorter than its header";
  const unsigned char *p = (const unsigned char *)blob;
  Layout L;
  memcpy(&L.h, p, sizeof L.h);
  const sc_lm_header &h = L.h;
  if (h.magic != SC_LM_MAGIC || h.version != SC_LM_VERSION) return "magic / version";
  if (h.V < 1 || h.order < 1 || h.order > SC_LM_MAX_ORDER || h.n_states < 1 || h.n_arcs < 0 || h.n_slots < 2 ||
      (h.n_slots & (h.n_slots - 1)) != 0)
    return "header: V, order, counts or a slot count that is no power of two >= 2";
  if (h.n_arcs >= h.n_slots) return "header: no unused slot";
  if (h.start_state < 0 || h.start_state >= h.n_states) return "header: start_state out of range";
  // (all counts are below 2^31: the sizes cannot overflow 64 bits)
  const size_t ns = (size_t)h.n_states, V = (size_t)h.V, nsl = (size_t)h.n_slots;
  L.backoff = sizeof(sc_lm_header);
  L.bo_state = L.backoff + 8 * ns;
  L.root_logp = L.bo_state + pad8(4 * ns);
  L.root_next = L.root_logp + 8 * V;
  L.slots = L.root_next + pad8(4 * V);
  L.bytes = L.slots + sizeof(sc_lm_slot) * nsl;
  if (L.bytes != bytes) return "size does not match the header";
  for (L.shift = 64; ((size_t)1 << (64 - L.shift)) < nsl;) --L.shift;
  auto f64 = [&](size_t off, size_t i) { double v; memcpy(&v, p + off + 8 * i, 8); return v; };
  auto i32 = [&](size_t off, size_t i) { int32_t v; memcpy(&v, p + off + 4 * i, 4); return v; };
  for (size_t s = 0; s < ns; ++s) {
    if (!std::isfinite(f64(L.backoff, s))) return "a backoff that is not finite";
    const int32_t b = i32(L.bo_state, s);
    if (b < 0 || b >= h.n_states) return "a bo_state out of range";
  }
  if (i32(L.bo_state, 0) != 0) return "bo_state of state 0";
  for (size_t s = 0; s < ns; ++s) {   // (a cycle never reaches 0)
    int32_t at = (int32_t)s;
    for (int k = 0; k < SC_LM_MAX_ORDER - 1 && at != 0; ++k) at = i32(L.bo_state, (size_t)at);
    if (at != 0) return "a bo_state chain that does not end at state 0 within SC_LM_MAX_ORDER - 1 steps";
  }
  for (size_t v = 0; v < V; ++v) {
    if (!std::isfinite(f64(L.root_logp, v))) return "a unigram logp that is not finite";
    const int32_t nx = i32(L.root_next, v);
    if (nx < 0 || nx >= h.n_states) return "a unigram next out of range";
  }
  std::vector<sc_lm_slot> sl(nsl);
  memcpy(sl.data(), p + L.slots, sizeof(sc_lm_slot) * nsl);
  size_t used = 0;
  for (size_t k = 0; k < nsl; ++k) {
    const sc_lm_slot &s = sl[k];
    if (s.key == SC_LM_EMPTY) continue;
    ++used;
    const uint64_t st = s.key >> 32, tok = s.key & 0xffffffffull;
    if (st < 1 || st >= ns || tok >= V) return "a key whose state or token is out of range";
    if (!std::isfinite(s.logp)) return "an arc logp that is not finite";
    if (s.next < 0 || s.next >= h.n_states) return "an arc next out of range";
    // the probe run from the key's home slot reaches this slot before an unused one and meets the key nowhere else
    size_t at = (size_t)home(s.key, L.shift);
    for (size_t n = 0; at != k; ++n, at = (at + 1) & (nsl - 1)) {
      if (n >= nsl || sl[at].key == SC_LM_EMPTY) return "a key that its probe run does not reach";
      if (sl[at].key == s.key) return "a key twice";
    }
  }
  if (used != (size_t)h.n_arcs) return "n_arcs does not count the used slots";
  // (used < n_slots: an unused slot exists, so every probe run ends; a duplicate behind the first copy of a key is
  // caught above, since the run from the home slot to the second copy passes the first)
  if (out) *out = L;
  return nullptr;
}

}  // namespace lm_blob
