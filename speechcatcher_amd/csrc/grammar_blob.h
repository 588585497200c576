// Validation of a grammar blob (include/scasr.h, "grammar-constrained CTC prefix beam") before any byte of
// it reaches the device: the kernel follows arc_off, arc_tok and arc_next without a bound of its own beyond what is
// checked here.
//
// Plain C++17 and nothing of the engine or of HIP: tests/host/grammar_blob_check.cpp drives this file alone with a host
// compiler.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/scasr.h"

namespace grammar_blob {

// where the sections of a blob lie, in bytes from its start
struct Layout {
  sc_grammar_header h{};
  size_t arc_off = 0, arc_tok = 0, arc_next = 0, accept = 0, bytes = 0;
};

inline size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

// nullptr: the blob is sound and *out describes it; else what is wrong with it.  Reads nothing outside [blob, blob + bytes).
inline const char *validate(const void *blob, size_t bytes, Layout *out) {
  if (!blob) return "null blob";
  if (bytes < sizeof(sc_grammar_header)) return "shorter than its header";
  const unsigned char *p = (const unsigned char *)blob;
  Layout L;
  memcpy(&L.h, p, sizeof L.h);
  const sc_grammar_header &h = L.h;
  if (h.magic != SC_GRAMMAR_MAGIC || h.version != SC_GRAMMAR_VERSION) return "magic / version";
  if (h.V < 1 || h.blank < 0 || h.blank >= h.V) return "header: V or a blank outside [0, V)";
  if (h.n_states < 1 || h.n_states > SC_GRAMMAR_MAX_STATES || h.n_arcs < 0 || h.n_arcs > SC_GRAMMAR_MAX_ARCS)
    return "header: state or arc count out of range";
  if (h.start_state < 0 || h.start_state >= h.n_states) return "header: start_state out of range";
  if (h.reserved != 0) return "header: reserved word not 0";
  // (the counts are bounded above: the sizes cannot overflow)
  const size_t ns = (size_t)h.n_states, na = (size_t)h.n_arcs;
  L.arc_off = sizeof(sc_grammar_header);
  L.arc_tok = L.arc_off + pad8(4 * (ns + 1));
  L.arc_next = L.arc_tok + pad8(4 * na);
  L.accept = L.arc_next + pad8(4 * na);
  L.bytes = L.accept + pad8(4 * ns);
  if (L.bytes != bytes) return "size does not match the header";
  auto i32 = [&](size_t off, size_t i) { int32_t v; memcpy(&v, p + off + 4 * i, 4); return v; };
  if (i32(L.arc_off, 0) != 0 || i32(L.arc_off, ns) != h.n_arcs) return "arc_off does not run from 0 to n_arcs";
  for (size_t s = 0; s < ns; ++s) {
    const int32_t a = i32(L.arc_off, s), b = i32(L.arc_off, s + 1);
    if (a < 0 || b < a || b > h.n_arcs) return "arc_off not monotone";
  }
  for (size_t s = 0; s < ns; ++s) {
    const int32_t a = i32(L.arc_off, s), b = i32(L.arc_off, s + 1);
    for (int32_t k = a; k < b; ++k) {
      const int32_t t = i32(L.arc_tok, (size_t)k);
      if (t < 0 || t >= h.V) return "an arc token out of range";
      if (t == h.blank) return "an arc labelled with the blank";
      if (k > a && t <= i32(L.arc_tok, (size_t)k - 1)) return "the tokens of a state not strictly ascending";
    }
    const int32_t f = i32(L.accept, s);
    if (f != 0 && f != 1) return "an accept flag that is neither 0 nor 1";
  }
  for (size_t k = 0; k < na; ++k) {
    const int32_t nx = i32(L.arc_next, k);
    if (nx < 0 || nx >= h.n_states) return "an arc next out of range";
  }
  if (out) *out = L;
  return nullptr;
}

}  // namespace grammar_blob
