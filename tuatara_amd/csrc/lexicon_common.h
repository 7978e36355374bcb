// What the lexicon's scorers share (lexicon.hip, lexicon_fuzzy.hip): the table's geometry, the total order, the per-thread sorted lists and the wave
// selection over them, and the bytes of a word's record.  Internal to those two files: everything lives in an unnamed namespace.
#pragma once
#include "common.h"

namespace ttr {

namespace {
constexpr int kPos = 26, kCls = 95, kStride = 96, kTile = 4;        // positions per crop, classes, floats per table row, crops per workgroup
constexpr int kTable = kPos * kStride;                               // floats per crop's table
constexpr int kNone = 0x7fffffff;                                    // the index of an empty list entry: it sorts behind every word
constexpr size_t kLexPartialCap = (size_t)32 << 20;                  // partial entries (8 bytes each) beyond which the chunk doubles

// the total order: logp descending, index ascending (an empty entry, -inf / kNone, sorts last; a kept score is never -inf or NaN)
__device__ __forceinline__ bool lex_before(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

// a sorted list of CAP entries in registers: insert (s, i) where it belongs, the last entry drops out
template <int CAP>
__device__ __forceinline__ void lex_insert(float (&ts)[CAP], int (&ti)[CAP], float s, int i) {
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    const bool b = lex_before(s, i, ts[j], ti[j]);
    const float os = ts[j]; const int oi = ti[j];
    ts[j] = b ? s : os; ti[j] = b ? i : oi;
    s = b ? os : s; i = b ? oi : i;
  }
}

// The M best of the union of a wave's 64 sorted lists, by the total order: lane j (j < M) returns the j-th in (out_s, out_i), every other lane and every
// slot past the union's size (-INFINITY, kNone).  M rounds of a wave arg-max over the lists' heads; the lane that held the winner drops it.  Indices are
// unique across the lists, so exactly one lane holds the winner.  The lists are consumed.
template <int CAP>
__device__ __forceinline__ void wave_select(float (&ts)[CAP], int (&ti)[CAP], int M, int lane, float& out_s, int& out_i) {
  out_s = -INFINITY; out_i = kNone;
  for (int j = 0; j < M; ++j) {                                      // (M is wave-uniform; nothing below is indexed by j)
    float bs = ts[0]; int bi = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o); const int oi = __shfl_xor(bi, o);
      if (lex_before(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    if (bi == kNone) break;                                          // (wave-uniform) nothing left: the remaining slots stay empty
    if (ti[0] == bi) {
#pragma unroll
      for (int k = 0; k + 1 < CAP; ++k) { ts[k] = ts[k + 1]; ti[k] = ti[k + 1]; }
      ts[CAP - 1] = -INFINITY; ti[CAP - 1] = kNone;
    }
    if (lane == j) { out_s = bs; out_i = bi; }
  }
}

__device__ __forceinline__ unsigned rec_byte(const uint4& a, const uint4& b, int k) {   // byte k of a 32-byte record (k is a compile-time constant where this is used)
  const unsigned w = k < 4 ? a.x : k < 8 ? a.y : k < 12 ? a.z : k < 16 ? a.w : k < 20 ? b.x : k < 24 ? b.y : k < 28 ? b.z : b.w;
  return (w >> (8 * (k & 3))) & 0xffu;
}
}  // namespace

}  // namespace ttr
