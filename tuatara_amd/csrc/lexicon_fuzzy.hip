// Fuzzy alignment of lexicon entries (DESIGN.md "Lexicon matching", Fuzzy alignment): lexicon.hip's scorer with the look-up of character j at position j
// replaced by a banded alignment, so that an entry still matches a reading in which a character was dropped or doubled.
//
//   lp[p][c]   the lexicon's table, unchanged: (x[p][c] - x[p][id[p]]) + logf(prob[p]) for an allowed class c, -inf for a blocked one; fp32
//   band B     0..3, gap g fp32, finite, <= 0: the log-probability charged for one dropped or one extra character
//   D[j][p]    "j characters of the entry and p positions of the reading consumed": exists for 0 <= j <= L, 0 <= p <= 25, |j - p| <= B; a pair (score, edits)
//              D[0][0] = (0.0f, 0), every other cell starts at (-inf, 0); a candidate replaces the cell's value iff cand.score > cur.score, or
//              cand.score == cur.score and cand.edits < cur.edits (comparisons with NaN are false: a NaN is never taken up and never spreads)
//              candidates, each only from a cell that exists:   match    (D[j-1][p-1].score + lp[p-1][w[j-1]], edits)
//                                                               extra    (D[j][p-1].score + g, edits + 1)      position p-1 of the reading skipped
//                                                               dropped  (D[j-1][p].score + g, edits + 1)      entry character j-1 skipped
//   the end    over the cells D[L][p] that exist, the candidates (D[L][p].score + lp[p][0], edits) under the same rule from (-inf, 0): logp(w), edits(w)
//
// Every operation is one fp32 addition or one comparison: nothing can be contracted, the order of the additions along a path is the path's own, and the
// result is a function of (table, entry, B, g) alone - not of chunks, tiles, threads or arrival order, like the rigid scorer's.  Two candidates of equal score
// carry the same score on, so the scores do not depend on the edits at all: the scorer runs on scores alone, and the edits of the few winners are found by a
// second small kernel that repeats the rule with pairs.  At B = 0 the only path is the diagonal and logp is the rigid scorer's value bit for bit.
//
// How the rule is walked (fuzzy_dp): one row of W = 2B + 1 cells, row[k] = D[j][j + k - B], in registers.  Step j = 1..26 reads the W match terms
// m[k] = row[k] + lp[j - 1 + k - B][w[j-1]] (the same offset k: a match keeps j - p), then forms row j from m (match), its own left neighbour (extra) and the
// old row's right neighbour (dropped).  A record's bytes behind the word are zero, the EOS class: at step j = L + 1 the match terms ARE the end's candidates
// D[L][p] + lp[p][0], so the end costs no read of its own and is taken under j == L + 1; lanes whose word has ended keep their row by a select (j <= L), not
// by a branch.  j is unrolled and B is a template parameter: every register index and every LDS row offset is a compile-time constant, the address is
// constant + 4 * class as in the rigid loop, cells outside 0..25 are dropped at compile time, and no register array is indexed by a run-time value.
//
// lexicon_fuzzy_score_kernel<CAP, B>: the rigid scorer's geometry - 256 threads, a tile of 4 crops and a chunk of words per workgroup, the same 26 x 96
// tables in LDS (lex_tile_tables, shared with lexicon_tables_kernel, the dump the tests read), one word per thread held in registers from two 16-byte loads,
// the same per-thread lists, wave selection, partial layout and merge (lexicon_common.h, launch_lexicon_merge).  The alignment runs one crop at a time, so
// its row is not held four times.  LDS reads per (word, crop): (2B + 1) * 26 less the cells outside 0..25 - 26, 76, 124, 170 for B = 0..3 - against the
// rigid scorer's 26; the expectation that the cost grows roughly with 2B + 1 is an estimate from this count (profiles/lexicon_fuzzy.md holds what was measured).
// The bank-conflict analysis of lexicon.hip holds read for read: lanes hold different words of one crop.
// lexicon_fuzzy_edits_kernel<B>: one thread per (crop, slot) behind the merge, at most N * 8; the pair rule for the winner, the table's entries formed
// straight from global memory by the same lex_lp.
//
// Compiler report (hipcc of ROCm 7.2, -O3, gfx950; scratch 0 in every instantiation; LDS 40,960 bytes a workgroup, which allows 4 workgroups per CU):
//   VGPRs of lexicon_fuzzy_score_kernel<CAP, B>    B = 0   B = 1   B = 2   B = 3     waves per SIMD by registers
//                                      CAP = 1       77     103     106     112      4
//                                      CAP = 2       85     111     114     120      4
//                                      CAP = 4      101     127     123     128      4
//                                      CAP = 8      138     160     162     168      3 (one workgroup per CU fewer than the LDS allows)
//   lexicon_fuzzy_edits_kernel<B>: 4 / 132 / 142 / 152 VGPRs for B = 0..3 (at B = 0 every edit count is 0 and the rule folds away), scratch 0; for B >= 1
//   the compiler keeps each lane's row mask in 3,072 bytes of LDS.  lexicon_tables_kernel: 50 VGPRs, LDS 40,768 bytes, scratch 0.
#include "common.h"
#include "kernels.h"
#include "lexicon_common.h"

namespace ttr {

namespace {
// ---- the table: the two expressions of the rule, restated once for the scorer, the dump and the edits kernel
// one entry from its row's constants: xid = x[p][id[p]], lprob = logf(prob[p])
__device__ __forceinline__ float lex_lp(float x, float xid, float lprob, bool allowed) { return allowed ? (x - xid) + lprob : -INFINITY; }

// a row's constants; r = crop * 26 + position
__device__ __forceinline__ void lex_row_consts(const float* __restrict__ logits, const int* __restrict__ ids, const float* __restrict__ prob, int r, float& xid,
                                               float& lprob) {
  const int id = min(max(ids[r], 0), kCls - 1);                      // (whatever is stored, the load stays inside the row)
  xid = logits[(int64_t)r * kCls + id];
  lprob = logf(prob[r]);
}

// The tables of the tile of crops n0 .. n0 + tile_n - 1 into lp (kTile * kTable floats of LDS), by the whole workgroup of 256 threads; row_x / row_l: 104
// floats of LDS each for the rows' constants.  Both barriers are inside; column 95 of every row is -inf.
__device__ __forceinline__ void lex_tile_tables(float* lp, float* row_x, float* row_l, const float* __restrict__ logits, const int* __restrict__ ids,
                                                const float* __restrict__ prob, int n0, int tile_n, const ClassMask& cm, const RowMask* __restrict__ row_masks) {
  const int tid = threadIdx.x;
  if (tid < tile_n * kPos) lex_row_consts(logits, ids, prob, n0 * kPos + tid, row_x[tid], row_l[tid]);
  __syncthreads();
  for (int t = 0; t < tile_n; ++t) {                                 // crop after crop: the crop, and with it its class mask, is uniform
    const int n = n0 + t;
    const RowClassMask rm = row_class_mask(cm, row_masks, n);
    for (int e = tid; e < kTable; e += 256) {
      const int p = e / kStride, c = e - p * kStride;
      const bool ok = c < kCls && rm.allows(c);
      const float x = ok ? logits[(int64_t)(n * kPos + p) * kCls + c] : 0.0f;
      lp[t * kTable + e] = lex_lp(x, row_x[t * kPos + p], row_l[t * kPos + p], ok);
    }
  }
  __syncthreads();
}

// ---- the rule
// the replacement rule on one cell
template <bool EDITS>
__device__ __forceinline__ void fz_take(float& s, int& e, float cs, int ce) {
  const bool t = cs > s || (EDITS && cs == s && ce < e);
  s = t ? cs : s;
  if (EDITS) e = t ? ce : e;
}

// logp and edits of the word in (ra, rb) of length L under band B and gap g; lp(p, c) is the table's entry, p a compile-time constant at every call.
// EDITS = false: scores alone (out_e stays 0).
template <int B, bool EDITS, class LP>
__device__ __forceinline__ void fuzzy_dp(const uint4& ra, const uint4& rb, int L, float g, LP lp, float& out_s, int& out_e) {
  constexpr int W = 2 * B + 1;
  float rs[W]; int re[W];                                            // row j: cell k is D[j][j + k - B]
#pragma unroll
  for (int k = 0; k < W; ++k) {                                      // row 0: D[0][0] = 0, D[0][p] = D[0][p-1] + g
    rs[k] = -INFINITY; re[k] = 0;
    if (k == B) rs[k] = 0.0f;
    if (k > B) fz_take<EDITS>(rs[k], re[k], rs[k - 1] + g, re[k - 1] + 1);
  }
  out_s = -INFINITY; out_e = 0;
#pragma unroll
  for (int j = 1; j <= kPos; ++j) {
    const int c = (int)rec_byte(ra, rb, j);                          // entry character j-1; behind the word 0, the EOS (a class byte is < 95 by lexicon_encode)
    float ms[W];                                                     // the match terms out of row j-1, D[j-1][q] + lp[q][c] with q = j - 1 + k - B
    float es = -INFINITY; int ee = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int q = j - 1 + k - B;
      ms[k] = -INFINITY;
      if (q >= 0 && q < kPos) {
        ms[k] = rs[k] + lp(q, c);
        fz_take<EDITS>(es, ee, ms[k], re[k]);
      }
    }
    const bool at_end = j == L + 1;                                  // c is the EOS here: the match terms are the end's candidates
    out_s = at_end ? es : out_s;
    if (EDITS) out_e = at_end ? ee : out_e;
    if (j < kPos) {                                                  // row j (an entry has at most 25 characters)
      float ns[W]; int ne[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const int p = j + k - B;
        ns[k] = -INFINITY; ne[k] = 0;
        if (p >= 0 && p < kPos) {
          if (p >= 1) fz_take<EDITS>(ns[k], ne[k], ms[k], re[k]);                                // match
          if (k >= 1 && p >= 1) fz_take<EDITS>(ns[k], ne[k], ns[k - 1] + g, ne[k - 1] + 1);      // extra: D[j][p-1]
          if (k + 1 < W) fz_take<EDITS>(ns[k], ne[k], rs[k + 1] + g, re[k + 1] + 1);             // dropped: D[j-1][p]
        }
      }
      const bool live = j <= L;                                      // a word that has ended keeps its row
#pragma unroll
      for (int k = 0; k < W; ++k) {
        rs[k] = live ? ns[k] : rs[k];
        if (EDITS) re[k] = live ? ne[k] : re[k];
      }
    }
  }
}
}  // namespace

template <int CAP, int B>
__global__ void __launch_bounds__(256) lexicon_fuzzy_score_kernel(const float* __restrict__ logits, int N, const int* __restrict__ ids,
                                                                  const float* __restrict__ prob, const uint4* __restrict__ records, int V, int chunk, int chunks,
                                                                  int M, float gap, int* __restrict__ part_idx, float* __restrict__ part_logp, ClassMask cm,
                                                                  const RowMask* __restrict__ row_masks) {
  __shared__ float lp[kTile * kTable];                               // 39,936 bytes
  __shared__ float xs[kTile][4][8];                                  // the four waves' top-M of every crop of the tile: the scores ...
  __shared__ float xi[kTile][4][8];                                  // ... and the indices, as bit patterns; before the scoring loop, the rows' constants (as lexicon.hip)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.y * kTile, tile_n = min(kTile, N - n0);    // (tile_n >= 1: the grid has ceil(N / kTile) tiles)
  const int ck = blockIdx.x;
  lex_tile_tables(lp, &xs[0][0][0], &xi[0][0][0], logits, ids, prob, n0, tile_n, cm, row_masks);
  float ts[kTile][CAP]; int ti[kTile][CAP];
#pragma unroll
  for (int t = 0; t < kTile; ++t)
#pragma unroll
    for (int j = 0; j < CAP; ++j) { ts[t][j] = -INFINITY; ti[t][j] = kNone; }
  const int w_end = min(V, (ck + 1) * chunk);                        // (chunk * chunks < 2^31: V <= 2^20 and chunk <= V rounded up)
  for (int w = ck * chunk + tid; w < w_end; w += 256) {
    const uint4 ra = records[2 * (size_t)w], rb = records[2 * (size_t)w + 1];
    const int L = (int)rec_byte(ra, rb, 0);
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      if (t < tile_n) {                                              // (uniform over the workgroup)
        float s; int e;
        fuzzy_dp<B, false>(ra, rb, L, gap, [&](int p, int c) { return lp[t * kTable + p * kStride + c]; }, s, e);
        if (s > -INFINITY) lex_insert<CAP>(ts[t], ti[t], s, w);      // (false for -inf and for NaN)
      }
    }
  }
  // per crop: the wave's top-M, lane j holding slot j
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    if (t < tile_n) {
      float os; int oi;
      wave_select<CAP>(ts[t], ti[t], M, lane, os, oi);
      if (lane < M) { xs[t][wave][lane] = os; xi[t][wave][lane] = __int_as_float(oi); }
    }
  }
  __syncthreads();
  // wave t: crop t's 4 M candidates, one per lane, to the partial of (crop, chunk)
  if (wave < tile_n) {
    float a[1] = {-INFINITY}; int b[1] = {kNone};
    if (lane < 4 * M) { a[0] = xs[wave][lane / M][lane % M]; b[0] = __float_as_int(xi[wave][lane / M][lane % M]); }
    float os; int oi;
    wave_select<1>(a, b, M, lane, os, oi);
    if (lane < M) {
      const size_t o = ((size_t)(n0 + wave) * chunks + ck) * M + lane;
      part_idx[o] = oi == kNone ? -1 : oi;
      part_logp[o] = os;
    }
  }
}

// the edits of the merged matches: thread (n, slot) repeats the rule with pairs for word idx[n][slot]
template <int B>
__global__ void __launch_bounds__(256) lexicon_fuzzy_edits_kernel(const float* __restrict__ logits, int N, const int* __restrict__ ids, const float* __restrict__ prob,
                                                                  const uint4* __restrict__ records, int M, float gap, const int* __restrict__ idx,
                                                                  int* __restrict__ edits, ClassMask cm, const RowMask* __restrict__ row_masks) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= N * M) return;
  const int n = g / M, w = idx[g];
  if (w < 0) { edits[g] = -1; return; }
  RowClassMask rm{cm.blocked[0], cm.blocked[1], cm.blocked[2]};      // (the crop differs from lane to lane here: the row's mask by a load of the lane's own)
  if (row_masks) { const RowMask r = row_masks[n]; rm.b0 = r.x; rm.b1 = r.y; rm.b2 = r.z; }
  float xid[kPos], lpr[kPos];                                        // the rows' constants (indexed by compile-time positions only)
#pragma unroll
  for (int p = 0; p < kPos; ++p) lex_row_consts(logits, ids, prob, n * kPos + p, xid[p], lpr[p]);
  const uint4 ra = records[2 * (size_t)w], rb = records[2 * (size_t)w + 1];
  const int L = (int)rec_byte(ra, rb, 0);
  float s; int e;
  fuzzy_dp<B, true>(ra, rb, L, gap, [&](int p, int c) {
    const bool ok = c < kCls && rm.allows(c);
    const float x = ok ? logits[(int64_t)(n * kPos + p) * kCls + c] : 0.0f;
    return lex_lp(x, xid[p], lpr[p], ok);
  }, s, e);
  edits[g] = e;
}

// the tables as a workgroup forms them, for tests: one workgroup per tile, LDS to global
__global__ void __launch_bounds__(256) lexicon_tables_kernel(const float* __restrict__ logits, int N, const int* __restrict__ ids, const float* __restrict__ prob,
                                                             float* __restrict__ out, ClassMask cm, const RowMask* __restrict__ row_masks) {
  __shared__ float lp[kTile * kTable];
  __shared__ float row_x[kTile * kPos], row_l[kTile * kPos];
  const int n0 = blockIdx.x * kTile, tile_n = min(kTile, N - n0);
  lex_tile_tables(lp, row_x, row_l, logits, ids, prob, n0, tile_n, cm, row_masks);
  for (int e = threadIdx.x; e < tile_n * kTable; e += 256) out[(size_t)n0 * kTable + e] = lp[e];
}

void launch_lexicon_tables(const float* logits, int N, const int* ids, const float* prob, float* lp, hipStream_t s, ClassMask cm, const RowMask* row_masks) {
  if (N <= 0) return;
  hipLaunchKernelGGL(lexicon_tables_kernel, dim3((N + kTile - 1) / kTile), dim3(256), 0, s, logits, N, ids, prob, lp, cm, row_masks);
}

template <int B>
static void launch_fuzzy_band(const float* logits, int N, const int* ids, const float* prob, const uint4* rec, int V, int M, float gap, int chunk, int chunks,
                              const int* idx, int* edits, int* part_idx, float* part_logp, hipStream_t s, ClassMask cm, const RowMask* row_masks, bool score) {
  const dim3 grid(chunks, (N + kTile - 1) / kTile);
  if (score) {
#define TTR_FZ_LAUNCH(CAP) \
  hipLaunchKernelGGL((lexicon_fuzzy_score_kernel<CAP, B>), grid, dim3(256), 0, s, logits, N, ids, prob, rec, V, chunk, chunks, M, gap, part_idx, part_logp, cm, row_masks)
    if (M == 1) TTR_FZ_LAUNCH(1); else if (M == 2) TTR_FZ_LAUNCH(2); else if (M <= 4) TTR_FZ_LAUNCH(4); else TTR_FZ_LAUNCH(8);
#undef TTR_FZ_LAUNCH
  } else {
    hipLaunchKernelGGL(lexicon_fuzzy_edits_kernel<B>, dim3((N * M + 255) / 256), dim3(256), 0, s, logits, N, ids, prob, rec, M, gap, idx, edits, cm, row_masks);
  }
}

void launch_lexicon_fuzzy(const float* logits, int N, const int* ids, const float* prob, const void* records, int V, int M, int band, float gap, int* idx,
                          float* logp, int* edits, int* part_idx, float* part_logp, hipStream_t s, ClassMask cm, const RowMask* row_masks) {
  if (N <= 0) return;
  if (V < 1 || V > (1 << 20)) throw std::runtime_error("lexicon: the number of words must lie in 1..2^20");
  if (M < 1 || M > 8) throw std::runtime_error("lexicon: M must lie in 1..8");
  if (N > kTile * 65535) throw std::runtime_error("lexicon: more than 262140 crops in one launch");   // (the crop tiles are the grid's y)
  if (band < 0 || band > 3) throw std::runtime_error("lexicon: the fuzzy band must lie in 0..3");
  if (!(gap <= 0.0f) || gap == -INFINITY) throw std::runtime_error("lexicon: the fuzzy gap must be finite and <= 0");
  const int chunk = (int)lexicon_chunk_words(N, V, M), chunks = (V + chunk - 1) / chunk;
  const uint4* rec = static_cast<const uint4*>(records);
  auto pass = [&](bool score) {
    switch (band) {
      case 0: launch_fuzzy_band<0>(logits, N, ids, prob, rec, V, M, gap, chunk, chunks, idx, edits, part_idx, part_logp, s, cm, row_masks, score); break;
      case 1: launch_fuzzy_band<1>(logits, N, ids, prob, rec, V, M, gap, chunk, chunks, idx, edits, part_idx, part_logp, s, cm, row_masks, score); break;
      case 2: launch_fuzzy_band<2>(logits, N, ids, prob, rec, V, M, gap, chunk, chunks, idx, edits, part_idx, part_logp, s, cm, row_masks, score); break;
      default: launch_fuzzy_band<3>(logits, N, ids, prob, rec, V, M, gap, chunk, chunks, idx, edits, part_idx, part_logp, s, cm, row_masks, score); break;
    }
  };
  pass(true);
  launch_lexicon_merge(part_idx, part_logp, N, chunks, M, idx, logp, s);
  if (edits) pass(false);
}

}  // namespace ttr
