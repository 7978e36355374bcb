// Lexicon matching behind the recogniser's final decode (DESIGN.md "Lexicon matching"): the log-probability of every word of a caller's list under each
// crop's refined per-position distributions, and per crop the M best words.
//
//   lp[p][c] = (x[p][c] - x[p][id[p]]) + logf(prob[p])   for an allowed class c, -inf for a blocked one; fp32, full-precision logf.  id and prob are read
//              from the standard block: prob already is 1 / sum over the allowed classes, so no maximum or sum is formed a second time
//   logp(w)  = the sum, in position order from 0.0f, of lp[p][w_p] for p < L, then + lp[L][0] (the EOS behind the word)
//   idx / logp [N][M]   per crop the words in the TOTAL order (logp descending, index ascending); a score of -inf or NaN is never kept; the slots left
//              over hold -1 / -INFINITY
//
// The order is total (no two entries compare equal: indices are unique), every selection below picks "the best of a set" by that order, and a word's score
// is one fixed chain of fp32 additions over table look-ups.  So the result does not depend on how the lexicon is split into chunks, the crops into tiles, the
// words over threads, or on the order in which workgroups finish: there are no floating-point atomics, no atomics at all, and no merge by arrival order.
// lp is formed once per (crop, position, class) and then only looked up, so two entries that spell the same word get identical bits.
//
// lexicon_score_kernel: a workgroup (256 threads) owns a tile of kTile = 4 crops and a chunk of the words (kLexChunk = 1024, or that times a power of two
// when the partials would grow past kLexPartialCap).  It builds the tile's four lp tables in LDS (26 rows of kStride = 96 floats each, 9984 bytes a crop;
// a row's x[id] and logf(prob) are formed first, once per row, by one thread per (crop, position)),
// then every thread fetches its words - a 32-byte record each: length, 25 class bytes, zeros, two 16-byte loads - keeps a word's classes in registers and
// scores it against the four crops: 26 ds_read_b32 per (word, crop) whose address is a compile-time (crop, position) offset plus 4 * class.  The zero
// padding of a record is the EOS class, so position L needs no special case, and positions behind it are read and not added.  Each thread keeps a sorted
// top-CAP per crop in registers (CAP = 1, 2, 4 or 8 at compile time, the smallest that holds M: no register array is indexed by a run-time value); a wave
// reduces its 64 lists to the wave's top-M by M rounds of a shuffle arg-max (the winner's lane drops its head), the four waves' lists meet in LDS, and wave t
// reduces crop t's 4 M candidates the same way and stores the partial [crop][chunk][M].  lexicon_merge_kernel: one wave per crop reads that crop's
// chunks * M partial entries into per-lane sorted lists and reduces them once more.
//
// LDS bank conflicts of the gather.  ds_read_b32 serves a wave as two groups of 32 lanes, bank = (address / 4) mod 32.  Lanes hold DIFFERENT WORDS of ONE
// crop: at position p a group reads 32 classes out of one 95-float row, so the bank is (p * kStride + c) mod 32 - for any stride a function of c mod 32
// alone within the group, and lanes that read the same class share one address (a broadcast, no conflict).  The conflict degree of a read is therefore the
// largest number of DISTINCT classes among the group's 32 lanes that agree mod 32.  The class table puts the ten digits at 1..10, a..z at 11..36 and A..Z at
// 37..62: each alphabet covers at most 26 consecutive classes, so within one alphabet distinct letters never share a bank, and a single-case vocabulary reads
// conflict-free; conflicts come from mixing alphabets - the classes 32 apart: the digits 0..3 with w..z, a..t with G..Z -, degree 2, rarely 3 (a third class
// 64 apart is punctuation).  Words drawn uniformly over all classes - the tests' and the profile's kind, the worst case - give an expected
// degree near 3 (32 lanes into 32 banks, equal classes merged).  The other layout, the same word for different crops across the lanes, would be free of
// conflicts with a table stride of 1 mod 32, but needs 32 crops' tables (312 KB) resident, and a page has about 12 crops.  kStride = 96 is chosen for the
// build (rows start 16-byte aligned, the pad column keeps every class byte < 96 inside its row), not for the gather, which no row stride can help.
#include "common.h"
#include "kernels.h"
#include "lexicon_common.h"

namespace ttr {

template <int CAP>
__global__ void __launch_bounds__(256) lexicon_score_kernel(const float* __restrict__ logits, int N, const int* __restrict__ ids, const float* __restrict__ prob,
                                                            const uint4* __restrict__ records, int V, int chunk, int chunks, int M,
                                                            int* __restrict__ part_idx, float* __restrict__ part_logp, ClassMask cm,
                                                            const RowMask* __restrict__ row_masks) {
  __shared__ float lp[kTile * kTable];                               // 39,936 bytes
  __shared__ float xs[kTile][4][8];                                  // the four waves' top-M of every crop of the tile: the scores ...
  __shared__ float xi[kTile][4][8];                                  // ... and the indices, as bit patterns (__int_as_float)
  // per (crop, position): x[id] and logf(prob), formed once.  They live in xs / xi (104 of 128 floats each), which are written only behind the scoring
  // loop, two barriers later: a second pair of arrays would take the block past 40 KB and the CU from four workgroups to three
  float* const row_x = &xs[0][0][0];
  float* const row_l = &xi[0][0][0];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.y * kTile, tile_n = min(kTile, N - n0);    // (tile_n >= 1: the grid has ceil(N / kTile) tiles)
  const int ck = blockIdx.x;
  // the rows' constants first, one thread per (crop, position): one logf and one look-up of x[id] per row, not one per class
  if (tid < tile_n * kPos) {
    const int r = n0 * kPos + tid;
    const int id = min(max(ids[r], 0), kCls - 1);                    // (decode_conf_kernel's ids lie inside the classes; whatever is stored, the load stays inside the row)
    row_x[tid] = logits[(int64_t)r * kCls + id];
    row_l[tid] = logf(prob[r]);
  }
  __syncthreads();
  // the tile's tables: crop after crop (so that the crop, and with it its class mask, is uniform), 2496 entries over 256 threads
  for (int t = 0; t < tile_n; ++t) {
    const int n = n0 + t;
    const RowClassMask rm = row_class_mask(cm, row_masks, n);
    for (int e = tid; e < kTable; e += 256) {
      const int p = e / kStride, c = e - p * kStride;
      float v = -INFINITY;
      if (c < kCls && rm.allows(c)) {
        v = (logits[(int64_t)(n * kPos + p) * kCls + c] - row_x[t * kPos + p]) + row_l[t * kPos + p];
      }
      lp[t * kTable + e] = v;
    }
  }
  __syncthreads();
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
        float s = 0.0f;
#pragma unroll
        for (int p = 0; p < kPos; ++p) {
          const float v = lp[t * kTable + p * kStride + (int)rec_byte(ra, rb, p + 1)];   // (a class byte is < 95 by lexicon_encode, the padding 0: inside the row)
          s = p <= L ? s + v : s;
        }
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
    const float rs = os; const int ri = oi;
    if (lane < M) {
      const size_t o = ((size_t)(n0 + wave) * chunks + ck) * M + lane;
      part_idx[o] = ri == kNone ? -1 : ri;
      part_logp[o] = rs;
    }
  }
}

template <int CAP>
__global__ void __launch_bounds__(256) lexicon_merge_kernel(const int* __restrict__ part_idx, const float* __restrict__ part_logp, int N, int entries, int M,
                                                            int* __restrict__ idx, float* __restrict__ logp) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                                // (a whole wave; the kernel has no barrier)
  float ts[CAP]; int ti[CAP];
#pragma unroll
  for (int j = 0; j < CAP; ++j) { ts[j] = -INFINITY; ti[j] = kNone; }
  const int* pi = part_idx + (size_t)n * entries;
  const float* ps = part_logp + (size_t)n * entries;
  for (int e = lane; e < entries; e += 64) {
    const int i = pi[e];
    if (i >= 0) lex_insert<CAP>(ts, ti, ps[e], i);
  }
  float os; int oi;
  wave_select<CAP>(ts, ti, M, lane, os, oi);
  if (lane < M) {
    idx[(size_t)n * M + lane] = oi == kNone ? -1 : oi;
    logp[(size_t)n * M + lane] = os;
  }
}

size_t lexicon_chunk_words(int N, int V, int M) {
  size_t chunk = kLexChunk;
  while ((size_t)std::max(N, 1) * ((V + chunk - 1) / chunk) * M > kLexPartialCap) chunk *= 2;
  return chunk;
}

size_t lexicon_partial_entries(int N, int V, int M) {   // (a launch of n <= N crops writes n * chunks(n) * M <= this: chunks(n) <= V / kLexChunk rounded up, and the rule above)
  return std::min((size_t)std::max(N, 1) * (((size_t)std::max(V, 1) + kLexChunk - 1) / kLexChunk) * M, kLexPartialCap);
}

void launch_lexicon(const float* logits, int N, const int* ids, const float* prob, const void* records, int V, int M, int* idx, float* logp, int* part_idx,
                    float* part_logp, hipStream_t s, ClassMask cm, const RowMask* row_masks) {
  if (N <= 0) return;
  if (V < 1 || V > (1 << 20)) throw std::runtime_error("lexicon: the number of words must lie in 1..2^20");
  if (M < 1 || M > 8) throw std::runtime_error("lexicon: M must lie in 1..8");
  if (N > kTile * 65535) throw std::runtime_error("lexicon: more than 262140 crops in one launch");   // (the crop tiles are the grid's y)
  const int chunk = (int)lexicon_chunk_words(N, V, M), chunks = (V + chunk - 1) / chunk;
  const dim3 grid(chunks, (N + kTile - 1) / kTile), merge_grid((N + 3) / 4);
  const uint4* rec = static_cast<const uint4*>(records);
#define TTR_LEX_LAUNCH(CAP)                                                                                                                                  \
  do {                                                                                                                                                       \
    hipLaunchKernelGGL(lexicon_score_kernel<CAP>, grid, dim3(256), 0, s, logits, N, ids, prob, rec, V, chunk, chunks, M, part_idx, part_logp, cm, row_masks); \
    hipLaunchKernelGGL(lexicon_merge_kernel<CAP>, merge_grid, dim3(256), 0, s, part_idx, part_logp, N, chunks * M, M, idx, logp);                              \
  } while (0)
  if (M == 1) TTR_LEX_LAUNCH(1); else if (M == 2) TTR_LEX_LAUNCH(2); else if (M <= 4) TTR_LEX_LAUNCH(4); else TTR_LEX_LAUNCH(8);
#undef TTR_LEX_LAUNCH
}

void launch_lexicon_merge(const int* part_idx, const float* part_logp, int N, int chunks, int M, int* idx, float* logp, hipStream_t s) {
  if (N <= 0) return;
  const dim3 merge_grid((N + 3) / 4);
#define TTR_LEX_MERGE(CAP) hipLaunchKernelGGL(lexicon_merge_kernel<CAP>, merge_grid, dim3(256), 0, s, part_idx, part_logp, N, chunks * M, M, idx, logp)
  if (M == 1) TTR_LEX_MERGE(1); else if (M == 2) TTR_LEX_MERGE(2); else if (M <= 4) TTR_LEX_MERGE(4); else TTR_LEX_MERGE(8);
#undef TTR_LEX_MERGE
}

}  // namespace ttr
