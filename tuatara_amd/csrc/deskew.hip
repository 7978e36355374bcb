// Deskew (DESIGN.md "Deskew"): every page's skew estimated from its ink bitmap, and the page resampled upright about its centre before the detector reads it.
//
// deskew_score_kernel   step 2 of the rule.  One workgroup of 256 threads per (candidate slope, page).  in: the ink bitmap table_ink_kernel writes (tables.hip:
//                       bits [page][h][ceil(w / 64)], a few dozen KB a page, read by all 2 M + 1 candidates from L2).  A thread takes a 64-pixel word: under
//                       slope k the row offset (x k + 256) >> 9 is constant over runs of x (at least 4 px at |k| = 128), so the word's share of a bin is the
//                       popcount of a masked segment - one LDS integer atomic per segment that holds ink, none for a blank word.  Bins: h + 2 (w M / 512 + 1)
//                       uint32 in LDS.  Then the squares, summed as uint64 over the workgroup: scores [page][2 M + 1].  Integer sums: order-free, exact.
// deskew_rotate_kernel  steps 3 and 5.  pages x tiles of 256 px x 4 rows, 256 threads, a thread four pixels of one row.  Every wave repeats the choice from
//                       the page's 2 M + 1 scores (a shuffle reduction over (score, |k|, k)), takes the slope's (C, S) from the host's table and walks its
//                       pixels by adding (2 C, 2 S) to the source coordinates; the four taps are byte gathers, the twelve result bytes go out as three dwords
//                       where the destination is dword-aligned and by bytes elsewhere.  Tile (0, 0)'s first thread writes the page's record.
// Source and destination pages come as page-table rows (page_table.h), so a batch may mix sizes and a source may be a window with any base and stride.
// The outputs are the host rule's (geometry.cpp: deskew_from_page) bit for bit.
#include "common.h"
#include "kernels.h"
#include "page_table.h"
#include "deskew_rule.h"

namespace ttr {

namespace {
constexpr int kDsThreads = 256;
constexpr int kRotTileW = 256, kRotTileH = 4;
}  // namespace

__global__ __launch_bounds__(kDsThreads) void deskew_score_kernel(const unsigned long long* __restrict__ bits, const PageRow* __restrict__ table, int Hcap, int Wcap, int M,
                                                                  unsigned long long* __restrict__ scores) {
  extern __shared__ __attribute__((aligned(16))) unsigned ds_bins[];
  __shared__ unsigned long long wsum[kDsThreads / 64];
  const int pg = (int)blockIdx.y, k = (int)blockIdx.x - M, tid = (int)threadIdx.x;
  const int h = table[pg].h, w = table[pg].w, nw = (w + 63) >> 6;
  const int bias = dsk_bias(w, M), nb = dsk_bins(h, w, M);       // (nb <= dsk_bins(Hcap, Wcap, M), the launch's LDS)
  for (int i = tid; i < nb; i += kDsThreads) ds_bins[i] = 0;
  __syncthreads();
  const unsigned long long* const bm = bits + (size_t)pg * ((size_t)Hcap * (size_t)((Wcap + 63) >> 6));
  const int words = h * nw;                                       // (below 2^20: both sides are below 8192)
  for (int idx = tid; idx < words; idx += kDsThreads) {
    const unsigned long long v = bm[idx];
    if (!v) continue;
    const int y = idx / nw, xw = 64 * (idx - y * nw);
    if (k == 0) { atomicAdd(&ds_bins[y + bias], (unsigned)__popcll(v)); continue; }
    int x = xw;
    while (x < xw + 64 && (v >> (x - xw)) != 0) {
      const int nx = min(dsk_next(x, k), xw + 64), len = nx - x;
      const unsigned long long mask = (len >= 64 ? ~0ull : ((1ull << len) - 1)) << (x - xw);
      const unsigned c = (unsigned)__popcll(v & mask);
      if (c) atomicAdd(&ds_bins[y - dsk_off(x, k) + bias], c);   // (in 0..nb - 1: |offset| < bias)
      x = nx;
    }
  }
  __syncthreads();
  unsigned long long s = 0;
  for (int i = tid; i < nb; i += kDsThreads) { const unsigned long long c = ds_bins[i]; s += c * c; }
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) scores[(size_t)pg * (2 * M + 1) + (k + M)] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(kDsThreads) void deskew_rotate_kernel(const PageRow* __restrict__ src_table, const PageRow* __restrict__ dst_table, int M, int gain,
                                                                   const unsigned long long* __restrict__ scores, const int* __restrict__ cs, DeskewRec* __restrict__ recs) {
  const int pg = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63;
  const PageRow P = src_table[pg];
  const int h = P.h, w = P.w;
  const int x0 = (int)blockIdx.x * kRotTileW + 4 * lane, y = (int)blockIdx.y * kRotTileH + (tid >> 6);
  if ((int)blockIdx.x * kRotTileW >= w || (int)blockIdx.y * kRotTileH >= h) return;   // (the launch covers the largest page of a mixed batch; whole workgroups leave)
  // 3: the choice, once per wave
  const unsigned long long* const sc = scores + (size_t)pg * (2 * M + 1);
  const unsigned long long s0 = sc[M];
  unsigned long long bs = s0;
  int bk = 0;
  for (int i = lane; i < 2 * M + 1; i += 64) {
    const unsigned long long s = sc[i];
    if (dsk_better(s, i - M, bs, bk)) { bs = s; bk = i - M; }
  }
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long os = __shfl_xor(bs, d);
    const int ok = __shfl_xor(bk, d);
    if (dsk_better(os, ok, bs, bk)) { bs = os; bk = ok; }
  }
  const int slope = dsk_slope(bk, bs, s0, gain);
  const int C = cs[2 * (slope + kDskMaxSlope)], S = cs[2 * (slope + kDskMaxSlope) + 1];
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) recs[pg] = DeskewRec{slope, bk, C, S, w, h, slope != 0 ? 1 : 0, 0, s0, bs};
  if (y >= h || x0 >= w) return;
  // 5: four pixels of row y
  const PageRow D = dst_table[pg];
  uint8_t* const out = const_cast<uint8_t*>(D.data) + (size_t)y * (size_t)D.stride + (size_t)x0 * 3;
  int64_t U, V;
  dsk_source(C, S, w, h, x0, y, &U, &V);
  const int n = min(4, w - x0);
  uint32_t b[12];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p < n) {
      const int fx = (int)((U >> 9) & 255), fy = (int)((V >> 9) & 255);
      const int xa = dsk_clamp(U >> 17, w), xb = dsk_clamp((U >> 17) + 1, w), ya = dsk_clamp(V >> 17, h), yb = dsk_clamp((V >> 17) + 1, h);
      const uint8_t* ra = P.data + (size_t)ya * (size_t)P.stride;
      const uint8_t* rb = P.data + (size_t)yb * (size_t)P.stride;
#pragma unroll
      for (int c = 0; c < 3; ++c) b[3 * p + c] = (uint32_t)dsk_blend(ra[3 * xa + c], ra[3 * xb + c], rb[3 * xa + c], rb[3 * xb + c], fx, fy);
    } else {
      b[3 * p] = b[3 * p + 1] = b[3 * p + 2] = 0;
    }
    U += 2 * (int64_t)C; V += 2 * (int64_t)S;
  }
  if (n == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
    o[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    o[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    o[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
  } else {
    for (int i = 0; i < 3 * n; ++i) out[i] = (uint8_t)b[i];
  }
}

void launch_deskew_score(const uint64_t* bits, const PageRow* table, int pages, int Hcap, int Wcap, int max_slope, uint64_t* scores, hipStream_t s) {
  if (pages <= 0) return;
  if (Hcap <= 0 || Wcap <= 0 || Hcap >= kDskSideCap || Wcap >= kDskSideCap || max_slope < 1 || max_slope > kDskMaxSlope)
    throw std::runtime_error("deskew_score: a page side outside 1..8191 or max_slope outside 1..128");
  const size_t lds = (size_t)dsk_bins(Hcap, Wcap, max_slope) * 4;   // at most 12287 integers
  hipLaunchKernelGGL(deskew_score_kernel, dim3(2 * max_slope + 1, pages), dim3(kDsThreads), lds, s, reinterpret_cast<const unsigned long long*>(bits), table, Hcap, Wcap,
                     max_slope, reinterpret_cast<unsigned long long*>(scores));
}

void launch_deskew_rotate(const PageRow* src_table, const PageRow* dst_table, int pages, int Hcap, int Wcap, int max_slope, int gain, const uint64_t* scores, const int* cs,
                          DeskewRec* recs, hipStream_t s) {
  if (pages <= 0) return;
  if (Hcap <= 0 || Wcap <= 0 || Hcap >= kDskSideCap || Wcap >= kDskSideCap) throw std::runtime_error("deskew_rotate: a page side outside 1..8191");
  const dim3 grid((Wcap + kRotTileW - 1) / kRotTileW, (Hcap + kRotTileH - 1) / kRotTileH, pages);
  hipLaunchKernelGGL(deskew_rotate_kernel, grid, dim3(kDsThreads), 0, s, src_table, dst_table, max_slope, gain, reinterpret_cast<const unsigned long long*>(scores), cs, recs);
}

}  // namespace ttr
