// Selection marks (DESIGN.md "Selection marks"): checkboxes found on the pages' ink bitmaps, their state read from the ink inside, every item's mark and every
// mark's label.
//
// mark_cand_kernel   the candidate pass.  pages x row bands of 32 rows, 256 threads: thread t owns row t / 8 of the band and the t % 8-th eighth of the row's
//                    words, so thread order IS (y, x) order.  A thread forms its words' corners (mark_corners: shifts and two ands a word), puts each through
//                    steps 3 - 5 (mark_test, marks_rule.h: ctz over the runs, popcount over the interior) and counts; the counts are block-scanned, and a second
//                    walk writes the kept records into the band's slots in order.  out: cand [page][band][512][12] (a band beyond 512 keeps its first 512: the
//                    page is beyond the cap anyway) and counts [page][band][2] = kept, corners examined.  in: bits / bitsT as the pixel passes leave them
//                    (ink_tile.h); a page's lines are read through their own ceil(len / 64) words and never beyond.
// mark_page_kernel   one workgroup of 256 per page: scans the band counts, compacts the records into the side block in (y, x) order, applies the cap, then a
//                    thread an item for the items' marks and a thread a mark for the labels (mark_item / mark_label, the host rule's own functions).
// No atomic anywhere: every slot is a scan's.  Integer arithmetic only: the outputs are the host rule's (geometry.cpp: marks_from_bits, marks_items) bit for bit.
#include "common.h"
#include "kernels.h"
#include "marks_rule.h"
#include "page_table.h"

namespace ttr {

namespace {

constexpr int kMkThreads = 256, kMkSegs = kMkThreads / kMarkBandRows;
static_assert(kMkSegs * kMarkBandRows == kMkThreads, "a thread per (row, segment)");

// exclusive scan of one value per thread over the workgroup of 256; *total = the sum.  Two barriers.
__device__ __forceinline__ int mk_scan(int v, int* wsum, int tid, int* total) {
  const int lane = tid & 63, wv = tid >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int k = 0; k < kMkThreads / 64; ++k) { const int s = wsum[k]; base += k < wv ? s : 0; tot += s; }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

}  // namespace

__global__ __launch_bounds__(kMkThreads) void mark_cand_kernel(const unsigned long long* __restrict__ bits_all, const unsigned long long* __restrict__ bitsT_all, int h_, int w_,
                                                               const PageRow* __restrict__ table, int Hcap, int Wcap, int bands, int min_side, int max_side, int fill,
                                                               int* __restrict__ cand, int* __restrict__ counts) {
  __shared__ int wsum[kMkThreads / 64];
  const int pg = (int)blockIdx.y, band = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int h = table ? table[pg].h : h_, w = table ? table[pg].w : w_;
  const int nwx = (w + 63) >> 6, nwy = (h + 63) >> 6;
  const uint64_t* const bits = reinterpret_cast<const uint64_t*>(bits_all) + (size_t)pg * ((size_t)Hcap * (size_t)((Wcap + 63) >> 6));
  const uint64_t* const bitsT = reinterpret_cast<const uint64_t*>(bitsT_all) + (size_t)pg * ((size_t)Wcap * (size_t)((Hcap + 63) >> 6));
  int* const cnt_out = counts + 2 * ((size_t)pg * bands + band);
  if (band * kMarkBandRows >= h) {                                      // (the launch covers the largest page of a mixed batch)
    if (tid == 0) { cnt_out[0] = 0; cnt_out[1] = 0; }
    return;
  }
  const int y = band * kMarkBandRows + tid / kMkSegs, seg = tid % kMkSegs;
  const int per = (nwx + kMkSegs - 1) / kMkSegs;
  const int k0 = seg * per, k1 = y < h ? (k0 + per < nwx ? k0 + per : nwx) : 0;   // this thread's words [k0, k1) of row y; none beyond the page
  const uint64_t* const row = bits + (size_t)(y < h ? y : 0) * nwx;
  const uint64_t* const above = y > 0 && y < h ? row - nwx : nullptr;
  int32_t rec[kMarkRec];
  int kept = 0, corners = 0;
  for (int k = k0; k < k1; ++k) {
    uint64_t c = mark_corners(row, above, k);
    corners += mark_popc(c);
    while (c) {
      const int x = 64 * k + mark_ctz(c);
      c &= c - 1;
      kept += mark_test(bits, nwx, bitsT, nwy, x, y, min_side, max_side, fill, rec) ? 1 : 0;
    }
  }
  int total, all_corners;
  int at = mk_scan(kept, wsum, tid, &total);
  (void)mk_scan(corners, wsum, tid, &all_corners);
  if (tid == 0) { cnt_out[0] = total; cnt_out[1] = all_corners; }
  if (!kept) return;
  int* const slots = cand + ((size_t)pg * bands + band) * (size_t)(kMarkCap * kMarkRec);
  for (int k = k0; k < k1; ++k) {
    uint64_t c = mark_corners(row, above, k);
    while (c) {
      const int x = 64 * k + mark_ctz(c);
      c &= c - 1;
      if (!mark_test(bits, nwx, bitsT, nwy, x, y, min_side, max_side, fill, rec)) continue;
      if (at < kMarkCap)
        for (int j = 0; j < kMarkRec; ++j) slots[at * kMarkRec + j] = rec[j];
      ++at;
    }
  }
}

__global__ __launch_bounds__(kMkThreads) void mark_page_kernel(const int* __restrict__ cand, const int* __restrict__ counts, int bands, const int* __restrict__ centres,
                                                               const int* __restrict__ first, int* side_all, int* item_mark) {
  __shared__ int wsum[kMkThreads / 64];
  const int pg = (int)blockIdx.x, tid = (int)threadIdx.x;
  int* const side = side_all + (size_t)pg * kMarkSideInts;
  const int* const cnt = counts + 2 * (size_t)pg * bands;
  // 6: the bands' offsets, in band order; the cap
  int n = 0, corners = 0;
  for (int b0 = 0; b0 < bands; b0 += kMkThreads) {
    const int b = b0 + tid;
    int total, c;
    (void)mk_scan(b < bands ? cnt[2 * b] : 0, wsum, tid, &total);
    (void)mk_scan(b < bands ? cnt[2 * b + 1] : 0, wsum, tid, &c);
    n += total; corners += c;
  }
  const bool over = n > kMarkCap;
  if (!over) {
    int base = 0;
    for (int b0 = 0; b0 < bands; b0 += kMkThreads) {
      const int b = b0 + tid, mine = b < bands ? cnt[2 * b] : 0;
      int total;
      const int at = base + mk_scan(mine, wsum, tid, &total);
      const int* const src = cand + ((size_t)pg * bands + b) * (size_t)(kMarkCap * kMarkRec);
      for (int j = 0; j < mine * kMarkRec; ++j) side[kMarkHdr + at * kMarkRec + j] = src[j];   // (mine <= n <= the cap: inside the band's slots and the block)
      base += total;
    }
  }
  if (tid < kMarkHdr) side[tid] = tid == 0 ? (over ? -6 : 1) : tid == 1 ? (over ? 0 : n) : tid == 2 ? corners : tid == 3 ? n : 0;
  __syncthreads();                                                       // (the records and the header, written above, are read below)
  // 7: the items' marks, then the marks' labels
  const int i0 = first[pg], ni = first[pg + 1] - i0;
  for (int i = tid; i < ni; i += kMkThreads) item_mark[i0 + i] = mark_item(side, centres[2 * (i0 + i)], centres[2 * (i0 + i) + 1]);
  __syncthreads();
  if (!over)
    for (int m = tid; m < n; m += kMkThreads) {
      int* const r = side + kMarkHdr + kMarkRec * m;
      r[11] = mark_label(r, centres + 2 * (size_t)i0, item_mark + i0, ni);
    }
}

void launch_mark_cand(const uint64_t* bits, const uint64_t* bitsT, int h, int w, const PageRow* table, int pages, int Hcap, int Wcap, int min_side, int max_side, int fill,
                      int* cand, int* counts, hipStream_t s) {
  if (pages <= 0) return;
  if (Hcap <= 0 || Wcap <= 0 || Hcap >= 32768 || Wcap >= 32768 || (!table && (h > Hcap || w > Wcap))) throw std::runtime_error("mark_cand: a page side outside 1..32767");
  if (!marks_args_ok(min_side, max_side, fill, 128)) throw std::runtime_error("mark_cand: bad parameters");
  const int bands = marks_bands(Hcap);
  hipLaunchKernelGGL(mark_cand_kernel, dim3(bands, pages), dim3(kMkThreads), 0, s, reinterpret_cast<const unsigned long long*>(bits),
                     reinterpret_cast<const unsigned long long*>(bitsT), h, w, table, Hcap, Wcap, bands, min_side, max_side, fill, cand, counts);
}

void launch_mark_page(const int* cand, const int* counts, int pages, int Hcap, const int* centres, const int* first, int* side, int* item_mark, hipStream_t s) {
  if (pages <= 0) return;
  hipLaunchKernelGGL(mark_page_kernel, dim3(pages), dim3(kMkThreads), 0, s, cand, counts, marks_bands(Hcap), centres, first, side, item_mark);
}

}  // namespace ttr
