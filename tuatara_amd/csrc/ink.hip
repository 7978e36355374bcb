// Local ink (DESIGN.md "Local ink"): the adaptive threshold of ink_rule.h as two bandwidth passes, in the place of table_ink_kernel's fixed rule.  Two launches,
// because the page's polarity - a sum over the whole page - must exist before any pixel is thresholded.
//
// ink_rows_kernel   pages x tiles of 256 px x 16 rows, 256 threads.  in: the pages as table_ink_kernel takes them (uniform, or the page table).  A tile's rows
//                   with a halo of R px on either side go into LDS as s = b0 + b1 + b2, zero beyond the page: by 12-byte loads - four pixels - where the page's
//                   base and row stride are multiples of 4 (every load of a thread is issued before the first is used), by bytes elsewhere and at a row's ragged
//                   end.  Each wave then turns four rows into inclusive prefix sums in place (six values a lane, one shuffle scan), and a thread forms its
//                   column's window sums as differences of two prefixes.  out: H [page][y][x] uint32 = the horizontal window sum | s << 20 (ink_rule.h), rows
//                   Wcap apart in a slot of Hcap x Wcap; and the page's sum of s, added into its record by one device-scope atomic per wave behind a shuffle
//                   reduction (integer sums are order-free: the value is exact).  The records are zeroed by a memset on the same stream.
// ink_local_kernel  pages x tiles of 256 px x 64 rows, 256 threads, a thread a column.  It reads H for rows y0 - R .. y0 + 63 + R, forms the vertical sums by a
//                   running add and subtract down its column, decides the page's polarity from the record's sum, applies the rule, and writes bits and bitsT
//                   through table_ink_kernel's LDS tile and transposition (ink_tile.h) - so everything behind the bitmaps reads what it always read.  The first
//                   tile's first thread completes the page's record.
// Integer arithmetic only: the outputs are the host rule's (geometry.cpp: ink_from_page) bit for bit.
#include "common.h"
#include "kernels.h"
#include "ink_rule.h"
#include "ink_tile.h"
#include "page_table.h"

namespace ttr {

namespace {

constexpr int kInkRowsH = 16;                           // rows of a tile of the first pass
constexpr int kInkSpan = kInkTileW + 2 * kInkRadiusMax;   // 384: a tile's row with the widest halo
constexpr int kInkQuads = kInkSpan / 4;                 // 96 four-pixel loads a row
constexpr int kInkLoads = kInkRowsH * kInkQuads / 256;  // 6 a thread
static_assert(kInkRowsH * kInkQuads % 256 == 0 && kInkSpan % 64 == 0 && kInkRowsH % 4 == 0, "the first pass's tile divides among 256 threads and 4 waves");

}  // namespace

__global__ __launch_bounds__(256) void ink_rows_kernel(const uint8_t* __restrict__ images, size_t page_bytes, int stride_, int h_, int w_, const PageRow* __restrict__ table,
                                                       int Hcap, int Wcap, int R, uint32_t* __restrict__ Hws, InkRec* __restrict__ recs) {
  __shared__ uint32_t P[kInkRowsH][kInkSpan];           // s, then its inclusive prefix sums; column c is pixel x0 - 64 + c
  const int pg = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TabPage Pg = tab_page(images, page_bytes, stride_, h_, w_, table, pg);
  const int x0 = (int)blockIdx.x * kInkTileW, y0 = (int)blockIdx.y * kInkRowsH;
  if (x0 >= Pg.w || y0 >= Pg.h) return;                 // (the launch covers the largest page of a mixed batch)
  const int xb = x0 - kInkRadiusMax;                    // pixel of column 0: a multiple of 4, and so is 3 xb
  const int xlo = x0 - R, xhi = x0 + kInkTileW - 1 + R;   // the pixels this tile's windows reach
  const bool wide = (reinterpret_cast<uintptr_t>(Pg.data) & 3) == 0 && (Pg.stride & 3) == 0;
  unsigned long long own = 0;                           // the sum of s over this thread's pixels of the tile itself
  if (wide) {
    TabPx4 v[kInkLoads];
#pragma unroll
    for (int k = 0; k < kInkLoads; ++k) {
      const int i = tid + 256 * k, row = i / kInkQuads, q = i % kInkQuads, px = xb + 4 * q, y = y0 + row;
      v[k] = TabPx4{0u, 0u, 0u};
      if (y < Pg.h && px >= 0 && px + 3 < Pg.w && px + 3 >= xlo && px <= xhi)
        v[k] = *reinterpret_cast<const TabPx4*>(Pg.data + (size_t)y * (size_t)Pg.stride + (size_t)px * 3);
    }
#pragma unroll
    for (int k = 0; k < kInkLoads; ++k) {
      const int i = tid + 256 * k, row = i / kInkQuads, q = i % kInkQuads, px = xb + 4 * q, y = y0 + row;
      const TabPx4 t = v[k];
      uint32_t s[4] = {(t.a & 255) + ((t.a >> 8) & 255) + ((t.a >> 16) & 255), (t.a >> 24) + (t.b & 255) + ((t.b >> 8) & 255),
                       ((t.b >> 16) & 255) + (t.b >> 24) + (t.c & 255), ((t.c >> 8) & 255) + ((t.c >> 16) & 255) + (t.c >> 24)};
      if (y < Pg.h && px >= 0 && px < Pg.w && px + 3 >= Pg.w && px + 3 >= xlo && px <= xhi) {   // the row's ragged end: by bytes
        const uint8_t* rp = Pg.data + (size_t)y * (size_t)Pg.stride + (size_t)px * 3;
        for (int j = 0; j < 4; ++j)
          if (px + j < Pg.w) s[j] = (uint32_t)rp[3 * j] + (uint32_t)rp[3 * j + 1] + (uint32_t)rp[3 * j + 2];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) P[row][4 * q + j] = s[j];
      if (px >= x0 && px < x0 + kInkTileW) own += (unsigned long long)s[0] + s[1] + s[2] + s[3];   // (zero beyond the page)
    }
  } else {
    for (int i = tid; i < kInkRowsH * kInkSpan; i += 256) {
      const int row = i / kInkSpan, c = i % kInkSpan, x = xb + c, y = y0 + row;
      uint32_t s = 0;
      if (y < Pg.h && x >= 0 && x < Pg.w && x >= xlo && x <= xhi) {
        const uint8_t* p = Pg.data + (size_t)y * (size_t)Pg.stride + (size_t)x * 3;
        s = (uint32_t)p[0] + (uint32_t)p[1] + (uint32_t)p[2];
      }
      P[row][c] = s;
      if (x >= x0 && x < x0 + kInkTileW) own += s;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) own += __shfl_xor(own, d);
  if (lane == 0 && own) atomicAdd(reinterpret_cast<unsigned long long*>(&recs[pg].sum), own);
  __syncthreads();
  // the rows' prefix sums, in place: a wave a row at a time, a lane six consecutive values
  constexpr int kPer = kInkSpan / 64;
  for (int r = 0; r < kInkRowsH / 4; ++r) {
    uint32_t* const row = P[wave * (kInkRowsH / 4) + r];
    uint32_t a[kPer], run = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) { run += row[kPer * lane + j]; a[j] = run; }
    uint32_t inc = run;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    const uint32_t base = inc - run;
#pragma unroll
    for (int j = 0; j < kPer; ++j) row[kPer * lane + j] = base + a[j];
  }
  __syncthreads();
  const int x = x0 + tid, c = kInkRadiusMax + tid;      // this thread's column; c - R - 1 >= -1 and c + R <= 383
  if (x >= Pg.w) return;
  uint32_t* const out = Hws + (size_t)pg * ((size_t)Hcap * (size_t)Wcap) + (size_t)x;
  for (int r = 0; r < kInkRowsH; ++r) {
    const int y = y0 + r;
    if (y >= Pg.h) break;
    const uint32_t below = c - R - 1 >= 0 ? P[r][c - R - 1] : 0u;
    const uint32_t Hx = P[r][c + R] - below, s = P[r][c] - P[r][c - 1];
    out[(size_t)y * (size_t)Wcap] = Hx | (s << kInkSShift);
  }
}

__global__ __launch_bounds__(256) void ink_local_kernel(const uint32_t* __restrict__ Hws, int h_, int w_, const PageRow* __restrict__ table, int Hcap, int Wcap, int R, int drop,
                                                        int polarity, InkRec* __restrict__ recs, unsigned long long* __restrict__ bits, unsigned long long* __restrict__ bitsT) {
  __shared__ unsigned long long tile[kInkTileH][4];
  const int pg = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = table ? table[pg].h : h_, w = table ? table[pg].w : w_;
  const int x0 = (int)blockIdx.x * kInkTileW, y0 = (int)blockIdx.y * kInkTileH;
  if (x0 >= w || y0 >= h) return;
  const unsigned long long sum = recs[pg].sum;          // (complete: ink_rows_kernel is ahead on the stream)
  const int inverted = ink_inverted(polarity, sum, h, w);
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    InkRec* const rec = recs + pg;
    rec->radius = R; rec->drop = drop; rec->polarity = polarity; rec->inverted = inverted; rec->w = w; rec->h = h;
  }
  const int x = x0 + tid;
  const bool live = x < w;
  const uint32_t* const col = Hws + (size_t)pg * ((size_t)Hcap * (size_t)Wcap) + (size_t)(live ? x : 0);
  const int nx = live ? ink_span(x, R, w) : 0;
  uint32_t S = 0;                                       // the window sum of row y: rows max(y - R, 0) .. min(y + R, h - 1)
  if (live) {
    const int a = y0 - R < 0 ? 0 : y0 - R, b = y0 + R > h - 1 ? h - 1 : y0 + R;
    for (int yy = a; yy <= b; ++yy) S += col[(size_t)yy * (size_t)Wcap] & kInkHMask;
  }
  for (int r = 0; r < kInkTileH; ++r) {
    const int y = y0 + r;
    bool on = false;
    if (live && y < h) {
      const int s = (int)(col[(size_t)y * (size_t)Wcap] >> kInkSShift);
      on = ink_local(s, nx * ink_span(y, R, h), S, drop, inverted);
      if (y + 1 + R <= h - 1) S += col[(size_t)(y + 1 + R) * (size_t)Wcap] & kInkHMask;
      if (y - R >= 0) S -= col[(size_t)(y - R) * (size_t)Wcap] & kInkHMask;
    }
    const unsigned long long m = __ballot(on);
    if (lane == 0) tile[r][wave] = m;
  }
  __syncthreads();
  ink_tile_store(tile, w, h, pg, Hcap, Wcap, bits, bitsT);
}

void launch_ink_local(const uint8_t* images, size_t page_bytes, int stride, int h, int w, const PageRow* table, int pages, int Hcap, int Wcap, int radius, int drop,
                      int polarity, uint32_t* Hws, InkRec* recs, uint64_t* bits, uint64_t* bitsT, hipStream_t s) {
  if (pages <= 0) return;
  if (Hcap <= 0 || Wcap <= 0 || Hcap >= 32768 || Wcap >= 32768 || (!table && (h > Hcap || w > Wcap))) throw std::runtime_error("ink_local: a page side outside 1..32767");
  if (!ink_args_ok(radius, drop, polarity)) throw std::runtime_error("ink_local: radius must lie in 1..64, drop in 1..255 and polarity in 0..2");
  TTR_HIP_CHECK(hipMemsetAsync(recs, 0, (size_t)pages * sizeof(InkRec), s));   // the pages' sums start at zero
  const dim3 ga((Wcap + kInkTileW - 1) / kInkTileW, (Hcap + kInkRowsH - 1) / kInkRowsH, pages);
  hipLaunchKernelGGL(ink_rows_kernel, ga, dim3(256), 0, s, images, page_bytes, stride, h, w, table, Hcap, Wcap, radius, Hws, recs);
  const dim3 gb((Wcap + kInkTileW - 1) / kInkTileW, (Hcap + kInkTileH - 1) / kInkTileH, pages);
  hipLaunchKernelGGL(ink_local_kernel, gb, dim3(256), 0, s, Hws, h, w, table, Hcap, Wcap, radius, drop, polarity, recs, reinterpret_cast<unsigned long long*>(bits),
                     reinterpret_cast<unsigned long long*>(bitsT));
}

}  // namespace ttr
