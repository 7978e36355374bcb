// The ink bitmaps' tile (device code shared by tables.hip and ink.hip): how the pixel passes find a page, and how a workgroup's 256 px x 64 rows of ink bits
// leave it - through LDS once, out as they are (bits) and transposed (bitsT).  One statement, so that every ink rule writes one layout.
#pragma once
#include "common.h"
#include "page_table.h"

namespace ttr {

struct __attribute__((aligned(4))) TabPx4 { uint32_t a, b, c; };   // four pixels

struct TabPage { const uint8_t* data; int h, w, stride; };
__device__ __forceinline__ TabPage tab_page(const uint8_t* images, size_t page_bytes, int stride, int h, int w, const PageRow* table, int pg) {
  if (table) { const PageRow r = table[pg]; return TabPage{r.data, r.h, r.w, r.stride}; }
  return TabPage{images + (size_t)pg * page_bytes, h, w, stride};
}

constexpr int kInkTileW = 256, kInkTileH = 64;

// tile[row][k]: bit b of word k = the ink of pixel (x0 + 64 k + b, y0 + row), zero beyond the page.  Called by all 256 threads behind a barrier.
__device__ __forceinline__ void ink_tile_store(const unsigned long long (*tile)[4], int pw, int ph, int pg, int Hcap, int Wcap, unsigned long long* __restrict__ bits,
                                               unsigned long long* __restrict__ bitsT) {
  const int tid = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kInkTileW, y0 = (int)blockIdx.y * kInkTileH;
  const int nwx = (pw + 63) >> 6, nwy = (ph + 63) >> 6;
  {
    const int row = tid >> 2, k = tid & 3, y = y0 + row, wx = (int)blockIdx.x * 4 + k;
    if (y < ph && wx < nwx) bits[(size_t)pg * ((size_t)Hcap * (size_t)((Wcap + 63) >> 6)) + (size_t)y * nwx + wx] = tile[row][k];
  }
  const int x = x0 + tid;
  if (x < pw) {
    const int k = tid >> 6, b = tid & 63;
    unsigned long long col = 0;
    for (int r = 0; r < kInkTileH; ++r) col |= ((tile[r][k] >> b) & 1ull) << r;
    bitsT[(size_t)pg * ((size_t)Wcap * (size_t)((Hcap + 63) >> 6)) + (size_t)x * nwy + (int)blockIdx.y] = col;
  }
}

}  // namespace ttr
