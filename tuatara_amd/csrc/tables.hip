// Tables (DESIGN.md "Tables"): ruling lines found in the pages' own pixels, grouped into tables, each table's grid and merged cells, and every word's cell.
//
// table_ink_kernel   the pixel pass.  pages x tiles of 256 px x 64 rows, 256 threads.  in: the pages as the packers take them (uniform, or the page table).
//                    out: bits [page][h][ceil(w / 64)] uint64, one bit per pixel along x (step 1 of the rule), and bitsT [page][w][ceil(h / 64)], the same bits
//                    along y, for the vertical pass.  A page whose base and row stride are multiples of 4 is read with one 12-byte load per lane - four pixels -
//                    so a wave reads 768 contiguous bytes of a row; the four ink bits of a lane are shifted to their place and OR-ed over 16 lanes (shuffles)
//                    into the row's four words; a wave issues the loads of its 16 rows before it uses the first.  Any other page (a window into a larger image) is read by bytes, a lane a pixel, and __ballot forms the word.
//                    The tile's 64 x 4 words go through LDS once: out as they are, and transposed (thread x collects bit x of the 64 rows).
//                    (ink_tile.h: ink_tile_store - the local rule's ink_local_kernel, ink.hip, leaves its tiles through the same function.)
// table_grid_kernel  everything behind the bitmaps, one workgroup of 1024 threads per page.  First the runs of both directions, by per-line count, block scan and write (the
//                    rule's order, no atomics), into the launch's run lists in global memory; then per direction union-find in LDS by compare-and-swap, the smaller root winning
//                    (the scheme of block_group_kernel); the components' extents and areas by LDS atomics on integers; rulings numbered by a block scan over
//                    the roots.  Then the meet graph by compare-and-swap over the ruling pairs, steps 6 - 7 by one lane through tables_rule.h's tables_grid -
//                    the host rule's own function, on a few hundred rulings at the most - and the words' cells, a thread a word.
//                    LDS: parent | three statistics arrays [8192] each (reused as tables_grid's scratch) | the rulings' parents [512] | 16 wave sums.
// Integer arithmetic only: the outputs are the host rule's (geometry.cpp: tables_from_page) bit for bit.
#include "common.h"
#include "kernels.h"
#include "ink_tile.h"
#include "page_table.h"
#include "tables_rule.h"

namespace ttr {

__global__ __launch_bounds__(256) void table_ink_kernel(const uint8_t* __restrict__ images, size_t page_bytes, int stride_, int h_, int w_, const PageRow* __restrict__ table,
                                                        int Hcap, int Wcap, int ink, unsigned long long* __restrict__ bits, unsigned long long* __restrict__ bitsT) {
  __shared__ unsigned long long tile[kInkTileH][4];
  const int pg = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TabPage P = tab_page(images, page_bytes, stride_, h_, w_, table, pg);
  const int x0 = (int)blockIdx.x * kInkTileW, y0 = (int)blockIdx.y * kInkTileH;
  if (x0 >= P.w || y0 >= P.h) return;                                 // (the launch covers the largest page of a mixed batch)
  const bool wide = (reinterpret_cast<uintptr_t>(P.data) & 3) == 0 && (P.stride & 3) == 0;
  if (wide) {
    // every row's load first, so that the wave's 16 rows are in flight together (one row at a time, a small page runs at one memory latency per row)
    constexpr int kRows = kInkTileH / 4;
    const int px = x0 + 4 * lane;
    const bool whole = px + 3 < P.w;
    TabPx4 v[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int y = y0 + wave * kRows + r;
      v[r] = TabPx4{0xffffffffu, 0xffffffffu, 0xffffffffu};                          // (white: s = 765 is never below 3 ink)
      if (whole && y < P.h) v[r] = *reinterpret_cast<const TabPx4*>(P.data + (size_t)y * (size_t)P.stride + (size_t)x0 * 3 + 12 * lane);   // (3 x0 is a multiple of 4)
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int row = wave * kRows + r, y = y0 + row;
      const TabPx4 q = v[r];
      const int s0 = (q.a & 255) + ((q.a >> 8) & 255) + ((q.a >> 16) & 255), s1 = (q.a >> 24) + (q.b & 255) + ((q.b >> 8) & 255);
      const int s2 = ((q.b >> 16) & 255) + (q.b >> 24) + (q.c & 255), s3 = ((q.c >> 8) & 255) + ((q.c >> 16) & 255) + (q.c >> 24);
      unsigned nib = (tab_ink(s0, ink) ? 1u : 0u) | (tab_ink(s1, ink) ? 2u : 0u) | (tab_ink(s2, ink) ? 4u : 0u) | (tab_ink(s3, ink) ? 8u : 0u);
      if (!whole && y < P.h) {                                                       // the row's ragged end: by bytes
        const uint8_t* rp = P.data + (size_t)y * (size_t)P.stride + (size_t)px * 3;
        for (int k = 0; k < 4; ++k)
          if (px + k < P.w) nib |= tab_ink((int)rp[3 * k] + (int)rp[3 * k + 1] + (int)rp[3 * k + 2], ink) ? 1u << k : 0u;
      }
      unsigned long long w64 = (unsigned long long)nib << (4 * (lane & 15));
      for (int d = 1; d < 16; d <<= 1) w64 |= __shfl_xor(w64, d);
      if ((lane & 15) == 0) tile[row][lane >> 4] = w64;
    }
  } else {
    for (int r = 0; r < kInkTileH / 4; ++r) {
      const int row = wave * (kInkTileH / 4) + r, y = y0 + row;
      if (y >= P.h) { if (lane < 4) tile[row][lane] = 0; continue; }
      const uint8_t* rp = P.data + (size_t)y * (size_t)P.stride + (size_t)x0 * 3;
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + 64 * k + lane;
        bool on = false;
        if (x < P.w) {
          const uint8_t* p = rp + 3 * (64 * k + lane);
          on = tab_ink((int)p[0] + (int)p[1] + (int)p[2], ink);
        }
        const unsigned long long m = __ballot(on);
        if (lane == 0) tile[row][k] = m;
      }
    }
  }
  __syncthreads();
  ink_tile_store(tile, P.w, P.h, pg, Hcap, Wcap, bits, bitsT);   // (ink_tile.h: the layout every ink rule writes)
}

namespace {

constexpr int kTgThreads = 1024;
constexpr int kTgLdsInts = 4 * kTabRunCap + 2 * kTabRulingCap + 16 + 8;
static_assert(4 * kTabRunCap >= kTabScratchInts, "tables_grid's scratch lies over the four run arrays");

__device__ __forceinline__ int tg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int tg_find(int* parent, int i) {
  int p = tg_load(&parent[i]);
  while (p != i) { i = p; p = tg_load(&parent[i]); }
  return i;
}
__device__ __forceinline__ void tg_union(int* parent, int a, int b) {
  while (true) {
    a = tg_find(parent, a); b = tg_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(&parent[a], a, b);   // a > b: a root is only ever hooked under a smaller index
    if (old == a) return;
    a = old;
  }
}

// exclusive scan of one value per thread over the workgroup of 1024; *total = the sum.  Two barriers.
__device__ __forceinline__ int tg_scan(int v, int* wsum, int tid, int* total) {
  const int lane = tid & 63, wv = tid >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int k = 0; k < kTgThreads / 64; ++k) { const int s = wsum[k]; base += k < wv ? s : 0; tot += s; }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// the runs of at least kTabR set bits of one line of nw words (len bits, zero beyond): f(first, last) for each, in order
template <typename F> __device__ __forceinline__ void tg_walk(const unsigned long long* __restrict__ line, int nw, int len, F&& f) {
  int start = -1;
  for (int k = 0; k < nw; ++k) {
    const unsigned long long v = line[k];
    int p = 0;
    while (p < 64) {
      const unsigned long long rest = (start < 0 ? v : ~v) >> p;
      if (!rest) break;
      p += __builtin_ctzll(rest);
      if (start < 0) start = 64 * k + p;
      else { if (64 * k + p - start >= kTabR) f(start, 64 * k + p - 1); start = -1; }
    }
  }
  if (start >= 0 && len - start >= kTabR) f(start, len - 1);
}

}  // namespace

__global__ __launch_bounds__(kTgThreads) void table_grid_kernel(const unsigned long long* __restrict__ bits, const unsigned long long* __restrict__ bitsT, int h_, int w_,
                                                                const PageRow* __restrict__ table, int Hcap, int Wcap, int min_len, const int* __restrict__ centres,
                                                                const int* __restrict__ first, int* runs_all, int* side_all,
                                                                int* items) {
  extern __shared__ __attribute__((aligned(16))) int tg_lds[];
  const int pg = (int)blockIdx.x, tid = (int)threadIdx.x;
  int* const parent = tg_lds;
  int* const S1 = parent + kTabRunCap;
  int* const S2 = S1 + kTabRunCap;
  int* const S3 = S2 + kTabRunCap;
  int* const rparent = S3 + kTabRunCap;
  int* const wsum = rparent + 2 * kTabRulingCap;
  const int h = table ? table[pg].h : h_, w = table ? table[pg].w : w_;
  int* const side = side_all + (size_t)pg * kTabSideInts;
  int* const rul = side + kTabRulings;
  int mode = 1, count[2] = {0, 0}, nruns[2] = {0, 0};

  for (int dir = 0; dir < 2 && mode == 1; ++dir) {
    const unsigned long long* const bm = dir ? bitsT + (size_t)pg * ((size_t)Wcap * (size_t)((Hcap + 63) >> 6)) : bits + (size_t)pg * ((size_t)Hcap * (size_t)((Wcap + 63) >> 6));
    const int lines = dir ? w : h, len = dir ? h : w, nw = (len + 63) >> 6;
    int* const rn = runs_all + ((size_t)pg * 2 + dir) * kTabRunCap * 3;
    // 2: runs
    int n = 0;
    for (int l0 = 0; l0 < lines; l0 += kTgThreads) {
      const int l = l0 + tid;
      int cnt = 0;
      if (l < lines) tg_walk(bm + (size_t)l * nw, nw, len, [&](int, int) { ++cnt; });
      int total;
      int at = n + tg_scan(cnt, wsum, tid, &total);
      if (n + total > kTabRunCap) { mode = -2; break; }                   // (total is the same in every thread)
      if (cnt) tg_walk(bm + (size_t)l * nw, nw, len, [&](int a, int b) { rn[3 * at] = l; rn[3 * at + 1] = a; rn[3 * at + 2] = b; ++at; });
      n += total;
    }
    if (mode != 1) break;
    nruns[dir] = n;
  }
  // (the runs of both directions are counted before any ruling is formed: a page beyond the run cap in either reports -2 whatever its rulings, as on the host)
  for (int dir = 0; dir < 2 && mode == 1; ++dir) {
    const int* const rn = runs_all + ((size_t)pg * 2 + dir) * kTabRunCap * 3;
    const int n = nruns[dir];
    for (int i = tid; i < n; i += kTgThreads) parent[i] = i;
    __syncthreads();                                                      // (the run list, written above, is read below)
    // 3: links to the next line
    for (int i = tid; i < n; i += kTgThreads) {
      const int li = rn[3 * i], a0 = rn[3 * i + 1], a1 = rn[3 * i + 2];
      int lo = i + 1, hi = n;                                             // the first run of a later line
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (rn[3 * mid] > li) hi = mid; else lo = mid + 1; }
      for (int k = lo; k < n && rn[3 * k] == li + 1 && rn[3 * k + 1] <= a1 + 1; ++k)
        if (tab_link(a0, a1, rn[3 * k + 1], rn[3 * k + 2])) tg_union(parent, i, k);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kTgThreads) S1[i] = tg_find(parent, i);   // (through S1: no find reads a parent another thread is flattening)
    __syncthreads();
    for (int i = tid; i < n; i += kTgThreads) { parent[i] = S1[i]; }
    __syncthreads();
    // 4: per root the smallest first, the largest last, the last line; then the area
    for (int i = tid; i < n; i += kTgThreads) { S1[i] = 32768; S2[i] = -1; S3[i] = -1; }
    __syncthreads();
    for (int i = tid; i < n; i += kTgThreads) {
      const int r = parent[i];
      atomicMin(&S1[r], rn[3 * i + 1]); atomicMax(&S2[r], rn[3 * i + 2]); atomicMax(&S3[r], rn[3 * i]);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kTgThreads)
      if (parent[i] == i) { S2[i] |= S3[i] << 16; S3[i] = 0; }            // (both below 32768)
    __syncthreads();
    for (int i = tid; i < n; i += kTgThreads) atomicAdd(&S3[parent[i]], rn[3 * i + 2] - rn[3 * i + 1] + 1);
    __syncthreads();
    int nr = 0;
    for (int i0 = 0; i0 < n; i0 += kTgThreads) {
      const int i = i0 + tid;
      int is = 0, amin = 0, amax = 0, lmax = 0;
      if (i < n && parent[i] == i) {
        amin = S1[i]; amax = S2[i] & 0xffff; lmax = S2[i] >> 16;
        is = tab_is_ruling(amax - amin + 1, lmax - rn[3 * i] + 1, S3[i], min_len) ? 1 : 0;
      }
      int total;
      const int at = nr + tg_scan(is, wsum, tid, &total);
      if (nr + total > kTabRulingCap) { mode = -4; break; }
      if (is) {
        int* q = rul + 6 * ((dir ? count[0] : 0) + at);
        q[0] = dir;
        if (dir == 0) { q[1] = amin; q[2] = rn[3 * i]; q[3] = amax; q[4] = lmax; }
        else { q[1] = rn[3 * i]; q[2] = amin; q[3] = lmax; q[4] = amax; }
        q[5] = -1;
      }
      nr += total;
    }
    count[dir] = nr;
    __syncthreads();                                                      // (the arrays are reused by the next direction)
  }

  if (mode == 1) {
    const int nh = count[0], nv = count[1];
    // 5: the meet graph
    for (int r = tid; r < nh + nv; r += kTgThreads) rparent[r] = r;
    __syncthreads();                                                      // (... and the rulings, written above, are read below)
    for (int t = tid; t < nh * nv; t += kTgThreads) {
      const int a = t / nv, b = nh + t % nv;
      if (tab_meet(rul + 6 * a, rul + 6 * b)) tg_union(rparent, a, b);
    }
    __syncthreads();
    for (int r = tid; r < nh + nv; r += kTgThreads) rul[6 * r + 5] = tg_find(rparent, r);   // (reads only: nothing is flattened)
    __syncthreads();
    if (tid == 0) {   // 6, 7: the host rule's own function
      for (int k = 0; k < kTabHdr; ++k) side[k] = 0;
      side[1] = nh; side[2] = nv; side[5] = nruns[0]; side[6] = nruns[1];
      const int m = tables_grid(side, tg_lds);
      if (m != 1) tables_clear(side, m); else side[0] = 1;
    }
  } else if (tid == 0) {
    tables_clear(side, mode);
  }
  __syncthreads();
  // 8: the words' cells
  for (int i = first[pg] + tid; i < first[pg + 1]; i += kTgThreads) tab_word_cell(side, centres[2 * i], centres[2 * i + 1], items + 2 * (size_t)i);
}

void launch_table_ink(const uint8_t* images, size_t page_bytes, int stride, int h, int w, const PageRow* table, int pages, int Hcap, int Wcap, int ink,
                      uint64_t* bits, uint64_t* bitsT, hipStream_t s) {
  if (pages <= 0) return;
  if (Hcap <= 0 || Wcap <= 0 || Hcap >= 32768 || Wcap >= 32768 || (!table && (h > Hcap || w > Wcap))) throw std::runtime_error("table_ink: a page side outside 1..32767");
  const dim3 grid((Wcap + kInkTileW - 1) / kInkTileW, (Hcap + kInkTileH - 1) / kInkTileH, pages);
  hipLaunchKernelGGL(table_ink_kernel, grid, dim3(256), 0, s, images, page_bytes, stride, h, w, table, Hcap, Wcap, ink, reinterpret_cast<unsigned long long*>(bits),
                     reinterpret_cast<unsigned long long*>(bitsT));
}

void launch_table_grid(const uint64_t* bits, const uint64_t* bitsT, int h, int w, const PageRow* table, int pages, int Hcap, int Wcap, int min_len, const int* centres,
                       const int* first, int* runs, int* side, int* items, hipStream_t s) {
  if (pages <= 0) return;
  static PerDeviceOnce once;
  once.run([&] { TTR_HIP_CHECK(hipFuncSetAttribute((const void*)table_grid_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kTgLdsInts * 4)); });
  hipLaunchKernelGGL(table_grid_kernel, dim3(pages), dim3(kTgThreads), (size_t)kTgLdsInts * 4, s, reinterpret_cast<const unsigned long long*>(bits),
                     reinterpret_cast<const unsigned long long*>(bitsT), h, w, table, Hcap, Wcap, min_len, centres, first, runs, side, items);
}

}  // namespace ttr
