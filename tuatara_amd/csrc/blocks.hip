// Text blocks (DESIGN.md "Text blocks"): the text lines of every page of a batch grouped into blocks, the blocks in reading order.
//
//   in   cuv [N][6] int32 and first [pages + 1]: what line_group_kernel read (lines.hip); lside: its side block [N] line | [N] word | [pages] n_lines,
//        read here on the device, behind it on the same stream
//   out  the side block [N] int32 block | [N] int32 pos | [pages] int32 n_blocks | [pages] int32 mode: per line of the page (indexed within the page's
//        word range; -1 beyond its lines) the rank of its block in reading order and its own rank inside that block
//
// One workgroup per page.  Integer arithmetic only, every product an int32 x int32 -> int64 (the keys of step 4 a 64-bit product), so the result is the
// host rule's (geometry.cpp: blocks_from_lines) bit for bit.  LDS, in ints, M = the launch's largest word count: parent [M] | aux [M] | R [max(6 M,
// 16384)] | the block table [9][512] | the unplaced set [16] | two minima | the block count.  R holds six ints per line - first the sums of step 1,
// then C, D, H - and is reused: D becomes the line's key, the roots' slots become their blocks' boxes, and once the boxes sit in the block table
// R holds the two 512 x 512 bit matrices.  At M = 4096 that is 149 584 bytes of the workgroup's 160 KB.
//   1  descriptors: the words add themselves to their line's count and 64-bit height sums (LDS atomics: integer sums, any order); the line's first
//      and last word give C and D, the sums H
//   2  links: line i tests the lines j > i (j runs alike over a wave's lanes: broadcast reads) and unites linked pairs, the larger root hooked under
//      the smaller by compare-and-swap (the scheme of line_group_kernel); then every parent becomes the root
//   3  key_l = C_l . Hs, Hs the sum of H over the block's lines; pos_l = the number of block-mates with a smaller (key, index): no sort
//   4  boxes: the words min / max themselves into their block's root slot; the roots are numbered by counting
//   5  more than 512 blocks: block = the number of roots with a smaller (y0, x0, root); mode 0.  Else the block table, the ranks by cy and by key,
//      X[b] = the blocks that overlap b in x as a bit row in cy rank ("S lies between A and B" is then a range of bits), P[b] = the blocks that
//      precede b, and the selection: one round per block, every unplaced block whose P row misses the unplaced set bids its key rank (a held
//      block bids 512 more, so a cycle falls to the smallest key), two barriers a round
#include <climits>

#include "common.h"
#include "kernels.h"

namespace ttr {

namespace {

constexpr int kBgRowWords = kBlocksCap / 32;                 // one bit row of a matrix
constexpr int kBgMatrixInts = 2 * kBlocksCap * kBgRowWords;   // X and P
constexpr int kBgTableInts = 9 * kBlocksCap + kBgRowWords + 4;

__host__ __device__ constexpr int bg_region_ints(int M) { return 6 * M > kBgMatrixInts ? 6 * M : kBgMatrixInts; }
__host__ __device__ constexpr int bg_lds_ints(int M) { return 2 * M + bg_region_ints(M) + kBgTableInts; }

__device__ __forceinline__ int bg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int bg_find(int* parent, int i) {
  int p = bg_load(&parent[i]);
  while (p != i) { i = p; p = bg_load(&parent[i]); }
  return i;
}
__device__ __forceinline__ void bg_union(int* parent, int a, int b) {
  while (true) {
    a = bg_find(parent, a); b = bg_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(&parent[a], a, b);   // a > b: a root is only ever hooked under a smaller index
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ long long bg_mul(int a, int b) { return (long long)a * (long long)b; }
__device__ __forceinline__ long long bg_abs(long long x) { return x < 0 ? -x : x; }
__device__ __forceinline__ long long bg_min(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long bg_max(long long a, long long b) { return a > b ? a : b; }
__device__ __forceinline__ int bg_iabs(int x) { return x < 0 ? -x : x; }

struct BgLine { int Cx, Cy, Dx, Dy, Hx, Hy; };
__device__ __forceinline__ BgLine bg_line(const int* r) { return BgLine{r[0], r[1], r[2], r[3], r[4], r[5]}; }

// b seen from a's frame (d = C_b - C_a): overlapping along a's axis (the stacking test is made by the caller)
__device__ __forceinline__ bool bg_overlap(const BgLine& a, long long DDa, const BgLine& b, int dx, int dy) {
  const long long s = bg_mul(dx, a.Dx) + bg_mul(dy, a.Dy), e = bg_abs(bg_mul(b.Dx, a.Dx) + bg_mul(b.Dy, a.Dy));
  return bg_min(DDa, s + e) - bg_max(-DDa, s - e) >= bg_min(DDa, e);
}

}  // namespace

__global__ __launch_bounds__(1024) void block_group_kernel(const int* __restrict__ cuv, const int* __restrict__ first, const int* __restrict__ lside, int N,
                                                           int M, int* __restrict__ side) {
  extern __shared__ __attribute__((aligned(16))) int bg_lds[];
  const int pg = blockIdx.x, pages = (int)gridDim.x, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int c0 = first[pg], nw = min(first[pg + 1] - c0, M);
  const int nl = min(max(lside[2 * (size_t)N + pg], 0), nw);   // (lines never outnumber words)
  int* const parent = bg_lds;
  int* const aux = parent + M;
  int* const R = aux + M;                                      // (an even offset: the 64-bit slots below are aligned)
  int* const tab = R + bg_region_ints(M);
  int *const bx0 = tab, *const bx1 = tab + kBlocksCap, *const by0 = tab + 2 * kBlocksCap, *const bcy = tab + 3 * kBlocksCap, *const cyr = tab + 4 * kBlocksCap,
      *const bycy = tab + 5 * kBlocksCap, *const keyr = tab + 6 * kBlocksCap, *const bykey = tab + 7 * kBlocksCap, *const bord = tab + 8 * kBlocksCap;
  unsigned* const U = reinterpret_cast<unsigned*>(tab + 9 * kBlocksCap);
  int* const slot = tab + 9 * kBlocksCap + kBgRowWords;
  int* const s_nb = slot + 2;
  const int* const wline = lside + c0;
  const int* const wword = lside + N + c0;
  const int* const wc = cuv + 6 * (size_t)c0;
  int* const oblock = side + c0;
  int* const opos = side + N + c0;

  for (int l = nl + tid; l < first[pg + 1] - c0; l += nt) { oblock[l] = -1; opos[l] = -1; }
  if (nl == 0) {
    if (tid == 0) { side[2 * (size_t)N + pg] = 0; side[2 * (size_t)N + pages + pg] = 1; }
    return;
  }

  // 1: descriptors.  R[6 l] = members, [6 l + 1] = first word, [6 l + 2 .. 5] = the 64-bit sums of v; aux[l] = last word
  for (int k = tid; k < 6 * nl; k += nt) R[k] = 0;
  for (int l = tid; l < nl; l += nt) aux[l] = 0;
  __syncthreads();
  for (int i = tid; i < nw; i += nt) {
    const int l = wline[i];
    if ((unsigned)l >= (unsigned)nl) continue;
    atomicAdd(&R[6 * l], 1);
    atomicAdd(reinterpret_cast<unsigned long long*>(R + 6 * l + 2), (unsigned long long)(long long)wc[6 * i + 4]);
    atomicAdd(reinterpret_cast<unsigned long long*>(R + 6 * l + 4), (unsigned long long)(long long)wc[6 * i + 5]);
    if (wword[i] == 0) R[6 * l + 1] = i;
  }
  __syncthreads();
  for (int i = tid; i < nw; i += nt) {
    const int l = wline[i];
    if ((unsigned)l < (unsigned)nl && wword[i] == R[6 * l] - 1) aux[l] = i;
  }
  __syncthreads();
  for (int l = tid; l < nl; l += nt) {
    const int m = max(R[6 * l], 1), f = R[6 * l + 1], e = aux[l];
    const long long Vx = *reinterpret_cast<const long long*>(R + 6 * l + 2), Vy = *reinterpret_cast<const long long*>(R + 6 * l + 4);
    const int ax = wc[6 * f] - wc[6 * f + 2], ay = wc[6 * f + 1] - wc[6 * f + 3];
    const int bx = wc[6 * e] + wc[6 * e + 2], by = wc[6 * e + 1] + wc[6 * e + 3];
    R[6 * l] = ax + bx; R[6 * l + 1] = ay + by; R[6 * l + 2] = bx - ax; R[6 * l + 3] = by - ay;
    R[6 * l + 4] = (int)(Vx / m); R[6 * l + 5] = (int)(Vy / m);   // (truncating, as the host's)
    parent[l] = l;
  }
  __syncthreads();

  // 2: links
  for (int i = tid; i < nl; i += nt) {
    const BgLine a = bg_line(R + 6 * i);
    const long long DD = bg_mul(a.Dx, a.Dx) + bg_mul(a.Dy, a.Dy), HH = bg_mul(a.Hx, a.Hx) + bg_mul(a.Hy, a.Hy);
    if (DD == 0 || HH == 0 || bg_mul(a.Dx, a.Hy) - bg_mul(a.Dy, a.Hx) == 0) continue;   // links to nothing
    for (int j = (i & ~63) + 1; j < nl; ++j) {                                         // (from the wave's first line on: the same j in every lane)
      if (j <= i) continue;
      const BgLine b = bg_line(R + 6 * j);
      const int dx = b.Cx - a.Cx, dy = b.Cy - a.Cy;
      if (bg_abs(bg_mul(dx, a.Hx) + bg_mul(dy, a.Hy)) > 9 * HH) continue;               // stacked, i's frame: rejects most pairs
      const long long dot = bg_mul(a.Dx, b.Dx) + bg_mul(a.Dy, b.Dy);
      if (dot <= 0 || 64 * bg_abs(bg_mul(a.Dx, b.Dy) - bg_mul(a.Dy, b.Dx)) > 17 * dot) continue;   // same direction
      const long long HHj = bg_mul(b.Hx, b.Hx) + bg_mul(b.Hy, b.Hy);
      if (4 * HH > 9 * HHj || 4 * HHj > 9 * HH) continue;                               // similar height
      const long long DDj = bg_mul(b.Dx, b.Dx) + bg_mul(b.Dy, b.Dy);
      if (DDj == 0 || HHj == 0 || bg_mul(b.Dx, b.Hy) - bg_mul(b.Dy, b.Hx) == 0) continue;
      if (bg_abs(bg_mul(dx, b.Hx) + bg_mul(dy, b.Hy)) > 9 * HHj) continue;              // stacked, j's frame
      if (!bg_overlap(a, DD, b, dx, dy) || !bg_overlap(b, DDj, a, -dx, -dy)) continue;
      bg_union(parent, i, j);
    }
  }
  __syncthreads();
  for (int i = tid; i < nl; i += nt) aux[i] = bg_find(parent, i);   // (through aux: no find reads a parent another thread is flattening)
  __syncthreads();
  for (int i = tid; i < nl; i += nt) parent[i] = aux[i];
  __syncthreads();

  // 3: key = C . Hs into the D slot (8 bytes at int 6 i + 2), then the rank among the block-mates
  for (int i = tid; i < nl; i += nt) {
    const int r = parent[i];
    long long Sx = 0, Sy = 0;
    for (int j = r; j < nl; ++j)                                     // (the root is the block's smallest line)
      if (parent[j] == r) { Sx += R[6 * j + 4]; Sy += R[6 * j + 5]; }
    *reinterpret_cast<long long*>(R + 6 * i + 2) = (long long)R[6 * i] * Sx + (long long)R[6 * i + 1] * Sy;
  }
  __syncthreads();
  for (int i = tid; i < nl; i += nt) {
    const int r = parent[i];
    const long long key = *reinterpret_cast<const long long*>(R + 6 * i + 2);
    int cnt = 0;
    for (int j = r; j < nl; ++j) {
      if (parent[j] != r) continue;
      const long long kj = *reinterpret_cast<const long long*>(R + 6 * j + 2);
      cnt += (kj < key || (kj == key && j < i)) ? 1 : 0;
    }
    opos[i] = cnt;
  }
  __syncthreads();

  // 4: boxes in the roots' slots: x0, y0, x1, y1; the roots numbered in index order (aux), their count
  for (int l = tid; l < nl; l += nt)
    if (parent[l] == l) { R[6 * l] = INT_MAX; R[6 * l + 1] = INT_MAX; R[6 * l + 2] = INT_MIN; R[6 * l + 3] = INT_MIN; }
  __syncthreads();
  for (int i = tid; i < nw; i += nt) {
    const int l = wline[i];
    if ((unsigned)l >= (unsigned)nl) continue;
    const int r = parent[l];
    const int* t = wc + 6 * i;
    const int ex = bg_iabs(t[2]) + bg_iabs(t[4]), ey = bg_iabs(t[3]) + bg_iabs(t[5]);
    atomicMin(&R[6 * r], t[0] - ex); atomicMin(&R[6 * r + 1], t[1] - ey);
    atomicMax(&R[6 * r + 2], t[0] + ex); atomicMax(&R[6 * r + 3], t[1] + ey);
  }
  for (int l = tid; l < nl; l += nt) {
    if (parent[l] != l) continue;
    int below = 0, all = 0;
    for (int j = 0; j < nl; ++j) {
      const int is_root = parent[j] == j ? 1 : 0;
      all += is_root;
      below += j < l ? is_root : 0;
    }
    aux[l] = below;
    if (l == 0) *s_nb = all;                                         // (line 0 is always a root)
  }
  __syncthreads();
  const int nb = *s_nb;

  if (nb > kBlocksCap) {   // 5, mode 0: by key alone
    for (int l = tid; l < nl; l += nt) {
      if (parent[l] != l) continue;
      const int y = R[6 * l + 1], x = R[6 * l];
      int cnt = 0;
      for (int j = 0; j < nl; ++j) {
        if (parent[j] != j) continue;
        const int yj = R[6 * j + 1], xj = R[6 * j];
        cnt += (yj < y || (yj == y && (xj < x || (xj == x && j < l)))) ? 1 : 0;
      }
      aux[l] = cnt;
    }
    __syncthreads();
    for (int l = tid; l < nl; l += nt) oblock[l] = aux[parent[l]];
    if (tid == 0) { side[2 * (size_t)N + pg] = nb; side[2 * (size_t)N + pages + pg] = 0; }
    return;
  }

  // 5, mode 1: the block table
  for (int l = tid; l < nl; l += nt) {
    if (parent[l] != l) continue;
    const int b = aux[l];
    bx0[b] = R[6 * l]; by0[b] = R[6 * l + 1]; bx1[b] = R[6 * l + 2]; bcy[b] = R[6 * l + 1] + R[6 * l + 3];
  }
  __syncthreads();
  for (int b = tid; b < nb; b += nt) {   // ranks by (cy, root) and by (y0, x0, root): the table is in root order
    const int cy = bcy[b], y = by0[b], x = bx0[b];
    int rc = 0, rk = 0;
    for (int j = 0; j < nb; ++j) {
      const int cj = bcy[j], yj = by0[j], xj = bx0[j];
      rc += (cj < cy || (cj == cy && j < b)) ? 1 : 0;
      rk += (yj < y || (yj == y && (xj < x || (xj == x && j < b)))) ? 1 : 0;
    }
    cyr[b] = rc; bycy[rc] = b; keyr[b] = rk; bykey[rk] = b;
  }
  __syncthreads();
  const int W = (nb + 31) >> 5;
  unsigned* const X = reinterpret_cast<unsigned*>(R);                              // X[b][w]: bit k = the block of cy rank 32 w + k overlaps b in x
  unsigned* const P = reinterpret_cast<unsigned*>(R) + kBlocksCap * kBgRowWords;   // P[b][w]: bit k = block 32 w + k precedes b
  for (int t = tid; t < nb * kBgRowWords; t += nt) {
    const int b = t / kBgRowWords, w = t % kBgRowWords;
    unsigned bits = 0;
    if (w < W) {
      const int x0 = bx0[b], x1 = bx1[b];
      for (int k = 0; k < 32; ++k) {
        const int r = 32 * w + k;
        if (r >= nb) break;
        const int s = bycy[r];
        bits |= (bx0[s] < x1 && x0 < bx1[s]) ? 1u << k : 0u;
      }
    }
    X[t] = bits;
  }
  __syncthreads();
  for (int t = tid; t < nb * kBgRowWords; t += nt) {
    const int b = t / kBgRowWords, w = t % kBgRowWords;
    unsigned bits = 0;
    if (w < W) {
      const int x0b = bx0[b], x1b = bx1[b], rb = cyr[b];
      for (int k = 0; k < 32; ++k) {
        const int a = 32 * w + k;
        if (a >= nb) break;
        if (a == b) continue;
        const int x0a = bx0[a], x1a = bx1[a], ra = cyr[a];
        bool p = x0a < x1b && x0b < x1a && ra < rb;
        if (!p && x1a <= x0b) {                                      // left of b, unless a block between them in cy spans both
          const int lo = min(ra, rb) + 1, hi = max(ra, rb);          // the ranks strictly between: [lo, hi)
          bool spanned = false;
          if (lo < hi)
            for (int ww = lo >> 5; ww <= (hi - 1) >> 5; ++ww) {
              unsigned m = X[a * kBgRowWords + ww] & X[b * kBgRowWords + ww];
              if (ww == lo >> 5) m &= ~0u << (lo & 31);
              if (ww == hi >> 5) m &= (1u << (hi & 31)) - 1u;
              if (m) { spanned = true; break; }
            }
          p = !spanned;
        }
        bits |= p ? 1u << k : 0u;
      }
    }
    P[t] = bits;
  }
  if (tid < kBgRowWords) {
    const int left = nb - 32 * tid;
    U[tid] = left >= 32 ? ~0u : left > 0 ? (1u << left) - 1u : 0u;
  }
  if (tid == 0) { slot[0] = INT_MAX; slot[1] = INT_MAX; }
  __syncthreads();

  // the selection: thread b owns block b (blockDim.x >= nb: the launch gives min(1024, the word count rounded up to 64) threads)
  bool placed = tid >= nb;
  for (int round = 0; round < nb; ++round) {
    int* const s = slot + (round & 1);
    if (!placed) {
      bool held = false;
      for (int w = 0; w < W; ++w) held = held || (P[tid * kBgRowWords + w] & U[w]) != 0;
      atomicMin(s, keyr[tid] + (held ? kBlocksCap : 0));
    }
    __syncthreads();
    const int pick = bykey[bg_load(s) & (kBlocksCap - 1)];
    if (tid == pick) {
      placed = true;
      bord[pick] = round;
      U[pick >> 5] &= ~(1u << (pick & 31));
      slot[(round + 1) & 1] = INT_MAX;
    }
    __syncthreads();
  }
  for (int l = tid; l < nl; l += nt) oblock[l] = bord[aux[parent[l]]];
  if (tid == 0) { side[2 * (size_t)N + pg] = nb; side[2 * (size_t)N + pages + pg] = 1; }
}

void launch_block_group(const int* cuv, const int* first, const int* lside, int pages, int N, int max_words, int* side, hipStream_t s) {
  if (pages <= 0) return;
  if (max_words > kLinesMaxWords) throw std::runtime_error("block_group: a page has " + std::to_string(max_words) + " words, more than " + std::to_string(kLinesMaxWords));
  static PerDeviceOnce once;
  once.run([&] { TTR_HIP_CHECK(hipFuncSetAttribute((const void*)block_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bg_lds_ints(kLinesMaxWords) * 4)); });
  const int M = std::max(max_words, 1);
  const int threads = std::min(1024, std::max(64, (M + 63) & ~63));
  hipLaunchKernelGGL(block_group_kernel, dim3(pages), dim3(threads), (size_t)bg_lds_ints(M) * 4, s, cuv, first, lside, N, M, side);
}

}  // namespace ttr
