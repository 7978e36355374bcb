// Text lines (DESIGN.md "Text lines"): the words of every page of a batch grouped into lines, in reading order.
//
//   in   cuv [N][6] int32: per word {c.x, c.y, u.x, u.y, v.x, v.y} in the rule's fixed point (geometry.h: lines_cuv; c = 4 x the centre, u = 2 x the
//        width vector, v = 2 x the height vector, units of 1/16 px), words ordered by page; first [pages + 1]: each page's first word
//   out  the side block [N] int32 line | [N] int32 word | [pages] int32 n_lines: each word's line in line order and its position inside that line
//
// One workgroup per page, the page's words in LDS (28 bytes per word: cuv and a parent; at kLinesMaxWords = 4096 words 112 KB, dynamic).  Integer
// arithmetic only: every product is an int32 x int32 -> int64, so the result is the host rule's (geometry.cpp: lines_from_cuv) bit for bit.
//   1  links: word i tests the words j > i (j runs alike over a wave's lanes, so its LDS reads are broadcasts) and unites linked pairs by hooking the
//      larger root under the smaller (compare-and-swap on the LDS parent, the scheme of ccl_merge_kernel); the root of a line is its smallest member
//      whatever the threads' timing
//   2  every parent becomes the root
//   3  key_i = c_i . U, U the sum of u over the line's members (each word sums its own line: integer sums, any order), kept in the word's v slot
//   4  word_i = the number of line-mates with a smaller (key, index): no sort; the word with rank 0 writes itself into its root's u.x slot
//   5  line_i = the number of lines whose first word has a smaller (c.y, c.x, index) than the first word of i's line; n_lines = the number of firsts
#include "common.h"
#include "kernels.h"

namespace ttr {

namespace {

__device__ __forceinline__ int lg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lg_find(int* parent, int i) {
  int p = lg_load(&parent[i]);
  while (p != i) { i = p; p = lg_load(&parent[i]); }
  return i;
}
__device__ __forceinline__ void lg_union(int* parent, int a, int b) {
  while (true) {
    a = lg_find(parent, a); b = lg_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicCAS(&parent[a], a, b);   // a > b: a root is only ever hooked under a smaller index
    if (old == a) return;
    a = old;                                       // hooked by another thread meanwhile: go on from its new parent
  }
}

__device__ __forceinline__ long long lg_mul(int a, int b) { return (long long)a * (long long)b; }
__device__ __forceinline__ long long lg_abs(long long x) { return x < 0 ? -x : x; }

struct LgWord { int cx, cy, ux, uy, vx, vy; };
__device__ __forceinline__ LgWord lg_word(const int* w) { return LgWord{w[0], w[1], w[2], w[3], w[4], w[5]}; }

// j seen from i's frame (d = c_j - c_i): same band and near
__device__ __forceinline__ bool lg_frame(const LgWord& i, long long uu_i, long long vv_i, long long A_i, const LgWord& j, int dx, int dy) {
  if (lg_abs(lg_mul(dx, i.vx) + lg_mul(dy, i.vy)) > vv_i) return false;
  const long long s = lg_mul(dx, i.ux) + lg_mul(dy, i.uy);
  const long long e = lg_abs(lg_mul(j.ux, i.ux) + lg_mul(j.uy, i.uy)) + lg_abs(lg_mul(j.vx, i.ux) + lg_mul(j.vy, i.uy));
  const long long g0 = s - e - uu_i, g1 = -s - e - uu_i;
  return (g0 > g1 ? g0 : g1) <= 2 * A_i;
}

}  // namespace

__global__ __launch_bounds__(1024) void line_group_kernel(const int* __restrict__ cuv, const int* __restrict__ first, int N, int* __restrict__ side) {
  extern __shared__ __attribute__((aligned(16))) int lg_lds[];
  const int pg = blockIdx.x, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int c0 = first[pg], n = first[pg + 1] - c0;
  int* const W = lg_lds;               // [n][6]
  int* const parent = lg_lds + 6 * n;  // [n]
  int* const line = side + c0;
  int* const word = side + N + c0;
  for (int k = tid; k < 6 * n; k += nt) W[k] = cuv[6 * (size_t)c0 + k];
  for (int i = tid; i < n; i += nt) parent[i] = i;
  __syncthreads();

  // 1: links
  for (int i = tid; i < n; i += nt) {
    const LgWord a = lg_word(W + 6 * i);
    const long long uu = lg_mul(a.ux, a.ux) + lg_mul(a.uy, a.uy), vv = lg_mul(a.vx, a.vx) + lg_mul(a.vy, a.vy);
    const long long A = lg_abs(lg_mul(a.ux, a.vy) - lg_mul(a.uy, a.vx));
    if (uu == 0 || vv == 0 || A == 0) continue;            // links to nothing
    for (int j = (i & ~63) + 1; j < n; ++j) {              // (from the wave's first word on: the same j in every lane)
      if (j <= i) continue;
      const LgWord b = lg_word(W + 6 * j);
      const int dx = b.cx - a.cx, dy = b.cy - a.cy;
      if (lg_abs(lg_mul(dx, a.vx) + lg_mul(dy, a.vy)) > vv) continue;              // same band, i's frame: rejects most pairs
      const long long dot = lg_mul(a.ux, b.ux) + lg_mul(a.uy, b.uy);
      if (dot <= 0 || 64 * lg_abs(lg_mul(a.ux, b.uy) - lg_mul(a.uy, b.ux)) > 17 * dot) continue;   // same direction
      const long long vvj = lg_mul(b.vx, b.vx) + lg_mul(b.vy, b.vy);
      if (vv > 4 * vvj || vvj > 4 * vv) continue;                                  // similar height
      const long long uuj = lg_mul(b.ux, b.ux) + lg_mul(b.uy, b.uy), Aj = lg_abs(lg_mul(b.ux, b.vy) - lg_mul(b.uy, b.vx));
      if (uuj == 0 || vvj == 0 || Aj == 0) continue;
      if (!lg_frame(a, uu, vv, A, b, dx, dy) || !lg_frame(b, uuj, vvj, Aj, a, -dx, -dy)) continue;
      lg_union(parent, i, j);
    }
  }
  __syncthreads();

  // 2: parent -> root (through the v.x slot, which the links no longer need: no find reads a parent another thread is flattening)
  for (int i = tid; i < n; i += nt) W[6 * i + 4] = lg_find(parent, i);
  __syncthreads();
  for (int i = tid; i < n; i += nt) parent[i] = W[6 * i + 4];
  __syncthreads();

  // 3: key = c . U into the v slot (8 bytes at byte 24 i + 16)
  for (int i = tid; i < n; i += nt) {
    const int r = parent[i];
    long long Ux = 0, Uy = 0;
    for (int j = r; j < n; ++j)                            // (the root is the line's smallest member)
      if (parent[j] == r) { Ux += W[6 * j + 2]; Uy += W[6 * j + 3]; }
    *reinterpret_cast<long long*>(W + 6 * i + 4) = (long long)W[6 * i] * Ux + (long long)W[6 * i + 1] * Uy;
  }
  __syncthreads();

  // 4: position inside the line
  for (int i = tid; i < n; i += nt) {
    const int r = parent[i];
    const long long key = *reinterpret_cast<const long long*>(W + 6 * i + 4);
    int cnt = 0;
    for (int j = r; j < n; ++j) {
      if (parent[j] != r) continue;
      const long long kj = *reinterpret_cast<const long long*>(W + 6 * j + 4);
      cnt += (kj < key || (kj == key && j < i)) ? 1 : 0;
    }
    word[i] = cnt;
    W[6 * i + 3] = cnt;                 // (u is no longer needed: u.y = the rank, the root's u.x = the line's first word)
    if (cnt == 0) W[6 * r + 2] = i;
  }
  __syncthreads();

  // 5: the line's place among the lines
  int total = 0;
  for (int i = tid; i < n; i += nt) {
    const int f = W[6 * parent[i] + 2];
    const int fx = W[6 * f], fy = W[6 * f + 1];
    int cnt = 0;
    total = 0;
    for (int j = 0; j < n; ++j) {
      if (W[6 * j + 3] != 0) continue;
      ++total;
      const int jx = W[6 * j], jy = W[6 * j + 1];
      cnt += (jy < fy || (jy == fy && (jx < fx || (jx == fx && j < f)))) ? 1 : 0;
    }
    line[i] = cnt;
  }
  if (tid == 0) side[2 * (size_t)N + pg] = total;   // (thread 0 owns word 0 when the page has one; else 0 lines)
}

void launch_line_group(const int* cuv, const int* first, int pages, int N, int max_words, int* side, hipStream_t s) {
  if (pages <= 0) return;
  if (max_words > kLinesMaxWords) throw std::runtime_error("line_group: a page has " + std::to_string(max_words) + " words, more than " + std::to_string(kLinesMaxWords));
  static PerDeviceOnce once;
  once.run([&] { TTR_HIP_CHECK(hipFuncSetAttribute((const void*)line_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLinesMaxWords * 28)); });
  const int threads = std::min(1024, std::max(64, (max_words + 63) & ~63));
  const size_t lds = (size_t)std::max(max_words, 1) * 28;
  hipLaunchKernelGGL(line_group_kernel, dim3(pages), dim3(threads), lds, s, cuv, first, N, side);
}

}  // namespace ttr
