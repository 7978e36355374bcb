// Wide words (DESIGN.md "Wide words"): every wide word's frame is profiled on the page's own pixels and cut into n pieces at the gaps between characters.
//
//   in   words [Wn] WideWord: the frame {X0f, Axf, Bxf, Y0f, Ayf, Byf} in 2^-16 px over U = 128 n columns and 32 rows, n (2..16; 1 is accepted), the word's
//        page, its row of the coefficient table and the first of its n - 1 extra rows; the pages as the packers take them (uniform, or the page table)
//   out  coef [rows][8] int64: the n packer rows {1, X0_p, Ax_p, Bx_p, Y0_p, Ay_p, By_p, 0} of the pieces, at the word's row and its extra rows;
//        the side block [Wn][17] int32 cuts | [Wn][2048] u16 profile (columns beyond U are 0)
//
// One workgroup of 256 threads per word.  Threads stride over the U <= 2048 columns; a thread samples its column's 32 nearest pixels (clamped to the page),
// y = R + 2 G + B, and writes q[u] = max - min to LDS.  Integer arithmetic only, so the result is the host rule's (geometry.cpp: wide_profile,
// wide_cuts_from_profile, wide_piece_coef) bit for bit.  The DP over the cuts runs in LDS with a barrier per piece: two int32 rows of 2049 costs,
// double-buffered, and the argmin as width - 64 in a byte [16][2049].  Thread 0 walks back from D[n][U]; then n threads write the coefficient rows.
// LDS: 4096 (q) + 16392 (D) + 32784 (arg) + 68 (cuts) bytes = 53340.
#include "common.h"
#include "kernels.h"
#include "page_table.h"

namespace ttr {

namespace {
constexpr int kNP = 16, kV = 32, kCols = 128, kWLo = 64, kWHi = 192, kMaxU = kNP * kCols, kInf = 0x3fffffff;
}

__global__ __launch_bounds__(256) void wide_cut_kernel(const WideWord* __restrict__ words, int Wn, const uint8_t* __restrict__ images, size_t page_bytes,
                                                       int stride_u, int h_u, int w_u, const PageRow* __restrict__ table, long long* __restrict__ coef,
                                                       int rows, int* __restrict__ side) {
  __shared__ unsigned short q[kMaxU];
  __shared__ int D[2][kMaxU + 1];
  __shared__ unsigned char arg[kNP][kMaxU + 1];
  __shared__ int cuts[kNP + 1];
  const int wi = blockIdx.x, tid = (int)threadIdx.x;
  if (wi >= Wn) return;
  const WideWord W = words[wi];
  const int n = W.n < 1 ? 1 : W.n > kNP ? kNP : W.n;
  const int U = kCols * n;
  const uint8_t* image; int stride, h, w;
  if (table) { const PageRow& r = table[W.page]; image = r.data; stride = r.stride; h = r.h; w = r.w; }
  else { image = images + (size_t)W.page * page_bytes; stride = stride_u; h = h_u; w = w_u; }

  // the profile: columns tid, tid + 256, ...
  for (int u = tid; u < kMaxU; u += 256) {
    int d = 0;
    if (u < U) {
      const long long x = W.f[0] + u * W.f[1] + 32768, y = W.f[3] + u * W.f[4] + 32768;
      int lo = 0, hi = 0;
      for (int v = 0; v < kV; ++v) {
        long long sx = (x + v * W.f[2]) >> 16, sy = (y + v * W.f[5]) >> 16;
        sx = sx < 0 ? 0 : sx > w - 1 ? w - 1 : sx;
        sy = sy < 0 ? 0 : sy > h - 1 ? h - 1 : sy;
        const uint8_t* p = image + (size_t)sy * (size_t)stride + (size_t)sx * 3;
        const int l = (int)p[0] + 2 * (int)p[1] + (int)p[2];
        lo = v == 0 ? l : min(lo, l);
        hi = v == 0 ? l : max(hi, l);
      }
      d = hi - lo;
    }
    q[u] = (unsigned short)d;
  }
  for (int c = tid; c <= kMaxU; c += 256) D[0][c] = c == 0 ? 0 : kInf;
  if (tid <= kNP) cuts[tid] = -1;
  __syncthreads();

  // the cuts: D[j][c] = the cheapest way to end piece j at column c
  for (int j = 1; j <= n; ++j) {
    const int* prev = D[(j - 1) & 1];
    int* cur = D[j & 1];
    const bool last = j == n;
    for (int c = tid; c <= U; c += 256) {
      int best = kInf, bw = kWLo;
      if (last ? c == U : (c >= 1 && c <= U - 1)) {
        const int gap = last ? 0 : (int)q[c - 1] + (int)q[c];
        const int whi = min(kWHi, c);
        for (int wd = kWLo; wd <= whi; ++wd) {
          const int d = prev[c - wd];
          if (d >= kInf) continue;
          const int dev = wd < kCols ? kCols - wd : wd - kCols;
          const int cost = d + 2 * dev + gap;
          if (cost < best) { best = cost; bw = wd; }
        }
      }
      cur[c] = best;
      arg[j - 1][c] = (unsigned char)(bw - kWLo);
    }
    __syncthreads();
  }
  if (tid == 0) {
    int c = U;
    for (int j = n; j >= 1; --j) {
      cuts[j] = c;
      c -= (int)arg[j - 1][c] + kWLo;
      c = c < 0 ? 0 : c;   // (never: the all-128 path exists; keeps the walk inside the table whatever the input)
    }
    cuts[0] = c;
  }
  __syncthreads();

  // the pieces' packer rows, straight into the coefficient table
  if (tid < n) {
    const int c0 = cuts[tid], c1 = cuts[tid + 1];
    const long long wd = c1 - c0;
    const long long Axp = (W.f[1] * wd + 64) >> 7, Ayp = (W.f[4] * wd + 64) >> 7;
    const int row = tid == 0 ? W.row : W.extra + tid - 1;
    if (row >= 0 && row < rows) {
      long long* o = coef + 8 * (size_t)row;
      o[0] = 1;
      o[1] = W.f[0] + W.f[1] * c0 + ((Axp - W.f[1]) >> 1); o[2] = Axp; o[3] = W.f[2];
      o[4] = W.f[3] + W.f[4] * c0 + ((Ayp - W.f[4]) >> 1); o[5] = Ayp; o[6] = W.f[5];
      o[7] = 0;
    }
  }
  int* const out_cuts = side + (size_t)wi * (kNP + 1);
  unsigned* const out_q = reinterpret_cast<unsigned*>(side + (size_t)Wn * (kNP + 1)) + (size_t)wi * (kMaxU / 2);
  if (tid <= kNP) out_cuts[tid] = cuts[tid];
  for (int k = tid; k < kMaxU / 2; k += 256) out_q[k] = (unsigned)q[2 * k] | ((unsigned)q[2 * k + 1] << 16);
}

void launch_wide_cut(const WideWord* words, int Wn, const uint8_t* images, size_t page_bytes, int stride, int h, int w, const PageRow* table, int64_t* coef,
                     int rows, int* side, hipStream_t s) {
  if (Wn <= 0) return;
  if (!words || !coef || !side || rows <= 0 || (!table && (!images || stride <= 0 || h <= 0 || w <= 0))) throw std::runtime_error("wide_cut: bad arguments");
  hipLaunchKernelGGL(wide_cut_kernel, dim3(Wn), dim3(256), 0, s, words, Wn, images, page_bytes, stride, h, w, table, reinterpret_cast<long long*>(coef), rows, side);
}

}  // namespace ttr
