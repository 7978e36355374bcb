// Curved words (DESIGN.md "Curved words"): every candidate word's spine is found in the page's own pixels, and a word that is curved has its row of the crop
// batch resampled along that spine.
//
//   in   words [N] CurveIn: the frame {X0, Ax, Bx, Y0, Ay, By} in 2^-16 px over 128 columns and 64 rows, the word's page and its row of `crops`; the pages as
//        the packers take them (uniform, or the page table); crops u8 [rows][32][128][3] as the unchanged packer left them
//   out  crops: the rows of the curved words, overwritten; every other row untouched
//        the side block [N] flag | [N][2] hb | [N][2][9] spine | (8-byte aligned) [N][9][4] int64 knot table
//
// One workgroup of 128 threads per word, thread u = column u.  A pass: the thread walks its column over 66 nearest-pixel reads (rows -1..64) and leaves
// G, M, first, last in LDS; the ink threshold, the tallest ink and the band come from LDS atomics on integers (order-free); nine threads form the nine windows
// and knots.  Pass 1 walks the frame's columns, pass 2 the columns of pass 1's band.  Every integer step is curve_rule.h's, the host rule's own (geometry.cpp:
// curve_word), so the outputs agree bit for bit.  No floating point.  LDS: 4 x 512 (statistics) + 128 (valid) + 5 x 36 (windows) + 144 (centres) + 2 x 288
// (tables) + 84 (outputs) + 20 bytes.
#include "common.h"
#include "kernels.h"
#include "page_table.h"
#include "curve_rule.h"

namespace ttr {

namespace {

struct CurveLds {
  int32_t G[kCurveU], M[kCurveU], first[kCurveU], last[kCurveU];
  uint8_t valid[kCurveU];
  int32_t r[kCurveK], t[kCurveK], own[kCurveK], carried[kCurveK], spine[kCurveK];
  int64_t C[kCurveK][2], table1[kCurveK][4], table2[kCurveK][4];
  int32_t out[21];                       // flag | hb[2] | spine[2][9]
  int32_t gsum, emax, reach, ok, pad;
};

struct CurvePage { const uint8_t* image; int stride, h, w; };

// one pass over the frame (table null) or over the band of `table`: leaves s.spine and returns the windows that hold a valid column; *hb = the half band
__device__ __forceinline__ int curve_pass(CurveLds& s, const CurvePage& pg, const int64_t* frame, const int64_t* table, int u, int32_t* hb) {
  if (u == 0) { s.gsum = 0; s.emax = 0; s.reach = 0; }
  const CurveColumn col = curve_column(frame, table, u);
  CurveAcc acc;
  for (int v = -1; v <= kCurveV; ++v) {
    int64_t x, y;
    curve_column_at(col, v, &x, &y);
    long long ix = (x + 32768) >> 16, iy = (y + 32768) >> 16;
    ix = ix < 0 ? 0 : ix > pg.w - 1 ? pg.w - 1 : ix;
    iy = iy < 0 ? 0 : iy > pg.h - 1 ? pg.h - 1 : iy;
    const uint8_t* p = pg.image + (size_t)iy * (size_t)pg.stride + (size_t)ix * 3;
    curve_acc_step(acc, v, (int32_t)p[0] + 2 * (int32_t)p[1] + (int32_t)p[2]);
  }
  s.G[u] = acc.G; s.M[u] = acc.M; s.first[u] = acc.first; s.last[u] = acc.last;
  __syncthreads();                                           // the reset above is ordered before the atomics below
  atomicAdd(&s.gsum, acc.G);                                 // (at most 128 x 66300: int32 holds it)
  __syncthreads();
  const bool inked = curve_inked(acc.G, acc.first, curve_ink_threshold(s.gsum));
  if (inked) atomicMax(&s.emax, acc.last - acc.first);
  __syncthreads();
  s.valid[u] = curve_valid(inked, acc.first, acc.last, s.emax) ? 1 : 0;
  __syncthreads();
  if (u < kCurveK) curve_window(u, s.G, s.M, s.valid, s.r, s.t, s.own);
  __syncthreads();
  int n = 0;
  for (int j = 0; j < kCurveK; ++j) n += s.own[j];
  if (u < kCurveK) { s.carried[u] = s.own[u] ? curve_carry(u, s.r, s.t, s.own) : 0; s.spine[u] = 0; }
  __syncthreads();
  *hb = 0;
  if (n == 0) return 0;                                      // (uniform over the workgroup)
  if (u < kCurveK) s.spine[u] = s.own[u] ? s.carried[u] : curve_fill(u, s.carried, s.own);
  __syncthreads();
  if (inked) atomicMax(&s.reach, curve_reach(s.spine, u, acc.first, acc.last));
  __syncthreads();
  *hb = curve_half_band(s.reach);
  return n;
}

}  // namespace

__global__ __launch_bounds__(128) void curve_crop_kernel(const CurveIn* __restrict__ words, int N, const uint8_t* __restrict__ images, size_t page_bytes,
                                                         int stride_u, int h_u, int w_u, const PageRow* __restrict__ table, uint8_t* __restrict__ crops,
                                                         int rows, int* __restrict__ side) {
  __shared__ CurveLds s;
  const int wi = blockIdx.x, u = (int)threadIdx.x;
  if (wi >= N) return;
  const CurveIn W = words[wi];
  CurvePage pg;
  if (table) { const PageRow& r = table[W.page]; pg.image = r.data; pg.stride = r.stride; pg.h = r.h; pg.w = r.w; }
  else { pg.image = images + (size_t)W.page * page_bytes; pg.stride = stride_u; pg.h = h_u; pg.w = w_u; }
  const int64_t* frame = W.f;

  if (u < 21) s.out[u] = 0;
  if (u < 4 * kCurveK) { (&s.table1[0][0])[u] = 0; (&s.table2[0][0])[u] = 0; }
  if (u == 0) s.ok = 1;
  __syncthreads();

  // pass 1: the frame's columns
  int32_t hb1 = 0, hb2 = 0;
  const int n1 = curve_pass(s, pg, frame, nullptr, u, &hb1);
  if (u < kCurveK) s.out[3 + u] = s.spine[u];
  bool go = n1 >= 3;
  const int64_t L = curve_isqrt(frame[2] * frame[2] + frame[5] * frame[5]);
  if (go) {
    if (u < kCurveK) curve_centre_frame(frame, u, s.spine[u], s.C[u]);
    __syncthreads();
    if (u < kCurveK && !curve_normal(&s.C[0][0], u, (int64_t)hb1 * L, frame[2], frame[5], s.table1[u])) atomicAnd(&s.ok, 0);
    __syncthreads();
    go = s.ok != 0;
  }
  // pass 2: the same measurement over the band of pass 1
  if (go) {
    const int n2 = curve_pass(s, pg, frame, &s.table1[0][0], u, &hb2);
    if (u < kCurveK) s.out[3 + kCurveK + u] = s.spine[u];
    go = n2 >= 3;
  }
  if (go) {
    const int64_t L2 = ((int64_t)hb1 * hb2 * L) >> 5;
    if (u < kCurveK) curve_centre_band(&s.table1[0][0], u, s.spine[u], s.C[u]);
    __syncthreads();
    if (u < kCurveK && !curve_normal(&s.C[0][0], u, L2, frame[2], frame[5], s.table2[u])) atomicAnd(&s.ok, 0);
    __syncthreads();
    if (u == 0) s.out[0] = s.ok != 0 && hb1 * hb2 <= 32 * kCurveHbCurved && curve_bent(&s.table2[0][0], L2);
  }
  if (u == 0) { s.out[1] = hb1; s.out[2] = hb2; }
  __syncthreads();

  // a curved word: its row of the crop batch, resampled along the knot table - four adjacent pixels of a row per thread, three dwords per store
  if (s.out[0] && W.row >= 0 && W.row < rows) {
    uint32_t* o = reinterpret_cast<uint32_t*>(crops + (size_t)W.row * 32 * 128 * 3);
    const int64_t* tb = &s.table2[0][0];
    for (int q = u; q < 32 * 32; q += 128) {
      const int v = q >> 5, u0 = (q & 31) * 4;
      uint8_t px[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int64_t sx, sy;
        curve_sample_at(tb, u0 + k, v, &sx, &sy);
        const long long ix = sx >> 16, iy = sy >> 16;
        const int fx = (int)((sx >> 5) & 2047), fy = (int)((sy >> 5) & 2047);
        const int x0 = (int)(ix < 0 ? 0 : (ix > pg.w - 1 ? pg.w - 1 : ix)), x1 = (int)(ix + 1 < 0 ? 0 : (ix + 1 > pg.w - 1 ? pg.w - 1 : ix + 1));
        const int y0 = (int)(iy < 0 ? 0 : (iy > pg.h - 1 ? pg.h - 1 : iy)), y1 = (int)(iy + 1 < 0 ? 0 : (iy + 1 > pg.h - 1 ? pg.h - 1 : iy + 1));
        const uint8_t* r0 = pg.image + (size_t)y0 * pg.stride;
        const uint8_t* r1 = pg.image + (size_t)y1 * pg.stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int t = (2048 - fx) * r0[x0 * 3 + c] + fx * r0[x1 * 3 + c];
          const int b = (2048 - fx) * r1[x0 * 3 + c] + fx * r1[x1 * 3 + c];
          const int val = ((2048 - fy) * t + fy * b + (1 << 21)) >> 22;
          px[3 * k + c] = (uint8_t)(val > 255 ? 255 : val);
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o[3 * q + k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    }
  }

  // the side block
  if (u == 0) side[wi] = s.out[0];
  if (u < 2) side[(size_t)N + 2 * (size_t)wi + u] = s.out[1 + u];
  if (u < 2 * kCurveK) side[3 * (size_t)N + 2 * kCurveK * (size_t)wi + u] = s.out[3 + u];
  if (u < 4 * kCurveK) {
    long long* tab = reinterpret_cast<long long*>(reinterpret_cast<uint8_t*>(side) + curve_side_table_offset(N));
    tab[4 * kCurveK * (size_t)wi + u] = (&s.table2[0][0])[u];
  }
}

void launch_curve_crop(const CurveIn* words, int N, const uint8_t* images, size_t page_bytes, int stride, int h, int w, const PageRow* table, uint8_t* crops,
                       int rows, int* side, hipStream_t s) {
  if (N <= 0) return;
  if (!words || !crops || !side || rows <= 0 || (!table && (!images || stride <= 0 || h <= 0 || w <= 0))) throw std::runtime_error("curve_crop: bad arguments");
  hipLaunchKernelGGL(curve_crop_kernel, dim3(N), dim3(128), 0, s, words, N, images, page_bytes, stride, h, w, table, crops, rows, side);
}

}  // namespace ttr
