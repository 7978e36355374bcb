// Character boxes (DESIGN.md "Character boxes"): every word's K cells cut from the detector's normalised region map.
//
//   in   map [pages][H2][W2] f32: the region plane binarize_kernel wrote (a per-slot copy of tnorm); coef [N][KT][6] int64: per word and turn
//        {X0, Ax, Bx, Y0, Ay, By} in 2^-16 heat pixels (geometry.h: chars_coef; KT = 1: turn 0 only, KT = 4: the four turns); page_of [N];
//        turns [N] (the chosen turn 0..3, null = 0); K per word from ids [N][26] (|S| of the confidence rule) or from nchars [N]
//   out  the side block [N][27] int32 cuts | [N] int32 mode | [N][128] u8 profile
//
// One workgroup of 128 threads per word.  Thread u samples column u of the 128 x 16 grid (16 loads, clamped to the map) and writes the byte q[u]
// to LDS; from there on integer arithmetic only, so the result is the host rule's (geometry.cpp: chars_cuts_from_profile) bit for bit.  The DP
// over the cuts runs in LDS: thread c - 1 owns column c (1..128), a barrier per character, two rows of 129 costs double-buffered, the argmin
// bytes in [27][129].  Thread 0 walks back from D[K][u1]; threads 0..26 store the cuts, threads 0..31 the profile as 32 words.
#include "common.h"
#include "kernels.h"

namespace ttr {

namespace {
constexpr int kU = 128, kV = 16, kLam = 64, kMaxK = 26, kInf = 0x3fffffff;
}

__global__ __launch_bounds__(128) void char_cut_kernel(const float* __restrict__ map, int H2, int W2, const long long* __restrict__ coef, int KT,
                                                       const int* __restrict__ page_of, const int* __restrict__ turns, const int* __restrict__ ids,
                                                       const int* __restrict__ nchars, int qlow, int N, int* __restrict__ side) {
  __shared__ int q[kU];
  __shared__ int D[2][kU + 1];
  __shared__ unsigned char arg[kMaxK + 1][kU + 1];
  __shared__ int cuts[kMaxK + 1];
  __shared__ int ext[2];
  const int c = blockIdx.x, tid = (int)threadIdx.x;
  if (c >= N) return;
  const int t = turns ? (turns[c] & 3) : 0;
  int K = 0;
  if (nchars) K = nchars[c];
  else
    for (int p = 0; p < 26; ++p) {
      const int id = ids[(size_t)c * 26 + p];
      if (id == 0) break;
      if (id != 88 && id >= 0 && id < 98) ++K;
    }
  K = K < 0 ? 0 : K > kMaxK ? kMaxK : K;

  // the profile: column tid
  {
    const long long* f = coef + ((size_t)c * KT + (KT == 4 ? t : 0)) * 6;
    const float* T = map + (size_t)page_of[c] * H2 * W2;
    const long long x = f[0] + tid * f[1] + 32768, y = f[3] + tid * f[4] + 32768, bx = f[2], by = f[5];
    float P = 0.f;
#pragma unroll
    for (int v = 0; v < kV; ++v) {
      long long sx = (x + v * bx) >> 16, sy = (y + v * by) >> 16;
      sx = sx < 0 ? 0 : sx > W2 - 1 ? W2 - 1 : sx;
      sy = sy < 0 ? 0 : sy > H2 - 1 ? H2 - 1 : sy;
      const float s = T[(size_t)sy * W2 + (size_t)sx];
      P = v == 0 ? s : fmaxf(P, s);
    }
    q[tid] = (int)fminf(fmaxf(P, 0.f) * 255.f, 255.f);
  }
  if (tid <= kMaxK) cuts[tid] = -1;
  if (tid == 0) { ext[0] = kU; ext[1] = 0; }
  __syncthreads();
  if (q[tid] > qlow) { atomicMin(&ext[0], tid); atomicMax(&ext[1], tid + 1); }
  __syncthreads();
  const bool ink = ext[1] > 0;
  const int u0 = ink ? ext[0] : 0, u1 = ink ? ext[1] : kU, L = u1 - u0;
  const int mode = K > 0 && ink && L >= 2 * K ? 1 : 0;

  if (K > 0 && !mode) {
    if (tid <= K) cuts[tid] = 256 * u0 + (256 * L * tid) / K;
  } else if (mode) {
    const int wlo = max(1, L / (2 * K)), whi = min(L, (2 * L + K - 1) / K);
    const int col = tid + 1;                       // this thread's column
    D[0][tid] = kInf;
    if (tid == 0) D[0][kU] = kInf;
    __syncthreads();
    if (tid == 0) D[0][u0] = 0;
    __syncthreads();
    for (int j = 1; j <= K; ++j) {
      const int* prev = D[(j - 1) & 1];
      int best = kInf, bc = 0;
      if (col > u0 && col <= u1) {
        for (int cp = max(u0, col - whi); cp <= col - wlo; ++cp) {
          const int d = prev[cp];
          if (d >= kInf) continue;
          int dev = (col - cp) * K - L;
          dev = dev < 0 ? -dev : dev;
          const int cost = d + (j > 1 ? q[cp - 1] + q[cp] : 0) + (kLam * dev) / L;
          if (cost < best) { best = cost; bc = cp; }
        }
      }
      D[j & 1][col] = best;
      if (tid == 0) D[j & 1][0] = kInf;
      arg[j][col] = (unsigned char)bc;
      __syncthreads();
    }
    if (tid == 0) {
      int cc = u1;
      for (int j = K; j >= 1; --j) { cuts[j] = 256 * cc; cc = arg[j][cc]; }
      cuts[0] = 256 * cc;
    }
  }
  __syncthreads();
  int* const out_cuts = side + (size_t)c * (kMaxK + 1);
  int* const out_mode = side + (size_t)N * (kMaxK + 1) + c;
  unsigned* const out_q = reinterpret_cast<unsigned*>(side + (size_t)N * (kMaxK + 2)) + (size_t)c * (kU / 4);
  if (tid <= kMaxK) out_cuts[tid] = cuts[tid];
  if (tid == 0) *out_mode = mode;
  if (tid < kU / 4) out_q[tid] = (unsigned)q[4 * tid] | ((unsigned)q[4 * tid + 1] << 8) | ((unsigned)q[4 * tid + 2] << 16) | ((unsigned)q[4 * tid + 3] << 24);
}

void launch_char_cut(const float* map, int H2, int W2, const int64_t* coef, int KT, const int* page_of, const int* turns, const int* ids, const int* nchars,
                     int qlow, int N, int* side, hipStream_t s) {
  if (N <= 0) return;
  if (KT != 1 && KT != 4) throw std::runtime_error("char_cut: KT must be 1 or 4");
  if (H2 <= 0 || W2 <= 0 || (!ids && !nchars)) throw std::runtime_error("char_cut: bad arguments");
  hipLaunchKernelGGL(char_cut_kernel, dim3(N), dim3(128), 0, s, map, H2, W2, reinterpret_cast<const long long*>(coef), KT, page_of, turns, ids, nchars, qlow, N, side);
}

}  // namespace ttr
