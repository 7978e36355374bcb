// Deskew (DESIGN.md "Deskew"): the constants, the record and every step of the rule, one statement of each, shared by the host rule (geometry.cpp:
// deskew_from_page) and the two kernels (deskew.hip).  Integer arithmetic only, except for the table of (C, S) pairs, which the host alone forms
// (deskew_consts, geometry.cpp) and hands to the kernels.  tests/deskew_ref.py restates all of it in numpy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TTR_DSK_HD __host__ __device__ inline
#else
#define TTR_DSK_HD inline
#endif

namespace ttr {

constexpr int kDskMaxSlope = 128;                          // candidate slopes are k in -M..M, M in 1..128: a line drops k px per 512 px to the right
constexpr int kDskSlopes = 2 * kDskMaxSlope + 1;           // the (C, S) table's pairs, indexed by k + 128 whatever M is
constexpr int kDskGainLo = 256, kDskGainHi = 65535;        // the gate, in 1/256ths
constexpr int kDskSideCap = 8192;                          // a page side must be below it

// One page's skew record, as the kernels write it and the result carries it.
struct DeskewRec {
  int32_t slope, found;          // the slope the page was turned by (0 = left as it was); the slope of the largest score
  int32_t C, S;                  // llrint(65536 cos), llrint(65536 sin) of `slope`
  int32_t w, h;
  int32_t mode, pad;             // 1 resampled, 0 left as it was
  uint64_t score0, score_found;
};
static_assert(sizeof(DeskewRec) == 48, "the record is 48 bytes on host and device alike");

TTR_DSK_HD bool dsk_args_ok(int max_slope, int gain, int ink) {
  return max_slope >= 1 && max_slope <= kDskMaxSlope && gain >= kDskGainLo && gain <= kDskGainHi && ink >= 1 && ink <= 255;
}

// 2: the row offset of column x under slope k (an arithmetic shift: a floor); ink pixel (x, y) falls into bin y - dsk_off(x, k)
TTR_DSK_HD int dsk_off(int x, int k) { return (x * k + 256) >> 9; }
// ... the bins of an h x w page under slopes up to M are bias + (-bias .. h - 1 + bias): dsk_bins of them
TTR_DSK_HD int dsk_bias(int w, int M) { return (w * M) / 512 + 1; }
TTR_DSK_HD int dsk_bins(int h, int w, int M) { return h + 2 * dsk_bias(w, M); }
// ... the first column past x whose offset differs from x's (k != 0)
TTR_DSK_HD int dsk_next(int x, int k) {
  const int off = dsk_off(x, k);
  return k > 0 ? ((off + 1) * 512 - 256 + k - 1) / k : (256 - off * 512) / (-k) + 1;
}

// 3: the choice.  a (score sa, slope ka) is better than b: the larger score, then the smaller |k|, then the negative k
TTR_DSK_HD bool dsk_better(uint64_t sa, int ka, uint64_t sb, int kb) {
  if (sa != sb) return sa > sb;
  const int aa = ka < 0 ? -ka : ka, ab = kb < 0 ? -kb : kb;
  if (aa != ab) return aa < ab;
  return ka < kb;
}
// ... a * m >= b * g in 128 bits (m, g below 2^16; the scores reach (h w)^2, beyond 2^48)
TTR_DSK_HD bool dsk_gate(uint64_t a, uint32_t m, uint64_t b, uint32_t g) {
  const uint64_t al = (a & 0xffffffffull) * m, ah = (a >> 32) * m + (al >> 32);
  const uint64_t bl = (b & 0xffffffffull) * g, bh = (b >> 32) * g + (bl >> 32);
  if (ah != bh) return ah > bh;
  return (al & 0xffffffffull) >= (bl & 0xffffffffull);
}
TTR_DSK_HD int dsk_slope(int found, uint64_t score_found, uint64_t score0, int gain) {
  return found != 0 && dsk_gate(score_found, 256, score0, (uint32_t)gain) ? found : 0;
}

// 5: the source coordinates of output pixel (x, y) in 1 / 131072 px
TTR_DSK_HD void dsk_source(int C, int S, int w, int h, int x, int y, int64_t* U, int64_t* V) {
  const int64_t dx = 2 * (int64_t)x + 1 - w, dy = 2 * (int64_t)y + 1 - h;
  *U = (int64_t)C * dx - (int64_t)S * dy + 65536 * (int64_t)(w - 1);
  *V = (int64_t)S * dx + (int64_t)C * dy + 65536 * (int64_t)(h - 1);
}
TTR_DSK_HD int dsk_clamp(int64_t v, int n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : (int)v; }
TTR_DSK_HD int dsk_blend(int p00, int p01, int p10, int p11, int fx, int fy) {
  return (p00 * (256 - fx) * (256 - fy) + p01 * fx * (256 - fy) + p10 * (256 - fx) * fy + p11 * fx * fy + 32768) >> 16;
}
// ... one output pixel's three bytes from a page u8 [h][w][3] whose rows are `stride` bytes apart
TTR_DSK_HD void dsk_pixel(const uint8_t* src, int h, int w, int64_t stride, int C, int S, int x, int y, uint8_t* out3) {
  int64_t U, V;
  dsk_source(C, S, w, h, x, y, &U, &V);
  const int fx = (int)((U >> 9) & 255), fy = (int)((V >> 9) & 255);
  const int xa = dsk_clamp(U >> 17, w), xb = dsk_clamp((U >> 17) + 1, w), ya = dsk_clamp(V >> 17, h), yb = dsk_clamp((V >> 17) + 1, h);
  const uint8_t* ra = src + (int64_t)ya * stride;
  const uint8_t* rb = src + (int64_t)yb * stride;
  for (int c = 0; c < 3; ++c) out3[c] = (uint8_t)dsk_blend(ra[3 * xa + c], ra[3 * xb + c], rb[3 * xa + c], rb[3 * xb + c], fx, fy);
}

}  // namespace ttr
