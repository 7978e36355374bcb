// Local ink (DESIGN.md "Local ink"): the adaptive threshold that tables and deskew may take their ink bitmap from, one statement of each step, shared by the
// host rule (geometry.cpp: ink_from_page) and the two kernels (ink.hip).  Integer arithmetic only.  tests/ink_ref.py restates it in numpy.
//   s(x, y) = b0 + b1 + b2                       0..765
//   inverted: polarity 1, or polarity 2 and 2 * (the page's sum of s) < 765 h w (a tie stays dark); then s -> 765 - s everywhere below
//   window   [x - R, x + R] x [y - R, y + R] clipped to the page: n its area, S the sum of s over it (<= 765 * 129^2: 32 bits)
//   ink      s * n * 256 < S * (256 - drop), in 64 bits
// A blank page and an all-black page carry no ink (s n 256 < s n (256 - drop) never holds); a solid region thicker than the window loses its interior; and the
// bitmap of 255 - page under light ink is the bitmap of page under dark ink, bit for bit: the inverted s of 255 - page is 765 - (765 - s) = s.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TTR_INK_HD __host__ __device__ inline
#else
#define TTR_INK_HD inline
#endif

namespace ttr {

constexpr int kInkRadiusMax = 64;
constexpr int kInkDark = 0, kInkLight = 1, kInkAuto = 2;
constexpr int kInkSMax = 765;
// the workspace between the two passes, one uint32 per pixel: the horizontal window sum (< 2^17) below, the pixel's own s (< 2^10) above
constexpr int kInkSShift = 20;
constexpr uint32_t kInkHMask = (1u << kInkSShift) - 1;

// one page's record, as the second kernel and the host rule write it
struct InkRec {
  int32_t radius, drop, polarity, inverted;
  uint64_t sum;          // the page's sum of s, before any inversion
  int32_t w, h;
};
static_assert(sizeof(InkRec) == 32, "the record is 32 bytes on host and device alike");

TTR_INK_HD bool ink_args_ok(int radius, int drop, int polarity) { return radius >= 1 && radius <= kInkRadiusMax && drop >= 1 && drop <= 255 && polarity >= 0 && polarity <= 2; }
// 2: the page's polarity
TTR_INK_HD int ink_inverted(int polarity, uint64_t sum, int h, int w) {
  return polarity == kInkLight || (polarity == kInkAuto && 2 * sum < (uint64_t)kInkSMax * (uint64_t)h * (uint64_t)w) ? 1 : 0;
}
// 3: how many of [p - R, p + R] lie in [0, len)
TTR_INK_HD int ink_span(int p, int R, int len) {
  const int lo = p - R < 0 ? 0 : p - R, hi = p + R > len - 1 ? len - 1 : p + R;
  return hi - lo + 1;
}
// 4: s the pixel's sum, n and S the window's area and sum, all before inversion
TTR_INK_HD bool ink_local(int s, int n, uint32_t S, int drop, int inverted) {
  if (inverted) { s = kInkSMax - s; S = (uint32_t)kInkSMax * (uint32_t)n - S; }
  return (uint64_t)s * (uint64_t)n * 256u < (uint64_t)S * (uint64_t)(256 - drop);
}

}  // namespace ttr
