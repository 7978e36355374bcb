// Curved words (DESIGN.md "Curved words"): the integer steps of the rule, one statement of each, shared by the host rule (geometry.cpp) and
// curve_crop_kernel (curve.hip).  The host walks them in loops, the kernel hands one column or one knot to a thread; every step reads and writes plain
// int32 / int64 arrays (host memory or LDS), so the two agree bit for bit by construction.  tests/curve_ref.py restates them in Python integers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TTR_CURVE_HD __host__ __device__ inline
#else
#define TTR_CURVE_HD inline
#endif

namespace ttr {

constexpr int kCurveU = 128, kCurveV = 64, kCurveS = 8, kCurveK = 9;        // columns, rows, spine segments, knots
constexpr int kCurveInk = 64, kCurveGMin = 16;                              // an ink edge: |dy| above kCurveInk (y = R + 2 G + B, 0..1020); the least G of an inked column
constexpr int kCurveHbMax = kCurveV / 2, kCurveHbCurved = 3 * kCurveV / 8;  // the cap of a half band; the largest half band (frame rows) a curved word may have
constexpr int kCurveRowMax = (kCurveV - 1) * 256, kCurveMid = (kCurveV - 1) * 128;   // spine rows live in [0, V - 1]; the band's middle row, in 1/256 row

// floor(sqrt(x)), x >= 0
TTR_CURVE_HD int64_t curve_isqrt(int64_t x) {
  uint64_t v = (uint64_t)x, r = 0, bit = (uint64_t)1 << 62;
  while (bit > v) bit >>= 2;
  while (bit) {
    if (v >= r + bit) { v -= r + bit; r = (r >> 1) + bit; }
    else r >>= 1;
    bit >>= 2;
  }
  return (int64_t)r;
}

// one row of one column, both passes: the page position in 2^-16 px of row v (-1..V) of column u.  table null: the frame {X0, Ax, Bx, Y0, Ay, By};
// else the band of a knot table [K][4] = {Cx, Cy, Hx, Hy}: C(u) + ((2 v + 1 - V) H(u)) >> 6, C and H linear between the knots at half-column 2 u + 1
struct CurveColumn { int64_t x0, y0, dx, dy; bool band; };
TTR_CURVE_HD CurveColumn curve_column(const int64_t* frame, const int64_t* table, int u) {
  CurveColumn c;
  if (!table) {
    c.x0 = frame[0] + u * frame[1]; c.y0 = frame[3] + u * frame[4]; c.dx = frame[2]; c.dy = frame[5]; c.band = false;
  } else {
    const int k = 2 * u + 1, j = k >> 5, f = k & 31;
    const int64_t* a = table + 4 * j;
    c.x0 = (a[0] * (32 - f) + a[4] * f) >> 5; c.y0 = (a[1] * (32 - f) + a[5] * f) >> 5;
    c.dx = (a[2] * (32 - f) + a[6] * f) >> 5; c.dy = (a[3] * (32 - f) + a[7] * f) >> 5; c.band = true;
  }
  return c;
}
TTR_CURVE_HD void curve_column_at(const CurveColumn& c, int v, int64_t* x, int64_t* y) {
  if (c.band) { *x = c.x0 + (((2 * v + 1 - kCurveV) * c.dx) >> 6); *y = c.y0 + (((2 * v + 1 - kCurveV) * c.dy) >> 6); }
  else { *x = c.x0 + v * c.dx; *y = c.y0 + v * c.dy; }
}

// the statistics of one column from its V + 2 luma values taken one at a time: edge e (0..V) lies between rows e - 1 and e
struct CurveAcc { int32_t G, M, first, last, prev; };
TTR_CURVE_HD void curve_acc_step(CurveAcc& a, int v, int32_t y) {   // v = -1..V in order
  if (v == -1) { a.G = 0; a.M = 0; a.first = -1; a.last = -1; a.prev = y; return; }
  const int32_t g = y > a.prev ? y - a.prev : a.prev - y;
  if (g > kCurveInk) {   // an ink edge; weaker steps (paper grain, noise) count for nothing
    a.G += g; a.M += (2 * v + 1) * g;
    if (a.first < 0) a.first = v;
    a.last = v;
  }
  a.prev = y;
}

// a column is inked when it has an ink edge and a quarter of the mean column's gradient; it is valid when its ink is at least half as tall as the tallest
TTR_CURVE_HD int32_t curve_ink_threshold(int64_t gsum) { const int64_t t = gsum >> 9; return (int32_t)(t < kCurveGMin ? kCurveGMin : t); }
TTR_CURVE_HD bool curve_inked(int32_t G, int32_t first, int32_t thr) { return G >= thr && first >= 0; }
TTR_CURVE_HD bool curve_valid(bool inked, int32_t first, int32_t last, int32_t emax) { return inked && 2 * (last - first) >= emax; }

// window j: the mean row r (1/256 row) and mean column t (1/16 column) of the valid columns within 16 columns of knot j; own = it holds one
TTR_CURVE_HD void curve_window(int j, const int32_t* G, const int32_t* M, const uint8_t* valid, int32_t* r, int32_t* t, int32_t* own) {
  int64_t sg = 0, sm = 0, su = 0;
  const int lo = 16 * j - 16 < 0 ? 0 : 16 * j - 16, hi = 16 * j + 16 > kCurveU ? kCurveU : 16 * j + 16;
  for (int u = lo; u < hi; ++u)
    if (valid[u]) { sg += G[u]; sm += M[u]; su += (int64_t)G[u] * (2 * u + 1); }
  if (sg > 0) { r[j] = (int32_t)((128 * sm) / sg - 256); t[j] = (int32_t)((8 * su) / sg); own[j] = 1; }
  else { r[j] = 0; t[j] = 0; own[j] = 0; }
}

// knot j of a window that holds a column: its mean carried from its mean column to the knot along the neighbouring windows' slope
TTR_CURVE_HD int32_t curve_carry(int j, const int32_t* r, const int32_t* t, const int32_t* own) {
  const int a = j > 0 && own[j - 1] ? j - 1 : j, b = j < kCurveK - 1 && own[j + 1] ? j + 1 : j;
  int64_t s = r[j];
  if (t[b] > t[a]) s += ((int64_t)(256 * j - t[j]) * (int64_t)(r[b] - r[a])) / (int64_t)(t[b] - t[a]);   // (truncates toward zero)
  return (int32_t)(s < 0 ? 0 : s > kCurveRowMax ? kCurveRowMax : s);
}

// knot j of a window that holds none: the nearest knot that does, the lower one on a tie (some knot does)
TTR_CURVE_HD int32_t curve_fill(int j, const int32_t* carried, const int32_t* own) {
  for (int d = 0; d < kCurveK; ++d) {
    if (j - d >= 0 && own[j - d]) return carried[j - d];
    if (j + d < kCurveK && own[j + d]) return carried[j + d];
  }
  return 0;
}

TTR_CURVE_HD int32_t curve_spine_at(const int32_t* spine, int u) {
  const int k = 2 * u + 1, j = k >> 5, f = k & 31;
  return (spine[j] * (32 - f) + spine[j + 1] * f) >> 5;
}

// how far (1/256 row) an inked column's ink reaches from the spine
TTR_CURVE_HD int32_t curve_reach(const int32_t* spine, int u, int32_t first, int32_t last) {
  const int32_t sp = curve_spine_at(spine, u), up = sp - (2 * first - 1) * 128, down = (2 * last - 1) * 128 - sp;
  return up > down ? up : down;
}
TTR_CURVE_HD int32_t curve_half_band(int32_t reach) { const int32_t hb = ((reach < 0 ? 0 : reach) + 255) / 256 + 1; return hb > kCurveHbMax ? kCurveHbMax : hb; }

// pass 1: the centre of knot j, the frame point (16 j - 1/2, spine_j)
TTR_CURVE_HD void curve_centre_frame(const int64_t* frame, int j, int32_t spine_j, int64_t* c2) {
  c2[0] = frame[0] + (((32 * j - 1) * frame[1]) >> 1) + (((int64_t)spine_j * frame[2]) >> 8);
  c2[1] = frame[3] + (((32 * j - 1) * frame[4]) >> 1) + (((int64_t)spine_j * frame[5]) >> 8);
}
// pass 2: the centre of knot j moved along its half-band vector by what the band's spine row differs from the band's middle
TTR_CURVE_HD void curve_centre_band(const int64_t* table1, int j, int32_t spine_j, int64_t* c2) {
  c2[0] = table1[4 * j] + (((int64_t)(spine_j - kCurveMid) * table1[4 * j + 2]) >> 13);
  c2[1] = table1[4 * j + 1] + (((int64_t)(spine_j - kCurveMid) * table1[4 * j + 3]) >> 13);
}

// row j of the knot table from the centres C [K][2]: H_j normal to the spine's tangent (C_{j+1} - C_{j-1}; at the ends the one-sided second-order
// difference), `length` long, on the side the frame's rows run to.  Returns 0 when the tangent has no length (H_j = 0 then).
TTR_CURVE_HD int curve_normal(const int64_t* C, int j, int64_t length, int64_t Bx, int64_t By, int64_t* row4) {
  int64_t tx, ty;
  if (j == 0) { tx = 4 * (C[2] - C[0]) - (C[4] - C[0]); ty = 4 * (C[3] - C[1]) - (C[5] - C[1]); }
  else if (j == kCurveK - 1) { tx = 4 * (C[16] - C[14]) - (C[16] - C[12]); ty = 4 * (C[17] - C[15]) - (C[17] - C[13]); }
  else { tx = C[2 * j + 2] - C[2 * j - 2]; ty = C[2 * j + 3] - C[2 * j - 1]; }
  tx >>= 8; ty >>= 8;
  const int64_t nt = curve_isqrt(tx * tx + ty * ty);
  int64_t px = -ty, py = tx;
  if (px * Bx + py * By < 0) { px = -px; py = -py; }
  row4[0] = C[2 * j]; row4[1] = C[2 * j + 1];
  if (nt == 0) { row4[2] = 0; row4[3] = 0; return 0; }
  row4[2] = (px * length) / nt; row4[3] = (py * length) / nt;
  return 1;
}

// 1 when a centre of the table lies at least length / 2 off the straight line through the first and the last
TTR_CURVE_HD int curve_bent(const int64_t* table, int64_t length) {
  const int64_t ex = (table[32] - table[0]) >> 8, ey = (table[33] - table[1]) >> 8;
  const int64_t ne = curve_isqrt(ex * ex + ey * ey);
  int64_t dev = 0;
  for (int j = 0; j < kCurveK; ++j) {
    int64_t d = ((table[4 * j] - table[0]) >> 8) * ey - ((table[4 * j + 1] - table[1]) >> 8) * ex;
    d = d < 0 ? -d : d;
    dev = d > dev ? d : dev;
  }
  return ne > 0 && 2 * dev >= (length >> 8) * ne ? 1 : 0;
}

// the page position (2^-16 px) that crop pixel (u, v) of a curved word samples
TTR_CURVE_HD void curve_sample_at(const int64_t* table, int u, int v, int64_t* sx, int64_t* sy) {
  const int k = 2 * u + 1, j = k >> 5, f = k & 31;
  const int64_t* a = table + 4 * j;
  const int64_t cx = (a[0] * (32 - f) + a[4] * f) >> 5, cy = (a[1] * (32 - f) + a[5] * f) >> 5;
  const int64_t hx = (a[2] * (32 - f) + a[6] * f) >> 5, hy = (a[3] * (32 - f) + a[7] * f) >> 5;
  *sx = cx + (((2 * v + 1 - 32) * hx) >> 5); *sy = cy + (((2 * v + 1 - 32) * hy) >> 5);
}

}  // namespace ttr
