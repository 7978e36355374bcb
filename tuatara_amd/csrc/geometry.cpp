// Host-side geometry and text decoding.  Replaces the OpenCV calls the reference makes
// after connected-component labelling (tuatara.cpp:162-179, :236-274, :416) and its
// Tokenizer (tuatara.cpp:25-117).  float32 throughout where OpenCV is float32.
#include "geometry.h"
#include "curve_rule.h"
#include "tables_rule.h"
#include "deskew_rule.h"
#include "ink_rule.h"
#include "barcodes_rule.h"
#include "marks_rule.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cfloat>
#include <limits>
#include <map>
#include <set>
#include <stdexcept>
#include <cstdio>
#include <cstring>

namespace ttr {

static const double kPi = 3.1415926535897932384626433832795;  // CV_PI

static inline int cv_floor(double v) { int i = (int)v; return i - (v < i); }
static inline int cv_ceil(double v) { int i = (int)v; return i + (v > i); }

void rect_points(const RRect& r, Pt2f pt[4]) {
  double ang = r.angle * kPi / 180.;
  float b = (float)std::cos(ang) * 0.5f;
  float a = (float)std::sin(ang) * 0.5f;
  pt[0].x = r.cx - a * r.h - b * r.w;
  pt[0].y = r.cy + b * r.h - a * r.w;
  pt[1].x = r.cx + a * r.h - b * r.w;
  pt[1].y = r.cy - b * r.h - a * r.w;
  pt[2].x = 2 * r.cx - pt[0].x;
  pt[2].y = 2 * r.cy - pt[0].y;
  pt[3].x = 2 * r.cx - pt[1].x;
  pt[3].y = 2 * r.cy - pt[1].y;
}

void bounding_rect(const RRect& r, int xywh[4]) {
  Pt2f p[4];
  rect_points(r, p);
  float mnx = std::min(std::min(p[0].x, p[1].x), std::min(p[2].x, p[3].x));
  float mny = std::min(std::min(p[0].y, p[1].y), std::min(p[2].y, p[3].y));
  float mxx = std::max(std::max(p[0].x, p[1].x), std::max(p[2].x, p[3].x));
  float mxy = std::max(std::max(p[0].y, p[1].y), std::max(p[2].y, p[3].y));
  xywh[0] = cv_floor(mnx);
  xywh[1] = cv_floor(mny);
  xywh[2] = cv_ceil(mxx) - xywh[0] + 1;
  xywh[3] = cv_ceil(mxy) - xywh[1] + 1;
}

void tesseract_bbox(const RRect& r, float bbox[4]) {
  Pt2f v[4];
  rect_points(r, v);
  float min_x = std::min(std::min(v[0].x, v[1].x), std::min(v[2].x, v[3].x));
  float min_y = std::min(std::min(v[0].y, v[1].y), std::min(v[2].y, v[3].y));
  float max_x = std::max(std::max(v[0].x, v[1].x), std::max(v[2].x, v[3].x));
  float max_y = std::max(std::max(v[0].y, v[1].y), std::max(v[2].y, v[3].y));
  bbox[0] = std::round(min_x); bbox[1] = std::round(min_y); bbox[2] = std::round(max_x); bbox[3] = std::round(max_y);
}

// ---------------------------------------------------------------- rectified crops (DESIGN.md "Rectified crops")
// The side P[s] -> P[s+1] of rect_points runs at r.angle + (s - 1) * 90 degrees (P0 -> P1 is the h side, P1 -> P2 the w side; the
// order P0..P3 is clockwise on screen).  The baseline is the side whose direction, folded, lies in (-45, 45]; a tie at 45 goes to
// the longer side, then to the side at +45.  Every step is exact in double on the float angle, so tests/rectify_ref.py repeats it.
int deskew_quad(const RRect& r, Pt2f quad[4], double coef[6]) {
  Pt2f p[4];
  rect_points(r, p);
  const double a = r.angle;
  const double j = std::isfinite(a) ? std::ceil((a - 45.) / 90.) : 0.;
  const double theta = a - 90. * j;                       // the baseline's direction, in (-45, 45]
  int s = (int)(((1 - (long long)j) % 4 + 4) % 4);
  if (theta == 45.) {                                     // the side at -45 is P[s-1] -> P[s]; even s is an h side, odd s a w side
    const float len_s = (s & 1) ? r.w : r.h, len_m = (s & 1) ? r.h : r.w;
    if (len_m > len_s) s = (s + 3) & 3;
  }
  for (int i = 0; i < 4; ++i) quad[i] = p[(s + i) & 3];
  quad_coef(quad, coef);
  return std::isfinite(a) && std::fmod(a, 90.) == 0. ? 0 : 1;
}

void quad_coef(const Pt2f quad[4], double coef[6]) {
  // A = tr - tl, B = bl - tl; X0 = tl.x + 0.5 A.x / 128 + 0.5 B.x / 32, left to right, one statement per rounding (no contraction)
  const double Ax = ((double)quad[1].x - (double)quad[0].x) / 128., Bx = ((double)quad[3].x - (double)quad[0].x) / 32.;
  const double Ay = ((double)quad[1].y - (double)quad[0].y) / 128., By = ((double)quad[3].y - (double)quad[0].y) / 32.;
  double x0 = (double)quad[0].x + 0.5 * Ax;
  x0 = x0 + 0.5 * Bx;
  double y0 = (double)quad[0].y + 0.5 * Ay;
  y0 = y0 + 0.5 * By;
  coef[0] = x0; coef[1] = Ax; coef[2] = Bx; coef[3] = y0; coef[4] = Ay; coef[5] = By;
}

void deskew_fixed(const double coef[6], int64_t fixed[6]) {
  for (int i = 0; i < 6; ++i) fixed[i] = (int64_t)std::llrint(coef[i] * 65536.);
}

// ---------------------------------------------------------------- regions (DESIGN.md "Regions and per-row character sets")
bool region_quad_ok(const float* q) {
  for (int i = 0; i < 8; ++i) if (!std::isfinite(q[i]) || !(std::fabs(q[i]) < 32768.f)) return false;
  return true;
}

void region_coef(const float* q, int64_t fixed[6]) {
  const Pt2f p[4] = {{q[0], q[1]}, {q[2], q[3]}, {q[4], q[5]}, {q[6], q[7]}};
  double cf[6];
  quad_coef(p, cf);
  deskew_fixed(cf, fixed);
}

void region_bbox(const float* q, float bbox[4]) {
  bbox[0] = bbox[2] = q[0]; bbox[1] = bbox[3] = q[1];
  for (int i = 1; i < 4; ++i) {
    bbox[0] = std::min(bbox[0], q[2 * i]); bbox[1] = std::min(bbox[1], q[2 * i + 1]);
    bbox[2] = std::max(bbox[2], q[2 * i]); bbox[3] = std::max(bbox[3], q[2 * i + 1]);
  }
}

bool region_inside(const float* q, int h, int w) {
  for (int i = 0; i < 4; ++i)
    if (!(q[2 * i] >= -0.5f && q[2 * i] <= (float)w - 0.5f && q[2 * i + 1] >= -0.5f && q[2 * i + 1] <= (float)h - 0.5f)) return false;
  return true;
}

// ---------------------------------------------------------------- wide words (DESIGN.md "Wide words")
bool wide_aspect_ok(float a) { return a == 0.f || (std::isfinite(a) && a >= 2.f && a <= 64.f); }

int wide_plan(const float* q, float max_aspect, int64_t frame[6]) {
  const double Ax = (double)q[2] - (double)q[0], Ay = (double)q[3] - (double)q[1];
  const double Bx = (double)q[6] - (double)q[0], By = (double)q[7] - (double)q[1];
  const double a2 = Ax * Ax + Ay * Ay, b2 = Bx * Bx + By * By;
  int n = 1;
  if (b2 != 0. && max_aspect > 0.f) {
    const double r = std::ceil(std::sqrt(a2 / b2) / (double)max_aspect);
    n = !(r >= 1.) ? 1 : r >= (double)kWideMaxPieces ? kWideMaxPieces : (int)r;
  }
  const double U = (double)(kWideCols * n);
  const double Axf = Ax / U, Bxf = Bx / 32., Ayf = Ay / U, Byf = By / 32.;
  double x0 = (double)q[0] + 0.5 * Axf;
  x0 = x0 + 0.5 * Bxf;
  double y0 = (double)q[1] + 0.5 * Ayf;
  y0 = y0 + 0.5 * Byf;
  const double cf[6] = {x0, Axf, Bxf, y0, Ayf, Byf};
  deskew_fixed(cf, frame);
  return n;
}

void wide_profile(const uint8_t* image, int h, int w, int stride, const int64_t f[6], int n, uint16_t* q) {
  const int U = kWideCols * n;
  for (int u = 0; u < U; ++u) {
    int lo = 0, hi = 0;
    for (int v = 0; v < kWideV; ++v) {
      int64_t ix = (f[0] + u * f[1] + v * f[2] + 32768) >> 16, iy = (f[3] + u * f[4] + v * f[5] + 32768) >> 16;
      ix = ix < 0 ? 0 : ix > w - 1 ? w - 1 : ix;
      iy = iy < 0 ? 0 : iy > h - 1 ? h - 1 : iy;
      const uint8_t* p = image + (size_t)iy * (size_t)stride + (size_t)ix * 3;
      const int y = p[0] + 2 * p[1] + p[2];
      if (v == 0) lo = hi = y;
      else { lo = std::min(lo, y); hi = std::max(hi, y); }
    }
    q[u] = (uint16_t)(hi - lo);
  }
}

void wide_cuts_from_profile(const uint16_t* q, int n, int32_t cuts[17]) {
  for (int i = 0; i <= kWideMaxPieces; ++i) cuts[i] = -1;
  if (n < 1 || n > kWideMaxPieces) return;
  const int U = kWideCols * n;
  std::vector<int32_t> D[2] = {std::vector<int32_t>((size_t)U + 1, kWideInf), std::vector<int32_t>((size_t)U + 1, kWideInf)};
  std::vector<uint8_t> arg((size_t)(n + 1) * ((size_t)U + 1), 0);
  D[0][0] = 0;
  for (int j = 1; j <= n; ++j) {
    const std::vector<int32_t>& prev = D[(j - 1) & 1];
    std::vector<int32_t>& cur = D[j & 1];
    std::fill(cur.begin(), cur.end(), kWideInf);
    for (int c = (j < n ? 1 : U); c <= (j < n ? U - 1 : U); ++c) {
      int32_t best = kWideInf; int bw = kWideWLo;
      const int32_t gap = j < n ? (int32_t)q[c - 1] + (int32_t)q[c] : 0;
      for (int wd = kWideWLo; wd <= kWideWHi && c - wd >= 0; ++wd) {
        const int32_t d = prev[(size_t)(c - wd)];
        if (d >= kWideInf) continue;
        const int32_t cost = d + 2 * std::abs(wd - kWideCols) + gap;
        if (cost < best) { best = cost; bw = wd; }
      }
      cur[(size_t)c] = best;
      arg[(size_t)j * ((size_t)U + 1) + (size_t)c] = (uint8_t)(bw - kWideWLo);
    }
  }
  int c = U;
  for (int j = n; j >= 1; --j) {
    cuts[j] = c;
    c -= (int)arg[(size_t)j * ((size_t)U + 1) + (size_t)c] + kWideWLo;
    if (c < 0) c = 0;   // (never: the all-128 path exists; keeps the walk inside the table whatever the input)
  }
  cuts[0] = c;
}

void wide_piece_coef(const int64_t f[6], int c0, int c1, int64_t row[8]) {
  const int64_t wd = c1 - c0;
  const int64_t Axp = (f[1] * wd + 64) >> 7, Ayp = (f[4] * wd + 64) >> 7;
  row[0] = 1;
  row[1] = f[0] + f[1] * c0 + ((Axp - f[1]) >> 1); row[2] = Axp; row[3] = f[2];
  row[4] = f[3] + f[4] * c0 + ((Ayp - f[4]) >> 1); row[5] = Ayp; row[6] = f[5];
  row[7] = 0;
}

void wide_piece_quads(const float* q, const int32_t* cuts, int n, float* quads) {
  const double U = (double)(kWideCols * n);
  const double tlx = q[0], tly = q[1], blx = q[6], bly = q[7];
  const double Ax = (double)q[2] - tlx, Ay = (double)q[3] - tly, Cx = (double)q[4] - blx, Cy = (double)q[5] - bly;
  for (int j = 0; j < n; ++j) {
    const double t0 = (double)cuts[j] / U, t1 = (double)cuts[j + 1] / U;
    float* o = quads + 8 * (size_t)j;
    o[0] = (float)(tlx + t0 * Ax); o[1] = (float)(tly + t0 * Ay);
    o[2] = (float)(tlx + t1 * Ax); o[3] = (float)(tly + t1 * Ay);
    o[4] = (float)(blx + t1 * Cx); o[5] = (float)(bly + t1 * Cy);
    o[6] = (float)(blx + t0 * Cx); o[7] = (float)(bly + t0 * Cy);
  }
}

bool wide_cuts_valid(const int32_t cuts[17], int n) {
  if (n < 1 || n > kWideMaxPieces || cuts[0] != 0 || cuts[n] != kWideCols * n) return false;
  for (int j = 0; j < n; ++j) {
    const int wd = cuts[j + 1] - cuts[j];
    if (wd < kWideWLo || wd > kWideWHi) return false;
  }
  for (int j = n + 1; j <= kWideMaxPieces; ++j) if (cuts[j] != -1) return false;
  return true;
}

// ---------------------------------------------------------------- curved words (DESIGN.md "Curved words"; the integer steps are curve_rule.h's)
void curve_frame(const float* q, int64_t frame[6]) {
  const double Ax = ((double)q[2] - (double)q[0]) / (double)kCurveU, Bx = ((double)q[6] - (double)q[0]) / (double)kCurveV;
  const double Ay = ((double)q[3] - (double)q[1]) / (double)kCurveU, By = ((double)q[7] - (double)q[1]) / (double)kCurveV;
  double x0 = (double)q[0] + 0.5 * Ax;
  x0 = x0 + 0.5 * Bx;
  double y0 = (double)q[1] + 0.5 * Ay;
  y0 = y0 + 0.5 * By;
  const double cf[6] = {x0, Ax, Bx, y0, Ay, By};
  deskew_fixed(cf, frame);
}

void curve_columns(const uint8_t* image, int h, int w, int stride, const int64_t frame[6], const int64_t* table, int32_t* stats) {
  for (int u = 0; u < kCurveU; ++u) {
    const CurveColumn col = curve_column(frame, table, u);
    CurveAcc acc{};
    for (int v = -1; v <= kCurveV; ++v) {
      int64_t x, y;
      curve_column_at(col, v, &x, &y);
      int64_t ix = (x + 32768) >> 16, iy = (y + 32768) >> 16;
      ix = ix < 0 ? 0 : ix > w - 1 ? w - 1 : ix;
      iy = iy < 0 ? 0 : iy > h - 1 ? h - 1 : iy;
      const uint8_t* p = image + (size_t)iy * (size_t)stride + (size_t)ix * 3;
      curve_acc_step(acc, v, (int32_t)p[0] + 2 * (int32_t)p[1] + (int32_t)p[2]);
    }
    stats[u] = acc.G; stats[kCurveU + u] = acc.M; stats[2 * kCurveU + u] = acc.first; stats[3 * kCurveU + u] = acc.last;
  }
}

// the statistics of one pass -> the nine spine rows and the half band; returns how many windows hold a valid column
static int curve_knots(const int32_t* stats, int32_t spine[9], int32_t* hb) {
  const int32_t *G = stats, *M = stats + kCurveU, *first = stats + 2 * kCurveU, *last = stats + 3 * kCurveU;
  int64_t gsum = 0;
  for (int u = 0; u < kCurveU; ++u) gsum += G[u];
  const int32_t thr = curve_ink_threshold(gsum);
  uint8_t inked[kCurveU], valid[kCurveU];
  int32_t emax = 0;
  for (int u = 0; u < kCurveU; ++u) {
    inked[u] = curve_inked(G[u], first[u], thr);
    if (inked[u]) emax = std::max(emax, last[u] - first[u]);
  }
  for (int u = 0; u < kCurveU; ++u) valid[u] = curve_valid(inked[u] != 0, first[u], last[u], emax);
  int32_t r[kCurveK], t[kCurveK], own[kCurveK], carried[kCurveK];
  int n = 0;
  for (int j = 0; j < kCurveK; ++j) { curve_window(j, G, M, valid, r, t, own); n += own[j]; }
  for (int j = 0; j < kCurveK; ++j) { spine[j] = 0; carried[j] = own[j] ? curve_carry(j, r, t, own) : 0; }
  *hb = 0;
  if (n == 0) return 0;
  for (int j = 0; j < kCurveK; ++j) spine[j] = own[j] ? carried[j] : curve_fill(j, carried, own);
  int32_t reach = 0;
  for (int u = 0; u < kCurveU; ++u)
    if (inked[u]) reach = std::max(reach, curve_reach(spine, u, first[u], last[u]));
  *hb = curve_half_band(reach);
  return n;
}

void curve_word(const uint8_t* image, int h, int w, int stride, const int64_t frame[6], CurveWord* out, int64_t* table1_out) {
  std::memset(out, 0, sizeof(CurveWord));
  int64_t table1[kCurveK][4] = {};
  std::vector<int32_t> stats((size_t)4 * kCurveU);
  int64_t C[kCurveK][2];
  // pass 1: the frame's columns
  curve_columns(image, h, w, stride, frame, nullptr, stats.data());
  const int n1 = curve_knots(stats.data(), out->spine[0], &out->hb[0]);
  int ok = n1 >= 3;
  if (ok) {
    const int64_t L = curve_isqrt(frame[2] * frame[2] + frame[5] * frame[5]);
    for (int j = 0; j < kCurveK; ++j) curve_centre_frame(frame, j, out->spine[0][j], C[j]);
    for (int j = 0; j < kCurveK; ++j) ok &= curve_normal(&C[0][0], j, (int64_t)out->hb[0] * L, frame[2], frame[5], table1[j]);
    if (table1_out) std::memcpy(table1_out, table1, sizeof(table1));
    if (ok) {
      // pass 2: the same measurement over the band of pass 1
      curve_columns(image, h, w, stride, frame, &table1[0][0], stats.data());
      const int n2 = curve_knots(stats.data(), out->spine[1], &out->hb[1]);
      ok = n2 >= 3;
      if (ok) {
        const int64_t L2 = ((int64_t)out->hb[0] * out->hb[1] * L) >> 5;
        for (int j = 0; j < kCurveK; ++j) curve_centre_band(&table1[0][0], j, out->spine[1][j], C[j]);
        for (int j = 0; j < kCurveK; ++j) ok &= curve_normal(&C[0][0], j, L2, frame[2], frame[5], out->table[j]);
        out->flag = ok && out->hb[0] * out->hb[1] <= 32 * kCurveHbCurved && curve_bent(&out->table[0][0], L2);
      }
    }
  } else if (table1_out) {
    std::memset(table1_out, 0, sizeof(table1));
  }
}

void curve_crop(const uint8_t* image, int h, int w, int stride, const int64_t* table, uint8_t* crop) {
  for (int v = 0; v < 32; ++v)
    for (int u = 0; u < kCurveU; ++u) {
      int64_t sx, sy;
      curve_sample_at(table, u, v, &sx, &sy);
      const int64_t ix = sx >> 16, iy = sy >> 16;
      const int fx = (int)((sx >> 5) & 2047), fy = (int)((sy >> 5) & 2047);
      const int64_t x0 = std::min<int64_t>(std::max<int64_t>(ix, 0), w - 1), x1 = std::min<int64_t>(std::max<int64_t>(ix + 1, 0), w - 1);
      const int64_t y0 = std::min<int64_t>(std::max<int64_t>(iy, 0), h - 1), y1 = std::min<int64_t>(std::max<int64_t>(iy + 1, 0), h - 1);
      const uint8_t *r0 = image + (size_t)y0 * (size_t)stride, *r1 = image + (size_t)y1 * (size_t)stride;
      for (int c = 0; c < 3; ++c) {
        const int t = (2048 - fx) * r0[x0 * 3 + c] + fx * r0[x1 * 3 + c];
        const int b = (2048 - fx) * r1[x0 * 3 + c] + fx * r1[x1 * 3 + c];
        const int val = ((2048 - fy) * t + fy * b + (1 << 21)) >> 22;
        crop[((size_t)v * kCurveU + u) * 3 + c] = (uint8_t)(val > 255 ? 255 : val);
      }
    }
}

void curve_outline(const float* q, int flag, const int64_t* table, float* out) {
  for (int j = 0; j < kCurveK; ++j) {
    float* top = out + 2 * j;
    float* bot = out + 2 * (2 * kCurveK - 1 - j);
    if (flag) {
      const int64_t* t = table + 4 * j;
      top[0] = (float)((double)(t[0] - t[2]) / 65536.); top[1] = (float)((double)(t[1] - t[3]) / 65536.);
      bot[0] = (float)((double)(t[0] + t[2]) / 65536.); bot[1] = (float)((double)(t[1] + t[3]) / 65536.);
    } else {
      const double s = (double)j / (double)kCurveS;
      top[0] = (float)((double)q[0] + s * ((double)q[2] - (double)q[0])); top[1] = (float)((double)q[1] + s * ((double)q[3] - (double)q[1]));
      bot[0] = (float)((double)q[6] + s * ((double)q[4] - (double)q[6])); bot[1] = (float)((double)q[7] + s * ((double)q[5] - (double)q[7]));
    }
  }
}

bool curve_word_valid(const CurveWord& w) {
  if (w.flag != 0 && w.flag != 1) return false;
  for (int p = 0; p < 2; ++p) if (w.hb[p] < 0 || w.hb[p] > kCurveHbMax) return false;
  if (w.flag)
    for (int j = 0; j < kCurveK; ++j)
      for (int c = 0; c < 2; ++c)
        for (int sgn = -1; sgn <= 1; sgn += 2) {
          const int64_t px = (w.table[j][c] + sgn * w.table[j][2 + c]) >> 16;
          if (px < (int64_t)INT32_MIN || px > (int64_t)INT32_MAX) return false;
        }
  return true;
}

// ---------------------------------------------------------------- word orientation (DESIGN.md "Word orientation")
void box_edge_quad(int x0, int y0, int x1, int y1, Pt2f quad[4]) {
  const float l = (float)x0 - 0.5f, t = (float)y0 - 0.5f, r = (float)x1 - 0.5f, b = (float)y1 - 0.5f;
  quad[0] = Pt2f{l, t}; quad[1] = Pt2f{r, t}; quad[2] = Pt2f{r, b}; quad[3] = Pt2f{l, b};
}

void turn_coef(const Pt2f quad[4], int turn, int64_t fixed[6]) {
  Pt2f q[4];
  for (int k = 0; k < 4; ++k) q[k] = quad[(k + turn) & 3];
  double cf[6];
  quad_coef(q, cf);
  deskew_fixed(cf, fixed);
}

int text_chars(const int32_t* ids) {   // |S| of the confidence rule: characters before the first EOS (id 0), id 88 and ids outside [0, 98) dropped
  int k = 0;
  for (int p = 0; p < 26; ++p) {
    if (ids[p] == 0) break;
    if (ids[p] != 88 && ids[p] >= 0 && ids[p] < 98) ++k;
  }
  return k;
}

void orient_select(const float* conf, const int32_t* ids, int n, int k, int per_page, int32_t* turns, int32_t* page_turn) {
  int votes[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    int best = 0;
    for (int j = 1; j < k; ++j) if (conf[(size_t)i * k + j] > conf[(size_t)i * k + best]) best = j;
    turns[i] = best;
    if (text_chars(ids + ((size_t)i * k + best) * 26) >= 2) ++votes[best];
  }
  int pt = 0;
  for (int j = 1; j < k; ++j) if (votes[j] > votes[pt]) pt = j;
  const int step = k == 2 ? 2 : 1;   // candidate column -> turn
  for (int i = 0; i < n; ++i) turns[i] = step * (per_page ? pt : turns[i]);
  *page_turn = step * pt;
}

// ---------------------------------------------------------------- text lines (DESIGN.md "Text lines")
bool lines_cuv(const float* q, int32_t cuv[6]) {
  int64_t p[8];
  for (int k = 0; k < 8; ++k) {
    if (!std::isfinite(q[k]) || std::fabs(q[k]) >= 32768.f) return false;
    p[k] = (int64_t)std::llrint(16. * (double)q[k]);
  }
  for (int a = 0; a < 2; ++a) {   // tl = p[0..1], tr = p[2..3], br = p[4..5], bl = p[6..7]
    cuv[a] = (int32_t)(p[a] + p[2 + a] + p[4 + a] + p[6 + a]);
    cuv[2 + a] = (int32_t)((p[2 + a] - p[a]) + (p[4 + a] - p[6 + a]));
    cuv[4 + a] = (int32_t)((p[6 + a] - p[a]) + (p[4 + a] - p[2 + a]));
  }
  return true;
}

namespace {
struct LineWord {
  int64_t cx, cy, ux, uy, vx, vy, uu, vv, A;
  bool ok;
};
inline int64_t iabs64(int64_t x) { return x < 0 ? -x : x; }
// j seen from i's frame: same band and near
inline bool lines_frame(const LineWord& i, const LineWord& j) {
  const int64_t dx = j.cx - i.cx, dy = j.cy - i.cy;
  if (iabs64(dx * i.vx + dy * i.vy) > i.vv) return false;
  const int64_t s = dx * i.ux + dy * i.uy;
  const int64_t e = iabs64(j.ux * i.ux + j.uy * i.uy) + iabs64(j.vx * i.ux + j.vy * i.uy);
  return std::max(s - e - i.uu, -s - e - i.uu) <= 2 * i.A;
}
inline bool lines_link(const LineWord& i, const LineWord& j) {
  if (!i.ok || !j.ok) return false;
  const int64_t dot = i.ux * j.ux + i.uy * j.uy;
  if (dot <= 0 || 64 * iabs64(i.ux * j.uy - i.uy * j.ux) > 17 * dot) return false;
  if (i.vv > 4 * j.vv || j.vv > 4 * i.vv) return false;
  return lines_frame(i, j) && lines_frame(j, i);
}
}  // namespace

void lines_from_cuv(const int32_t* cuv, int n, int32_t* line, int32_t* word, int32_t* n_lines) {
  *n_lines = 0;
  if (n <= 0) return;
  std::vector<LineWord> w((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int32_t* t = cuv + 6 * (size_t)i;
    LineWord& a = w[i];
    a.cx = t[0]; a.cy = t[1]; a.ux = t[2]; a.uy = t[3]; a.vx = t[4]; a.vy = t[5];
    a.uu = a.ux * a.ux + a.uy * a.uy; a.vv = a.vx * a.vx + a.vy * a.vy; a.A = iabs64(a.ux * a.vy - a.uy * a.vx);
    a.ok = a.uu != 0 && a.vv != 0 && a.A != 0;
  }
  std::vector<int> root((size_t)n);   // the smallest member index of each word's line
  for (int i = 0; i < n; ++i) root[i] = i;
  auto find = [&](int i) { while (root[i] != i) { root[i] = root[root[i]]; i = root[i]; } return i; };
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (lines_link(w[i], w[j])) {
        const int a = find(i), b = find(j);
        if (a != b) root[std::max(a, b)] = std::min(a, b);
      }
  for (int i = 0; i < n; ++i) root[i] = find(i);
  std::vector<int64_t> Ux((size_t)n, 0), Uy((size_t)n, 0), key((size_t)n);
  for (int i = 0; i < n; ++i) { Ux[root[i]] += w[i].ux; Uy[root[i]] += w[i].uy; }
  for (int i = 0; i < n; ++i) key[i] = w[i].cx * Ux[root[i]] + w[i].cy * Uy[root[i]];
  std::vector<int> idx((size_t)n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](int a, int b) {   // lines together, each in word order
    if (root[a] != root[b]) return root[a] < root[b];
    if (key[a] != key[b]) return key[a] < key[b];
    return a < b;
  });
  std::vector<int> firsts;           // each line's first word
  for (int k = 0, pos = 0; k < n; ++k) {
    pos = k > 0 && root[idx[k]] == root[idx[k - 1]] ? pos + 1 : 0;
    word[idx[k]] = pos;
    if (pos == 0) firsts.push_back(idx[k]);
  }
  std::sort(firsts.begin(), firsts.end(), [&](int a, int b) {
    if (w[a].cy != w[b].cy) return w[a].cy < w[b].cy;
    if (w[a].cx != w[b].cx) return w[a].cx < w[b].cx;
    return a < b;
  });
  std::vector<int> line_of_root((size_t)n, 0);
  for (size_t l = 0; l < firsts.size(); ++l) line_of_root[root[firsts[l]]] = (int)l;
  for (int i = 0; i < n; ++i) line[i] = line_of_root[root[i]];
  *n_lines = (int32_t)firsts.size();
}

bool lines_reading_order(const int32_t* line, const int32_t* word, int n, int n_lines, int32_t* order, int32_t* line_first) {
  if (n_lines < 0 || n_lines > n) return false;
  std::fill(line_first, line_first + n_lines + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (line[i] < 0 || line[i] >= n_lines) return false;
    line_first[line[i] + 1]++;
  }
  for (int l = 0; l < n_lines; ++l) {
    if (line_first[l + 1] == 0) return false;
    line_first[l + 1] += line_first[l];
  }
  std::fill(order, order + n, -1);
  for (int i = 0; i < n; ++i) {
    if (word[i] < 0 || word[i] >= line_first[line[i] + 1] - line_first[line[i]]) return false;
    int32_t& o = order[line_first[line[i]] + word[i]];
    if (o >= 0) return false;
    o = i;
  }
  return true;
}

// ---------------------------------------------------------------- text blocks (DESIGN.md "Text blocks")
namespace {
struct BlockLine {
  int64_t Cx, Cy, Dx, Dy, Hx, Hy, DD, HH;
  bool ok;
};
// b seen from a's frame: stacked and overlapping along a's axis
inline bool blocks_frame(const BlockLine& a, const BlockLine& b) {
  const int64_t dx = b.Cx - a.Cx, dy = b.Cy - a.Cy;
  if (iabs64(dx * a.Hx + dy * a.Hy) > 9 * a.HH) return false;
  const int64_t s = dx * a.Dx + dy * a.Dy, e = iabs64(b.Dx * a.Dx + b.Dy * a.Dy);
  return std::min(a.DD, s + e) - std::max(-a.DD, s - e) >= std::min(a.DD, e);
}
inline bool blocks_link(const BlockLine& a, const BlockLine& b) {
  if (!a.ok || !b.ok) return false;
  const int64_t dot = a.Dx * b.Dx + a.Dy * b.Dy;
  if (dot <= 0 || 64 * iabs64(a.Dx * b.Dy - a.Dy * b.Dx) > 17 * dot) return false;
  if (4 * a.HH > 9 * b.HH || 4 * b.HH > 9 * a.HH) return false;
  return blocks_frame(a, b) && blocks_frame(b, a);
}
struct BlockBox {
  int32_t x0, y0, x1, y1, root;
  int64_t cy() const { return (int64_t)y0 + y1; }
};
}  // namespace

void blocks_from_lines(const int32_t* cuv, int n, const int32_t* line, const int32_t* word, int n_lines, int32_t* block, int32_t* pos, int32_t* n_blocks,
                       int32_t* mode) {
  *n_blocks = 0;
  *mode = 1;
  std::fill(block, block + std::max(n, 0), -1);
  std::fill(pos, pos + std::max(n, 0), -1);
  if (n <= 0 || n_lines <= 0) return;
  const int nl = n_lines;
  // 1: the lines' descriptors
  std::vector<int> cnt((size_t)nl, 0), fst((size_t)nl, 0), lst((size_t)nl, 0);
  std::vector<int64_t> Vx((size_t)nl, 0), Vy((size_t)nl, 0);
  for (int i = 0; i < n; ++i) { ++cnt[line[i]]; Vx[line[i]] += cuv[6 * (size_t)i + 4]; Vy[line[i]] += cuv[6 * (size_t)i + 5]; }
  for (int i = 0; i < n; ++i) {
    if (word[i] == 0) fst[line[i]] = i;
    if (word[i] == cnt[line[i]] - 1) lst[line[i]] = i;
  }
  std::vector<BlockLine> L((size_t)nl);
  for (int l = 0; l < nl; ++l) {
    const int32_t *f = cuv + 6 * (size_t)fst[l], *e = cuv + 6 * (size_t)lst[l];
    const int64_t ax = (int64_t)f[0] - f[2], ay = (int64_t)f[1] - f[3], bx = (int64_t)e[0] + e[2], by = (int64_t)e[1] + e[3];
    BlockLine& a = L[l];
    a.Cx = ax + bx; a.Cy = ay + by; a.Dx = bx - ax; a.Dy = by - ay;
    a.Hx = Vx[l] / cnt[l]; a.Hy = Vy[l] / cnt[l];      // (truncating)
    a.DD = a.Dx * a.Dx + a.Dy * a.Dy; a.HH = a.Hx * a.Hx + a.Hy * a.Hy;
    a.ok = a.DD != 0 && a.HH != 0 && a.Dx * a.Hy - a.Dy * a.Hx != 0;
  }
  // 2, 3: links -> components, the root the smallest line
  std::vector<int> root((size_t)nl);
  for (int l = 0; l < nl; ++l) root[l] = l;
  auto find = [&](int i) { while (root[i] != i) { root[i] = root[root[i]]; i = root[i]; } return i; };
  for (int i = 0; i < nl; ++i)
    for (int j = i + 1; j < nl; ++j)
      if (blocks_link(L[i], L[j])) {
        const int a = find(i), b = find(j);
        if (a != b) root[std::max(a, b)] = std::min(a, b);
      }
  for (int l = 0; l < nl; ++l) root[l] = find(l);
  // 4: the lines' order inside their block
  std::vector<int64_t> Sx((size_t)nl, 0), Sy((size_t)nl, 0), key((size_t)nl);
  for (int l = 0; l < nl; ++l) { Sx[root[l]] += L[l].Hx; Sy[root[l]] += L[l].Hy; }
  for (int l = 0; l < nl; ++l) key[l] = L[l].Cx * Sx[root[l]] + L[l].Cy * Sy[root[l]];
  std::vector<int> idx((size_t)nl);
  for (int l = 0; l < nl; ++l) idx[l] = l;
  std::sort(idx.begin(), idx.end(), [&](int a, int b) {
    if (root[a] != root[b]) return root[a] < root[b];
    if (key[a] != key[b]) return key[a] < key[b];
    return a < b;
  });
  for (int k = 0, p = 0; k < nl; ++k) {
    p = k > 0 && root[idx[k]] == root[idx[k - 1]] ? p + 1 : 0;
    pos[idx[k]] = p;
  }
  // 5: the blocks' boxes, in root order
  std::vector<int> bix((size_t)nl, -1);
  std::vector<BlockBox> B;
  for (int l = 0; l < nl; ++l)
    if (root[l] == l) { bix[l] = (int)B.size(); B.push_back(BlockBox{INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, l}); }
  for (int i = 0; i < n; ++i) {
    const int32_t* t = cuv + 6 * (size_t)i;
    BlockBox& b = B[bix[root[line[i]]]];
    const int32_t ex = std::abs(t[2]) + std::abs(t[4]), ey = std::abs(t[3]) + std::abs(t[5]);
    b.x0 = std::min(b.x0, t[0] - ex); b.x1 = std::max(b.x1, t[0] + ex);
    b.y0 = std::min(b.y0, t[1] - ey); b.y1 = std::max(b.y1, t[1] + ey);
  }
  const int nb = (int)B.size();
  auto key_less = [&](int a, int b) {
    if (B[a].y0 != B[b].y0) return B[a].y0 < B[b].y0;
    if (B[a].x0 != B[b].x0) return B[a].x0 < B[b].x0;
    return a < b;                                      // (the blocks are in root order)
  };
  std::vector<int> by_key((size_t)nb), rank((size_t)nb);
  for (int b = 0; b < nb; ++b) by_key[b] = b;
  std::sort(by_key.begin(), by_key.end(), key_less);
  *n_blocks = nb;
  if (nb > kBlocksMaxOrdered) {                        // 8: by key alone
    *mode = 0;
    for (int k = 0; k < nb; ++k) rank[by_key[k]] = k;
  } else {
    // 6: precedence.  The blocks ranked by cy: "S lies between A and B" is a range of ranks, so the clause is an AND of two rows of the
    // x-overlap matrix (columns in cy rank) under a range mask
    const int W = (nb + 63) / 64;
    std::vector<int> by_cy((size_t)nb), cyr((size_t)nb);
    for (int b = 0; b < nb; ++b) by_cy[b] = b;
    std::sort(by_cy.begin(), by_cy.end(), [&](int a, int b) { return B[a].cy() != B[b].cy() ? B[a].cy() < B[b].cy() : a < b; });
    for (int k = 0; k < nb; ++k) cyr[by_cy[k]] = k;
    auto xov = [&](int a, int b) { return B[a].x0 < B[b].x1 && B[b].x0 < B[a].x1; };
    std::vector<uint64_t> X((size_t)nb * W, 0), P((size_t)nb * W, 0);   // X[a]: bit cyr[s] = xov(s, a); P[b]: bit a = a precedes b
    for (int a = 0; a < nb; ++a)
      for (int s = 0; s < nb; ++s)
        if (xov(s, a)) X[(size_t)a * W + (cyr[s] >> 6)] |= 1ull << (cyr[s] & 63);
    for (int b = 0; b < nb; ++b)
      for (int a = 0; a < nb; ++a) {
        if (a == b) continue;
        bool p = xov(a, b) && cyr[a] < cyr[b];
        if (!p && B[a].x1 <= B[b].x0) {
          const int lo = std::min(cyr[a], cyr[b]) + 1, hi = std::max(cyr[a], cyr[b]);   // the ranks strictly between: [lo, hi)
          bool spanned = false;
          for (int w = lo >> 6; w <= (hi - 1) >> 6 && lo < hi && !spanned; ++w) {
            uint64_t m = X[(size_t)a * W + w] & X[(size_t)b * W + w];
            if (w == lo >> 6) m &= ~0ull << (lo & 63);
            if (w == hi >> 6) m &= (1ull << (hi & 63)) - 1;
            spanned = m != 0;
          }
          p = !spanned;
        }
        if (p) P[(size_t)b * W + (a >> 6)] |= 1ull << (a & 63);
      }
    // 7: the order
    std::vector<uint64_t> U((size_t)W, 0);             // the unplaced blocks
    for (int b = 0; b < nb; ++b) U[b >> 6] |= 1ull << (b & 63);
    for (int round = 0; round < nb; ++round) {
      int pick = -1, any = -1;
      for (int k = 0; k < nb && pick < 0; ++k) {       // (ascending key)
        const int b = by_key[k];
        if (!(U[b >> 6] >> (b & 63) & 1)) continue;
        if (any < 0) any = b;
        bool held = false;
        for (int w = 0; w < W && !held; ++w) held = (P[(size_t)b * W + w] & U[w]) != 0;
        if (!held) pick = b;
      }
      if (pick < 0) pick = any;                        // a cycle
      rank[pick] = round;
      U[pick >> 6] &= ~(1ull << (pick & 63));
    }
  }
  for (int l = 0; l < nl; ++l) block[l] = rank[bix[root[l]]];
}

// ---------------------------------------------------------------- character boxes (DESIGN.md "Character boxes")
double chars_scale(float ratio) {
  const float ratio_w = 1.f / ratio;
  const float twice = ratio_w * 2.f;
  return 1.0 / (double)twice;
}

bool chars_coef(const float* q, int turn, double k, int64_t fixed[6]) {
  if (!(k > 0.) || !(k <= 1024.)) return false;
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(q[i]) || std::fabs(q[i]) >= 32768.f) return false;
  const float* tl = q + 2 * (turn & 3);
  const float* tr = q + 2 * ((turn + 1) & 3);
  const float* bl = q + 2 * ((turn + 3) & 3);
  for (int a = 0; a < 2; ++a) {   // x, then y: one statement per rounding (no contraction)
    const double A = (double)tr[a] - (double)tl[a], B = (double)bl[a] - (double)tl[a];
    const double Ak = A * k, Bk = B * k;
    const double Au = Ak / (double)kCharsU, Bv = Bk / (double)kCharsV;
    const double hA = 0.5 * Au, hB = 0.5 * Bv;
    double x0 = (double)tl[a] * k;
    x0 = x0 + hA;
    x0 = x0 + hB;
    const double s0 = 65536. * x0, s1 = 65536. * Au, s2 = 65536. * Bv;
    fixed[3 * a] = (int64_t)std::llrint(s0); fixed[3 * a + 1] = (int64_t)std::llrint(s1); fixed[3 * a + 2] = (int64_t)std::llrint(s2);
  }
  return true;
}

void chars_profile(const float* T, int H2, int W2, const int64_t fx[6], uint8_t q[128]) {
  for (int u = 0; u < kCharsU; ++u) {
    float P = 0.f;
    for (int v = 0; v < kCharsV; ++v) {
      const int64_t sx = (fx[0] + u * fx[1] + v * fx[2] + 32768) >> 16, sy = (fx[3] + u * fx[4] + v * fx[5] + 32768) >> 16;
      const int ix = (int)std::min<int64_t>(std::max<int64_t>(sx, 0), W2 - 1), iy = (int)std::min<int64_t>(std::max<int64_t>(sy, 0), H2 - 1);
      const float t = T[(size_t)iy * W2 + ix];
      P = v == 0 ? t : std::fmax(P, t);     // (fmaxf: a NaN loses against a number)
    }
    const float s = std::fmax(P, 0.f) * 255.f;
    q[u] = (uint8_t)(int)std::fmin(s, 255.f);
  }
}

void chars_cuts_from_profile(const uint8_t* q, int K, int qlow, int32_t cuts[27], int32_t* mode) {
  std::fill(cuts, cuts + kCharsMax + 1, -1);
  *mode = 0;
  if (K <= 0) return;
  K = std::min(K, kCharsMax);
  int u0 = -1, u1 = 0;
  for (int u = 0; u < kCharsU; ++u)
    if ((int)q[u] > qlow) { if (u0 < 0) u0 = u; u1 = u + 1; }
  const bool ink = u0 >= 0;
  if (!ink) { u0 = 0; u1 = kCharsU; }
  const int L = u1 - u0;
  if (!ink || L < 2 * K) {                         // the uniform fallback
    for (int j = 0; j <= K; ++j) cuts[j] = 256 * u0 + (256 * L * j) / K;
    return;
  }
  *mode = 1;
  constexpr int32_t kInf = 0x3fffffff;
  const int wlo = std::max(1, L / (2 * K)), whi = std::min(L, (2 * L + K - 1) / K);
  int32_t D[2][kCharsU + 1];
  uint8_t arg[kCharsMax + 1][kCharsU + 1];
  std::fill(D[0], D[0] + kCharsU + 1, kInf);
  D[0][u0] = 0;
  for (int j = 1; j <= K; ++j) {
    const int32_t* prev = D[(j - 1) & 1];
    int32_t* cur = D[j & 1];
    std::fill(cur, cur + kCharsU + 1, kInf);
    for (int c = j == K ? u1 : u0 + 1; c <= u1; ++c) {
      int32_t best = kInf; int bc = 0;
      for (int cp = std::max(u0, c - whi); cp <= c - wlo; ++cp) {
        if (prev[cp] >= kInf) continue;
        const int w = c - cp, dev = w * K - L;
        const int32_t cost = prev[cp] + (j > 1 ? (int)q[cp - 1] + (int)q[cp] : 0) + (kCharsLam * (dev < 0 ? -dev : dev)) / L;
        if (cost < best) { best = cost; bc = cp; }   // (strict: ties go to the smallest c')
      }
      cur[c] = best; arg[j][c] = (uint8_t)bc;
    }
  }
  int c = u1;
  for (int j = K; j >= 1; --j) { cuts[j] = 256 * c; c = arg[j][c]; }
  cuts[0] = 256 * c;
}

void chars_quads_from_cuts(const float* q, int turn, const int32_t* cuts, int K, float* quads, float* bboxes) {
  double p[4][2];
  for (int j = 0; j < 4; ++j) { p[j][0] = q[2 * ((j + turn) & 3)]; p[j][1] = q[2 * ((j + turn) & 3) + 1]; }   // tl', tr', br', bl'
  for (int j = 0; j < K; ++j) {
    const double t0 = (double)cuts[j] / 32768., t1 = (double)cuts[j + 1] / 32768.;
    float* o = quads + 8 * (size_t)j;
    for (int a = 0; a < 2; ++a) {
      const double top = p[1][a] - p[0][a], bot = p[2][a] - p[3][a];
      o[a] = (float)(p[0][a] + t0 * top); o[2 + a] = (float)(p[0][a] + t1 * top);
      o[4 + a] = (float)(p[3][a] + t1 * bot); o[6 + a] = (float)(p[3][a] + t0 * bot);
    }
    float* b = bboxes + 4 * (size_t)j;
    b[0] = std::min(std::min(o[0], o[2]), std::min(o[4], o[6])); b[1] = std::min(std::min(o[1], o[3]), std::min(o[5], o[7]));
    b[2] = std::max(std::max(o[0], o[2]), std::max(o[4], o[6])); b[3] = std::max(std::max(o[1], o[3]), std::max(o[5], o[7]));
  }
}

bool chars_cuts_valid(const int32_t cuts[27], int K) {
  if (K < 0 || K > kCharsMax) return false;
  if (K == 0) { for (int j = 0; j <= kCharsMax; ++j) if (cuts[j] != -1) return false; return true; }
  if (cuts[0] < 0 || cuts[K] > 32768) return false;
  for (int j = 0; j < K; ++j) if (cuts[j + 1] < cuts[j]) return false;
  for (int j = K + 1; j <= kCharsMax; ++j) if (cuts[j] != -1) return false;
  return true;
}

// ---------------------------------------------------------------- convex hull (monotone chain, exact on integer-valued input)
static double cross(const Pt2f& o, const Pt2f& a, const Pt2f& b) {
  return ((double)a.x - o.x) * ((double)b.y - o.y) - ((double)a.y - o.y) * ((double)b.x - o.x);
}

static std::vector<Pt2f> convex_hull(std::vector<Pt2f> p) {
  std::sort(p.begin(), p.end(), [](const Pt2f& a, const Pt2f& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
  p.erase(std::unique(p.begin(), p.end(), [](const Pt2f& a, const Pt2f& b) { return a.x == b.x && a.y == b.y; }), p.end());
  const int n = (int)p.size();
  if (n < 3) return p;
  std::vector<Pt2f> h(2 * n);
  int k = 0;
  for (int i = 0; i < n; ++i) { while (k >= 2 && cross(h[k - 2], h[k - 1], p[i]) <= 0) --k; h[k++] = p[i]; }
  for (int i = n - 2, t = k + 1; i >= 0; --i) { while (k >= t && cross(h[k - 2], h[k - 1], p[i]) <= 0) --k; h[k++] = p[i]; }
  h.resize(k - 1);
  return h;
}

// ---------------------------------------------------------------- rotating calipers (float32, minimum-area mode)
// The four calipers sides are (a,b), (-b,a), (-a,-b), (b,-a); at every step the side
// making the smallest angle with its polygon edge becomes flush with it.  out = corner,
// edge vector 1, edge vector 2.
static void rotating_calipers_min_area(const Pt2f* points, int n, float out[6]) {
  float minarea = FLT_MAX;
  std::vector<float> inv_len(n);
  std::vector<Pt2f> vect(n);
  int left = 0, bottom = 0, right = 0, top = 0;
  int seq[4];
  float orientation = 0.f, base_a, base_b = 0.f;
  Pt2f pt0 = points[0];
  float left_x = pt0.x, right_x = pt0.x, top_y = pt0.y, bottom_y = pt0.y;
  for (int i = 0; i < n; ++i) {
    if (pt0.x < left_x) left_x = pt0.x, left = i;
    if (pt0.x > right_x) right_x = pt0.x, right = i;
    if (pt0.y > top_y) top_y = pt0.y, top = i;
    if (pt0.y < bottom_y) bottom_y = pt0.y, bottom = i;
    Pt2f pt = points[i + 1 < n ? i + 1 : 0];
    double dx = pt.x - pt0.x, dy = pt.y - pt0.y;
    vect[i].x = (float)dx; vect[i].y = (float)dy;
    inv_len[i] = (float)(1. / std::sqrt(dx * dx + dy * dy));
    pt0 = pt;
  }
  {
    double ax = vect[n - 1].x, ay = vect[n - 1].y;
    for (int i = 0; i < n; ++i) {
      double bx = vect[i].x, by = vect[i].y;
      double convexity = ax * by - ay * bx;
      if (convexity != 0) { orientation = convexity > 0 ? 1.f : -1.f; break; }
      ax = bx; ay = by;
    }
  }
  base_a = orientation;
  seq[0] = bottom; seq[1] = right; seq[2] = top; seq[3] = left;
  int best_left = 0, best_bottom = 0;
  float best_a = 1.f, best_b = 0.f, best_w = 0.f, best_h = 0.f;
  for (int k = 0; k < n; ++k) {
    float dp[4] = {
        +base_a * vect[seq[0]].x + base_b * vect[seq[0]].y,
        -base_b * vect[seq[1]].x + base_a * vect[seq[1]].y,
        -base_a * vect[seq[2]].x - base_b * vect[seq[2]].y,
        +base_b * vect[seq[3]].x - base_a * vect[seq[3]].y,
    };
    float maxcos = dp[0] * inv_len[seq[0]];
    int main_element = 0;
    for (int i = 1; i < 4; ++i) {
      float cosalpha = dp[i] * inv_len[seq[i]];
      if (cosalpha > maxcos) { main_element = i; maxcos = cosalpha; }
    }
    {
      int pindex = seq[main_element];
      float lead_x = vect[pindex].x * inv_len[pindex], lead_y = vect[pindex].y * inv_len[pindex];
      switch (main_element) {
        case 0: base_a = lead_x; base_b = lead_y; break;
        case 1: base_a = lead_y; base_b = -lead_x; break;
        case 2: base_a = -lead_x; base_b = -lead_y; break;
        default: base_a = -lead_y; base_b = lead_x; break;
      }
    }
    seq[main_element] += 1;
    if (seq[main_element] == n) seq[main_element] = 0;
    float dx = points[seq[1]].x - points[seq[3]].x, dy = points[seq[1]].y - points[seq[3]].y;
    float width = dx * base_a + dy * base_b;
    dx = points[seq[2]].x - points[seq[0]].x; dy = points[seq[2]].y - points[seq[0]].y;
    float height = -dx * base_b + dy * base_a;
    float area = width * height;
    if (area <= minarea) {
      minarea = area;
      best_left = seq[3]; best_bottom = seq[0];
      best_a = base_a; best_b = base_b; best_w = width; best_h = height;
    }
  }
  float A1 = best_a, B1 = best_b, A2 = -best_b, B2 = best_a;
  float C1 = A1 * points[best_left].x + points[best_left].y * B1;
  float C2 = A2 * points[best_bottom].x + points[best_bottom].y * B2;
  float idet = 1.f / (A1 * B2 - A2 * B1);
  out[0] = (C1 * B2 - C2 * B1) * idet;
  out[1] = (A1 * C2 - A2 * C1) * idet;
  out[2] = A1 * best_w; out[3] = B1 * best_w;
  out[4] = A2 * best_h; out[5] = B2 * best_h;
}

RRect finish_min_area_rect(int kind, const float v[6]) {
  RRect box;
  if (kind == 1) {
    box.cx = v[0] + (v[2] + v[4]) * 0.5f;
    box.cy = v[1] + (v[3] + v[5]) * 0.5f;
    box.w = (float)std::sqrt((double)v[2] * v[2] + (double)v[3] * v[3]);
    box.h = (float)std::sqrt((double)v[4] * v[4] + (double)v[5] * v[5]);
    box.angle = (float)std::atan2((double)v[3], (double)v[2]);
  } else if (kind == 3) {
    box.cx = (v[0] + v[2]) * 0.5f;
    box.cy = (v[1] + v[3]) * 0.5f;
    double dx = v[2] - v[0], dy = v[3] - v[1];
    box.w = (float)std::sqrt(dx * dx + dy * dy);
    box.h = 0;
    box.angle = (float)std::atan2(dy, dx);
  } else if (kind == 4) {
    box.cx = v[0]; box.cy = v[1];
  }
  box.angle = (float)(box.angle * 180 / kPi);
  return box;
}

RRect min_area_rect(const Pt2f* pts, int n) {
  std::vector<Pt2f> hull = convex_hull(std::vector<Pt2f>(pts, pts + n));
  const int hn = (int)hull.size();
  float v[6] = {0, 0, 0, 0, 0, 0};
  if (hn > 2) { rotating_calipers_min_area(hull.data(), hn, v); return finish_min_area_rect(1, v); }
  if (hn == 2) { v[0] = hull[0].x; v[1] = hull[0].y; v[2] = hull[1].x; v[3] = hull[1].y; return finish_min_area_rect(3, v); }
  if (hn == 1) { v[0] = hull[0].x; v[1] = hull[0].y; return finish_min_area_rect(4, v); }
  return finish_min_area_rect(0, v);
}

RRect adjust_coordinates(const RRect& r, float ratio_w, float ratio_h, float ratio_net) {
  Pt2f c[4];
  rect_points(r, c);
  for (int i = 0; i < 4; ++i) { c[i].x *= (ratio_w * ratio_net); c[i].y *= (ratio_h * ratio_net); }
  return min_area_rect(c, 4);
}

bool component_to_rect(const Component& c, int H, int W, RRect* out) {
  const int x = c.x0, y = c.y0, w = c.x1 - c.x0 + 1, h = c.y1 - c.y0 + 1, size = c.area;
  const int niter = (int)std::sqrt((double)(size * std::min(w, h) / (w * h) * 2));  // tuatara.cpp:166, integer inside the sqrt
  const int sx = std::max(0, x - niter), sy = std::max(0, y - niter);               // :168-169
  const int ex = std::min(W, x + w + niter + 1), ey = std::min(H, y + h + niter + 1);  // :170-171
  const int k = 1 + niter, a = k / 2, back = k - 1 - a;  // MORPH_RECT k x k, anchor (k/2,k/2): source s lights [s-back, s+a]
  std::vector<Pt2f> pts;
  pts.reserve(2 * (h + k));
  for (int oy = std::max(sy, y - back); oy <= std::min(ey - 1, y + h - 1 + a); ++oy) {
    int mn = INT_MAX, mx = -1;
    for (int s = std::max(y, oy - a); s <= std::min(y + h - 1, oy + back); ++s) {
      const int* r = c.rows + 2 * (s - y);
      if (r[1] < 0) continue;
      mn = std::min(mn, r[0]); mx = std::max(mx, r[1]);
    }
    if (mx < 0) continue;
    mn = std::max(mn - back, sx); mx = std::min(mx + a, ex - 1);
    pts.push_back(Pt2f{(float)mn, (float)oy});
    if (mx != mn) pts.push_back(Pt2f{(float)mx, (float)oy});
  }
  if (pts.empty()) return false;
  *out = min_area_rect(pts.data(), (int)pts.size());
  return true;
}

CanvasGeom canvas_geometry(int height, int width, int square_size, float mag_ratio) {
  CanvasGeom g;
  float target_size = mag_ratio * std::max(height, width);
  if (target_size > square_size) target_size = (float)square_size;
  g.ratio = target_size / std::max(height, width);
  g.target_h = (int)(height * g.ratio);
  g.target_w = (int)(width * g.ratio);
  g.h32 = g.target_h % 32 != 0 ? g.target_h + (32 - g.target_h % 32) : g.target_h;
  g.w32 = g.target_w % 32 != 0 ? g.target_w + (32 - g.target_w % 32) : g.target_w;
  return g;
}

Tokenizer::Tokenizer() {
  const std::string charset =
      "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ!\"#$%&"
      "\\'()*+,-./:;<=>?@[\\]^_`{|}~";
  itos = charset;
  itos.insert(itos.begin(), ']');
  itos.push_back('[');
  itos.push_back('P');
  std::map<char, size_t> stoi;
  for (size_t i = 0; i < itos.size(); ++i) stoi[itos[i]] = i;  // duplicates: last index wins
  eos_id = (int)stoi[']'];
  bos_id = (int)stoi['['];
  pad_id = (int)stoi['P'];
}

std::string Tokenizer::decode(const int* ids, int n) const {
  std::string s;
  for (int i = 0; i < n; ++i) {
    if (ids[i] == eos_id) continue;
    if (ids[i] < 0 || ids[i] >= (int)itos.size()) continue;
    char ch = itos[ids[i]];
    if (ch == ']') break;
    s.push_back(ch);
  }
  return s;
}

int charset_mask(const Tokenizer& tok, const char* allow, const char* deny, uint32_t mask[3]) {
  constexpr int kClasses = 95;
  auto quote = [](unsigned char ch) {           // ASCII as itself, anything else as \xNN
    char b[16];
    if (ch >= 0x20 && ch < 0x7f) snprintf(b, sizeof b, "'%c'", ch); else snprintf(b, sizeof b, "'\\x%02x'", ch);
    return std::string(b);
  };
  auto classes_of = [&](const char* set, const char* which, bool in[kClasses]) {
    for (int i = 0; i < kClasses; ++i) in[i] = false;
    for (const char* q = set; *q; ++q) {
      bool any = false;
      for (int i = 1; i < kClasses; ++i) if (tok.itos[i] == *q) { in[i] = true; any = true; }
      if (!any) throw std::runtime_error(std::string("charset: ") + which + " holds " + quote((unsigned char)*q) + ", which names no recogniser class");
    }
  };
  const bool has_allow = allow && *allow, has_deny = deny && *deny;
  bool a[kClasses], d[kClasses];
  if (has_allow) classes_of(allow, "allow", a);
  if (has_deny) classes_of(deny, "deny", d);
  uint32_t m[3] = {1u, 0u, 0u};                  // EOS
  int n = 0;
  for (int i = 1; i < kClasses; ++i)
    if ((!has_allow || a[i]) && !(has_deny && d[i])) { m[i >> 5] |= 1u << (i & 31); ++n; }
  if (n == 0) throw std::runtime_error("charset: deny removes every character of allow: only the end of the text would be left");
  for (int i = 0; i < 3; ++i) mask[i] = m[i];
  return n;
}

std::vector<Reading> nbest_from_alts(const Tokenizer& tok, const int32_t* alt_ids, const float* alt_prob, int k, int m) {
  auto is_char = [](int id) { return id >= 1 && id < 95 && id != 88; };
  auto pr = [&](int p, int j) { const float v = alt_prob[(size_t)p * k + j]; return v == v ? v : 0.f; };   // (a NaN orders nothing: it counts as 0)
  int e = -1;
  for (int p = 0; p < 26 && e < 0; ++p) if (alt_ids[(size_t)p * k] == 0) e = p;
  std::vector<int> S;
  std::vector<std::vector<int>> opt;   // per position of S: its option slots in rank order
  for (int p = 0; p < (e < 0 ? 26 : e); ++p) {
    if (!is_char(alt_ids[(size_t)p * k])) continue;
    std::vector<int> o;
    for (int j = 0; j < k; ++j) if (is_char(alt_ids[(size_t)p * k + j])) o.push_back(j);
    std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return pr(p, a) > pr(p, b); });
    S.push_back(p);
    opt.push_back(std::move(o));
  }
  const size_t L = S.size();
  typedef std::vector<uint8_t> Tuple;
  auto score = [&](const Tuple& t) {
    float c = 1.f;
    for (size_t i = 0; i < L; ++i) c *= pr(S[i], opt[i][t[i]]);
    if (e >= 0) c *= pr(e, 0);
    return c;
  };
  typedef std::pair<float, Tuple> Node;
  auto before = [](const Node& a, const Node& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; };   // a is read before b
  std::set<Node, decltype(before)> open(before);   // the frontier, best first
  std::set<Tuple> seen;
  const Tuple zero(L, 0);
  open.insert(Node(score(zero), zero));
  seen.insert(zero);
  std::vector<Reading> out;
  while ((int)out.size() < m && !open.empty()) {
    const Node top = *open.begin();
    open.erase(open.begin());
    Reading r;
    r.score = top.first;
    for (size_t i = 0; i < L; ++i) r.text.push_back(tok.itos[(size_t)alt_ids[(size_t)S[i] * k + opt[i][top.second[i]]]]);
    out.push_back(std::move(r));
    for (size_t i = 0; i < L; ++i) {
      if ((size_t)top.second[i] + 1 >= opt[i].size()) continue;
      Tuple t = top.second;
      ++t[i];
      if (seen.insert(t).second) open.insert(Node(score(t), t));
    }
  }
  return out;
}

int confidence_from_probs(const int* ids, const float* probs, int n, float* char_conf, float* conf) {
  float c = 1.f;
  int k = 0;
  for (int p = 0; p < n; ++p) {
    if (ids[p] == 0) { c *= probs[p]; break; }                 // the EOS ends the text; its probability counts (upstream PARSeq's probs[:eos + 1])
    if (ids[p] == 88 || ids[p] < 0 || ids[p] >= 98) continue;   // dropped by Tokenizer::decode
    c *= probs[p];
    if (char_conf) char_conf[k] = probs[p];
    ++k;
  }
  if (conf) *conf = c;
  return k;
}

void lexicon_encode(const Tokenizer& tok, const char* const* words, int n, uint8_t* records) {
  if (!words || !records) throw std::runtime_error("lexicon: null argument");
  if (n < 1 || n > kLexMaxWords) throw std::runtime_error("lexicon: the number of words must lie in 1..1048576, got " + std::to_string(n));
  int cls[256];                                 // byte -> its one class, -1 = none, -2 = more than one
  for (int b = 0; b < 256; ++b) cls[b] = -1;
  for (int i = 1; i < 95; ++i) {
    if (i == 88) continue;                      // ']' : the id that decodes to nothing
    int& c = cls[(unsigned char)tok.itos[(size_t)i]];
    c = c == -1 ? i : -2;
  }
  cls[(unsigned char)']'] = -1;
  for (int w = 0; w < n; ++w) {
    const char* s = words[w];
    const std::string at = "lexicon: word " + std::to_string(w);
    if (!s) throw std::runtime_error(at + " is null");
    const size_t L = strnlen(s, (size_t)kLexMaxLen + 1);
    if (L == 0) throw std::runtime_error(at + " is empty");
    if (L > (size_t)kLexMaxLen) throw std::runtime_error(at + " is longer than 25 bytes");
    uint8_t* r = records + (size_t)w * kLexRecord;
    memset(r, 0, kLexRecord);
    r[0] = (uint8_t)L;
    for (size_t p = 0; p < L; ++p) {
      const unsigned char ch = (unsigned char)s[p];
      if (cls[ch] < 0) {
        char b[16];
        if (ch >= 0x20 && ch < 0x7f) snprintf(b, sizeof b, "'%c'", ch); else snprintf(b, sizeof b, "'\\x%02x'", ch);
        throw std::runtime_error(at + " holds " + b + (cls[ch] == -2 ? ", which names two recogniser classes (ids 69 and 87)" : ", which names no recogniser class"));
      }
      r[1 + p] = (uint8_t)cls[ch];
    }
  }
}

int lexicon_fuzzy_from_lp(const float* lp, const uint8_t* records, int n, int band, float gap, float* logp, int32_t* edits) {
  constexpr int kP = 26, kStride = 96;          // positions and floats per row of the table
  if (!lp || !records || !logp || !edits || n < 0) return -1;
  if (band < 0 || band > kLexMaxBand) return -1;
  if (!std::isfinite(gap) || gap > 0.f) return -1;
  for (int i = 0; i < n; ++i) {                 // everything is checked before anything is written
    const uint8_t* r = records + (size_t)i * kLexRecord;
    if (r[0] < 1 || r[0] > kLexMaxLen) return -1;
    for (int k = 1; k <= kLexMaxLen; ++k) if (r[k] >= kStride) return -1;
  }
  struct Cell { float s; int e; };
  const float ninf = -std::numeric_limits<float>::infinity();
  auto take = [](Cell& cur, float s, int e) { if (s > cur.s || (s == cur.s && e < cur.e)) cur = Cell{s, e}; };
  for (int i = 0; i < n; ++i) {
    const uint8_t* r = records + (size_t)i * kLexRecord;
    const int L = r[0];
    Cell D[kLexMaxLen + 1][kP];
    auto exists = [&](int j, int p) { return j >= 0 && j <= L && p >= 0 && p < kP && std::abs(j - p) <= band; };
    for (int j = 0; j <= L; ++j) {
      for (int p = 0; p < kP; ++p) {
        Cell& c = D[j][p];
        c = Cell{ninf, 0};
        if (!exists(j, p)) continue;
        if (j == 0 && p == 0) { c = Cell{0.0f, 0}; continue; }
        if (exists(j - 1, p - 1)) take(c, D[j - 1][p - 1].s + lp[(p - 1) * kStride + r[j]], D[j - 1][p - 1].e);   // match: r[j] is entry character j-1
        if (exists(j, p - 1)) take(c, D[j][p - 1].s + gap, D[j][p - 1].e + 1);                                     // extra character in the reading
        if (exists(j - 1, p)) take(c, D[j - 1][p].s + gap, D[j - 1][p].e + 1);                                     // dropped character
      }
    }
    Cell best{ninf, 0};
    for (int p = 0; p < kP; ++p) if (exists(L, p)) take(best, D[L][p].s + lp[p * kStride], D[L][p].e);
    logp[i] = best.s; edits[i] = best.e;
  }
  return 0;
}

// ---- tiled pages (geometry.h; DESIGN.md "Tiled pages")
static inline int c32(int x) { return (x + 31) / 32 * 32; }

static int tile_axis(const char* side, int L, int S, int O, int* o, int* e, int* canvas) {
  if (L <= S) { o[0] = 0; e[0] = L; *canvas = c32(L); return 1; }
  const int D = S - O, n = (L - S + D - 1) / D + 1;
  if (n > kTileMaxAxis)
    throw std::runtime_error(std::string("tiled pages: at most 16 tiles per axis, the ") + side + " " + std::to_string(L) + " needs " + std::to_string(n));
  for (int k = 0; k < n - 1; ++k) o[k] = k * D;
  o[n - 1] = c32(L - S);
  for (int k = 0; k < n; ++k) e[k] = std::min(S, L - o[k]);
  *canvas = S;
  return n;
}

TilePlan tile_plan(int h, int w, int S, int O, float mag_ratio) {
  if (S <= 0 || S % 32) throw std::runtime_error("tiled pages: canvas_size must be a positive multiple of 32, got " + std::to_string(S));
  if (O % 32 || O < 64 || O > S / 4)
    throw std::runtime_error("tiled pages: the overlap must be a multiple of 32 in [64, canvas_size / 4 = " + std::to_string(S / 4) + "], got " + std::to_string(O));
  if (!(mag_ratio == 1.0f)) throw std::runtime_error("tiled pages: mag_ratio must be 1.0 (tiles are cut at the page's own scale), got " + std::to_string(mag_ratio));
  if (h <= 0 || w <= 0) throw std::runtime_error("Error reading image from file");
  if (h > kTileMaxSide || w > kTileMaxSide)
    throw std::runtime_error("tiled pages: a page side may be at most 8192 pixels, got " + std::to_string(std::max(h, w)));
  TilePlan p{};
  p.ny = tile_axis("height", h, S, O, p.oy, p.ey, &p.Hc);
  p.nx = tile_axis("width", w, S, O, p.ox, p.ex, &p.Wc);
  if (p.ny * p.nx > kTileMaxPage)
    throw std::runtime_error("tiled pages: at most 64 tiles per page, " + std::to_string(h) + " x " + std::to_string(w) + " needs " + std::to_string(p.ny) + " x " +
                             std::to_string(p.nx) + " = " + std::to_string(p.ny * p.nx));
  p.hp = c32(h); p.wp = c32(w); p.H2 = p.hp / 2; p.W2 = p.wp / 2;
  return p;
}

static void tile_axis_check(const char* axis, const int* o, int n, int canvas, int map_len) {
  const std::string at = std::string("tile plan, ") + axis + ": ";
  if (n < 1 || n > kTileMaxAxis) throw std::runtime_error(at + "the number of tiles must lie in 1..16, got " + std::to_string(n));
  if (canvas <= 0 || canvas % 32 || canvas > kTileMaxSide) throw std::runtime_error(at + "the tile canvas must be a multiple of 32 in 32..8192, got " + std::to_string(canvas));
  if (map_len <= 0 || map_len > kTileMaxSide / 2) throw std::runtime_error(at + "the page map must have 1..4096 pixels, got " + std::to_string(map_len));
  if (!o) throw std::runtime_error(at + "null origins");
  if (o[0] != 0) throw std::runtime_error(at + "the first origin must be 0, got " + std::to_string(o[0]));
  const int s = canvas / 2;
  int prev_c = 0;
  for (int k = 0; k < n; ++k) {
    if (o[k] < 0 || o[k] % 32 || o[k] > kTileMaxSide) throw std::runtime_error(at + "origin " + std::to_string(k) + " must be a multiple of 32 in 0..8192, got " + std::to_string(o[k]));
    if (k + 1 == n) break;
    if (o[k + 1] <= o[k]) throw std::runtime_error(at + "origins must ascend, origin " + std::to_string(k + 1) + " is " + std::to_string(o[k + 1]) + " after " + std::to_string(o[k]));
    const int lap = o[k] + canvas - o[k + 1];
    if (lap < 2 * kTileBand) throw std::runtime_error(at + "tiles " + std::to_string(k) + " and " + std::to_string(k + 1) + " overlap by " + std::to_string(lap) + " pixels, a feather band needs 32");
    const int c = (o[k + 1] / 2 + o[k] / 2 + s) / 2;
    if (k > 0 && c - kTileBand / 2 < prev_c + kTileBand / 2)
      throw std::runtime_error(at + "the feather bands of seams " + std::to_string(k - 1) + " and " + std::to_string(k) + " touch (centres " + std::to_string(prev_c) + " and " + std::to_string(c) + ")");
    prev_c = c;
  }
  if (o[n - 1] / 2 + s != map_len)
    throw std::runtime_error(at + "the last tile must end at the map's end " + std::to_string(map_len) + ", it ends at " + std::to_string(o[n - 1] / 2 + s));
}

TilePlan tile_plan_from_origins(int ny, int nx, const int* oy, const int* ox, int Hc, int Wc, int H2, int W2) {
  tile_axis_check("y", oy, ny, Hc, H2);
  tile_axis_check("x", ox, nx, Wc, W2);
  if (ny * nx > kTileMaxPage) throw std::runtime_error("tile plan: at most 64 tiles per page, got " + std::to_string(ny * nx));
  TilePlan p{};
  p.ny = ny; p.nx = nx; p.Hc = Hc; p.Wc = Wc; p.H2 = H2; p.W2 = W2; p.hp = 2 * H2; p.wp = 2 * W2;
  for (int k = 0; k < ny; ++k) { p.oy[k] = oy[k]; p.ey[k] = std::min(Hc, p.hp - oy[k]); }
  for (int k = 0; k < nx; ++k) { p.ox[k] = ox[k]; p.ex[k] = std::min(Wc, p.wp - ox[k]); }
  return p;
}

// a + t (b - a) in three roundings: no step may be contracted into an FMA (tile_stitch_kernel uses __fsub_rn / __fmul_rn / __fadd_rn)
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
static inline float tile_lerp(float a, float b, float t) {
  const float d = b - a;
  const float m = t * d;
  return a + m;
}

void stitch_tiles(const float* tiles, int pages, const TilePlan& P, float* out) {
  if (!tiles || !out || pages < 0) throw std::runtime_error("stitch_tiles: null argument");
  const int sy = P.Hc / 2, sx = P.Wc / 2, T = P.ny * P.nx;
  const size_t tile_floats = (size_t)sy * sx * 2;
  for (int pg = 0; pg < pages; ++pg) {
    const float* tp = tiles + (size_t)pg * T * tile_floats;
    float* op = out + (size_t)pg * P.H2 * P.W2 * 2;
    for (int y = 0; y < P.H2; ++y) {
      const TileSeg gy = tile_seg(P.oy, P.ny, sy, y);
      for (int x = 0; x < P.W2; ++x) {
        const TileSeg gx = tile_seg(P.ox, P.nx, sx, x);
        for (int ch = 0; ch < 2; ++ch) {
          auto at = [&](int ty, int tx) { return tp[(size_t)(ty * P.nx + tx) * tile_floats + ((size_t)(y - P.oy[ty] / 2) * sx + (x - P.ox[tx] / 2)) * 2 + ch]; };
          auto row = [&](int ty) { return gx.blend ? tile_lerp(at(ty, gx.k), at(ty, gx.k + 1), gx.t) : at(ty, gx.k); };
          op[((size_t)y * P.W2 + x) * 2 + ch] = gy.blend ? tile_lerp(row(gy.k), row(gy.k + 1), gy.t) : row(gy.k);
        }
      }
    }
  }
}

// ---- tables (DESIGN.md "Tables"): the host rule; integers only.  The predicates and steps 6 - 7 are tables_rule.h's.
bool tables_args_ok(int min_len, int ink) { return min_len >= kTabMinLenLo && min_len <= kTabMinLenHi && ink >= 1 && ink <= 255; }

void tables_ink(const uint8_t* image, int h, int w, int stride, int ink, uint64_t* bits) {
  const int nw = (w + 63) / 64;
  for (int y = 0; y < h; ++y) {
    const uint8_t* row = image + (size_t)y * stride;
    uint64_t* out = bits + (size_t)y * nw;
    for (int k = 0; k < nw; ++k) out[k] = 0;
    for (int x = 0; x < w; ++x)
      if (tab_ink((int)row[3 * x] + (int)row[3 * x + 1] + (int)row[3 * x + 2], ink)) out[x >> 6] |= (uint64_t)1 << (x & 63);
  }
}

int tables_runs(const uint64_t* bits, int h, int w, int dir, int32_t* runs) {
  const int nw = (w + 63) / 64, lines = dir ? w : h, len = dir ? h : w;
  int n = 0;
  for (int l = 0; l < lines; ++l) {
    int start = -1;
    for (int p = 0; p <= len; ++p) {
      const bool on = p < len && (dir ? (bits[(size_t)p * nw + (l >> 6)] >> (l & 63)) & 1 : (bits[(size_t)l * nw + (p >> 6)] >> (p & 63)) & 1);
      if (on) { if (start < 0) start = p; continue; }
      if (start >= 0 && p - start >= kTabR) {
        if (n == kTabRunCap) return kTabRunCap + 1;
        runs[3 * n] = l; runs[3 * n + 1] = start; runs[3 * n + 2] = p - 1;
        ++n;
      }
      start = -1;
    }
  }
  return n;
}

static bool page_args_ok(const uint8_t* image, int h, int w, int stride, const int32_t* side, const InkRule& rule) {
  return image && side && h > 0 && w > 0 && h < 32768 && w < 32768 && stride >= 3 * w && (!rule.radius || ink_args_ok(rule.radius, rule.drop, rule.polarity));
}

void ink_bits(const uint8_t* image, int h, int w, int stride, const InkRule& rule, uint64_t* bits, uint64_t* bitsT) {
  if (rule.radius) return ink_from_page(image, h, w, stride, rule.radius, rule.drop, rule.polarity, bits, bitsT, nullptr);
  tables_ink(image, h, w, stride, rule.ink, bits);
  if (bitsT) marks_transpose(bits, h, w, bitsT);
}

int tables_from_page(const uint8_t* image, int h, int w, int stride, int min_len, const InkRule& rule, int32_t* side, int32_t* runs_out, uint64_t* bits_out) {
  if (!page_args_ok(image, h, w, stride, side, rule) || !tables_args_ok(min_len, rule.layer_ink())) throw std::runtime_error("tables_from_page: bad argument");
  std::vector<uint64_t> own_bits;
  uint64_t* bits = bits_out;
  if (!bits) { own_bits.resize(tables_bitmap_words(h, w)); bits = own_bits.data(); }
  ink_bits(image, h, w, stride, rule, bits, nullptr);
  return tables_from_bits(bits, h, w, min_len, side, runs_out);
}

// steps 2 - 7 behind a ready bitmap: the one body of the rule, whichever ink rule made the bits
int tables_from_bits(const uint64_t* bits, int h, int w, int min_len, int32_t* side, int32_t* runs_out) {
  std::fill(side, side + kTabSideInts, 0);
  std::vector<int32_t> own_runs;
  int32_t* runs = runs_out;
  if (!runs) { own_runs.resize((size_t)2 * kTabRunCap * 3); runs = own_runs.data(); }
  else std::fill(runs, runs + (size_t)2 * kTabRunCap * 3, 0);
  int nr[2];
  for (int dir = 0; dir < 2; ++dir) {   // 2
    nr[dir] = tables_runs(bits, h, w, dir, runs + (size_t)dir * kTabRunCap * 3);
    if (nr[dir] > kTabRunCap) { tables_clear(side, -2); return -2; }
  }
  std::vector<int32_t> parent(kTabRunCap), stat((size_t)kTabRunCap * 4);
  int count[2] = {0, 0};
  for (int dir = 0; dir < 2; ++dir) {   // 3, 4
    const int32_t* rn = runs + (size_t)dir * kTabRunCap * 3;
    const int n = nr[dir];
    for (int i = 0; i < n; ++i) parent[i] = i;
    for (int i = 0, j = 0; i < n; ++i) {   // j: the first run of the next line that may still link
      while (j < n && (rn[3 * j] < rn[3 * i] + 1)) ++j;
      for (int k = j; k < n && rn[3 * k] == rn[3 * i] + 1 && rn[3 * k + 1] <= rn[3 * i + 2] + 1; ++k)
        if (tab_link(rn[3 * i + 1], rn[3 * i + 2], rn[3 * k + 1], rn[3 * k + 2])) tab_union(parent.data(), i, k);
    }
    for (int i = 0; i < n; ++i) { stat[4 * i] = 32768; stat[4 * i + 1] = -1; stat[4 * i + 2] = -1; stat[4 * i + 3] = 0; }
    for (int i = 0; i < n; ++i) {   // per root: smallest a0, largest a1, last line, area
      const int r = tab_find(parent.data(), i);
      stat[4 * r] = std::min(stat[4 * r], rn[3 * i + 1]); stat[4 * r + 1] = std::max(stat[4 * r + 1], rn[3 * i + 2]);
      stat[4 * r + 2] = std::max(stat[4 * r + 2], rn[3 * i]); stat[4 * r + 3] += rn[3 * i + 2] - rn[3 * i + 1] + 1;
    }
    for (int i = 0; i < n; ++i) {
      if (parent[i] != i) continue;
      const int L = stat[4 * i + 1] - stat[4 * i] + 1, T = stat[4 * i + 2] - rn[3 * i] + 1;   // (the root is the component's first run: its line is the first)
      if (!tab_is_ruling(L, T, stat[4 * i + 3], min_len)) continue;
      if (count[dir] == kTabRulingCap) { tables_clear(side, -4); return -4; }
      int32_t* q = side + kTabRulings + 6 * (count[0] + count[1]);
      q[0] = dir;
      if (dir == 0) { q[1] = stat[4 * i]; q[2] = rn[3 * i]; q[3] = stat[4 * i + 1]; q[4] = stat[4 * i + 2]; }
      else { q[1] = rn[3 * i]; q[2] = stat[4 * i]; q[3] = stat[4 * i + 2]; q[4] = stat[4 * i + 1]; }
      q[5] = -1;
      ++count[dir];
    }
  }
  const int nh = count[0], nv = count[1];
  side[1] = nh; side[2] = nv; side[5] = nr[0]; side[6] = nr[1];
  int32_t* rul = side + kTabRulings;
  for (int r = 0; r < nh + nv; ++r) parent[r] = r;   // 5
  for (int a = 0; a < nh; ++a)
    for (int b = nh; b < nh + nv; ++b)
      if (tab_meet(rul + 6 * a, rul + 6 * b)) tab_union(parent.data(), a, b);
  for (int r = 0; r < nh + nv; ++r) rul[6 * r + 5] = tab_find(parent.data(), r);
  std::vector<int32_t> scratch(kTabScratchInts);
  const int mode = tables_grid(side, scratch.data());   // 6, 7
  if (mode != 1) { tables_clear(side, mode); return mode; }
  side[0] = 1;
  return 1;
}

void tables_word_centre(const float* q, int32_t c[2]) {
  long long cx = 0, cy = 0;
  for (int k = 0; k < 4; ++k) { cx += std::llrint(16.0 * (double)q[2 * k]); cy += std::llrint(16.0 * (double)q[2 * k + 1]); }
  c[0] = (int32_t)cx; c[1] = (int32_t)cy;
}

void tables_words(const int32_t* side, const int32_t* centres, int n, int32_t* out) {
  for (int i = 0; i < n; ++i) tab_word_cell(side, centres[2 * i], centres[2 * i + 1], out + 2 * (size_t)i);
}

void tables_export(const int32_t* s, int32_t counts[4], int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells) {
  const bool ok = s[0] == 1;
  const int nr = ok ? s[1] + s[2] : 0, nt = ok ? s[3] : 0, nc = ok ? s[4] : 0;
  int nl = 0;
  for (int t = 0; t < nt; ++t) {
    const int32_t* T = s + kTabTables + 8 * t;
    const int32_t* Y = s + kTabLines + 2 * kTabLineCap * t;
    if (lines) {
      std::copy(Y, Y + T[4] + 1, lines + nl);
      std::copy(Y + kTabLineCap, Y + kTabLineCap + T[5] + 1, lines + nl + T[4] + 1);
    }
    nl += T[4] + T[5] + 2;
  }
  if (counts) { counts[0] = nr; counts[1] = nt; counts[2] = nc; counts[3] = nl; }
  if (rulings) std::copy(s + kTabRulings, s + kTabRulings + 6 * nr, rulings);
  if (tables) std::copy(s + kTabTables, s + kTabTables + 8 * nt, tables);
  if (cells) std::copy(s + kTabCells, s + kTabCells + 9 * nc, cells);
}

bool tables_side_valid(const int32_t* s, std::string* why) {
  auto bad = [&](const char* m) { if (why) *why = m; return false; };
  const int mode = s[0];
  if (mode != 1 && mode != -2 && mode != -4 && mode != -6 && mode != -7) return bad("a mode that is none of 1, -2, -4, -6, -7");
  if (mode != 1) { for (int k = 1; k < 5; ++k) if (s[k] != 0) return bad("counts beside an overflow mode"); return true; }
  const int nh = s[1], nv = s[2], nt = s[3], nc = s[4];
  if (nh < 0 || nh > kTabRulingCap || nv < 0 || nv > kTabRulingCap || nt < 0 || nt > kTabTableCap || nc < 0 || nc > kTabCellCap) return bad("a count beyond its cap");
  for (int r = 0; r < nh + nv; ++r) {
    const int32_t* q = s + kTabRulings + 6 * r;
    if (q[0] != (r < nh ? 0 : 1) || q[1] < 0 || q[2] < 0 || q[3] < q[1] || q[4] < q[2] || q[3] >= 32768 || q[4] >= 32768 || q[5] < -1 || q[5] >= nt) return bad("a ruling out of range");
  }
  int next = 0;
  std::vector<uint8_t> seen;
  for (int t = 0; t < nt; ++t) {
    const int32_t* T = s + kTabTables + 8 * t;
    const int rows = T[4], cols = T[5];
    if (rows < 1 || rows >= kTabLineCap || cols < 1 || cols >= kTabLineCap || T[6] != next || T[7] < 1 || T[7] > rows * cols || T[6] + T[7] > nc) return bad("a table out of range");
    const int32_t* Y = s + kTabLines + 2 * kTabLineCap * t;
    const int32_t* X = Y + kTabLineCap;
    for (int i = 0; i <= rows; ++i) if (Y[i] < 0 || Y[i] >= 65536 || (i && Y[i] <= Y[i - 1])) return bad("row lines that do not ascend");
    for (int j = 0; j <= cols; ++j) if (X[j] < 0 || X[j] >= 65536 || (j && X[j] <= X[j - 1])) return bad("column lines that do not ascend");
    seen.assign((size_t)rows * cols, 0);
    for (int c = T[6]; c < T[6] + T[7]; ++c) {
      const int32_t* C = s + kTabCells + 9 * c;
      if (C[0] != t || C[1] < 0 || C[2] < 0 || C[3] < 1 || C[4] < 1 || C[1] + C[3] > rows || C[2] + C[4] > cols) return bad("a cell out of range");
      for (int i = C[1]; i < C[1] + C[3]; ++i)
        for (int j = C[2]; j < C[2] + C[4]; ++j) {
          if (seen[(size_t)i * cols + j]) return bad("two cells over one base cell");
          seen[(size_t)i * cols + j] = 1;
        }
    }
    for (uint8_t v : seen) if (!v) return bad("a base cell in no cell");
    next += T[7];
  }
  if (next != nc) return bad("cells that belong to no table");
  return true;
}

// ---- deskew (DESIGN.md "Deskew"): the host rule; the steps themselves are deskew_rule.h's
void deskew_consts(int32_t* cs) {
  for (int k = -kDskMaxSlope; k <= kDskMaxSlope; ++k) {
    const double d = std::sqrt(262144.0 + (double)(k * k));
    cs[2 * (k + kDskMaxSlope)] = (int32_t)std::llrint(33554432.0 / d);
    cs[2 * (k + kDskMaxSlope) + 1] = (int32_t)std::llrint(65536.0 * (double)k / d);
  }
}

void deskew_scores(const uint64_t* bits, int h, int w, int max_slope, uint64_t* scores) {
  const int nw = (w + 63) / 64, bias = dsk_bias(w, max_slope);
  std::vector<uint32_t> bins((size_t)dsk_bins(h, w, max_slope));
  for (int k = -max_slope; k <= max_slope; ++k) {
    std::fill(bins.begin(), bins.end(), 0u);
    for (int y = 0; y < h; ++y)
      for (int j = 0; j < nw; ++j) {
        uint64_t v = bits[(size_t)y * nw + j];
        while (v) {
          const int x = 64 * j + __builtin_ctzll(v);
          v &= v - 1;
          ++bins[(size_t)(y - dsk_off(x, k) + bias)];
        }
      }
    uint64_t s = 0;
    for (uint32_t c : bins) s += (uint64_t)c * c;
    scores[k + max_slope] = s;
  }
}

void deskew_choose(const uint64_t* scores, int max_slope, int gain, int h, int w, const int32_t* cs, DeskewRec* rec) {
  int found = 0;
  for (int k = -max_slope; k <= max_slope; ++k)
    if (dsk_better(scores[k + max_slope], k, scores[found + max_slope], found)) found = k;
  const int slope = dsk_slope(found, scores[found + max_slope], scores[max_slope], gain);
  *rec = DeskewRec{slope, found, cs[2 * (slope + kDskMaxSlope)], cs[2 * (slope + kDskMaxSlope) + 1], w, h, slope != 0 ? 1 : 0, 0, scores[max_slope], scores[found + max_slope]};
}

void deskew_resample(const uint8_t* image, int h, int w, int stride, int C, int S, uint8_t* out, int out_stride) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) dsk_pixel(image, h, w, stride, C, S, x, y, out + (size_t)y * out_stride + 3 * (size_t)x);
}

void deskew_from_page(const uint8_t* image, int h, int w, int stride, int max_slope, int gain, const InkRule& rule, uint8_t* out, int out_stride, DeskewRec* rec,
                      uint64_t* scores) {
  std::vector<uint64_t> bits(tables_bitmap_words(h, w));
  ink_bits(image, h, w, stride, rule, bits.data(), nullptr);
  deskew_from_bits(bits.data(), image, h, w, stride, max_slope, gain, out, out_stride, rec, scores);
}

// steps 2 - 5 behind a ready bitmap: the one body of the rule, whichever ink rule made the bits
void deskew_from_bits(const uint64_t* bits, const uint8_t* image, int h, int w, int stride, int max_slope, int gain, uint8_t* out, int out_stride, DeskewRec* rec, uint64_t* scores) {
  std::vector<uint64_t> sc((size_t)2 * max_slope + 1);
  std::vector<int32_t> cs(2 * kDskSlopes);
  deskew_scores(bits, h, w, max_slope, sc.data());
  deskew_consts(cs.data());
  DeskewRec r;
  deskew_choose(sc.data(), max_slope, gain, h, w, cs.data(), &r);
  if (out) deskew_resample(image, h, w, stride, r.C, r.S, out, out_stride);
  if (rec) *rec = r;
  if (scores) std::copy(sc.begin(), sc.end(), scores);
}

bool deskew_rec_valid(const DeskewRec& r, int max_slope, int h, int w, const int32_t* cs, std::string* why) {
  auto bad = [&](const char* m) { if (why) *why = m; return false; };
  if (r.found < -max_slope || r.found > max_slope) return bad("a found slope outside -max_slope..max_slope");
  if (r.slope != 0 && r.slope != r.found) return bad("a slope that is neither 0 nor the found one");
  if (r.C != cs[2 * (r.slope + kDskMaxSlope)] || r.S != cs[2 * (r.slope + kDskMaxSlope) + 1]) return bad("constants that are not the table's for its slope");
  if (r.w != w || r.h != h) return bad("another page's size");
  if (r.mode != (r.slope != 0 ? 1 : 0)) return bad("a mode that does not match its slope");
  if (r.score_found < r.score0) return bad("a found score below the score of slope 0");
  return true;
}

void deskew_to_page(const DeskewRec& r, const float* xy_in, int n, float* xy_out) {
  const double cx = (r.w - 1) / 2.0, cy = (r.h - 1) / 2.0;
  for (int i = 0; i < n; ++i) {
    const double x = (double)xy_in[2 * (size_t)i] - cx, y = (double)xy_in[2 * (size_t)i + 1] - cy;
    xy_out[2 * (size_t)i] = (float)(cx + ((double)r.C * x - (double)r.S * y) / 65536.0);
    xy_out[2 * (size_t)i + 1] = (float)(cy + ((double)r.S * x + (double)r.C * y) / 65536.0);
  }
}

// ---- local ink (DESIGN.md "Local ink"): the host rule; the steps themselves are ink_rule.h's
void ink_from_page(const uint8_t* image, int h, int w, int stride, int radius, int drop, int polarity, uint64_t* bits, uint64_t* bitsT, InkRec* rec) {
  if (!image || h <= 0 || w <= 0 || h >= 32768 || w >= 32768 || stride < 3 * w || !ink_args_ok(radius, drop, polarity)) throw std::runtime_error("ink_from_page: bad argument");
  const int R = radius, nwx = (w + 63) / 64, nwy = (h + 63) / 64;
  // 1, 3: s and its horizontal window sums, by a prefix sum along each row; the page's sum
  std::vector<uint16_t> s((size_t)h * w);
  std::vector<uint32_t> H((size_t)h * w), pre((size_t)w + 1);
  uint64_t sum = 0;
  for (int y = 0; y < h; ++y) {
    const uint8_t* row = image + (size_t)y * stride;
    uint16_t* sr = &s[(size_t)y * w];
    pre[0] = 0;
    for (int x = 0; x < w; ++x) { sr[x] = (uint16_t)((int)row[3 * x] + (int)row[3 * x + 1] + (int)row[3 * x + 2]); pre[(size_t)x + 1] = pre[x] + sr[x]; }
    sum += pre[(size_t)w];
    for (int x = 0; x < w; ++x) H[(size_t)y * w + x] = pre[(size_t)std::min(x + R, w - 1) + 1] - pre[(size_t)std::max(x - R, 0)];
  }
  const int inverted = ink_inverted(polarity, sum, h, w);   // 2
  if (rec) *rec = InkRec{radius, drop, polarity, inverted, sum, w, h};
  if (bits) std::fill(bits, bits + (size_t)h * nwx, (uint64_t)0);
  if (bitsT) std::fill(bitsT, bitsT + (size_t)w * nwy, (uint64_t)0);
  // 3, 4: the vertical sums by a running add and subtract down the columns, then the rule
  std::vector<uint32_t> S((size_t)w, 0u);
  for (int yy = 0; yy <= std::min(R, h - 1); ++yy)
    for (int x = 0; x < w; ++x) S[x] += H[(size_t)yy * w + x];
  for (int y = 0; y < h; ++y) {
    const int ny = ink_span(y, R, h);
    for (int x = 0; x < w; ++x) {
      if (!ink_local(s[(size_t)y * w + x], ink_span(x, R, w) * ny, S[x], drop, inverted)) continue;
      if (bits) bits[(size_t)y * nwx + (x >> 6)] |= (uint64_t)1 << (x & 63);
      if (bitsT) bitsT[(size_t)x * nwy + (y >> 6)] |= (uint64_t)1 << (y & 63);
    }
    if (y + 1 + R <= h - 1) for (int x = 0; x < w; ++x) S[x] += H[(size_t)(y + 1 + R) * w + x];
    if (y - R >= 0) for (int x = 0; x < w; ++x) S[x] -= H[(size_t)(y - R) * w + x];
  }
}

bool ink_rec_valid(const InkRec& r, int radius, int drop, int polarity, int h, int w, std::string* why) {
  auto bad = [&](const char* m) { if (why) *why = m; return false; };
  if (r.radius != radius || r.drop != drop || r.polarity != polarity) return bad("parameters that are not the engine's");
  if (r.w != w || r.h != h) return bad("another page's size");
  if (r.sum > (uint64_t)kInkSMax * (uint64_t)h * (uint64_t)w) return bad("a sum beyond 765 h w");
  if (r.inverted != 0 && r.inverted != 1) return bad("an inverted flag that is neither 0 nor 1");
  if (r.inverted != ink_inverted(polarity, r.sum, h, w)) return bad("an inverted flag that does not follow from polarity and sum");
  return true;
}

// ---- selection marks (DESIGN.md "Selection marks"): the host rule; integers only.  Every step is marks_rule.h's.
void marks_transpose(const uint64_t* bits, int h, int w, uint64_t* bitsT) {
  const int nwx = (w + 63) / 64, nwy = (h + 63) / 64;
  std::fill(bitsT, bitsT + (size_t)w * nwy, (uint64_t)0);
  for (int y = 0; y < h; ++y)
    for (int k = 0; k < nwx; ++k)
      for (uint64_t v = bits[(size_t)y * nwx + k]; v; v &= v - 1) {
        const int x = 64 * k + mark_ctz(v);
        if (x < w) bitsT[(size_t)x * nwy + (y >> 6)] |= (uint64_t)1 << (y & 63);
      }
}

int marks_from_bits(const uint64_t* bits, const uint64_t* bitsT, int h, int w, int min_side, int max_side, int fill, int32_t* side, int32_t* counts) {
  if (!bits || !bitsT || !side || h <= 0 || w <= 0 || h >= 32768 || w >= 32768 || !marks_args_ok(min_side, max_side, fill, 128)) throw std::runtime_error("marks_from_bits: bad argument");
  std::fill(side, side + kMarkSideInts, 0);
  const int nwx = (w + 63) / 64, nwy = (h + 63) / 64;
  if (counts) std::fill(counts, counts + 2 * (size_t)((h + 31) / 32), 0);
  int n = 0, corners = 0;
  int32_t rec[kMarkRec];
  for (int y = 0; y < h; ++y) {   // 2 - 5, in (y, x) order
    const uint64_t* row = bits + (size_t)y * nwx;
    for (int k = 0; k < nwx; ++k)
      for (uint64_t c = mark_corners(row, y ? row - nwx : nullptr, k); c; c &= c - 1) {
        ++corners;
        if (counts) counts[2 * (y / 32) + 1]++;
        if (!mark_test(bits, nwx, bitsT, nwy, 64 * k + mark_ctz(c), y, min_side, max_side, fill, rec)) continue;
        if (counts) counts[2 * (y / 32)]++;
        if (n < kMarkCap) std::copy(rec, rec + kMarkRec, side + kMarkHdr + kMarkRec * n);
        ++n;
      }
  }
  side[2] = corners; side[3] = n;
  if (n > kMarkCap) {   // 6: the cap
    std::fill(side + kMarkHdr, side + kMarkSideInts, 0);
    side[0] = -6;
    return -6;
  }
  side[0] = 1; side[1] = n;
  return 1;
}

void marks_items(int32_t* side, const int32_t* centres, int n, int32_t* item_mark) {
  std::vector<int32_t> own;
  if (!item_mark) { own.resize((size_t)n); item_mark = own.data(); }
  for (int i = 0; i < n; ++i) item_mark[i] = mark_item(side, centres[2 * (size_t)i], centres[2 * (size_t)i + 1]);
  if (side[0] != 1) return;
  for (int m = 0; m < side[1]; ++m) {
    int32_t* r = side + kMarkHdr + kMarkRec * m;
    r[11] = mark_label(r, centres, item_mark, n);
  }
}

int marks_from_page(const uint8_t* image, int h, int w, int stride, int min_side, int max_side, int fill, const InkRule& rule, int32_t* side, int32_t* counts) {
  if (!page_args_ok(image, h, w, stride, side, rule) || !marks_args_ok(min_side, max_side, fill, rule.layer_ink())) throw std::runtime_error("marks_from_page: bad argument");
  std::vector<uint64_t> bits(tables_bitmap_words(h, w)), bitsT(tables_bitmap_words(w, h));
  ink_bits(image, h, w, stride, rule, bits.data(), bitsT.data());
  return marks_from_bits(bits.data(), bitsT.data(), h, w, min_side, max_side, fill, side, counts);
}

bool marks_side_valid(const int32_t* s, int h, int w, int fill, int items, std::string* why) {
  auto bad = [&](const char* m) { if (why) *why = m; return false; };
  if (s[0] != 1 && s[0] != -6) return bad("a mode that is neither 1 nor -6");
  if (s[1] < 0 || s[1] > kMarkCap) return bad("a mark count beyond the cap");
  if (s[0] == -6 && s[1] != 0) return bad("marks on a page beyond the cap");
  if (s[2] < 0 || s[3] < s[1] || (s[0] == 1 && s[3] != s[1]) || (s[0] == -6 && s[3] <= kMarkCap)) return bad("counters that do not match its mode");
  for (int m = 0; m < s[1]; ++m) {
    const int32_t* r = s + kMarkHdr + kMarkRec * m;
    if (r[0] < 0 || r[1] < 0 || r[2] >= w || r[3] >= h || r[0] > r[2] || r[1] > r[3]) return bad("a box outside the page");
    if (r[4] <= r[0] || r[5] <= r[1] || r[6] >= r[2] || r[7] >= r[3] || r[4] > r[6] || r[5] > r[7]) return bad("an interior outside its box");
    if (r[9] != (r[6] - r[4] + 1) * (r[7] - r[5] + 1) || r[8] < 0 || r[8] > r[9]) return bad("an ink count beyond its interior");
    if (r[10] != (256 * r[8] >= fill * r[9] ? 1 : 0)) return bad("a state that is not the rule's");
    if (r[11] < -1 || r[11] >= items) return bad("a label that is no item");
    if (m && (r[1] < r[-kMarkRec + 1] || (r[1] == r[-kMarkRec + 1] && r[0] <= r[-kMarkRec]))) return bad("marks out of (y, x) order");
  }
  return true;
}

// ---- barcodes (DESIGN.md "Barcodes"): the host rule; integers only.  Every step is barcodes_rule.h's.
int barcodes_from_bits(const uint64_t* bits, const uint64_t* bitsT, int h, int w, int min_lines, int symbologies, int32_t* side, int32_t* hits_out, int32_t* cnt_out) {
  if (!bits || !bitsT || !side || h <= 0 || w <= 0 || h >= 32768 || w >= 32768 || !barcodes_args_ok(min_lines, 128, symbologies)) throw std::runtime_error("barcodes_from_bits: bad argument");
  static const std::vector<uint8_t> tab = [] { std::vector<uint8_t> t(kBcTableBytes); bc_tables_clear(t.data(), 0, 1); bc_tables_fill(t.data(), 0, 1); return t; }();
  std::fill(side, side + kBcSideInts, 0);
  const int nwx = (w + 63) / 64, nwy = (h + 63) / 64, lines = h + w;
  std::vector<int32_t> hits((size_t)lines * 2 * kBcLineHits * kBcHit, 0), cnt((size_t)lines * 2 * kBcCnt, 0);
  // 2 - 6: every line, both readings, the candidates in position order
  for (int L = 0; L < lines; ++L) {
    const uint64_t* line = L < h ? bits + (size_t)L * nwx : bitsT + (size_t)(L - h) * nwy;
    const int len = L < h ? w : h, nw = L < h ? nwx : nwy;
    for (int rev = 0; rev < 2; ++rev) {
      int32_t* c = cnt.data() + (size_t)kBcCnt * (2 * L + rev);
      int32_t* slots = hits.data() + (size_t)(2 * L + rev) * kBcLineHits * kBcHit;
      for (int k = 0; k < nw; ++k)
        for (uint64_t m = bc_candidates(line, nw, k, rev); m; m &= m - 1) {
          const int x = 64 * k + mark_ctz(m), u0 = rev ? len - 1 - x : x;
          int starts = 0;
          ++c[2];
          const bool hit = bc_decode(tab.data(), line, len, rev, u0, symbologies, c[0] < kBcLineHits ? slots + (size_t)c[0] * kBcHit : nullptr, &starts);
          c[3] += starts;
          if (hit) { if (c[0] < kBcLineHits) { slots[(size_t)c[0] * kBcHit + 6] = -1; slots[(size_t)c[0] * kBcHit + 7] = -1; ++c[0]; } else ++c[1]; }
          else if (c[0] < kBcLineHits) std::fill(slots + (size_t)c[0] * kBcHit, slots + (size_t)(c[0] + 1) * kBcHit, 0);   // (a text begun and given up)
        }
      side[2] += c[2]; side[3] += c[3]; side[4] += c[0]; side[5] += c[1];
    }
  }
  // 7: every hit's partner, then its chain's first hit
  auto kind = [&](int L, int& L0, int& L1) { L0 = L < h ? 0 : h; L1 = L < h ? h : lines; };
  for (int L = 0; L < lines; ++L)
    for (int rev = 0; rev < 2; ++rev)
      for (int s = 0; s < cnt[(size_t)kBcCnt * (2 * L + rev)]; ++s) {
        int L0, L1; kind(L, L0, L1);
        hits[(size_t)((2 * L + rev) * kBcLineHits + s) * kBcHit + 6] = bc_pred(hits.data(), cnt.data(), L0, L, rev, s);
      }
  for (int L = 0; L < lines; ++L)
    for (int rev = 0; rev < 2; ++rev)
      for (int s = 0; s < cnt[(size_t)kBcCnt * (2 * L + rev)]; ++s) {
        int id = (2 * L + rev) * kBcLineHits + s, root = id;
        while (hits[(size_t)root * kBcHit + 6] >= 0) root = hits[(size_t)root * kBcHit + 6];
        hits[(size_t)id * kBcHit + 7] = root;
      }
  // 7 - 8: the chains of min_lines hits or more, sorted
  std::vector<std::pair<int, std::vector<int32_t>>> found;
  for (int L = 0; L < lines; ++L)
    for (int rev = 0; rev < 2; ++rev)
      for (int s = 0; s < cnt[(size_t)kBcCnt * (2 * L + rev)]; ++s) {
        const int id = (2 * L + rev) * kBcLineHits + s;
        if (hits[(size_t)id * kBcHit + 6] >= 0) continue;
        int L0, L1; kind(L, L0, L1);
        std::vector<int32_t> rec(kBcRec, 0);
        if (bc_chain(hits.data(), cnt.data(), L0, L1, L, rev, s, L >= h, rec.data()) >= min_lines) found.emplace_back(id, std::move(rec)); else ++side[6];
      }
  if (hits_out) std::copy(hits.begin(), hits.end(), hits_out);
  if (cnt_out) std::copy(cnt.begin(), cnt.end(), cnt_out);
  if ((int)found.size() > kBcCap) { side[0] = -7; return -7; }
  std::sort(found.begin(), found.end(), [](const auto& a, const auto& b) { return bc_before(a.second.data(), a.first, b.second.data(), b.first); });
  for (size_t m = 0; m < found.size(); ++m) std::copy(found[m].second.begin(), found[m].second.end(), side + kBcHdr + kBcRec * m);
  side[0] = 1; side[1] = (int)found.size();
  return 1;
}

void barcodes_items(const int32_t* side, const int32_t* centres, int n, int32_t* item_barcode) {
  for (int i = 0; i < n; ++i) item_barcode[i] = bc_item(side, centres[2 * (size_t)i], centres[2 * (size_t)i + 1]);
}

int barcodes_from_page(const uint8_t* image, int h, int w, int stride, int min_lines, const InkRule& rule, int symbologies, int32_t* side, int32_t* hits, int32_t* cnt) {
  if (!page_args_ok(image, h, w, stride, side, rule) || !barcodes_args_ok(min_lines, rule.layer_ink(), symbologies)) throw std::runtime_error("barcodes_from_page: bad argument");
  std::vector<uint64_t> bits(tables_bitmap_words(h, w)), bitsT(tables_bitmap_words(w, h));
  ink_bits(image, h, w, stride, rule, bits.data(), bitsT.data());
  return barcodes_from_bits(bits.data(), bitsT.data(), h, w, min_lines, symbologies, side, hits, cnt);
}

bool barcodes_side_valid(const int32_t* s, int h, int w, int min_lines, int symbologies, std::string* why) {
  auto bad = [&](const char* m) { if (why) *why = m; return false; };
  if (s[0] != 1 && s[0] != -7) return bad("a mode that is neither 1 nor -7");
  if (s[1] < 0 || s[1] > kBcCap) return bad("a barcode count beyond the cap");
  if (s[0] == -7 && s[1] != 0) return bad("barcodes on a page beyond the cap");
  for (int i = 2; i < 7; ++i) if (s[i] < 0) return bad("a negative counter");
  if (s[7] != 0 || s[3] > 2 * s[2] || s[4] > s[2]) return bad("counters that do not match each other");
  for (int m = 0; m < s[1]; ++m) {
    const int32_t* r = s + kBcHdr + kBcRec * m;
    if (r[0] < 0 || r[1] < 0 || r[2] >= w || r[3] >= h || r[0] > r[2] || r[1] > r[3]) return bad("a box outside the page");
    if ((r[4] != 1 && r[4] != 2) || !(symbologies & r[4])) return bad("a symbology that was not asked for");
    if (r[5] < 0 || r[5] > 3) return bad("a direction outside 0..3");
    if (r[6] < min_lines || r[7] < 64) return bad("a line count below min_lines or a module below one pixel");
    if (r[8] & ~kBcFlagsMask || (r[4] == 2 && r[8])) return bad("flags beyond the mask");
    if (r[9] < 0 || r[9] > kBcText || r[10] != 0 || r[11] != 0) return bad("a text length beyond 48");
    const uint8_t* t = reinterpret_cast<const uint8_t*>(r + 12);
    for (int i = r[9]; i < kBcText; ++i) if (t[i]) return bad("text bytes beyond its length");
    if (m && bc_before(r, 1, r - kBcRec, 0)) return bad("barcodes out of (y0, x0, dir) order");
  }
  return true;
}

}  // namespace ttr
