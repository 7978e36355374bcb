// Selection marks (DESIGN.md "Selection marks"): the constants, the side block's layout and every step of the rule behind the ink bitmaps, one statement of
// each, shared by the host rule (geometry.cpp: marks_from_bits) and the two kernels (marks.hip).  The host loops over the page's corners and the candidate kernel
// spreads them over row bands, both through mark_corners and mark_test below; the items' marks and the marks' labels are mark_item and mark_label on either side,
// so the three agree bit for bit by construction.  Integer arithmetic only; every value is below 2^31 (cx - 64 (x1 + 1) and 64 * 8 * a stay below 2^23).
// tests/marks_ref.py restates all of it in numpy and Python integers.
//
// The bitmaps are tables.hip's (ink_tile.h): bits [h][ceil(w / 64)] uint64, bit x % 64 of word x / 64 of row y, and bitsT [w][ceil(h / 64)] the same bits along y;
// both are zero beyond the page inside their last word, and nothing here reads a word beyond a line's own ceil(len / 64).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TTR_MARK_HD __host__ __device__ inline
#else
#define TTR_MARK_HD inline
#endif

namespace ttr {

constexpr int kMarkMinLo = 8, kMarkMinHi = 64, kMarkMaxHi = 128;   // min_side in 8..64, max_side in min_side..128
constexpr int kMarkCap = 512;                                      // marks per page
constexpr int kMarkRec = 12;                                       // x0, y0, x1, y1, ix0, iy0, ix1, iy1, inked, area, state, label
constexpr int kMarkLabelSides = 8;                                 // a label starts within 8 sides of the frame's right edge

// The side block of one page, int32: a header, then the records.
//   header  [0] mode (1, or -6: more than kMarkCap marks)  [1] marks  [2] corners examined (step 2)  [3] candidates kept by steps 3 - 5 (= [1] unless the cap
//           was passed)  [4..7] 0
//   marks   [512][12]  in (y0, x0) order
constexpr int kMarkHdr = 8;
constexpr int kMarkSideInts = kMarkHdr + kMarkCap * kMarkRec;
// a batch's side blocks: [pages][kMarkSideInts] | [N] every item's mark
constexpr size_t marks_side_bytes(int pages, int N) { return ((size_t)pages * kMarkSideInts + (size_t)N) * 4; }

TTR_MARK_HD bool marks_args_ok(int min_side, int max_side, int fill, int ink) {
  return min_side >= kMarkMinLo && min_side <= kMarkMinHi && max_side >= min_side && max_side <= kMarkMaxHi && fill >= 1 && fill <= 255 && ink >= 1 && ink <= 255;
}

TTR_MARK_HD int mark_ctz(uint64_t v) { return __builtin_ctzll(v); }          // (v != 0)
TTR_MARK_HD int mark_popc(uint64_t v) { return __builtin_popcountll(v); }

// the number of consecutive set bits of a line of nw words from bit p on, counted up to limit (p >= 0; bits beyond the line's words are clear)
TTR_MARK_HD int mark_run(const uint64_t* line, int nw, int p, int limit) {
  int n = 0, k = p >> 6, o = p & 63;
  while (n < limit && k < nw) {
    const uint64_t v = ~(line[k] >> o);               // (the o bits shifted in are clear, so set here: the count ends at the word's end at the latest)
    const int c = v ? mark_ctz(v) : 64;
    n += c;
    if (c < 64 - o) break;
    ++k; o = 0;
  }
  return n < limit ? n : limit;
}
// bits p0..p1 of the line are all set (p0 <= p1)
TTR_MARK_HD bool mark_full(const uint64_t* line, int nw, int p0, int p1) { return mark_run(line, nw, p0, p1 - p0 + 1) == p1 - p0 + 1; }
// the number of set bits among bits p0..p1 of the line (p0 <= p1)
TTR_MARK_HD int mark_count(const uint64_t* line, int nw, int p0, int p1) {
  int n = 0;
  for (int k = p0 >> 6; k <= (p1 >> 6) && k < nw; ++k) {
    uint64_t v = line[k];
    if (k == (p0 >> 6)) v &= ~(uint64_t)0 << (p0 & 63);
    if (k == (p1 >> 6)) v &= ~(uint64_t)0 >> (63 - (p1 & 63));
    n += mark_popc(v);
  }
  return n;
}

// 2: the corners among the 64 pixels of word k of row y: ink, no ink to the left, no ink above.  row = the row's words, above = row y - 1's words or null (y = 0)
TTR_MARK_HD uint64_t mark_corners(const uint64_t* row, const uint64_t* above, int k) {
  const uint64_t w = row[k], carry = k ? row[k - 1] >> 63 : 0;
  return w & ~(w << 1 | carry) & ~(above ? above[k] : 0);
}

// 3 - 5 on the corner (x, y): true when it is a mark, and rec [12] then holds its record (label -1).  bits / bitsT are the page's own bitmaps (rows nwx = ceil(w /
// 64) and nwy = ceil(h / 64) words apart).
TTR_MARK_HD bool mark_test(const uint64_t* bits, int nwx, const uint64_t* bitsT, int nwy, int x, int y, int min_side, int max_side, int fill, int32_t* rec) {
  // 3: sides
  const int a = mark_run(bits + (size_t)y * nwx, nwx, x, max_side + 1);
  if (a < min_side || a > max_side) return false;
  const int b = mark_run(bitsT + (size_t)x * nwy, nwy, y, max_side + 1);
  if (b < min_side || b > max_side) return false;
  const int m = a < b ? a : b, d = a < b ? b - a : a - b;
  if (4 * d > m) return false;
  const int x1 = x + a - 1, y1 = y + b - 1;
  if (!mark_full(bits + (size_t)y1 * nwx, nwx, x, x1) || !mark_full(bitsT + (size_t)x1 * nwy, nwy, y, y1)) return false;
  // 4: frame (the outer line of every side is ink by now, so every t is at least 1)
  const int q = m / 4;
  int tt = 1, tb = 1, tl = 1, tr = 1;
  while (tt < q && mark_full(bits + (size_t)(y + tt) * nwx, nwx, x, x1)) ++tt;
  while (tb < q && mark_full(bits + (size_t)(y1 - tb) * nwx, nwx, x, x1)) ++tb;
  while (tl < q && mark_full(bitsT + (size_t)(x + tl) * nwy, nwy, y, y1)) ++tl;
  while (tr < q && mark_full(bitsT + (size_t)(x1 - tr) * nwy, nwy, y, y1)) ++tr;
  if (tt == q || tb == q || tl == q || tr == q) return false;
  const int ix0 = x + tl + 1, ix1 = x1 - tr - 1, iy0 = y + tt + 1, iy1 = y1 - tb - 1;
  if (ix0 > ix1 || iy0 > iy1) return false;
  // 5: state
  int inked = 0;
  for (int r = iy0; r <= iy1; ++r) inked += mark_count(bits + (size_t)r * nwx, nwx, ix0, ix1);
  const int area = (ix1 - ix0 + 1) * (iy1 - iy0 + 1);
  rec[0] = x; rec[1] = y; rec[2] = x1; rec[3] = y1; rec[4] = ix0; rec[5] = iy0; rec[6] = ix1; rec[7] = iy1;
  rec[8] = inked; rec[9] = area; rec[10] = 256 * inked >= fill * area ? 1 : 0; rec[11] = -1;
  return true;
}

// 7: the mark of an item at (cx, cy) = 64 x its centre: the first mark, in mark order, whose box holds the centre; -1 when there is none or the page is beyond the cap
TTR_MARK_HD int mark_item(const int32_t* side, int cx, int cy) {
  if (side[0] != 1) return -1;
  for (int m = 0; m < side[1]; ++m) {
    const int32_t* r = side + kMarkHdr + kMarkRec * m;
    if (cx >= 64 * r[0] && cx < 64 * (r[2] + 1) && cy >= 64 * r[1] && cy < 64 * (r[3] + 1)) return m;
  }
  return -1;
}
// 7: the label of mark r among n items (centres [n][2], item_mark [n]): the item in no mark, level with the box and within 8 sides of its right edge, with the
// smallest cx; ties go to the smaller index; -1 when there is none
TTR_MARK_HD int mark_label(const int32_t* r, const int32_t* centres, const int32_t* item_mark, int n) {
  const int a = r[2] - r[0] + 1, right = 64 * (r[2] + 1);
  int best = -1, best_cx = 0;
  for (int i = 0; i < n; ++i) {
    if (item_mark[i] != -1) continue;
    const int cx = centres[2 * i], cy = centres[2 * i + 1];
    if (cy < 64 * r[1] || cy >= 64 * (r[3] + 1) || cx - right < 0 || cx - right > 64 * kMarkLabelSides * a) continue;
    if (best < 0 || cx < best_cx) { best = i; best_cx = cx; }
  }
  return best;
}

}  // namespace ttr
