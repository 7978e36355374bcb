// Barcodes (DESIGN.md "Barcodes"): the constants, the tables, the side block's layout and every step of the rule behind the ink bitmaps, one statement of each,
// shared by the host rule (geometry.cpp: barcodes_from_bits) and the two kernels (barcodes.hip).  A scan line is a row of bits or a row of bitsT; it is read in
// READING coordinates u = 0..len - 1, pixel u forwards and pixel len - 1 - u backwards, so that one walk serves all four directions.  Integer arithmetic only;
// every value is below 2^31 (26 r, 64 S and the weighted check sum of 79 symbols stay below 2^22).  tests/barcodes_ref.py restates all of it on run lists.
//
// The bitmaps are tables.hip's (ink_tile.h), as marks_rule.h describes them; nothing here reads a word beyond a line's own ceil(len / 64).
#pragma once
#include <stdint.h>
#include "marks_rule.h"

namespace ttr {

constexpr int kBcMinLo = 4, kBcMinHi = 256;   // min_lines in 4..256
constexpr int kBcCap = 64;                    // barcodes per page
constexpr int kBcRec = 24;                    // x0, y0, x1, y1, symbology (1 = Code 128, 2 = Code 39), dir, lines, module64, flags, len, 0, 0, text [12]
constexpr int kBcText = 48;                   // bytes of text
constexpr int kBcLineHits = 8;                // hits a line keeps per direction
constexpr int kBcMaxSym = 80;                 // Code 128: start, data and check symbols together
constexpr int kBcLinkLines = 3;               // hits chain over at most this many lines
// flags of a record: bit 0 GS1 (FNC1 first), bit 1 FNC2, bit 2 FNC3, bit 3 FNC4
constexpr int kBcFlagsMask = 15;

// The side block of one page, int32: a header, then the records.
//   header  [0] mode (1, or -7: more than kBcCap barcodes)  [1] barcodes  [2] candidates examined (ink-run starts, both readings of every line)
//           [3] start patterns matched  [4] hits kept  [5] hits dropped (beyond 8 on a line and direction)  [6] chains below min_lines  [7] 0
//   records [64][24]  in (y0, x0, dir) order
constexpr int kBcHdr = 8;
constexpr int kBcSideInts = kBcHdr + kBcCap * kBcRec;
// a batch's side blocks: [pages][kBcSideInts] | [N] every item's barcode
constexpr size_t barcodes_side_bytes(int pages, int N) { return ((size_t)pages * kBcSideInts + (size_t)N) * 4; }

// A hit, int32 [20]: [0] p0  [1] p1 (pixels along the line, first bar to last)  [2] 64 x the module (narrow-run) width  [3] flags  [4] len  [5] symbology
// [6] the hit it chains to, -1 = none  [7] its chain's first hit  [8..19] text.  A line L (rows 0..h - 1, then columns) and a reading rev (0 forwards, 1
// backwards) own the slots ((2 L + rev) 8 + s) and the counters [4] = kept, dropped, candidates, starts at (2 L + rev).
constexpr int kBcHit = 20, kBcCnt = 4;

TTR_MARK_HD bool barcodes_args_ok(int min_lines, int ink, int symbologies) {
  return min_lines >= kBcMinLo && min_lines <= kBcMinHi && ink >= 1 && ink <= 255 && symbologies >= 1 && symbologies <= 3;
}

// ---- the tables: Code 128's values 0..105 as six widths in decimal digits, then the Stop's first six widths forwards (106) and reversed (107)
TTR_MARK_HD int bc128_pattern(int v) {
  static constexpr int32_t t[108] = {
      212222, 222122, 222221, 121223, 121322, 131222, 122213, 122312, 132212, 221213, 221312, 231212, 112232, 122132, 122231, 113222,
      123122, 123221, 223211, 221132, 221231, 213212, 223112, 312131, 311222, 321122, 321221, 312212, 322112, 322211, 212123, 212321,
      232121, 111323, 131123, 131321, 112313, 132113, 132311, 211313, 231113, 231311, 112133, 112331, 132131, 113123, 113321, 133121,
      313121, 211331, 231131, 213113, 213311, 213131, 311123, 311321, 331121, 312113, 312311, 332111, 314111, 221411, 431111, 111224,
      111422, 121124, 121421, 141122, 141221, 112214, 112412, 122114, 122411, 142112, 142211, 241211, 221114, 413111, 241112, 134111,
      111242, 121142, 121241, 114212, 124112, 124211, 411212, 421112, 421211, 212141, 214121, 412121, 111143, 111341, 131141, 114113,
      114311, 411113, 411311, 113141, 114131, 311141, 411131, 211412, 211214, 211232, 233111, 211133};
  return t[v];
}
// Code 39: the 43 characters and `*` as nine wide bits, first run = most significant
TTR_MARK_HD int bc39_pattern(int i) {
  static constexpr int16_t t[44] = {0x034, 0x121, 0x061, 0x160, 0x031, 0x130, 0x070, 0x025, 0x124, 0x064, 0x109, 0x049, 0x148, 0x019, 0x118,
                                    0x058, 0x00D, 0x10C, 0x04C, 0x01C, 0x103, 0x043, 0x142, 0x013, 0x112, 0x052, 0x007, 0x106, 0x046, 0x016,
                                    0x181, 0x0C1, 0x1C0, 0x091, 0x190, 0x0D0, 0x085, 0x184, 0x0C4, 0x0A8, 0x0A2, 0x08A, 0x02A, 0x094};
  return t[i];
}
TTR_MARK_HD int bc39_char(int i) {
  return i < 10 ? '0' + i : i < 36 ? 'A' + i - 10 : i == 36 ? '-' : i == 37 ? '.' : i == 38 ? ' ' : i == 39 ? '$' : i == 40 ? '/' : i == 41 ? '+' : i == 42 ? '%' : '*';
}
constexpr int kBc128Entries = 4096, kBc39Entries = 512, kBcTableBytes = kBc128Entries + kBc39Entries;
// the index of Code 128's value v in the 4096-entry table: its six widths minus one in two bits each, the first the most significant
TTR_MARK_HD int bc128_index(int v) {
  int p = bc128_pattern(v), idx = 0;
  for (int i = 0; i < 6; ++i) { idx |= (p % 10 - 1) << (2 * i); p /= 10; }
  return idx;
}
// the lookup tables [4096 + 512] bytes, 255 = no symbol: entries j, j + step, .. (a thread of a workgroup each, or the host with j = 0, step = 1)
TTR_MARK_HD void bc_tables_clear(uint8_t* t, int j, int step) { for (int i = j; i < kBcTableBytes; i += step) t[i] = 255; }
TTR_MARK_HD void bc_tables_fill(uint8_t* t, int j, int step) {
  for (int v = j; v < 108; v += step) t[bc128_index(v)] = (uint8_t)v;
  for (int v = j; v < 44; v += step) t[kBc128Entries + bc39_pattern(v)] = (uint8_t)v;
}

TTR_MARK_HD int bc_clz(uint64_t v) { return __builtin_clzll(v); }   // (v != 0)

// the number of consecutive pixels equal to val from pixel x on in direction step (+1 / -1), inside the line's pixels 0..len - 1 (0 <= x < len)
TTR_MARK_HD int bc_span(const uint64_t* line, int len, int x, int step, int val) {
  int n = 0, k = x >> 6, o = x & 63;
  if (step > 0) {
    const int nw = (len + 63) >> 6;
    while (k < nw) {
      uint64_t v = line[k] >> o;
      if (val) v = ~v;
      int c = v ? mark_ctz(v) : 64;
      if (c > 64 - o) c = 64 - o;
      n += c;
      if (c < 64 - o) break;
      ++k; o = 0;
    }
    return n < len - x ? n : len - x;
  }
  while (k >= 0) {
    uint64_t v = line[k] << (63 - o);
    if (val) v = ~v;
    int c = v ? bc_clz(v) : 64;
    if (c > o + 1) c = o + 1;
    n += c;
    if (c < o + 1) break;
    --k; o = 63;
  }
  return n;
}
// the same in reading coordinates: from u on in reading direction (back = 0) or against it (back = 1)
TTR_MARK_HD int bc_uspan(const uint64_t* line, int len, int rev, int u, int back, int val) { return bc_span(line, len, rev ? len - 1 - u : u, rev != back ? -1 : 1, val); }

// n runs from u on, ink first: their widths into r and their sum returned; 0 when the line ends before the n-th run begins
TTR_MARK_HD int bc_read(const uint64_t* line, int len, int rev, int u, int n, int* r) {
  int S = 0;
  for (int i = 0; i < n; ++i) {
    if (u + S >= len) return 0;
    const int c = bc_uspan(line, len, rev, u + S, 0, (i & 1) ^ 1);
    if (c == 0) return 0;   // (u is not where a run of ink begins: no caller does that)
    r[i] = c; S += c;
  }
  return S;
}
// the quiet zone: the q pixels without ink before u (back = 1, u > 0) or from u on (back = 0); the page's edge counts as a zone of any length.  True when
// den q >= num S.
TTR_MARK_HD bool bc_quiet(const uint64_t* line, int len, int rev, int u, int back, int num, int S, int den) {
  if (back ? u <= 0 : u >= len) return true;
  const int q = bc_uspan(line, len, rev, back ? u - 1 : u, back, 0);
  if (back ? u - q <= 0 : u + q >= len) return true;
  return den * q >= num * S;
}

// 3: Code 128's six runs of sum S -> the table's value, 255 when a measure leaves 1..4 or they do not sum to 11
TTR_MARK_HD int bc128_value(const uint8_t* tab, const int* r, int S) {
  int idx = 0, sum = 0;
  for (int i = 0; i < 6; ++i) {
    const int m = (22 * r[i] + S) / (2 * S);
    if (m < 1 || m > 4) return 255;
    idx = idx << 2 | (m - 1); sum += m;
  }
  return sum == 11 ? tab[idx] : 255;
}
// the Stop: seven runs of sum S measured against 13 modules must be 2331112
TTR_MARK_HD bool bc128_stop(const int* r, int S) {
  int p = 2331112;
  for (int i = 6; i >= 0; --i) {
    if ((26 * r[i] + S) / (2 * S) != p % 10) return false;
    p /= 10;
  }
  return true;
}

// 4: Code 128 from the candidate u0 (ink at u0, none before it).  Returns 0: no start pattern; 1: a start pattern and no hit; 2: a hit, and hit [20] (when
// not null) then holds its record but for [6] and [7].
TTR_MARK_HD int bc128_decode(const uint8_t* tab, const uint64_t* line, int len, int rev, int u0, int32_t* hit) {
  int r[7];
  const int S0 = bc_read(line, len, rev, u0, 6, r);
  if (!S0) return 0;
  const int start = bc128_value(tab, r, S0);
  if (start < 103 || start > 105) return 0;
  if (!bc_quiet(line, len, rev, u0, 1, 5, S0, 11)) return 1;
  int u = u0 + S0, prevS = S0, nsym = 1, sum = start, before = start, last = 0;
  for (;;) {
    if (nsym >= 3) {   // the Stop, once a data symbol and a check symbol can stand before it
      const int S7 = bc_read(line, len, rev, u, 7, r);
      const int d = 11 * S7 - 13 * prevS;
      if (S7 && bc128_stop(r, S7) && 4 * (d < 0 ? -d : d) <= 13 * prevS && bc_quiet(line, len, rev, u + S7, 0, 5, S7, 13)) {
        if (before % 103 != last) return 1;
        u += S7;   // (the Stop's last run is ink: u is now one past the last bar)
        break;
      }
    }
    const int S = bc_read(line, len, rev, u, 6, r);
    const int d = S - prevS;
    if (!S || 4 * (d < 0 ? -d : d) > prevS) return 1;
    const int v = bc128_value(tab, r, S);
    if (v >= 103 || nsym >= kBcMaxSym) return 1;
    before = sum; sum += nsym * v; last = v;
    ++nsym; prevS = S; u += S;
  }
  // the text: the nsym - 2 data symbols again, under the sets
  int set = start - 103, shift = 0, n = 0, flags = 0, w = u0 + S0;
  if (hit) for (int i = 0; i < kBcText / 4; ++i) hit[8 + i] = 0;
  for (int i = 0; i < nsym - 2; ++i) {
    const int S = bc_read(line, len, rev, w, 6, r);
    const int v = bc128_value(tab, r, S);
    w += S;
    int b0 = -1, b1 = -1;
    if (set == 2) {
      if (v < 100) { b0 = '0' + v / 10; b1 = '0' + v % 10; }
      else if (v == 100) set = 1;
      else if (v == 101) set = 0;
      else if (i == 0) flags |= 1; else b0 = 0x1D;
    } else {
      const int eff = shift ? 1 - set : set;
      shift = 0;
      if (v < 96) b0 = eff == 1 || v < 64 ? 32 + v : v - 64;
      else if (v == 96) flags |= 4;
      else if (v == 97) flags |= 2;
      else if (v == 98) shift = 1;
      else if (v == 99) set = 2;
      else if (v == 102) { if (i == 0) flags |= 1; else b0 = 0x1D; }
      else if ((v == 100) == (eff == 0)) set = 1 - eff;   // Code B in set A, Code A in set B
      else flags |= 8;                                    // FNC4
    }
    if (b0 >= 0) { if (hit && n < kBcText) hit[8 + (n >> 2)] |= b0 << (8 * (n & 3)); ++n; }
    if (b1 >= 0) { if (hit && n < kBcText) hit[8 + (n >> 2)] |= b1 << (8 * (n & 3)); ++n; }
  }
  if (n > kBcText) return 1;
  if (hit) {
    const int span = u - u0;
    hit[0] = rev ? len - u : u0; hit[1] = rev ? len - 1 - u0 : u - 1;
    hit[2] = 64 * span / (11 * nsym + 13); hit[3] = flags; hit[4] = n; hit[5] = 1;
  }
  return 2;
}

// 5: a Code 39 character from u on: its index 0..43 (43 = `*`), -1 when there is none; *S its width, *mn its narrowest run, *narrow the sum of its six narrow runs
TTR_MARK_HD int bc39_read(const uint8_t* tab, const uint64_t* line, int len, int rev, int u, int* S, int* mn_out, int* narrow) {
  int r[9];
  *S = bc_read(line, len, rev, u, 9, r);
  if (!*S) return -1;
  int mn = r[0], mx = r[0];
  for (int i = 1; i < 9; ++i) { mn = r[i] < mn ? r[i] : mn; mx = r[i] > mx ? r[i] : mx; }
  int bits = 0, wide = 0, wmin = mx, nmax = mn, nsum = 0;
  for (int i = 0; i < 9; ++i) {
    const bool wd = 2 * r[i] > mn + mx;
    bits = bits << 1 | (wd ? 1 : 0);
    if (wd) { ++wide; wmin = r[i] < wmin ? r[i] : wmin; } else { nmax = r[i] > nmax ? r[i] : nmax; nsum += r[i]; }
  }
  if (wide != 3 || 2 * wmin < 3 * nmax) return -1;
  *mn_out = mn; *narrow = nsum;
  const int v = tab[kBc128Entries + bits];
  return v == 255 ? -1 : v;
}
// 5: Code 39 from the candidate u0; as bc128_decode
TTR_MARK_HD int bc39_decode(const uint8_t* tab, const uint64_t* line, int len, int rev, int u0, int32_t* hit) {
  int S, mn, ns;
  if (bc39_read(tab, line, len, rev, u0, &S, &mn, &ns) != 43) return 0;
  if (!bc_quiet(line, len, rev, u0, 1, 5, mn, 1)) return 1;
  if (hit) for (int i = 0; i < kBcText / 4; ++i) hit[8 + i] = 0;
  int u = u0 + S, n = 0, narrow = ns, chars = 1;
  for (;;) {
    if (u >= len) return 1;
    const int g = bc_uspan(line, len, rev, u, 0, 0);
    if (3 * g > S || u + g >= len) return 1;
    int S2;
    const int v = bc39_read(tab, line, len, rev, u + g, &S2, &mn, &ns);
    const int d = S2 - S;
    if (v < 0 || 4 * (d < 0 ? -d : d) > S) return 1;
    u += g + S2; S = S2; narrow += ns; ++chars;
    if (v == 43) break;
    if (n >= kBcText) return 1;   // a text over 48 bytes is no hit
    if (hit) hit[8 + (n >> 2)] |= bc39_char(v) << (8 * (n & 3));
    ++n;
  }
  if (n < 1 || !bc_quiet(line, len, rev, u, 0, 5, mn, 1)) return 1;
  if (hit) {
    hit[0] = rev ? len - u : u0; hit[1] = rev ? len - 1 - u0 : u - 1;
    hit[2] = 64 * narrow / (6 * chars); hit[3] = 0; hit[4] = n; hit[5] = 2;
  }
  return 2;
}
// 4 - 5 on one candidate: Code 128 first, Code 39 where that gave no hit.  *starts counts the start patterns matched.
TTR_MARK_HD bool bc_decode(const uint8_t* tab, const uint64_t* line, int len, int rev, int u0, int symbologies, int32_t* hit, int* starts) {
  if (symbologies & 1) {
    const int a = bc128_decode(tab, line, len, rev, u0, hit);
    *starts += a ? 1 : 0;
    if (a == 2) return true;
  }
  if (symbologies & 2) {
    const int a = bc39_decode(tab, line, len, rev, u0, hit);
    *starts += a ? 1 : 0;
    if (a == 2) return true;
  }
  return false;
}
// 4: the candidates among the 64 pixels of word k of a line of nw words: ink with no ink before it in reading direction
TTR_MARK_HD uint64_t bc_candidates(const uint64_t* line, int nw, int k, int rev) {
  const uint64_t w = line[k];
  if (!rev) return w & ~(w << 1 | (k ? line[k - 1] >> 63 : 0));
  return w & ~(w >> 1 | (k + 1 < nw ? line[k + 1] << 63 : 0));
}

// 7: hit a chains to hit b (of a line up to three before it, in the same reading): symbology, flags and text agree, and they overlap by half the shorter
TTR_MARK_HD bool bc_link(const int32_t* a, const int32_t* b) {
  for (int i = 3; i < kBcHit; ++i)
    if (i != 6 && i != 7 && a[i] != b[i]) return false;
  const int lo = a[0] > b[0] ? a[0] : b[0], hi = a[1] < b[1] ? a[1] : b[1];
  const int la = a[1] - a[0] + 1, lb = b[1] - b[0] + 1;
  return 2 * (hi - lo + 1) >= (la < lb ? la : lb);
}
// 7: the hit that slot s of line L, reading rev, chains to: the nearest line before it first (not before L0, the first line of its kind), the lowest slot
// first; -1 when there is none.  A hit has one such partner, so chains are trees and a chain is a tree's hits: a function of the hit set alone.
TTR_MARK_HD int bc_pred(const int32_t* hits, const int32_t* cnt, int L0, int L, int rev, int s) {
  const int32_t* a = hits + (size_t)((2 * L + rev) * kBcLineHits + s) * kBcHit;
  for (int d = 1; d <= kBcLinkLines && L - d >= L0; ++d) {
    const int q = 2 * (L - d) + rev;
    for (int t = 0; t < cnt[kBcCnt * q]; ++t)
      if (bc_link(a, hits + (size_t)(q * kBcLineHits + t) * kBcHit)) return q * kBcLineHits + t;
  }
  return -1;
}
// 7: the chain whose first hit is slot s of line L: rec [24] (zero-filled by the caller) gets the record; returns its hit count.  L1 = one past the last
// line of its kind; col = the lines are columns.  Every hit's [7] names its chain's first hit by now.
TTR_MARK_HD int bc_chain(const int32_t* hits, const int32_t* cnt, int L0, int L1, int L, int rev, int s, int col, int32_t* rec) {
  const int id = (2 * L + rev) * kBcLineHits + s;
  const int32_t* a = hits + (size_t)id * kBcHit;
  int n = 1, p0 = a[0], p1 = a[1], last = L, mod = a[2];
  for (int M = L + 1, miss = 0; M < L1 && miss < kBcLinkLines; ++M) {
    const int q = 2 * M + rev;
    bool found = false;
    for (int t = 0; t < cnt[kBcCnt * q]; ++t) {
      const int32_t* b = hits + (size_t)(q * kBcLineHits + t) * kBcHit;
      if (b[7] != id) continue;
      found = true; ++n; mod += b[2]; last = M;
      p0 = b[0] < p0 ? b[0] : p0; p1 = b[1] > p1 ? b[1] : p1;
    }
    miss = found ? 0 : miss + 1;
  }
  rec[0] = col ? L - L0 : p0; rec[1] = col ? p0 : L - L0; rec[2] = col ? last - L0 : p1; rec[3] = col ? p1 : last - L0;
  rec[4] = a[5]; rec[5] = 2 * rev + col; rec[6] = n; rec[7] = mod / n; rec[8] = a[3]; rec[9] = a[4];
  for (int i = 0; i < kBcText / 4; ++i) rec[12 + i] = a[8 + i];
  return n;
}
// 8: record a comes before record b: (y0, x0, dir) order, then the chains' first hits' order
TTR_MARK_HD bool bc_before(const int32_t* a, int ida, const int32_t* b, int idb) {
  if (a[1] != b[1]) return a[1] < b[1];
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[5] != b[5]) return a[5] < b[5];
  return ida < idb;
}
// 9: the barcode of an item at (cx, cy) = 64 x its centre: the first whose box holds the centre; -1 when there is none or the page is beyond the cap
TTR_MARK_HD int bc_item(const int32_t* side, int cx, int cy) {
  if (side[0] != 1) return -1;
  for (int m = 0; m < side[1]; ++m) {
    const int32_t* r = side + kBcHdr + kBcRec * m;
    if (cx >= 64 * r[0] && cx < 64 * (r[2] + 1) && cy >= 64 * r[1] && cy < 64 * (r[3] + 1)) return m;
  }
  return -1;
}

}  // namespace ttr
