// The selection-marks host rule (tuatara_amd/csrc/geometry.cpp + marks_rule.h; DESIGN.md "Selection marks") under sanitizers: a stand-alone program, host code
// only.
//   marks_san <seed> <pages>   drives tables_ink, marks_transpose, marks_from_bits, marks_from_page (under both ink rules), marks_items and marks_side_valid over
//                              seeded pages of the kinds the tests use - random bits, frames of random side, thickness and aspect with crosses inside, frames on
//                              the page's edges and across word boundaries, sides up to 128, a grid of 8-px boxes beyond the cap (mode -6), widths about the word
//                              size, padded strides - with the page, both bitmaps and every output in exactly sized heap buffers, so that any access outside
//                              them (a run read beyond a line's last word, a row beyond the page), and any signed overflow, is a sanitizer report.
//                              Prints "pages P marks M selected S overflows O".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/geometry.h"
#include "../../tuatara_amd/csrc/marks_rule.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: marks_san <seed> <pages>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int pages = std::atoi(argv[2]);
  long n_marks = 0, n_sel = 0, n_over = 0;
  const int widths[8] = {1, 63, 64, 65, 129, 193, 200, 300};
  for (int t = 0; t < pages; ++t) {
    const int kind = t % 6;
    int h = 1 + (int)(rng() % 200), w = widths[rng() % 8];
    if (kind == 3) { h = 170; w = 324; }
    if (kind == 4) { h = 150; w = 200; }
    const int pad = (int)(rng() % 3) * 5, stride = w * 3 + pad;
    std::vector<uint8_t> page((size_t)h * stride, 255);
    auto dark = [&](int y, int x) { if (y >= 0 && y < h && x >= 0 && x < w) for (int c = 0; c < 3; ++c) page[(size_t)y * stride + 3 * x + c] = (uint8_t)(rng() % 100); };
    auto frame = [&](int x, int y, int sx, int sy, int th) {
      for (int k = 0; k < th; ++k) {
        for (int i = 0; i < sx; ++i) { dark(y + k, x + i); dark(y + sy - 1 - k, x + i); }
        for (int j = 0; j < sy; ++j) { dark(y + j, x + k); dark(y + j, x + sx - 1 - k); }
      }
    };
    if (kind == 0) for (size_t i = 0; i < page.size(); ++i) page[i] = (rng() % 10) < 7 ? 0 : 255;
    if (kind == 1 || kind == 2) {   // frames anywhere, the page's edges included (kind 2: some cut by them)
      const int n = 1 + (int)(rng() % 10);
      for (int i = 0; i < n; ++i) {
        const int sx = 6 + (int)(rng() % 130), sy = std::max(4, sx + (int)(rng() % 9) - 4);
        const int x = kind == 2 ? (int)(rng() % (unsigned)(w + 1)) - 3 : (w > sx ? (int)(rng() % (unsigned)(w - sx + 1)) : 0);
        const int y = kind == 2 ? (int)(rng() % (unsigned)(h + 1)) - 3 : (h > sy ? (int)(rng() % (unsigned)(h - sy + 1)) : 0);
        frame(x, y, sx, sy, 1 + (int)(rng() % 4));
        if (rng() % 2) for (int k = 0; k < sx / 2; ++k) { dark(y + sy / 4 + k, x + sx / 4 + k); dark(y + sy / 4 + k, x + sx / 4 + sx / 2 - 1 - k); }
      }
    }
    if (kind == 3) for (int k = 0; k < 513; ++k) frame(2 + 10 * (k % 32), 2 + 10 * (k / 32), 8, 8, 1);   // 513 boxes of 8 px at 10-px pitch
    if (kind == 4) { frame(58, 40, 17, 17, 1); frame(30, 20, 128, 128, 2); frame(0, 0, 12, 12, 1); frame(w - 12, h - 12, 12, 12, 1); }   // (the 17-px one inside the 128-px one)
    if (kind == 4) for (int k = 0; k < 8; ++k) { dark(44 + k, 62 + k); dark(44 + k, 69 - k); }                   // ... and ticked
    if (kind == 5) for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) if (rng() % 50 == 0) dark(y, x);
    const int min_side = kind == 3 || kind == 4 ? 8 : 8 + (int)(rng() % 20), max_side = kind == 4 ? 128 : min_side + (int)(rng() % (unsigned)(129 - min_side));
    const int fill = kind == 4 ? 20 : 1 + (int)(rng() % 255), ink = kind >= 3 ? 128 : 1 + (int)(rng() % 255);
    if (!marks_args_ok(min_side, max_side, fill, ink) || marks_args_ok(7, max_side, fill, ink) || marks_args_ok(65, 128, fill, ink) || marks_args_ok(min_side, min_side - 1, fill, ink) ||
        marks_args_ok(min_side, 129, fill, ink) || marks_args_ok(min_side, max_side, 0, ink) || marks_args_ok(min_side, max_side, 256, ink) || marks_args_ok(min_side, max_side, fill, 0))
      return fail("marks_args_ok");
    std::vector<uint64_t> bits(tables_bitmap_words(h, w)), bitsT(tables_bitmap_words(w, h));
    tables_ink(page.data(), h, w, stride, ink, bits.data());
    marks_transpose(bits.data(), h, w, bitsT.data());
    std::vector<int32_t> side(kMarkSideInts), side2(kMarkSideInts), counts((size_t)2 * ((h + 31) / 32)), side3(kMarkSideInts);
    const int mode = marks_from_bits(bits.data(), bitsT.data(), h, w, min_side, max_side, fill, side.data(), counts.data());
    if (marks_from_page(page.data(), h, w, stride, min_side, max_side, fill, ink, side2.data()) != mode || side != side2) return fail("marks_from_page and marks_from_bits differ");
    if (kind == 3 && mode != -6) return fail("513 boxes: mode " + std::to_string(mode));
    if (kind == 4 && (mode != 1 || side[1] != 4)) return fail("the drawn boxes: " + std::to_string(side[1]) + " marks where 4 were drawn");
    long kept = 0, corners = 0;
    for (size_t b = 0; b < counts.size() / 2; ++b) { kept += counts[2 * b]; corners += counts[2 * b + 1]; }
    if (kept != side[3] || corners != side[2]) return fail("the band counts do not add up to the header's");
    const int nq = (int)(rng() % 50);
    std::vector<int32_t> centres((size_t)nq * 2), item_mark((size_t)nq);
    for (int i = 0; i < nq; ++i) {
      float q[8];
      const float cx = (float)((double)(rng() % 20000) / 64. - 20.), cy = (float)((double)(rng() % 14000) / 64. - 20.);
      const float qq[8] = {cx - 5, cy - 2, cx + 5, cy - 2, cx + 5, cy + 2, cx - 5, cy + 2};
      for (int k = 0; k < 8; ++k) q[k] = i % 16 == 15 ? (k & 1 ? -32767.f : 32767.f) : qq[k];
      if (!region_quad_ok(q)) return fail("a generated quad left the rule's domain");
      tables_word_centre(q, &centres[2 * (size_t)i]);
    }
    marks_items(side.data(), centres.data(), nq, item_mark.data());
    std::string why;
    if (mode != side[0] || !marks_side_valid(side.data(), h, w, fill, nq, &why)) return fail("a block decode_pages would refuse: " + why);
    for (int i = 0; i < nq; ++i)
      if (item_mark[(size_t)i] < -1 || item_mark[(size_t)i] >= side[1]) return fail("marks_items: an index out of range");
    if (h >= 3 && w >= 3) {   // the same under the local rule's bitmap
      const int lm = marks_from_page(page.data(), h, w, stride, min_side, max_side, fill, InkRule::local(1 + (int)(rng() % 64), 1 + (int)(rng() % 255), (int)(rng() % 3)), side3.data());
      if (lm != side3[0] || !marks_side_valid(side3.data(), h, w, fill, 0, &why)) return fail("marks_from_page under the local rule: a block decode_pages would refuse: " + why);
    }
    if (mode == 1 && side[1] > 0) {   // what decode_pages must refuse
      std::vector<int32_t> bad = side;
      bad[0] = 2;
      if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts a mode of 2");
      bad = side; bad[1] = kMarkCap + 1;
      if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts 513 marks");
      bad = side; bad[kMarkHdr + 2] = w;
      if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts a box beyond the page");
      bad = side; bad[kMarkHdr + 4] = bad[kMarkHdr];
      if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts an interior on its frame");
      bad = side; bad[kMarkHdr + 8] = bad[kMarkHdr + 9] + 1;
      if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts more ink than area");
      bad = side; bad[kMarkHdr + 10] ^= 1;
      if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts a state that is not the rule's");
      bad = side; bad[kMarkHdr + 11] = nq;
      if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts a label that is no item");
      if (side[1] > 1) {
        bad = side;
        for (int k = 0; k < kMarkRec; ++k) std::swap(bad[kMarkHdr + k], bad[kMarkHdr + kMarkRec + k]);
        if (marks_side_valid(bad.data(), h, w, fill, nq)) return fail("marks_side_valid accepts marks out of order");
      }
    }
    n_marks += side[1]; n_over += mode != 1;
    for (int m = 0; m < side[1]; ++m) n_sel += side[kMarkHdr + kMarkRec * m + 10];
  }
  std::cout << "pages " << pages << " marks " << n_marks << " selected " << n_sel << " overflows " << n_over << std::endl;
  return 0;
}
