// The tables host rule (tuatara_amd/csrc/geometry.cpp + tables_rule.h; DESIGN.md "Tables") under sanitizers: a stand-alone program, host code only.
//   tables_san <seed> <pages>   drives tables_ink, tables_runs, tables_from_page, tables_words, tables_export and tables_side_valid over seeded pages of the
//                               kinds the tests use - random bits, drawn grids with gaps in their borders, dashes beyond the run cap, combs beyond the ruling
//                               cap, a table of 66 row lines, a grid of 34 x 34 cells and a page beyond two caps at once (modes -6, -7, -2), rulings on the
//                               page's edges, widths about the word size, padded strides - with the page and every output in exactly
//                               sized heap buffers, so that any access outside them, and any signed overflow, is a sanitizer report.
//                               Prints "pages P tables T cells C overflows O".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/geometry.h"
#include "../../tuatara_amd/csrc/tables_rule.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: tables_san <seed> <pages>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int pages = std::atoi(argv[2]);
  long n_tables = 0, n_cells = 0, n_over = 0;
  const int widths[8] = {1, 63, 64, 65, 129, 193, 200, 300};
  for (int t = 0; t < pages; ++t) {
    const int kind = t % 8;
    int h = 1 + (int)(rng() % 200), w = widths[rng() % 8];
    if (kind == 2) { h = 400; w = 400; }
    if (kind == 3) { h = 600; w = 40; }
    if (kind == 5) { h = 540; w = 100; }
    if (kind == 6) { h = 290; w = 290; }
    if (kind == 7) { h = 600; w = 700; }
    const int pad = (int)(rng() % 3) * 5, stride = w * 3 + pad;
    std::vector<uint8_t> page((size_t)h * stride, 255);
    auto dark = [&](int y, int x) { if (y >= 0 && y < h && x >= 0 && x < w) for (int c = 0; c < 3; ++c) page[(size_t)y * stride + 3 * x + c] = (uint8_t)(rng() % 100); };
    if (kind == 0) for (size_t i = 0; i < page.size(); ++i) page[i] = (rng() % 10) < 7 ? 0 : 255;
    if (kind == 1 || kind == 4) {   // a grid of 2..6 x 2..6 lines, some borders broken; kind 4 reaches the page's edges
      const int nr = 2 + (int)(rng() % 5), nc = 2 + (int)(rng() % 5), m = kind == 4 ? 0 : 5;
      for (int i = 0; i < nr; ++i) {
        const int y = m + (int)((long)(h - 1 - 2 * m) * i / (nr - 1));
        for (int x = m; x < w - m; ++x) if (rng() % 40) { dark(y, x); dark(y + 1, x); }
      }
      for (int j = 0; j < nc; ++j) {
        const int x = m + (int)((long)(w - 1 - 2 * m) * j / (nc - 1));
        for (int y = m; y < h - m; ++y) if (rng() % 40) { dark(y, x); dark(y, x + 1); }
      }
    }
    if (kind == 2) for (int y = 0; y < h; ++y) for (int x = 0; x + 12 < w; x += 16) for (int k = 0; k < 12; ++k) dark(y, x + k);
    if (kind == 3 || kind == 7) for (int y = 0; y < h; y += 2) for (int x = 4; x < 36; ++x) dark(y, x);
    if (kind == 5) {   // 66 row lines between two column lines
      for (int i = 0; i < 66; ++i) for (int x = 10; x < 90; ++x) dark(4 + 8 * i, x);
      for (int y = 4; y <= 4 + 8 * 65; ++y) { dark(y, 10); dark(y, 89); }
    }
    if (kind == 6) for (int i = 0; i < 35; ++i) for (int k = 0; k <= 8 * 34; ++k) { dark(5 + 8 * i, 5 + k); dark(5 + k, 5 + 8 * i); }
    if (kind == 7) for (int y = 0; y + 12 < h; y += 16) for (int k = 0; k < 12; ++k) for (int x = 100; x < 600; ++x) dark(y + k, x);
    const int min_len = 16 + (int)(rng() % 40), ink = kind >= 5 ? 128 : 1 + (int)(rng() % 255);
    const int want_mode = kind == 5 ? -6 : kind == 6 ? -7 : kind == 7 ? -2 : 0;
    if (!tables_args_ok(min_len, ink) || tables_args_ok(15, ink) || tables_args_ok(4097, ink) || tables_args_ok(min_len, 0) || tables_args_ok(min_len, 256))
      return fail("tables_args_ok");
    std::vector<uint64_t> bits(tables_bitmap_words(h, w));
    std::vector<int32_t> side(kTabSideInts), runs((size_t)2 * kTabRunCap * 3);
    const int mode = tables_from_page(page.data(), h, w, stride, min_len, ink, side.data(), runs.data(), bits.data());
    if (want_mode && mode != want_mode) return fail("tables_from_page: mode " + std::to_string(mode) + " where the page was made for " + std::to_string(want_mode));
    std::string why;
    if (mode != side[0] || !tables_side_valid(side.data(), &why)) return fail("tables_from_page: a block decode_pages would refuse: " + why);
    std::vector<uint64_t> bits2(bits.size());
    tables_ink(page.data(), h, w, stride, ink, bits2.data());
    if (bits != bits2) return fail("tables_ink: two passes differ");
    for (int dir = 0; dir < 2; ++dir) {
      std::vector<int32_t> rn((size_t)kTabRunCap * 3);
      const int n = tables_runs(bits.data(), h, w, dir, rn.data());
      if ((n > kTabRunCap && mode != -2) || (mode == 1 && n != side[5 + dir])) return fail("tables_runs: count");
      for (int i = 0; i < n && i < kTabRunCap; ++i)
        if (rn[3 * i + 2] - rn[3 * i + 1] + 1 < kTabR || rn[3 * i + 1] < 0 || rn[3 * i + 2] >= (dir ? h : w) || rn[3 * i] >= (dir ? w : h)) return fail("tables_runs: a run out of range");
    }
    int32_t counts[4];
    tables_export(side.data(), counts, nullptr, nullptr, nullptr, nullptr);
    std::vector<int32_t> rul((size_t)counts[0] * 6), tab((size_t)counts[1] * 8), lin((size_t)counts[3]), cel((size_t)counts[2] * 9);
    tables_export(side.data(), counts, rul.data(), tab.data(), lin.data(), cel.data());
    const int nq = (int)(rng() % 50);
    std::vector<int32_t> centres((size_t)nq * 2), items((size_t)nq * 2);
    for (int i = 0; i < nq; ++i) {
      float q[8];
      const float cx = (float)((double)(rng() % 40000) / 64. - 100.), cy = (float)((double)(rng() % 30000) / 64. - 100.);
      const float qq[8] = {cx - 5, cy - 2, cx + 5, cy - 2, cx + 5, cy + 2, cx - 5, cy + 2};
      for (int k = 0; k < 8; ++k) q[k] = i % 16 == 15 ? (k & 1 ? -32767.f : 32767.f) : qq[k];
      if (!region_quad_ok(q)) return fail("a generated quad left the rule's domain");
      tables_word_centre(q, &centres[2 * (size_t)i]);
    }
    tables_words(side.data(), centres.data(), nq, items.data());
    for (int i = 0; i < nq; ++i) {
      const int tt = items[2 * (size_t)i], cc = items[2 * (size_t)i + 1];
      if (tt == -1 && cc == -1) continue;
      if (tt < 0 || tt >= counts[1] || cc < tab[8 * (size_t)tt + 6] || cc >= tab[8 * (size_t)tt + 6] + tab[8 * (size_t)tt + 7]) return fail("tables_words: an index out of range");
    }
    // what decode_pages must refuse
    if (mode == 1) {
      std::vector<int32_t> bad = side;
      bad[0] = 2;
      if (tables_side_valid(bad.data())) return fail("tables_side_valid accepts a mode of 2");
      bad = side; bad[3] = kTabTableCap + 1;
      if (tables_side_valid(bad.data())) return fail("tables_side_valid accepts 33 tables");
      if (counts[2] > 0) {
        bad = side; bad[kTabCells + 3] += 1000;
        if (tables_side_valid(bad.data())) return fail("tables_side_valid accepts a cell beyond its grid");
        bad = side; bad[kTabCells + 1] = -1;
        if (tables_side_valid(bad.data())) return fail("tables_side_valid accepts a negative row");
      }
    }
    n_tables += counts[1]; n_cells += counts[2]; n_over += mode != 1;
  }
  std::cout << "pages " << pages << " tables " << n_tables << " cells " << n_cells << " overflows " << n_over << std::endl;
  return 0;
}
