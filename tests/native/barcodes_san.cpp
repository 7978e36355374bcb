// The barcode host rule (tuatara_amd/csrc/geometry.cpp + barcodes_rule.h; DESIGN.md "Barcodes") under sanitizers: a stand-alone program, host code only.
//   barcodes_san <seed> <pages>   drives tables_ink, marks_transpose, barcodes_from_bits, barcodes_from_page (under both ink rules), barcodes_items and
//                                 barcodes_side_valid over seeded pages of the kinds the tests use - random bits, Code 128 and Code 39 codes of random text,
//                                 module, place and direction, codes on and cut by the page's edges and across word boundaries, codes cut short, 65 codes on
//                                 a page (mode -7), widths about the word size, padded strides - with the page, both bitmaps and every output in exactly sized
//                                 heap buffers, so that any access outside them (a run read beyond a line's last word, a line beyond the page), and any signed
//                                 overflow, is a sanitizer report.  Prints "pages P barcodes B hits H overflows O".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/barcodes_rule.h"
#include "../../tuatara_amd/csrc/geometry.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

// a code's runs in modules, bar first
static std::vector<int> code128(std::mt19937& rng, int n) {
  std::vector<int> vals{103 + (int)(rng() % 3)};
  for (int i = 0; i < n; ++i) vals.push_back((int)(rng() % 103));
  long sum = vals[0];
  for (int i = 1; i <= n; ++i) sum += (long)i * vals[i];
  vals.push_back((int)(sum % 103));
  std::vector<int> runs;
  for (int v : vals) { const std::string p = std::to_string(bc128_pattern(v)); for (char c : p) runs.push_back(c - '0'); }
  for (char c : std::string("2331112")) runs.push_back(c - '0');
  return runs;
}
static std::vector<int> code39(std::mt19937& rng, int n) {
  std::vector<int> runs;
  for (int k = 0; k < n + 2; ++k) {
    const int bits = bc39_pattern(k == 0 || k == n + 1 ? 43 : (int)(rng() % 43));
    if (k) runs.push_back(1);
    for (int i = 0; i < 9; ++i) runs.push_back(bits >> (8 - i) & 1 ? 3 : 1);
  }
  return runs;
}

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: barcodes_san <seed> <pages>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int pages = std::atoi(argv[2]);
  long n_codes = 0, n_hits = 0, n_over = 0;
  const int widths[8] = {1, 63, 64, 65, 129, 193, 260, 400};
  for (int t = 0; t < pages; ++t) {
    const int kind = t % 5;
    int h = 1 + (int)(rng() % 200), w = widths[rng() % 8];
    if (kind == 3) { h = 80; w = 500; }
    const int pad = (int)(rng() % 3) * 5, stride = w * 3 + pad;
    std::vector<uint8_t> page((size_t)h * stride, 255);
    auto dark = [&](int y, int x) { if (y >= 0 && y < h && x >= 0 && x < w) for (int c = 0; c < 3; ++c) page[(size_t)y * stride + 3 * x + c] = (uint8_t)(rng() % 100); };
    // the runs drawn from (x, y) on in direction dir, `across` pixels high, the first `keep` runs of them
    auto draw = [&](const std::vector<int>& runs, int module, int x, int y, int across, int dir, size_t keep) {
      int total = 0;
      for (int r : runs) total += r * module;
      int pos = 0;
      for (size_t i = 0; i < runs.size() && i < keep; pos += runs[i] * module, ++i) {
        if (i & 1) continue;
        for (int p = pos; p < pos + runs[i] * module; ++p)
          for (int a = 0; a < across; ++a) {
            const int q = dir >= 2 ? total - 1 - p : p;
            if (dir & 1) dark(y + q, x + a); else dark(y + a, x + q);
          }
      }
    };
    if (kind == 0) for (size_t i = 0; i < page.size(); ++i) page[i] = (rng() % 10) < 5 ? 0 : 255;
    if (kind == 1 || kind == 2) {   // codes anywhere (kind 2: some cut by the page's edges or cut short)
      const int n = 1 + (int)(rng() % 4);
      for (int i = 0; i < n; ++i) {
        const std::vector<int> runs = rng() % 2 ? code128(rng, 1 + (int)(rng() % 6)) : code39(rng, 1 + (int)(rng() % 4));
        const int x = (int)(rng() % (unsigned)(w + 1)) - (kind == 2 ? 3 : 0), y = (int)(rng() % (unsigned)(h + 1)) - (kind == 2 ? 3 : 0);
        draw(runs, 1 + (int)(rng() % 3), kind == 1 ? x / 3 : x, kind == 1 ? y / 3 : y, 4 + (int)(rng() % 20), (int)(rng() % 4), kind == 2 && rng() % 3 == 0 ? rng() % runs.size() : runs.size());
      }
    }
    if (kind == 3) {   // 65 short Code 39 codes, 8 on a line
      std::mt19937 fixed(7);
      const std::vector<int> runs = code39(fixed, 1);
      for (int k = 0; k < 65; ++k) draw(runs, 1, 4 + 55 * (k % 8), 2 + 8 * (k / 8), 5, 0, runs.size());
    }
    if (kind == 4) for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) if (rng() % 6 == 0) dark(y, x);
    const int min_lines = kind == 3 ? 4 : 4 + (int)(rng() % 8), sym = 1 + (int)(rng() % 3), ink = kind == 3 ? 128 : 1 + (int)(rng() % 255);
    const int syms = kind == 3 ? 3 : sym;
    if (!barcodes_args_ok(min_lines, ink, syms) || barcodes_args_ok(3, ink, syms) || barcodes_args_ok(257, ink, syms) || barcodes_args_ok(min_lines, 0, syms) ||
        barcodes_args_ok(min_lines, 256, syms) || barcodes_args_ok(min_lines, ink, 0) || barcodes_args_ok(min_lines, ink, 4))
      return fail("barcodes_args_ok");
    std::vector<uint64_t> bits(tables_bitmap_words(h, w)), bitsT(tables_bitmap_words(w, h));
    tables_ink(page.data(), h, w, stride, ink, bits.data());
    marks_transpose(bits.data(), h, w, bitsT.data());
    std::vector<int32_t> side(kBcSideInts), side2(kBcSideInts), side3(kBcSideInts), hits((size_t)(h + w) * 2 * kBcLineHits * kBcHit), cnt((size_t)(h + w) * 2 * kBcCnt);
    const int mode = barcodes_from_bits(bits.data(), bitsT.data(), h, w, min_lines, syms, side.data(), hits.data(), cnt.data());
    if (barcodes_from_page(page.data(), h, w, stride, min_lines, ink, syms, side2.data()) != mode || side != side2) return fail("barcodes_from_page and barcodes_from_bits differ");
    if (kind == 3 && (mode != -7 || side[1] != 0 || side[4] != 65 * 5 || side[5] != 0)) return fail("65 codes: mode " + std::to_string(mode) + ", " + std::to_string(side[4]) + " hits");
    long kept = 0, dropped = 0, cands = 0, starts = 0;
    for (size_t q = 0; q < cnt.size() / kBcCnt; ++q) { kept += cnt[kBcCnt * q]; dropped += cnt[kBcCnt * q + 1]; cands += cnt[kBcCnt * q + 2]; starts += cnt[kBcCnt * q + 3]; }
    if (kept != side[4] || dropped != side[5] || cands != side[2] || starts != side[3]) return fail("the lines' counters do not add up to the header's");
    const int nq = (int)(rng() % 50);
    std::vector<int32_t> centres((size_t)nq * 2), item((size_t)nq);
    for (int i = 0; i < nq; ++i) {
      float q[8];
      const float cx = (float)((double)(rng() % 30000) / 64. - 20.), cy = (float)((double)(rng() % 14000) / 64. - 20.);
      const float qq[8] = {cx - 5, cy - 2, cx + 5, cy - 2, cx + 5, cy + 2, cx - 5, cy + 2};
      for (int k = 0; k < 8; ++k) q[k] = i % 16 == 15 ? (k & 1 ? -32767.f : 32767.f) : qq[k];
      if (!region_quad_ok(q)) return fail("a generated quad left the rule's domain");
      tables_word_centre(q, &centres[2 * (size_t)i]);
    }
    barcodes_items(side.data(), centres.data(), nq, item.data());
    std::string why;
    if (mode != side[0] || !barcodes_side_valid(side.data(), h, w, min_lines, syms, &why)) return fail("a block decode_pages would refuse: " + why);
    for (int i = 0; i < nq; ++i)
      if (item[(size_t)i] < -1 || item[(size_t)i] >= side[1]) return fail("barcodes_items: an index out of range");
    if (h >= 3 && w >= 3) {   // the same under the local rule's bitmap
      const int lm = barcodes_from_page(page.data(), h, w, stride, min_lines, InkRule::local(1 + (int)(rng() % 64), 1 + (int)(rng() % 255), (int)(rng() % 3)), syms, side3.data());
      if (lm != side3[0] || !barcodes_side_valid(side3.data(), h, w, min_lines, syms, &why)) return fail("barcodes_from_page under the local rule: a block decode_pages would refuse: " + why);
    }
    if (mode == 1 && side[1] > 0) {   // what decode_pages must refuse
      std::vector<int32_t> bad = side;
      bad[0] = 2;
      if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts a mode of 2");
      bad = side; bad[1] = kBcCap + 1;
      if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts 65 barcodes");
      bad = side; bad[kBcHdr + 2] = w;
      if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts a box beyond the page");
      bad = side; bad[kBcHdr + 4] = 3;
      if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts a symbology of 3");
      bad = side; bad[kBcHdr + 5] = 4;
      if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts a direction of 4");
      bad = side; bad[kBcHdr + 8] = 16;
      if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts flags beyond the mask");
      bad = side; bad[kBcHdr + 9] = 49;
      if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts a text of 49 bytes");
      bad = side; bad[kBcHdr + kBcRec - 1] |= 0x41000000;
      if (side[kBcHdr + 9] < kBcText && barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts bytes beyond the text");
      if (side[1] > 1) {
        bad = side;
        for (int k = 0; k < kBcRec; ++k) std::swap(bad[kBcHdr + k], bad[kBcHdr + kBcRec + k]);
        if (barcodes_side_valid(bad.data(), h, w, min_lines, syms)) return fail("barcodes_side_valid accepts barcodes out of order");
      }
    }
    n_codes += side[1]; n_hits += side[4]; n_over += mode != 1;
  }
  std::cout << "pages " << pages << " barcodes " << n_codes << " hits " << n_hits << " overflows " << n_over << std::endl;
  return 0;
}
