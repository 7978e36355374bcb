// The deskew host rule (tuatara_amd/csrc/geometry.cpp + deskew_rule.h; DESIGN.md "Deskew") under sanitizers: a stand-alone program, host code only.
//   deskew_san <seed> <pages>   drives deskew_consts, deskew_from_page (ink, scores, choice, resampling), deskew_rec_valid and deskew_to_page over seeded
//                               pages - random ink, level lines tilted by a seeded slope, single pixels in the four corners (the first and the last bin
//                               under slopes +-M), blank and all-ink pages, widths about the word size, heights of 1, padded strides, max_slope 1 to 128 -
//                               with the page and every output in exactly sized heap buffers, so that any access outside them, and any signed overflow, is
//                               a sanitizer report.  Prints "pages P turned T".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/geometry.h"
#include "../../tuatara_amd/csrc/deskew_rule.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: deskew_san <seed> <pages>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int pages = std::atoi(argv[2]);
  long turned = 0;
  std::vector<int32_t> cs(2 * kDskSlopes);
  deskew_consts(cs.data());
  if (cs[2 * kDskMaxSlope] != 65536 || cs[2 * kDskMaxSlope + 1] != 0 || cs[0] != 63579 || cs[1] != -15895 || cs[2 * (kDskSlopes - 1)] != 63579 || cs[2 * (kDskSlopes - 1) + 1] != 15895)
    return fail("deskew_consts");
  if (dsk_args_ok(0, 288, 128) || dsk_args_ok(129, 288, 128) || dsk_args_ok(64, 255, 128) || dsk_args_ok(64, 65536, 128) || dsk_args_ok(64, 288, 0) || dsk_args_ok(64, 288, 256) ||
      !dsk_args_ok(1, 256, 1) || !dsk_args_ok(128, 65535, 255))
    return fail("dsk_args_ok");
  const int widths[8] = {1, 2, 63, 64, 65, 129, 193, 300};
  for (int t = 0; t < pages; ++t) {
    const int kind = t % 6;
    int h = 1 + (int)(rng() % 120), w = widths[rng() % 8];
    if (kind == 5) h = 1;
    const int pad = (int)(rng() % 3) * 5, stride = w * 3 + pad;
    const int M = kind == 2 ? kDskMaxSlope : 1 + (int)(rng() % kDskMaxSlope), gain = 256 + (int)(rng() % 200), ink = 1 + (int)(rng() % 255);
    std::vector<uint8_t> page((size_t)h * stride, 255);
    auto dark = [&](int y, int x) { if (y >= 0 && y < h && x >= 0 && x < w) for (int c = 0; c < 3; ++c) page[(size_t)y * stride + 3 * x + c] = 0; };
    if (kind == 0 || kind == 5) for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) if (rng() % 10 < 3) dark(y, x);
    if (kind == 1) {   // lines that drop k px per 512 px
      const int k = (int)(rng() % (2 * M + 1)) - M;
      for (int y0 = 0; y0 < h; y0 += 9) for (int x = 0; x < w; ++x) dark(y0 + dsk_off(x, k), x);
    }
    if (kind == 2) { dark(0, 0); dark(0, w - 1); dark(h - 1, 0); dark(h - 1, w - 1); }
    if (kind == 3) std::fill(page.begin(), page.end(), (uint8_t)0);
    // (kind 4: blank)
    std::vector<uint8_t> out((size_t)h * w * 3);
    std::vector<uint64_t> scores((size_t)2 * M + 1);
    DeskewRec rec;
    deskew_from_page(page.data(), h, w, stride, M, gain, ink, out.data(), w * 3, &rec, scores.data());
    std::string why;
    if (!deskew_rec_valid(rec, M, h, w, cs.data(), &why)) return fail("deskew_from_page: a record decode_pages would refuse: " + why);
    uint64_t total = 0;
    {   // every ink pixel is binned under every slope: each score lies between the ink count and its square
      std::vector<uint64_t> bits(tables_bitmap_words(h, w));
      tables_ink(page.data(), h, w, stride, ink, bits.data());
      for (uint64_t v : bits) total += (uint64_t)__builtin_popcountll(v);
    }
    for (uint64_t s : scores) if (s < total || s > total * total) return fail("deskew_scores: a score outside [ink, ink^2]");
    if (kind == 4 && (rec.slope != 0 || rec.score0 != 0)) return fail("a blank page turned");
    if (rec.slope == 0)
      for (int y = 0; y < h; ++y) for (int x = 0; x < 3 * w; ++x) if (out[(size_t)y * w * 3 + x] != page[(size_t)y * stride + x]) return fail("slope 0 is not the identity");
    DeskewRec bad = rec;
    bad.slope = M + 1; bad.found = M + 1;
    if (deskew_rec_valid(bad, M, h, w, cs.data())) return fail("deskew_rec_valid accepts a slope beyond max_slope");
    bad = rec; bad.C += 1;
    if (deskew_rec_valid(bad, M, h, w, cs.data())) return fail("deskew_rec_valid accepts constants that are not the table's");
    bad = rec; bad.w += 1;
    if (deskew_rec_valid(bad, M, h, w, cs.data())) return fail("deskew_rec_valid accepts another page's size");
    const int n = (int)(rng() % 9);
    std::vector<float> in((size_t)n * 2), back((size_t)n * 2);
    for (float& v : in) v = (float)((double)(rng() % 100000) / 7. - 3000.);
    deskew_to_page(rec, in.data(), n, back.data());
    if (rec.slope == 0) for (int i = 0; i < 2 * n; ++i) if (back[i] != in[i]) return fail("deskew_to_page: slope 0 is not the identity");
    turned += rec.mode;
  }
  std::cout << "pages " << pages << " turned " << turned << std::endl;
  return 0;
}
