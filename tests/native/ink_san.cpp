// The local ink host rule (tuatara_amd/csrc/geometry.cpp + ink_rule.h; DESIGN.md "Local ink") under sanitizers: a stand-alone program, host code only.
//   ink_san <seed> <pages>   drives ink_from_page, ink_rec_valid and the ink forms of the tables and deskew rules over seeded pages - random ink over a
//                            gradient, blank and all-black pages, the inverse of a page, widths about the word size, heights of 1, pages smaller than the
//                            window in both axes, padded strides, radius 1 to 64, drop 1 to 255, every polarity - with the page and every output in
//                            exactly sized heap buffers, so that any access outside them, and any signed overflow, is a sanitizer report.  Each bitmap is
//                            held to the rule evaluated pixel by pixel from its definition.  Prints "pages P light L ink I".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/geometry.h"
#include "../../tuatara_amd/csrc/deskew_rule.h"
#include "../../tuatara_amd/csrc/ink_rule.h"
#include "../../tuatara_amd/csrc/tables_rule.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: ink_san <seed> <pages>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int pages = std::atoi(argv[2]);
  long light = 0, inked = 0;
  if (ink_args_ok(0, 38, 0) || ink_args_ok(65, 38, 0) || ink_args_ok(16, 0, 0) || ink_args_ok(16, 256, 0) || ink_args_ok(16, 38, 3) || ink_args_ok(16, 38, -1) ||
      !ink_args_ok(1, 1, 0) || !ink_args_ok(64, 255, 2))
    return fail("ink_args_ok");
  const int widths[8] = {1, 2, 63, 64, 65, 129, 193, 300};
  for (int t = 0; t < pages; ++t) {
    const int kind = t % 6;
    int h = 1 + (int)(rng() % 140), w = widths[rng() % 8];
    if (kind == 5) h = 1;
    const int pad = (int)(rng() % 3) * 5, stride = w * 3 + pad;
    const int R = kind == 2 ? kInkRadiusMax : 1 + (int)(rng() % kInkRadiusMax), drop = 1 + (int)(rng() % 255), pol = (int)(rng() % 3);
    std::vector<uint8_t> page((size_t)h * stride, 255);
    if (kind == 0 || kind == 2 || kind == 5)
      for (int y = 0; y < h; ++y) for (int x = 0; x < 3 * w; ++x) page[(size_t)y * stride + x] = (uint8_t)((40 + 150 * (x / 3) / w + (int)(rng() % 90)) & 255);
    if (kind == 1) for (int y = 0; y < h; y += 7) for (int x = 0; x < 3 * w; ++x) page[(size_t)y * stride + x] = 0;
    if (kind == 3) std::fill(page.begin(), page.end(), (uint8_t)0);
    // (kind 4: blank)
    const int nwx = (w + 63) / 64, nwy = (h + 63) / 64;
    std::vector<uint64_t> bits((size_t)h * nwx), bitsT((size_t)w * nwy);
    InkRec rec;
    ink_from_page(page.data(), h, w, stride, R, drop, pol, bits.data(), bitsT.data(), &rec);
    std::string why;
    if (!ink_rec_valid(rec, R, drop, pol, h, w, &why)) return fail("ink_from_page: a record decode_pages would refuse: " + why);
    auto s_at = [&](int y, int x) { const uint8_t* p = &page[(size_t)y * stride + 3 * x]; return (int)p[0] + p[1] + p[2]; };
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {   // the rule from its definition
        uint64_t S = 0; int n = 0;
        for (int yy = std::max(y - R, 0); yy <= std::min(y + R, h - 1); ++yy)
          for (int xx = std::max(x - R, 0); xx <= std::min(x + R, w - 1); ++xx) { S += (uint64_t)(rec.inverted ? 765 - s_at(yy, xx) : s_at(yy, xx)); ++n; }
        const uint64_t s = (uint64_t)(rec.inverted ? 765 - s_at(y, x) : s_at(y, x));
        const bool want = s * (uint64_t)n * 256u < S * (uint64_t)(256 - drop);
        const bool a = (bits[(size_t)y * nwx + (x >> 6)] >> (x & 63)) & 1, b = (bitsT[(size_t)x * nwy + (y >> 6)] >> (y & 63)) & 1;
        if (a != want || b != want) return fail("ink_from_page: a bit that is not the rule's");
        inked += want;
      }
    for (int y = 0; y < h; ++y) if (w & 63) if (bits[(size_t)y * nwx + nwx - 1] >> (w & 63)) return fail("bits beyond the page's width");
    for (int x = 0; x < w; ++x) if (h & 63) if (bitsT[(size_t)x * nwy + nwy - 1] >> (h & 63)) return fail("bitsT beyond the page's height");
    if (kind == 3 || kind == 4) for (uint64_t v : bits) if (v) return fail("a uniform page carries ink");
    {   // the inverse page under the opposite fixed polarity: the same bits
      std::vector<uint8_t> inv(page.size());
      for (size_t i = 0; i < page.size(); ++i) inv[i] = (uint8_t)(255 - page[i]);
      std::vector<uint64_t> b2((size_t)h * nwx);
      ink_from_page(inv.data(), h, w, stride, R, drop, rec.inverted ? kInkDark : kInkLight, b2.data(), nullptr, nullptr);
      if (b2 != bits) return fail("the inverse page under the other polarity differs");
    }
    InkRec bad = rec;
    bad.inverted ^= 1;
    if (ink_rec_valid(bad, R, drop, pol, h, w)) return fail("ink_rec_valid accepts an inverted flag that does not follow");
    bad = rec; bad.w += 1;
    if (ink_rec_valid(bad, R, drop, pol, h, w)) return fail("ink_rec_valid accepts another page's size");
    bad = rec; bad.radius += 1;
    if (ink_rec_valid(bad, R, drop, pol, h, w)) return fail("ink_rec_valid accepts another radius");
    // the ink forms of the two rules equal their bodies behind this bitmap
    std::vector<int32_t> side(kTabSideInts), side2(kTabSideInts);
    const int m1 = tables_from_page(page.data(), h, w, stride, 16, InkRule::local(R, drop, pol), side.data());
    const int m2 = tables_from_bits(bits.data(), h, w, 16, side2.data());
    if (m1 != m2 || side != side2) return fail("tables_from_page under the local rule is not tables_from_bits behind ink_from_page");
    const int M = 1 + (int)(rng() % 32);
    std::vector<uint8_t> out((size_t)h * w * 3);
    std::vector<uint64_t> scores((size_t)2 * M + 1);
    DeskewRec drec;
    deskew_from_page(page.data(), h, w, stride, M, 288, InkRule::local(R, drop, pol), out.data(), w * 3, &drec, scores.data());
    if (drec.w != w || drec.h != h) return fail("deskew_from_page under the local rule: another page's size");
    light += rec.inverted;
  }
  std::cout << "pages " << pages << " light " << light << " ink " << inked << std::endl;
  return 0;
}
