// The curved-word host rule (tuatara_amd/csrc/geometry.cpp + curve_rule.h; DESIGN.md "Curved words") under sanitizers: a stand-alone program, host code only.
//   curve_san <seed> <words>   drives curve_frame, curve_columns, curve_word, curve_crop, curve_outline and curve_word_valid over seeded inputs of the kinds
//                              the tests use - random, flat, saturated and arc pages; upright and tilted quads, quads partly and wholly outside the page,
//                              degenerate quads and quads at the edge of the rule's domain - with the page and every output in exactly sized heap buffers,
//                              so that any access outside them, and any signed overflow, is a sanitizer report.  Prints "words W curved C".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/geometry.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: curve_san <seed> <words>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int words = std::atoi(argv[2]);
  auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
  long curved = 0;
  for (int t = 0; t < words; ++t) {
    const int h = 1 + (int)(rng() % 200), w = 1 + (int)(rng() % 300), pad = (int)(rng() % 3) * 5, stride = w * 3 + pad;
    std::vector<uint8_t> page((size_t)h * stride);
    const int kind = t % 4;
    for (size_t i = 0; i < page.size(); ++i) page[i] = kind == 0 ? (uint8_t)rng() : kind == 1 ? 200 : kind == 2 ? 235 : (uint8_t)((rng() & 1) * 255);
    if (kind == 2) {   // a dark band along a parabola across the page: a curved word
      const double sag = uni(4., 30.), thick = uni(3., 12.), y0 = h / 2. + uni(-10., 10.);
      for (int x = 0; x < w; ++x) {
        const double u = 2. * x / (double)w - 1., yc = y0 + sag * (u * u - 0.5);
        for (int y = 0; y < h; ++y)
          if (std::fabs(y - yc) <= thick / 2. && (x / 5) % 2 == 0) for (int c = 0; c < 3; ++c) page[(size_t)y * stride + 3 * x + c] = 20;
      }
    }
    // a quad: a length x height rectangle at some tilt, somewhere on, across or beyond the page; every eighth one degenerate, every sixteenth at the domain's edge
    const double len = uni(1., 400.), hgt = t % 8 == 7 ? 0. : uni(0.5, 120.), a = uni(-3.2, 3.2);
    double x0 = uni(-300., w + 100.), y0 = uni(-200., h + 100.);
    if (kind == 2 && t % 8 != 7) { x0 = 0.; y0 = h / 2. - 40.; }
    const double ux = std::cos(a), uy = std::sin(a);
    float quad[8] = {(float)x0, (float)y0, (float)(x0 + len * ux), (float)(y0 + len * uy), (float)(x0 + len * ux - hgt * uy), (float)(y0 + len * uy + hgt * ux),
                     (float)(x0 - hgt * uy), (float)(y0 + hgt * ux)};
    if (kind == 2 && t % 8 != 7) { const float q2[8] = {0.f, (float)y0, (float)w, (float)y0, (float)w, (float)(y0 + 80.), 0.f, (float)(y0 + 80.)}; for (int k = 0; k < 8; ++k) quad[k] = q2[k]; }
    if (t % 16 == 15) for (int k = 2; k < 8; ++k) quad[k] = quad[k & 1];             // all four corners on one point
    if (t % 16 == 11) { quad[0] = -32767.f; quad[1] = -32767.f; quad[2] = 32767.f; quad[3] = -32767.f; quad[4] = 32767.f; quad[5] = 32767.f; quad[6] = -32767.f; quad[7] = 32767.f; }
    if (!region_quad_ok(quad)) return fail("a generated quad left the rule's domain");
    std::vector<int64_t> frame(6), table1(36);
    curve_frame(quad, frame.data());
    std::vector<int32_t> stats((size_t)4 * 128);
    curve_columns(page.data(), h, w, stride, frame.data(), nullptr, stats.data());
    for (int u = 0; u < 128; ++u) {
      if (stats[u] < 0 || stats[u] > 65 * 1020 || stats[128 + u] < 0) return fail("curve_columns: G or M out of range");
      if (stats[256 + u] < -1 || stats[256 + u] > 64 || stats[384 + u] < stats[256 + u] || stats[384 + u] > 64) return fail("curve_columns: first / last out of range");
    }
    std::vector<CurveWord> cw(1);
    curve_word(page.data(), h, w, stride, frame.data(), cw.data(), table1.data());
    if (!curve_word_valid(cw[0])) return fail("curve_word: a word decode_pages would refuse");
    for (int p = 0; p < 2; ++p) for (int j = 0; j < 9; ++j) if (cw[0].spine[p][j] < 0 || cw[0].spine[p][j] > 63 * 256) return fail("curve_word: a spine row out of range");
    curve_columns(page.data(), h, w, stride, frame.data(), table1.data(), stats.data());   // pass 2's columns wherever pass 1's table lies
    std::vector<uint8_t> crop((size_t)32 * 128 * 3);
    curve_crop(page.data(), h, w, stride, &cw[0].table[0][0], crop.data());
    std::vector<float> outline(36);
    curve_outline(quad, cw[0].flag, &cw[0].table[0][0], outline.data());
    for (float v : outline) if (!std::isfinite(v)) return fail("curve_outline: not finite");
    curve_outline(quad, 0, nullptr, outline.data());
    if (outline[0] != quad[0] || outline[1] != quad[1] || outline[34] != quad[6] || outline[35] != quad[7]) return fail("curve_outline: the quad's corners");
    // what decode_pages must refuse
    CurveWord bad = cw[0];
    bad.flag = 2;
    if (curve_word_valid(bad)) return fail("curve_word_valid accepts a flag of 2");
    bad = cw[0]; bad.flag = 1; bad.table[3][0] = INT64_MAX / 2;
    if (curve_word_valid(bad)) return fail("curve_word_valid accepts a knot outside the int32 pixel range");
    curved += cw[0].flag;
  }
  std::cout << "words " << words << " curved " << curved << std::endl;
  return 0;
}
