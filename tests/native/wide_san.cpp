// The wide-word host rule (tuatara_amd/csrc/geometry.cpp; DESIGN.md "Wide words") under sanitizers: a stand-alone program, host code only.
//   wide_san <seed> <words>   drives wide_plan, wide_profile, wide_cuts_from_profile, wide_piece_coef, wide_piece_quads and wide_cuts_valid over seeded
//                             inputs of the kinds the tests use - random, flat, one dark column and saturated pages; upright and tilted quads, quads partly and
//                             wholly outside the page, degenerate quads, every max_aspect of the setter's domain - with the page and every output in exactly
//                             sized heap buffers, so that any access outside them is a sanitizer report.  Prints "words W pieces P".
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
  if (argc != 3) return fail("usage: wide_san <seed> <words>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int words = std::atoi(argv[2]);
  auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
  long pieces = 0;
  for (int t = 0; t < words; ++t) {
    const int h = 1 + (int)(rng() % 90), w = 1 + (int)(rng() % 1500), pad = (int)(rng() % 3) * 5, stride = w * 3 + pad;
    std::vector<uint8_t> page((size_t)h * stride);
    const int kind = t % 4;
    for (size_t i = 0; i < page.size(); ++i) page[i] = kind == 0 ? (uint8_t)rng() : kind == 1 ? 200 : kind == 2 ? 255 : (uint8_t)((rng() & 1) * 255);
    if (kind == 2) { const int x = (int)(rng() % w); for (int y = 0; y < h; ++y) for (int c = 0; c < 3; ++c) page[(size_t)y * stride + 3 * x + c] = 0; }
    // a quad: a length x height rectangle at some tilt, somewhere on, across or beyond the page; every eighth one degenerate
    const double len = uni(1., 3000.), hgt = t % 8 == 7 ? 0. : uni(0.5, 60.), a = uni(-0.6, 0.6);
    const double x0 = uni(-2000., w + 500.), y0 = uni(-300., h + 300.);
    const double ux = std::cos(a), uy = std::sin(a);
    float quad[8] = {(float)x0, (float)y0, (float)(x0 + len * ux), (float)(y0 + len * uy), (float)(x0 + len * ux - hgt * uy), (float)(y0 + len * uy + hgt * ux),
                     (float)(x0 - hgt * uy), (float)(y0 + hgt * ux)};
    if (t % 16 == 15) for (int k = 2; k < 8; ++k) quad[k] = quad[k & 1];             // all four corners on one point
    if (!region_quad_ok(quad)) return fail("a generated quad left the rule's domain");
    const float aspects[] = {2.f, 3.5f, 8.f, 64.f};
    const float aspect = aspects[rng() % 4];
    if (!wide_aspect_ok(aspect) || wide_aspect_ok(1.f) || wide_aspect_ok(NAN) || !wide_aspect_ok(0.f)) return fail("wide_aspect_ok");
    int64_t frame[6];
    const int n = wide_plan(quad, aspect, frame);
    if (n < 1 || n > kWideMaxPieces) return fail("wide_plan: n out of range");
    std::vector<uint16_t> q((size_t)kWideCols * n);
    wide_profile(page.data(), h, w, stride, frame, n, q.data());
    for (uint16_t v : q) if (v > 1020) return fail("wide_profile: a value above 1020");
    if (t % 5 == 4) for (uint16_t& v : q) v = (uint16_t)(rng() % 3 == 0 ? 65535 : rng());   // profiles no page gives: the DP must stay inside int32 and its tables
    std::vector<int32_t> cuts(17);
    wide_cuts_from_profile(q.data(), n, cuts.data());
    if (!wide_cuts_valid(cuts.data(), n)) return fail("wide_cuts_from_profile: cuts that decode_pages would refuse");
    std::vector<float> quads((size_t)n * 8);
    wide_piece_quads(quad, cuts.data(), n, quads.data());
    for (int j = 0; j < n; ++j) {
      std::vector<int64_t> row(8);
      wide_piece_coef(frame, cuts[j], cuts[j + 1], row.data());
      if (row[0] != 1 || row[7] != 0 || row[3] != frame[2] || row[6] != frame[5]) return fail("wide_piece_coef");
      for (int k = 0; k < 8; ++k) if (!std::isfinite(quads[(size_t)j * 8 + k])) return fail("wide_piece_quads: not finite");
    }
    // what decode_pages must refuse
    std::vector<int32_t> bad(cuts);
    bad[n] += 1;
    if (wide_cuts_valid(bad.data(), n)) return fail("wide_cuts_valid accepts a wrong end");
    pieces += n;
  }
  // the two ends of n, with out-of-range n refused without a write
  std::vector<uint16_t> q((size_t)kWideMaxU, 7);
  std::vector<int32_t> cuts(17, 5);
  wide_cuts_from_profile(q.data(), 0, cuts.data());
  wide_cuts_from_profile(q.data(), 17, cuts.data());
  for (int32_t c : cuts) if (c != -1) return fail("an n out of range must leave -1");
  std::cout << "words " << words << " pieces " << pieces << std::endl;
  return 0;
}
