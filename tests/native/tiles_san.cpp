// Tiled pages' host rule (tuatara_amd/csrc/geometry.cpp: tile_plan, tile_plan_from_origins, stitch_tiles; DESIGN.md "Tiled pages") under sanitizers: a
// stand-alone program, host code only.
//   tiles_san <seed> <plans>   plans seeded pages under seeded (canvas_size, overlap) - sizes at and around the tile boundaries, pages of one tile, pages the
//                              rule refuses - then stitches seeded tile maps (NaN, denormals and huge values included) of every accepted plan whose maps stay
//                              small, through both plan forms, with the tiles and the page map in exactly sized heap buffers: any access outside them, and
//                              any signed overflow, is a sanitizer report.  Also walks every map coordinate of each axis and checks that the tile a segment
//                              names holds it.  Prints "plans P stitched S refused R".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/geometry.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

static bool axis_ok(const int* o, int n, int canvas, int map_len) {
  const int s = canvas / 2;
  for (int u = 0; u < map_len; ++u) {
    const TileSeg g = tile_seg(o, n, s, u);
    if (g.k < 0 || g.k >= n || (g.blend && g.k + 1 >= n)) return false;
    if (u - o[g.k] / 2 < 0 || u - o[g.k] / 2 >= s) return false;
    if (g.blend && (u - o[g.k + 1] / 2 < 0 || u - o[g.k + 1] / 2 >= s || !(g.t > 0.f && g.t < 1.f))) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: tiles_san <seed> <plans>");
  std::mt19937 rng((unsigned)std::atoi(argv[1]));
  const int plans = std::atoi(argv[2]);
  long stitched = 0, refused = 0;
  for (int t = 0; t < plans; ++t) {
    const int S = 32 * (2 + (int)(rng() % 31));                              // 64 .. 1024
    int O = 32 * (1 + (int)(rng() % 9));                                     // 32 .. 288: some below 64, some above S / 4
    if (t % 3 == 0 && S >= 256) O = 64 + 32 * (int)(rng() % ((S / 4 - 64) / 32 + 1));   // a permitted one
    const int D = S > O ? S - O : 32;
    auto side = [&]() {
      switch (rng() % 6) {
        case 0: return 1 + (int)(rng() % S);                                 // one tile
        case 1: return S + (int)(rng() % 3) - 1;                             // at the canvas
        case 2: return S + D * (1 + (int)(rng() % 4)) + (int)(rng() % 5) - 2;   // at a tile boundary
        case 3: return 1 + (int)(rng() % 9000);                              // anything, past 8192 at times
        case 4: return 8192 - (int)(rng() % 2);
        default: return 1 + (int)(rng() % (5 * S));
      }
    };
    const int h = side(), w = side();
    const float mag = t % 17 == 5 ? 1.5f : 1.0f;
    TilePlan P;
    try { P = tile_plan(h, w, S, O, mag); }
    catch (const std::runtime_error&) { ++refused; continue; }
    if (!axis_ok(P.oy, P.ny, P.Hc, P.H2) || !axis_ok(P.ox, P.nx, P.Wc, P.W2)) return fail("a segment leaves its tile at plan " + std::to_string(t));
    for (int k = 0; k < P.ny; ++k) if (P.oy[k] + P.ey[k] > h || P.ey[k] <= 0 || P.ey[k] > P.Hc) return fail("a tile leaves the page (y)");
    for (int k = 0; k < P.nx; ++k) if (P.ox[k] + P.ex[k] > w || P.ex[k] <= 0 || P.ex[k] > P.Wc) return fail("a tile leaves the page (x)");
    const TilePlan Q = tile_plan_from_origins(P.ny, P.nx, P.oy, P.ox, P.Hc, P.Wc, P.H2, P.W2);   // the plan's own origins pass the stage form's checks
    if (Q.ny != P.ny || Q.nx != P.nx || Q.H2 != P.H2 || Q.W2 != P.W2) return fail("the two plan forms differ");
    const size_t tile_floats = (size_t)(P.Hc / 2) * (P.Wc / 2) * 2, in_floats = tile_floats * P.tiles(), out_floats = (size_t)P.H2 * P.W2 * 2;
    if (in_floats > ((size_t)1 << 21)) continue;                             // (keeps the run short; the plan itself was checked above)
    const int pages = 1 + (int)(rng() % 2);
    std::vector<float> tiles(in_floats * pages), out(out_floats * pages, -1.f);
    for (float& v : tiles) {
      const unsigned r = rng();
      switch (r % 23) {
        case 0: v = -0.0f; break;
        case 1: v = std::numeric_limits<float>::denorm_min() * (float)(r >> 12); break;
        case 2: v = 3.0e38f + (float)(r >> 8) * 1.0e30f; break;
        case 3: v = t % 5 == 0 ? std::numeric_limits<float>::quiet_NaN() : 1.f; break;
        default: v = (float)(int)(r >> 9) / 4194304.f - 1.f;
      }
    }
    stitch_tiles(tiles.data(), pages, t % 2 ? Q : P, out.data());
    // the corners are copies: no band reaches them
    const int sx = P.Wc / 2;
    if (std::memcmp(&out[0], &tiles[0], 8) != 0) return fail("the first pixel is not tile 0's");
    const size_t last_tile = (size_t)(P.tiles() - 1) * tile_floats, last_px = ((size_t)(P.Hc / 2 - 1) * sx + (sx - 1)) * 2;
    if (std::memcmp(&out[out_floats - 2], &tiles[last_tile + last_px], 8) != 0) return fail("the last pixel is not the last tile's");
    ++stitched;
  }
  // origins the stage form must refuse, each alone
  const int good_y[1] = {0};
  const int cases[5][2] = {{0, 0}, {0, 200}, {0, 256}, {32, 192}, {0, 192}};
  const int w2[5] = {128, 228, 256, 224, 200};
  for (int i = 0; i < 5; ++i) {
    bool threw = false;
    try { (void)tile_plan_from_origins(1, 2, good_y, cases[i], 256, 256, 128, w2[i]); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) return fail("bad origins " + std::to_string(i) + " were accepted");
  }
  std::cout << "plans " << plans << " stitched " << stitched << " refused " << refused << std::endl;
  return 0;
}
