// Tiled pages (ttr_engine_set_tiled; DESIGN.md "Tiled pages"): the plan of one page canvas, plain data shared by the host rule (geometry.cpp) and the stitch
// kernel (tiles.hip), which takes it by value.
#pragma once

namespace ttr {

constexpr int kTileMaxAxis = 16;     // tiles per axis, at most
constexpr int kTileMaxPage = 64;     // tiles per page, at most
constexpr int kTileMaxSide = 8192;   // longest page side, in pixels
constexpr int kTileBand = 16;        // width of a feather band, in heat-map pixels

// Tile (ty, tx) of a page is the window [oy[ty], oy[ty] + ey[ty]) x [ox[tx], ox[tx] + ex[tx]) of the page, on a canvas of Hc x Wc (zeros behind the window);
// the tiles of a page travel in (ty, tx) order.  The page canvas is hp x wp = c32(h) x c32(w), its heat map H2 x W2 = hp / 2 x wp / 2.  The origins and the
// canvas depend on the page through (hp, wp) alone; the extents on (h, w).
struct TilePlan {
  int ny, nx;
  int oy[kTileMaxAxis], ox[kTileMaxAxis];   // origins, image pixels (multiples of 32)
  int ey[kTileMaxAxis], ex[kTileMaxAxis];   // extents: min(canvas, side - origin)
  int Hc, Wc;                               // the tiles' shared canvas
  int hp, wp, H2, W2;                       // the page canvas and its heat map
  int tiles() const { return ny * nx; }
};

#ifdef __HIPCC__
#define TTR_TILE_HD __host__ __device__
#else
#define TTR_TILE_HD
#endif

// One axis of the stitch at heat-map coordinate u: `o` the tiles' origins in image pixels, s the tile map's length.  Seam k sits at
// c = (o[k + 1] / 2 + o[k] / 2 + s) / 2; outside the bands [c - 8, c + 8) the coordinate belongs to tile k alone (blend 0); inside, tile k + 1 has the
// weight t = (2 j + 1) / 32 with j = u - (c - 8) - exact in fp32.
struct TileSeg { int k, blend; float t; };
TTR_TILE_HD inline TileSeg tile_seg(const int* o, int n, int s, int u) {
  for (int k = 0; k + 1 < n; ++k) {
    const int c = (o[k + 1] / 2 + o[k] / 2 + s) / 2;
    if (u < c - kTileBand / 2) return TileSeg{k, 0, 0.f};
    if (u < c + kTileBand / 2) return TileSeg{k, 1, (float)(2 * (u - (c - kTileBand / 2)) + 1) * (1.f / 32.f)};
  }
  return TileSeg{n - 1, 0, 0.f};
}

}  // namespace ttr
