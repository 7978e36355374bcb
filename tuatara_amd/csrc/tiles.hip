// Tiled pages (DESIGN.md "Tiled pages"): the heat maps of a page's overlapping tiles stitched into one page map.
//
//   in   tiles [pages][ny nx][Hc / 2][Wc / 2][2] f32: the detector's maps of the tile canvases, a page's tiles in (ty, tx) order; the plan by value
//   out  [pages][H2][W2][2] f32: the page maps
//
// One launch for all pages of a batch: grid (pairs of a row / 256, H2, pages), so that a row's y decision (one tile, or the band between two) is uniform per
// workgroup.  A lane handles two neighbouring pixels = 16 bytes: band edges are multiples of 8 and tile origins multiples of 16 map pixels, so a pair never
// straddles a band or a tile and every access is a 16-byte one.  Outside the bands the value is a copy; inside lerp(a, b, t) = a + t (b - a), x first, then
// y, each operation rounded on its own (nothing contracts into an FMA: lerp3 below) - the host rule's bits (geometry.cpp: stitch_tiles).
// Bandwidth-bound: every output byte is written once, every input byte outside the overlaps read once.
#include "common.h"
#include "kernels.h"

namespace ttr {

// Three roundings, no FMA.  __fsub_rn / __fmul_rn / __fadd_rn do not give that here: the compiler's header defines them as plain -, * and + compiled under its
// default contraction, and a + t * d came out as v_pk_fma_f32 (seen as one-ulp differences from the host rule in the bands).  The operations are therefore
// written out under a contraction pragma of their own, which the operations carry through inlining.
namespace {
__device__ inline float lerp3(float a, float b, float t) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float m = t * d;
  return a + m;
}
__device__ inline float4 lerp3(const float4& a, const float4& b, float t0, float t1) {
  return make_float4(lerp3(a.x, b.x, t0), lerp3(a.y, b.y, t0), lerp3(a.z, b.z, t1), lerp3(a.w, b.w, t1));
}
}  // namespace

__global__ __launch_bounds__(256) void tile_stitch_kernel(const float* __restrict__ tiles, float* __restrict__ out, const TilePlan P) {
  const int sy = P.Hc >> 1, sx = P.Wc >> 1;
  const int y = (int)blockIdx.y, pg = (int)blockIdx.z;
  const int x = 2 * (int)(blockIdx.x * 256 + threadIdx.x);
  if (x >= P.W2) return;
  const TileSeg gy = tile_seg(P.oy, P.ny, sy, y);
  const TileSeg gx = tile_seg(P.ox, P.nx, sx, x), gx1 = tile_seg(P.ox, P.nx, sx, x + 1);   // (same tile or band as x: the weight alone differs)
  const size_t tile_floats = (size_t)sy * sx * 2;
  const float* tp = tiles + (size_t)pg * (P.ny * P.nx) * tile_floats;
  auto at = [&](int ty, int tx) {
    return *reinterpret_cast<const float4*>(tp + (size_t)(ty * P.nx + tx) * tile_floats + ((size_t)(y - (P.oy[ty] >> 1)) * sx + (x - (P.ox[tx] >> 1))) * 2);
  };
  auto row = [&](int ty) { return gx.blend ? lerp3(at(ty, gx.k), at(ty, gx.k + 1), gx.t, gx1.t) : at(ty, gx.k); };
  float4 v = row(gy.k);
  if (gy.blend) v = lerp3(v, row(gy.k + 1), gy.t, gy.t);
  *reinterpret_cast<float4*>(out + ((size_t)pg * P.H2 * P.W2 + (size_t)y * P.W2 + x) * 2) = v;
}

// (the plan must come from tile_plan / tile_plan_from_origins: they check every bound this kernel relies on)
void launch_tile_stitch(const float* tiles, float* out, const TilePlan& plan, int pages, hipStream_t s) {
  if (pages <= 0) return;
  if (plan.ny < 1 || plan.ny > kTileMaxAxis || plan.nx < 1 || plan.nx > kTileMaxAxis || plan.W2 % 2 || plan.Wc % 4 || plan.H2 <= 0 || plan.H2 > 65535 || pages > 65535 ||
      plan.oy[plan.ny - 1] / 2 + plan.Hc / 2 != plan.H2 || plan.ox[plan.nx - 1] / 2 + plan.Wc / 2 != plan.W2)
    throw std::runtime_error("tile_stitch: bad plan");
  hipLaunchKernelGGL(tile_stitch_kernel, dim3((plan.W2 / 2 + 255) / 256, plan.H2, pages), dim3(256), 0, s, tiles, out, plan);
}

}  // namespace ttr
