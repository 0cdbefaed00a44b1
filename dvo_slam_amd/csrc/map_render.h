// map_render.h -- a view of the keyframe map (include/dvo_hip.h, dvo_hip_map_render and dvo_hip_map_render_frames): the voxels of the
// table of cloud_map.h projected into a pinhole camera at a pose, the nearest surface per pixel, as tight intensity and depth planes.
// Not in the reference, which only draws its map in a PCL window; this is what lets the tracker align a frame against the fused model.
// Shared by the kernels (map_render.hip: k_render_fill, k_map_render, k_render_resolve) and the host compiler of the CPU tier
// (tests/test_map_render.py), the yardstick the device planes are compared with bit for bit: float32 throughout (the view's inverse pose
// alone is formed in double), compiled without contraction (clang: the pragma below; a host compiler: -ffp-contract=off), division
// correctly rounded on both sides.  Every product, quotient and sum is rounded on its own, left to right as parenthesised.
//
// View.  width, height, K = {fx, fy, ox, oy} and the pose T = [R | t] (camera -> world; the row-major 4 x 4 double of
// dvo_hip_result::transformation).  map_view_prepare forms the inverse ONCE per view in double and rounds it to float once:
//   r = R^T (r[3 i + j] = float(T[4 j + i])),   t'[i] = float(-((R[0][i] t[0] + R[1][i] t[1]) + R[2][i] t[2]))
// Source.  Every occupied slot of the table with min_points <= n <= 2^20 (kMapVoxelMaxPoints); its record {P.x, P.y, P.z, I} is exactly
// what map_extract_voxel returns, so a render sees what dvo_hip_map_extract reports.
// Projection (map_render_record).
//   p[i] = ((r[3 i] P.x + r[3 i + 1] P.y) + r[3 i + 2] P.z) + t'[i]
//   the voxel is SKIPPED unless p.z is finite and > 0, and min_depth <= p.z <= max_depth when the range is on (selection_range_on)
//   u' = (fx * p.x) / p.z + ox,   v' = (fy * p.y) / p.z + oy;   skipped unless both are finite
// Footprint, per axis (map_render_axis; c = u', f = fx, size = width -- or v', fy, height):
//   half = (((splat * 0.5f) * leaf) * f) / p.z                      (may be +infinity: the cap below bounds the range)
//   lo = ceilf(c - half), hi = floorf(c + half): the pixel centres the voxel's square covers
//   near = floorf(c + 0.5f): the nearest pixel.  If lo > hi (no centre is covered) lo = hi = near.
//   m = (max_splat - 1) / 2;  lo = max(lo, near - m), hi = min(hi, near + m): at most max_splat pixels, centred on the nearest one
//   lo = max(lo, 0), hi = min(hi, size - 1): clipped to the image; the axis is empty if lo > hi now
//   all of it in float (every value is an integer or infinite, so max, min and near -+ m are exact below 2^24), converted to int last.
//   splat is a float in (0, 4], max_splat an odd integer in 1 .. 15: it bounds every loop.
// Z-buffer.  One uint64 per pixel, ~0 at the start.  Every covered pixel takes min(element, uint64(bits(p.z)) << 32 | bits(max(I, 0))).
//   p.z is finite and > 0 and the intensity >= 0 (a NaN becomes 0), so both halves order as unsigned integers like their values, and no
//   value is ~0.  A minimum over integers does not depend on the order of the voxels; equal depths are broken by the LOWER intensity, not
//   by slot, because which key sits in which slot does depend on the order of insertion.
// Resolve.  A pixel whose element is still ~0 is a hole: Z = NaN (kMapHole, 0x7FC00000), I = 0.  Otherwise Z and I are the two halves.
//
// Properties.  This is a FLAT SQUARE splat: the depth is constant across a footprint (the voxel centroid's p.z, no surface normal), and a
// foreground silhouette grows by up to splat * leaf / 2 on each side.  Centroids may lie anywhere in their cells, so the centroids of
// face-adjacent voxels project up to 2 leaf sizes apart: only with splat >= 2 (the default) do their squares always overlap, and a
// fronto-parallel surface whose voxels are all occupied then renders without gaps as long as no footprint is cut by max_splat
// (2 hx + 1 <= max_splat); with a smaller splat, on slanted surfaces and where the map is sparse holes remain, and nothing fills them.
// The grown silhouettes put foreground depth on background pixels: where near objects stand in front of a far background, a model view
// meant for TRACKING wants max_splat = 1 (one pixel per voxel) or a small splat and a depth range instead (profiles/map_render.md).
#pragma once
#include <math.h>
#include <stdint.h>

#include "cloud_map.h"

namespace dvo_hip {

constexpr uint64_t kRenderEmpty = ~0ull;
constexpr int kRenderMaxSplat = 15;

struct MapView {
  float r[9], t[3];                    // world -> camera
  float K[4];
  int w, h;
};

// what the views of one call share
struct RenderArgs {
  float min_depth, max_depth;
  float splat, leaf;
  int max_splat;
  uint32_t min_points;
};

// the pixels a voxel covers, u0 .. u1 x v0 .. v1 (inside the image, at most max_splat each way), and the z-buffer element they take
struct RenderFootprint {
  int u0, u1, v0, v1;
  uint64_t value;
};

DVO_HD uint32_t render_bits(float x) {
  union { float f; uint32_t u; } c;
  c.f = x;
  return c.u;
}
DVO_HD float render_float(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}

DVO_HD MapView map_view_prepare(const double* T16, const float K[4], int w, int h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  MapView v;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) v.r[i * 3 + j] = float(T16[j * 4 + i]);
    v.t[i] = float(-((T16[0 * 4 + i] * T16[3] + T16[1 * 4 + i] * T16[7]) + T16[2 * 4 + i] * T16[11]));
  }
  for (int k = 0; k < 4; ++k) v.K[k] = K[k];
  v.w = w;
  v.h = h;
  return v;
}

// one axis of the footprint; false = no pixel
DVO_HD bool map_render_axis(float c, float f, float z, float splat, float leaf, int max_splat, int size, int* lo_out, int* hi_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float half = (((splat * 0.5f) * leaf) * f) / z;
  float lo = ceilf(c - half), hi = floorf(c + half);
  const float near = floorf(c + 0.5f), m = float((max_splat - 1) / 2);
  if (!(lo <= hi)) lo = hi = near;
  lo = lo > near - m ? lo : near - m;
  hi = hi < near + m ? hi : near + m;
  lo = lo > 0.0f ? lo : 0.0f;
  hi = hi < float(size - 1) ? hi : float(size - 1);
  if (!(lo <= hi)) return false;
  *lo_out = int(lo);
  *hi_out = int(hi);
  return true;
}

// the footprint of the record {P.x, P.y, P.z, I} of a voxel of n points in view v; false = the voxel leaves nothing
DVO_HD bool map_render_record(const MapView& v, const RenderArgs& a, const float rec[4], uint32_t n, RenderFootprint* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (n < a.min_points || n > kMapVoxelMaxPoints) return false;
  const float px = ((v.r[0] * rec[0] + v.r[1] * rec[1]) + v.r[2] * rec[2]) + v.t[0];
  const float py = ((v.r[3] * rec[0] + v.r[4] * rec[1]) + v.r[5] * rec[2]) + v.t[1];
  const float pz = ((v.r[6] * rec[0] + v.r[7] * rec[1]) + v.r[8] * rec[2]) + v.t[2];
  if (!(pz > 0.0f && pz < __builtin_inff())) return false;
  if (selection_range_on(a.min_depth, a.max_depth) && !(a.min_depth <= pz && pz <= a.max_depth)) return false;
  const float uc = (v.K[0] * px) / pz + v.K[2], vc = (v.K[1] * py) / pz + v.K[3];
  if (!map_finite(uc) || !map_finite(vc)) return false;
  if (!map_render_axis(uc, v.K[0], pz, a.splat, a.leaf, a.max_splat, v.w, &out->u0, &out->u1)) return false;
  if (!map_render_axis(vc, v.K[1], pz, a.splat, a.leaf, a.max_splat, v.h, &out->v0, &out->v1)) return false;
  const float I = rec[3] >= 0.0f ? rec[3] : 0.0f;
  out->value = uint64_t(render_bits(pz)) << 32 | uint64_t(render_bits(I));
  return true;
}

// ... of a slot of the table (key != kMapEmptyKey)
DVO_HD bool map_render_voxel(const MapView& v, const RenderArgs& a, uint64_t key, uint32_t n, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t si,
                             RenderFootprint* out) {
  if (n < a.min_points || n > kMapVoxelMaxPoints) return false;   // (n == 0: min_points >= 1)
  float rec[4];
  map_extract_voxel(key, n, sx, sy, sz, si, a.leaf, rec);
  return map_render_record(v, a, rec, n, out);
}

// a z-buffer element as the planes' pixel
DVO_HD void map_render_resolve(uint64_t e, float* I, float* Z) {
  const bool hole = e == kRenderEmpty;
  *Z = render_float(hole ? kMapHole : uint32_t(e >> 32));
  *I = hole ? 0.0f : render_float(uint32_t(e));
}

}  // namespace dvo_hip
