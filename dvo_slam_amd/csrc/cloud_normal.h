// cloud_normal.h -- surface normals in the keyframe map (include/dvo_hip.h, dvo_hip_frames_normals, dvo_hip_map_create_ex with
// DVO_HIP_MAP_NORMALS, dvo_hip_map_extract_normals and dvo_hip_map_render_normals): which way the surface under a pixel faces, how a
// voxel fuses the normals of its points, and how a view of the map carries them.  Not in the reference, whose map is a PointXYZRGB cloud;
// this is the PointXYZRGBNormal a PCL user would export, computed where the depth planes already are.  Shared by the kernels
// (cloud_normal.hip: k_frame_normals; cloud_map.hip: k_map_insert, k_map_extract, k_map_rehash, k_map_clear; map_render.hip: k_map_render,
// k_render_resolve) and the host compiler of the CPU tier (tests/test_map_normals.py), the yardstick the device results are compared with
// bit for bit: compiled without contraction (clang: the pragma below; a host compiler: -ffp-contract=off).  Every product, quotient and
// sum is rounded on its own, left to right as parenthesised.  Where a square root or a normalising division is needed the arithmetic is
// DOUBLE and uses only + - * / and sqrt, which are correctly rounded on both sides (pose_graph.h is the precedent); there is no float
// square root, no reciprocal square root and no libm call.
//
// Camera-frame normal of pixel (u, v) of a level with intrinsics K = {fx, fy, ox, oy} and that level's depth plane.
//   p(u, v) = (((u - ox) / fx) * z, ((v - oy) / fy) * z, z) in float: the X, Y, z of map_world_point.
//   The pixel HAS A NORMAL iff it is not on the level's border (1 <= u <= w - 2, 1 <= v <= h - 2), it is USABLE in map_world_point's
//   sense (depth range included), its four neighbours (u +- 1, v), (u, v +- 1) have a depth that is finite and > 0 (the depth range is
//   NOT applied to the neighbours), and the two tests below pass.
//   a = p(u + 1, v) - p(u - 1, v),  b = p(u, v + 1) - p(u, v - 1),  c = b x a, each component (b_i * a_j) - (b_j * a_i), in float.  With
//   x right, y down and z forward this is the side of the surface that faces the camera.  Then, in double:
//   dot = (c0 p0 + c1 p1) + c2 p2,  L = sqrt((c0^2 + c1^2) + c2^2),  Lp = sqrt((p0^2 + p1^2) + p2^2)
//   The tests: L is finite and > 0; dot < 0 and -dot >= kNormalMinCos * (L * Lp).  n_i = float(double(c_i) / L).
//   kNormalMinCos = 0.1f widened to double: a surface seen at more than about 84 degrees from its normal gets none, and neither does a
//   stencil that straddles a depth step large enough to look like one (at level 0 with fx ~ 525: a step above roughly 4 % of the depth).
//   This is a DEFINITION, not a tolerance: nobody has measured a best value, it is one constant and has no knob.
// World normal under a pose.  N = R n with the frame's MapPose, each row as (r0 n0 + r1 n1) + r2 n2 in float: no translation, no
//   renormalisation.
// Quantisation and sums.  Per component q = int(floorf(N_c * 511.0f + 0.5f)) + 511, clamped into [0, 1022] (a NaN: 0).  The bias keeps
//   the sums unsigned, so they are added as whole 64-bit words like every other sum of the table.  A map with normals has a side table
//   parallel to the MapSlot table, same index: MapNormalSlot {snx, sny, snz, nn}; nn is the number of the voxel's points that had a
//   normal.  A point without a normal is inserted exactly as without the side table and adds NOTHING to it.  1022 * 2^20 < 2^30: nothing
//   wraps up to kMapVoxelMaxPoints.  {snx, sny} and {snz, nn} are each one 64-bit add (normal_word); a removal adds the two's complement
//   (map_negate, cloud_map.h).  A slot that is vacant or empty holds zeros.
// Extraction of a voxel's normal, in double, rounded to float once.  m_c = double(s_c) - 511.0 * double(nn) (exact);
//   len = sqrt((m0^2 + m1^2) + m2^2).  nn == 0 or len == 0: the record is {0, 0, 0, 0}.  Otherwise
//   {float(m0 / len), float(m1 / len), float(m2 / len), float(len / (511.0 * double(nn)))}: the unit normal and the AGREEMENT of the fused
//   normals -- about 1 on a flat patch, falling where a voxel holds a crease or both sides of a thin wall.
// Merge (cloud_map.h, Merge).  A RECORD of a map with normals has the 16 bytes of MapNormalSlot at the same index of a third array.  A plain
//   merge adds normal_word(snx, sny) and normal_word(snz, nn) as whole words, negated for sign -1.  A posed merge extends map_pose_record:
//   the position part stays as it is, nn is unchanged, and the normal sums become, in double,
//   M_i = (double(r[3 i]) m0 + double(r[3 i + 1]) m1) + double(r[3 i + 2]) m2,  s'_i = clamp(int64(rint(M_i)) + 511 nn, 0, 1022 nn)
//   (normal_pose_sums): the voxel's summed normal is turned, not its points one by one.  Deterministic; a posed subtraction under the
//   same float pose restores the words.
// Render element.  uint64(bits(p.z)) << 32 | payload: the high half is the one of map_render.h, so the depth plane of a normals view
//   equals the grey view's bit for bit.  A voxel whose extracted normal is non-zero: payload = 1 << 30 | qx << 20 | qy << 10 | qz, the q
//   the 10-bit quantisation above of the voxel's extracted WORLD normal; a voxel without one: payload 0.  Equal depths are broken by the
//   LOWER payload -- a value, never a slot index.  Resolve: a hole gives Z = NaN (kMapHole) and the record {0, 0, 0, 0}; a covered pixel
//   with payload 0 gives {0, 0, 0, 0} with its Z; any other the normal in the VIEW'S CAMERA coordinates -- each component dequantised as
//   float(q - 511) / 511.0f, rotated by the MapView's r (rows as above) -- and 1.0f as the fourth component.  The result is not
//   renormalised: its length is within the quantisation (sqrt(3) / (2 * 511) per unit) of 1.
#pragma once
#include <math.h>
#include <stdint.h>

#include "cloud_map.h"
#include "map_render.h"

namespace dvo_hip {

constexpr float kNormalMinCos = 0.1f;                    // a definition, not a measured optimum (above)
constexpr float kNormalScale = 511.0f;
constexpr uint32_t kNormalBias = 511u, kNormalMaxQ = 1022u;
constexpr uint32_t kNormalPayloadHas = 1u << 30;

// one slot of the side table of a map with normals, 16 bytes: {snx, sny} and {snz, nn} are also addressed as 64-bit words
struct alignas(16) MapNormalSlot {
  uint32_t snx, sny, snz, nn;
};

DVO_HD bool normal_interior(int w, int h, int u, int v) { return u >= 1 && u <= w - 2 && v >= 1 && v <= h - 2; }
DVO_HD bool normal_depth_ok(float z) { return z > 0.0f && z < __builtin_inff(); }   // (NaN: no)

// p(u, v): the camera-frame point of a pixel
DVO_HD void normal_point(const float K[4], int u, int v, float z, float p[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  p[0] = ((float(u) - K[2]) / K[0]) * z;
  p[1] = ((float(v) - K[3]) / K[1]) * z;
  p[2] = z;
}

// The camera-frame normal n[0..2] of the interior, usable pixel (u, v) with depth z from the depths left, right, above and below it;
// false (n = 0) where the pixel has none.
DVO_HD bool normal_camera(const float K[4], int u, int v, float z, float z_left, float z_right, float z_up, float z_down, float n[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  n[0] = n[1] = n[2] = 0.0f;
  if (!(normal_depth_ok(z_left) && normal_depth_ok(z_right) && normal_depth_ok(z_up) && normal_depth_ok(z_down))) return false;
  float p[3], pl[3], pr[3], pu[3], pd[3];
  normal_point(K, u, v, z, p);
  normal_point(K, u - 1, v, z_left, pl);
  normal_point(K, u + 1, v, z_right, pr);
  normal_point(K, u, v - 1, z_up, pu);
  normal_point(K, u, v + 1, z_down, pd);
  const float a[3] = {pr[0] - pl[0], pr[1] - pl[1], pr[2] - pl[2]}, b[3] = {pd[0] - pu[0], pd[1] - pu[1], pd[2] - pu[2]};
  const float c[3] = {(b[1] * a[2]) - (b[2] * a[1]), (b[2] * a[0]) - (b[0] * a[2]), (b[0] * a[1]) - (b[1] * a[0])};
  const double c0 = double(c[0]), c1 = double(c[1]), c2 = double(c[2]), p0 = double(p[0]), p1 = double(p[1]), p2 = double(p[2]);
  const double dot = (c0 * p0 + c1 * p1) + c2 * p2;
  const double L = sqrt((c0 * c0 + c1 * c1) + c2 * c2), Lp = sqrt((p0 * p0 + p1 * p1) + p2 * p2);
  if (!(L > 0.0 && L < double(__builtin_inff()))) return false;   // (finite and > 0; a NaN: no)
  if (!(dot < 0.0 && -dot >= double(kNormalMinCos) * (L * Lp))) return false;
  n[0] = float(c0 / L);
  n[1] = float(c1 / L);
  n[2] = float(c2 / L);
  return true;
}

// N = R n: no translation, no renormalisation
DVO_HD void normal_world(const MapPose& p, const float n[3], float N[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  N[0] = (p.r[0] * n[0] + p.r[1] * n[1]) + p.r[2] * n[2];
  N[1] = (p.r[3] * n[0] + p.r[4] * n[1]) + p.r[5] * n[2];
  N[2] = (p.r[6] * n[0] + p.r[7] * n[1]) + p.r[8] * n[2];
}

// one component into [0, 1022]
DVO_HD uint32_t normal_quantise(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float r = floorf(x * kNormalScale + 0.5f);
  if (!(r > -kNormalScale)) return 0u;                   // (also a NaN)
  return r >= kNormalScale ? kNormalMaxQ : uint32_t(int(r) + int(kNormalBias));
}

DVO_HD float normal_dequantise(uint32_t q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return float(int(q) - int(kNormalBias)) / kNormalScale;
}

// {snx, sny} resp. {snz, nn} of a point (or of a run of points) as the 64-bit word the side table adds it in: the first low
DVO_HD uint64_t normal_word(uint32_t lo, uint32_t hi) { return map_word(lo, hi); }

// a voxel's normal record: out[0..2] the unit normal, out[3] the agreement; zeros where the voxel has none
DVO_HD void normal_extract(uint32_t snx, uint32_t sny, uint32_t snz, uint32_t nn, float out[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  out[0] = out[1] = out[2] = out[3] = 0.0f;
  if (nn == 0u) return;
  const double bias = double(kNormalScale) * double(nn);
  const double m0 = double(snx) - bias, m1 = double(sny) - bias, m2 = double(snz) - bias;
  const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
  if (!(len > 0.0)) return;
  out[0] = float(m0 / len);
  out[1] = float(m1 / len);
  out[2] = float(m2 / len);
  out[3] = float(len / bias);
}

// The normal sums {snx, sny, snz} of a record of nn > 0 points under the pose p of a posed merge (cloud_map.h, map_pose_record, which
// moves the position part): out[0..2], nn itself is unchanged.  Deterministic; a posed subtraction under the same float pose computes the
// same addends, so it restores the words.
DVO_HD void normal_pose_sums(const MapPose& p, uint32_t snx, uint32_t sny, uint32_t snz, uint32_t nn, uint32_t out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double bias = double(kNormalScale) * double(nn);
  const double m0 = double(snx) - bias, m1 = double(sny) - bias, m2 = double(snz) - bias;
  const int64_t centre = int64_t(kNormalBias) * int64_t(nn), top = int64_t(kNormalMaxQ) * int64_t(nn);
  for (int i = 0; i < 3; ++i) {
    const double M = (double(p.r[3 * i]) * m0 + double(p.r[3 * i + 1]) * m1) + double(p.r[3 * i + 2]) * m2;
    // (|M| <= 3 * 2^128 * 2^31 for a finite pose: far inside a double; beyond +-2^62 -- or a NaN -- the sum is clamped all the same)
    int64_t s = M >= 4611686018427387904.0 ? top : !(M > -4611686018427387904.0) ? 0 : int64_t(__builtin_rint(M)) + centre;
    s = s < 0 ? 0 : s > top ? top : s;
    out[i] = uint32_t(s);
  }
}

// the low half of a normals view's z-buffer element from a voxel's normal record
DVO_HD uint32_t normal_payload(const float rec[4]) {
  if (rec[0] == 0.0f && rec[1] == 0.0f && rec[2] == 0.0f) return 0u;
  return kNormalPayloadHas | normal_quantise(rec[0]) << 20 | normal_quantise(rec[1]) << 10 | normal_quantise(rec[2]);
}

// the z-buffer element of a normals view from the grey view's (map_render.h: the same depth half) and the voxel's side-table sums
DVO_HD uint64_t normal_render_value(uint64_t grey_value, uint32_t snx, uint32_t sny, uint32_t snz, uint32_t nn) {
  float rec[4];
  normal_extract(snx, sny, snz, nn, rec);
  return (grey_value & 0xffffffff00000000ull) | uint64_t(normal_payload(rec));
}

// a z-buffer element as the normals view's pixel: out[0..3] and the bits of Z
DVO_HD void normal_render_resolve(uint64_t e, const MapView& v, float out[4], uint32_t* z_bits) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool hole = e == kRenderEmpty;
  *z_bits = hole ? kMapHole : uint32_t(e >> 32);
  const uint32_t payload = uint32_t(e);
  out[0] = out[1] = out[2] = out[3] = 0.0f;
  if (hole || payload == 0u) return;
  const float N[3] = {normal_dequantise((payload >> 20) & 0x3ffu), normal_dequantise((payload >> 10) & 0x3ffu), normal_dequantise(payload & 0x3ffu)};
  out[0] = (v.r[0] * N[0] + v.r[1] * N[1]) + v.r[2] * N[2];
  out[1] = (v.r[3] * N[0] + v.r[4] * N[1]) + v.r[5] * N[2];
  out[2] = (v.r[6] * N[0] + v.r[7] * N[1]) + v.r[8] * N[2];
  out[3] = 1.0f;
}

}  // namespace dvo_hip
