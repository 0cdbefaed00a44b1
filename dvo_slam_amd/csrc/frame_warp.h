// frame_warp.h -- frames warped under a pose (include/dvo_hip.h, dvo_hip_frames_warp_inverse and dvo_hip_frames_warp_forward): the
// reference's RgbdImage::warpIntensity, warpIntensityForward, warpDepthForward and warpDepthForwardAdvanced
// (dvo_core/include/dvo/core/rgbd_image.h:199-213, dvo_core/src/core/rgbd_image.cpp:545-781, dvo_core/src/core/interpolation.cpp:55-110).
// Shared by the kernels (frame_warp.hip: k_warp_inverse, k_warp_forward) and the host compiler of the CPU tier (tests/test_frame_warp.py),
// the yardstick the device planes are compared with bit for bit: float32 throughout, compiled without contraction (clang: the pragma
// below; a host compiler: -ffp-contract=off), division correctly rounded on both sides.  Every product, quotient and sum is rounded on
// its own, in the order written here.
//
// Transform.  The row-major 4 x 4 double of the rest of the API, converted to float ONCE per item (map_pose_prepare, cloud_map.h).  The
// linear part is applied as given, without an orthonormality check; each row is ((r0 X + r1 Y) + r2 z) + t.
// NaN.  Every NaN this header stores is the one pattern 0x7FC00000 (kWarpNaN); a NaN that arithmetic produces (a NaN intensity tap, say)
// is replaced by it before the store, so that "bit for bit" does not depend on payloads.
//
// INVERSE warp (warp_inverse_pixel; RgbdImage::warpIntensity, the scalar one, rgbd_image.cpp:564-597, with
// Interpolation::bilinearWithDepthBuffer, interpolation.cpp:55-110).  A raster frame R (the reference's owner of reference_pointcloud), a
// sampled frame S (the reference's `this`) and T, R's camera -> S's camera (the reference's argument), at one pyramid level at which both
// have the size w x h; K_R back-projects, K_S projects.  Per raster pixel (x, y) with z = Z_R(x, y):
//   1. z not finite: I_w = Z_w = NaN.
//   2. X = ((x - ox_R) / fx_R) * z, Y likewise; p = T (X, Y, z).
//   3. p.z not finite or p.z <= 0: both NaN.  DEVIATION: the reference tests only finiteness and would sample with a point behind the camera.
//   4. u = (p.x * fx_S) / p.z + ox_S, v likewise.  Unless 0 <= u < w and 0 <= v < h, compared in float (NaN fails): both NaN.
//   5. Z_w = p.z.  x0 = floor(u), y0 = floor(v), x1 = x0 + 1, y1 = y0 + 1.
//   6. x1 >= w or y1 >= h: I_w = NaN; Z_w stays p.z, as in the reference.
//   7. else, with wx1 = u - x0, wx0 = 1 - wx1 and the same for y, the four taps in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1): a tap
//      COUNTS when Z_S(tap) is finite and Z_S(tap) > p.z - occlusion_margin; for a counting tap val += (wx * wy) * I_S(tap) and
//      sum += wx * wy.  I_w = val / sum if sum > 0, else NaN.
//   8. the optional difference plane D = I_w - I_R(x, y) (warp_difference): NaN where I_w is NaN.
//
// FORWARD warp (warp_forward_pixel; warpIntensityForward rgbd_image.cpp:654-721, warpDepthForward :604-652 and warpDepthForwardAdvanced
// :723-781, made independent of the visiting order).  A source frame F and T, F's camera -> the target camera (the reference's argument);
// the target has F's own size and K at the level, as the reference's single `intrinsics` implies.  Per source pixel (x, y), z = Z_F(x, y):
//   1. skipped unless z is finite and > 0, and min_depth <= z <= max_depth when the range is on (selection_range_on: 0 and +INFINITY = off).
//   2. X, Y and p as above; skipped unless p.z is finite and > 0.
//   3. u = (p.x * fx) / p.z + ox, v likewise.
//   4. the footprint, by mode:
//      DVO_HIP_WARP_NEAREST: skipped unless 0 <= u < w and 0 <= v < h (float); the one pixel (int(floorf(u)), int(floorf(v))).
//      DVO_HIP_WARP_SPLAT (warpDepthForwardAdvanced, rgbd_image.cpp:734-763): per item, once, in float (warp_splat_prepare)
//          zf1 = R00 + R01 * (fx / fy),  xf1 = -R20 - R21 * (fx / fy),  zf2 = R11 + R10 * (fy / fx),  yf2 = -R21 - R20 * (fy / fx);
//        per pixel xlen = int(ceilf(zf1 + xf1 * (X / z))) + 1, ylen = int(ceilf(zf2 + yf2 * (Y / z))) + 1, each CUT to kWarpMaxFootprint = 8
//        (warp_length: the cut is taken in float before the conversion, so a huge or NaN length is 8 and no conversion overflows);
//        xp = floorf(u), yp = floorf(v); skipped unless u and v are finite.  The footprint is [max(xp, 0), min(xp + xlen, w)) x
//        [max(yp, 0), min(yp + ylen, h)), formed in float (every value is an integer: exact below 2^24, and beyond it the range is empty
//        either way) and converted to int last; an empty range draws nothing.
//   5. every covered pixel takes the unsigned 64-bit minimum of bits(p.z) << 32 | bits(max(I_F(x, y), 0)): the z-buffer element of
//      map_render.h, resolved by map_render_resolve -- a hole is Z = NaN (0x7FC00000), I = 0.
// The nearest surface wins and the intensity plane is that surface's; the minimum is over integers, so the planes do not depend on the
// order the source pixels are visited in.
//
// DEVIATIONS from the reference.
//   * warpDepthForward keeps an order-dependent 5 cm hysteresis (rgbd_image.cpp:639) and stores the UNTRANSFORMED depth (:640);
//     warpIntensityForward lets the last writer win (:692) and returns the source's depth plane.  Neither is followed: both modes store
//     p.z of the nearest surface and its intensity.
//   * rotation() of an Eigen Affine (rgbd_image.cpp:734-738) is a decomposition; here the linear part is used.  For a rigid T they agree.
//   * The Z plane of SPLAT is, for rigid T and footprints within the cap, exactly the reference's: its `!isfinite(*v) || *v > z`
//     (rgbd_image.cpp:771) is a minimum.  The operation order of the length is zf1 + xf1 * (X / z), not the reference's (xf1 * X) / z.
//   * the inverse warp refuses points behind the camera (step 3).
#pragma once
#include <math.h>
#include <stdint.h>

#include "map_render.h"   // render_bits, render_float, map_render_resolve, kRenderEmpty; cloud_map.h: MapPose, map_pose_prepare, map_finite; hd_compat.h: DVO_HD
#include "../../include/dvo_hip.h"

namespace dvo_hip {

constexpr uint32_t kWarpNaN = 0x7FC00000u;
constexpr int kWarpMaxFootprint = 8;

// a sample of the sampled frame: {I, Z} of one pixel
struct WarpTap {
  float I, Z;
};

// what the SPLAT footprint of one item needs per pixel
struct WarpSplat {
  float zf1, xf1, zf2, yf2;
};

// the pixels [u0, u1) x [v0, v1) a source pixel covers (inside the image, at most kWarpMaxFootprint each way), and the element they take
struct WarpFootprint {
  int u0, u1, v0, v1;
  uint64_t value;
};

DVO_HD float warp_nan() { return render_float(kWarpNaN); }
DVO_HD float warp_canonical(float x) { return x != x ? warp_nan() : x; }
// finite and positive (NaN: no)
DVO_HD bool warp_usable(float z) { return z > 0.0f && z < __builtin_inff(); }

// step 2 of both warps: p = T (X, Y, z), the point of pixel (x, y), depth z, of a camera K; X and Y are returned for the SPLAT lengths
DVO_HD void warp_point(const MapPose& T, const float K[4], int x, int y, float z, float p[3], float* X_out, float* Y_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float X = ((float(x) - K[2]) / K[0]) * z, Y = ((float(y) - K[3]) / K[1]) * z;
  p[0] = ((T.r[0] * X + T.r[1] * Y) + T.r[2] * z) + T.t[0];
  p[1] = ((T.r[3] * X + T.r[4] * Y) + T.r[5] * z) + T.t[1];
  p[2] = ((T.r[6] * X + T.r[7] * Y) + T.r[8] * z) + T.t[2];
  *X_out = X;
  *Y_out = Y;
}

// The inverse warp of raster pixel (x, y) of depth z.  taps(xx, yy) returns the WarpTap of pixel (xx, yy) of the sampled frame; it is
// called for the four taps, all inside the image (0 <= x0 < x1 <= w - 1, 0 <= y0 < y1 <= h - 1), and only when step 7 is reached.
template <class Taps>
DVO_HD void warp_inverse_pixel(const MapPose& T, const float KR[4], const float KS[4], int w, int h, int x, int y, float z, float margin,
                               const Taps& taps, float* Iw, float* Zw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *Iw = *Zw = warp_nan();
  if (!map_finite(z)) return;
  float p[3], X, Y;
  warp_point(T, KR, x, y, z, p, &X, &Y);
  if (!warp_usable(p[2])) return;
  const float u = (p[0] * KS[0]) / p[2] + KS[2], v = (p[1] * KS[1]) / p[2] + KS[3];
  if (!(u >= 0.0f && u < float(w) && v >= 0.0f && v < float(h))) return;
  *Zw = p[2];
  const float fx0 = floorf(u), fy0 = floorf(v);
  const int x0 = int(fx0), y0 = int(fy0), x1 = x0 + 1, y1 = y0 + 1;   // (0 <= u < w <= 2^24: the conversions are exact)
  if (x1 >= w || y1 >= h) return;
  const float wx1 = u - fx0, wx0 = 1.0f - wx1, wy1 = v - fy0, wy0 = 1.0f - wy1;
  const float zeps = p[2] - margin;
  const WarpTap t[4] = {taps(x0, y0), taps(x1, y0), taps(x0, y1), taps(x1, y1)};
  const float wgt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
  float val = 0.0f, sum = 0.0f;
  for (int k = 0; k < 4; ++k) {
    if (map_finite(t[k].Z) && t[k].Z > zeps) {
      val += wgt[k] * t[k].I;
      sum += wgt[k];
    }
  }
  if (sum > 0.0f) *Iw = warp_canonical(val / sum);
}

// step 8: D = I_w - I_R, NaN where either is
DVO_HD float warp_difference(float Iw, float IR) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return warp_canonical(Iw - IR);
}

DVO_HD WarpSplat warp_splat_prepare(const MapPose& T, const float K[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  WarpSplat s;
  s.zf1 = T.r[0] + T.r[1] * (K[0] / K[1]);
  s.xf1 = -T.r[6] - T.r[7] * (K[0] / K[1]);
  s.zf2 = T.r[4] + T.r[3] * (K[1] / K[0]);
  s.yf2 = -T.r[7] - T.r[6] * (K[1] / K[0]);
  return s;
}

// int(ceilf(a)) + 1 cut to kWarpMaxFootprint; the cut is taken in float: a NaN or huge a gives the cap, a very negative one 0
DVO_HD int warp_length(float a) {
  const float c = ceilf(a);
  if (!(c < float(kWarpMaxFootprint - 1))) return kWarpMaxFootprint;
  if (c < -1.0f) return 0;
  return int(c) + 1;
}

// one axis of the SPLAT footprint: [max(at, 0), min(at + len, size)) in float, at = floorf(u); false = empty
DVO_HD bool warp_axis(float at, int len, int size, int* lo_out, int* hi_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float end = at + float(len);
  const float lo = at > 0.0f ? at : 0.0f, hi = end < float(size) ? end : float(size);
  if (!(lo < hi)) return false;
  *lo_out = int(lo);
  *hi_out = int(hi);
  return true;
}

// The forward warp of source pixel (x, y), intensity I and depth z; false = the pixel leaves nothing.
DVO_HD bool warp_forward_pixel(const MapPose& T, const WarpSplat& s, const float K[4], int w, int h, int mode, float min_depth, float max_depth,
                               int x, int y, float I, float z, WarpFootprint* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!warp_usable(z)) return false;
  if (selection_range_on(min_depth, max_depth) && !(min_depth <= z && z <= max_depth)) return false;
  float p[3], X, Y;
  warp_point(T, K, x, y, z, p, &X, &Y);
  if (!warp_usable(p[2])) return false;
  const float u = (p[0] * K[0]) / p[2] + K[2], v = (p[1] * K[1]) / p[2] + K[3];
  if (mode == DVO_HIP_WARP_NEAREST) {
    if (!(u >= 0.0f && u < float(w) && v >= 0.0f && v < float(h))) return false;
    out->u0 = int(floorf(u));
    out->v0 = int(floorf(v));
    out->u1 = out->u0 + 1;
    out->v1 = out->v0 + 1;
  } else {
    if (!map_finite(u) || !map_finite(v)) return false;
    const int xlen = warp_length(s.zf1 + s.xf1 * (X / z)), ylen = warp_length(s.zf2 + s.yf2 * (Y / z));
    if (!warp_axis(floorf(u), xlen, w, &out->u0, &out->u1)) return false;
    if (!warp_axis(floorf(v), ylen, h, &out->v0, &out->v1)) return false;
  }
  const float In = I >= 0.0f ? I : 0.0f;
  out->value = uint64_t(render_bits(p[2])) << 32 | uint64_t(render_bits(In));
  return true;
}

}  // namespace dvo_hip
