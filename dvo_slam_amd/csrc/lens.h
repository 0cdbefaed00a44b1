// lens.h -- the lens model of the rectifying ingest (include/dvo_hip.h, dvo_hip_frames_set_lens): where a pixel of the rectified (pinhole)
// image lies in the raw camera image, and what the rectified planes hold there.  The forward model of OpenCV / ROS "plumb_bob" and
// "rational_polynomial" (D = k1 k2 p1 p2 k3 k4 k5 k6, zeros switch terms off) -- the map cv::initUndistortRectifyMap tabulates for the
// image_proc stage the reference's nodes sit behind (dvo_ros/src/camera_base.cpp:30-31) -- in closed form, float32 throughout.  Shared by
// the rectify pass (rectify.hip, k_rectify) and the host compiler of the CPU tier (tests/test_lens.py), which is the yardstick the
// device planes are compared with bit for bit: every function that decides a tap or a blend is compiled without contraction (clang:
// the pragma below; a host compiler: -ffp-contract=off), and division is correctly rounded on both sides.
//
// For the rectified pixel (u, v) of a frame with intrinsics K = {fx, fy, ox, oy} and a lens {K_raw = {fxr, fyr, oxr, oyr}, D}:
//   x = (u - ox) / fx,  y = (v - oy) / fy,  r2 = x x + y y
//   radial = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
//   xd = x radial + 2 p1 x y + p2 (r2 + 2 x^2),   yd = y radial + p1 (r2 + 2 y^2) + 2 p2 x y
//   sx = fxr xd + oxr,  sy = fyr yd + oyr
// evaluated as the pinhole part plus the displacement the distortion adds -- the same function, in the order that keeps the small term
// small:
//   sx = (u * (fxr / fx) + (oxr - ox * (fxr / fx))) + fxr * dx,   dx = (x * q + (2 p1) * (x y)) + p2 * (r2 + 2 x^2)
//   sy = (v * (fyr / fy) + (oyr - oy * (fyr / fy))) + fyr * dy,   dy = (y * q + p1 * (r2 + 2 y^2)) + (2 p2) * (x y)
//   q = radial - 1 = r2 * (d1 + r2 * (d2 + r2 * d3)) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6))),   d1 = k1 - k4, d2 = k2 - k5, d3 = k3 - k6
// (Horner, every product and sum rounded on its own, left to right as parenthesised; lens_prepare computes the eight constants once per
// lens, in float32).  A lens with D = 0 and K_raw = K has scale 1, offset 0 and displacement 0: it maps every pixel EXACTLY onto itself.
// No iteration, no table: about 30 float operations per pixel in registers.
//
// A rectified pixel is VALID iff 0 <= sx <= w - 1 and 0 <= sy <= h - 1 (NaN and infinities fail).  Then
//   intensity = the float bilinear blend of the four source taps around (sx, sy): x0 = min(int(sx), w - 2), ax = sx - x0 (likewise y),
//               (1 - ay) * ((1 - ax) * t00 + ax * t10) + ay * ((1 - ax) * t01 + ax * t11); a tap is the source value as a float (an 8-bit
//               colour tap: colour.h's grey first).  Not rounded back to 8 bits: a float intensity taken as is (DVO_HIP_PIXEL_F32).
//               A coordinate exactly on w - 1 (h - 1) has weight 1 on the last column (row): that tap, exactly (finite taps).
//   depth     = the converted depth of the NEAREST source pixel (int(sx + 0.5f), int(sy + 0.5f)) -- never a blend: no phantom surface
//               across a depth edge -- or, with rectify_depth 0, of the pixel (u, v) itself (depth that is rendered or already
//               rectified).
// An invalid pixel holds I = 0 and Z = NaN, whatever rectify_depth says: a pixel without an intensity is no measurement.
#pragma once
#include <stdint.h>

#include "colour.h"
#include "hd_compat.h"

namespace dvo_hip {

// what the map of one lens over one camera needs per pixel (lens_prepare)
struct LensMap {
  float fx, fy, ox, oy;          // K of the rectified frame
  float sxk, cx, syk, cy;        // the pinhole part: sx = u * sxk + cx + ..., sy = v * syk + cy + ...
  float fxr, fyr;                // K_raw's focal lengths scale the displacement
  float d1, d2, d3, k4, k5, k6;  // radial - 1 = r2 (d1 + r2 (d2 + r2 d3)) / (1 + r2 (k4 + r2 (k5 + r2 k6)))
  float p1, p2, p1x2, p2x2;      // tangential terms
};

// K = {fx, fy, ox, oy} of the frame, K_raw likewise of the raw camera, D = k1 k2 p1 p2 k3 k4 k5 k6
DVO_HD LensMap lens_prepare(const float K[4], const float K_raw[4], const float D[8]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  LensMap m;
  m.fx = K[0]; m.fy = K[1]; m.ox = K[2]; m.oy = K[3];
  m.sxk = K_raw[0] / K[0];
  m.syk = K_raw[1] / K[1];
  m.cx = K_raw[2] - K[2] * m.sxk;
  m.cy = K_raw[3] - K[3] * m.syk;
  m.fxr = K_raw[0]; m.fyr = K_raw[1];
  m.d1 = D[0] - D[5]; m.d2 = D[1] - D[6]; m.d3 = D[4] - D[7];
  m.k4 = D[5]; m.k5 = D[6]; m.k6 = D[7];
  m.p1 = D[2]; m.p2 = D[3];
  m.p1x2 = 2.0f * D[2]; m.p2x2 = 2.0f * D[3];
  return m;
}

// (sx, sy): where the rectified pixel (u, v) lies in the raw image
DVO_HD void lens_map(const LensMap& m, int u, int v, float* sx, float* sy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float fu = float(u), fv = float(v);
  const float x = (fu - m.ox) / m.fx, y = (fv - m.oy) / m.fy;
  const float x2 = x * x, y2 = y * y, xy = x * y;
  const float r2 = x2 + y2;
  const float num = r2 * (m.d1 + r2 * (m.d2 + r2 * m.d3));
  const float den = 1.0f + r2 * (m.k4 + r2 * (m.k5 + r2 * m.k6));
  const float q = num / den;
  const float dx = (x * q + m.p1x2 * xy) + m.p2 * (r2 + 2.0f * x2);
  const float dy = (y * q + m.p1 * (r2 + 2.0f * y2)) + m.p2x2 * xy;
  *sx = (fu * m.sxk + m.cx) + m.fxr * dx;
  *sy = (fv * m.syk + m.cy) + m.fyr * dy;
}

// inside the raw image of w x h pixels (NaN: no)
DVO_HD bool lens_valid(float sx, float sy, int w, int h) { return sx >= 0.0f && sx <= float(w - 1) && sy >= 0.0f && sy <= float(h - 1); }

// One rectified pixel.  image(x, y) / depth(x, y): the source taps as floats, already converted (grey of a colour pixel; NaN for a u16 0,
// value * depth_scale; depth_of_f32) -- the caller's loads, everything else is here.  w, h >= 2.
template <typename ImageTap, typename DepthTap>
DVO_HD void lens_rectify_pixel(const LensMap& m, int w, int h, int u, int v, bool rectify_depth, ImageTap image, DepthTap depth, float* I, float* Z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float sx, sy;
  lens_map(m, u, v, &sx, &sy);
  if (!lens_valid(sx, sy, w, h)) {
    *I = 0.0f;
    *Z = __builtin_nanf("");
    return;
  }
  const int x0 = int(sx) < w - 2 ? int(sx) : w - 2, y0 = int(sy) < h - 2 ? int(sy) : h - 2;
  const float ax = sx - float(x0), ay = sy - float(y0);
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const float t00 = image(x0, y0), t10 = image(x0 + 1, y0), t01 = image(x0, y0 + 1), t11 = image(x0 + 1, y0 + 1);
  const float top = bx * t00 + ax * t10, bottom = bx * t01 + ax * t11;
  *I = by * top + ay * bottom;
  *Z = rectify_depth ? depth(int(sx + 0.5f), int(sy + 0.5f)) : depth(u, v);
}

// the u16 depth conversion of the ingest (0 = hole)
DVO_HD float depth_of_u16(uint16_t d, float scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return d == 0 ? __builtin_nanf("") : float(d) * scale;
}

}  // namespace dvo_hip
