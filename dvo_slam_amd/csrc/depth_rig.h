// depth_rig.h -- the depth rig of the registering ingest (include/dvo_hip.h, dvo_hip_frames_set_depth_rig): where a pixel of the DEPTH
// sensor's image lands in the colour camera's image, and at what depth.  A structured-light or stereo RGB-D rig measures depth from a lens
// a few centimetres beside the colour camera, with intrinsics of its own; the reference's nodes subscribe to
// camera/depth_registered/image_rect_raw (dvo_ros/src/camera_base.cpp:30-33), behind a CPU depth_image_proc/register stage.  These are
// that stage's semantics WITHOUT hole filling: a nearest-pixel forward scatter, the nearest surface wins, and target pixels that nothing
// lands on stay holes (NaN).  Shared by the register pass (depth_register.hip, k_depth_fill + k_depth_register) and the host compiler of
// the CPU tier (tests/test_depth_rig.py), which is the yardstick the device planes are compared with bit for bit: float32 throughout,
// compiled without contraction (clang: the pragma below; a host compiler: -ffp-contract=off), division correctly rounded on both sides.
//
// For a frame of w x h pixels with intrinsics K = {fx, fy, ox, oy} and a rig {K_depth = {fxd, fyd, oxd, oyd}, T = [R | t]} (row-major
// 3 x 4, depth-sensor coordinates -> colour-camera coordinates, metres; R is NOT checked for orthonormality -- it is applied as given):
//   1. the z-buffer is the frame's own level-0 plane Z, read as uint32; every element is first set to kDepthRigHole = 0x7FC00000, a quiet
//      NaN.  As an unsigned integer that pattern lies above +infinity and above every positive finite float, and positive floats order
//      as their bits do: no resolve pass is needed, an untouched element is already a hole;
//   2. for every source pixel (u, v): z = the converted depth (u16: 0 -> NaN, else value * depth_scale; float: value * depth_scale);
//      skip the pixel unless z is finite and z > 0;
//   3. X = ((u - oxd) / fxd) * z,  Y = ((v - oyd) / fyd) * z,  P' = R (X, Y, z) + t, each row as ((r0 X + r1 Y) + r2 z) + t;
//      skip unless P'.z is finite and > 0;
//   4. u' = (fx * P'.x) / P'.z + ox,  v' = (fy * P'.y) / P'.z + oy;  skip unless -0.5 <= u' < w - 0.5 and -0.5 <= v' < h - 0.5, compared
//      in float (NaN fails);  xi = int(floorf(u' + 0.5f)), yi likewise, each clamped into the image AFTER the test (u' + 0.5f may round
//      up to w);
//   5. Z[yi * w + xi] = min(Z[yi * w + xi], P'.z) as an unsigned minimum on the float's bits.
// Every product, quotient and sum is rounded on its own, left to right as parenthesised.  The result does not depend on the order in
// which the source pixels are visited, so the device (atomic minima in any order) and the host build of this header agree bit for bit.
// The identity rig (K_depth = K, R = I, t = 0) reproduces a plane of positive finite depths exactly where ((u - ox) / fx * z * fx) / z
// + ox rounds back into pixel u -- true of every camera the tests use -- and turns zeros (u16), NaN, negative values and infinities into
// NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#include "colour.h"   // depth_of_f32
#include "hd_compat.h"
#include "lens.h"     // depth_of_u16
#include "../../include/dvo_hip.h"

namespace dvo_hip {

constexpr uint32_t kDepthRigHole = 0x7FC00000u;   // what k_depth_fill stores: a quiet NaN, above every finite float's bits

// what the projection of one rig over one camera needs per pixel (depth_rig_prepare)
struct DepthRigMap {
  float fxd, fyd, oxd, oyd;      // K_depth
  float r[9], t[3];              // R row-major, t
  float fx, fy, ox, oy;          // K of the frame (the colour camera, rectified)
};

DVO_HD DepthRigMap depth_rig_prepare(const float K[4], const dvo_hip_depth_rig& rig) {
  DepthRigMap m;
  m.fxd = rig.K_depth[0]; m.fyd = rig.K_depth[1]; m.oxd = rig.K_depth[2]; m.oyd = rig.K_depth[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) m.r[i * 3 + j] = rig.T[i * 4 + j];
    m.t[i] = rig.T[i * 4 + 3];
  }
  m.fx = K[0]; m.fy = K[1]; m.ox = K[2]; m.oy = K[3];
  return m;
}

// finite and positive (NaN: no)
DVO_HD bool depth_rig_usable(float z) { return z > 0.0f && z < __builtin_inff(); }

// Steps 2-4 for the source pixel (u, v) of converted depth z: false = skipped; else *at = yi * w + xi and *bits = P'.z as the unsigned
// the z-buffer takes the minimum of.
DVO_HD bool depth_rig_project(const DepthRigMap& m, int w, int h, int u, int v, float z, int* at, uint32_t* bits) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!depth_rig_usable(z)) return false;
  const float X = ((float(u) - m.oxd) / m.fxd) * z, Y = ((float(v) - m.oyd) / m.fyd) * z;
  const float px = ((m.r[0] * X + m.r[1] * Y) + m.r[2] * z) + m.t[0];
  const float py = ((m.r[3] * X + m.r[4] * Y) + m.r[5] * z) + m.t[1];
  const float pz = ((m.r[6] * X + m.r[7] * Y) + m.r[8] * z) + m.t[2];
  if (!depth_rig_usable(pz)) return false;
  const float tu = (m.fx * px) / pz + m.ox, tv = (m.fy * py) / pz + m.oy;
  if (!(tu >= -0.5f && tu < float(w) - 0.5f && tv >= -0.5f && tv < float(h) - 0.5f)) return false;
  int xi = int(floorf(tu + 0.5f)), yi = int(floorf(tv + 0.5f));
  xi = xi < 0 ? 0 : xi > w - 1 ? w - 1 : xi;
  yi = yi < 0 ? 0 : yi > h - 1 ? h - 1 : yi;
  *at = yi * w + xi;
  uint32_t b;
  __builtin_memcpy(&b, &pz, 4);
  *bits = b;
  return true;
}

}  // namespace dvo_hip
