// depth_filter.h -- the depth conditioning of the ingest (include/dvo_hip.h, dvo_hip_frames_set_depth_filter): what a raw depth plane
// becomes before the frame is built from it.  Raw structured-light and time-of-flight depth has mixed ("flying") pixels at depth
// discontinuities and axial noise that grows with z * z; users of camera/depth/image_raw run a CPU pass against both
// (cv::bilateralFilter, PCL's fast bilateral filter, an edge erosion).  The reference has no such pass
// (SurfacePyramid::convertRawDepthImage only scales and maps 0 to NaN): this is an extension, as the lens and the depth rig are.  Shared
// by the filter pass (depth_filter.hip, k_depth_filter) and the host compiler of the CPU tier (tests/test_depth_filter.py), which is the
// yardstick the device planes are compared with bit for bit: float32 throughout, every product, quotient and sum rounded on its own in
// the order written (clang: the pragma below; a host compiler: -ffp-contract=off), division correctly rounded on both sides, no exp on
// the device -- the two weight tables are computed on the host in double, rounded to float once (depth_filter_prepare) and handed to
// the kernel as bits.
//
// Every output pixel is a pure function of the INPUT window: no decision cascades from pixel to pixel.  z_c = the converted input depth
// (depth_of_u16 / depth_of_f32), VALID iff finite and > 0.  Taps outside the image are no taps.
//   hole     an invalid input gives kDepthFilterHole = 0x7FC00000, the canonical quiet NaN;
//   edge     a valid pixel is rejected (-> that NaN) if any in-image valid tap within Chebyshev distance edge_radius has
//            |z_n - z_c| > tau(z_c), tau(z) = edge_abs + edge_rel * z.  Both sides of a step go, each by its own tau, and so do the
//            mixed pixels between them;
//   erosion  a valid pixel is rejected if any in-image tap within Chebyshev distance hole_radius is invalid.  The image border itself
//            erodes nothing;
//   smooth   a kept pixel: taps row-major over dy, dx in [-radius, radius], in the image and valid (taps that are themselves rejected
//            still count).  d = z_n - z_c, t = |d| * inv with inv = 64 / (gate * sigma(z_c)), sigma(z) = noise_a + noise_b * (z * z);
//            the tap is skipped unless t < 64; bin = int(t), w = ws[dy][dx] * wr[bin]; acc_w += w, acc_d += w * d;
//            out = z_c + acc_d / acc_w.  The centre tap (d = 0) always counts where inv is finite, so acc_w > 0; where it is not
//            (gate * sigma(z_c) underflows to 0) the pixel is a hole.  radius 0: a kept pixel keeps its bits.
//
// THE DEFAULTS (depth_filter_default_params) are recalled from published Kinect axial-noise fits.  They are NOT VERIFIED here, and no
// test depends on their being good.
#pragma once
#include <math.h>
#include <stdint.h>

#include "colour.h"   // depth_of_f32
#include "hd_compat.h"
#include "lens.h"     // depth_of_u16
#include "../../include/dvo_hip.h"

namespace dvo_hip {

constexpr uint32_t kDepthFilterHole = 0x7FC00000u;
constexpr int kDepthFilterMaxRadius = 3;          // of the smoothing window
constexpr int kDepthFilterMaxReject = 2;          // of edge_radius and hole_radius
constexpr int kDepthFilterBins = 64;

// what the kernel receives as an argument and the host yardstick reads: tables plus scalars, 4 * (49 + 64 + 5) + 4 * 4 = 488 bytes
struct DepthFilterPrepared {
  float ws[2 * kDepthFilterMaxRadius + 1][2 * kDepthFilterMaxRadius + 1];   // [dy + 3][dx + 3]; 0 outside the window
  float wr[kDepthFilterBins];
  float noise_a, noise_b, gate, edge_abs, edge_rel;
  int radius, edge_radius, hole_radius, reserved;
};

DVO_HD float depth_filter_hole() {
  const uint32_t b = kDepthFilterHole;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}

// finite and positive (NaN: no)
DVO_HD bool depth_filter_valid(float z) { return z > 0.0f && z < __builtin_inff(); }

DVO_HD float depth_filter_tau(const DepthFilterPrepared& P, float zc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float r = P.edge_rel * zc;
  return P.edge_abs + r;
}

DVO_HD float depth_filter_inv(const DepthFilterPrepared& P, float zc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float zz = zc * zc;
  const float s = P.noise_b * zz;
  const float sigma = P.noise_a + s;
  const float g = P.gate * sigma;
  return 64.0f / g;
}

// a valid in-image tap of depth zn within the edge window of a pixel of depth zc: does it reject the pixel?
DVO_HD bool depth_filter_edge(float zn, float zc, float tau) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = zn - zc;
  return fabsf(d) > tau;
}

// one valid in-image tap of the smoothing window: wsv = ws[dy][dx], wr = the range table (any address space: the kernel keeps it in LDS)
template <typename Table>
DVO_HD void depth_filter_tap(float zn, float zc, float inv, float wsv, Table wr, float* acc_w, float* acc_d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = zn - zc;
  const float t = fabsf(d) * inv;
  if (!(t < 64.0f)) return;
  const int bin = int(t);
  const float w = wsv * wr[bin];
  const float wd = w * d;
  *acc_w = *acc_w + w;
  *acc_d = *acc_d + wd;
}

DVO_HD float depth_filter_result(float zc, float acc_w, float acc_d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(acc_w > 0.0f)) return depth_filter_hole();
  const float q = acc_d / acc_w;
  return zc + q;
}

// ---- host only from here (plain inline functions: a device pass parses them and emits nothing)
// the suggested defaults (NOT verified here: see the head of this file)
inline dvo_hip_depth_filter depth_filter_default_params() {
  dvo_hip_depth_filter f;
  f.radius = 2; f.sigma_space = 1.5f;
  f.noise_a = 0.0012f; f.noise_b = 0.0019f; f.gate = 3.0f;
  f.edge_radius = 1; f.edge_abs = 0.01f; f.edge_rel = 0.03f;
  f.hole_radius = 0;
  f.reserved[0] = f.reserved[1] = 0;
  return f;
}

// null = acceptable, else what is wrong with it (include/dvo_hip.h, "invalid parameters")
inline const char* depth_filter_check(const dvo_hip_depth_filter& f) {
  const float fields[7] = {f.sigma_space, f.noise_a, f.noise_b, f.gate, f.edge_abs, f.edge_rel, 0.0f};
  for (float v : fields)
    if (!(v - v == 0.0f)) return "a field is not finite";
  if (f.radius < 0 || f.radius > kDepthFilterMaxRadius) return "radius must be 0..3";
  if (f.edge_radius < 0 || f.edge_radius > kDepthFilterMaxReject) return "edge_radius must be 0..2";
  if (f.hole_radius < 0 || f.hole_radius > kDepthFilterMaxReject) return "hole_radius must be 0..2";
  if (f.radius > 0 && !(f.sigma_space > 0.0f)) return "sigma_space must be > 0 when radius > 0";
  if (!(f.gate > 0.0f)) return "gate must be > 0";
  if (f.noise_a < 0.0f || f.noise_b < 0.0f || f.edge_abs < 0.0f || f.edge_rel < 0.0f) return "noise_* and edge_* must not be negative";
  if (!(f.noise_a > 0.0f || f.noise_b > 0.0f)) return "sigma(z) must be positive: noise_a and noise_b are both 0";
  if (f.reserved[0] != 0 || f.reserved[1] != 0) return "reserved must be 0";
  return nullptr;
}

// the tables in double, rounded to float once; params must have passed depth_filter_check
inline DepthFilterPrepared depth_filter_prepare(const dvo_hip_depth_filter& f) {
  DepthFilterPrepared P;
  const int R = kDepthFilterMaxRadius;
  for (int dy = -R; dy <= R; ++dy)
    for (int dx = -R; dx <= R; ++dx) {
      const bool in = dy >= -f.radius && dy <= f.radius && dx >= -f.radius && dx <= f.radius && f.radius > 0;
      const double ss = double(f.sigma_space);
      P.ws[dy + R][dx + R] = in ? float(exp(-double(dx * dx + dy * dy) / (2.0 * ss * ss))) : (dx == 0 && dy == 0 ? 1.0f : 0.0f);
    }
  for (int b = 0; b < kDepthFilterBins; ++b) {
    const double u = (double(b) + 0.5) * double(f.gate) / 64.0;
    P.wr[b] = float(exp(-0.5 * (u * u)));
  }
  P.noise_a = f.noise_a; P.noise_b = f.noise_b; P.gate = f.gate; P.edge_abs = f.edge_abs; P.edge_rel = f.edge_rel;
  P.radius = f.radius; P.edge_radius = f.edge_radius; P.hole_radius = f.hole_radius; P.reserved = 0;
  return P;
}

// The rule for one pixel (x, y) of a w x h plane of CONVERTED depths, rows of `pitch` floats: the yardstick.
inline float depth_filter_pixel(const DepthFilterPrepared& P, const float* z, int w, int h, int pitch, int x, int y) {
  const float zc = z[size_t(y) * pitch + x];
  if (!depth_filter_valid(zc)) return depth_filter_hole();
  const float tau = depth_filter_tau(P, zc);
  const int reach = P.edge_radius > P.hole_radius ? P.edge_radius : P.hole_radius;
  for (int dy = -reach; dy <= reach; ++dy)
    for (int dx = -reach; dx <= reach; ++dx) {
      const int xx = x + dx, yy = y + dy;
      if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
      const int cheb = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy);
      const float zn = z[size_t(yy) * pitch + xx];
      if (!depth_filter_valid(zn)) {
        if (cheb <= P.hole_radius) return depth_filter_hole();
      } else if (cheb <= P.edge_radius && depth_filter_edge(zn, zc, tau)) {
        return depth_filter_hole();
      }
    }
  if (P.radius == 0) return zc;
  const float inv = depth_filter_inv(P, zc);
  float acc_w = 0.0f, acc_d = 0.0f;
  for (int dy = -P.radius; dy <= P.radius; ++dy)
    for (int dx = -P.radius; dx <= P.radius; ++dx) {
      const int xx = x + dx, yy = y + dy;
      if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
      const float zn = z[size_t(yy) * pitch + xx];
      if (!depth_filter_valid(zn)) continue;
      depth_filter_tap(zn, zc, inv, P.ws[dy + kDepthFilterMaxRadius][dx + kDepthFilterMaxRadius], P.wr, &acc_w, &acc_d);
    }
  return depth_filter_result(zc, acc_w, acc_d);
}

// a whole plane: out is tight (w floats a row)
inline void depth_filter_plane(const DepthFilterPrepared& P, const float* z, int w, int h, int pitch, float* out) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) out[size_t(y) * w + x] = depth_filter_pixel(P, z, w, h, pitch, x, y);
}
}  // namespace dvo_hip
