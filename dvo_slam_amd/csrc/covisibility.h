// covisibility.h -- how much of one keyframe's surface another keyframe also sees (include/dvo_hip.h, dvo_hip_frames_covisibility): the
// count that proposes loop closures.  The reference has no such routine: NearestNeighborConstraintSearch::findPossibleConstraints
// (dvo_slam/src/keyframe_constraint_search.cpp:41-72, called from dvo_slam/src/keyframe_graph.cpp:233 and :456) radius-searches the
// keyframes' translations and hands every hit to the validator, whatever the two cameras look at.  This header states what replaces that
// proposal, once, for the kernel (covisibility.hip: k_covisibility) and for the host compiler of the CPU tier (tests/test_covisibility.py):
// float32 throughout, compiled without contraction (clang: the pragma below; a host compiler: -ffp-contract=off), division correctly
// rounded on both sides, every product, quotient and sum rounded on its own in the order written here.  All outputs are integers, so
// the device records EQUAL the host build's.
//
// One ordered pair (a, b, T) at pyramid level L: T carries a's camera into b's camera, the row-major 4 x 4 double of the rest of the API
// converted to float ONCE per pair (map_pose_prepare, cloud_map.h), its linear part applied as given (warp_point, frame_warp.h).  a has the
// size w_a x h_a and the intrinsics K_a of the level, b its own w_b x h_b and K_b: the two need not agree in size or camera.
// Per pixel (x, y) of a, with z = Z_a(x, y) and I_a = I_a(x, y) (covis_pixel):
//   1. the pixel is SKIPPED unless warp_usable(z) (finite and > 0) and, when the depth range is on (selection_range_on: 0 and +INFINITY =
//      off), min_depth <= z <= max_depth.  Otherwise valid += 1.
//   2. p = warp_point(T, K_a, x, y, z).  Nothing more unless warp_usable(p.z).
//   3. u = (p.x * fx_b) / p.z + ox_b, v likewise; xr = floorf(u + 0.5f), yr = floorf(v + 0.5f).  Integer coordinates are pixel CENTRES,
//      as in the bilinear taps of the inverse warp, so the nearest pixel is the rounded one and the identity lands every pixel on
//      itself whatever the last bit of u.  Nothing more unless 0 <= xr < w_b and 0 <= yr < h_b, compared in float (NaN fails).
//      Otherwise in_view += 1.
//   4. zb = Z_b(int(xr), int(yr)).  zb not finite (map_finite): unknown += 1, nothing more.
//   5. tol = depth_tolerance + depth_tolerance_rel * p.z, d = zb - p.z.
//        d < -tol   occluded += 1: b sees a nearer surface there.
//        d > tol    seen_through += 1: b sees past the point -- a free-space conflict, a pose error or something that moved.
//        otherwise  consistent += 1 and photo += q(fabsf(I_a - I_b(int(xr), int(yr)))),
//      q(e) = uint32(e * 16.0f + 0.5f) when e < 4096, otherwise (NaN included) 65535: sixteenths of a grey level, so that the sum is an
//      integer and does not depend on the order of the pixels.
// INVARIANT, by construction: in_view == unknown + occluded + seen_through + consistent, and in_view <= valid <= w_a * h_a.
//
// The record is 32 bytes: six uint32 {valid, in_view, unknown, occluded, seen_through, consistent} and one uint64 photo
// (dvo_hip_covis_record).  The kernel adds to it in three PAIRS of counts and the sum, four 64-bit integer additions (covis_words):
// a count is at most w_a * h_a < 2^31, so the low half of a word never carries into the high one.
//
// DEVIATIONS.  There is no reference routine to deviate from; what differs from the routines this one stands beside:
//   * the inverse warp (warp_inverse_pixel) tests 0 <= u < w on the unrounded u and samples bilinearly; here the ROUNDED coordinate is
//     tested and the one nearest pixel is read, so a point up to half a pixel outside the left or top edge still lands on the border pixel
//     and one from half a pixel inside the right or bottom edge does not.
//   * the inverse warp's occlusion test is one-sided (a tap nearer than p.z - margin is left out); here both sides are classified and
//     the tolerance may grow with the depth (depth_tolerance_rel), as the noise of a depth camera does.
//   * the reference's proposal (the radius search) is kept beside this one, not replaced: dvo_slam::CovisibilityConstraintSearch
//     (include/dvo_slam/keyframe_covisibility.h) applies it first and the counts to the survivors.
#pragma once
#include <math.h>
#include <stdint.h>

#include "frame_warp.h"   // warp_point, warp_usable, WarpTap; cloud_map.h: MapPose, map_pose_prepare, map_finite; selection.h: selection_range_on
#include "../../include/dvo_hip.h"

namespace dvo_hip {

// what a pixel of a is, in the order of the record's fields; a class from kCovisUnknown on is in view
constexpr int kCovisSkipped = 0, kCovisValid = 1, kCovisUnknown = 2, kCovisOccluded = 3, kCovisSeenThrough = 4, kCovisConsistent = 5;
constexpr uint32_t kCovisPhotoMax = 65535u;

// step 5's q: the absolute intensity difference in sixteenths, rounded half up; 65535 for 4096 and beyond and for NaN
DVO_HD uint32_t covis_photo(float Ia, float Ib) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float e = fabsf(Ia - Ib);
  return e < 4096.0f ? uint32_t(e * 16.0f + 0.5f) : kCovisPhotoMax;   // (e < 4096: the product is below 65536.5, the conversion exact)
}

// The class of pixel (x, y) of a, intensity Ia and depth z.  tap(xx, yy) returns the WarpTap {I, Z} of pixel (xx, yy) of b; it is called
// at most once, only when step 4 is reached, with 0 <= xx < wb and 0 <= yy < hb.  *photo: q of a consistent pixel, else 0.
template <class Tap>
DVO_HD int covis_pixel(const MapPose& T, const float Ka[4], const float Kb[4], int wb, int hb, const dvo_hip_covis_params& par, int x, int y,
                       float Ia, float z, const Tap& tap, uint32_t* photo) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *photo = 0u;
  if (!warp_usable(z)) return kCovisSkipped;
  if (selection_range_on(par.min_depth, par.max_depth) && !(par.min_depth <= z && z <= par.max_depth)) return kCovisSkipped;
  float p[3], X, Y;
  warp_point(T, Ka, x, y, z, p, &X, &Y);
  if (!warp_usable(p[2])) return kCovisValid;
  const float u = (p[0] * Kb[0]) / p[2] + Kb[2], v = (p[1] * Kb[1]) / p[2] + Kb[3];
  const float xr = floorf(u + 0.5f), yr = floorf(v + 0.5f);
  if (!(xr >= 0.0f && xr < float(wb) && yr >= 0.0f && yr < float(hb))) return kCovisValid;
  const WarpTap t = tap(int(xr), int(yr));                     // (0 <= xr < wb <= 2^24: the conversions are exact)
  if (!map_finite(t.Z)) return kCovisUnknown;
  const float tol = par.depth_tolerance + par.depth_tolerance_rel * p[2];
  const float d = t.Z - p[2];
  if (d < -tol) return kCovisOccluded;
  if (d > tol) return kCovisSeenThrough;
  *photo = covis_photo(Ia, t.I);
  return kCovisConsistent;
}

// a record as the four 64-bit words it is added to in: {valid, in_view}, {unknown, occluded}, {seen_through, consistent}, photo -- the
// first field of a pair in the low half (little endian: the layout of dvo_hip_covis_record)
struct CovisWords {
  uint64_t w[4];
};

// the words one pixel of class c adds
DVO_HD CovisWords covis_words(int c, uint32_t photo) {
  CovisWords r;
  r.w[0] = uint64_t(c >= kCovisValid ? 1u : 0u) | uint64_t(c >= kCovisUnknown ? 1u : 0u) << 32;
  r.w[1] = uint64_t(c == kCovisUnknown ? 1u : 0u) | uint64_t(c == kCovisOccluded ? 1u : 0u) << 32;
  r.w[2] = uint64_t(c == kCovisSeenThrough ? 1u : 0u) | uint64_t(c == kCovisConsistent ? 1u : 0u) << 32;
  r.w[3] = photo;
  return r;
}

}  // namespace dvo_hip
