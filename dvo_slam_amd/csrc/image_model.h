// image_model.h -- the per-pixel arithmetic of the image data model, stated once: what a pyramid level is made of (2 x 2 mean, depth
// subsample), its derivative planes (clamped central differences) and which pixels PointSelection takes.  Shared by every frame-build
// kernel (pyramid_kernels.hip, ingest_strips.hip: tile, LDS and register forms all call these) and the host compiler of the CPU tier
// (tests/test_image_model.py, bit for bit against the oracle).
//   pyr-down      dvo_core/src/core/rgbd_image.cpp:38-55 (2x2 mean), :127-139 (depth subsample)
//   derivatives   dvo_core/src/core/rgbd_image.cpp:419-489
//   selection     dvo_core/include/dvo/core/point_selection.h:63-66
// Every operation is rounded on its own: a caller's product (a depth times its scale) must not fuse into a difference here (clang: the
// pragmas below; a host compiler: -ffp-contract=off).
#pragma once
#include "hd_compat.h"

namespace dvo_hip {

// ValidPointAndGradientThresholdPredicate (point_selection.h:63-66): a finite depth with finite depth derivatives -- a hole next to the
// pixel makes them NaN (Q19) -- and at least one derivative above its threshold
DVO_HD bool selects(float z0, float idx, float idy, float zdx, float zdy, float ithr, float dthr) {
  return z0 == z0 && zdx == zdx && zdy == zdy && (fabsf(idx) > ithr || fabsf(idy) > ithr || fabsf(zdx) > dthr || fabsf(zdy) > dthr);
}

// The derivative of a plane along an axis (rgbd_image.cpp:419-489): half the difference of the two neighbours, whose indices are clamped
// to the plane -- at a border the pixel itself stands in for the neighbour outside.
DVO_HD float central_difference(float prev, float next) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (next - prev) * 0.5f;
}
DVO_HD int clamp_index(int i, int n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

// The next pyramid level's intensity (rgbd_image.cpp:38-55): a, b = the quad's upper row, c, d its lower one, summed in this order
DVO_HD float mean_2x2(float a, float b, float c, float d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (a + b + c + d) / 4.0f;
}
// ... and its depth (rgbd_image.cpp:127-139): the quad's top-left sample as it is, a NaN hole kept (Q18)
DVO_HD float depth_subsample(float top_left) { return top_left; }

// A pixel with its four derivatives.  `at(x, y)` gives the pixel's {I, Z} as a float2: planar planes or an interleaved one, a host array.
struct Derivs {
  float i0, z0, idx, idy, zdx, zdy;
};
template <typename Source>
DVO_HD Derivs derive_at(const Source& at, int w, int h, int x, int y) {
  const float2 c = at(x, y);
  const float2 l = at(clamp_index(x - 1, w), y), r = at(clamp_index(x + 1, w), y);
  const float2 u = at(x, clamp_index(y - 1, h)), d = at(x, clamp_index(y + 1, h));
  return Derivs{c.x, c.y, central_difference(l.x, r.x), central_difference(u.x, d.x), central_difference(l.y, r.y), central_difference(u.y, d.y)};
}

}  // namespace dvo_hip
