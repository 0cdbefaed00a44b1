// colour.h -- the source conversions of the ingest.  Float depth: depth_of_f32 at the end.  8-bit colour pixels to the 8-bit grey the ingest works on: OpenCV's CV_BGR2GRAY fixed point (ITU-R BT.601 weights with
// 14 fractional bits), the conversion the reference's callers run on the host before RgbdCameraPyramid::create
// (dvo_benchmark/src/benchmark_slam.cpp:55-69, dvo_ros/src/camera_dense_tracking.cpp:222-224).  Shared by the ingest kernels
// (ingest_strips.hip, pyramid_kernels.hip) and the host compiler of the CPU tier (tests/test_colour_ingest.py).
// Every intermediate is below 2^24 (255 * 16384 + 8192): u24 multiply-adds and f32 would both be exact; plain u32 is what is written.
#pragma once
#include <stdint.h>

#include "hd_compat.h"
#include "../../include/dvo_hip.h"

namespace dvo_hip {

constexpr unsigned kGreyWB = 1868u, kGreyWG = 9617u, kGreyWR = 4899u;

// bytes per pixel of a DVO_HIP_PIXEL_* format, 0 for an unknown one
DVO_HD int pixel_channels(int format) {
  return format == DVO_HIP_PIXEL_BGR8 || format == DVO_HIP_PIXEL_RGB8 ? 3 : format == DVO_HIP_PIXEL_BGRA8 || format == DVO_HIP_PIXEL_RGBA8 ? 4 : 0;
}
// true: the first byte of a pixel is red
DVO_HD bool pixel_red_first(int format) { return format == DVO_HIP_PIXEL_RGB8 || format == DVO_HIP_PIXEL_RGBA8; }

// the weight of a pixel's first and third byte: (B, R) in BGR order, (R, B) in RGB order -- one wave-uniform select, no second variant
struct GreyWeights {
  unsigned first, third;
};
DVO_HD GreyWeights grey_weights(bool red_first) { return GreyWeights{red_first ? kGreyWR : kGreyWB, red_first ? kGreyWB : kGreyWR}; }

// grey of the pixel whose bytes are c0, c1, c2 in memory order
DVO_HD unsigned grey_of(unsigned c0, unsigned c1, unsigned c2, GreyWeights w) { return (c0 * w.first + c1 * kGreyWG + c2 * w.third + 8192u) >> 14; }

// grey of the pixel whose bytes sit at bit `shift` of `bits` (bytes shift / 8 .. shift / 8 + 2)
DVO_HD unsigned grey_at_bits(unsigned long long bits, int shift, GreyWeights w) {
  return grey_of(unsigned(bits >> shift) & 0xffu, unsigned(bits >> (shift + 8)) & 0xffu, unsigned(bits >> (shift + 16)) & 0xffu, w);
}

// The value a float depth plane's pixel is stored as (DVO_HIP_DEPTH_F32): metres times the caller's scale, ONE rounding of its own -- never
// contracted into the differences and means that follow it.  Nothing else: NaN (a hole) stays NaN; 0, negative values and infinities
// are taken as they are.  scale 1 is exact.
DVO_HD float depth_of_f32(float z, float scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return z * scale;
}

}  // namespace dvo_hip
