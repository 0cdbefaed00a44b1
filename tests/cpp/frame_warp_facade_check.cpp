// The C++ facade's image warps (include/dvo/core/rgbd_image.h, RgbdImage::warpIntensity, warpIntensityForward, warpDepthForward and
// warpDepthForwardAdvanced; include/dvo_hip.h, dvo_hip_frames_warp_inverse / _forward): usage: frame_warp_facade_check <output file>.
//  1. two pyramids of 64 x 48 (the formulas of tests/test_gpu_frame_warp.py::facade_frame); at level 1 the second image is warped into
//     the first one's raster, and the first one forward under the same transformation with the footprint and without;
//  2. warpDepthForward and warpIntensityForward give the same planes, warpDepthForwardAdvanced has no more holes than they;
//  3. intrinsics that are not the level's own are refused through the error handler;
//  4. the planes go to the output file (inverse I, Z; nearest I, Z; splat I, Z; float32) for the test to compare with
//     dvo_slam_amd.warp_inverse_batch and warp_forward_batch.
// Prints "ok" or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvo/core/rgbd_image.h"

using namespace dvo::core;

namespace {

const int W = 64, H = 48, LEVEL = 1;
int refusals = 0;

void count_refusal(const char*, const char*) { ++refusals; }

void frame(int k, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      i[y * W + x] = float((x * 7 + y * 13 + k * 5) % 256);
      z[y * W + x] = (x / 2 + 2 * (y / 2) + k) % 29 == 0 ? NAN : float(1000 + (x * 3 + y * 5 + k * 11) % 512) * 0.001f;
    }
}

size_t holes(const dvo::compat::ImageMat& m) {
  size_t n = 0;
  const float* p = dvo::compat::image_ptr(m);
  for (int i = 0; i < dvo::compat::image_rows(m) * dvo::compat::image_cols(m); ++i) n += std::isnan(p[i]) ? 1 : 0;
  return n;
}

bool same(const dvo::compat::ImageMat& a, const dvo::compat::ImageMat& b) {
  const size_t n = size_t(dvo::compat::image_rows(a)) * dvo::compat::image_cols(a);
  return dvo::compat::image_rows(a) == dvo::compat::image_rows(b) && dvo::compat::image_cols(a) == dvo::compat::image_cols(b) &&
         std::memcmp(dvo::compat::image_ptr(a), dvo::compat::image_ptr(b), n * 4) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: frame_warp_facade_check <file>\n"); return 2; }
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(3);
  dvo::compat::ImageMat I0, Z0, I1, Z1;
  frame(0, I0, Z0);
  frame(1, I1, Z1);
  RgbdImagePyramidPtr a = camera.create(I0, Z0), b = camera.create(I1, Z1);
  a->build(3);
  b->build(3);
  dvo::compat::Affine3d T;
  T.setIdentity();
  T.matrix()(0, 2) = 1.0 / 64;
  T.matrix()(2, 0) = -1.0 / 64;
  T.matrix()(0, 3) = 0.02;
  T.matrix()(1, 3) = -0.01;
  T.matrix()(2, 3) = -0.15;

  // 1. the warps at level 1
  RgbdImage& ra = a->level(LEVEL);
  RgbdImage& rb = b->level(LEVEL);
  const RgbdCamera& cam = camera.level(LEVEL);
  RgbdImagePtr inverse = cam.create(), nearest = cam.create(), nearest_i = cam.create(), splat = cam.create();
  rb.warpIntensity(T, ra, *inverse);
  ra.warpDepthForward(T, cam.intrinsics(), *nearest);
  ra.warpIntensityForward(T, cam.intrinsics(), *nearest_i);
  ra.warpDepthForwardAdvanced(T, cam.intrinsics(), *splat);
  const dvo::compat::ImageMat* planes[6] = {&inverse->intensity, &inverse->depth, &nearest->intensity, &nearest->depth, &splat->intensity, &splat->depth};
  for (int k = 0; k < 6; ++k)
    if (dvo::compat::image_rows(*planes[k]) != H >> LEVEL || dvo::compat::image_cols(*planes[k]) != W >> LEVEL) {
      std::printf("plane %d has the wrong size\n", k);
      return 1;
    }
  const size_t pixels = size_t(W >> LEVEL) * (H >> LEVEL);
  if (holes(inverse->depth) == pixels || holes(inverse->intensity) < holes(inverse->depth)) { std::printf("the inverse warp's holes\n"); return 1; }

  // 2. the forward modes
  if (!same(nearest->intensity, nearest_i->intensity) || !same(nearest->depth, nearest_i->depth)) { std::printf("the nearest warps differ\n"); return 1; }
  if (holes(nearest->depth) == pixels || holes(splat->depth) > holes(nearest->depth) || same(nearest->depth, splat->depth)) {
    std::printf("%zu holes with the footprint, %zu without\n", holes(splat->depth), holes(nearest->depth));
    return 1;
  }

  // 3. foreign intrinsics
  DeviceContext::setErrorHandler(count_refusal);
  RgbdImagePtr none = cam.create();
  ra.warpDepthForward(T, camera.level(0).intrinsics(), *none);
  DeviceContext::setErrorHandler(0);
  if (refusals != 1 || none->hasDepth()) { std::printf("foreign intrinsics were not refused\n"); return 1; }

  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[1]); return 1; }
  for (int k = 0; k < 6; ++k) std::fwrite(dvo::compat::image_ptr(*planes[k]), 4, pixels, f);
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
