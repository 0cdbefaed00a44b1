// The C++ facade's model views (include/dvo/visualization/point_cloud_aggregator.h, PointCloudAggregator::render and renderInto;
// include/dvo_hip.h, dvo_hip_map_render*): usage: map_render_facade_check <n keyframes> <output file>.
//  1. before the first build() there is no map: render() returns null, renderInto() false;
//  2. n keyframes of 64 x 48 (the formulas of tests/cpp/map_facade_check.cpp and tests/test_gpu_cloud_map.py::facade_frame) are built
//     into the map; render() at a pose off the keyframes gives a pyramid whose level-0 planes -- holes and filled pixels both present --
//     go to the output file (I, then Z, float32) for the test to compare with dvo_slam_amd.KeyframeMap.render;
//  3. renderInto() an existing pyramid gives the same level-0 planes bit for bit, and the same level 1 as the pyramid render() made;
//  4. a render with other parameters differs.
// Prints "ok" or the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dvo/core/rgbd_image.h"
#include "dvo/visualization/point_cloud_aggregator.h"

using namespace dvo::core;
using dvo::visualization::PointCloudAggregator;

namespace {

const int W = 64, H = 48;

void keyframe(int k, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z, dvo::compat::Affine3d& T) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      i[y * W + x] = float((x * 7 + y * 13 + k * 5) % 256);
      z[y * W + x] = (x + 2 * y + k) % 29 == 0 ? NAN : float(1000 + (x * 3 + y * 5 + k * 11) % 512) * 0.001f;
    }
  T.setIdentity();
  const double a = double(k) / 1024.0;
  T.matrix()(0, 2) = a;
  T.matrix()(2, 0) = -a;
  T.matrix()(0, 3) = 0.01 * k;
  T.matrix()(1, 3) = -0.005 * k;
  T.matrix()(2, 3) = 0.002 * k;
}

// planes 0 and 1 of a level, as the device holds them
void planes_of(RgbdImagePyramid& p, int level, std::vector<float>& I, std::vector<float>& Z) {
  int w = 0, h = 0;
  dvo_hip_frame_info(p.device_frame(), level, &w, &h, 0);
  I.assign(size_t(w) * h, -1.0f);
  Z.assign(size_t(w) * h, -1.0f);
  dvo_hip_check(p.device_context(), dvo_hip_frame_download_plane(p.device_context(), p.device_frame(), level, 0, I.data()), "download");
  dvo_hip_check(p.device_context(), dvo_hip_frame_download_plane(p.device_context(), p.device_frame(), level, 1, Z.data()), "download");
}

bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::printf("usage: map_render_facade_check <n> <file>\n"); return 2; }
  const int n = std::atoi(argv[1]);
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(2);
  dvo::compat::Affine3d pose;
  pose.setIdentity();
  pose.matrix()(0, 3) = 0.03;
  pose.matrix()(1, 3) = -0.02;
  pose.matrix()(2, 3) = -0.05;

  // 1. no map yet
  PointCloudAggregator aggregator(size_t(1) << 20);
  dvo::compat::ImageMat I0, Z0;
  dvo::compat::Affine3d T0;
  keyframe(0, I0, Z0, T0);
  RgbdImagePyramidPtr target = camera.create(I0, Z0);
  target->build(2);
  if (aggregator.render(camera, pose) || aggregator.renderInto(*target, pose)) { std::printf("a render without a map\n"); return 1; }

  // 2. the map, and a view of it
  for (int k = 0; k < n; ++k) {
    dvo::compat::ImageMat I, Z;
    dvo::compat::Affine3d T;
    keyframe(k, I, Z, T);
    char name[16];
    std::snprintf(name, sizeof name, "kf%04d", k);
    aggregator.add(name, camera.create(I, Z), T);
  }
  if (aggregator.build()->size() < 1000) { std::printf("the map is too small\n"); return 1; }
  RgbdImagePyramidPtr view = aggregator.render(camera, pose);
  if (!view) { std::printf("render() returned null\n"); return 1; }
  view->build(2);
  std::vector<float> I, Z, I1, Z1;
  planes_of(*view, 0, I, Z);
  planes_of(*view, 1, I1, Z1);
  size_t holes = 0, filled = 0;
  for (size_t i = 0; i < Z.size(); ++i) {
    if (std::isnan(Z[i])) { ++holes; if (I[i] != 0.0f) { std::printf("a hole with an intensity\n"); return 1; } }
    else { ++filled; if (!(Z[i] > 0.5f && Z[i] < 2.0f)) { std::printf("pixel %zu: depth %g\n", i, Z[i]); return 1; } }
  }
  if (holes == 0 || filled < Z.size() / 2) { std::printf("%zu holes, %zu filled pixels\n", holes, filled); return 1; }
  const float* hi = dvo::compat::image_ptr(view->level(0).intensity);
  if (std::memcmp(hi, I.data(), I.size() * 4) != 0) { std::printf("level(0).intensity is not the rendered plane\n"); return 1; }

  // 3. the streaming form
  if (!aggregator.renderInto(*target, pose)) { std::printf("renderInto() failed\n"); return 1; }
  std::vector<float> J, Y, J1, Y1;
  planes_of(*target, 0, J, Y);
  planes_of(*target, 1, J1, Y1);
  if (!same(I, J) || !same(Z, Y)) { std::printf("renderInto: level 0 differs from render()\n"); return 1; }
  if (!same(I1, J1) || !same(Z1, Y1)) { std::printf("renderInto: level 1 differs from render()\n"); return 1; }

  // 4. other parameters
  dvo_hip_render_params narrow = dvo_hip_render_params_default();
  narrow.splat = 0.25f;
  narrow.max_splat = 1;
  RgbdImagePyramidPtr sparse = aggregator.render(camera, pose, narrow);
  std::vector<float> Is, Zs;
  if (!sparse) { std::printf("render(narrow) returned null\n"); return 1; }
  planes_of(*sparse, 0, Is, Zs);
  if (same(Z, Zs)) { std::printf("the parameters changed nothing\n"); return 1; }

  std::FILE* f = std::fopen(argv[2], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[2]); return 1; }
  std::fwrite(I.data(), 4, I.size(), f);
  std::fwrite(Z.data(), 4, Z.size(), f);
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
