// The C++ facade's map classes (include/dvo/visualization/point_cloud_aggregator.h, async_point_cloud_builder.h; include/dvo_hip.h,
// dvo_hip_map_*): usage: map_facade_check <n keyframes> <output file>.
//  1. an empty aggregator builds one default point;
//  2. BuildJob::build returns the organised cloud of level 0: at the identity pose the RgbdCamera::buildPointCloud formula bit for
//     bit, NaN where the depth is NaN, the intensities as they are;
//  3. n keyframes of 64 x 48 (integer-valued formulas, the same as tests/test_gpu_cloud_map.py::facade_frame) registered in a
//     shuffled order; build() takes every step-th in name order, and its cloud -- sorted by voxel key -- goes to the output file as
//     float32 quadruples for the test to compare with dvo_slam_amd.KeyframeMap; building twice gives the same cloud; remove() works.
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
using dvo::visualization::AsyncPointCloudBuilder;
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
  const double a = double(k) / 1024.0;            // (applied as given: no trigonometry that two math libraries could round differently)
  T.matrix()(0, 2) = a;
  T.matrix()(2, 0) = -a;
  T.matrix()(0, 3) = 0.01 * k;
  T.matrix()(1, 3) = -0.005 * k;
  T.matrix()(2, 3) = 0.002 * k;
}

bool same_cloud(const PointCloudAggregator::PointCloud& a, const PointCloudAggregator::PointCloud& b) {
  return a.size() == b.size() && std::memcmp(a.x.data(), b.x.data(), a.size() * 4) == 0 && std::memcmp(a.y.data(), b.y.data(), a.size() * 4) == 0 &&
         std::memcmp(a.z.data(), b.z.data(), a.size() * 4) == 0 && std::memcmp(a.intensity.data(), b.intensity.data(), a.size() * 4) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::printf("usage: map_facade_check <n> <file>\n"); return 2; }
  const int n = std::atoi(argv[1]);
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(1);

  // 1. empty
  PointCloudAggregator aggregator(size_t(1) << 20);
  {
    PointCloudAggregator::PointCloud::Ptr one = aggregator.build();
    if (one->size() != 1 || one->x[0] != 0.0f || one->intensity[0] != 0.0f) { std::printf("the empty aggregator did not return one default point\n"); return 1; }
  }

  // 2. the organised cloud
  {
    dvo::compat::ImageMat I, Z;
    dvo::compat::Affine3d T;
    keyframe(1, I, Z, T);
    RgbdImagePyramidPtr pyramid = camera.create(I, Z);
    AsyncPointCloudBuilder::BuildJob job(*pyramid);
    AsyncPointCloudBuilder::PointCloud::Ptr cloud = job.build();
    if (cloud->width != size_t(W) || cloud->height != size_t(H) || cloud->size() != size_t(W * H)) { std::printf("the organised cloud has the wrong shape\n"); return 1; }
    const float* i = dvo::compat::image_ptr(I);
    const float* z = dvo::compat::image_ptr(Z);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int at = y * W + x;
        const volatile float tx = (float(x) - 31.5f) / 60.0f, ty = (float(y) - 23.5f) / 60.0f;
        const volatile float px = tx * z[at], py = ty * z[at];
        const bool hole = std::isnan(z[at]);
        const bool ok = hole ? std::isnan(cloud->x[at]) && std::isnan(cloud->y[at]) && std::isnan(cloud->z[at])
                             : cloud->x[at] == px && cloud->y[at] == py && cloud->z[at] == z[at];
        if (!ok || cloud->intensity[at] != i[at]) { std::printf("organised cloud: pixel (%d, %d) differs\n", x, y); return 1; }
      }
    AsyncPointCloudBuilder::BuildJob moved(*pyramid, T);
    AsyncPointCloudBuilder::PointCloud::Ptr other = moved.build();
    if (same_cloud(*cloud, *other)) { std::printf("the pose changed nothing\n"); return 1; }
  }

  // 3. n keyframes, registered in a shuffled order
  for (int j = 0; j < n; ++j) {
    const int k = int((long(j) * 7919L + 3L) % n);   // (7919 is prime and larger than n: a permutation)
    dvo::compat::ImageMat I, Z;
    dvo::compat::Affine3d T;
    keyframe(k, I, Z, T);
    char name[16];
    std::snprintf(name, sizeof name, "kf%04d", k);
    aggregator.add(name, camera.create(I, Z), T);
  }
  if (aggregator.size() != size_t(n)) { std::printf("%zu keyframes registered, not %d\n", aggregator.size(), n); return 1; }
  PointCloudAggregator::PointCloud::Ptr cloud = aggregator.build();
  PointCloudAggregator::PointCloud::Ptr again = aggregator.build();
  if (cloud->size() < 1000 || !same_cloud(*cloud, *again)) { std::printf("two builds differ (%zu / %zu points)\n", cloud->size(), again->size()); return 1; }
  aggregator.remove("kf0000");
  PointCloudAggregator::PointCloud::Ptr fewer = aggregator.build();
  if (aggregator.size() != size_t(n - 1) || same_cloud(*cloud, *fewer)) { std::printf("remove() changed nothing\n"); return 1; }
  std::FILE* f = std::fopen(argv[2], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[2]); return 1; }
  for (size_t i = 0; i < cloud->size(); ++i) {
    const float rec[4] = {cloud->x[i], cloud->y[i], cloud->z[i], cloud->intensity[i]};
    std::fwrite(rec, sizeof rec, 1, f);
  }
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
