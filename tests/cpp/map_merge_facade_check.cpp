// The C++ facade's sub-maps (include/dvo/visualization/point_cloud_aggregator.h, merge / subtract / moveSubmaps / exportRecords /
// absorbRecords; include/dvo_hip.h, dvo_hip_map_merge / _move_submaps / _export / _merge_records): usage: map_merge_facade_check <output file>.
// Keyframes 0-1 go to aggregator A, 2-3 to B, all four to W (64 x 48, the formulas of tests/cpp/map_facade_check.cpp):
//  1. an empty aggregator that merges A and B holds W's cloud, bit for bit;
//  2. subtracting B leaves A's cloud;
//  3. A and B merged under anchor poses, then B moved to another pose: the cloud of merging B under the new pose at once;
//  4. W's exported records absorbed by a fresh aggregator give W's cloud.
// The cloud of step 3 goes to the output file as float32 quadruples.  Prints "ok" or the first mismatch.
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

dvo::compat::Affine3d anchor(double x, double tilt) {
  dvo::compat::Affine3d T;
  T.setIdentity();
  T.matrix()(0, 3) = x;
  T.matrix()(1, 2) = tilt;
  T.matrix()(2, 1) = -tilt;
  return T;
}

bool same_cloud(const PointCloudAggregator::PointCloud& a, const PointCloudAggregator::PointCloud& b) {
  return a.size() == b.size() && std::memcmp(a.x.data(), b.x.data(), a.size() * 4) == 0 && std::memcmp(a.y.data(), b.y.data(), a.size() * 4) == 0 &&
         std::memcmp(a.z.data(), b.z.data(), a.size() * 4) == 0 && std::memcmp(a.intensity.data(), b.intensity.data(), a.size() * 4) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: map_merge_facade_check <file>\n"); return 2; }
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(1);
  const size_t slots = size_t(1) << 18;
  PointCloudAggregator a(slots), b(slots), whole(slots);
  const char* names[4] = {"kf0", "kf1", "kf2", "kf3"};
  for (int k = 0; k < 4; ++k) {
    dvo::compat::ImageMat I, Z;
    dvo::compat::Affine3d T;
    keyframe(k, I, Z, T);
    RgbdImagePyramidPtr p = camera.create(I, Z);
    (k < 2 ? a : b).add(names[k], p, T);
    whole.add(names[k], p, T);
  }
  PointCloudAggregator::PointCloud::Ptr cloud_a = a.build(), cloud_b = b.build(), cloud_whole = whole.build();
  if (cloud_whole->size() < 1000 || cloud_a->size() >= cloud_whole->size()) { std::printf("the clouds are too small\n"); return 1; }

  // 1. the sum of the sub-maps is the single build
  PointCloudAggregator sum(slots);
  if (!sum.merge(a) || !sum.merge(b)) { std::printf("step 1: merge failed\n"); return 1; }
  if (!same_cloud(*sum.cloud(), *cloud_whole)) { std::printf("step 1: a + b differs from the single build\n"); return 1; }
  if (sum.merge(sum)) { std::printf("step 1: a map merged into itself\n"); return 1; }
  // 2. ... and b leaves exactly
  if (!sum.subtract(b) || !same_cloud(*sum.cloud(), *cloud_a)) { std::printf("step 2: a + b - b differs from a\n"); return 1; }

  // 3. under anchor poses, then b re-posed
  const dvo::compat::Affine3d Ta = anchor(0.25, 2.0 / 1024.0), Tb = anchor(-0.125, -3.0 / 1024.0), Tb2 = anchor(-0.117, -5.0 / 1024.0);
  PointCloudAggregator moved(slots), direct(slots);
  if (!moved.merge(a, Ta) || !moved.merge(b, Tb)) { std::printf("step 3: posed merge failed\n"); return 1; }
  PointCloudAggregator::PointCloud::Ptr before = moved.cloud();
  std::vector<const PointCloudAggregator*> subs(1, &b);
  if (!moved.moveSubmaps(subs, std::vector<dvo::compat::Affine3d>(1, Tb), std::vector<dvo::compat::Affine3d>(1, Tb2))) { std::printf("step 3: moveSubmaps failed\n"); return 1; }
  if (!direct.merge(a, Ta) || !direct.merge(b, Tb2)) { std::printf("step 3: posed merge failed\n"); return 1; }
  PointCloudAggregator::PointCloud::Ptr step3 = moved.cloud();
  if (same_cloud(*step3, *before)) { std::printf("step 3: the move changed nothing\n"); return 1; }
  if (!same_cloud(*step3, *direct.cloud())) { std::printf("step 3: the moved map differs from the one merged under the new pose\n"); return 1; }

  // 4. records out, records in
  std::vector<PointCloudAggregator::VoxelRecord> records;
  std::vector<PointCloudAggregator::VoxelColourRecord> colour;
  float leaf = 0.0f;
  if (!whole.exportRecords(records, colour, &leaf) || records.size() != cloud_whole->size() || !colour.empty() || leaf != 0.01f) {
    std::printf("step 4: exportRecords gave %zu records of leaf %g\n", records.size(), double(leaf));
    return 1;
  }
  PointCloudAggregator restored(slots);
  if (!restored.merge(a) || !restored.subtract(a) || !restored.absorbRecords(records, colour, leaf)) { std::printf("step 4: absorbRecords failed\n"); return 1; }
  if (!same_cloud(*restored.cloud(), *cloud_whole)) { std::printf("step 4: the restored cloud differs\n"); return 1; }

  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[1]); return 1; }
  for (size_t i = 0; i < step3->size(); ++i) {
    const float rec[4] = {step3->x[i], step3->y[i], step3->z[i], step3->intensity[i]};
    std::fwrite(rec, sizeof rec, 1, f);
  }
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
