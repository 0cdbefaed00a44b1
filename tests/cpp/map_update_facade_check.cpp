// The C++ facade's incremental PointCloudAggregator (include/dvo/visualization/point_cloud_aggregator.h, setIncremental; include/dvo_hip.h,
// dvo_hip_map_remove / _move / _rehash): usage: map_update_facade_check <output file>.
// Two aggregators are fed the same keyframes (64 x 48, the formulas of tests/cpp/map_facade_check.cpp), one incremental, one not:
//  1. add, add, add, add, build: the first incremental build is the rebuild;
//  2. add one more, build: one insert of one frame, nothing removed;
//  3. remove one, re-pose another, build: one frame removed, one moved, nothing else touched;
//  4. a registered name given another pyramid, build: the old one leaves, the new one enters;
//  5. all but one keyframe removed, build: the vacated slots outnumber the live voxels and the table is rehashed.
// After every build the incremental cloud equals the other one bit for bit.  The cloud of step 3 goes to the output file as float32
// quadruples.  Prints "ok" or the first mismatch.
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

bool same_cloud(const PointCloudAggregator::PointCloud& a, const PointCloudAggregator::PointCloud& b) {
  return a.size() == b.size() && std::memcmp(a.x.data(), b.x.data(), a.size() * 4) == 0 && std::memcmp(a.y.data(), b.y.data(), a.size() * 4) == 0 &&
         std::memcmp(a.z.data(), b.z.data(), a.size() * 4) == 0 && std::memcmp(a.intensity.data(), b.intensity.data(), a.size() * 4) == 0;
}

struct Counters {
  long long inserts, removes, rehashes;
};

Counters counters(dvo_hip_context* ctx) {
  Counters c = {0, 0, 0};
  dvo_hip_get_counter(ctx, "map_inserts", &c.inserts);
  dvo_hip_get_counter(ctx, "map_removes", &c.removes);
  dvo_hip_get_counter(ctx, "map_rehashes", &c.rehashes);
  return c;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: map_update_facade_check <file>\n"); return 2; }
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(1);
  PointCloudAggregator incremental(size_t(1) << 18), plain(size_t(1) << 18);
  incremental.setIncremental(true);
  if (!incremental.incremental() || plain.incremental()) { std::printf("setIncremental did not stick\n"); return 1; }

  std::vector<RgbdImagePyramidPtr> pyramids;
  std::vector<dvo::compat::Affine3d> poses;
  for (int k = 0; k < 7; ++k) {
    dvo::compat::ImageMat I, Z;
    dvo::compat::Affine3d T;
    keyframe(k, I, Z, T);
    pyramids.push_back(camera.create(I, Z));
    poses.push_back(T);
  }
  dvo_hip_context* ctx = pyramids[0]->device_context();
  const char* names[7] = {"kf0", "kf1", "kf2", "kf3", "kf4", "kf5", "kf6"};
  PointCloudAggregator::PointCloud::Ptr got, want, step3;
  Counters before, after;

#define BUILD_AND_COMPARE(step, d_inserts, d_removes, d_rehashes)                                                                      \
  before = counters(ctx);                                                                                                              \
  got = incremental.build();                                                                                                           \
  after = counters(ctx);                                                                                                               \
  want = plain.build();                                                                                                                \
  if (!same_cloud(*got, *want)) { std::printf("step %d: the incremental cloud differs (%zu / %zu points)\n", step, got->size(), want->size()); return 1; } \
  if (after.inserts - before.inserts != (d_inserts) || after.removes - before.removes != (d_removes) || after.rehashes - before.rehashes != (d_rehashes)) { \
    std::printf("step %d: %lld frames inserted, %lld removed, %lld rehashes\n", step, after.inserts - before.inserts, after.removes - before.removes, \
                after.rehashes - before.rehashes);                                                                                     \
    return 1;                                                                                                                          \
  }

  // 1. the first build
  for (int k = 0; k < 4; ++k) {
    incremental.add(names[k], pyramids[k], poses[k]);
    plain.add(names[k], pyramids[k], poses[k]);
  }
  BUILD_AND_COMPARE(1, 4, 0, 0)
  if (got->size() < 1000) { std::printf("step 1: only %zu points\n", got->size()); return 1; }
  // ... and a build without a change: nothing is launched
  BUILD_AND_COMPARE(1, 0, 0, 0)

  // 2. one more
  incremental.add(names[4], pyramids[4], poses[4]);
  plain.add(names[4], pyramids[4], poses[4]);
  BUILD_AND_COMPARE(2, 1, 0, 0)

  // 3. one leaves, one moves
  PointCloudAggregator::PointCloud::Ptr previous = got;
  dvo::compat::Affine3d moved = poses[2];
  moved.matrix()(0, 3) += 0.013;
  moved.matrix()(1, 2) = 3.0 / 1024.0;
  moved.matrix()(2, 1) = -3.0 / 1024.0;
  incremental.remove(names[1]);
  plain.remove(names[1]);
  incremental.add(names[2], pyramids[2], moved);
  plain.add(names[2], pyramids[2], moved);
  BUILD_AND_COMPARE(3, 1, 2, 0)
  if (same_cloud(*got, *previous)) { std::printf("step 3: the update changed nothing\n"); return 1; }
  step3 = got;

  // 4. a name with another pyramid
  incremental.add(names[3], pyramids[5], poses[5]);
  plain.add(names[3], pyramids[5], poses[5]);
  BUILD_AND_COMPARE(4, 1, 1, 0)

  // 5. all but one leave: the table is rehashed
  for (int k = 0; k < 5; ++k)
    if (k != 2) {
      incremental.remove(names[k]);
      plain.remove(names[k]);
    }
  BUILD_AND_COMPARE(5, 0, 3, 1)
  // ... and takes keyframes again
  incremental.add(names[6], pyramids[6], poses[6]);
  plain.add(names[6], pyramids[6], poses[6]);
  BUILD_AND_COMPARE(6, 1, 0, 0)

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
