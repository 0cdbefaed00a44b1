// The C++ facade's map with normals (include/dvo/visualization/point_cloud_aggregator.h; include/dvo_hip.h, DVO_HIP_MAP_NORMALS,
// dvo_hip_map_extract_normals, dvo_hip_map_render_normals): usage: map_normals_facade_check <output file>.
//  1. three keyframes of 64 x 48 on a slanted plane with holes (integer-valued formulas, the same as
//     tests/test_gpu_map_normals.py::facade_normals_frame); an aggregator with setNormals(true) builds, and its cloud -- sorted by voxel key
//     -- goes to the output file as {x, y, z, intensity, nx, ny, nz, agreement} records of 32 bytes for the test to compare with
//     dvo_slam_amd.KeyframeMap(normals=True); building twice gives the same cloud; an aggregator never asked for normals gives the same
//     x, y, z, intensity and no normals;
//  2. renderNormals() gives width * height records and a depth plane equal to the depth of render()'s pyramid where that is finite;
//     it refuses on an aggregator without normals;
//  3. sub-maps: a second aggregator with normals merges into the first and leaves it again, exactly; an aggregator without normals is
//     refused; the records with their normal records go out and, into an empty aggregator, come back as the same cloud; records without
//     normal records are refused by a map with normals.
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

void on_error(const char* what, const char* message) {
  std::printf("%s: %s\n", what, message ? message : "?");
  std::exit(1);
}

void keyframe(int k, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z, dvo::compat::Affine3d& T) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int at = y * W + x;
      i[at] = float((x * 7 + y * 13 + k * 5) % 256);
      z[at] = (x + 2 * y + k) % 29 == 0 ? NAN : float(1000 + 4 * x + 2 * y + k) * 0.001f;
    }
  T.setIdentity();
  const double a = double(k) / 1024.0;
  T.matrix()(0, 2) = a;
  T.matrix()(2, 0) = -a;
  T.matrix()(0, 3) = 0.01 * k;
  T.matrix()(1, 3) = -0.005 * k;
  T.matrix()(2, 3) = 0.002 * k;
}

bool same_points(const PointCloudAggregator::PointCloud& a, const PointCloudAggregator::PointCloud& b) {
  return a.size() == b.size() && std::memcmp(a.x.data(), b.x.data(), a.size() * 4) == 0 && std::memcmp(a.y.data(), b.y.data(), a.size() * 4) == 0 &&
         std::memcmp(a.z.data(), b.z.data(), a.size() * 4) == 0 && std::memcmp(a.intensity.data(), b.intensity.data(), a.size() * 4) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: map_normals_facade_check <file>\n"); return 2; }
  DeviceContext::setErrorHandler(on_error);
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(1);

  // 1. three keyframes
  PointCloudAggregator aggregator(size_t(1) << 20), plain(size_t(1) << 20);
  aggregator.setNormals(true);
  if (!aggregator.normals() || plain.normals()) { std::printf("normals() is wrong\n"); return 1; }
  dvo::compat::Affine3d first;
  for (int k = 0; k < 3; ++k) {
    dvo::compat::ImageMat I, Z;
    dvo::compat::Affine3d T;
    keyframe(k, I, Z, T);
    if (k == 0) first = T;
    RgbdImagePyramidPtr p = camera.create(I, Z);
    char name[16];
    std::snprintf(name, sizeof name, "kf%04d", k);
    aggregator.add(name, p, T);
    plain.add(name, p, T);
  }
  PointCloudAggregator::PointCloud::Ptr cloud = aggregator.build();
  PointCloudAggregator::PointCloud::Ptr again = aggregator.build();
  if (cloud->size() < 1000 || !cloud->hasNormals()) { std::printf("the build gave %zu points, %zu normals\n", cloud->size(), cloud->normal_x.size()); return 1; }
  if (!same_points(*cloud, *again) || cloud->normal_x != again->normal_x || cloud->normal_y != again->normal_y || cloud->normal_z != again->normal_z ||
      cloud->agreement != again->agreement) { std::printf("two builds differ\n"); return 1; }
  size_t with = 0;
  for (size_t i = 0; i < cloud->size(); ++i) {
    const float x = cloud->normal_x[i], y = cloud->normal_y[i], z = cloud->normal_z[i], a = cloud->agreement[i];
    if (a == 0.0f) {
      if (x != 0.0f || y != 0.0f || z != 0.0f) { std::printf("voxel %zu: a normal without agreement\n", i); return 1; }
      continue;
    }
    ++with;
    const float len = std::sqrt(x * x + y * y + z * z);
    if (!(std::fabs(len - 1.0f) < 1e-5f) || !(a > 0.0f && a < 1.01f)) { std::printf("voxel %zu: |n| = %g, agreement %g\n", i, len, a); return 1; }
    if (!(z < 0.0f)) { std::printf("voxel %zu: the normal of a surface seen from the front has n.z = %g\n", i, z); return 1; }
  }
  if (with < cloud->size() / 2) { std::printf("only %zu of %zu voxels have a normal\n", with, cloud->size()); return 1; }
  PointCloudAggregator::PointCloud::Ptr bare = plain.build();
  if (!same_points(*cloud, *bare) || bare->hasNormals() || !bare->agreement.empty()) { std::printf("the plain aggregator's cloud differs, or holds normals\n"); return 1; }

  // 2. a view of the normals
  {
    std::vector<float> normals, depth;
    if (!aggregator.renderNormals(camera, first, normals, depth)) { std::printf("renderNormals failed\n"); return 1; }
    if (normals.size() != size_t(W * H * 4) || depth.size() != size_t(W * H)) { std::printf("renderNormals: wrong sizes\n"); return 1; }
    RgbdImagePyramidPtr view = aggregator.render(camera, first);
    if (!view) { std::printf("render failed\n"); return 1; }
    const float* z = dvo::compat::image_ptr(view->level(0).depth);
    size_t seen = 0;
    for (int at = 0; at < W * H; ++at) {
      const bool hole = std::isnan(depth[size_t(at)]);
      if (hole != std::isnan(z[at]) || (!hole && depth[size_t(at)] != z[at])) { std::printf("pixel %d: the depth of the normals view differs\n", at); return 1; }
      const float has = normals[4 * size_t(at) + 3];
      if (has != 0.0f && has != 1.0f) { std::printf("pixel %d: has = %g\n", at, has); return 1; }
      if (hole && has != 0.0f) { std::printf("pixel %d: a hole with a normal\n", at); return 1; }
      seen += has == 1.0f;
    }
    if (seen < size_t(W * H / 4)) { std::printf("the view shows %zu normals\n", seen); return 1; }
    std::vector<float> none_n, none_z;
    if (plain.renderNormals(camera, first, none_n, none_z)) { std::printf("an aggregator without normals rendered some\n"); return 1; }
  }

  // 3. sub-maps
  {
    PointCloudAggregator other(size_t(1) << 20), collector(size_t(1) << 20);
    other.setNormals(true);
    dvo::compat::ImageMat I, Z;
    dvo::compat::Affine3d T;
    keyframe(7, I, Z, T);
    other.add("kf0007", camera.create(I, Z), T);
    other.build();
    if (!aggregator.merge(other)) { std::printf("merge of a map with normals failed\n"); return 1; }
    PointCloudAggregator::PointCloud::Ptr sum = aggregator.cloud();
    if (sum->size() <= cloud->size() || !sum->hasNormals()) { std::printf("the merge added nothing\n"); return 1; }
    if (!aggregator.subtract(other)) { std::printf("subtract failed\n"); return 1; }
    PointCloudAggregator::PointCloud::Ptr after = aggregator.cloud();
    if (!same_points(*after, *cloud) || after->normal_x != cloud->normal_x || after->normal_z != cloud->normal_z || after->agreement != cloud->agreement) {
      std::printf("merge and subtract did not restore the map\n");
      return 1;
    }
    if (aggregator.merge(plain) || plain.merge(other)) { std::printf("maps with and without normals merged\n"); return 1; }
    std::vector<PointCloudAggregator::VoxelRecord> records;
    std::vector<PointCloudAggregator::VoxelColourRecord> colour;
    std::vector<PointCloudAggregator::VoxelNormalRecord> normals;
    float leaf = 0.0f;
    if (!aggregator.exportRecords(records, colour, normals, &leaf) || records.size() != cloud->size() || normals.size() != records.size() || !colour.empty()) {
      std::printf("exportRecords with normals failed\n");
      return 1;
    }
    if (!collector.merge(other) || !collector.subtract(other)) { std::printf("the collector did not take a sub-map\n"); return 1; }   // (an empty map with normals)
    if (collector.absorbRecords(records, colour, leaf)) { std::printf("records without normal records went into a map with normals\n"); return 1; }
    if (!collector.absorbRecords(records, colour, normals, leaf)) { std::printf("absorbRecords with normals failed\n"); return 1; }
    PointCloudAggregator::PointCloud::Ptr copy = collector.cloud();
    if (!same_points(*copy, *cloud) || copy->normal_x != cloud->normal_x || copy->normal_y != cloud->normal_y || copy->normal_z != cloud->normal_z ||
        copy->agreement != cloud->agreement) { std::printf("the records did not come back as the same cloud\n"); return 1; }
  }

  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[1]); return 1; }
  for (size_t i = 0; i < cloud->size(); ++i) {
    const float rec[8] = {cloud->x[i], cloud->y[i], cloud->z[i], cloud->intensity[i], cloud->normal_x[i], cloud->normal_y[i], cloud->normal_z[i], cloud->agreement[i]};
    std::fwrite(rec, sizeof rec, 1, f);
  }
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
