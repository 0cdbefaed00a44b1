// The C++ facade's coloured map (include/dvo/visualization/point_cloud_aggregator.h, async_point_cloud_builder.h,
// include/dvo/core/rgbd_image.h; include/dvo_hip.h, dvo_hip_frames_set_colour, dvo_hip_map_create_ex, dvo_hip_map_extract_colour):
// usage: map_colour_facade_check <output file>.
//  1. three keyframes of 64 x 48 (integer-valued formulas, the same as tests/test_gpu_map_colour.py::facade_colour) whose level(0).rgb
//     holds float B, G, R with fractions, values below 0 and above 255; an aggregator with setColour(true) attaches them (truncated,
//     saturated), and its cloud -- sorted by voxel key -- goes to the output file as {x, y, z, intensity, rgba} records of 20 bytes for
//     the test to compare with dvo_slam_amd.KeyframeMap(colour=True); building twice gives the same cloud;
//  2. BuildJob::build of a pyramid that carries colour fills rgba with the pixels, A = 0xFF; of one without, rgba stays empty;
//  3. a keyframe without rgb: the aggregator says so through the error handler and builds the grey map (rgba empty), equal in x, y, z
//     and intensity to the cloud of an aggregator that was never asked for colour.
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
int g_warnings = 0;

void on_error(const char* what, const char* message) {
  if (std::strcmp(what, "PointCloudAggregator::build") == 0) {
    ++g_warnings;
    return;
  }
  std::printf("%s: %s\n", what, message ? message : "?");
  std::exit(1);
}

void keyframe(int k, dvo::compat::ImageMat& I, dvo::compat::ImageMat& Z, dvo::compat::ImageMat& rgb, dvo::compat::Affine3d& T) {
  I = dvo::compat::image_create(H, W);
  Z = dvo::compat::image_create(H, W);
  rgb = dvo::compat::image_create3(H, W);
  float* i = dvo::compat::image_ptr_mut(I);
  float* z = dvo::compat::image_ptr_mut(Z);
  float* c = dvo::compat::image_ptr_mut(rgb);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int at = y * W + x;
      i[at] = float((x * 7 + y * 13 + k * 5) % 256);
      z[at] = (x + 2 * y + k) % 29 == 0 ? NAN : float(1000 + (x * 3 + y * 5 + k * 11) % 512) * 0.001f;
      c[3 * at + 0] = float((x * 5 + y * 3 + k * 7) % 300 - 20) + 0.5f;   // B: -19.5 .. 279.5
      c[3 * at + 1] = float((x * 11 + y * 2 + k) % 256) + 0.75f;          // G
      c[3 * at + 2] = float((x + y * 9 + k * 3) % 256);                   // R
    }
  T.setIdentity();
  const double a = double(k) / 1024.0;
  T.matrix()(0, 2) = a;
  T.matrix()(2, 0) = -a;
  T.matrix()(0, 3) = 0.01 * k;
  T.matrix()(1, 3) = -0.005 * k;
  T.matrix()(2, 3) = 0.002 * k;
}

uint32_t pixel_of(const float* c) {
  uint32_t v[3];
  for (int k = 0; k < 3; ++k) v[k] = c[k] >= 255.0f ? 255u : c[k] >= 0.0f ? uint32_t(c[k]) : 0u;
  return 0xFF000000u | v[2] << 16 | v[1] << 8 | v[0];
}

bool same_points(const PointCloudAggregator::PointCloud& a, const PointCloudAggregator::PointCloud& b) {
  return a.size() == b.size() && std::memcmp(a.x.data(), b.x.data(), a.size() * 4) == 0 && std::memcmp(a.y.data(), b.y.data(), a.size() * 4) == 0 &&
         std::memcmp(a.z.data(), b.z.data(), a.size() * 4) == 0 && std::memcmp(a.intensity.data(), b.intensity.data(), a.size() * 4) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: map_colour_facade_check <file>\n"); return 2; }
  DeviceContext::setErrorHandler(on_error);
  const IntrinsicMatrix K = IntrinsicMatrix::create(60.0f, 60.0f, 31.5f, 23.5f);
  RgbdCameraPyramid camera(W, H, K);
  camera.build(1);

  // 1. three coloured keyframes
  PointCloudAggregator aggregator(size_t(1) << 20), grey(size_t(1) << 20);
  aggregator.setColour(true);
  std::vector<RgbdImagePyramidPtr> pyramids;
  std::vector<dvo::compat::ImageMat> colours;
  for (int k = 0; k < 3; ++k) {
    dvo::compat::ImageMat I, Z, rgb;
    dvo::compat::Affine3d T;
    keyframe(k, I, Z, rgb, T);
    RgbdImagePyramidPtr p = camera.create(I, Z);
    p->level(0).rgb = rgb;
    if (!p->level(0).hasRgb() || p->hasColour()) { std::printf("hasRgb / hasColour are wrong before the build\n"); return 1; }
    char name[16];
    std::snprintf(name, sizeof name, "kf%04d", k);
    aggregator.add(name, p, T);
    grey.add(name, p, T);
    pyramids.push_back(p);
    colours.push_back(rgb);
  }
  PointCloudAggregator::PointCloud::Ptr cloud = aggregator.build();
  PointCloudAggregator::PointCloud::Ptr again = aggregator.build();
  if (cloud->size() < 1000 || !cloud->hasColour()) { std::printf("the coloured build gave %zu points, %zu colours\n", cloud->size(), cloud->rgba.size()); return 1; }
  if (!same_points(*cloud, *again) || cloud->rgba != again->rgba) { std::printf("two coloured builds differ\n"); return 1; }
  if (g_warnings != 0 || !pyramids[0]->hasColour()) { std::printf("the build did not attach the colour\n"); return 1; }
  for (size_t i = 0; i < cloud->size(); ++i)
    if ((cloud->rgba[i] >> 24) != 0xFFu) { std::printf("voxel %zu has alpha %u\n", i, unsigned(cloud->rgba[i] >> 24)); return 1; }
  PointCloudAggregator::PointCloud::Ptr plain = grey.build();
  if (!same_points(*cloud, *plain) || !plain->rgba.empty()) { std::printf("the grey aggregator's cloud differs in x, y, z, intensity, or holds colour\n"); return 1; }

  // 2. the organised cloud carries the pixels
  {
    AsyncPointCloudBuilder::BuildJob job(*pyramids[1]);
    AsyncPointCloudBuilder::PointCloud::Ptr organised = job.build();
    if (organised->size() != size_t(W * H) || !organised->hasColour()) { std::printf("the organised cloud holds no colour\n"); return 1; }
    const float* c = dvo::compat::image_ptr(colours[1]);
    for (int at = 0; at < W * H; ++at)
      if (organised->rgba[size_t(at)] != pixel_of(c + 3 * at)) { std::printf("organised cloud: the colour of pixel %d differs\n", at); return 1; }
    dvo::compat::ImageMat I, Z, rgb;
    dvo::compat::Affine3d T;
    keyframe(5, I, Z, rgb, T);
    RgbdImagePyramidPtr bare = camera.create(I, Z);
    AsyncPointCloudBuilder::BuildJob bare_job(*bare);
    if (!bare_job.build()->rgba.empty()) { std::printf("a pyramid without colour gave a coloured cloud\n"); return 1; }

    // 3. ... and registered, it turns the coloured aggregator grey
    aggregator.add("kf0005", bare, T);
    grey.add("kf0005", bare, T);
    PointCloudAggregator::PointCloud::Ptr fallback = aggregator.build();
    PointCloudAggregator::PointCloud::Ptr want = grey.build();
    if (g_warnings != 1) { std::printf("the fallback was reported %d times, not once\n", g_warnings); return 1; }
    if (!fallback->rgba.empty() || !same_points(*fallback, *want) || same_points(*fallback, *cloud)) { std::printf("the fallback is not the grey map\n"); return 1; }
    aggregator.remove("kf0005");
    PointCloudAggregator::PointCloud::Ptr back = aggregator.build();
    if (!same_points(*back, *cloud) || back->rgba != cloud->rgba) { std::printf("the coloured map did not come back\n"); return 1; }
  }

  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[1]); return 1; }
  for (size_t i = 0; i < cloud->size(); ++i) {
    const float rec[4] = {cloud->x[i], cloud->y[i], cloud->z[i], cloud->intensity[i]};
    std::fwrite(rec, sizeof rec, 1, f);
    std::fwrite(&cloud->rgba[i], 4, 1, f);
  }
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
