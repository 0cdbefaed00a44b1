// The C++ facade's colour ingest (RgbdCameraPyramid::createFromColour): a BGR frame and its depth become a device pyramid.  Checks that
// the level-0 intensity the engine holds is the CV_BGR2GRAY grey of the frame, and, with host mirrors on (as the drop-in bridge runs),
// that level 0's host matrices, point cloud and acceleration structure are filled from the device.  Prints "ok <pixels checked>" or the
// first mismatch.
#include <cstdio>
#include <vector>

#include "dvo/core/rgbd_image.h"
#include "dvo_benchmark/image_io.h"

int main() {
  const int w = 64, h = 48;
  dvo::core::IntrinsicMatrix K = dvo::core::IntrinsicMatrix::create(50.0f, 50.0f, 31.5f, 23.5f);
  dvo::core::RgbdCameraPyramid camera(w, h, K);
  camera.build(3);
  std::vector<uint8_t> bgr(size_t(w) * h * 3);
  std::vector<uint16_t> depth(size_t(w) * h);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      uint8_t* p = &bgr[(size_t(y) * w + x) * 3];
      p[0] = uint8_t(x * 4 + y);
      p[1] = uint8_t(y * 5 + 3 * x);
      p[2] = uint8_t(255 - x * 3);
      depth[size_t(y) * w + x] = uint16_t(5000 + 10 * x + 7 * y);
    }
  dvo::core::RgbdImage::hostMirrors(true);
  dvo::core::RgbdImagePyramidPtr pyr = camera.createFromColour(bgr.data(), DVO_HIP_PIXEL_BGR8, 0, depth.data());
  pyr->build(3);
  std::vector<float> intensity(size_t(w) * h);
  if (dvo_hip_frame_download_plane(pyr->device_context(), pyr->device_frame(), 0, 0, intensity.data()) != DVO_HIP_OK) {
    std::printf("download failed: %s\n", dvo_hip_last_error(pyr->device_context()));
    return 1;
  }
  for (size_t i = 0; i < intensity.size(); ++i) {
    const uint8_t* p = &bgr[i * 3];
    const float want = float(dvo_benchmark::greyFromRgb8(p[2], p[1], p[0]));
    if (intensity[i] != want) {
      std::printf("pixel %zu: %g != %g\n", i, double(intensity[i]), double(want));
      return 1;
    }
  }
  // level 0's host mirrors: the grey and the depth in metres as soon as the pyramid is built, then the point cloud and the
  // interleaved acceleration structure (LocalTracker's calls, dvo_slam/src/local_tracker.cpp:163-169)
  dvo::core::RgbdImage& l0 = pyr->level(0);
  if (dvo::compat::image_empty(l0.intensity) || dvo::compat::image_empty(l0.depth) || dvo::compat::image_rows(l0.intensity) != h ||
      dvo::compat::image_cols(l0.intensity) != w) {
    std::printf("level 0 has no host intensity / depth\n");
    return 1;
  }
  for (size_t i = 0; i < intensity.size(); ++i) {
    const float z = float(depth[i]) * (1.0f / 5000.0f);
    if (dvo::compat::image_ptr(l0.intensity)[i] != intensity[i] || dvo::compat::image_ptr(l0.depth)[i] != z) {
      std::printf("host mirror pixel %zu: %g %g\n", i, double(dvo::compat::image_ptr(l0.intensity)[i]), double(dvo::compat::image_ptr(l0.depth)[i]));
      return 1;
    }
  }
  l0.buildPointCloud();
  l0.buildAccelerationStructure();
  if (size_t(l0.pointcloud.cols()) != intensity.size() || dvo::compat::image_empty(l0.intensity_dx)) {
    std::printf("level 0: point cloud of %d points, derivatives %s\n", int(l0.pointcloud.cols()), dvo::compat::image_empty(l0.intensity_dx) ? "missing" : "present");
    return 1;
  }
  for (size_t i = 0; i < intensity.size(); ++i)
    if (l0.pointcloud(2, int(i)) != dvo::compat::image_ptr(l0.depth)[i]) {
      std::printf("point %zu: z %g != depth %g\n", i, double(l0.pointcloud(2, int(i))), double(dvo::compat::image_ptr(l0.depth)[i]));
      return 1;
    }
  std::printf("ok %zu\n", intensity.size());
  return 0;
}
