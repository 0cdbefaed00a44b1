// The C++ facade with raw sensor planes (include/dvo_hip.h, DVO_HIP_PIXEL_BAYER_* / _YUYV8 / _UYVY8): RgbdCameraPyramid::createFromColour from a
// Bayer GRBG mosaic as the Kinect / OpenNI driver publishes it, and RgbdImagePyramid::setColour from a YUYV plane.  The planes are constant,
// so the expected values follow from the definitions without a demosaic of their own: a constant mosaic of value v is the BGR image
// (v, v, v), whose grey is v; Y = 126, U = V = 128 is the BGR pixel (128, 128, 128).  Prints "ok <pixels checked>" or the first mismatch.
#include <cstdio>
#include <vector>

#include "dvo/core/rgbd_image.h"

int main() {
  const int w = 64, h = 48;
  dvo::core::IntrinsicMatrix K = dvo::core::IntrinsicMatrix::create(50.0f, 50.0f, 31.5f, 23.5f);
  dvo::core::RgbdCameraPyramid camera(w, h, K);
  camera.build(3);
  const std::vector<uint8_t> mosaic(size_t(w) * h, uint8_t(93));
  std::vector<uint8_t> yuyv(size_t(w) * h * 2);
  for (size_t i = 0; i < yuyv.size(); ++i) yuyv[i] = i % 2 == 0 ? uint8_t(126) : uint8_t(128);
  std::vector<uint16_t> depth(size_t(w) * h, uint16_t(7500));
  dvo::core::RgbdImagePyramidPtr pyr = camera.createFromColour(mosaic.data(), DVO_HIP_PIXEL_BAYER_GRBG8, 0, depth.data());
  pyr->build(3);
  std::vector<float> intensity(size_t(w) * h);
  if (dvo_hip_frame_download_plane(pyr->device_context(), pyr->device_frame(), 0, 0, intensity.data()) != DVO_HIP_OK) {
    std::printf("download failed: %s\n", dvo_hip_last_error(pyr->device_context()));
    return 1;
  }
  for (size_t i = 0; i < intensity.size(); ++i)
    if (intensity[i] != 93.0f) {
      std::printf("pixel %zu: %g != 93\n", i, double(intensity[i]));
      return 1;
    }
  if (!pyr->setColour(yuyv.data(), 0, DVO_HIP_PIXEL_YUYV8) || !pyr->hasColour()) {
    std::printf("setColour failed: %s\n", dvo_hip_last_error(pyr->device_context()));
    return 1;
  }
  std::vector<uint32_t> colour(size_t(w) * h);
  if (dvo_hip_frame_download_colour(pyr->device_context(), pyr->device_frame(), 0, colour.data()) != DVO_HIP_OK) {
    std::printf("download_colour failed: %s\n", dvo_hip_last_error(pyr->device_context()));
    return 1;
  }
  for (size_t i = 0; i < colour.size(); ++i)
    if (colour[i] != 0x00808080u) {
      std::printf("colour %zu: %08x != 00808080\n", i, unsigned(colour[i]));
      return 1;
    }
  std::printf("ok %zu\n", intensity.size());
  return 0;
}
