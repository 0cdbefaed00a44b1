// sensor_formats.h -- raw sensor planes as the ingest takes them (include/dvo_hip.h, DVO_HIP_PIXEL_BAYER_* and DVO_HIP_PIXEL_YUYV8 /
// _UYVY8): what a camera driver publishes as image_raw, before the image_proc stage the reference's nodes sit behind
// (dvo_ros/src/camera_base.cpp:30 subscribes to camera/rgb/image_rect: debayered, then rectified).  Every sensor format is DEFINED by
// its BGR8 image, stated here once; the frame is then a BGR8 frame: its grey is colour.h's grey_of with the BGR weights of that image
// (sensor_grey), its colour the packed 0x00RRGGBB of that image (sensor_packed, cloud_colour.h's layout).  Shared by the kernel
// (sensor_convert.hip) and the host compiler of the CPU tier (tests/test_sensor_formats.py), which holds it to a second statement in
// numpy.  INTEGER ONLY: nothing here is ever a float.
//
// Bayer mosaics, 8 bit.  A format is named by the 2 x 2 block at the image's top-left corner, row-major (RGGB: R G / G B).  Bilinear
// demosaic in OpenCV's arithmetic (COLOR_Bayer*2BGR): at a red or blue site of value v the own colour is v,
// G = (N + S + W + E + 2) >> 2 and the opposite colour = (NW + NE + SW + SE + 2) >> 2; at a green site the colour of its row's
// non-green sites = (W + E + 1) >> 1 and the other colour = (N + S + 1) >> 1.  Neighbours outside the image are read by reflection
// about the edge pixel (index -1 -> 1, w -> w - 2, rows alike), which keeps the mosaic's phase.  THE INTERIOR IS OPENCV'S, THE BORDER
// IS OURS: at the one-pixel border OpenCV copies the neighbouring results instead.  Needs w >= 2 and h >= 2.
//
// YUV 4:2:2, 8 bit: YUYV (bytes Y0 U Y1 V per pixel pair, ROS "yuv422_yuy2") and UYVY (U Y0 V Y1, ROS "yuv422").  BT.601 limited
// range in 20-bit fixed point, int32, arithmetic shift; both pixels of a pair use the pair's U and V:
//   y = max(0, Y - 16) * 1220542 + (1 << 19),  u = U - 128,  v = V - 128
//   R = sat8((y + 1673527 v) >> 20),  G = sat8((y - 409993 u - 852492 v) >> 20),  B = sat8((y + 2116026 u) >> 20)
// The constants ARE the definition.  They are meant to be those of OpenCV's COLOR_YUV2BGR_YUY2 / _UYVY; that equality is not checked
// anywhere in this repository.  Every intermediate fits int32: |.| < 239 * 1220542 + 2^19 + 128 * 2116026 < 2^30.  Needs an even w.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "colour.h"

namespace dvo_hip {

DVO_HD bool sensor_is_bayer(int format) { return format >= DVO_HIP_PIXEL_BAYER_RGGB8 && format <= DVO_HIP_PIXEL_BAYER_GRBG8; }
DVO_HD bool sensor_is_yuv(int format) { return format == DVO_HIP_PIXEL_YUYV8 || format == DVO_HIP_PIXEL_UYVY8; }
// bytes per pixel of a sensor format, 0 for any other value
DVO_HD int sensor_bytes(int format) { return sensor_is_bayer(format) ? 1 : sensor_is_yuv(format) ? 2 : 0; }
// the phase (x & 1, y & 1) of a Bayer format's red sites; the blue sites have the opposite phase in both
DVO_HD int bayer_red_x(int format) { return format == DVO_HIP_PIXEL_BAYER_BGGR8 || format == DVO_HIP_PIXEL_BAYER_GRBG8 ? 1 : 0; }
DVO_HD int bayer_red_y(int format) { return format == DVO_HIP_PIXEL_BAYER_BGGR8 || format == DVO_HIP_PIXEL_BAYER_GBRG8 ? 1 : 0; }
// true: the luma byte of a YUV pixel comes first (YUYV)
DVO_HD bool yuv_luma_first(int format) { return format == DVO_HIP_PIXEL_YUYV8; }

struct SensorBgr {
  unsigned b, g, r;
};
DVO_HD unsigned sensor_grey(SensorBgr c) { return grey_of(c.b, c.g, c.r, grey_weights(false)); }
DVO_HD uint32_t sensor_packed(SensorBgr c) { return uint32_t(c.r << 16 | c.g << 8 | c.b); }

// index i of a row (or column) of n >= 2 samples, -1 <= i <= n, reflected about the edge sample
DVO_HD int sensor_reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

// The pixel at a mosaic site of value v from its eight neighbours.  px, py: the site's phase against the red sites', (x & 1) ^ red_x
// and (y & 1) ^ red_y -- (0, 0) red, (1, 1) blue, (1, 0) green of a red row, (0, 1) green of a blue row.  One path with selects.
DVO_HD SensorBgr bayer_site(int px, int py, unsigned v, unsigned n, unsigned s, unsigned w, unsigned e, unsigned nw, unsigned ne, unsigned sw,
                            unsigned se) {
  const unsigned cross = (n + s + w + e + 2u) >> 2, diag = (nw + ne + sw + se + 2u) >> 2;
  const unsigned hor = (w + e + 1u) >> 1, ver = (n + s + 1u) >> 1;
  const bool green = px != py, red_row = py == 0;
  const unsigned of_row = green ? hor : v, of_other = green ? ver : diag;   // the colour of this row's non-green sites, and the other one
  SensorBgr c;
  c.g = green ? v : cross;
  c.r = red_row ? of_row : of_other;
  c.b = red_row ? of_other : of_row;
  return c;
}

// pixel (x, y) of the w x h mosaic `plane` (rows of `pitch` bytes), red sites at phase (red_x, red_y): reads stay inside the image
DVO_HD SensorBgr bayer_pixel(const uint8_t* plane, size_t pitch, int w, int h, int x, int y, int red_x, int red_y) {
  const uint8_t* rn = plane + size_t(sensor_reflect(y - 1, h)) * pitch;
  const uint8_t* rc = plane + size_t(y) * pitch;
  const uint8_t* rs = plane + size_t(sensor_reflect(y + 1, h)) * pitch;
  const int xw = sensor_reflect(x - 1, w), xe = sensor_reflect(x + 1, w);
  return bayer_site((x & 1) ^ red_x, (y & 1) ^ red_y, rc[x], rn[x], rs[x], rc[xw], rc[xe], rn[xw], rn[xe], rs[xw], rs[xe]);
}

DVO_HD unsigned sensor_sat8(int v) { return v < 0 ? 0u : v > 255 ? 255u : unsigned(v); }

// the pixel of luma Y and its pair's chroma U, V
DVO_HD SensorBgr yuv_pixel(int Y, int U, int V) {
  const int y = (Y > 16 ? Y - 16 : 0) * 1220542 + (1 << 19), u = U - 128, v = V - 128;
  SensorBgr c;
  c.r = sensor_sat8((y + 1673527 * v) >> 20);
  c.g = sensor_sat8((y - 409993 * u - 852492 * v) >> 20);
  c.b = sensor_sat8((y + 2116026 * u) >> 20);
  return c;
}

// pixel (x, y) of the YUV 4:2:2 `plane` (rows of `pitch` bytes, 2 bytes per pixel)
DVO_HD SensorBgr yuv_at(const uint8_t* plane, size_t pitch, int x, int y, bool luma_first) {
  const uint8_t* pair = plane + size_t(y) * pitch + size_t(x & ~1) * 2;   // the 4 bytes of the pixel pair
  const int l = luma_first ? 0 : 1, c = luma_first ? 1 : 0;
  return yuv_pixel(pair[l + 2 * (x & 1)], pair[c], pair[c + 2]);
}

}  // namespace dvo_hip
