// cloud_colour.h -- colour in the keyframe map (include/dvo_hip.h, dvo_hip_frames_set_colour, dvo_hip_map_create_ex,
// dvo_hip_map_extract_colour and dvo_hip_map_render_colour): what the colour of a pixel of a pyramid level is, how a voxel fuses the
// colours of its points, and how a view of the map carries them.  These are the semantics of the reference's coloured map --
// benchmark_slam.cpp:89-90 keeps the camera image in level(0).rgb, AsyncPointCloudBuilder::BuildJob::build
// (dvo_core/src/visualization/async_point_cloud_builder.cpp:72-104) writes p.b, p.g, p.r from it whenever hasRgb(), and
// PointCloudAggregator::build voxel-filters PointXYZRGB clouds -- with an EXACT rounded per-voxel mean in place of PCL's float average.
// Shared by the kernels (cloud_colour.hip: k_colour_pack, k_colour_level; cloud_map.hip: k_map_insert, k_map_extract; map_render.hip:
// k_map_render, k_render_resolve) and the host compiler of the CPU tier (tests/test_map_colour.py), the yardstick the device results
// are compared with bit for bit.  INTEGER ONLY: no value here is ever a float, so there is nothing to contract or to round twice.
//
// Packed pixel.  A uint32 0x00RRGGBB: PCL's PointXYZRGB::rgba layout with A = 0.  colour_pack reads the 3 or 4 bytes of a pixel in one of
// the four DVO_HIP_PIXEL_{BGR8, RGB8, BGRA8, RGBA8} formats; alpha is ignored.
// Colour of level L at (u, v).  Taken from the frame's LEVEL-0 plane of packed pixels, per channel the rounded mean of the 2^L x 2^L block
// whose top-left pixel is (u << L, v << L):
//   c = (sum over the block + (1 << (2 L - 1))) >> 2 L;   L = 0: the pixel itself.
// The pyramid's level sizes are w0 >> L and h0 >> L (dvo_hip_frame_info; each level halves the one before, rounding down), so
// (u << L) + 2^L - 1 <= ((w0 >> L) << L) - 1 <= w0 - 1: every block lies inside level 0 and nothing is clamped.  A block's sum is at most
// 255 * 4^7 < 2^22 (kMaxLevels = 8).  This is NOT the intensity pyramid's chain of 2 x 2 float means: it is one mean over the whole block.
// Accumulation.  A coloured map has a side table parallel to the MapSlot table, same index: MapColourSlot {sr, sg, sb, pad}.  Each point
// adds its three 8-bit channels; 255 * 2^20 < 2^28, so nothing wraps up to kMapVoxelMaxPoints points.  {sr, sg} is addressed as one
// 64-bit word and sb as a 32-bit one (colour_word); a removal adds the two's complement of the same words (map_negate, cloud_map.h), the
// exact inverse of the insertion's adds.  A slot that is vacant or empty holds zeros.
// Extraction.  Per channel c = (2 s + n) / (2 n) in unsigned 64-bit integer division -- the mean s / n rounded half up -- clamped to 255;
// the record is 0xFF000000 | r << 16 | g << 8 | b.
// Render element.  uint64(bits(p.z)) << 32 | rgb24, rgb24 = the voxel's extracted colour without its alpha: the high half is the one of
// map_render.h, so the depth plane of a colour view equals the depth plane of the grey view bit for bit (the high half of a minimum is
// the minimum of the high halves).  Equal depths are broken by the LOWER packed colour.  A hole (the element still ~0) resolves to
// Z = NaN (kMapHole) and the colour word 0; a covered pixel has A = 0xFF.
#pragma once
#include <stdint.h>

#include "cloud_map.h"
#include "colour.h"   // pixel_channels, pixel_red_first

namespace dvo_hip {

// one slot of a coloured map's side table, 16 bytes: {sr, sg} is also addressed as a 64-bit word (cloud_map.hip: one atomic add)
struct alignas(16) MapColourSlot {
  uint32_t sr, sg, sb, pad;
};

DVO_HD uint32_t colour_rgb(uint32_t r, uint32_t g, uint32_t b) { return r << 16 | g << 8 | b; }
DVO_HD uint32_t colour_r(uint32_t c) { return (c >> 16) & 0xffu; }
DVO_HD uint32_t colour_g(uint32_t c) { return (c >> 8) & 0xffu; }
DVO_HD uint32_t colour_b(uint32_t c) { return c & 0xffu; }

// the packed pixel of the bytes at px (pixel_channels(pixel_format) of them; the format is one of the four colour formats)
DVO_HD uint32_t colour_pack(const uint8_t* px, int pixel_format) {
  const bool red_first = pixel_red_first(pixel_format);
  return colour_rgb(red_first ? px[0] : px[2], px[1], red_first ? px[2] : px[0]);
}

// the colour of pixel (u, v) of level `shift` from the level-0 plane (rows of `pitch` dwords); the block lies inside the plane (above)
DVO_HD uint32_t colour_level(const uint32_t* plane, int pitch, int u, int v, int shift) {
  if (shift == 0) return plane[size_t(v) * size_t(pitch) + size_t(u)];
  const int side = 1 << shift;
  const uint32_t* row = plane + size_t(v << shift) * size_t(pitch) + size_t(u << shift);
  uint32_t sr = 0, sg = 0, sb = 0;
  for (int y = 0; y < side; ++y, row += pitch)
    for (int x = 0; x < side; ++x) {
      const uint32_t c = row[x];
      sr += colour_r(c);
      sg += colour_g(c);
      sb += colour_b(c);
    }
  const uint32_t half = 1u << (2 * shift - 1);
  return colour_rgb((sr + half) >> (2 * shift), (sg + half) >> (2 * shift), (sb + half) >> (2 * shift));
}

// {sr, sg} of a point (or of a run of points) as the 64-bit word the side table adds it in: sr low
DVO_HD uint64_t colour_word(uint32_t sr, uint32_t sg) { return map_word(sr, sg); }

// the mean of a channel's sum over n > 0 points, rounded half up, clamped to 255
DVO_HD uint32_t colour_mean(uint32_t s, uint32_t n) {
  const uint64_t c = (2ull * uint64_t(s) + uint64_t(n)) / (2ull * uint64_t(n));
  return c > 255ull ? 255u : uint32_t(c);
}

// a voxel's colour record (n > 0)
DVO_HD uint32_t colour_extract(uint32_t n, uint32_t sr, uint32_t sg, uint32_t sb) {
  return 0xFF000000u | colour_rgb(colour_mean(sr, n), colour_mean(sg, n), colour_mean(sb, n));
}

// the z-buffer element of a colour view from the grey view's (map_render.h: the same depth half) and the voxel's colour record
DVO_HD uint64_t colour_render_value(uint64_t grey_value, uint32_t rgba) { return (grey_value & 0xffffffff00000000ull) | uint64_t(rgba & 0x00ffffffu); }

// a z-buffer element as the colour view's pixel
DVO_HD void colour_render_resolve(uint64_t e, uint32_t* rgba, uint32_t* z_bits) {
  const bool hole = e == ~0ull;
  *z_bits = hole ? kMapHole : uint32_t(e >> 32);
  *rgba = hole ? 0u : 0xFF000000u | (uint32_t(e) & 0x00ffffffu);
}

}  // namespace dvo_hip
