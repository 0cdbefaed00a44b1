// cloud_colour.hip -- the colour planes of frames on the device (cloud_colour.h; include/dvo_hip.h, dvo_hip_frames_set_colour and
// dvo_hip_frame_download_colour): the caller's 8-bit BGR / RGB / BGRA / RGBA planes -> the frames' level-0 planes of packed pixels
// (k_colour_pack), and the colour plane of a pyramid level as the map's insertion sees it (k_colour_level).
//
// k_colour_pack runs over planes x pixels in one launch: a lane owns one pixel, a wavefront 64 consecutive pixels in raster order, a
// workgroup 256; planes of different sizes share the launch, a workgroup finds its plane by bisecting the table's first_block column
// (map_device.h, as k_map_insert does).  A lane reads its 3 or 4 bytes with byte loads -- a 3-byte pixel is aligned to nothing, and
// this runs once per keyframe, not per match -- and stores one dword, coalesced.
// k_colour_level: a lane per pixel of the level, the 2^L x 2^L block of level 0 read with dword loads (the rows of an odd-width plane are
// not 16-byte aligned), one dword stored.  No LDS, no barriers, no atomics, 256-thread workgroups.
#include "global_ptr.h"
#include "launch.h"
#include "cloud_colour.h"
#include "map_device.h"

namespace dvo_hip {

namespace {

__global__ __launch_bounds__(256) void k_colour_pack(const ColourPlane* __restrict__ tbl, int n_planes, int pixel_format) {
  const ColourPlane& f = tbl[map_frame_of(tbl, n_planes, int(blockIdx.x))];
  const int i = (int(blockIdx.x) - f.first_block) * 256 + int(threadIdx.x);
  if (i >= f.w * f.h) return;                                  // (i < w * h: inside both planes)
  const int u = i % f.w, v = i / f.w, channels = pixel_channels(pixel_format);
  const uint8_t* px = f.src + size_t(v) * size_t(f.pitch) + size_t(u) * size_t(channels);   // (pitch >= w * channels: inside the row)
  f.dst[i] = colour_pack(px, pixel_format);
}

__global__ __launch_bounds__(256) void k_colour_level(const uint32_t* __restrict__ plane, int pitch, int shift, int w, int h, uint32_t* __restrict__ out) {
  const int i = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (i >= w * h) return;                                      // (w, h: the level's size, so the block lies inside level 0, cloud_colour.h)
  out[i] = colour_level(plane, pitch, i % w, i / w, shift);
}

}  // namespace

void launch_colour_pack(hipStream_t s, const ColourPlane* tbl, int n_planes, int total_blocks, int pixel_format) {
  k_colour_pack<<<dim3(total_blocks), dim3(256), 0, s>>>(tbl, n_planes, pixel_format);
}

void launch_colour_level(hipStream_t s, const uint32_t* plane, int pitch, int shift, int w, int h, uint32_t* out) {
  k_colour_level<<<dim3((w * h + 255) / 256), dim3(256), 0, s>>>(plane, pitch, shift, w, h, out);
}

}  // namespace dvo_hip
