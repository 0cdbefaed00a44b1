// cloud_normal.hip -- the organised normal planes of keyframes on the device (cloud_normal.h; include/dvo_hip.h, dvo_hip_frames_normals):
// the depth plane of one pyramid level of n keyframes under their poses -> one 16-byte record {N.x, N.y, N.z, has} per pixel, the world
// normal exactly as an insertion into a map with normals sees it.
//
// k_frame_normals runs over frames x pixels in one launch like k_world_points: a lane owns one pixel, a wavefront 64 consecutive pixels
// in raster order, a workgroup 256; frames of different sizes share the launch (MapFrame, map_frame_of).  A lane reads its own {I, Z}
// pair (8 B) and, where the pixel is usable and not on the border, the four neighbouring depths: two of them are its wavefront's own
// cache lines, the rows above and below were or will be read by other wavefronts and mostly hit the L2.  The record is stored
// coalesced.  No LDS, no barriers, no atomics.
#include "global_ptr.h"
#include "launch.h"
#include "cloud_normal.h"
#include "map_device.h"

namespace dvo_hip {

namespace {

__global__ __launch_bounds__(256) void k_frame_normals(const MapFrame* __restrict__ tbl, int n_frames, float min_depth, float max_depth) {
#pragma clang fp contract(off)
  const MapFrame& f = tbl[map_frame_of(tbl, n_frames, int(blockIdx.x))];
  const int i = (int(blockIdx.x) - f.first_block) * 256 + int(threadIdx.x);
  if (i >= f.w * f.h) return;
  const int u = i % f.w, v = i / f.w;
  const float z = frame_depth(f, i);
  const float K[4] = {f.K[0], f.K[1], f.K[2], f.K[3]};
  float P[3], N[3];
  const bool usable = map_world_point(f.pose, K, u, v, z, min_depth, max_depth, P);
  const bool has = frame_normal(f, K, i, u, v, z, usable, N);
  const GlobalF32x4 rec = {N[0], N[1], N[2], has ? 1.0f : 0.0f};
  *((Global<GlobalF32x4>)global_ptr(f.out) + i) = rec;
}

}  // namespace

void launch_frame_normals(hipStream_t s, const MapFrame* tbl, int n_frames, int total_blocks, float min_depth, float max_depth) {
  k_frame_normals<<<dim3(total_blocks), dim3(256), 0, s>>>(tbl, n_frames, min_depth, max_depth);
}

}  // namespace dvo_hip
