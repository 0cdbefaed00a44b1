// map_device.h -- what the kernels of the keyframe map share on the device (cloud_map.hip, map_merge.hip, cloud_colour.hip): which entry of
// a launch's table a workgroup belongs to, the per-wavefront counter updates, and the normal of a frame's pixel (cloud_normal.hip too).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "global_ptr.h"

namespace dvo_hip {

// the entry (a MapFrame, a MapMergeEntry, a ColourPlane) that owns workgroup b: first_block is strictly increasing (every entry has at least one
// pixel or record), tbl[n_entries] ends the list
template <typename Entry>
__device__ __forceinline__ int map_frame_of(const Entry* __restrict__ tbl, int n_entries, int b) {
  int lo = 0, hi = n_entries;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tbl[mid].first_block <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void wave_count(unsigned long long* counter, unsigned long long mask, int lane) {
  if (lane == 0 && mask != 0) (void)__hip_atomic_fetch_add(counter, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ... or, for a frame that is being removed, the count taken back (two's complement: the counter holds what the map's frames added)
__device__ __forceinline__ void wave_uncount(unsigned long long* counter, unsigned long long mask, int lane) {
  if (lane == 0 && mask != 0) (void)__hip_atomic_fetch_add(counter, 0ull - (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the depth of pixel i of a frame's level (i inside the plane)
__device__ __forceinline__ float frame_depth(const MapFrame& f, int i) {
  return *(Global<const float>)global_ptr(f.iz + size_t(i) * size_t(f.stride) + 1);
}

// The world normal N[0..2] of pixel i = (u, v), depth z, of a frame's level (cloud_normal.h; k_frame_normals, and k_map_insert into a
// map with normals): the four neighbouring depths are loaded only where the pixel is usable and not on the border, so every index
// i - w, i - 1, i + 1, i + w lies inside the plane.  false (N = 0): the pixel has no normal.
__device__ __forceinline__ bool frame_normal(const MapFrame& f, const float K[4], int i, int u, int v, float z, bool usable, float N[3]) {
  N[0] = N[1] = N[2] = 0.0f;
  if (!usable || !normal_interior(f.w, f.h, u, v)) return false;
  float n[3];
  if (!normal_camera(K, u, v, z, frame_depth(f, i - 1), frame_depth(f, i + 1), frame_depth(f, i - f.w), frame_depth(f, i + f.w), n)) return false;
  normal_world(f.pose, n, N);
  return true;
}

}  // namespace dvo_hip
