// map_device.h -- what the kernels of the keyframe map share on the device (cloud_map.hip, map_merge.hip, cloud_colour.hip): which entry of
// a launch's table a workgroup belongs to, and the per-wavefront counter updates.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace dvo_hip
