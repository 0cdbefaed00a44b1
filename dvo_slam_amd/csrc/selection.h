// selection.h -- the caller selection of a reference frame (include/dvo_hip.h, dvo_hip_frames_set_selection): which of the pixels the
// threshold predicate selected at pyramid level `level` stay selected.  Shared by the apply pass (pyramid_kernels.hip,
// k_apply_selection) and the host compiler of the CPU tier (tests/test_selection.py).
// A coarse pixel carries the depth of the level-0 pixel (x << level, y << level) (the depth pyramid subsamples,
// rgbd_image.cpp:128-140, 169), so that is the mask byte it is judged by: no mask pyramid is stored.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hd_compat.h"

namespace dvo_hip {

// A depth range is off when it admits every non-negative depth: [0, +inf) (the default), or anything wider.
DVO_HD bool selection_range_on(float min_depth, float max_depth) { return min_depth > 0.0f || !(max_depth >= 3.402823466e+38f); }

// true: the selected pixel (x, y) of `level`, depth z, stays selected.  mask0 (null: no mask) is the level-0 mask, `pitch` bytes per row.
DVO_HD bool selection_keeps(const uint8_t* mask0, size_t pitch, int level, int x, int y, float z, bool range_on, float min_depth,
                            float max_depth) {
  if (mask0 && mask0[(size_t(y) << level) * pitch + (size_t(x) << level)] == 0) return false;
  return !range_on || (min_depth <= z && z <= max_depth);
}

}  // namespace dvo_hip
