// capi_normal.inc -- surface normals behind the C-ABI (include/dvo_hip.h, dvo_hip_frames_normals, dvo_hip_map_extract_normals and
// dvo_hip_map_render_normals; semantics: cloud_normal.h; kernels: cloud_normal.hip, cloud_map.hip, map_render.hip).  Each is the twin of
// a call of capi_map.inc and shares its body: the same checks, streams and staging, one more array.  Textually included by capi.hip
// inside its extern "C" block, behind capi_map.inc.
static_assert(sizeof(MapNormalSlot) == 16, "a voxel's normal sums are 16 bytes (include/dvo_hip.h)");

int dvo_hip_frames_normals(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const double* poses, int level, float min_depth,
                           float max_depth, float* const* out, int out_on_device) {
  DVO_ENTER(ctx);
  return frames_organised(ctx, n_frames, frames, poses, level, min_depth, max_depth, out, out_on_device, true, "frames_normals");
}

int dvo_hip_map_extract_normals(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_points, float* xyzi, float* normals, uint32_t* rgba_or_null,
                                uint32_t* counts_or_null, uint64_t* keys_or_null, int out_on_device, size_t* n_points) {
  DVO_LOCK(ctx);
  return map_extract(ctx, map, max_points, xyzi, false, rgba_or_null, counts_or_null, keys_or_null, out_on_device, n_points, "map_extract_normals",
                     true, normals);
}

int dvo_hip_map_render_normals(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4], const double* poses,
                               const dvo_hip_render_params* params, float* const* normals_out, float* const* depth_out, int out_on_device) {
  DVO_ENTER(ctx);
  return map_render(ctx, map, n_views, width, height, K, poses, params, false, reinterpret_cast<void* const*>(normals_out), depth_out, out_on_device,
                    "map_render_normals", true);
}
