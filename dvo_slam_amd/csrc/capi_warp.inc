// capi_warp.inc -- frames warped under a pose behind the C-ABI (include/dvo_hip.h, dvo_hip_frames_warp_inverse and
// dvo_hip_frames_warp_forward; semantics: frame_warp.h; kernels: frame_warp.hip): calls that read frames at a level
// (capi_frame_calls.inc), the item's transform standing where a map launch has the pose.  Arguments are checked before anything is
// launched or changed.  Textually included by capi.hip inside its extern "C" block.
static_assert(sizeof(dvo_hip_warp_params) == 32, "dvo_hip_warp_params: four fields and four reserved words");

dvo_hip_warp_params dvo_hip_warp_params_default(void) {
  dvo_hip_warp_params p;
  std::memset(&p, 0, sizeof p);
  p.mode = DVO_HIP_WARP_SPLAT;
  p.occlusion_margin = 0.05f;
  p.min_depth = 0.0f;
  p.max_depth = INFINITY;
  return p;
}

namespace {

// everything a warp call is refused for; sampled: the second frame of every pair (inverse) or null (forward); n_out lists of n planes,
// *results: those planes as the call's results
int check_warp(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, dvo_hip_frame* const* sampled, bool paired, const double* transforms,
               int level, const dvo_hip_warp_params* params, float* const* const* outs, int n_out, int out_on_device, dvo_hip_warp_params* p,
               std::vector<ResultArray>* results, const char* who) {
  bool others = transforms != nullptr && (!paired || sampled != nullptr);
  for (int k = 0; k < n_out; ++k) others = others && outs[k] != nullptr;
  int rc = check_frame_count(ctx, n, frames, who, others);
  if (rc == DVO_HIP_OK)
    rc = check_frames_at_level(ctx, n, frames, level, paired ? 2 : 1, kMaxPixelBlocks, /*budget_early=*/false, who, [&](int i, const dvo_hip_frame* f) -> int {
      if (!paired) return DVO_HIP_OK;
      const dvo_hip_frame* s = sampled[i];
      const int rc_s = check_frame(ctx, s, who, /*own_context=*/true);
      if (rc_s != DVO_HIP_OK) return rc_s;
      if (level >= s->levels) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame does not have that level");
      if (s->lv[level].w != f->lv[level].w || s->lv[level].h != f->lv[level].h)
        return fail(ctx, DVO_HIP_ERR_INVALID, who, "the frames of a pair differ in size at the level");
      return DVO_HIP_OK;
    });
  if (rc != DVO_HIP_OK) return rc;
  if (!transforms_finite(transforms, size_t(n))) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a transform is not finite");
  *p = params ? *params : dvo_hip_warp_params_default();
  if (p->mode != DVO_HIP_WARP_NEAREST && p->mode != DVO_HIP_WARP_SPLAT) return fail(ctx, DVO_HIP_ERR_INVALID, who, "unknown mode");
  if (!(p->occlusion_margin >= 0.0f)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the occlusion margin must be >= 0 (no NaN)");
  rc = check_range_and_reserved(ctx, p->min_depth, p->max_depth, p->reserved, 4, who);
  if (rc != DVO_HIP_OK) return rc;
  *results = frame_planes(n, frames, level, outs, n_out, 4);
  return check_results(ctx, *results, out_on_device, who, "null output", "a device plane must be 16-byte aligned");
}

}  // namespace

int dvo_hip_frames_warp_inverse(dvo_hip_context* ctx, int n, dvo_hip_frame* const* raster_frames, dvo_hip_frame* const* sampled_frames,
                                const double* transforms, int level, const dvo_hip_warp_params* params_or_null, float* const* intensity_out,
                                float* const* depth_out, float* const* difference_out_or_null, int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "frames_warp_inverse";
  float* const* const outs[3] = {intensity_out, depth_out, difference_out_or_null};
  const int n_out = difference_out_or_null ? 3 : 2;
  dvo_hip_warp_params p;
  std::vector<ResultArray> results;
  int rc = check_warp(ctx, n, raster_frames, sampled_frames, true, transforms, level, params_or_null, outs, n_out, out_on_device, &p, &results, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<void*> dev;                                          // list k's plane of item i: dev[k * n + i]
  rc = stage_results(ctx, results, out_on_device, &dev);
  if (rc != DVO_HIP_OK) return rc;
  const auto plane = [&](int k, int i) { return static_cast<float*>(dev[size_t(k) * size_t(n) + size_t(i)]); };
  std::vector<FrameEntry> entries;
  std::vector<WarpPlanes> planes(static_cast<size_t>(n));
  long long max_pixels = 0;
  for (int i = 0; i < n; ++i) {
    entries.push_back(FrameEntry{raster_frames[i], map_pose_prepare(transforms + size_t(i) * 16), 1, nullptr});
    entries.push_back(FrameEntry{sampled_frames[i], MapPose{}, 1, nullptr});
    planes[size_t(i)] = WarpPlanes{plane(0, i), plane(1, i), n_out == 3 ? plane(2, i) : nullptr};
    max_pixels = std::max(max_pixels, static_cast<long long>(raster_frames[i]->lv[level].w) * raster_frames[i]->lv[level].h);
  }
  int blocks = 0;
  rc = upload_frame_entries(ctx, entries, level, &blocks);
  if (rc != DVO_HIP_OK) return rc;
  const size_t bytes = planes.size() * sizeof(WarpPlanes);
  DVO_HIP_TRY(ctx, ctx->side_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->side_tbl.p, planes.data(), bytes));
  launch_warp_inverse(ctx->stream, ctx->frame_tbl.as<MapFrame>(), ctx->side_tbl.as<WarpPlanes>(), n, max_pixels, p.occlusion_margin);
  DVO_HIP_TRY(ctx, hipGetLastError());
  ctx->frame_warps += n;
  return finish_results(ctx, results, out_on_device, dev);
}

int dvo_hip_frames_warp_forward(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const double* transforms, int level,
                                const dvo_hip_warp_params* params_or_null, float* const* intensity_out, float* const* depth_out,
                                int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "frames_warp_forward";
  float* const* const outs[2] = {intensity_out, depth_out};
  dvo_hip_warp_params p;
  std::vector<ResultArray> results;
  int rc = check_warp(ctx, n, frames, nullptr, false, transforms, level, params_or_null, outs, 2, out_on_device, &p, &results, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<void*> dev;                                          // item i's intensity plane: dev[i], its depth plane: dev[n + i]
  rc = stage_results(ctx, results, out_on_device, &dev);
  if (rc != DVO_HIP_OK) return rc;
  std::vector<FrameEntry> entries;
  std::vector<RenderPlanes> planes(static_cast<size_t>(n));
  std::vector<size_t> first(static_cast<size_t>(n));               // the item's first element in the z-buffers
  size_t elements = 0;
  bool one_size = true;
  for (int i = 0; i < n; ++i) {
    const FrameLevel& L = frames[i]->lv[level];
    entries.push_back(FrameEntry{frames[i], map_pose_prepare(transforms + size_t(i) * 16), 1, nullptr});
    planes[size_t(i)] = RenderPlanes{static_cast<float*>(dev[size_t(i)]), static_cast<float*>(dev[size_t(n) + size_t(i)])};
    first[size_t(i)] = elements;
    elements += size_t(L.w) * size_t(L.h);
    one_size = one_size && L.w == frames[0]->lv[level].w && L.h == frames[0]->lv[level].h;
  }
  int blocks = 0;
  rc = upload_frame_entries(ctx, entries, level, &blocks);
  if (rc != DVO_HIP_OK) return rc;
  const size_t bytes = planes.size() * sizeof(RenderPlanes);
  DVO_HIP_TRY(ctx, ctx->side_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->side_tbl.p, planes.data(), bytes));
  DVO_HIP_TRY(ctx, ctx->scratch_words.reserve(elements * sizeof(unsigned long long)));
  unsigned long long* zbuf = ctx->scratch_words.as<unsigned long long>();
  const MapFrame* tbl = ctx->frame_tbl.as<MapFrame>();
  const RenderPlanes* out = ctx->side_tbl.as<RenderPlanes>();
  launch_render_fill(ctx->stream, zbuf, static_cast<long long>(elements));
  if (one_size) {
    const long long pixels = static_cast<long long>(elements / size_t(n));
    launch_warp_forward(ctx->stream, tbl, n, pixels, p.mode, p.min_depth, p.max_depth, zbuf);
    launch_render_resolve(ctx->stream, zbuf, out, n, pixels, /*colour=*/false);
  } else {
    // items of differing sizes: the z-buffers lie behind one another all the same, and every item is a launch of its own
    for (int i = 0; i < n; ++i) {
      const long long pixels = static_cast<long long>(frames[i]->lv[level].w) * frames[i]->lv[level].h;
      launch_warp_forward(ctx->stream, tbl + i, 1, pixels, p.mode, p.min_depth, p.max_depth, zbuf + first[size_t(i)]);
      launch_render_resolve(ctx->stream, zbuf + first[size_t(i)], out + i, 1, pixels, /*colour=*/false);
    }
  }
  DVO_HIP_TRY(ctx, hipGetLastError());
  ctx->frame_warps += n;
  return finish_results(ctx, results, out_on_device, dev);
}
