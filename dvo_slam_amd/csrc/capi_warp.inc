// capi_warp.inc -- frames warped under a pose behind the C-ABI (include/dvo_hip.h, dvo_hip_frames_warp_inverse and
// dvo_hip_frames_warp_forward; semantics: frame_warp.h; kernels: frame_warp.hip).  The frames reach the kernels through the frame table of
// the keyframe-map launches (upload_map_entries, capi_map.inc: the launches run on the main stream behind the builds of the frames, the
// {I, Z} pairs of the level are built where a frame does not hold them); the item's transform stands where a map launch has the pose.
// Arguments are checked before anything is launched or changed.  Textually included by capi.hip inside its extern "C" block.
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

// everything a warp call is refused for; sampled: the second frame of every pair (inverse) or null (forward); n_out lists of n planes
int check_warp(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, dvo_hip_frame* const* sampled, bool paired, const double* transforms,
               int level, const dvo_hip_warp_params* params, float* const* const* outs, int n_out, int out_on_device, dvo_hip_warp_params* p,
               const char* who) {
  bool others = transforms != nullptr && (!paired || sampled != nullptr);
  for (int k = 0; k < n_out; ++k) others = others && outs[k] != nullptr;
  int rc = check_frame_count(ctx, n, frames, who, others);
  if (rc != DVO_HIP_OK) return rc;
  long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    const dvo_hip_frame* f = frames[i];
    rc = check_frame(ctx, f, who, /*own_context=*/true);
    if (rc != DVO_HIP_OK) return rc;
    if (level < 0 || level >= f->levels) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame does not have that level");
    if (paired) {
      const dvo_hip_frame* s = sampled[i];
      rc = check_frame(ctx, s, who, /*own_context=*/true);
      if (rc != DVO_HIP_OK) return rc;
      if (level >= s->levels) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame does not have that level");
      if (s->lv[level].w != f->lv[level].w || s->lv[level].h != f->lv[level].h)
        return fail(ctx, DVO_HIP_ERR_INVALID, who, "the frames of a pair differ in size at the level");
    }
    blocks += (paired ? 2 : 1) * ((static_cast<long long>(f->lv[level].w) * f->lv[level].h + 255) / 256);
  }
  if (blocks > 0x7fffffffll / 256) return fail(ctx, DVO_HIP_ERR_INVALID, who, "too many pixels for one call");
  for (size_t k = 0; k < size_t(n) * 16; ++k)
    if (!std::isfinite(transforms[k])) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a transform is not finite");
  *p = params ? *params : dvo_hip_warp_params_default();
  if (p->mode != DVO_HIP_WARP_NEAREST && p->mode != DVO_HIP_WARP_SPLAT) return fail(ctx, DVO_HIP_ERR_INVALID, who, "unknown mode");
  if (!(p->occlusion_margin >= 0.0f)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the occlusion margin must be >= 0 (no NaN)");
  if (!(p->min_depth <= p->max_depth)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "need min_depth <= max_depth (no NaN)");
  for (uint32_t r : p->reserved)
    if (r != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a reserved field is not 0");
  for (int k = 0; k < n_out; ++k)
    for (int i = 0; i < n; ++i) {
      if (!outs[k][i]) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null output");
      if (out_on_device && !aligned_to(outs[k][i], 16)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a device plane must be 16-byte aligned");
    }
  return DVO_HIP_OK;
}

// where the planes of a warp are written: the caller's device planes, or n_out planes per item in the context's staging area
int warp_targets(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, int level, float* const* const* outs, int n_out, int out_on_device,
                 std::vector<std::vector<float*>>* dev) {
  dev->assign(size_t(n_out), std::vector<float*>(size_t(n)));
  if (out_on_device) {
    for (int k = 0; k < n_out; ++k)
      for (int i = 0; i < n; ++i) (*dev)[size_t(k)][size_t(i)] = outs[k][i];
    return DVO_HIP_OK;
  }
  size_t bytes = 0;
  for (int i = 0; i < n; ++i) bytes += size_t(n_out) * ((size_t(frames[i]->lv[level].w) * frames[i]->lv[level].h * 4 + 15) & ~size_t(15));
  DVO_HIP_TRY(ctx, ctx->map_stage.reserve(bytes));
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    const size_t plane = (size_t(frames[i]->lv[level].w) * frames[i]->lv[level].h * 4 + 15) & ~size_t(15);
    for (int k = 0; k < n_out; ++k, at += plane) (*dev)[size_t(k)][size_t(i)] = reinterpret_cast<float*>(ctx->map_stage.as<char>() + at);
  }
  return DVO_HIP_OK;
}

// the end of a warp: staged planes to the caller's host arrays, and the wait (as dvo_hip_frames_world_points)
int warp_finish(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, int level, float* const* const* outs, int n_out, int out_on_device,
                const std::vector<std::vector<float*>>& dev) {
  if (!out_on_device)
    for (int k = 0; k < n_out; ++k)
      for (int i = 0; i < n; ++i)
        DVO_HIP_TRY(ctx, hipMemcpyAsync(outs[k][i], dev[size_t(k)][size_t(i)], size_t(frames[i]->lv[level].w) * frames[i]->lv[level].h * 4,
                                        hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
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
  int rc = check_warp(ctx, n, raster_frames, sampled_frames, true, transforms, level, params_or_null, outs, n_out, out_on_device, &p, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<std::vector<float*>> dev;
  rc = warp_targets(ctx, n, raster_frames, level, outs, n_out, out_on_device, &dev);
  if (rc != DVO_HIP_OK) return rc;
  std::vector<MapEntry> entries;
  std::vector<WarpPlanes> planes(static_cast<size_t>(n));
  long long max_pixels = 0;
  for (int i = 0; i < n; ++i) {
    entries.push_back(MapEntry{raster_frames[i], map_pose_prepare(transforms + size_t(i) * 16), 1, nullptr});
    entries.push_back(MapEntry{sampled_frames[i], MapPose{}, 1, nullptr});
    planes[size_t(i)] = WarpPlanes{dev[0][size_t(i)], dev[1][size_t(i)], n_out == 3 ? dev[2][size_t(i)] : nullptr};
    max_pixels = std::max(max_pixels, static_cast<long long>(raster_frames[i]->lv[level].w) * raster_frames[i]->lv[level].h);
  }
  int blocks = 0;
  rc = upload_map_entries(ctx, entries, level, &blocks);
  if (rc != DVO_HIP_OK) return rc;
  const size_t bytes = planes.size() * sizeof(WarpPlanes);
  DVO_HIP_TRY(ctx, ctx->render_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->render_tbl.p, planes.data(), bytes));
  launch_warp_inverse(ctx->stream, ctx->map_tbl.as<MapFrame>(), ctx->render_tbl.as<WarpPlanes>(), n, max_pixels, p.occlusion_margin);
  DVO_HIP_TRY(ctx, hipGetLastError());
  ctx->frame_warps += n;
  return warp_finish(ctx, n, raster_frames, level, outs, n_out, out_on_device, dev);
}

int dvo_hip_frames_warp_forward(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const double* transforms, int level,
                                const dvo_hip_warp_params* params_or_null, float* const* intensity_out, float* const* depth_out,
                                int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "frames_warp_forward";
  float* const* const outs[2] = {intensity_out, depth_out};
  dvo_hip_warp_params p;
  int rc = check_warp(ctx, n, frames, nullptr, false, transforms, level, params_or_null, outs, 2, out_on_device, &p, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<std::vector<float*>> dev;
  rc = warp_targets(ctx, n, frames, level, outs, 2, out_on_device, &dev);
  if (rc != DVO_HIP_OK) return rc;
  std::vector<MapEntry> entries;
  std::vector<RenderPlanes> planes(static_cast<size_t>(n));
  std::vector<size_t> first(static_cast<size_t>(n));               // the item's first element in the z-buffers
  size_t elements = 0;
  bool one_size = true;
  for (int i = 0; i < n; ++i) {
    const FrameLevel& L = frames[i]->lv[level];
    entries.push_back(MapEntry{frames[i], map_pose_prepare(transforms + size_t(i) * 16), 1, nullptr});
    planes[size_t(i)] = RenderPlanes{dev[0][size_t(i)], dev[1][size_t(i)]};
    first[size_t(i)] = elements;
    elements += size_t(L.w) * size_t(L.h);
    one_size = one_size && L.w == frames[0]->lv[level].w && L.h == frames[0]->lv[level].h;
  }
  int blocks = 0;
  rc = upload_map_entries(ctx, entries, level, &blocks);
  if (rc != DVO_HIP_OK) return rc;
  const size_t bytes = planes.size() * sizeof(RenderPlanes);
  DVO_HIP_TRY(ctx, ctx->render_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->render_tbl.p, planes.data(), bytes));
  DVO_HIP_TRY(ctx, ctx->render_zbuf.reserve(elements * sizeof(unsigned long long)));
  unsigned long long* zbuf = ctx->render_zbuf.as<unsigned long long>();
  const MapFrame* tbl = ctx->map_tbl.as<MapFrame>();
  const RenderPlanes* out = ctx->render_tbl.as<RenderPlanes>();
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
  return warp_finish(ctx, n, frames, level, outs, 2, out_on_device, dev);
}
