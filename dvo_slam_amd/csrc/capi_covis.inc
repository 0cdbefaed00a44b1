// capi_covis.inc -- keyframe covisibility behind the C-ABI (include/dvo_hip.h, dvo_hip_frames_covisibility; semantics: covisibility.h;
// kernel: covisibility.hip): a call that reads frames at a level (capi_frame_calls.inc), every listed frame ONCE in the frame table; the
// pairs, in the side table, index it.  Arguments are checked before anything is launched or changed.  Textually included by capi.hip
// inside its extern "C" block.
static_assert(sizeof(dvo_hip_covis_params) == 32, "dvo_hip_covis_params: four fields and four reserved words");
static_assert(sizeof(dvo_hip_covis_record) == 32 && offsetof(dvo_hip_covis_record, photo) == 24, "dvo_hip_covis_record: six counts and a sum");

dvo_hip_covis_params dvo_hip_covis_params_default(void) {
  dvo_hip_covis_params p;
  std::memset(&p, 0, sizeof p);
  p.depth_tolerance = 0.05f;
  p.depth_tolerance_rel = 0.0f;
  p.min_depth = 0.0f;
  p.max_depth = INFINITY;
  return p;
}

namespace {

constexpr int kCovisMaxPairs = 1 << 22;
constexpr size_t kCovisRingBytes = 32 * 1024;        // pair tables up to this size (585 pairs) go through the ring of pinned slots

// everything a covisibility call is refused for but a misaligned device array (as check_warp); *max_pixels: the largest a of the pairs
int check_covis(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int n_pairs, const int32_t* pair_a, const int32_t* pair_b,
                const double* transforms, int level, const dvo_hip_covis_params* params, const dvo_hip_covis_record* records,
                dvo_hip_covis_params* p, long long* max_pixels, const char* who) {
  int rc = check_frame_count(ctx, n_frames, frames, who, pair_a != nullptr && pair_b != nullptr && transforms != nullptr && records != nullptr);
  if (rc != DVO_HIP_OK) return rc;
  if (n_pairs < 1) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (n_pairs > kCovisMaxPairs) return fail(ctx, DVO_HIP_ERR_INVALID, who, "more than 2^22 pairs");   // (before any pair is read)
  rc = check_frames_at_level(ctx, n_frames, frames, level, 1, kMaxPixelBlocks, /*budget_early=*/true, who);
  if (rc != DVO_HIP_OK) return rc;
  *max_pixels = 0;
  for (int k = 0; k < n_pairs; ++k) {
    if (pair_a[k] < 0 || pair_a[k] >= n_frames || pair_b[k] < 0 || pair_b[k] >= n_frames)
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "a pair names a frame outside the list");
    const FrameLevel& L = frames[pair_a[k]]->lv[level];
    *max_pixels = std::max(*max_pixels, static_cast<long long>(L.w) * L.h);
  }
  if (!transforms_finite(transforms, size_t(n_pairs))) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a transform is not finite");
  *p = params ? *params : dvo_hip_covis_params_default();
  if (!(p->depth_tolerance >= 0.0f) || !(p->depth_tolerance_rel >= 0.0f))
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "the depth tolerances must be >= 0 (no NaN)");
  return check_range_and_reserved(ctx, p->min_depth, p->max_depth, p->reserved, 4, who);
}

}  // namespace

int dvo_hip_frames_covisibility(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int n_pairs, const int32_t* pair_a,
                                const int32_t* pair_b, const double* transforms, int level, const dvo_hip_covis_params* params_or_null,
                                dvo_hip_covis_record* records_out, int out_on_device) {
  DVO_ENTER(ctx);
  const char* who = "frames_covisibility";
  dvo_hip_covis_params p;
  long long max_pixels = 0;
  int rc = check_covis(ctx, n_frames, frames, n_pairs, pair_a, pair_b, transforms, level, params_or_null, records_out, &p, &max_pixels, who);
  if (rc != DVO_HIP_OK) return rc;
  const size_t record_bytes = size_t(n_pairs) * sizeof(dvo_hip_covis_record);
  const std::vector<ResultArray> results = {{records_out, record_bytes, 8}};
  rc = check_results(ctx, results, out_on_device, who, "bad argument", "device records must be 8-byte aligned");
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<void*> dev;
  rc = stage_results(ctx, results, out_on_device, &dev);
  if (rc != DVO_HIP_OK) return rc;
  unsigned long long* records = static_cast<unsigned long long*>(dev[0]);
  // the frame table: every listed frame once (no pose of it is read: the transform belongs to the pair)
  int blocks = 0;
  rc = upload_frames(ctx, n_frames, frames, nullptr, level, nullptr, &blocks);
  if (rc != DVO_HIP_OK) return rc;
  std::vector<CovisPair> pairs(static_cast<size_t>(n_pairs));
  for (int k = 0; k < n_pairs; ++k) pairs[size_t(k)] = CovisPair{pair_a[k], pair_b[k], map_pose_prepare(transforms + size_t(k) * 16)};
  const size_t bytes = pairs.size() * sizeof(CovisPair);
  DVO_HIP_TRY(ctx, ctx->side_tbl.reserve(bytes));
  if (bytes <= kCovisRingBytes) {
    DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->side_tbl.p, pairs.data(), bytes));
  } else {
    // a long pair list (n x n of 256 keyframes is 3.5 MB) goes past the ring of pinned slots, which would grow to 48 slots of that size
    // and keep a host copy: one plain copy, ordered on the stream; the call waits for the stream before `pairs` goes out of scope
    ctx->tables.forget(ctx->side_tbl.p);
    DVO_HIP_TRY(ctx, hipMemcpyAsync(ctx->side_tbl.p, pairs.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  DVO_HIP_TRY(ctx, hipMemsetAsync(records, 0, record_bytes, ctx->stream));
  launch_covisibility(ctx->stream, ctx->frame_tbl.as<MapFrame>(), ctx->side_tbl.as<CovisPair>(), n_pairs, max_pixels, p, records);
  DVO_HIP_TRY(ctx, hipGetLastError());
  ctx->covisibility_pairs += n_pairs;
  return finish_results(ctx, results, out_on_device, dev);
}
