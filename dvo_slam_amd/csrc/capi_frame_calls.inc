// capi_frame_calls.inc -- what the calls share that read the {I, Z} planes of a list of frames at one pyramid level (world points and
// normals, map insert / remove / move, renders into frames, warps, covisibility, fern codes): the check of the call's frames, the frame
// table their kernels read (MapFrame, map_device.h), and the way a call's results reach the caller's device or host arrays.  Every launch
// runs on the context's main stream, behind the build-stream work that wrote the frames; the scratch of the context they use, and what
// orders its uses, is listed where it is declared (capi.hip).  Textually included by capi.hip inside its extern "C" block, ahead of
// capi_map.inc; with C++ linkage, so that none of these names becomes a symbol of the library.
extern "C++" {
namespace {

// ---- the check of the frames ----

constexpr long long kMaxBlocks = 0x7fffffffll;               // a frame table counts its blocks of 256 pixels in an int ...
constexpr long long kMaxPixelBlocks = kMaxBlocks / 256;      // ... and the warps, covisibility and the codes count its pixels in one

// a call's own rule of frame i, behind the rules below; what it returns ends the check unless it is DVO_HIP_OK
using FrameRule = std::function<int(int, const dvo_hip_frame*)>;

// The frames of a call whose list check_frame_count has passed: every frame is one of this context and has the level, passes `rule`, and
// all of them, entries_per_frame table entries each, fit max_blocks.  budget_early: the budget is held to after every frame (a frame
// behind the one that breaks it is not looked at), else once, after the last.
int check_frames_at_level(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int level, int entries_per_frame, long long max_blocks,
                          bool budget_early, const char* who, const FrameRule& rule = nullptr) {
  long long blocks = 0;
  for (int i = 0; i < n_frames; ++i) {
    const dvo_hip_frame* f = frames[i];
    int rc = check_frame(ctx, f, who, /*own_context=*/true);
    if (rc != DVO_HIP_OK) return rc;
    if (level < 0 || level >= f->levels) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame does not have that level");
    if (rule && (rc = rule(i, f)) != DVO_HIP_OK) return rc;
    blocks += entries_per_frame * ((static_cast<long long>(f->lv[level].w) * f->lv[level].h + 255) / 256);
    if (blocks > max_blocks && (budget_early || i == n_frames - 1)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "too many pixels for one call");
  }
  return DVO_HIP_OK;
}

// n 4 x 4 transforms, 16 doubles each
bool transforms_finite(const double* T, size_t n) {
  for (size_t k = 0; k < n * 16; ++k)
    if (!std::isfinite(T[k])) return false;
  return true;
}

// what every params struct ends with: its depth range, then its reserved words
int check_range_and_reserved(dvo_hip_context* ctx, float min_depth, float max_depth, const uint32_t* reserved, int n_reserved, const char* who) {
  if (!(min_depth <= max_depth)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "need min_depth <= max_depth (no NaN)");
  for (int k = 0; k < n_reserved; ++k)
    if (reserved[k] != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a reserved field is not 0");
  return DVO_HIP_OK;
}

// ---- the frame table ----

// one entry of a launch's frame table: a frame under a pose, added (+1) or -- dvo_hip_map_remove, dvo_hip_map_move -- subtracted (-1)
struct FrameEntry {
  dvo_hip_frame* frame;
  MapPose pose;
  int sign;
  float* out;                          // MapFrame::out (k_world_points), else null
};

// The frame table of one launch on the main stream, into ctx->frame_tbl: the {I, Z} pairs of `level` come from plane C where the frame
// holds it, else from the taps A (built now where missing: what dvo_hip_frame_download_plane reads planes 0 and 1 from).  A frame may
// stand in several entries.  coloured: the entries also name the frames' colour planes (checked: check_map_colour).
int upload_frame_entries(dvo_hip_context* ctx, const std::vector<FrameEntry>& entries, int level, int* total_blocks, bool coloured = false) {
  std::vector<dvo_hip_frame*> frames;
  for (const FrameEntry& e : entries)
    if (std::find(frames.begin(), frames.end(), e.frame) == frames.end()) frames.push_back(e.frame);
  int rc = wait_for_build(ctx, int(frames.size()), frames.data());
  if (rc != DVO_HIP_OK) return rc;
  // the taps of the frames that hold neither flavour at this level, one ensure_roles per camera (it takes frames of one camera)
  std::vector<dvo_hip_frame*> missing;
  for (dvo_hip_frame* f : frames) {
    const FrameLevel& L = f->lv[level];
    if (!((L.cur_have & kCurC) && L.C) && !(L.cur_have & kCurAB)) missing.push_back(f);
  }
  while (!missing.empty()) {
    std::vector<dvo_hip_frame*> group, rest;
    for (dvo_hip_frame* f : missing) (f->cam == missing[0]->cam ? group : rest).push_back(f);
    rc = ensure_roles(ctx, int(group.size()), group.data(), 0, level, level, 0.0f, 0.0f);
    if (rc != DVO_HIP_OK) return rc;
    missing.swap(rest);
  }
  std::vector<MapFrame> host(entries.size() + 1);
  int blocks = 0;
  for (size_t i = 0; i < entries.size(); ++i) {
    const dvo_hip_frame* f = entries[i].frame;
    const FrameLevel& L = f->lv[level];
    MapFrame& m = host[i];
    const bool from_c = (L.cur_have & kCurC) && L.C;
    m.iz = from_c ? reinterpret_cast<const float*>(L.C) : reinterpret_cast<const float*>(L.A);
    m.stride = from_c ? 2 : 4;
    m.out = entries[i].out;
    m.pose = entries[i].pose;
    std::memcpy(m.K, f->cam->K[level], sizeof m.K);
    m.w = L.w;
    m.h = L.h;
    m.first_block = blocks;
    m.sign = entries[i].sign;
    m.colour = coloured ? f->colour.as<uint32_t>() : nullptr;
    m.colour_pitch = f->lv[0].w;
    m.shift = level;
    blocks += (L.w * L.h + 255) / 256;
  }
  *total_blocks = blocks;
  return upload_block_table(ctx, ctx->frame_tbl, host, blocks);
}

// ... of n frames, all added, under poses[16 * i ..] (null: no pose of them is read).  outs (may be null): MapFrame::out.
int upload_frames(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const double* poses, int level, void* const* outs,
                  int* total_blocks, bool coloured = false) {
  std::vector<FrameEntry> entries;
  for (int i = 0; i < n_frames; ++i)
    entries.push_back(FrameEntry{frames[i], poses ? map_pose_prepare(poses + size_t(i) * 16) : MapPose{}, 1,
                                 outs ? static_cast<float*>(outs[i]) : nullptr});
  return upload_frame_entries(ctx, entries, level, total_blocks, coloured);
}

// ---- the results ----

// one result array of a call: the caller's array (null: not wanted), its bytes, and the alignment the kernel that writes it needs
struct ResultArray {
  void* dst;
  size_t bytes, align;
};

// the results of a call that writes n_out planes per frame, bytes_per_pixel for every pixel of the frame's level: outs[k][i], list by list
std::vector<ResultArray> frame_planes(int n_frames, dvo_hip_frame* const* frames, int level, float* const* const* outs, int n_out, size_t bytes_per_pixel) {
  std::vector<ResultArray> results;
  for (int k = 0; k < n_out; ++k)
    for (int i = 0; i < n_frames; ++i)
      results.push_back(ResultArray{outs[k][i], size_t(frames[i]->lv[level].w) * frames[i]->lv[level].h * bytes_per_pixel, 16});
  return results;
}

// every result is there and, in device memory, aligned; in groups of `group` results, of which the missing are reported first
int check_results(dvo_hip_context* ctx, const std::vector<ResultArray>& results, int out_on_device, const char* who, const char* null_rule,
                  const char* align_rule, size_t group = 1) {
  for (size_t g = 0; g < results.size(); g += group) {
    for (size_t k = g; k < g + group; ++k)
      if (!results[k].dst) return fail(ctx, DVO_HIP_ERR_INVALID, who, null_rule);
    for (size_t k = g; k < g + group && out_on_device; ++k)
      if (!aligned_to(results[k].dst, results[k].align)) return fail(ctx, DVO_HIP_ERR_INVALID, who, align_rule);
  }
  return DVO_HIP_OK;
}

// Where the kernels write a call's results: dev[k] is the caller's own array in device memory, else a region of ctx->result_stage,
// aligned as the result asks, behind `scratch` bytes the call keeps for itself at the start of the area (null: not wanted).
int stage_results(dvo_hip_context* ctx, const std::vector<ResultArray>& results, int out_on_device, std::vector<void*>* dev, size_t scratch = 0) {
  dev->assign(results.size(), nullptr);
  std::vector<size_t> at(results.size(), 0);
  size_t bytes = scratch;
  for (size_t k = 0; k < results.size() && !out_on_device; ++k)
    if (results[k].dst) {
      at[k] = align_up(bytes, results[k].align);
      bytes = at[k] + results[k].bytes;
    }
  DVO_HIP_TRY(ctx, ctx->result_stage.reserve(bytes));
  for (size_t k = 0; k < results.size(); ++k)
    if (results[k].dst) (*dev)[k] = out_on_device ? results[k].dst : ctx->result_stage.as<char>() + at[k];
  return DVO_HIP_OK;
}

// The end of such a call, behind its last launch: staged results to the caller's host arrays, and the wait for the main stream -- with
// device results too: the next call may reallocate the scratch that this call's kernels read.
int finish_results(dvo_hip_context* ctx, const std::vector<ResultArray>& results, int out_on_device, const std::vector<void*>& dev) {
  for (size_t k = 0; k < results.size() && !out_on_device; ++k)
    if (results[k].dst) DVO_HIP_TRY(ctx, hipMemcpyAsync(results[k].dst, dev[k], results[k].bytes, hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}

}  // namespace
}  // extern "C++"
