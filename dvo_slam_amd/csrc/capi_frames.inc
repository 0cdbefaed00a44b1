// capi_frames.inc -- cameras, frames and their planes: build tickets, the per-level geometry of a camera, frame allocation, the batched frame
// build (raw ingest + pyramid), and the role planes of a batch's frames (ensure_roles).  Textually included by capi.hip inside its anonymous
// namespace (the context, the workspace and the error macros are defined there).
// ticket + event for work just enqueued on the build stream; stamps the frames it wrote
int stamp_build(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames) {
  const unsigned long long seq = ++ctx->build_seq;
  DVO_HIP_TRY(ctx, hipEventRecord(ctx->build_events[seq % dvo_hip_context::kBuildRing], ctx->build_stream));
  for (int i = 0; i < n; ++i) frames[i]->built_seq = seq;
  return DVO_HIP_OK;
}

// make `stream` (the main stream, or the upload stream about to overwrite a transfer buffer) wait for build ticket `need`
int wait_for_ticket(dvo_hip_context* ctx, unsigned long long need, bool upload) {
  unsigned long long& waited = upload ? ctx->upload_waited_seq : ctx->main_waited_seq;
  hipStream_t stream = upload ? ctx->upload_stream : ctx->stream;
  if (need <= waited) return DVO_HIP_OK;
  // tickets older than the ring have had their event re-recorded for a newer ticket of the same stream: waiting for the
  // oldest live one still orders us after `need`
  const unsigned long long oldest_live = ctx->build_seq >= dvo_hip_context::kBuildRing ? ctx->build_seq - dvo_hip_context::kBuildRing + 1 : 1;
  const unsigned long long use = need < oldest_live ? oldest_live : need;
  DVO_HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->build_events[use % dvo_hip_context::kBuildRing], 0));
  waited = use;
  return DVO_HIP_OK;
}

// the main stream must not touch these frames before the build-stream work that produced them is done
int wait_for_build(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames) {
  unsigned long long need = 0;
  for (int i = 0; i < n; ++i)
    if (frames[i] && frames[i]->built_seq > need) need = frames[i]->built_seq;
  return wait_for_ticket(ctx, need, /*upload=*/false);
}

// the reference role of a level is built for the thresholds (ithr, dthr), or holds an explicit accepted set (which no threshold replaces)
bool ref_ready(const FrameLevel& L, float ithr, float dthr) { return L.selected && (L.explicit_sel || (L.ithr == ithr && L.dthr == dthr)); }

void mark_selected(FrameLevel& L, float ithr, float dthr) {
  L.selected = true;
  L.explicit_sel = false;
  L.q3 = false;                                              // (a fresh plane R)
  L.ithr = ithr;
  L.dthr = dthr;
}

// Setting, replacing or clearing a frame's caller selection: every reference-role selection of the frame is stale.
void invalidate_reference_role(dvo_hip_frame* f) {
  for (int l = 0; l < f->levels; ++l) {
    f->lv[l].selected = false;
    f->lv[l].explicit_sel = false;
    f->lv[l].q3 = false;
  }
}

// The caller selection of those of the n frames that carry one, over their planes R of levels l0 .. l1 just built on `stream` (one launch,
// behind the kernel that built them).  Nothing is launched when no frame carries a selection.  report: dvo_hip_frame_select's mask (one
// frame, one level).
int apply_selection(dvo_hip_context* ctx, hipStream_t stream, int n, dvo_hip_frame* const* frames, int l0, int l1, int cap,
                    uint8_t* report = nullptr) {
  std::vector<SelectionApply> host;
  const unsigned long long visit = ++ctx->sel_visits;
  for (int i = 0; i < n; ++i) {
    dvo_hip_frame* f = frames[i];
    if (!f->sel_on || f->sel_visit == visit) continue;      // (a frame listed twice is applied once: its pixels would leave twice)
    f->sel_visit = visit;
    SelectionApply a;
    for (int l = 0; l < kMaxLevels; ++l) a.R[l] = l < f->levels ? f->lv[l].R : nullptr;
    a.sel_count = f->sel_count;
    a.mask = f->sel_has_mask ? f->sel_mask.as<uint8_t>() : nullptr;
    a.pitch = f->lv[0].w;
    a.range_on = selection_range_on(f->sel_min, f->sel_max) ? 1 : 0;
    a.min_depth = f->sel_min;
    a.max_depth = f->sel_max;
    a.report = report;
    host.push_back(a);
  }
  if (host.empty()) return DVO_HIP_OK;
  DevBuf& table = stream == ctx->build_stream ? ctx->sel_tbl_build : ctx->sel_tbl_main;
  const size_t bytes = host.size() * sizeof(SelectionApply);
  DVO_HIP_TRY(ctx, table.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(stream, table.p, host.data(), bytes));
  const CameraGeom* cam = frames[0]->cam;
  const LevelSpan span = level_span(l0, l1, cam->w, cam->h, /*pixel_blocks=*/true);
  launch_apply_selection(stream, table.as<SelectionApply>(), int(host.size()), span, cap);
  DVO_HIP_TRY(ctx, hipGetLastError());
  return DVO_HIP_OK;
}

// The error word of a resident launch: one of a ring of words of Workspace::host_status indexed by the launch counter (the per-step
// words start behind the ring).  A workgroup of an EARLIER launch that gives up late -- the host returns from the direct path as soon
// as every pair is done, not when every workgroup has left -- raises its own launch's word, not the one the next batch has just reset.
constexpr int kResidentErrorWords = 8;

const int kLlBlocksPerPair = 32;
const size_t kCostlyEmptyStepWorkgroups = 131072;   // (see chain_level: from here on the step ahead of the poll is held back on a level's tail)
const int kFusedLoglikMaxPixels = 160 * 120;      // any batch
const int kFusedLoglikMaxPixelsBatch = 320 * 240;  // batches of 512 pairs and more (schedule_of)

// RgbdCameraPyramid::build (rgbd_image.cpp:283-296) + RgbdCamera ctor template (:186-204)
int get_camera(dvo_hip_context* ctx, int w, int h, const float K[4], int levels, const CameraGeom** out) {
  // (before anything is allocated or compared: a NaN would go into the tx / ty tables and into the memcmp key below)
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(K[k])) return fail(ctx, DVO_HIP_ERR_INVALID, "frame_create: K must be finite");
  if (!(K[0] > 0.0f && K[1] > 0.0f)) return fail(ctx, DVO_HIP_ERR_INVALID, "frame_create: need fx > 0 and fy > 0");
  // one geometry per (size, intrinsics), with the tables of every level the size admits: frames of one camera share it
  // whatever level count each was created with (a batch only needs FirstLevel + 1 levels on each pyramid)
  for (CameraGeom* c : ctx->cameras)
    if (c->w0 == w && c->h0 == h && std::memcmp(c->K0, K, 16) == 0) {
      *out = c;
      return DVO_HIP_OK;
    }
  int all = 1;
  while (all < kMaxLevels && (w >> all) >= 2 && (h >> all) >= 2) ++all;
  levels = all > levels ? all : levels;
  CameraGeom* c = new CameraGeom();
  c->w0 = w; c->h0 = h; c->levels = levels;
  std::memcpy(c->K0, K, 16);
  size_t total = 0;
  for (int l = 0; l < levels; ++l) {
    c->w[l] = l == 0 ? w : c->w[l - 1] / 2;
    c->h[l] = l == 0 ? h : c->h[l - 1] / 2;
    for (int k = 0; k < 4; ++k) c->K[l][k] = l == 0 ? K[k] : c->K[l - 1][k] * 0.5f;   // IntrinsicMatrix::scale(0.5f), Q17
    total += align_up(size_t(c->w[l]) * 4, 256) + align_up(size_t(c->h[l]) * 4, 256);
  }
  hipError_t e = c->tables.reserve(total);
  if (e != hipSuccess) {
    delete c;
    ctx->err = std::string("hipMalloc(camera tables): ") + hipGetErrorString(e);
    return DVO_HIP_ERR_HIP;
  }
  std::vector<float> host;
  char* base = c->tables.as<char>();
  size_t off = 0;
  for (int l = 0; l < levels; ++l) {
    const float fx = c->K[l][0], fy = c->K[l][1], ox = c->K[l][2], oy = c->K[l][3];
    host.resize(size_t(c->w[l]) + c->h[l]);
    for (int x = 0; x < c->w[l]; ++x) host[x] = (float(x) - ox) / fx;            // rgbd_image.cpp:198
    for (int y = 0; y < c->h[l]; ++y) host[c->w[l] + y] = (float(y) - oy) / fy;  // rgbd_image.cpp:199
    c->tx[l] = reinterpret_cast<float*>(base + off);
    off += align_up(size_t(c->w[l]) * 4, 256);
    c->ty[l] = reinterpret_cast<float*>(base + off);
    off += align_up(size_t(c->h[l]) * 4, 256);
    e = hipMemcpy(c->tx[l], host.data(), size_t(c->w[l]) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->ty[l], host.data() + c->w[l], size_t(c->h[l]) * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      c->tables.release();
      delete c;
      ctx->err = std::string("hipMemcpy(camera tables): ") + hipGetErrorString(e);
      return DVO_HIP_ERR_HIP;
    }
  }
  ctx->cameras.push_back(c);
  *out = c;
  return DVO_HIP_OK;
}

// tiles of the sweep kernel for one pair (see LevelGeom::linear)
void level_tiles(int w, int h, int rows_per_wave, bool linear, int* tiles_x, int* tiles_y) {
  const int th = kWavesPerBlock * rows_per_wave;
  if (linear) {
    const int segments = (w * h + kTileW - 1) / kTileW;
    *tiles_x = 1;
    *tiles_y = (segments + th - 1) / th;
  } else {
    *tiles_x = (w + kTileW - 1) / kTileW;
    *tiles_y = (h + th - 1) / th;
  }
}

// the contracted window sweep (align_fast.hip, variants 8 / 9) also takes widths that are no multiple of its 64 columns (160 x 120)
bool level_uses_fast_window(const dvo_hip_context* ctx, int w, int h) {
  return ctx->opt_variant >= 8 && fast_sweep_takes_width(w) && w < 32768 && h < 32768;   // (option "ref_compat" included: the COMPAT instantiations)
}

// the sweep with the whole current level in LDS (align_small.hip): the default schedule's levels that the window sweeps do not take
bool level_uses_small(const dvo_hip_context* ctx, int w, int h);

bool level_is_linear(const dvo_hip_context* ctx, int w) { return ctx->opt_variant >= 5 && w % kTileW != 0 && !level_uses_fast_window(ctx, w, 4); }

// the sweep that stages the current frame's window in LDS (align_window.hip, variants 6 / 7; align_fast.hip) handles this level; its tile is 64 x 16
bool level_uses_window(const dvo_hip_context* ctx, int w, int h) {
  return (ctx->opt_variant >= 6 && w % kTileW == 0 && w < 32768 && h < 32768) || level_uses_fast_window(ctx, w, h);
}

bool level_uses_small(const dvo_hip_context* ctx, int w, int h) {
  return ctx->opt_small_sweep && ctx->opt_variant >= 8 && !ctx->opt_ref_compat && !ctx->opt_ref_order && !level_uses_window(ctx, w, h) && level_is_linear(ctx, w) && small_sweep_takes(w, h);
}

LevelGeom make_geom(const dvo_hip_context* ctx, const CameraGeom* cam, int level, int rows_per_wave) {
  LevelGeom g;
  g.w = cam->w[level]; g.h = cam->h[level];
  g.fx = cam->K[level][0]; g.fy = cam->K[level][1]; g.ox = cam->K[level][2]; g.oy = cam->K[level][3];
  g.wi_x = 0.5f * g.fx / 255.0f; g.wi_y = 0.5f * g.fy / 255.0f;
  g.half_wi_x = 0.5f * g.wi_x; g.half_wi_y = 0.5f * g.wi_y; g.half_fx = 0.5f * g.fx; g.half_fy = 0.5f * g.fy;
  g.tx = cam->tx[level]; g.ty = cam->ty[level];
  g.level = level;
  g.pair_list = nullptr;
  g.skip_flags = nullptr;
  g.linear = level_is_linear(ctx, g.w) ? 1 : 0;
  level_tiles(g.w, g.h, rows_per_wave, g.linear != 0, &g.tiles_x, &g.tiles_y);
  g.rcp_table = ctx->opt_ref_compat ? ctx->rcp_table.as<float>() : nullptr;
  g.rcp_shift = ctx->rcp_shift;
  g.rcp_packed = ctx->opt_ref_compat == 1 ? ctx->rcp_packed : 0;   // (2: the table through memory, the path of a table that does not pack)
  // (not under "ref_compat": a run that is compared with the reference's own numbers keeps every low part -- round-5 advisor finding)
  g.gram_hi_j = !ctx->opt_gram_lo_parts && !ctx->opt_deterministic && !ctx->opt_ref_compat && ctx->opt_variant == 8 && size_t(g.w) * g.h >= 150000 ? 1 : 0;
  g.small = level_uses_small(ctx, g.w, g.h) ? 1 : 0;
  // (not under "ref_order": its passes read the residual pairs by pixel, ref_order.hip)
  g.compact = ctx->opt_compact_residuals && !ctx->opt_ref_order && ctx->opt_variant >= 8 && rows_per_wave == 4 && fast_sweep_supports(g) ? 1 : 0;   // (launch_residual_reduce's test)
  return g;
}

// rows of 64 pixels each wavefront sweeps: large tiles amortise the 85-value wave reduction, small tiles
// keep all 256 CUs busy when the batch is small
int pick_rows_per_wave(const dvo_hip_context* ctx, const CameraGeom* cam, int level, int n_pairs) {
  if (level_uses_window(ctx, cam->w[level], cam->h[level])) return 4;
  if (level_uses_small(ctx, cam->w[level], cam->h[level]) && ctx->opt_rows_per_wave == 0) {
    // segments per wavefront such that a pair gets BatchPolicy::small_level_tiles workgroups
    const int tiles = ctx->opt_small_tiles > 0 ? ctx->opt_small_tiles : BatchPolicy(ctx->compute_units).small_level_tiles(n_pairs);
    const int segments = (cam->w[level] * cam->h[level] + kTileW - 1) / kTileW;
    const int rows = (segments + kWavesPerBlock * tiles - 1) / (kWavesPerBlock * tiles);
    return rows < 1 ? 1 : rows;
  }
  if (ctx->opt_deterministic) return ctx->opt_rows_per_wave > 0 ? ctx->opt_rows_per_wave : 4;   // one tile height whatever the batch
  if (ctx->opt_rows_per_wave > 0) return ctx->opt_rows_per_wave;
  // A large batch fills the device whatever the tile: short tiles (2 rows per wavefront: the schedule with the pinned prologue) run the
  // coarse levels' sweeps 6-11 % faster than tall ones since the f16 Gram (scripts/ab_sweep.py: 1024 pairs, 160x120 0.200 -> 0.187 ms,
  // 80x60 0.056 -> 0.050 ms; bench step 14.22 -> 13.89 ms)
  if (BatchPolicy(ctx->compute_units).short_gather_tiles(n_pairs) && ctx->opt_variant >= 7) return 2;
  const int candidates[4] = {8, 4, 2, 1};   // measured (profiles/r01_c_tile_sweep.txt): 8 rows is at or near the optimum on every level
  // The tallest tile that still yields this many workgroups.  Fewer, taller tiles also mean fewer partial rows for the
  // bookkeeping kernel, which matters most when there are few pairs (whole-match timings: profiles/r01_f_tile_heuristic.txt).
  const size_t enough = ctx->opt_min_workgroups > 0 ? size_t(ctx->opt_min_workgroups) : size_t(BatchPolicy(ctx->compute_units).min_workgroups(n_pairs));
  for (int r : candidates) {
    int tx, ty;
    level_tiles(cam->w[level], cam->h[level], r, level_is_linear(ctx, cam->w[level]), &tx, &ty);
    if (size_t(tx) * ty * n_pairs >= enough) return r;
  }
  return 1;
}

// (whatever the schedule variant of the moment: a frame outlives option changes)
static bool width_may_use_window(int w) { return w % kTileW == 0 || fast_sweep_takes_width(w); }
// (... or the small-level sweep: both read plane C)
static bool level_may_read_plane_c(int w, int h) { return width_may_use_window(w) || small_sweep_takes(w, h); }

// device layout of a frame: [raw staging][per level: I Z A B R][sel counts]
int frame_alloc(dvo_hip_context* ctx, int w, int h, const float K[4], int levels, dvo_hip_frame** out, size_t* raw_off) {
  if (!ctx) return DVO_HIP_ERR_INVALID;
  if (w < 4 || h < 4 || levels < 1 || levels > kMaxLevels || (w >> (levels - 1)) < 2 || (h >> (levels - 1)) < 2)
    return fail(ctx, DVO_HIP_ERR_INVALID, "frame_create: bad width/height/levels");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const CameraGeom* cam = nullptr;
  int rc = get_camera(ctx, w, h, K, levels, &cam);
  if (rc != DVO_HIP_OK) return rc;
  dvo_hip_frame* f = new dvo_hip_frame();
  f->levels = levels;
  f->cam = cam;
  size_t total = align_up(size_t(w) * h * 3, 256);   // u8 grey + u16 depth staging
  *raw_off = 0;
  size_t offs[kMaxLevels][6];
  for (int l = 0; l < levels; ++l) {
    const size_t n = size_t(cam->w[l]) * cam->h[l];
    // (C = {I, Z} of a current frame, the plane the window sweep stages in LDS: levels that sweep can handle)
    const size_t sz[6] = {n * 4, n * 4, n * 16, n * 8, n * 8, level_may_read_plane_c(cam->w[l], cam->h[l]) ? n * 8 : 0};
    for (int k = 0; k < 6; ++k) {
      offs[l][k] = total;
      total += align_up(sz[k], 256);
    }
  }
  const size_t cnt_off = total;
  total += 256;
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < ctx->frame_pool.size(); ++k)
    if (ctx->frame_pool[k].bytes == total) {                 // a block of a destroyed frame of this very layout
      f->pool.p = ctx->frame_pool[k].p;
      f->pool.bytes = total;
      ctx->frame_pool_bytes -= total;
      ctx->frame_pool.erase(ctx->frame_pool.begin() + long(k));
      break;
    }
  if (!f->pool.p) e = f->pool.reserve(total);
  if (e != hipSuccess) {
    delete f;
    ctx->err = std::string("hipMalloc(frame): ") + hipGetErrorString(e);
    return DVO_HIP_ERR_HIP;
  }
  char* base = f->pool.as<char>();
  for (int l = 0; l < levels; ++l) {
    FrameLevel& L = f->lv[l];
    L.w = cam->w[l]; L.h = cam->h[l];
    L.I = reinterpret_cast<float*>(base + offs[l][0]);
    L.Z = reinterpret_cast<float*>(base + offs[l][1]);
    L.A = reinterpret_cast<float4*>(base + offs[l][2]);
    L.B = reinterpret_cast<float2*>(base + offs[l][3]);
    L.R = reinterpret_cast<float2*>(base + offs[l][4]);
    L.C = level_may_read_plane_c(cam->w[l], cam->h[l]) ? reinterpret_cast<float2*>(base + offs[l][5]) : nullptr;
  }
  f->sel_count = reinterpret_cast<int*>(base + cnt_off);
  *out = f;
  return DVO_HIP_OK;
}

void fill_build_ptrs(dvo_hip_frame* f, FrameBuildPtrs& p) {
  p.grey = nullptr;
  p.raw = nullptr;
  p.keep_grey = nullptr;
  p.keep_raw = nullptr;
  for (int l = 0; l < f->levels; ++l) {
    p.I[l] = f->lv[l].I; p.Z[l] = f->lv[l].Z; p.A[l] = f->lv[l].A; p.B[l] = f->lv[l].B; p.R[l] = f->lv[l].R; p.C[l] = f->lv[l].C;
  }
  for (int l = f->levels; l < kMaxLevels; ++l) p.C[l] = nullptr;
  p.sel_count = f->sel_count;
  p.colour = nullptr;
  p.colour_pitch = 0;
  p.colour_format = 0;
  p.depth_f32 = nullptr;
  p.depth_pitch = 0;
  p.keep_planes = 0;
}

// the frame's own staging area: [u16 depth][u8 grey], see frame_alloc
uint16_t* staging_depth(dvo_hip_frame* f) { return f->pool.as<uint16_t>(); }
uint8_t* staging_grey(dvo_hip_frame* f) { return f->pool.as<uint8_t>() + size_t(f->lv[0].w) * f->lv[0].h * 2; }

bool aligned_to(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// RgbdImagePyramid::build (rgbd_image.cpp:156-172) for n frames of one camera.  From float planes (src == null: level 0 is
// already in place): the pyr-down chain, one launch per level for the whole batch; derived planes are built lazily per role
// (ensure_roles), like the reference's buildAccelerationStructure / PointSelection caches.  From raw planes: one fused pass
// (k_build_from_raw) that also writes level 0 in role `role` (-1: not known yet, 0: current, 1: reference with the given
// thresholds) and leaves a copy of the raw planes in the frame unless the current-role planes make it redundant.
// flavours of the current role a consumer of `n_frames` freshly built frames will most likely ask for at `level`: where the window
// sweep handles the level, a batch too large for the resident kernel only ever reads the 8-byte plane C (a third of the bytes to
// write); a small one may run the level resident (taps A + B) or on the launch path (C): both.  Whatever is missing at match time is
// derived then (ensure_roles).
int eager_current_flavor(const dvo_hip_context* ctx, const CameraGeom* cam, int level, int n_frames) {
  // a small level (align_small.hip reads plane C): a batch that may still run this level in the resident kernel (the gathered taps) gets
  // both flavours -- 38 KB and 115 KB per frame at 80 x 60 -- a larger one plane C alone
  if (level_uses_small(ctx, cam->w[level], cam->h[level]))
    return BatchPolicy(ctx->compute_units).resident_first_level_fits(n_frames) ? (kCurAB | kCurC) : kCurC;
  if (!level_uses_window(ctx, cam->w[level], cam->h[level])) return kCurAB;
  // (round 5: from an eighth as many frames as compute units on, plane C alone -- the taps cost three times the bytes to write, and a
  // streaming step of 32 / 48 / 64 pairs that re-ingests them every step is 0.885 / 0.98 / 1.24 -> 0.783 / 0.93 / 1.09 ms without them and
  // with the first level alone resident: plan_resident looks at what the frames hold)
  return BatchPolicy(ctx->compute_units).ingest_skips_taps(n_frames) ? kCurC : (kCurAB | kCurC);
}

// The rectify pass of n frames that carry a lens (the same one: check_source), on the build stream: the caller's planes `src` through the
// lens into each frame's own float planes I / Z of level 0, depth conversion included (lens.h, rectify.hip).  What follows in
// frames_build is the float ingest of those planes, read where they lie: no staging, nothing the context owns but the pointer table.
int rectify_frames(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& src) {
  const CameraGeom* cam = frames[0]->cam;
  const dvo_hip_lens& lens = frames[0]->lens;
  const bool image_f32 = src.format == DVO_HIP_PIXEL_F32, depth_f32 = src.depth_format == DVO_HIP_DEPTH_F32;
  std::vector<RectifyPtrs> host(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) host[i] = RectifyPtrs{src.planes[i], src.depth[i], frames[i]->lv[0].I, frames[i]->lv[0].Z};
  RectifyArgs a;
  a.map = lens_prepare(cam->K0, lens.K_raw, lens.D);
  a.w = cam->w[0];
  a.h = cam->h[0];
  a.image_pitch = int(src.pitch);
  a.depth_pitch = depth_f32 ? int(src.depth_pitch) : cam->w[0] * 2;   // (u16 depth planes are tight)
  a.red_first = pixel_red_first(src.format) ? 1 : 0;
  a.rectify_depth = lens.rectify_depth;
  a.depth_scale = src.depth_scale;
  const size_t bytes = host.size() * sizeof(RectifyPtrs);
  DVO_HIP_TRY(ctx, ctx->lens_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->build_stream, ctx->lens_tbl.p, host.data(), bytes));
  launch_rectify(ctx->build_stream, ctx->lens_tbl.as<RectifyPtrs>(), n, a, image_f32 ? kChF32 : pixel_channels(src.format), depth_f32,
                 ctx->opt_build_workgroups, ctx->opt_stream_policy != 0);
  DVO_HIP_TRY(ctx, hipGetLastError());
  return DVO_HIP_OK;
}

// The register pass of n frames that carry a depth rig (the same one: check_source), on the build stream: the depth sensor's planes of
// `src` through the rig into each frame's own float plane Z of level 0, depth conversion included (depth_rig.h, depth_register.hip): a
// fill with the hole pattern, then the scatter.  What follows in frames_build reads Z where it lies as float depth of scale 1.
int register_frames(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& src) {
  const CameraGeom* cam = frames[0]->cam;
  const bool depth_f32 = src.depth_format == DVO_HIP_DEPTH_F32;
  std::vector<DepthRigPtrs> host(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) host[i] = DepthRigPtrs{src.depth[i], frames[i]->lv[0].Z};
  DepthRigArgs a;
  a.map = depth_rig_prepare(cam->K0, frames[0]->rig);
  a.w = cam->w[0];
  a.h = cam->h[0];
  a.depth_pitch = depth_f32 ? int(src.depth_pitch) : cam->w[0] * 2;   // (u16 depth planes are tight)
  a.depth_scale = src.depth_scale;
  const size_t bytes = host.size() * sizeof(DepthRigPtrs);
  DVO_HIP_TRY(ctx, ctx->rig_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->build_stream, ctx->rig_tbl.p, host.data(), bytes));
  launch_depth_register(ctx->build_stream, ctx->rig_tbl.as<DepthRigPtrs>(), n, a, depth_f32, ctx->opt_build_workgroups, ctx->opt_stream_policy != 0);
  DVO_HIP_TRY(ctx, hipGetLastError());
  return DVO_HIP_OK;
}

// The sensor-format pass of n frames fed a Bayer mosaic or a YUV 4:2:2 plane (sensor_formats.h, sensor_convert.hip), on the build stream:
// the caller's planes -> the 8-bit grey of their BGR8 image in each frame's own u8 staging plane (staging_grey: no steady-state call
// allocates; nothing the context owns but the pointer table).  What follows in frames_build reads a tight grey8 source at that address.
int sensor_frames(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& src) {
  const CameraGeom* cam = frames[0]->cam;
  std::vector<SensorPtrs> host(static_cast<size_t>(n));
  SensorArgs a;
  a.w = cam->w[0];
  a.h = cam->h[0];
  a.pitch = int(src.pitch);
  a.format = src.format;
  a.src_dwords = 1;
  a.dst_wide = a.w % 4 == 0 ? 1 : 0;
  for (int i = 0; i < n; ++i) {
    host[size_t(i)] = SensorPtrs{static_cast<const uint8_t*>(src.planes[i]), staging_grey(frames[i])};
    if (!sensor_src_dwords(src.planes[i], src.pitch)) a.src_dwords = 0;
    if (!aligned_to(staging_grey(frames[i]), 4)) a.dst_wide = 0;
  }
  const size_t bytes = host.size() * sizeof(SensorPtrs);
  DVO_HIP_TRY(ctx, ctx->sensor_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->build_stream, ctx->sensor_tbl.p, host.data(), bytes));
  launch_sensor_convert(ctx->build_stream, ctx->sensor_tbl.as<SensorPtrs>(), n, a, /*packed=*/false, ctx->opt_build_workgroups, ctx->opt_stream_policy != 0);
  DVO_HIP_TRY(ctx, hipGetLastError());
  return DVO_HIP_OK;
}

// src: device planes whose pitch is resolved, of frames that share camera and levels (check_ingest has seen to both).  From a colour
// source the kernels convert and leave grey in the frames' raw copies.
int frames_build(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource* src, int role = -1, float ithr = 0.0f,
                 float dthr = 0.0f, bool keep_raw_copy = true) {
  Range range("build");
  const CameraGeom* cam = frames[0]->cam;
  const int levels = frames[0]->levels;
  // Frames that carry a lens: the caller's planes are rectified into the frames' float planes of level 0 (depth scaled there), and the
  // ingest below is the float ingest of THOSE planes, in place -- the frame ends as a lens-less frame fed the rectified pair would.
  // Frames that carry a depth rig: the depth sensor's plane is registered into the frames' float plane Z of level 0 first (depth scaled
  // there), and everything below -- the lens pass, the ingest -- takes the caller's image plane in its own format with float depth of
  // scale 1 read from THAT plane, in place: the frame ends as a rig-less frame fed the image and the registered plane would.  Under a
  // lens (rectify_depth 0: dvo_hip_frames_set_depth_rig) each lane of k_rectify reads and writes only its own element of Z.
  // Without a lens the ingest keeps its planes (keep_planes 1) and so stores Z back into the plane it reads, while other waves still
  // read their halo rows from it.  That is harmless only because the conversion is the identity here -- float depth of scale 1, z * 1.0f,
  // keeps every bit pattern, a NaN's payload included (kDepthRigHole is a quiet NaN) -- so a halo read sees the same bits before and
  // after a neighbour's store.  A conversion that changes any bit would need keep_planes 0 for Z, as under a lens.
  // Frames fed a sensor format (a Bayer mosaic, YUV 4:2:2): the caller's plane is converted into the frames' own u8 staging plane first,
  // and everything below -- the rig pass, the lens pass, the ingest -- takes a tight grey8 source at that address with the caller's depth:
  // the frame ends as one fed the grey of the format's BGR8 image through the grey entry points would.  The raw-copy bookkeeping below
  // needs no case of its own.  With u16 depth the source is not "in place" (the depth plane is the caller's), so an ingest that keeps a
  // copy gets keep_grey = the staging plane it reads and keep_raw beside it: every lane stores the grey bytes it loaded back where it
  // loaded them from, while other waves read their halo rows there -- harmless for the reason given for the rig's plane Z below, the
  // store changes no bit -- and the copy is complete (raw_copy true).  An ingest that keeps none leaves raw_copy false, whatever the
  // staging plane holds.  With float depth the copy is the float planes (keep_planes), as for any grey8 + float-depth ingest.
  const bool sensor = src != nullptr && sensor_bytes(src->format) != 0;
  std::vector<const void*> grey_planes;
  IngestSource converted;
  if (sensor) {
    const int rc = sensor_frames(ctx, n, frames, *src);
    if (rc != DVO_HIP_OK) return rc;
    grey_planes.resize(size_t(n));
    for (int i = 0; i < n; ++i) grey_planes[size_t(i)] = staging_grey(frames[i]);
    converted = IngestSource{grey_planes.data(), 0, size_t(cam->w[0]), src->depth, src->depth_scale, src->depth_format, src->depth_pitch};
    src = &converted;
  }
  const bool rig = src != nullptr && frames[0]->rig_on;
  std::vector<const void*> reg_planes;
  IngestSource registered;
  if (rig) {
    const int rc = register_frames(ctx, n, frames, *src);
    if (rc != DVO_HIP_OK) return rc;
    reg_planes.resize(size_t(n));
    for (int i = 0; i < n; ++i) reg_planes[size_t(i)] = frames[i]->lv[0].Z;
    registered = IngestSource{src->planes, src->format, src->pitch, reg_planes.data(), 1.0f, DVO_HIP_DEPTH_F32, size_t(cam->w[0]) * 4};
    src = &registered;
  }
  const bool lens = src != nullptr && frames[0]->lens_on;
  std::vector<const void*> rect_planes;
  IngestSource rectified;
  if (lens) {
    const int rc = rectify_frames(ctx, n, frames, *src);
    if (rc != DVO_HIP_OK) return rc;
    rect_planes.resize(2 * size_t(n));
    for (int i = 0; i < n; ++i) {
      rect_planes[size_t(i)] = frames[i]->lv[0].I;
      rect_planes[size_t(n) + i] = frames[i]->lv[0].Z;
    }
    const size_t row = size_t(cam->w[0]) * 4;
    rectified = IngestSource{rect_planes.data(), DVO_HIP_PIXEL_F32, row, rect_planes.data() + n, 1.0f, DVO_HIP_DEPTH_F32, row};
    src = &rectified;
  }
  std::vector<FrameBuildPtrs> host(n);
  bool wide = cam->w[0] % 4 == 0;
  const bool from_raw = src != nullptr;
  const bool image_f32 = from_raw && src->format == DVO_HIP_PIXEL_F32;
  const bool depth_f32 = from_raw && src->depth_format == DVO_HIP_DEPTH_F32;
  const bool colour = from_raw && src->format != 0 && !image_f32;
  const int channels = image_f32 ? kChF32 : colour ? pixel_channels(src->format) : 0;   // (the kernels' CH)
  if (image_f32) wide = cam->w[0] % 2 == 0;
  const float depth_scale = from_raw ? src->depth_scale : 0.0f;
  const int flavor0 = eager_current_flavor(ctx, cam, 0, n);
  for (int i = 0; i < n; ++i) {
    dvo_hip_frame* f = frames[i];
    fill_build_ptrs(f, host[i]);
    for (int l = 0; l < levels; ++l) {   // new pixels: every cached role plane is stale (PointSelection::setRgbdImagePyramid)
      f->lv[l].cur_have = 0;
      f->lv[l].selected = false;
      f->lv[l].explicit_sel = false;
      f->lv[l].q3 = false;
    }
    f->raw0 = from_raw;
    f->raw_copy = false;
    f->depth_scale = depth_scale;
    if (!from_raw) continue;
    if (role == 0) f->lv[0].cur_have = flavor0;
    if (role == 1) mark_selected(f->lv[0], ithr, dthr);
    if (colour || image_f32) {
      host[i].colour = static_cast<const uint8_t*>(src->planes[i]);
      host[i].colour_pitch = int(src->pitch);
      host[i].colour_format = src->format;
    } else {
      host[i].grey = static_cast<const uint8_t*>(src->planes[i]);
      host[i].colour_pitch = int(src->pitch);   // (read with float depth only: the u16 entry points take tight grey planes)
    }
    if (depth_f32) {
      // Float depth: the frame's raw copy is its float planes I / Z of level 0 -- the state of a frame created from float planes
      // (raw0 false), so another role, a reselection and a download derive from them like there.  Without a copy the frame is a
      // raw-ingested one that has nothing but the role planes just written.
      host[i].depth_f32 = static_cast<const float*>(src->depth[i]);
      host[i].depth_pitch = int(src->depth_pitch);
      if (role < 0 || (role == 1 && keep_raw_copy)) {
        host[i].keep_planes = lens ? 0 : 1;                    // (rectified planes already lie where the copy goes: nothing is written twice)
        f->raw0 = false;
      }
      wide = wide && f32_strips_aligned(host[i].depth_f32, src->depth_pitch) &&
             (image_f32 ? f32_strips_aligned(host[i].colour, src->pitch)
                        : colour ? colour_strips_aligned(host[i].colour, src->pitch, channels) : aligned_to(host[i].grey, 2) && src->pitch % 2 == 0);
      continue;
    }
    host[i].raw = static_cast<const uint16_t*>(src->depth[i]);
    const bool in_place = !colour && host[i].raw == staging_depth(f) && host[i].grey == staging_grey(f);
    if (in_place) {
      f->raw_copy = true;
    } else if (role < 0 || (role == 1 && keep_raw_copy)) {
      host[i].keep_grey = staging_grey(f);
      host[i].keep_raw = staging_depth(f);
      f->raw_copy = true;
    }
    wide = wide && (colour ? colour_strips_aligned(host[i].colour, src->pitch, channels) : aligned_to(host[i].grey, 4)) &&
           aligned_to(host[i].raw, 8) && aligned_to(staging_grey(f), 4);
  }
  hipStream_t bs = ctx->build_stream;
  // (one of a few buffers: the one that already holds this very table -- a streaming caller re-ingests the same frame sets from the same
  // planes step after step -- else the next in turn)
  int slot = ctx->tables.holder(ctx->build_tbl, dvo_hip_context::kTableSlots, bs, host.data(), size_t(n) * sizeof(FrameBuildPtrs));
  if (slot < 0) slot = int(ctx->build_tbl_next++ % dvo_hip_context::kTableSlots);
  DevBuf& build_tbl = ctx->build_tbl[slot];
  DVO_HIP_TRY(ctx, build_tbl.reserve(size_t(n) * sizeof(FrameBuildPtrs)));
  DVO_HIP_TRY(ctx, ctx->tables.upload(bs, build_tbl.p, host.data(), size_t(n) * sizeof(FrameBuildPtrs)));
  const FrameBuildPtrs* tbl = build_tbl.as<FrameBuildPtrs>();
  ctx->build_tbl_frames.assign(frames, frames + n);
  ctx->build_tbl_cur = &build_tbl;
  int built = 1;                                       // float ingest: level 0 is already in place
  if (from_raw) {
    // current frames: the {I, Z} plane of the pyramid levels the window sweep will read comes out of the same pass (no neighbours
    // needed), where the strip ingest runs (ingest_strips.hip)
    built = levels < 4 ? levels : 4;
    int c_levels = 0;
    const bool strips = ingest_strips_supports(cam->w[0], wide, image_f32);
    if (role == 0 && strips) {
      for (int l = 1; l < built; ++l)
        if (eager_current_flavor(ctx, cam, l, n) & kCurC) c_levels |= 1 << l;
      for (int i = 0; i < n; ++i)
        for (int l = 1; l < built; ++l)
          if ((c_levels >> l & 1) && frames[i]->lv[l].C) frames[i]->lv[l].cur_have |= kCurC;
    }
    launch_build_from_raw(bs, tbl, n, depth_scale, cam->w[0], cam->h[0], levels, role, strips, ithr, dthr, ctx->opt_build_workgroups, flavor0, c_levels,
                          channels, ctx->opt_stream_policy != 0, depth_f32);
    if (role == 1) {
      const int rc = apply_selection(ctx, bs, n, frames, 0, 0, ctx->opt_build_workgroups);
      if (rc != DVO_HIP_OK) return rc;
    }
    if (strips) ctx->strip_ingests += n;
    if (colour) ctx->colour_ingests += n;
    if (sensor) ctx->sensor_ingests += n;
    if (depth_f32) ctx->f32_ingests += n;
    if (lens) ctx->lens_ingests += n;
    if (rig) ctx->depth_registrations += n;
  }
  for (int l = built; l < levels; ++l) launch_pyr_down(bs, tbl, n, l, cam->w[l - 1], cam->h[l - 1]);
  DVO_HIP_TRY(ctx, hipGetLastError());
  return stamp_build(ctx, n, frames);
}

// Build the missing role planes of a set of frames for levels [l0, l1]: role 0 = current (flavours `cur_want[level]`, kCurAB | kCurC;
// null: the taps A + B), role 1 = reference (R + selection count for the given thresholds).  One launch per level (and source) for
// all frames that need it.
// `eager`: on the build stream (dvo_hip_frames_prepare), otherwise on the main stream right before the planes are used.
int ensure_roles(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, int role, int l0, int l1, float ithr, float dthr, bool eager = false,
                 const int* cur_want = nullptr) {
  const CameraGeom* cam = frames[0]->cam;
  const size_t slice = size_t(n) * sizeof(FrameBuildPtrs);
  DevBuf& table = eager ? (role == 0 ? ctx->prep_tbl_cur : ctx->prep_tbl_ref) : (role == 0 ? ctx->role_tbl_cur : ctx->role_tbl_ref);
  hipStream_t stream = eager ? ctx->build_stream : ctx->stream;
  const int cap = eager ? ctx->opt_build_workgroups : 0;   // planes needed right now are built at full width
  const bool stream_nt = eager && ctx->opt_stream_policy != 0;
  // What frame f lacks at level l.  Current role: `miss` = the flavours wanted there (plane C only where the camera's frames have one)
  // that the frame does not hold; reference role: whether its selection stands for these thresholds (miss 0).
  struct Lack { int miss; bool need; };
  auto lack_of = [&](const dvo_hip_frame* f, int l) -> Lack {
    const FrameLevel& L = f->lv[l];
    if (role != 0) return Lack{0, !ref_ready(L, ithr, dthr)};
    const int want = (cur_want ? cur_want[l] : kCurAB) & (L.C ? (kCurAB | kCurC) : kCurAB);
    return Lack{want & ~L.cur_have, (want & ~L.cur_have) != 0};
  };
  // Every frame is checked before the state of any is touched: a frame ingested straight into a role without a copy of its raw planes
  // (option "keep_raw_copy" 0) has nothing its level 0 could be derived from in another role, and the marks below -- planes "built" --
  // are set while the launches are still being gathered (round-5 advisor finding: the error used to leave earlier frames of the list
  // marked as built without their launches, and a retry aligned against stale planes).
  if (l0 == 0)
    for (int i = 0; i < n; ++i) {
      const dvo_hip_frame* f = frames[i];
      if (!f->raw0 || f->lv[0].cur_have != 0 || f->raw_copy) continue;
      if (lack_of(f, 0).need) return fail(ctx, DVO_HIP_ERR_INVALID, "frame has neither sampling planes nor a raw copy at level 0");
    }
  bool launched = false;
  int uploads = 0;                                           // table slices used so far (each launch reads its own)
  auto upload = [&](const std::vector<FrameBuildPtrs>& host, const FrameBuildPtrs** tbl, bool plane_pointers_only = true) -> int {
    if (plane_pointers_only && eager && ctx->build_tbl_cur && int(host.size()) == n && ctx->build_tbl_frames.size() == size_t(n) &&
        std::equal(frames, frames + n, ctx->build_tbl_frames.begin())) {
      *tbl = ctx->build_tbl_cur->as<FrameBuildPtrs>();      // the ingest of these very frames left their table on this stream
      return DVO_HIP_OK;
    }
    constexpr int kSlices = 4 * kMaxLevels;
    if (uploads == kSlices) {                                // (never in practice: a slice per level and source)
      DVO_HIP_TRY(ctx, hipStreamSynchronize(stream));
      uploads = 0;
    }
    DVO_HIP_TRY(ctx, table.reserve(slice * kSlices));
    FrameBuildPtrs* up = reinterpret_cast<FrameBuildPtrs*>(table.as<char>() + slice * uploads++);
    DVO_HIP_TRY(ctx, ctx->tables.upload(stream, up, host.data(), host.size() * sizeof(FrameBuildPtrs)));
    *tbl = up;
    return DVO_HIP_OK;
  };
  // Several levels, every frame missing the same planes on each of them, all to be derived from the float planes I / Z (a camera
  // frame that has just been built): ONE launch for all levels (k_derive_levels) instead of a table upload, a counter reset and a
  // launch per level.
  if (l1 > l0) {
    LevelSpan span = level_span(l0, l1, cam->w, cam->h);
    bool uniform = n <= 64;                                                             // (the check below is quadratic; large batches come through the ingest.
    // Round 6: the size test used to FOLLOW the double loop -- 524 288 comparisons per role of a 1024-pair batch, 0.4 ms of the host
    // thread in front of every streaming step's first launch)
    for (int i = 0; i < n && uniform; ++i)
      for (int j = 0; j < i && uniform; ++j) uniform = frames[i] != frames[j];        // (a frame listed twice: the general path skips its second visit)
    for (int l = l0; l <= l1 && uniform; ++l) {
      int miss_all = -1;
      for (int i = 0; i < n && uniform; ++i) {
        const dvo_hip_frame* f = frames[i];
        const Lack lack = lack_of(f, l);
        uniform = lack.need && !(l == 0 && f->raw0) && (role == 1 || f->lv[l].cur_have == 0) && (miss_all < 0 || lack.miss == miss_all);
        miss_all = lack.miss;
      }
      span.flavor[l] = miss_all;
    }
    if (uniform) {
      std::vector<FrameBuildPtrs> host(n);
      for (int i = 0; i < n; ++i) fill_build_ptrs(frames[i], host[i]);
      const FrameBuildPtrs* tbl = nullptr;
      const int rc = upload(host, &tbl);
      if (rc != DVO_HIP_OK) return rc;
      launch_derive_levels(stream, tbl, n, span, role, ithr, dthr, cap);
      for (int i = 0; i < n; ++i)
        for (int l = l0; l <= l1; ++l) {
          FrameLevel& L = frames[i]->lv[l];
          if (role == 0) L.cur_have |= span.flavor[l];
          else mark_selected(L, ithr, dthr);
        }
      if (role == 1) {
        const int rc = apply_selection(ctx, stream, n, frames, l0, l1, cap);
        if (rc != DVO_HIP_OK) return rc;
      }
      if (eager) {
        const int rc2 = stamp_build(ctx, n, frames);
        if (rc2 != DVO_HIP_OK) return rc2;
      }
      DVO_HIP_TRY(ctx, hipGetLastError());
      return DVO_HIP_OK;
    }
  }
  for (int l = l0; l <= l1; ++l) {
    // sources, per frame: float planes I / Z (levels >= 1, and level 0 of frames created from float planes); at level 0 of a frame
    // ingested from raw planes: the other flavour of the current role, else the frame's copy of its raw planes
    std::vector<FrameBuildPtrs> from_planes[4], from_raw[4], ab_from_c, c_from_a, ref_from_c;
    std::vector<dvo_hip_frame*> ref_from_ab, selected;
    float raw_scale = 0.0f;
    bool deferred = false;                                   // frames of another depth scale than the launch gathered so far
    for (int i = 0; i < n; ++i) {
      dvo_hip_frame* f = frames[i];
      FrameLevel& L = f->lv[l];
      const Lack lack = lack_of(f, l);
      const int miss = lack.miss;
      if (!lack.need) continue;   // also skips the second visit of a frame that is listed twice
      FrameBuildPtrs p;
      fill_build_ptrs(f, p);
      if (l == 0 && f->raw0) {
        if (role == 0 && (L.cur_have & kCurC)) {
          ab_from_c.push_back(p);
        } else if (role == 0 && (L.cur_have & kCurAB)) {
          c_from_a.push_back(p);
        } else if (role == 1 && (L.cur_have & kCurAB)) {
          ref_from_ab.push_back(f);
        } else if (role == 1 && (L.cur_have & kCurC)) {
          ref_from_c.push_back(p);
        } else if (f->raw_copy && (raw_scale == 0.0f || f->depth_scale == raw_scale)) {
          raw_scale = f->depth_scale;
          p.grey = staging_grey(f);
          p.raw = staging_depth(f);
          from_raw[miss].push_back(p);
        } else if (f->raw_copy) {
          deferred = true;     // another depth scale than the frames gathered so far: picked up by the pass below
          continue;
        } else {
          return fail(ctx, DVO_HIP_ERR_INVALID, "frame has neither sampling planes nor a raw copy at level 0");
        }
      } else {
        from_planes[miss].push_back(p);
      }
      if (role == 0) {
        L.cur_have |= miss;
      } else {
        mark_selected(L, ithr, dthr);
        selected.push_back(f);
      }
    }
    const FrameBuildPtrs* tbl = nullptr;
    for (int miss = 0; miss < 4; ++miss) {
      if (!from_planes[miss].empty()) {
        int rc = upload(from_planes[miss], &tbl);
        if (rc != DVO_HIP_OK) return rc;
        if (role == 0) launch_derive_current(stream, tbl, int(from_planes[miss].size()), l, cam->w[l], cam->h[l], cap, miss, stream_nt);
        else launch_derive_reference(stream, tbl, int(from_planes[miss].size()), l, cam->w[l], cam->h[l], ithr, dthr, cap, stream_nt);
        launched = true;
      }
      if (!from_raw[miss].empty()) {
        int rc = upload(from_raw[miss], &tbl, /*plane_pointers_only=*/false);
        if (rc != DVO_HIP_OK) return rc;
        launch_build_from_raw(stream, tbl, int(from_raw[miss].size()), raw_scale, cam->w[0], cam->h[0], /*levels=*/1, role,
                              ingest_strips_supports(cam->w[0], /*wide=*/true), ithr, dthr, cap, miss, 0, 0, stream_nt);
        launched = true;
      }
    }
    const struct { std::vector<FrameBuildPtrs>* list; int mode; } conversions[3] = {{&ab_from_c, 0}, {&c_from_a, 1}, {&ref_from_c, 2}};
    for (const auto& c : conversions) {
      if (c.list->empty()) continue;
      int rc = upload(*c.list, &tbl);
      if (rc != DVO_HIP_OK) return rc;
      launch_from_current_plane(stream, tbl, int(c.list->size()), l, cam->w[l], cam->h[l], c.mode, ithr, dthr, cap);
      launched = true;
    }
    for (dvo_hip_frame* f : ref_from_ab) {   // PointSelection over a frame that has been a current frame so far
      FrameLevel& L = f->lv[0];
      DVO_HIP_TRY(ctx, hipMemsetAsync(f->sel_count, 0, sizeof(int), stream));
      launch_select_pack(stream, L.A, L.B, L.w * L.h, ithr, dthr, L.R, f->sel_count, nullptr);
      launched = true;
    }
    if (!selected.empty()) {
      const int rc = apply_selection(ctx, stream, int(selected.size()), selected.data(), l, l, cap);
      if (rc != DVO_HIP_OK) return rc;
    }
    if (deferred) {   // frames of a second depth scale (one kernel launch takes one scale): rare, one more pass each
      if (eager && launched) {
        const int rc = stamp_build(ctx, n, frames);
        if (rc != DVO_HIP_OK) return rc;
      }
      DVO_HIP_TRY(ctx, hipStreamSynchronize(stream));   // the table slices are reused
      return ensure_roles(ctx, n, frames, role, l0, l1, ithr, dthr, eager, cur_want);
    }
  }
  if (eager && launched) {
    const int rc = stamp_build(ctx, n, frames);
    if (rc != DVO_HIP_OK) return rc;
  }
  DVO_HIP_TRY(ctx, hipGetLastError());
  return DVO_HIP_OK;
}

