// capi_frames.inc -- cameras, frames and their planes: build tickets, the per-level geometry of a camera, frame allocation, the batched frame
// build in parts (frames_build: the ingest's pre-passes as a chain of stages, one frame's source and raw copy, the build table, the
// launches), and the role planes of a batch's frames (ensure_roles: one RoleBuild per pass).  Textually included by capi.hip inside its
// anonymous namespace (the context, the workspace and the error macros are defined there).
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

// the option values that bear on the choice of a level's sweep, as they stand now (sweep_choice.h; the Gram schedule of a batch or a repeat
// rewrites opt_variant for a while: a plan made then holds the choices of that schedule)
SweepOptions sweep_options(const dvo_hip_context* ctx) {
  return SweepOptions{ctx->opt_variant, ctx->opt_small_sweep, ctx->opt_ref_compat, ctx->opt_ref_order, ctx->opt_compact_residuals};
}

LevelGeom make_geom(const dvo_hip_context* ctx, const CameraGeom* cam, int level, int rows_per_wave, const SweepChoice& choice) {
  LevelGeom g;
  g.w = cam->w[level]; g.h = cam->h[level];
  g.fx = cam->K[level][0]; g.fy = cam->K[level][1]; g.ox = cam->K[level][2]; g.oy = cam->K[level][3];
  g.wi_x = 0.5f * g.fx / 255.0f; g.wi_y = 0.5f * g.fy / 255.0f;
  g.half_wi_x = 0.5f * g.wi_x; g.half_wi_y = 0.5f * g.wi_y; g.half_fx = 0.5f * g.fx; g.half_fy = 0.5f * g.fy;
  g.tx = cam->tx[level]; g.ty = cam->ty[level];
  g.level = level;
  g.pair_list = nullptr;
  g.skip_flags = nullptr;
  g.linear = choice.linear ? 1 : 0;
  level_tiles(g.w, g.h, rows_per_wave, g.linear != 0, &g.tiles_x, &g.tiles_y);
  g.rcp_table = ctx->opt_ref_compat ? ctx->rcp_table.as<float>() : nullptr;
  g.rcp_shift = ctx->rcp_shift;
  g.rcp_packed = ctx->opt_ref_compat == 1 ? ctx->rcp_packed : 0;   // (2: the table through memory, the path of a table that does not pack)
  // (not under "ref_compat": a run that is compared with the reference's own numbers keeps every low part -- round-5 advisor finding)
  // (variant 8 alone: operand store 2 of the contracted schedules, mode 2 = no "ref_compat")
  g.gram_hi_j = !ctx->opt_gram_lo_parts && !ctx->opt_deterministic && choice.mode == 2 && choice.operand_store == 2 && size_t(g.w) * g.h >= 150000 ? 1 : 0;
  g.small = choice.kernel == SweepKernel::Small ? 1 : 0;
  g.compact = choice.compact ? 1 : 0;
  return g;
}

// rows of 64 pixels each wavefront sweeps: large tiles amortise the 85-value wave reduction, small tiles
// keep all 256 CUs busy when the batch is small
int pick_rows_per_wave(const dvo_hip_context* ctx, const CameraGeom* cam, int level, int n_pairs, const SweepChoice& choice) {
  if (choice.tile_rows > 0) return choice.tile_rows;
  if (choice.kernel == SweepKernel::Small && ctx->opt_rows_per_wave == 0) {
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
  if (BatchPolicy(ctx->compute_units).short_gather_tiles(n_pairs) && choice.mode >= 1) return 2;
  const int candidates[4] = {8, 4, 2, 1};   // measured (profiles/r01_c_tile_sweep.txt): 8 rows is at or near the optimum on every level
  // The tallest tile that still yields this many workgroups.  Fewer, taller tiles also mean fewer partial rows for the
  // bookkeeping kernel, which matters most when there are few pairs (whole-match timings: profiles/r01_f_tile_heuristic.txt).
  const size_t enough = ctx->opt_min_workgroups > 0 ? size_t(ctx->opt_min_workgroups) : size_t(BatchPolicy(ctx->compute_units).min_workgroups(n_pairs));
  for (int r : candidates) {
    int tx, ty;
    level_tiles(cam->w[level], cam->h[level], r, choice.linear, &tx, &ty);
    if (size_t(tx) * ty * n_pairs >= enough) return r;
  }
  return 1;
}

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
    const size_t sz[6] = {n * 4, n * 4, n * 16, n * 8, n * 8, any_sweep_reads_plane_c(cam->w[l], cam->h[l]) ? n * 8 : 0};
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
    L.C = any_sweep_reads_plane_c(cam->w[l], cam->h[l]) ? reinterpret_cast<float2*>(base + offs[l][5]) : nullptr;
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

// flavours of the current role a consumer of `n_frames` freshly built frames will most likely ask for at `level`: where the window
// sweep handles the level, a batch too large for the resident kernel only ever reads the 8-byte plane C (a third of the bytes to
// write); a small one may run the level resident (taps A + B) or on the launch path (C): both.  Whatever is missing at match time is
// derived then (ensure_roles).
int eager_current_flavor(const dvo_hip_context* ctx, const CameraGeom* cam, int level, int n_frames) {
  const SweepChoice choice = choose_sweep(sweep_options(ctx), cam->w[level], cam->h[level]);   // (no plan at ingest time)
  if (!choice.reads_c) return kCurAB;
  // a small level (align_small.hip reads plane C): a batch that may still run this level in the resident kernel (the gathered taps) gets
  // both flavours -- 38 KB and 115 KB per frame at 80 x 60 -- a larger one plane C alone
  if (choice.kernel == SweepKernel::Small)
    return BatchPolicy(ctx->compute_units).resident_first_level_fits(n_frames) ? (kCurAB | kCurC) : kCurC;
  // (round 5: from an eighth as many frames as compute units on, plane C alone -- the taps cost three times the bytes to write, and a
  // streaming step of 32 / 48 / 64 pairs that re-ingests them every step is 0.885 / 0.98 / 1.24 -> 0.783 / 0.93 / 1.09 ms without them and
  // with the first level alone resident: plan_resident looks at what the frames hold)
  return BatchPolicy(ctx->compute_units).ingest_skips_taps(n_frames) ? kCurC : (kCurAB | kCurC);
}

// ---- the pre-passes of a raw ingest, as stages.  Each runs on the build stream in front of the ingest for frames that carry its
// property (the same for all n: check_source), reads the planes of the IngestSource it is given, writes into the frames' own memory and
// hands on the IngestSource the next stage -- or the ingest -- reads instead.  Nothing is launched or allocated for frames without the
// property; a stage owns nothing but its pointer table.

// the plane arrays a rewritten source points into; frames_build owns one for the duration of the call.  A stage fills its table from the
// source it was given BEFORE it rewrites an array here (that source may point into the same array)
struct StagePlanes { std::vector<const void*> image, depth; };

// the pointer table of a stage: room in the stage's buffer, the records uploaded on the build stream; returns the device address (null:
// DVO_HIP_ERR_HIP, the context holds the text)
template <typename T>
const T* stage_table(dvo_hip_context* ctx, DevBuf& buf, const std::vector<T>& host) {
  const size_t bytes = host.size() * sizeof(T);
  hipError_t e = buf.reserve(bytes);
  if (e == hipSuccess) e = ctx->tables.upload(ctx->build_stream, buf.p, host.data(), bytes);
  if (e != hipSuccess) ctx->err = std::string("stage table: ") + hipGetErrorString(e);
  return e == hipSuccess ? buf.as<T>() : nullptr;
}

typedef int IngestStage(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& in, StagePlanes& planes, IngestSource* out);

// Frames fed a sensor format (a Bayer mosaic, YUV 4:2:2; sensor_formats.h, sensor_convert.hip): the caller's planes -> the 8-bit grey of
// their BGR8 image in each frame's own u8 staging plane (staging_grey: no steady-state call allocates).  Hands on a tight grey8 source at
// that address with the caller's depth: the frame ends as one fed that grey through the grey entry points would.  The raw copy needs no
// case of its own (frame_source).  With u16 depth the source is not "in place" (the depth plane is the caller's), so an ingest that keeps
// a copy gets keep_grey = the staging plane it reads: every lane stores the grey bytes it loaded back where it loaded them from, while
// other waves read their halo rows there -- harmless for the reason given at the rig stage, the store changes no bit.
int sensor_stage(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& in, StagePlanes& planes, IngestSource* out) {
  const CameraGeom* cam = frames[0]->cam;
  std::vector<SensorPtrs> host(static_cast<size_t>(n));
  SensorArgs a;
  a.w = cam->w[0]; a.h = cam->h[0];
  a.pitch = int(in.pitch);
  a.format = in.format;
  a.src_dwords = 1;
  a.dst_wide = a.w % 4 == 0 ? 1 : 0;
  for (int i = 0; i < n; ++i) {
    host[size_t(i)] = SensorPtrs{static_cast<const uint8_t*>(in.planes[i]), staging_grey(frames[i])};
    if (!sensor_src_dwords(in.planes[i], in.pitch)) a.src_dwords = 0;
    if (!aligned_to(staging_grey(frames[i]), 4)) a.dst_wide = 0;
  }
  const SensorPtrs* tbl = stage_table(ctx, ctx->sensor_tbl, host);
  if (!tbl) return DVO_HIP_ERR_HIP;
  launch_sensor_convert(ctx->build_stream, tbl, n, a, /*packed=*/false, ctx->opt_build_workgroups, ctx->opt_stream_policy != 0);
  DVO_HIP_TRY(ctx, hipGetLastError());
  planes.image.resize(size_t(n));
  for (int i = 0; i < n; ++i) planes.image[size_t(i)] = staging_grey(frames[i]);
  *out = IngestSource{planes.image.data(), 0, size_t(cam->w[0]), in.depth, in.depth_scale, in.depth_format, in.depth_pitch};
  return DVO_HIP_OK;
}

// Frames that carry a depth rig (depth_rig.h, depth_register.hip): the depth sensor's planes through the rig into each frame's own float
// plane Z of level 0, depth conversion included: a fill with the hole pattern, then the scatter.  Hands on the caller's image in its own
// format with float depth of scale 1 read from THAT plane, in place: the frame ends as a rig-less frame fed the image and the registered
// plane would.  Without a lens the ingest keeps its planes (keep_planes 1) and so stores Z back into the plane it reads, while other
// waves still read their halo rows from it.  That is harmless only because the conversion is the identity here -- float depth of scale
// 1, z * 1.0f, keeps every bit pattern, a NaN's payload included (kDepthRigHole is a quiet NaN) -- so a halo read sees the same bits
// before and after a neighbour's store.  A conversion that changes any bit would need keep_planes 0 for Z, as under a lens.
int rig_stage(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& in, StagePlanes& planes, IngestSource* out) {
  const CameraGeom* cam = frames[0]->cam;
  const bool depth_f32 = in.depth_format == DVO_HIP_DEPTH_F32;
  std::vector<DepthRigPtrs> host(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) host[i] = DepthRigPtrs{in.depth[i], frames[i]->lv[0].Z};
  DepthRigArgs a;
  a.map = depth_rig_prepare(cam->K0, frames[0]->rig);
  a.w = cam->w[0]; a.h = cam->h[0];
  a.depth_pitch = depth_f32 ? int(in.depth_pitch) : cam->w[0] * 2;   // (u16 depth planes are tight)
  a.depth_scale = in.depth_scale;
  const DepthRigPtrs* tbl = stage_table(ctx, ctx->rig_tbl, host);
  if (!tbl) return DVO_HIP_ERR_HIP;
  launch_depth_register(ctx->build_stream, tbl, n, a, depth_f32, ctx->opt_build_workgroups, ctx->opt_stream_policy != 0);
  DVO_HIP_TRY(ctx, hipGetLastError());
  planes.depth.resize(size_t(n));
  for (int i = 0; i < n; ++i) planes.depth[size_t(i)] = frames[i]->lv[0].Z;
  *out = IngestSource{in.planes, in.format, in.pitch, planes.depth.data(), 1.0f, DVO_HIP_DEPTH_F32, size_t(cam->w[0]) * 4};
  return DVO_HIP_OK;
}

// Frames that carry a lens (lens.h, rectify.hip): the planes of `in` through the lens into each frame's own float planes I / Z of level
// 0, depth conversion included.  Hands on float image and float depth of scale 1 at those planes: the ingest is the float ingest of THOSE
// planes, read where they lie, and the frame ends as a lens-less frame fed the rectified pair would.  The rectified planes already lie
// where a raw copy goes, so the ingest runs with keep_planes 0 (frame_source): nothing is written twice, and no lane stores into a plane
// others still read.  Behind a rig (rectify_depth 0: dvo_hip_frames_set_depth_rig) each lane of k_rectify reads and writes only its own
// element of Z.
int lens_stage(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& in, StagePlanes& planes, IngestSource* out) {
  const CameraGeom* cam = frames[0]->cam;
  const dvo_hip_lens& lens = frames[0]->lens;
  const bool image_f32 = in.format == DVO_HIP_PIXEL_F32, depth_f32 = in.depth_format == DVO_HIP_DEPTH_F32;
  std::vector<RectifyPtrs> host(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) host[i] = RectifyPtrs{in.planes[i], in.depth[i], frames[i]->lv[0].I, frames[i]->lv[0].Z};
  RectifyArgs a;
  a.map = lens_prepare(cam->K0, lens.K_raw, lens.D);
  a.w = cam->w[0]; a.h = cam->h[0];
  a.image_pitch = int(in.pitch);
  a.depth_pitch = depth_f32 ? int(in.depth_pitch) : cam->w[0] * 2;   // (u16 depth planes are tight)
  a.red_first = pixel_red_first(in.format) ? 1 : 0;
  a.rectify_depth = lens.rectify_depth;
  a.depth_scale = in.depth_scale;
  const RectifyPtrs* tbl = stage_table(ctx, ctx->lens_tbl, host);
  if (!tbl) return DVO_HIP_ERR_HIP;
  launch_rectify(ctx->build_stream, tbl, n, a, image_f32 ? kChF32 : pixel_channels(in.format), depth_f32, ctx->opt_build_workgroups,
                 ctx->opt_stream_policy != 0);
  DVO_HIP_TRY(ctx, hipGetLastError());
  planes.image.resize(size_t(n));
  planes.depth.resize(size_t(n));
  for (int i = 0; i < n; ++i) {
    planes.image[size_t(i)] = frames[i]->lv[0].I;
    planes.depth[size_t(i)] = frames[i]->lv[0].Z;
  }
  const size_t row = size_t(cam->w[0]) * 4;
  *out = IngestSource{planes.image.data(), DVO_HIP_PIXEL_F32, row, planes.depth.data(), 1.0f, DVO_HIP_DEPTH_F32, row};
  return DVO_HIP_OK;
}

// Frames that carry a depth filter (depth_filter.h, depth_filter.hip): the depth planes of `in` -- the caller's, or behind a rig or a lens
// the frame's own float plane Z of level 0 -- through the filter into each frame's FILTER PLANE (dvo_hip_frame::filter_plane, allocated
// when the filter was set), depth conversion included.  The last stage: it filters in the frame's own raster.  Hands on the image of
// `in` unchanged with float depth of scale 1 at the filter plane: the frame ends as a filter-less frame (same lens, same rig) fed that
// image and the filtered plane would.  The pass is NEVER in place -- a stencil must not write what its neighbours still read -- so the
// filtered plane lies beside the frame's Z, and an ingest that keeps a copy runs with keep_planes 1 (frame_source) and stores it into
// Z.  That holds behind a lens too, where the image it reads is the frame's own plane I: each lane then stores the I it loaded back
// where it loaded it from, and the float conversion keeps every bit (see rig_stage), so a neighbour's halo read sees the same bits
// before and after.  Nothing but the filter pass and the ingest behind it ever reads or writes the filter plane.
int filter_stage(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource& in, StagePlanes& planes, IngestSource* out) {
  const CameraGeom* cam = frames[0]->cam;
  const bool depth_f32 = in.depth_format == DVO_HIP_DEPTH_F32;
  std::vector<DepthFilterPtrs> host(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) host[size_t(i)] = DepthFilterPtrs{in.depth[i], frames[i]->filter_plane.as<float>()};
  DepthFilterArgs a;
  a.P = depth_filter_prepare(frames[0]->filter);
  a.w = cam->w[0]; a.h = cam->h[0];
  a.depth_pitch = depth_f32 ? int(in.depth_pitch) : cam->w[0] * 2;   // (u16 depth planes are tight)
  a.depth_scale = in.depth_scale;
  const DepthFilterPtrs* tbl = stage_table(ctx, ctx->filter_tbl, host);
  if (!tbl) return DVO_HIP_ERR_HIP;
  launch_depth_filter(ctx->build_stream, tbl, n, a, depth_f32, ctx->opt_build_workgroups, ctx->opt_stream_policy != 0);
  DVO_HIP_TRY(ctx, hipGetLastError());
  planes.depth.resize(size_t(n));                            // (the table above was filled first: in.depth may be this very array)
  for (int i = 0; i < n; ++i) planes.depth[size_t(i)] = frames[i]->filter_plane.p;
  *out = IngestSource{in.planes, in.format, in.pitch, planes.depth.data(), 1.0f, DVO_HIP_DEPTH_F32, size_t(cam->w[0]) * 4};
  return DVO_HIP_OK;
}

// which stages a call runs (frames_build runs them in this order)
struct StagesRun { bool sensor, rig, lens, filter; };

// new pixels: every cached role plane of the frame is stale (PointSelection::setRgbdImagePyramid)
void invalidate_roles(dvo_hip_frame* f) {
  for (int l = 0; l < f->levels; ++l) f->lv[l].cur_have = 0;
  invalidate_reference_role(f);
}

// what the kernels of an ingest are templated on: the formats of the (staged) source, `channels` = the kernels' CH; all false / 0 without one
struct SourceKind { bool image_f32, depth_f32, colour; int channels; };
SourceKind source_kind(const IngestSource* src) {
  const bool image_f32 = src && src->format == DVO_HIP_PIXEL_F32, colour = src && src->format != 0 && !image_f32;
  return SourceKind{image_f32, src && src->depth_format == DVO_HIP_DEPTH_F32, colour, image_f32 ? kChF32 : colour ? pixel_channels(src->format) : 0};
}

// One frame of a build: its entry `p` of the build table -- where the kernel reads frame i of the (staged) source `src` and where it
// leaves a copy -- and, returned, what the frame then holds of its raw planes and its share of `wide` (every plane's address and pitch
// suit the strip ingest's loads).  Without a source (a frame created from float planes: level 0 is in place) nothing but the planes.
struct FrameSource { bool raw0, raw_copy, wide; };
FrameSource frame_source(dvo_hip_frame* f, const IngestSource* src, int i, const SourceKind& kind, int role, bool keep_raw_copy, bool lens, bool filter,
                         FrameBuildPtrs& p) {
  fill_build_ptrs(f, p);
  if (!src) return FrameSource{false, false, true};
  if (kind.colour || kind.image_f32) {
    p.colour = static_cast<const uint8_t*>(src->planes[i]);
    p.colour_format = src->format;
  } else {
    p.grey = static_cast<const uint8_t*>(src->planes[i]);
  }
  p.colour_pitch = int(src->pitch);   // (a grey plane's is read with float depth only: the u16 entry points take tight grey planes)
  if (kind.depth_f32) {
    p.depth_f32 = static_cast<const float*>(src->depth[i]);
    p.depth_pitch = int(src->depth_pitch);
  } else {
    p.raw = static_cast<const uint16_t*>(src->depth[i]);
  }
  // The raw copy -- what another role, a reselection and a download can later derive level 0 from -- in one statement of cases.  An
  // ingest without a role keeps one, one into the reference role unless told otherwise (option "keep_raw_copy" 0), one into the current
  // role never: its planes A + B hold everything.
  const bool keeps = role < 0 || (role == 1 && keep_raw_copy);
  const bool in_place = !kind.depth_f32 && !kind.colour && p.raw == staging_depth(f) && p.grey == staging_grey(f);
  FrameSource s{true, false, true};
  if (kind.depth_f32 && keeps) {
    // float depth: the copy is the frame's float planes I / Z of level 0 -- the state of a frame created from float planes (raw0 false).
    // Rectified planes (lens) already lie where the copy goes: nothing is written twice -- unless a filter stands behind the lens: the
    // filtered depth lies in the frame's filter plane, and the copy puts it into Z (filter_stage)
    p.keep_planes = lens && !filter ? 0 : 1;
    s.raw0 = false;
  } else if (in_place) {
    s.raw_copy = true;                 // u16 depth, read from the frame's own staging area: that IS the copy, whatever the role
  } else if (!kind.depth_f32 && keeps) {
    p.keep_grey = staging_grey(f);     // u16 depth from elsewhere: the kernel leaves grey and depth in the staging area
    p.keep_raw = staging_depth(f);
    s.raw_copy = true;
  }                                    // else none: a raw-ingested frame that has nothing but the role planes just written
  if (kind.depth_f32)
    s.wide = f32_strips_aligned(p.depth_f32, src->depth_pitch) &&
             (kind.image_f32 ? f32_strips_aligned(p.colour, src->pitch)
                             : kind.colour ? colour_strips_aligned(p.colour, src->pitch, kind.channels) : aligned_to(p.grey, 2) && src->pitch % 2 == 0);
  else
    s.wide = (kind.colour ? colour_strips_aligned(p.colour, src->pitch, kind.channels) : aligned_to(p.grey, 4)) && aligned_to(p.raw, 8) &&
             aligned_to(staging_grey(f), 4);
  return s;
}

// The build table of these n frames on the build stream: in one of a few buffers -- the one that already holds this very table (a
// streaming caller re-ingests the same frame sets from the same planes step after step), else the next in turn -- and remembered as
// the table of this frame list (ensure_roles reuses it for an eager prepare of the same list).
int upload_build_table(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const std::vector<FrameBuildPtrs>& host, const FrameBuildPtrs** tbl) {
  const size_t bytes = size_t(n) * sizeof(FrameBuildPtrs);
  int slot = ctx->tables.holder(ctx->build_tbl, dvo_hip_context::kTableSlots, ctx->build_stream, host.data(), bytes);
  if (slot < 0) slot = int(ctx->build_tbl_next++ % dvo_hip_context::kTableSlots);
  DevBuf& build_tbl = ctx->build_tbl[slot];
  DVO_HIP_TRY(ctx, build_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->build_stream, build_tbl.p, host.data(), bytes));
  *tbl = build_tbl.as<FrameBuildPtrs>();
  ctx->build_tbl_frames.assign(frames, frames + n);
  ctx->build_tbl_cur = &build_tbl;
  return DVO_HIP_OK;
}

// The launches of a raw ingest and its counters: level 0 in role `role` and the pyramid levels 1..3 in one pass, then the caller
// selection of reference frames.  Current frames: the {I, Z} plane C of the pyramid levels the window sweep will read comes out of the
// same pass (no neighbours needed), where the strip ingest runs (ingest_strips.hip).  *built: the levels the pass has written.
int launch_raw_ingest(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const FrameBuildPtrs* tbl, const SourceKind& kind, bool wide,
                      float depth_scale, int role, float ithr, float dthr, int flavor0, const StagesRun& ran, int* built) {
  const CameraGeom* cam = frames[0]->cam;
  const int levels = frames[0]->levels;
  *built = levels < 4 ? levels : 4;
  int c_levels = 0;
  const bool strips = ingest_strips_supports(cam->w[0], wide, kind.image_f32);
  if (role == 0 && strips) {
    for (int l = 1; l < *built; ++l)
      if (eager_current_flavor(ctx, cam, l, n) & kCurC) c_levels |= 1 << l;
    for (int i = 0; i < n; ++i)
      for (int l = 1; l < *built; ++l)
        if ((c_levels >> l & 1) && frames[i]->lv[l].C) frames[i]->lv[l].cur_have |= kCurC;
  }
  launch_build_from_raw(ctx->build_stream, tbl, n, depth_scale, cam->w[0], cam->h[0], levels, role, strips, ithr, dthr, ctx->opt_build_workgroups,
                        flavor0, c_levels, kind.channels, ctx->opt_stream_policy != 0, kind.depth_f32);
  if (role == 1) {
    const int rc = apply_selection(ctx, ctx->build_stream, n, frames, 0, 0, ctx->opt_build_workgroups);
    if (rc != DVO_HIP_OK) return rc;
  }
  if (strips) ctx->strip_ingests += n;
  if (kind.colour) ctx->colour_ingests += n;
  if (ran.sensor) ctx->sensor_ingests += n;
  if (kind.depth_f32) ctx->f32_ingests += n;
  if (ran.lens) ctx->lens_ingests += n;
  if (ran.rig) ctx->depth_registrations += n;
  if (ran.filter) ctx->depth_filter_ingests += n;
  return DVO_HIP_OK;
}

// RgbdImagePyramid::build (rgbd_image.cpp:156-172) for n frames of one camera.  From float planes (src == null: level 0 is
// already in place): the pyr-down chain, one launch per level for the whole batch; derived planes are built lazily per role
// (ensure_roles), like the reference's buildAccelerationStructure / PointSelection caches.  From raw planes: the stages the frames
// ask for (above), then one fused pass (k_build_from_raw) that also writes level 0 in role `role` (-1: not known yet, 0: current, 1:
// reference with the given thresholds) and leaves a copy of the raw planes in the frame unless the role makes it redundant (frame_source).
// src: device planes whose pitch is resolved, of frames that share camera and levels (check_ingest has seen to both).  From a colour
// source the kernels convert and leave grey in the frames' raw copies.
int frames_build(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, const IngestSource* src, int role = -1, float ithr = 0.0f,
                 float dthr = 0.0f, bool keep_raw_copy = true) {
  Range range("build");
  const CameraGeom* cam = frames[0]->cam;
  const StagesRun run{src && sensor_bytes(src->format) != 0, src && frames[0]->rig_on, src && frames[0]->lens_on, src && frames[0]->filter_on};
  // the stages, in their order: sensor format -> grey, depth rig -> registered Z, lens -> rectified I / Z, depth filter -> the filter plane;
  // behind them src is what the ingest reads
  const struct { bool on; IngestStage* stage; } chain[4] = {{run.sensor, sensor_stage}, {run.rig, rig_stage}, {run.lens, lens_stage},
                                                           {run.filter, filter_stage}};
  StagePlanes planes;
  IngestSource staged;
  for (const auto& link : chain) {
    if (!link.on) continue;
    const int rc = link.stage(ctx, n, frames, *src, planes, &staged);
    if (rc != DVO_HIP_OK) return rc;
    src = &staged;
  }
  const SourceKind kind = source_kind(src);
  const float depth_scale = src ? src->depth_scale : 0.0f;
  const int flavor0 = eager_current_flavor(ctx, cam, 0, n);
  std::vector<FrameBuildPtrs> host(n);
  bool wide = cam->w[0] % (kind.image_f32 ? 2 : 4) == 0;
  for (int i = 0; i < n; ++i) {
    dvo_hip_frame* f = frames[i];
    invalidate_roles(f);
    const FrameSource s = frame_source(f, src, i, kind, role, keep_raw_copy, run.lens, run.filter, host[i]);
    f->raw0 = s.raw0;
    f->raw_copy = s.raw_copy;
    f->depth_scale = depth_scale;
    wide = wide && s.wide;
    if (src && role == 0) f->lv[0].cur_have = flavor0;
    if (src && role == 1) mark_selected(f->lv[0], ithr, dthr);
  }
  const FrameBuildPtrs* tbl = nullptr;
  int rc = upload_build_table(ctx, n, frames, host, &tbl);
  if (rc != DVO_HIP_OK) return rc;
  int built = 1;                                       // float ingest: level 0 is already in place
  if (src) {
    rc = launch_raw_ingest(ctx, n, frames, tbl, kind, wide, depth_scale, role, ithr, dthr, flavor0, run, &built);
    if (rc != DVO_HIP_OK) return rc;
  }
  for (int l = built; l < frames[0]->levels; ++l) launch_pyr_down(ctx->build_stream, tbl, n, l, cam->w[l - 1], cam->h[l - 1]);
  DVO_HIP_TRY(ctx, hipGetLastError());
  return stamp_build(ctx, n, frames);
}

// One pass of ensure_roles over a frame list: what the role is built for and where (stream, table, grid cap), and the state the pass
// gathers -- table slices used, whether anything was launched.
struct RoleBuild {
  dvo_hip_context* ctx;
  int n;
  dvo_hip_frame* const* frames;
  int role;
  float ithr, dthr;
  bool eager;
  const int* cur_want;
  const CameraGeom* cam;
  DevBuf& table;
  hipStream_t stream;
  int cap;                                                     // (eager only: planes needed right now are built at full width)
  bool stream_nt;
  int uploads = 0;                                             // table slices used so far (each launch reads its own)
  bool launched = false;

  RoleBuild(dvo_hip_context* c, int n_frames, dvo_hip_frame* const* fr, int r, float it, float dt, bool e, const int* want)
      : ctx(c), n(n_frames), frames(fr), role(r), ithr(it), dthr(dt), eager(e), cur_want(want), cam(fr[0]->cam),
        table(e ? (r == 0 ? c->prep_tbl_cur : c->prep_tbl_ref) : (r == 0 ? c->role_tbl_cur : c->role_tbl_ref)),
        stream(e ? c->build_stream : c->stream), cap(e ? c->opt_build_workgroups : 0), stream_nt(e && c->opt_stream_policy != 0) {}

  // What frame f lacks at level l.  Current role: `miss` = the flavours wanted there (plane C only where the camera's frames have one)
  // that the frame does not hold; reference role: whether its selection stands for these thresholds (miss 0).
  struct Lack { int miss; bool need; };
  Lack lack_of(const dvo_hip_frame* f, int l) const {
    const FrameLevel& L = f->lv[l];
    if (role != 0) return Lack{0, !ref_ready(L, ithr, dthr)};
    const int want = (cur_want ? cur_want[l] : kCurAB) & (L.C ? (kCurAB | kCurC) : kCurAB);
    return Lack{want & ~L.cur_have, (want & ~L.cur_have) != 0};
  }

  void mark_built(FrameLevel& L, int flavours) const {
    if (role == 0) L.cur_have |= flavours;
    else mark_selected(L, ithr, dthr);
  }

  // `host` in a table slice of its own on the stream; plane_pointers_only: the launch reads nothing but the frames' plane pointers, so
  // the table the ingest of these very frames left on this stream serves as well
  int upload(const std::vector<FrameBuildPtrs>& host, const FrameBuildPtrs** tbl, bool plane_pointers_only = true) {
    if (plane_pointers_only && eager && ctx->build_tbl_cur && int(host.size()) == n && ctx->build_tbl_frames.size() == size_t(n) &&
        std::equal(frames, frames + n, ctx->build_tbl_frames.begin())) {
      *tbl = ctx->build_tbl_cur->as<FrameBuildPtrs>();
      return DVO_HIP_OK;
    }
    constexpr int kSlices = 4 * kMaxLevels;
    const size_t slice = size_t(n) * sizeof(FrameBuildPtrs);
    if (uploads == kSlices) {                                  // (never in practice: a slice per level and source)
      DVO_HIP_TRY(ctx, hipStreamSynchronize(stream));
      uploads = 0;
    }
    DVO_HIP_TRY(ctx, table.reserve(slice * kSlices));
    FrameBuildPtrs* up = reinterpret_cast<FrameBuildPtrs*>(table.as<char>() + slice * uploads++);
    DVO_HIP_TRY(ctx, ctx->tables.upload(stream, up, host.data(), host.size() * sizeof(FrameBuildPtrs)));
    *tbl = up;
    return DVO_HIP_OK;
  }

  // Every frame is checked before the state of any is touched: a frame ingested straight into a role without a copy of its raw planes
  // (option "keep_raw_copy" 0) has nothing its level 0 could be derived from in another role, and the marks -- planes "built" -- are
  // set while the launches are still being gathered (round-5 advisor finding: the error used to leave earlier frames of the list
  // marked as built without their launches, and a retry aligned against stale planes).
  int check_level0_sources() const {
    for (int i = 0; i < n; ++i) {
      const dvo_hip_frame* f = frames[i];
      if (!f->raw0 || f->lv[0].cur_have != 0 || f->raw_copy) continue;
      if (lack_of(f, 0).need) return fail(ctx, DVO_HIP_ERR_INVALID, "frame has neither sampling planes nor a raw copy at level 0");
    }
    return DVO_HIP_OK;
  }

  // Several levels, every frame missing the same planes on each of them, all to be derived from the float planes I / Z (a camera frame
  // that has just been built): ONE launch for all levels (k_derive_levels) instead of a table upload, a counter reset and a launch per
  // level.  *done: that was the case, and the levels are built.
  int uniform_span(int l0, int l1, bool* done) {
    LevelSpan span = level_span(l0, l1, cam->w, cam->h);
    // (the duplicate check is quadratic; large batches come through the ingest.  Round 6: the size test used to FOLLOW the double loop --
    // 524 288 comparisons per role of a 1024-pair batch, 0.4 ms of the host thread in front of every streaming step's first launch)
    bool uniform = n <= 64;
    for (int i = 0; i < n && uniform; ++i)
      for (int j = 0; j < i && uniform; ++j) uniform = frames[i] != frames[j];   // (a frame listed twice: the general path skips its second visit)
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
    if (!uniform) return DVO_HIP_OK;
    std::vector<FrameBuildPtrs> host(n);
    for (int i = 0; i < n; ++i) fill_build_ptrs(frames[i], host[i]);
    const FrameBuildPtrs* tbl = nullptr;
    int rc = upload(host, &tbl);
    if (rc != DVO_HIP_OK) return rc;
    launch_derive_levels(stream, tbl, n, span, role, ithr, dthr, cap);
    launched = true;
    for (int i = 0; i < n; ++i)
      for (int l = l0; l <= l1; ++l) mark_built(frames[i]->lv[l], span.flavor[l]);
    if (role == 1) rc = apply_selection(ctx, stream, n, frames, l0, l1, cap);
    *done = rc == DVO_HIP_OK;
    return rc;
  }

  // One level of the general path: the frames that lack something there, sorted by what their planes are derived from -- the float
  // planes I / Z (levels >= 1, and level 0 of frames created from float planes); at level 0 of a frame ingested from raw planes: the
  // other flavour of the current role, else the frame's copy of its raw planes -- and one launch per source for all of them.
  // *second_pass: raw copies of another depth scale than the launch gathered were left out (one kernel launch takes one scale).
  int level(int l, bool* second_pass) {
    std::vector<FrameBuildPtrs> from_planes[4], from_raw[4], ab_from_c, c_from_a, ref_from_c;
    std::vector<dvo_hip_frame*> ref_from_ab, selected;
    float raw_scale = 0.0f;
    for (int i = 0; i < n; ++i) {
      dvo_hip_frame* f = frames[i];
      FrameLevel& L = f->lv[l];
      const Lack lack = lack_of(f, l);
      if (!lack.need) continue;   // also skips the second visit of a frame that is listed twice
      FrameBuildPtrs p;
      fill_build_ptrs(f, p);
      if (l != 0 || !f->raw0) {
        from_planes[lack.miss].push_back(p);
      } else if (role == 0 && (L.cur_have & kCurC)) {
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
        from_raw[lack.miss].push_back(p);
      } else if (f->raw_copy) {
        *second_pass = true;
        continue;
      } else {
        return fail(ctx, DVO_HIP_ERR_INVALID, "frame has neither sampling planes nor a raw copy at level 0");
      }
      mark_built(L, lack.miss);
      if (role == 1) selected.push_back(f);
    }
    const FrameBuildPtrs* tbl = nullptr;
    for (int miss = 0; miss < 4; ++miss) {
      if (!from_planes[miss].empty()) {
        const int rc = upload(from_planes[miss], &tbl);
        if (rc != DVO_HIP_OK) return rc;
        if (role == 0) launch_derive_current(stream, tbl, int(from_planes[miss].size()), l, cam->w[l], cam->h[l], cap, miss, stream_nt);
        else launch_derive_reference(stream, tbl, int(from_planes[miss].size()), l, cam->w[l], cam->h[l], ithr, dthr, cap, stream_nt);
        launched = true;
      }
      if (!from_raw[miss].empty()) {
        const int rc = upload(from_raw[miss], &tbl, /*plane_pointers_only=*/false);
        if (rc != DVO_HIP_OK) return rc;
        launch_build_from_raw(stream, tbl, int(from_raw[miss].size()), raw_scale, cam->w[0], cam->h[0], /*levels=*/1, role,
                              ingest_strips_supports(cam->w[0], /*wide=*/true), ithr, dthr, cap, miss, 0, 0, stream_nt);
        launched = true;
      }
    }
    const struct { std::vector<FrameBuildPtrs>* list; int mode; } conversions[3] = {{&ab_from_c, 0}, {&c_from_a, 1}, {&ref_from_c, 2}};
    for (const auto& c : conversions) {
      if (c.list->empty()) continue;
      const int rc = upload(*c.list, &tbl);
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
    if (selected.empty()) return DVO_HIP_OK;
    return apply_selection(ctx, stream, int(selected.size()), selected.data(), l, l, cap);
  }

  // the levels l0 .. l1: the fast path where it applies, else level by level, up to and including a level that asks for a second pass
  int run(int l0, int l1, bool* second_pass) {
    int rc = l0 == 0 ? check_level0_sources() : DVO_HIP_OK;
    bool done = false;
    if (rc == DVO_HIP_OK && l1 > l0) rc = uniform_span(l0, l1, &done);
    for (int l = l0; l <= l1 && rc == DVO_HIP_OK && !done && !*second_pass; ++l) rc = level(l, second_pass);
    if (rc == DVO_HIP_OK && eager && launched) rc = stamp_build(ctx, n, frames);   // (the frames' ticket: behind everything this pass enqueued)
    if (rc == DVO_HIP_OK && !*second_pass) DVO_HIP_TRY(ctx, hipGetLastError());
    return rc;
  }
};

// Build the missing role planes of a set of frames for levels [l0, l1]: role 0 = current (flavours `cur_want[level]`, kCurAB | kCurC;
// null: the taps A + B), role 1 = reference (R + selection count for the given thresholds).  One launch per level (and source) for
// all frames that need it.
// `eager`: on the build stream (dvo_hip_frames_prepare), otherwise on the main stream right before the planes are used.
int ensure_roles(dvo_hip_context* ctx, int n, dvo_hip_frame* const* frames, int role, int l0, int l1, float ithr, float dthr, bool eager = false,
                 const int* cur_want = nullptr) {
  for (;;) {
    // A pass that met raw copies of a second depth scale re-enters HERE (rare, one more pass each): the whole list again, with the
    // table slices from the start -- they are reused, so the stream drains first.
    RoleBuild pass(ctx, n, frames, role, ithr, dthr, eager, cur_want);
    bool second_pass = false;
    const int rc = pass.run(l0, l1, &second_pass);
    if (rc != DVO_HIP_OK || !second_pass) return rc;
    DVO_HIP_TRY(ctx, hipStreamSynchronize(pass.stream));
  }
}
