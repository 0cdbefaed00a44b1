// capi_ingest.inc -- the raw-frame ingest: dvo_hip_frame_create_*, dvo_hip_frames_update_raw* / _colour* / _f32*, dvo_hip_flush_deferred.  Every
// entry point describes its planes as one IngestSource (grey is the one-channel pixel format, float planes are a pixel and a depth format) and goes through one checker (check_ingest),
// one routine that records or builds (ingest) and, from host memory, one walker of the upload ring (upload_planes); the entry points
// themselves translate flags and name themselves.  Textually included by capi.hip inside its extern "C" block, where an unnamed
// namespace does not keep a function's name out of the library's symbol table: the helpers are static.

// bytes per pixel of an IngestSource's image plane, 0 for an unknown format
static int source_channels(int format) {
  return format == 0 ? 1 : format == DVO_HIP_PIXEL_F32 ? 4 : sensor_bytes(format) ? sensor_bytes(format) : pixel_channels(format);
}
// the pixel_format argument of a colour entry point as an IngestSource's format: 0 is grey in here and no DVO_HIP_PIXEL_* to a caller.
// The colour formats and the sensor formats (sensor_formats.h)
static int colour_format(int pixel_format) { return pixel_channels(pixel_format) || sensor_bytes(pixel_format) ? pixel_format : -1; }
// the pixel_format argument of a float-depth entry point: DVO_HIP_PIXEL_GREY8 (0) is the grey plane there
static int mixed_format(int pixel_format) { return pixel_format == DVO_HIP_PIXEL_GREY8 ? pixel_format : colour_format(pixel_format); }

// the byte ranges [a, a + na) and [b, b + nb) meet
static bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

// The planes of an ingest of n frames of width x height pixels: format, arrays and their entries, the pitch rules; resolves src->pitch.  With
// `frames` (entries not null), in the same pass: they share camera and levels -- a camera is shared by frames of any level count
// (get_camera), and frames_build writes one table and launches once per level for all of them.
static int check_source(dvo_hip_context* ctx, const char* who, int n, dvo_hip_frame* const* frames, int width, int height, IngestSource* src) {
  const int channels = src->format < 0 ? 0 : source_channels(src->format);
  if (channels == 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "unknown pixel format (DVO_HIP_PIXEL_*)");
  const bool image_f32 = src->format == DVO_HIP_PIXEL_F32, depth_f32 = src->depth_format == DVO_HIP_DEPTH_F32;
  if (!depth_f32 && src->depth_format != DVO_HIP_DEPTH_U16) return fail(ctx, DVO_HIP_ERR_INVALID, who, "unknown depth format (DVO_HIP_DEPTH_*)");
  if (image_f32 && !depth_f32) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a float image plane needs a float depth plane");
  if (!src->planes || !src->depth) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null argument");
  // (sensor_formats.h: the reflection needs two samples a side, a YUV 4:2:2 row is made of pixel pairs)
  if (sensor_is_bayer(src->format) && (width < 2 || height < 2)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a Bayer plane needs width >= 2 and height >= 2");
  if (sensor_is_yuv(src->format) && width % 2 != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a YUV 4:2:2 plane needs an even width");
  for (int i = 0; i < n; ++i) {
    if (frames && (!frames[i] || frames[i]->cam != frames[0]->cam || frames[i]->levels != frames[0]->levels))
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "frames of one build batch must share camera and levels");
    // (one rectify launch per ingest, one lens per launch: lens_stage)
    if (frames && (frames[i]->lens_on != frames[0]->lens_on || std::memcmp(&frames[i]->lens, &frames[0]->lens, sizeof(dvo_hip_lens)) != 0))
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "frames of one ingest must carry the same lens, or none (dvo_hip_frames_set_lens)");
    // (likewise one register pass per ingest, one depth rig per launch: rig_stage)
    if (frames && (frames[i]->rig_on != frames[0]->rig_on || std::memcmp(&frames[i]->rig, &frames[0]->rig, sizeof(dvo_hip_depth_rig)) != 0))
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "frames of one ingest must carry the same depth rig, or none (dvo_hip_frames_set_depth_rig)");
    // (and one filter pass per ingest, one depth filter per launch: filter_stage)
    if (frames && (frames[i]->filter_on != frames[0]->filter_on || std::memcmp(&frames[i]->filter, &frames[0]->filter, sizeof(dvo_hip_depth_filter)) != 0))
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "frames of one ingest must carry the same depth filter, or none (dvo_hip_frames_set_depth_filter)");
    if (!src->planes[i] || !src->depth[i]) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null entry");
    if ((image_f32 && !aligned_to(src->planes[i], 4)) || (depth_f32 && !aligned_to(src->depth[i], 4)))
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "a float plane must be 4-byte aligned");
  }
  const size_t tight = size_t(width > 0 ? width : 0) * channels;
  if (src->pitch != 0 && src->pitch < tight) return fail(ctx, DVO_HIP_ERR_INVALID, who, "pitch < width * channels");
  if (src->pitch > size_t(INT_MAX)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "pitch above 2^31 - 1");
  if (src->pitch == 0) src->pitch = tight;
  if (image_f32 && src->pitch % 4 != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a float plane's pitch must be a multiple of 4");
  if (depth_f32) {
    const size_t tight_z = size_t(width > 0 ? width : 0) * 4;
    if (src->depth_pitch != 0 && src->depth_pitch < tight_z) return fail(ctx, DVO_HIP_ERR_INVALID, who, "depth pitch < width * 4");
    if (src->depth_pitch > size_t(INT_MAX)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "depth pitch above 2^31 - 1");
    if (src->depth_pitch % 4 != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a float plane's pitch must be a multiple of 4");
    if (src->depth_pitch == 0) src->depth_pitch = tight_z;
  }
  // A frame with a lens is rectified INTO its own float planes of level 0 (lens_stage) while the pass gathers taps from the caller's
  // planes: a source that lies in those planes -- the in-place float ingest of a lens-less frame -- would be read while it is overwritten.
  // A frame with a depth rig is registered INTO its own float plane Z of level 0 (rig_stage), a scatter: a source that lies in
  // that plane -- depth or image -- would be overwritten by the fill before it is read.
  // A frame with a depth filter is filtered INTO its filter plane, a stencil, and the ingest behind it stores the frame's level-0 planes
  // while it reads that plane and the caller's image: a caller plane in any of the three is refused.
  if (frames && (frames[0]->lens_on || frames[0]->rig_on || frames[0]->filter_on)) {
    const size_t h = size_t(frames[0]->lv[0].h), own = size_t(width) * h * 4;
    const size_t image_bytes = src->pitch * h, depth_bytes = (depth_f32 ? src->depth_pitch : size_t(width) * 2) * h;
    auto reads = [&](int i, const void* mine) { return overlaps(src->planes[i], image_bytes, mine, own) || overlaps(src->depth[i], depth_bytes, mine, own); };
    for (int i = 0; i < n && frames[0]->lens_on; ++i)
      if (reads(i, frames[i]->lv[0].I) || reads(i, frames[i]->lv[0].Z))
        return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame that carries a lens cannot be ingested from its own level-0 planes");
    for (int i = 0; i < n && frames[0]->rig_on; ++i)
      if (reads(i, frames[i]->lv[0].Z))
        return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame that carries a depth rig cannot be ingested from its own level-0 plane Z");
    for (int i = 0; i < n && frames[0]->filter_on; ++i)
      if (reads(i, frames[i]->lv[0].I) || reads(i, frames[i]->lv[0].Z) || reads(i, frames[i]->filter_plane.p))
        return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame that carries a depth filter cannot be ingested from its own level-0 planes or its filter plane");
  }
  return DVO_HIP_OK;
}

// Every argument of an ingest, checked before any frame is touched and before any transfer is enqueued.  role -1 where the entry point
// admits a plain update (plain_ok; cfg ignored), else check_prepare_args.
static int check_ingest(dvo_hip_context* ctx, const char* who, int n_frames, dvo_hip_frame* const* frames, IngestSource* src, bool plain_ok, int role,
                        const dvo_hip_config* cfg) {
  if (!ctx) return DVO_HIP_ERR_INVALID;
  if (plain_ok && role == -1) {
    if (n_frames < 1 || !frames) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
    if (!frames[0]) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null entry");
  } else {
    const int rc = check_prepare_args(ctx, n_frames, frames, role, cfg, who);
    if (rc != DVO_HIP_OK) return rc;
  }
  return check_source(ctx, who, n_frames, frames, frames[0]->lv[0].w, frames[0]->lv[0].h, src);
}

namespace {   // (flush_deferred is declared there at the head of capi.hip, for DVO_FLUSH_DEFERRED)

// ingest of device-resident raw planes, optionally straight into a role (role < 0: none, cfg not read)
int update_raw_device(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const IngestSource& src, int role, const dvo_hip_config* cfg,
                      bool keep_raw_copy) {
  const bool ref = role == DVO_HIP_ROLE_REFERENCE;
  const int fused = role >= 0 && cfg->last_level == 0 ? (ref ? 1 : 0) : -1;   // level 0 is built in the same pass if it is used at all
  int rc = frames_build(ctx, n_frames, frames, &src, fused, ref ? cfg->intensity_derivative_threshold : 0.0f,
                        ref ? cfg->depth_derivative_threshold : 0.0f, keep_raw_copy);
  if (rc == DVO_HIP_OK && role >= 0) rc = prepare_roles(ctx, n_frames, frames, role, cfg);
  return rc;
}

// carry out the recorded ingests (option "defer_ingest"), oldest first; the first failure is returned, the list is empty afterwards
int flush_deferred(dvo_hip_context* ctx) {
  if (ctx->deferred.empty()) return DVO_HIP_OK;
  std::vector<dvo_hip_context::DeferredIngest> list;
  list.swap(ctx->deferred);
  int rc = DVO_HIP_OK;
  for (dvo_hip_context::DeferredIngest& d : list) {
    for (dvo_hip_frame* f : d.frames) f->deferred = 0;
    if (rc != DVO_HIP_OK) continue;
    ctx->deferred_ingests += 1;
    const IngestSource src{d.planes.data(), d.format, d.pitch, d.depth.data(), d.depth_scale, d.depth_format, d.depth_pitch};
    rc = update_raw_device(ctx, int(d.frames.size()), d.frames.data(), src, d.role, d.role >= 0 ? &d.cfg : nullptr, d.keep_raw_copy);
  }
  return rc;
}

}  // namespace

// Host planes into the next buffer of the upload ring, on the upload stream; the build stream waits for them.  The planes land in slots
// of [depth: u16, or float rows of `zrow` = 4 w bytes, tight][image plane, rows of `row` bytes, tight], each padded to an even size (to a
// multiple of 8 with a float plane in it: the strip kernel's rows); planes[i] / depth[i]: where frame i's went,
// *ring: the buffer.  From pinned memory (dvo_hip_host_alloc) the transfers are truly asynchronous, from pageable memory the runtime
// stages them (correct, but the call then blocks for most of the copy).  A frame whose tight 8-bit plane directly follows its depth plane
// moves in one transfer, and so does a run of such frames at the slot stride (without the last slot's padding, which may lie past the
// end of the caller's buffer); a padded host pitch is repacked by a 2-D transfer.
static int upload_planes(dvo_hip_context* ctx, int n_frames, int w, int h, size_t row, const IngestSource& host, const void** planes, const void** depth,
                         unsigned* ring) {
  const bool depth_f32 = host.depth_format == DVO_HIP_DEPTH_F32;
  const size_t plane = row * h;
  const size_t zrow = size_t(w) * (depth_f32 ? 4 : 2), zplane = zrow * h;
  const bool ztight = !depth_f32 || host.depth_pitch == zrow;
  const size_t slot_bytes = depth_f32 ? (zplane + plane + 7) & ~size_t(7) : (zplane + plane + 1) & ~size_t(1);
  const unsigned b = ctx->upload_next++ % dvo_hip_context::kUploadRing;
  DevBuf& buf = ctx->upload_buf[b];
  // the previous contents of this buffer may still be read by the build they were uploaded for
  const int rc = wait_for_ticket(ctx, ctx->upload_buf_seq[b], /*upload=*/true);
  if (rc != DVO_HIP_OK) return rc;
  if (buf.bytes < slot_bytes * size_t(n_frames)) {
    DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->build_stream));   // growing = free + malloc
    DVO_HIP_TRY(ctx, buf.reserve(slot_bytes * size_t(n_frames)));
  }
  char* base = buf.as<char>();
  const bool tight = host.pitch == row && ztight;
  for (int i = 0; i < n_frames;) {
    const char* hd = static_cast<const char*>(host.depth[i]);
    if (!tight || static_cast<const char*>(host.planes[i]) != hd + zplane) {   // separate planes: two transfers for this frame
      if (ztight) DVO_HIP_TRY(ctx, hipMemcpyAsync(base + slot_bytes * i, hd, zplane, hipMemcpyHostToDevice, ctx->upload_stream));
      else DVO_HIP_TRY(ctx, hipMemcpy2DAsync(base + slot_bytes * i, zrow, hd, host.depth_pitch, zrow, h, hipMemcpyHostToDevice, ctx->upload_stream));
      if (host.pitch == row) DVO_HIP_TRY(ctx, hipMemcpyAsync(base + slot_bytes * i + zplane, host.planes[i], plane, hipMemcpyHostToDevice, ctx->upload_stream));
      else DVO_HIP_TRY(ctx, hipMemcpy2DAsync(base + slot_bytes * i + zplane, row, host.planes[i], host.pitch, row, h, hipMemcpyHostToDevice, ctx->upload_stream));
      ++i;
      continue;
    }
    int j = i + 1;                                               // frames in the slot layout that follow each other in host memory
    while (j < n_frames && static_cast<const char*>(host.depth[j]) == hd + slot_bytes * size_t(j - i) &&
           static_cast<const char*>(host.planes[j]) == static_cast<const char*>(host.depth[j]) + zplane)
      ++j;
    DVO_HIP_TRY(ctx, hipMemcpyAsync(base + slot_bytes * i, hd, slot_bytes * size_t(j - i) - (slot_bytes - zplane - plane), hipMemcpyHostToDevice,
                                    ctx->upload_stream));
    i = j;
  }
  for (int i = 0; i < n_frames; ++i) {
    depth[i] = base + slot_bytes * i;
    planes[i] = base + slot_bytes * i + zplane;
  }
  DVO_HIP_TRY(ctx, hipEventRecord(ctx->upload_done, ctx->upload_stream));
  DVO_HIP_TRY(ctx, hipStreamWaitEvent(ctx->build_stream, ctx->upload_done, 0));
  *ring = b;
  return DVO_HIP_OK;
}

// The ingest behind every entry point: validate, then record the request (device planes, option "defer_ingest" / DVO_HIP_INGEST_DEFER)
// or carry out what is recorded and build -- a call that is refused or that records flushes nothing.  host_planes: the planes go
// through the upload ring first (streaming ingest from HOST memory: DMA on the upload stream, then the batched build on the build
// stream; returns at once).  defer / keep_raw_copy: -1 = what the context's options say ("defer_ingest", "keep_raw_copy"), 0 / 1 = for
// this call.
static int ingest(dvo_hip_context* ctx, const char* who, int n_frames, dvo_hip_frame* const* frames, IngestSource src, bool host_planes, bool plain_ok, int role,
                  const dvo_hip_config* cfg, int defer, int keep_raw_copy) {
  int rc = check_ingest(ctx, who, n_frames, frames, &src, plain_ok, role, cfg);
  if (rc != DVO_HIP_OK) return rc;
  const bool keep = keep_raw_copy < 0 ? ctx->opt_keep_raw_copy != 0 : keep_raw_copy != 0;
  if (!host_planes && (defer < 0 ? ctx->opt_defer_ingest != 0 : defer != 0)) {
    dvo_hip_context::DeferredIngest d;
    d.frames.assign(frames, frames + n_frames);
    d.planes.assign(src.planes, src.planes + n_frames);
    d.depth.assign(src.depth, src.depth + n_frames);
    d.format = src.format;
    d.pitch = src.pitch;
    d.depth_format = src.depth_format;
    d.depth_pitch = src.depth_pitch;
    d.depth_scale = src.depth_scale;
    d.role = role;
    if (role >= 0) d.cfg = *cfg;
    d.keep_raw_copy = keep;
    for (int i = 0; i < n_frames; ++i) frames[i]->deferred = 1;
    ctx->deferred.push_back(std::move(d));
    return DVO_HIP_OK;
  }
  DVO_FLUSH_DEFERRED(ctx);                                     // (nothing overtakes a recorded ingest)
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!host_planes) return update_raw_device(ctx, n_frames, frames, src, role, cfg, keep);
  std::vector<const void*> planes(static_cast<size_t>(n_frames)), depth(static_cast<size_t>(n_frames));
  const size_t row = size_t(frames[0]->lv[0].w) * source_channels(src.format);
  unsigned ring = 0;
  rc = upload_planes(ctx, n_frames, frames[0]->lv[0].w, frames[0]->lv[0].h, row, src, planes.data(), depth.data(), &ring);
  if (rc != DVO_HIP_OK) return rc;
  const IngestSource uploaded{planes.data(), src.format, row, depth.data(), src.depth_scale, src.depth_format, size_t(frames[0]->lv[0].w) * 4};
  rc = update_raw_device(ctx, n_frames, frames, uploaded, role, cfg, keep);
  ctx->upload_buf_seq[ring] = ctx->build_seq;          // the newest ticket is behind every reader of the buffer
  return rc;
}

// The end of every dvo_hip_frame_create_*: rc / e = what building frame f came to; a frame that failed is destroyed, a good one handed over.
static int frame_create_finish(dvo_hip_context* ctx, const char* who, dvo_hip_frame* f, int rc, hipError_t e, dvo_hip_frame** out) {
  if (e != hipSuccess) ctx->err = std::string(who) + ": " + hipGetErrorString(e);
  if (e != hipSuccess || rc != DVO_HIP_OK) {
    dvo_hip_frame_destroy(ctx, f);
    return rc != DVO_HIP_OK ? rc : DVO_HIP_ERR_HIP;
  }
  *out = f;
  return DVO_HIP_OK;
}

// A new frame from one frame's raw planes.  The routes differ for reasons:
enum CreateRoute {
  kCreateStaged,     // host planes copied into the frame's own 3-B staging area on the build stream: that IS the frame's raw copy, for free
  kCreateUploaded,   // host planes through the upload ring like a streaming ingest (the staging area cannot hold a colour plane)
  kCreateDevice      // device planes; asynchronous (build stream): every later use of the frame is ordered after the build
};
static int frame_create_raw(dvo_hip_context* ctx, const char* who, int width, int height, const float K[4], int levels, IngestSource src, CreateRoute route,
                            dvo_hip_frame** out) {
  if (!ctx || !out || !K) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null argument");
  int rc = check_source(ctx, who, 1, nullptr, width, height, &src);
  if (rc != DVO_HIP_OK) return rc;
  size_t raw_off;
  dvo_hip_frame* f = nullptr;
  rc = frame_alloc(ctx, width, height, K, levels, &f, &raw_off);
  if (rc != DVO_HIP_OK) return rc;
  hipError_t e = hipSuccess;
  const void* staged_grey[1] = {staging_grey(f)};
  const void* staged_depth[1] = {staging_depth(f)};
  if (route == kCreateStaged) {
    const size_t n = size_t(width) * height;
    e = hipMemcpyAsync(staging_depth(f), src.depth[0], n * 2, hipMemcpyHostToDevice, ctx->build_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(staging_grey(f), src.planes[0], n, hipMemcpyHostToDevice, ctx->build_stream);
    src.planes = staged_grey;
    src.depth = staged_depth;
  }
  if (e == hipSuccess) rc = ingest(ctx, who, 1, &f, src, route == kCreateUploaded, /*plain_ok=*/true, -1, nullptr, 0, 1);
  if (e == hipSuccess && rc == DVO_HIP_OK && route != kCreateDevice) e = sync_stream(ctx->build_stream);   // the caller's host buffers may go away
  return frame_create_finish(ctx, who, f, rc, e, out);
}

int dvo_hip_frame_create_f32(dvo_hip_context* ctx, int width, int height, const float K[4], const float* intensity,
                             const float* depth, int levels, dvo_hip_frame** out) {
  DVO_ENTER(ctx);
  if (!ctx || !out || !intensity || !depth || !K) return fail(ctx, DVO_HIP_ERR_INVALID, "frame_create_f32", "null argument");
  size_t raw_off;
  dvo_hip_frame* f = nullptr;
  int rc = frame_alloc(ctx, width, height, K, levels, &f, &raw_off);
  if (rc != DVO_HIP_OK) return rc;
  const size_t n = size_t(width) * height;
  hipError_t e = hipMemcpyAsync(f->lv[0].I, intensity, n * 4, hipMemcpyHostToDevice, ctx->build_stream);
  if (e == hipSuccess) e = hipMemcpyAsync(f->lv[0].Z, depth, n * 4, hipMemcpyHostToDevice, ctx->build_stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->sel_count, 0, sizeof(int) * kMaxLevels, ctx->build_stream);
  if (e == hipSuccess) {
    rc = frames_build(ctx, 1, &f, /*src=*/nullptr);
    if (rc == DVO_HIP_OK) e = sync_stream(ctx->build_stream);   // the caller's host buffers may go away
  }
  return frame_create_finish(ctx, "frame_create_f32", f, rc, e, out);
}

int dvo_hip_frame_create_raw(dvo_hip_context* ctx, int width, int height, const float K[4], const uint8_t* grey,
                             const uint16_t* raw_depth, float depth_scale, int levels, dvo_hip_frame** out) {
  DVO_ENTER(ctx);
  const void* g[1] = {grey};
  const void* r[1] = {raw_depth};
  return frame_create_raw(ctx, "frame_create_raw", width, height, K, levels, IngestSource{g, 0, 0, r, depth_scale}, kCreateStaged, out);
}

int dvo_hip_frame_create_raw_device(dvo_hip_context* ctx, int width, int height, const float K[4], const void* grey_dev,
                                    const void* raw_depth_dev, float depth_scale, int levels, dvo_hip_frame** out) {
  DVO_ENTER(ctx);
  const void* g[1] = {grey_dev};
  const void* r[1] = {raw_depth_dev};
  return frame_create_raw(ctx, "frame_create_raw_device", width, height, K, levels, IngestSource{g, 0, 0, r, depth_scale}, kCreateDevice, out);
}

int dvo_hip_frame_create_colour(dvo_hip_context* ctx, int width, int height, const float K[4], const void* colour, int pixel_format,
                                size_t colour_pitch, const uint16_t* raw_depth, float depth_scale, int levels, dvo_hip_frame** out) {
  DVO_ENTER(ctx);
  const void* c[1] = {colour};
  const void* r[1] = {raw_depth};
  return frame_create_raw(ctx, "frame_create_colour", width, height, K, levels, IngestSource{c, colour_format(pixel_format), colour_pitch, r, depth_scale},
                          kCreateUploaded, out);
}

int dvo_hip_frame_create_colour_device(dvo_hip_context* ctx, int width, int height, const float K[4], const void* colour_dev, int pixel_format,
                                       size_t colour_pitch, const void* raw_depth_dev, float depth_scale, int levels, dvo_hip_frame** out) {
  DVO_ENTER(ctx);
  const void* c[1] = {colour_dev};
  const void* r[1] = {raw_depth_dev};
  return frame_create_raw(ctx, "frame_create_colour_device", width, height, K, levels,
                          IngestSource{c, colour_format(pixel_format), colour_pitch, r, depth_scale}, kCreateDevice, out);
}

// ---- re-ingest of existing frames.  The grey entry points from device memory with a role and both colour ones validate first and flush
// only when they are about to build (inside ingest); the others carry out what is recorded on entry, like every other entry point. ----

int dvo_hip_frames_update_raw_device(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* grey_dev,
                                     const void* const* raw_depth_dev, float depth_scale) {
  DVO_ENTER(ctx);
  return ingest(ctx, "frames_update_raw_device", n_frames, frames, IngestSource{grey_dev, 0, 0, raw_depth_dev, depth_scale}, /*host_planes=*/false,
                /*plain_ok=*/true, -1, nullptr, 0, 1);
}

int dvo_hip_frame_update_raw_device(dvo_hip_context* ctx, dvo_hip_frame* frame, const void* grey_dev, const void* raw_depth_dev,
                                    float depth_scale) {
  dvo_hip_frame* f[1] = {frame};
  const void* g[1] = {grey_dev};
  const void* r[1] = {raw_depth_dev};
  return dvo_hip_frames_update_raw_device(ctx, 1, f, g, r, depth_scale);
}

int dvo_hip_frames_update_raw_device_as(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* grey_dev,
                                        const void* const* raw_depth_dev, float depth_scale, int role, const dvo_hip_config* cfg) {
  DVO_LOCK(ctx);
  return ingest(ctx, "frames_update_raw_device_as", n_frames, frames, IngestSource{grey_dev, 0, 0, raw_depth_dev, depth_scale}, /*host_planes=*/false,
                /*plain_ok=*/false, role, cfg, -1, -1);
}

int dvo_hip_frames_update_raw_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* grey_dev,
                                           const void* const* raw_depth_dev, float depth_scale, int role, const dvo_hip_config* cfg, unsigned flags) {
  DVO_LOCK(ctx);
  return ingest(ctx, "frames_update_raw_device_as_ex", n_frames, frames, IngestSource{grey_dev, 0, 0, raw_depth_dev, depth_scale}, /*host_planes=*/false,
                /*plain_ok=*/false, role, cfg, (flags & DVO_HIP_INGEST_DEFER) ? 1 : 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}

int dvo_hip_flush_deferred(dvo_hip_context* ctx) {
  if (!ctx) return DVO_HIP_ERR_INVALID;
  DVO_ENTER(ctx);
  return DVO_HIP_OK;
}

int dvo_hip_frames_update_raw(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const uint8_t* const* grey,
                              const uint16_t* const* raw_depth, float depth_scale) {
  DVO_ENTER(ctx);
  const IngestSource src{reinterpret_cast<const void* const*>(grey), 0, 0, reinterpret_cast<const void* const*>(raw_depth), depth_scale};
  return ingest(ctx, "frames_update_raw", n_frames, frames, src, /*host_planes=*/true, /*plain_ok=*/true, -1, nullptr, 0, 1);
}

int dvo_hip_frames_update_raw_as(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const uint8_t* const* grey,
                                 const uint16_t* const* raw_depth, float depth_scale, int role, const dvo_hip_config* cfg) {
  DVO_ENTER(ctx);
  const IngestSource src{reinterpret_cast<const void* const*>(grey), 0, 0, reinterpret_cast<const void* const*>(raw_depth), depth_scale};
  return ingest(ctx, "frames_update_raw_as", n_frames, frames, src, /*host_planes=*/true, /*plain_ok=*/false, role, cfg, 0, -1);
}

int dvo_hip_frames_update_raw_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const uint8_t* const* grey,
                                    const uint16_t* const* raw_depth, float depth_scale, int role, const dvo_hip_config* cfg, unsigned flags) {
  DVO_ENTER(ctx);
  const IngestSource src{reinterpret_cast<const void* const*>(grey), 0, 0, reinterpret_cast<const void* const*>(raw_depth), depth_scale};
  return ingest(ctx, "frames_update_raw_as_ex", n_frames, frames, src, /*host_planes=*/true, /*plain_ok=*/false, role, cfg, 0,
                (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}

// ---- colour (colour.h): the colour plane goes where the grey one went, the kernels convert it ----

int dvo_hip_frames_update_colour_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* colour_dev,
                                              int pixel_format, size_t colour_pitch, const void* const* raw_depth_dev, float depth_scale, int role,
                                              const dvo_hip_config* cfg, unsigned flags) {
  DVO_LOCK(ctx);
  return ingest(ctx, "frames_update_colour_device_as_ex", n_frames, frames,
                IngestSource{colour_dev, colour_format(pixel_format), colour_pitch, raw_depth_dev, depth_scale}, /*host_planes=*/false, /*plain_ok=*/true, role,
                cfg, (flags & DVO_HIP_INGEST_DEFER) ? 1 : 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}

int dvo_hip_frames_update_colour_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* colour,
                                       int pixel_format, size_t colour_pitch, const uint16_t* const* raw_depth, float depth_scale, int role,
                                       const dvo_hip_config* cfg, unsigned flags) {
  DVO_LOCK(ctx);
  return ingest(ctx, "frames_update_colour_as_ex", n_frames, frames,
                IngestSource{colour, colour_format(pixel_format), colour_pitch, reinterpret_cast<const void* const*>(raw_depth), depth_scale},
                /*host_planes=*/true, /*plain_ok=*/true, role, cfg, 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}

// ---- float planes: a float image and / or a float depth plane go where the 8-bit and the u16 plane went, the kernels read them as
// they are (DVO_HIP_PIXEL_F32, DVO_HIP_DEPTH_F32); the frame's raw copy is then its own float planes of level 0 (frames_build) ----

int dvo_hip_frame_create_f32_device(dvo_hip_context* ctx, int width, int height, const float K[4], const void* intensity_dev, const void* depth_dev,
                                    int levels, dvo_hip_frame** out) {
  DVO_ENTER(ctx);
  const void* i[1] = {intensity_dev};
  const void* z[1] = {depth_dev};
  return frame_create_raw(ctx, "frame_create_f32_device", width, height, K, levels, IngestSource{i, DVO_HIP_PIXEL_F32, 0, z, 1.0f, DVO_HIP_DEPTH_F32, 0},
                          kCreateDevice, out);
}

int dvo_hip_frames_update_f32_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* intensity_dev,
                                           size_t intensity_pitch, const void* const* depth_dev, size_t depth_pitch, float depth_scale, int role,
                                           const dvo_hip_config* cfg, unsigned flags) {
  DVO_LOCK(ctx);
  return ingest(ctx, "frames_update_f32_device_as_ex", n_frames, frames,
                IngestSource{intensity_dev, DVO_HIP_PIXEL_F32, intensity_pitch, depth_dev, depth_scale, DVO_HIP_DEPTH_F32, depth_pitch},
                /*host_planes=*/false, /*plain_ok=*/true, role, cfg, (flags & DVO_HIP_INGEST_DEFER) ? 1 : 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}

int dvo_hip_frames_update_f32_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const float* const* intensity,
                                    size_t intensity_pitch, const float* const* depth, size_t depth_pitch, float depth_scale, int role,
                                    const dvo_hip_config* cfg, unsigned flags) {
  DVO_LOCK(ctx);
  if (ctx && (flags & DVO_HIP_INGEST_DEFER)) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_update_f32_as_ex", "DVO_HIP_INGEST_DEFER takes device planes");
  return ingest(ctx, "frames_update_f32_as_ex", n_frames, frames,
                IngestSource{reinterpret_cast<const void* const*>(intensity), DVO_HIP_PIXEL_F32, intensity_pitch,
                             reinterpret_cast<const void* const*>(depth), depth_scale, DVO_HIP_DEPTH_F32, depth_pitch},
                /*host_planes=*/true, /*plain_ok=*/true, role, cfg, 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}

int dvo_hip_frames_update_colour_f32depth_device_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* colour_dev,
                                                       int pixel_format, size_t colour_pitch, const void* const* depth_dev, size_t depth_pitch,
                                                       float depth_scale, int role, const dvo_hip_config* cfg, unsigned flags) {
  DVO_LOCK(ctx);
  return ingest(ctx, "frames_update_colour_f32depth_device_as_ex", n_frames, frames,
                IngestSource{colour_dev, mixed_format(pixel_format), colour_pitch, depth_dev, depth_scale, DVO_HIP_DEPTH_F32, depth_pitch},
                /*host_planes=*/false, /*plain_ok=*/true, role, cfg, (flags & DVO_HIP_INGEST_DEFER) ? 1 : 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}

int dvo_hip_frames_update_colour_f32depth_as_ex(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* colour,
                                                int pixel_format, size_t colour_pitch, const float* const* depth, size_t depth_pitch, float depth_scale,
                                                int role, const dvo_hip_config* cfg, unsigned flags) {
  DVO_LOCK(ctx);
  if (ctx && (flags & DVO_HIP_INGEST_DEFER))
    return fail(ctx, DVO_HIP_ERR_INVALID, "frames_update_colour_f32depth_as_ex", "DVO_HIP_INGEST_DEFER takes device planes");
  return ingest(ctx, "frames_update_colour_f32depth_as_ex", n_frames, frames,
                IngestSource{colour, mixed_format(pixel_format), colour_pitch, reinterpret_cast<const void* const*>(depth), depth_scale, DVO_HIP_DEPTH_F32,
                             depth_pitch},
                /*host_planes=*/true, /*plain_ok=*/true, role, cfg, 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
}
