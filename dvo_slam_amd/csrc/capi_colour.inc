// capi_colour.inc -- the colour of frames behind the C-ABI (include/dvo_hip.h, dvo_hip_frames_set_colour, dvo_hip_frames_clear_colour and
// dvo_hip_frame_download_colour; semantics: cloud_colour.h; kernels: cloud_colour.hip).  A frame's colour is its own level-0 plane of
// packed pixels, written and read on the context's main stream only -- the stream every map call runs on -- so it needs no event of its
// own; arguments are checked before anything is launched or changed.  Textually included by capi.hip inside its extern "C" block.
int dvo_hip_frames_set_colour(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const void* const* colour, int pixel_format,
                              size_t colour_pitch, int on_device) {
  DVO_ENTER(ctx);
  const char* who = "frames_set_colour";
  int rc = check_frame_list(ctx, n_frames, frames, who, /*own_context=*/true);
  if (rc != DVO_HIP_OK) return rc;
  // (a sensor format -- a Bayer mosaic, YUV 4:2:2, sensor_formats.h -- is converted by k_sensor_convert in place of k_colour_pack)
  const bool sensor = sensor_bytes(pixel_format) != 0;
  const int channels = sensor ? sensor_bytes(pixel_format) : pixel_channels(pixel_format);
  if (channels == 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "unknown pixel format");
  if (!colour) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  long long blocks = 0;
  size_t stage_bytes = 0;
  for (int i = 0; i < n_frames; ++i) {
    const dvo_hip_frame* f = frames[i];
    if (!colour[i]) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null colour plane");
    const size_t row = size_t(f->lv[0].w) * size_t(channels);
    if (colour_pitch != 0 && colour_pitch < row) return fail(ctx, DVO_HIP_ERR_INVALID, who, "colour_pitch < width * channels");
    if (colour_pitch > size_t(INT_MAX)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "colour_pitch is too large");
    if (sensor_is_yuv(pixel_format) && f->lv[0].w % 2 != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a YUV 4:2:2 plane needs an even width");
    if (f->lens_on)
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame that carries a lens takes raw sensor planes; its colour must be attached rectified (clear the lens first, or attach to a frame without one)");
    for (int k = 0; k < i; ++k)
      if (frames[k] == f) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the same frame twice");
    blocks += (static_cast<long long>(f->lv[0].w) * f->lv[0].h + 255) / 256;
    stage_bytes += align_up(row * size_t(f->lv[0].h), 256);
  }
  if (blocks > 0x7fffffffll) return fail(ctx, DVO_HIP_ERR_INVALID, who, "too many pixels for one call");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // every allocation first: a failure leaves the frames as they were
  for (int i = 0; i < n_frames; ++i) {
    dvo_hip_frame* f = frames[i];
    const size_t bytes = size_t(f->lv[0].w) * size_t(f->lv[0].h) * 4;
    if (f->colour.bytes < bytes) {
      // (a smaller plane cannot be: a frame keeps its size.  Earlier readers of a plane that is replaced run on the main stream)
      DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      DVO_HIP_TRY(ctx, f->colour.reserve(bytes));
    }
  }
  if (!on_device) DVO_HIP_TRY(ctx, ctx->colour_stage.reserve(stage_bytes));
  std::vector<ColourPlane> host(size_t(n_frames) + 1);
  int at_block = 0;
  size_t at_stage = 0;
  for (int i = 0; i < n_frames; ++i) {
    dvo_hip_frame* f = frames[i];
    const int w = f->lv[0].w, h = f->lv[0].h;
    const size_t row = size_t(w) * size_t(channels), pitch = colour_pitch ? colour_pitch : row;
    ColourPlane& p = host[size_t(i)];
    if (on_device) {
      p.src = static_cast<const uint8_t*>(colour[i]);
      p.pitch = int(pitch);
    } else {
      // a host plane is staged tight, behind the main stream's earlier work (the staging area's last reader is an earlier k_colour_pack there)
      uint8_t* staged = ctx->colour_stage.as<uint8_t>() + at_stage;
      DVO_HIP_TRY(ctx, hipMemcpy2DAsync(staged, row, colour[i], pitch, row, size_t(h), hipMemcpyHostToDevice, ctx->stream));
      p.src = staged;
      p.pitch = int(row);
      at_stage += align_up(row * size_t(h), 256);
    }
    p.dst = f->colour.as<uint32_t>();
    p.w = w;
    p.h = h;
    p.first_block = at_block;
    at_block += (w * h + 255) / 256;
  }
  if (sensor) {
    // one launch per frame size (k_sensor_convert takes frames of one size): the table lists the frames size by size, each launch reads
    // its own run of it
    std::vector<SensorPtrs> table;
    std::vector<int> order;
    for (int i = 0; i < n_frames; ++i) {
      if (std::find(order.begin(), order.end(), i) != order.end()) continue;
      for (int k = i; k < n_frames; ++k)
        if (host[size_t(k)].w == host[size_t(i)].w && host[size_t(k)].h == host[size_t(i)].h && host[size_t(k)].pitch == host[size_t(i)].pitch) order.push_back(k);
    }
    for (int k : order) table.push_back(SensorPtrs{host[size_t(k)].src, host[size_t(k)].dst});
    const size_t bytes = table.size() * sizeof(SensorPtrs);
    DVO_HIP_TRY(ctx, ctx->colour_tbl.reserve(bytes));
    DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->colour_tbl.p, table.data(), bytes));
    for (size_t at = 0; at < order.size();) {
      const ColourPlane& first = host[size_t(order[at])];
      SensorArgs a;
      a.w = first.w;
      a.h = first.h;
      a.pitch = first.pitch;
      a.format = pixel_format;
      a.src_dwords = 1;
      a.dst_wide = a.w % 4 == 0 ? 1 : 0;
      size_t end = at;
      for (; end < order.size(); ++end) {
        const ColourPlane& p = host[size_t(order[end])];
        if (p.w != a.w || p.h != a.h || p.pitch != a.pitch) break;
        if (!sensor_src_dwords(p.src, size_t(p.pitch))) a.src_dwords = 0;
        if (!aligned_to(p.dst, 16)) a.dst_wide = 0;
      }
      launch_sensor_convert(ctx->stream, ctx->colour_tbl.as<SensorPtrs>() + at, int(end - at), a, /*packed=*/true, 0, false);
      at = end;
    }
  } else {
    rc = upload_block_table(ctx, ctx->colour_tbl, host, at_block);
    if (rc != DVO_HIP_OK) return rc;
    launch_colour_pack(ctx->stream, ctx->colour_tbl.as<ColourPlane>(), n_frames, at_block, pixel_format);
  }
  DVO_HIP_TRY(ctx, hipGetLastError());
  // the caller's memory, host or device, may be reused when the call returns
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < n_frames; ++i) frames[i]->colour_on = true;
  return DVO_HIP_OK;
}

int dvo_hip_frames_clear_colour(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames) {
  DVO_ENTER(ctx);
  const int rc = check_frame_list(ctx, n_frames, frames, "frames_clear_colour", /*own_context=*/true);
  if (rc != DVO_HIP_OK) return rc;
  for (int i = 0; i < n_frames; ++i) frames[i]->colour_on = false;   // (the plane is kept for the next colour)
  return DVO_HIP_OK;
}

int dvo_hip_frame_download_colour(dvo_hip_context* ctx, dvo_hip_frame* frame, int level, uint32_t* out) {
  DVO_ENTER(ctx);
  const char* who = "frame_download_colour";
  dvo_hip_frame* one[1] = {frame};
  const int rc = check_frame_list(ctx, frame ? 1 : 0, one, who, /*own_context=*/true);
  if (rc != DVO_HIP_OK) return rc;
  if (!out) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (level < 0 || level >= frame->levels) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the frame does not have that level");
  if (!frame->colour_on) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the frame carries no colour (dvo_hip_frames_set_colour)");
  const int w = frame->lv[level].w, h = frame->lv[level].h;
  if (w != frame->lv[0].w >> level || h != frame->lv[0].h >> level)
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "the level is not level 0 halved (cloud_colour.h)");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t bytes = size_t(w) * size_t(h) * 4;
  DVO_HIP_TRY(ctx, ctx->result_stage.reserve(bytes));
  launch_colour_level(ctx->stream, frame->colour.as<uint32_t>(), frame->lv[0].w, level, w, h, ctx->result_stage.as<uint32_t>());
  DVO_HIP_TRY(ctx, hipGetLastError());
  DVO_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->result_stage.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}
