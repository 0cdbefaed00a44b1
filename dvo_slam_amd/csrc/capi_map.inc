// capi_map.inc -- the keyframe map behind the C-ABI (include/dvo_hip.h, dvo_hip_map_* and dvo_hip_frames_world_points; semantics:
// cloud_map.h; kernels: cloud_map.hip).  Every launch runs on the context's main stream, behind the build-stream work that wrote the frames
// and behind every recorded ingest, as a match does; arguments are checked before anything is launched or changed.  Textually included
// by capi.hip inside its extern "C" block.
struct dvo_hip_map {
  dvo_hip_context* ctx = nullptr;
  float leaf = 0.0f;
  size_t capacity = 0;                 // slots, a power of two
  DevBuf slots, counters;
  DevBuf colour;                       // a coloured map (DVO_HIP_MAP_COLOUR): the side table, capacity * sizeof(MapColourSlot); else empty
  bool coloured = false;
  DevBuf normals;                      // a map with normals (DVO_HIP_MAP_NORMALS): the side table, capacity * sizeof(MapNormalSlot); else empty
  bool with_normals = false;
  // kMapCntCandidates, kMapCntDropped and kMapCntUnmatched as last read back (zero after a clear)
  unsigned long long candidates = 0, dropped = 0, unmatched = 0;
};
static_assert(sizeof(struct dvo_hip_map_stats) == 128 && offsetof(struct dvo_hip_map_stats, reserved) == 88, "dvo_hip_map_stats: 11 fields and 5 reserved words");

namespace {

MapTable map_table(const dvo_hip_map* map) {
  MapTable t;
  t.slots = map->slots.as<MapSlot>();
  t.counters = map->counters.as<unsigned long long>();
  t.capacity = map->capacity;
  t.leaf = map->leaf;
  t.colour = map->coloured ? map->colour.as<MapColourSlot>() : nullptr;
  t.normals = map->with_normals ? map->normals.as<MapNormalSlot>() : nullptr;
  return t;
}

// frames, poses, level and depth range of a keyframe-map call; `who` names the entry point in the error text
int check_map_frames(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const double* poses, int level, float min_depth,
                     float max_depth, const char* who, int entries_per_frame = 1) {
  int rc = check_frame_count(ctx, n_frames, frames, who, poses != nullptr);
  if (rc == DVO_HIP_OK) rc = check_range_and_reserved(ctx, min_depth, max_depth, nullptr, 0, who);
  if (rc != DVO_HIP_OK) return rc;
  return check_frames_at_level(ctx, n_frames, frames, level, entries_per_frame, kMaxBlocks, /*budget_early=*/false, who);
}

// ... and, for a coloured map, that every frame carries colour and that its level is level 0 halved (cloud_colour.h: every block lies inside)
int check_map_colour(dvo_hip_context* ctx, const dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, int level, const char* who) {
  if (!map->coloured) return DVO_HIP_OK;                       // (a grey map ignores attached colour)
  for (int i = 0; i < n_frames; ++i) {
    const dvo_hip_frame* f = frames[i];
    if (!f->colour_on) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a coloured map takes frames that carry colour (dvo_hip_frames_set_colour)");
    if (f->lv[level].w != f->lv[0].w >> level || f->lv[level].h != f->lv[0].h >> level)
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "the level is not level 0 halved (cloud_colour.h)");
  }
  return DVO_HIP_OK;
}

// (only k_map_insert moves the candidates, the dropped and the unmatched points, and every insert, remove and move ends with this read:
// the map's copy of them is current)
int read_map_counters(dvo_hip_context* ctx, dvo_hip_map* map, unsigned long long out[kMapCounters]) {
  DVO_HIP_TRY(ctx, hipMemcpyAsync(out, map->counters.p, sizeof(unsigned long long) * kMapCounters, hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  map->candidates = out[kMapCntCandidates];
  map->dropped = out[kMapCntDropped];
  map->unmatched = out[kMapCntUnmatched];
  return DVO_HIP_OK;
}

int check_map(dvo_hip_context* ctx, const dvo_hip_map* map, const char* who) {
  if (!ctx || !map) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (map->ctx != ctx) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a map of another context");
  return DVO_HIP_OK;
}

}  // namespace

int dvo_hip_map_create(dvo_hip_context* ctx, float leaf, size_t capacity_slots, dvo_hip_map** out) {
  return dvo_hip_map_create_ex(ctx, leaf, capacity_slots, 0u, out);
}

int dvo_hip_map_create_ex(dvo_hip_context* ctx, float leaf, size_t capacity_slots, unsigned flags, dvo_hip_map** out) {
  DVO_LOCK(ctx);
  if (!ctx || !out) return fail(ctx, DVO_HIP_ERR_INVALID, "map_create: bad argument");
  *out = nullptr;
  if (flags & ~(DVO_HIP_MAP_COLOUR | DVO_HIP_MAP_NORMALS)) return fail(ctx, DVO_HIP_ERR_INVALID, "map_create: unknown flag");
  if (!(leaf > 0.0f && leaf < INFINITY)) return fail(ctx, DVO_HIP_ERR_INVALID, "map_create: the leaf size must be finite and > 0");
  if (capacity_slots > (size_t(1) << 32)) return fail(ctx, DVO_HIP_ERR_INVALID, "map_create: at most 2^32 slots");
  size_t capacity = 64;
  while (capacity < capacity_slots) capacity *= 2;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  dvo_hip_map* map = new dvo_hip_map();
  map->ctx = ctx;
  map->leaf = leaf;
  map->capacity = capacity;
  map->coloured = (flags & DVO_HIP_MAP_COLOUR) != 0;
  map->with_normals = (flags & DVO_HIP_MAP_NORMALS) != 0;
  hipError_t e = map->slots.reserve(capacity * sizeof(MapSlot));
  if (e == hipSuccess && map->coloured) e = map->colour.reserve(capacity * sizeof(MapColourSlot));
  if (e == hipSuccess && map->with_normals) e = map->normals.reserve(capacity * sizeof(MapNormalSlot));
  if (e == hipSuccess) e = map->counters.reserve(sizeof(unsigned long long) * kMapCounters);
  if (e == hipSuccess) {
    launch_map_clear(ctx->stream, map_table(map));
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    map->slots.release();
    map->colour.release();
    map->normals.release();
    map->counters.release();
    delete map;
    ctx->err = std::string("map_create: ") + hipGetErrorString(e);
    return DVO_HIP_ERR_HIP;
  }
  *out = map;
  return DVO_HIP_OK;
}

void dvo_hip_map_destroy(dvo_hip_context* ctx, dvo_hip_map* map) {
  DVO_LOCK(ctx);
  if (!map) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  map->slots.release();
  map->colour.release();
  map->normals.release();
  map->counters.release();
  delete map;
}

int dvo_hip_map_clear(dvo_hip_context* ctx, dvo_hip_map* map) {
  DVO_LOCK(ctx);
  const int rc = check_map(ctx, map, "map_clear");
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_map_clear(ctx->stream, map_table(map));
  DVO_HIP_TRY(ctx, hipGetLastError());
  map->candidates = map->dropped = map->unmatched = 0;
  return DVO_HIP_OK;
}

namespace {

// The end of every launch that writes a map (k_map_insert, k_map_merge), called right behind it: reads the counters back -- the map's copy
// of them is what they held before the launch -- books the points the launch added and dropped, and the frames it inserted and removed,
// into the context's counters, and reports dropped and unmatched points.  hint: what may differ where points found no voxel to leave.
int finish_map_write(dvo_hip_context* ctx, dvo_hip_map* map, int inserts, int removes, const char* who, const char* hint) {
  DVO_HIP_TRY(ctx, hipGetLastError());
  const unsigned long long candidates_before = map->candidates, dropped_before = map->dropped, unmatched_before = map->unmatched;
  unsigned long long after[kMapCounters];
  const int rc = read_map_counters(ctx, map, after);
  if (rc != DVO_HIP_OK) return rc;
  const unsigned long long dropped = after[kMapCntDropped] - dropped_before, unmatched = after[kMapCntUnmatched] - unmatched_before;
  ctx->map_inserts += inserts;
  ctx->map_removes += removes;
  ctx->map_points += (long long)(after[kMapCntCandidates] - candidates_before - dropped);
  ctx->map_dropped += (long long)dropped;
  if (dropped != 0) return fail(ctx, DVO_HIP_ERR_CAPACITY, who, "the table dropped points (no free slot within the probe bound); the map keeps what it took");
  if (unmatched != 0) {
    ctx->err = std::string(who) + ": " + std::to_string(unmatched) + " points found no voxel to leave (" + hint + "); the map keeps what it did";
    return DVO_HIP_ERR_INVALID;
  }
  return DVO_HIP_OK;
}

enum MapUpdateMode { kMapInsert, kMapRemove, kMapMove };

// dvo_hip_map_insert (poses: where the frames enter), dvo_hip_map_remove (poses: where they leave; both with poses_new null) and
// dvo_hip_map_move: one launch of k_map_insert, over signed entries unless every frame is inserted
int map_update(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses, const double* poses_new,
               MapUpdateMode mode, int level, float min_depth, float max_depth, const char* who) {
  const bool move = mode == kMapMove, insert = mode == kMapInsert;
  int rc = check_map(ctx, map, who);
  if (rc == DVO_HIP_OK) rc = check_map_frames(ctx, n_frames, frames, poses, level, min_depth, max_depth, who, move ? 2 : 1);
  if (rc == DVO_HIP_OK) rc = check_map_colour(ctx, map, n_frames, frames, level, who);
  if (rc != DVO_HIP_OK) return rc;
  if (move && !poses_new) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (!insert && map->dropped != 0)
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map has dropped points since its last clear or rehash: what it holds of a frame is not known (dvo_hip_map_rehash into a larger table, or dvo_hip_map_clear)");
  std::vector<FrameEntry> entries;
  int removes = 0, inserts = 0;
  for (int i = 0; i < n_frames; ++i) {
    const MapPose at = map_pose_prepare(poses + size_t(i) * 16);
    if (move) {
      const MapPose to = map_pose_prepare(poses_new + size_t(i) * 16);
      if (std::memcmp(&at, &to, sizeof at) == 0) continue;     // (the same twelve floats: the same points, nothing to do)
      entries.push_back(FrameEntry{frames[i], at, -1, nullptr});
      entries.push_back(FrameEntry{frames[i], to, 1, nullptr});
    } else {
      entries.push_back(FrameEntry{frames[i], at, insert ? 1 : -1, nullptr});
    }
    inserts += insert || move;
    removes += !insert;
  }
  if (entries.empty()) return DVO_HIP_OK;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int blocks = 0;
  rc = upload_frame_entries(ctx, entries, level, &blocks, map->coloured);
  if (rc != DVO_HIP_OK) return rc;
  launch_map_insert(ctx->stream, ctx->frame_tbl.as<MapFrame>(), int(entries.size()), blocks, map_table(map), min_depth, max_depth, /*mixed=*/!insert);
  return finish_map_write(ctx, map, inserts, removes, who, "not the frame content, level, pose or depth range of the insertion?");
}

}  // namespace

int dvo_hip_map_insert(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses, int level,
                       float min_depth, float max_depth) {
  DVO_ENTER(ctx);
  return map_update(ctx, map, n_frames, frames, poses, nullptr, kMapInsert, level, min_depth, max_depth, "map_insert");
}

int dvo_hip_map_remove(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses, int level,
                       float min_depth, float max_depth) {
  DVO_ENTER(ctx);
  return map_update(ctx, map, n_frames, frames, poses, nullptr, kMapRemove, level, min_depth, max_depth, "map_remove");
}

int dvo_hip_map_move(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses_old,
                     const double* poses_new, int level, float min_depth, float max_depth) {
  DVO_ENTER(ctx);
  return map_update(ctx, map, n_frames, frames, poses_old, poses_new, kMapMove, level, min_depth, max_depth, "map_move");
}

int dvo_hip_map_rehash(dvo_hip_context* ctx, dvo_hip_map* map, size_t capacity_slots) {
  DVO_ENTER(ctx);
  const int rc0 = check_map(ctx, map, "map_rehash");
  if (rc0 != DVO_HIP_OK) return rc0;
  const size_t capacity = capacity_slots ? capacity_slots : map->capacity;
  if (capacity < 64 || capacity > (size_t(1) << 32) || (capacity & (capacity - 1)) != 0)
    return fail(ctx, DVO_HIP_ERR_INVALID, "map_rehash: the capacity must be a power of two, 64 .. 2^32 slots (0: as it is)");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the second table and its counters: both tables exist during this call only
  DevBuf slots, counters, colour, normals;
  hipError_t e = slots.reserve(capacity * sizeof(MapSlot));
  if (e == hipSuccess && map->coloured) e = colour.reserve(capacity * sizeof(MapColourSlot));
  if (e == hipSuccess && map->with_normals) e = normals.reserve(capacity * sizeof(MapNormalSlot));
  if (e == hipSuccess) e = counters.reserve(sizeof(unsigned long long) * kMapCounters);
  unsigned long long was[kMapCounters], now[kMapCounters];
  if (e == hipSuccess) {
    MapTable to = map_table(map);
    to.slots = slots.as<MapSlot>();
    to.counters = counters.as<unsigned long long>();
    to.capacity = capacity;
    to.colour = map->coloured ? colour.as<MapColourSlot>() : nullptr;
    to.normals = map->with_normals ? normals.as<MapNormalSlot>() : nullptr;
    launch_map_rehash(ctx->stream, map_table(map), to);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(was, map->counters.p, sizeof was, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(now, counters.p, sizeof now, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  const bool fits = e == hipSuccess && now[kMapCntDropped] == 0;
  if (fits) {
    // points is unchanged (what was dropped is forgotten), occupied = the live voxels, the histories are carried over
    now[kMapCntCandidates] = was[kMapCntCandidates] - was[kMapCntDropped];
    for (int k : {kMapCntOutOfRange, kMapCntUnusable, kMapCntUpdates, kMapCntRemoving, kMapCntUnmatched}) now[k] = was[k];
    e = hipMemcpyAsync(counters.p, now, sizeof now, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  if (e != hipSuccess || !fits) {
    if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);   // (nothing still writes the table that is freed)
    slots.release();
    colour.release();
    normals.release();
    counters.release();
    if (e != hipSuccess) {
      ctx->err = std::string("map_rehash: ") + hipGetErrorString(e);
      return DVO_HIP_ERR_HIP;
    }
    ctx->err = "map_rehash: " + std::to_string(now[kMapCntDropped]) + " voxels found no slot in the new table within the probe bound; the map is unchanged";
    return DVO_HIP_ERR_CAPACITY;
  }
  std::swap(map->slots, slots);
  std::swap(map->colour, colour);
  std::swap(map->normals, normals);
  std::swap(map->counters, counters);
  slots.release();
  colour.release();
  normals.release();
  counters.release();
  map->capacity = capacity;
  map->candidates = now[kMapCntCandidates];
  map->dropped = 0;
  map->unmatched = now[kMapCntUnmatched];
  ctx->map_rehashes += 1;
  return DVO_HIP_OK;
}

int dvo_hip_map_stats(dvo_hip_context* ctx, dvo_hip_map* map, struct dvo_hip_map_stats* out) {
  DVO_LOCK(ctx);
  const int rc0 = check_map(ctx, map, "map_stats");
  if (rc0 != DVO_HIP_OK) return rc0;
  if (!out) return fail(ctx, DVO_HIP_ERR_INVALID, "map_stats: bad argument");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, launch_map_extract(ctx->stream, map_table(map), 0, nullptr, nullptr, nullptr, nullptr));   // (counts the voxels over the limit)
  DVO_HIP_TRY(ctx, hipGetLastError());
  unsigned long long c[kMapCounters];
  const int rc = read_map_counters(ctx, map, c);
  if (rc != DVO_HIP_OK) return rc;
  std::memset(out, 0, sizeof *out);
  out->occupied = c[kMapCntOccupied];
  out->removed = c[kMapCntRemoving] - c[kMapCntUnmatched];
  out->points = c[kMapCntCandidates] - c[kMapCntDropped] - out->removed;
  out->dropped = c[kMapCntDropped];
  out->out_of_range = c[kMapCntOutOfRange];
  out->unusable = c[kMapCntUnusable];
  out->over_limit = c[kMapCntOverLimit];
  out->capacity = map->capacity;
  out->updates = c[kMapCntUpdates];
  out->vacant = c[kMapCntVacant];
  out->unmatched = c[kMapCntUnmatched];
  return DVO_HIP_OK;
}

namespace {

// one output array of a read-out: the caller's array (null: not wanted) and the bytes of one record in it
struct ReadOutArray {
  void* dst;
  size_t record_bytes;
};

// The read-out of a map's live voxels on the main stream (dvo_hip_map_extract, dvo_hip_map_extract_colour, dvo_hip_map_export):
// pass(n, dev) walks the table and writes at most n records to the device arrays dev[k] (null: not wanted).  The first pass counts
// (n = 0, every array null; c: the counters behind it, c[kMapCntCursor] the live voxels), the second fills *take = min(live, max) records:
// a host destination is staged for just that many and copied out (stage_results, every array aligned to its record); one synchronise.
int map_read_out(dvo_hip_context* ctx, dvo_hip_map* map, size_t max, const std::vector<ReadOutArray>& outs, int out_on_device,
                 const std::function<hipError_t(unsigned long long, void* const*)>& pass, unsigned long long c[kMapCounters], size_t* take) {
  *take = 0;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<void*> dev(outs.size(), nullptr);
  DVO_HIP_TRY(ctx, pass(0, dev.data()));
  DVO_HIP_TRY(ctx, hipGetLastError());
  int rc = read_map_counters(ctx, map, c);
  if (rc != DVO_HIP_OK) return rc;
  const size_t n = size_t(c[kMapCntCursor] < max ? c[kMapCntCursor] : max);
  if (n == 0) return DVO_HIP_OK;
  std::vector<ResultArray> results;
  for (const ReadOutArray& o : outs) results.push_back(ResultArray{o.dst, n * o.record_bytes, o.record_bytes});
  rc = stage_results(ctx, results, out_on_device, &dev);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, pass(n, dev.data()));
  DVO_HIP_TRY(ctx, hipGetLastError());
  rc = finish_results(ctx, results, out_on_device, dev);
  if (rc != DVO_HIP_OK) return rc;
  *take = n;
  return DVO_HIP_OK;
}

// dvo_hip_map_extract (with_colour false, rgba null), dvo_hip_map_extract_colour and -- with_normals, normals the records' array; rgba
// may be given for a map that also has colour -- dvo_hip_map_extract_normals
int map_extract(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_points, float* xyzi, bool with_colour, uint32_t* rgba, uint32_t* counts_or_null,
                uint64_t* keys_or_null, int out_on_device, size_t* n_points, const char* who, bool with_normals = false, float* normals = nullptr) {
  const int rc0 = check_map(ctx, map, who);
  if (rc0 != DVO_HIP_OK) return rc0;
  if (with_normals && !map->with_normals) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map holds no normals (dvo_hip_map_create_ex, DVO_HIP_MAP_NORMALS)");
  if ((with_colour || rgba) && !map->coloured) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map holds no colour (dvo_hip_map_create_ex, DVO_HIP_MAP_COLOUR)");
  if (!n_points || (max_points > 0 && (!xyzi || (with_colour && !rgba) || (with_normals && !normals)))) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (out_on_device && normals && reinterpret_cast<uintptr_t>(normals) % 16 != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a device normals array must be 16-byte aligned");
  if (out_on_device && xyzi && reinterpret_cast<uintptr_t>(xyzi) % 16 != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a device xyzi must be 16-byte aligned");
  if (out_on_device && rgba && reinterpret_cast<uintptr_t>(rgba) % 4 != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a device rgba must be 4-byte aligned");
  const MapTable t = map_table(map);
  unsigned long long c[kMapCounters];
  const int rc = map_read_out(ctx, map, max_points, {{xyzi, 16}, {normals, 16}, {keys_or_null, 8}, {counts_or_null, 4}, {rgba, 4}}, out_on_device,
                              [&](unsigned long long n, void* const* dev) {
                                return launch_map_extract(ctx->stream, t, n, static_cast<float4*>(dev[0]), static_cast<uint32_t*>(dev[3]),
                                                          static_cast<unsigned long long*>(dev[2]), static_cast<uint32_t*>(dev[4]),
                                                          static_cast<float4*>(dev[1]));
                              },
                              c, n_points);
  if (rc != DVO_HIP_OK) return rc;
  if (c[kMapCntCursor] > max_points) return fail(ctx, DVO_HIP_ERR_CAPACITY, who, "max_points is smaller than the number of occupied voxels (dvo_hip_map_stats)");
  if (c[kMapCntOverLimit] != 0) return fail(ctx, DVO_HIP_ERR_CAPACITY, who, "a voxel holds more than 2^20 points; its sums may have wrapped");
  return DVO_HIP_OK;
}

}  // namespace

int dvo_hip_map_extract(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_points, float* xyzi, uint32_t* counts_or_null, uint64_t* keys_or_null,
                        int out_on_device, size_t* n_points) {
  DVO_LOCK(ctx);
  return map_extract(ctx, map, max_points, xyzi, false, nullptr, counts_or_null, keys_or_null, out_on_device, n_points, "map_extract");
}

int dvo_hip_map_extract_colour(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_points, float* xyzi, uint32_t* rgba, uint32_t* counts_or_null,
                               uint64_t* keys_or_null, int out_on_device, size_t* n_points) {
  DVO_LOCK(ctx);
  return map_extract(ctx, map, max_points, xyzi, true, rgba, counts_or_null, keys_or_null, out_on_device, n_points, "map_extract_colour");
}

// ---- sub-maps: voxel tables and raw voxel records into and out of a map (cloud_map.h, Merge; kernels: map_merge.hip) ----

namespace {

// one source of a merge: a table or a record array in device memory, its leaf, and how it enters
struct MergeSource {
  const MapSlot* slots;
  const MapColourSlot* colour;
  const MapNormalSlot* normals;
  unsigned long long count;
  float leaf;
  int sign;
  MapPose pose;
  const dvo_hip_map* map;              // the map the records are the table of: a PLAIN merge carries its out-of-range and unusable counts along; else null
};

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// what every merge checks of one source once its pointers are known to be good: the sign, the leaf, the pose
int check_merge_source(dvo_hip_context* ctx, const dvo_hip_map* dst, float leaf_src, int sign, const double* pose_or_null, const char* who) {
  if (sign != 1 && sign != -1) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a sign is +1 or -1");
  if (!(leaf_src > 0.0f && leaf_src < INFINITY)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the source's leaf size must be finite and > 0");
  if (!pose_or_null && !same_bits(leaf_src, dst->leaf))
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "a plain merge adds voxels as they are: the source's leaf must be the destination's (a posed merge bins anew)");
  if (pose_or_null && !transforms_finite(pose_or_null, 1)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a pose has an entry that is not finite");
  if (sign < 0 && dst->dropped != 0)
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map has dropped points since its last clear or rehash: what it holds of a sub-map is not known (dvo_hip_map_rehash into a larger table, or dvo_hip_map_clear)");
  return DVO_HIP_OK;
}

// a source map of dvo_hip_map_merge / dvo_hip_map_move_submaps
int check_merge_map(dvo_hip_context* ctx, const dvo_hip_map* dst, const dvo_hip_map* src, const char* who) {
  if (!src) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null source map");
  if (src->ctx != ctx) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a source map of another context (dvo_hip_map_export there, dvo_hip_map_merge_records here)");
  if (src == dst) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a map cannot be merged into itself");
  if (src->coloured != dst->coloured) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a coloured and a grey map do not merge");
  if (src->with_normals != dst->with_normals) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a map with normals and one without do not merge");
  return DVO_HIP_OK;
}

MergeSource merge_source_of(const dvo_hip_map* src, int sign, const double* pose_or_null) {
  MergeSource s;
  s.slots = src->slots.as<MapSlot>();
  s.colour = src->coloured ? src->colour.as<MapColourSlot>() : nullptr;
  s.normals = src->with_normals ? src->normals.as<MapNormalSlot>() : nullptr;
  s.count = src->capacity;
  s.leaf = src->leaf;
  s.sign = sign;
  std::memset(&s.pose, 0, sizeof s.pose);
  if (pose_or_null) s.pose = map_pose_prepare(pose_or_null);
  s.map = pose_or_null ? nullptr : src;
  return s;
}

// One launch of k_map_merge over checked sources (all posed or all plain) on the main stream, then the read-back of the counters.
int run_map_merge(dvo_hip_context* ctx, dvo_hip_map* dst, const std::vector<MergeSource>& sources, bool posed, const char* who) {
  if (sources.empty()) return DVO_HIP_OK;
  long long blocks = 0;
  for (const MergeSource& s : sources) blocks += (long long)((s.count + 255) / 256);
  if (blocks > 0x7fffffffll) return fail(ctx, DVO_HIP_ERR_INVALID, who, "too many records for one call");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the counts a plain merge carries along from its source maps
  std::vector<unsigned long long> theirs(sources.size() * size_t(kMapCounters), 0ull);
  bool any = false;
  for (size_t i = 0; i < sources.size(); ++i)
    if (sources[i].map) {
      DVO_HIP_TRY(ctx, hipMemcpyAsync(&theirs[i * kMapCounters], sources[i].map->counters.p, sizeof(unsigned long long) * kMapCounters,
                                      hipMemcpyDeviceToHost, ctx->stream));
      any = true;
    }
  if (any) DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<MapMergeEntry> host(sources.size() + 1);
  std::memset(host.data(), 0, host.size() * sizeof(MapMergeEntry));
  int at = 0;
  for (size_t i = 0; i < sources.size(); ++i) {
    const MergeSource& s = sources[i];
    MapMergeEntry& e = host[i];
    e.slots = s.slots;
    e.colour = dst->coloured ? s.colour : nullptr;
    e.normals = dst->with_normals ? s.normals : nullptr;
    e.count = s.count;
    const unsigned long long oor = theirs[i * kMapCounters + kMapCntOutOfRange], unusable = theirs[i * kMapCounters + kMapCntUnusable];
    e.out_of_range = s.sign < 0 ? 0ull - oor : oor;
    e.unusable = s.sign < 0 ? 0ull - unusable : unusable;
    e.pose = s.pose;
    e.leaf_src = s.leaf;
    e.sign = s.sign;
    e.first_block = at;
    at += int((s.count + 255) / 256);
  }
  const int rc = upload_block_table(ctx, ctx->frame_tbl, host, at);
  if (rc != DVO_HIP_OK) return rc;
  launch_map_merge(ctx->stream, ctx->frame_tbl.as<MapMergeEntry>(), int(sources.size()), at, map_table(dst), posed);
  return finish_map_write(ctx, dst, 0, 0, who, "not the sub-map, or not the pose, that was merged?");
}

}  // namespace
static_assert(sizeof(MapSlot) == 32 && sizeof(MapColourSlot) == 16 && sizeof(MapNormalSlot) == 16,
              "a voxel record is 32 bytes, its colour record and its normal record 16 each (include/dvo_hip.h)");

int dvo_hip_map_info(dvo_hip_context* ctx, dvo_hip_map* map, float* leaf, unsigned* flags, uint64_t* capacity) {
  DVO_LOCK(ctx);
  const int rc = check_map(ctx, map, "map_info");
  if (rc != DVO_HIP_OK) return rc;
  if (leaf) *leaf = map->leaf;
  if (flags) *flags = (map->coloured ? DVO_HIP_MAP_COLOUR : 0u) | (map->with_normals ? DVO_HIP_MAP_NORMALS : 0u);
  if (capacity) *capacity = map->capacity;
  return DVO_HIP_OK;
}

int dvo_hip_map_merge(dvo_hip_context* ctx, dvo_hip_map* dst, int n_src, dvo_hip_map* const* src, const int* signs_or_null, const double* poses_or_null) {
  DVO_LOCK(ctx);
  const char* who = "map_merge";
  int rc = check_map(ctx, dst, who);
  if (rc != DVO_HIP_OK) return rc;
  if (n_src < 0 || (n_src > 0 && !src)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  std::vector<MergeSource> sources;
  for (int i = 0; i < n_src; ++i) {
    const double* pose = poses_or_null ? poses_or_null + size_t(i) * 16 : nullptr;
    const int sign = signs_or_null ? signs_or_null[i] : 1;
    rc = check_merge_map(ctx, dst, src[i], who);
    if (rc == DVO_HIP_OK) rc = check_merge_source(ctx, dst, src[i]->leaf, sign, pose, who);
    if (rc != DVO_HIP_OK) return rc;
    sources.push_back(merge_source_of(src[i], sign, pose));
  }
  return run_map_merge(ctx, dst, sources, poses_or_null != nullptr, who);
}

int dvo_hip_map_move_submaps(dvo_hip_context* ctx, dvo_hip_map* dst, int n_src, dvo_hip_map* const* src, const double* poses_old,
                             const double* poses_new) {
  DVO_LOCK(ctx);
  const char* who = "map_move_submaps";
  int rc = check_map(ctx, dst, who);
  if (rc != DVO_HIP_OK) return rc;
  if (n_src < 0 || (n_src > 0 && (!src || !poses_old || !poses_new))) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  std::vector<MergeSource> sources;
  for (int i = 0; i < n_src; ++i) {
    const double *from = poses_old + size_t(i) * 16, *to = poses_new + size_t(i) * 16;
    rc = check_merge_map(ctx, dst, src[i], who);
    if (rc == DVO_HIP_OK) rc = check_merge_source(ctx, dst, src[i]->leaf, -1, from, who);
    if (rc == DVO_HIP_OK) rc = check_merge_source(ctx, dst, src[i]->leaf, 1, to, who);
    if (rc != DVO_HIP_OK) return rc;
    const MergeSource out = merge_source_of(src[i], -1, from), in = merge_source_of(src[i], 1, to);
    if (std::memcmp(&out.pose, &in.pose, sizeof out.pose) == 0) continue;   // (the same twelve floats: the same records, nothing to do)
    sources.push_back(out);
    sources.push_back(in);
  }
  return run_map_merge(ctx, dst, sources, true, who);
}

namespace {

// dvo_hip_map_export (normal_records null) and dvo_hip_map_export_ex
int map_export(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_records, void* records, void* colour_records_or_null, void* normal_records_or_null,
               int out_on_device, size_t* n_records, const char* who) {
  const int rc0 = check_map(ctx, map, who);
  if (rc0 != DVO_HIP_OK) return rc0;
  if (!n_records || (max_records > 0 && !records)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (colour_records_or_null && !map->coloured) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map holds no colour (dvo_hip_map_create_ex, DVO_HIP_MAP_COLOUR)");
  if (normal_records_or_null && !map->with_normals) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map holds no normals (dvo_hip_map_create_ex, DVO_HIP_MAP_NORMALS)");
  if (out_on_device && ((records && !aligned_to(records, 16)) || (colour_records_or_null && !aligned_to(colour_records_or_null, 16)) ||
                        (normal_records_or_null && !aligned_to(normal_records_or_null, 16))))
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "device records must be 16-byte aligned");
  const MapTable t = map_table(map);
  unsigned long long c[kMapCounters];
  const int rc = map_read_out(ctx, map, max_records,
                              {{records, sizeof(MapSlot)}, {colour_records_or_null, sizeof(MapColourSlot)}, {normal_records_or_null, sizeof(MapNormalSlot)}},
                              out_on_device,
                              [&](unsigned long long n, void* const* dev) {
                                return launch_map_export(ctx->stream, t, n, static_cast<MapSlot*>(dev[0]), static_cast<MapColourSlot*>(dev[1]),
                                                         static_cast<MapNormalSlot*>(dev[2]));
                              },
                              c, n_records);
  if (rc != DVO_HIP_OK) return rc;
  if (!records) {                                            // (max_records is 0: the caller asks how many there are)
    *n_records = size_t(c[kMapCntCursor]);
    return DVO_HIP_OK;
  }
  if (c[kMapCntCursor] > max_records) return fail(ctx, DVO_HIP_ERR_CAPACITY, who, "max_records is smaller than the number of live voxels (dvo_hip_map_stats: occupied - vacant)");
  return DVO_HIP_OK;
}

}  // namespace

int dvo_hip_map_export(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_records, void* records, void* colour_records_or_null, int out_on_device,
                       size_t* n_records) {
  DVO_LOCK(ctx);
  return map_export(ctx, map, max_records, records, colour_records_or_null, nullptr, out_on_device, n_records, "map_export");
}

int dvo_hip_map_export_ex(dvo_hip_context* ctx, dvo_hip_map* map, size_t max_records, void* records, void* colour_records_or_null,
                          void* normal_records_or_null, int out_on_device, size_t* n_records) {
  DVO_LOCK(ctx);
  return map_export(ctx, map, max_records, records, colour_records_or_null, normal_records_or_null, out_on_device, n_records, "map_export_ex");
}

namespace {

// dvo_hip_map_merge_records (normals null: refused by a destination with normals, which it cannot supply) and dvo_hip_map_merge_records_ex
int map_merge_records(dvo_hip_context* ctx, dvo_hip_map* dst, size_t n_records, const void* records, const void* colour_or_null, const void* normals_or_null,
                      int on_device, float leaf_src, int sign, const double* pose_or_null, const char* who) {
  int rc = check_map(ctx, dst, who);
  if (rc != DVO_HIP_OK) return rc;
  if (dst->with_normals && n_records > 0 && !normals_or_null)
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "a map with normals takes records with normal records (dvo_hip_map_merge_records_ex)");
  if (!dst->with_normals && normals_or_null) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a map without normals takes no normal records");
  if (n_records > (size_t(1) << 32)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "at most 2^32 records");
  if (n_records > 0 && !records) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (dst->coloured && n_records > 0 && !colour_or_null) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a coloured map takes records with colour records");
  if (!dst->coloured && colour_or_null) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a grey map takes no colour records");
  if (on_device && ((records && !aligned_to(records, 16)) || (colour_or_null && !aligned_to(colour_or_null, 16)) ||
                    (normals_or_null && !aligned_to(normals_or_null, 16))))
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "device records must be 16-byte aligned");
  rc = check_merge_source(ctx, dst, leaf_src, sign, pose_or_null, who);
  if (rc != DVO_HIP_OK) return rc;
  if (n_records == 0) return DVO_HIP_OK;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MergeSource s;
  s.slots = static_cast<const MapSlot*>(records);
  s.colour = static_cast<const MapColourSlot*>(colour_or_null);
  s.normals = static_cast<const MapNormalSlot*>(normals_or_null);
  if (!on_device) {
    // host records: staged on the main stream, then the same kernel
    DVO_HIP_TRY(ctx, ctx->result_stage.reserve(n_records * (sizeof(MapSlot) + sizeof(MapColourSlot) + sizeof(MapNormalSlot))));
    char* stage = ctx->result_stage.as<char>();
    DVO_HIP_TRY(ctx, hipMemcpyAsync(stage, records, n_records * sizeof(MapSlot), hipMemcpyHostToDevice, ctx->stream));
    s.slots = reinterpret_cast<const MapSlot*>(stage);
    if (colour_or_null) {
      DVO_HIP_TRY(ctx, hipMemcpyAsync(stage + n_records * sizeof(MapSlot), colour_or_null, n_records * sizeof(MapColourSlot), hipMemcpyHostToDevice, ctx->stream));
      s.colour = reinterpret_cast<const MapColourSlot*>(stage + n_records * sizeof(MapSlot));
    }
    if (normals_or_null) {
      char* at = stage + n_records * (sizeof(MapSlot) + sizeof(MapColourSlot));
      DVO_HIP_TRY(ctx, hipMemcpyAsync(at, normals_or_null, n_records * sizeof(MapNormalSlot), hipMemcpyHostToDevice, ctx->stream));
      s.normals = reinterpret_cast<const MapNormalSlot*>(at);
    }
  }
  s.count = n_records;
  s.leaf = leaf_src;
  s.sign = sign;
  std::memset(&s.pose, 0, sizeof s.pose);
  if (pose_or_null) s.pose = map_pose_prepare(pose_or_null);
  s.map = nullptr;
  return run_map_merge(ctx, dst, std::vector<MergeSource>(1, s), pose_or_null != nullptr, who);
}

}  // namespace

int dvo_hip_map_merge_records(dvo_hip_context* ctx, dvo_hip_map* dst, size_t n_records, const void* records, const void* colour_or_null, int on_device,
                              float leaf_src, int sign, const double* pose_or_null) {
  DVO_LOCK(ctx);
  return map_merge_records(ctx, dst, n_records, records, colour_or_null, nullptr, on_device, leaf_src, sign, pose_or_null, "map_merge_records");
}

int dvo_hip_map_merge_records_ex(dvo_hip_context* ctx, dvo_hip_map* dst, size_t n_records, const void* records, const void* colour_or_null,
                                 const void* normals_or_null, int on_device, float leaf_src, int sign, const double* pose_or_null) {
  DVO_LOCK(ctx);
  return map_merge_records(ctx, dst, n_records, records, colour_or_null, normals_or_null, on_device, leaf_src, sign, pose_or_null, "map_merge_records_ex");
}

namespace {

// dvo_hip_frames_world_points and -- normals: k_frame_normals in place of k_world_points -- dvo_hip_frames_normals: one 16-byte record per
// pixel of every frame's level
int frames_organised(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const double* poses, int level, float min_depth,
                     float max_depth, float* const* out, int out_on_device, bool normals, const char* who) {
  int rc = check_map_frames(ctx, n_frames, frames, poses, level, min_depth, max_depth, who);
  if (rc != DVO_HIP_OK) return rc;
  if (!out) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  const std::vector<ResultArray> results = frame_planes(n_frames, frames, level, &out, 1, 16);
  rc = check_results(ctx, results, out_on_device, who, "null output", "a device output must be 16-byte aligned");
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<void*> dev;
  rc = stage_results(ctx, results, out_on_device, &dev);
  int blocks = 0;
  if (rc == DVO_HIP_OK) rc = upload_frames(ctx, n_frames, frames, poses, level, dev.data(), &blocks);
  if (rc != DVO_HIP_OK) return rc;
  if (normals) launch_frame_normals(ctx->stream, ctx->frame_tbl.as<MapFrame>(), n_frames, blocks, min_depth, max_depth);
  else launch_world_points(ctx->stream, ctx->frame_tbl.as<MapFrame>(), n_frames, blocks, min_depth, max_depth);
  DVO_HIP_TRY(ctx, hipGetLastError());
  return finish_results(ctx, results, out_on_device, dev);
}

}  // namespace

int dvo_hip_frames_world_points(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const double* poses, int level, float min_depth,
                                float max_depth, float* const* out, int out_on_device) {
  DVO_ENTER(ctx);
  return frames_organised(ctx, n_frames, frames, poses, level, min_depth, max_depth, out, out_on_device, false, "frames_world_points");
}

// ---- views of the map (map_render.h; kernels: map_render.hip) ----

namespace {

// params (null: the defaults), size, K and poses of a render; *args = what the kernels take
int check_render(dvo_hip_context* ctx, const dvo_hip_map* map, int n_views, int width, int height, const float* K, const double* poses,
                 const dvo_hip_render_params* params, RenderArgs* args, const char* who) {
  const int rc = check_map(ctx, map, who);
  if (rc != DVO_HIP_OK) return rc;
  if (n_views < 1 || !K || !poses) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (width < 1 || height < 1 || width > (1 << 24) || height > (1 << 24) || (long long)width * height * n_views > 0x7fffffffll)
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "need a positive size of at most 2^24 a side and 2^31 - 1 pixels in all views");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(K[k])) return fail(ctx, DVO_HIP_ERR_INVALID, who, "K must be finite");
  if (!(K[0] > 0.0f && K[1] > 0.0f)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "need fx > 0 and fy > 0");
  const dvo_hip_render_params p = params ? *params : dvo_hip_render_params_default();
  if (!(p.min_depth <= p.max_depth)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "need min_depth <= max_depth (no NaN)");
  if (!(p.splat > 0.0f && p.splat <= 4.0f)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "splat must lie in (0, 4]");
  if (p.max_splat < 1 || p.max_splat > kRenderMaxSplat || p.max_splat % 2 == 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "max_splat must be odd, 1 .. 15");
  if (p.min_points < 1) return fail(ctx, DVO_HIP_ERR_INVALID, who, "min_points must be at least 1");
  if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a reserved field is not 0");
  args->min_depth = p.min_depth;
  args->max_depth = p.max_depth;
  args->splat = p.splat;
  args->leaf = map->leaf;
  args->max_splat = p.max_splat;
  args->min_points = p.min_points;
  return DVO_HIP_OK;
}

// the view table of a render on the main stream: n MapView, then n RenderPlanes (view i writes planes[2 i] and, its depth, planes[2 i + 1]);
// and the z-buffers
int upload_views(dvo_hip_context* ctx, int n_views, int width, int height, const float* K, const double* poses, void* const* planes) {
  const size_t views_bytes = size_t(n_views) * sizeof(MapView), bytes = views_bytes + size_t(n_views) * sizeof(RenderPlanes);
  std::vector<char> host(bytes);
  for (int i = 0; i < n_views; ++i) {
    const MapView v = map_view_prepare(poses + size_t(i) * 16, K, width, height);
    const RenderPlanes o = {static_cast<float*>(planes[2 * i]), static_cast<float*>(planes[2 * i + 1])};
    std::memcpy(host.data() + size_t(i) * sizeof(MapView), &v, sizeof v);
    std::memcpy(host.data() + views_bytes + size_t(i) * sizeof(RenderPlanes), &o, sizeof o);
  }
  DVO_HIP_TRY(ctx, ctx->side_tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->side_tbl.p, host.data(), bytes));
  DVO_HIP_TRY(ctx, ctx->scratch_words.reserve(size_t(n_views) * size_t(width) * size_t(height) * sizeof(unsigned long long)));
  return DVO_HIP_OK;
}

// n pairs of planes of `plane` bytes each in one block of the context, (re)allocated here: pair i's first plane is planes[2 i], its second behind it
int reserve_plane_pairs(dvo_hip_context* ctx, DevBuf& block, size_t plane, int n, std::vector<void*>* planes) {
  DVO_HIP_TRY(ctx, block.reserve(plane * 2 * size_t(n)));
  for (size_t k = 0; k < 2 * size_t(n); ++k) planes->push_back(block.as<char>() + plane * k);
  return DVO_HIP_OK;
}

const MapView* render_views(const dvo_hip_context* ctx) { return ctx->side_tbl.as<MapView>(); }
const RenderPlanes* render_outs(const dvo_hip_context* ctx, int n_views) {
  return reinterpret_cast<const RenderPlanes*>(ctx->side_tbl.as<char>() + size_t(n_views) * sizeof(MapView));
}

}  // namespace
static_assert(sizeof(dvo_hip_render_params) == 32, "dvo_hip_render_params: five fields and three reserved words");
static_assert(sizeof(MapView) % alignof(RenderPlanes) == 0, "the planes' table lies behind the views");

dvo_hip_render_params dvo_hip_render_params_default(void) {
  dvo_hip_render_params p;
  std::memset(&p, 0, sizeof p);
  p.min_depth = 0.0f;
  p.max_depth = INFINITY;
  p.splat = 2.0f;
  p.max_splat = 7;
  p.min_points = 1;
  return p;
}

namespace {

// dvo_hip_map_render (first_out: float intensity planes), -- colour -- dvo_hip_map_render_colour (first_out: uint32 rgba planes) and
// -- normals -- dvo_hip_map_render_normals (first_out: planes of 16-byte records)
int map_render(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float* K, const double* poses,
               const dvo_hip_render_params* params, bool colour, void* const* first_out, float* const* depth_out, int out_on_device, const char* who,
               bool normals = false) {
  RenderArgs args;
  int rc = check_render(ctx, map, n_views, width, height, K, poses, params, &args, who);
  if (rc != DVO_HIP_OK) return rc;
  if (colour && !map->coloured) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map holds no colour (dvo_hip_map_create_ex, DVO_HIP_MAP_COLOUR)");
  if (normals && !map->with_normals) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the map holds no normals (dvo_hip_map_create_ex, DVO_HIP_MAP_NORMALS)");
  if (!first_out || !depth_out) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  const size_t pixels = size_t(width) * size_t(height);
  // (RenderPlanes::I holds the address of the uint32 rgba plane of a colour view: k_render_resolve stores the bits as they are; of a
  // normals view the address of the plane of 16-byte records)
  std::vector<ResultArray> results;
  for (int i = 0; i < n_views; ++i) {
    results.push_back(ResultArray{first_out[i], pixels * (normals ? 16 : 4), 16});
    results.push_back(ResultArray{depth_out[i], pixels * 4, 16});
  }
  rc = check_results(ctx, results, out_on_device, who, "null output", "a device plane must be 16-byte aligned", /*group=*/2);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<void*> dev;
  rc = stage_results(ctx, results, out_on_device, &dev);
  if (rc == DVO_HIP_OK) rc = upload_views(ctx, n_views, width, height, K, poses, dev.data());
  if (rc != DVO_HIP_OK) return rc;
  if (normals)
    launch_map_render_normals(ctx->stream, map_table(map), render_views(ctx), render_outs(ctx, n_views), n_views, (long long)pixels, args,
                              ctx->scratch_words.as<unsigned long long>());
  else
    launch_map_render(ctx->stream, map_table(map), render_views(ctx), render_outs(ctx, n_views), n_views, (long long)pixels, args,
                      ctx->scratch_words.as<unsigned long long>(), colour);
  DVO_HIP_TRY(ctx, hipGetLastError());
  ctx->map_renders += n_views;
  return out_on_device ? DVO_HIP_OK : finish_results(ctx, results, out_on_device, dev);   // (device planes are not waited for)
}

}  // namespace

int dvo_hip_map_render(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4], const double* poses,
                       const dvo_hip_render_params* params, float* const* intensity_out, float* const* depth_out, int out_on_device) {
  DVO_ENTER(ctx);
  return map_render(ctx, map, n_views, width, height, K, poses, params, false, reinterpret_cast<void* const*>(intensity_out), depth_out, out_on_device,
                    "map_render");
}

int dvo_hip_map_render_colour(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4], const double* poses,
                              const dvo_hip_render_params* params, uint32_t* const* rgba_out, float* const* depth_out, int out_on_device) {
  DVO_ENTER(ctx);
  return map_render(ctx, map, n_views, width, height, K, poses, params, true, reinterpret_cast<void* const*>(rgba_out), depth_out, out_on_device,
                    "map_render_colour");
}

int dvo_hip_map_render_frames(dvo_hip_context* ctx, dvo_hip_map* map, int n_frames, dvo_hip_frame* const* frames, const double* poses,
                              const dvo_hip_render_params* params, int role, const dvo_hip_config* cfg, unsigned flags) {
  DVO_ENTER(ctx);
  const char* who = "map_render_frames";
  int rc = check_map(ctx, map, who);
  if (rc != DVO_HIP_OK) return rc;
  rc = check_frame_count(ctx, n_frames, frames, who, poses != nullptr);
  if (rc != DVO_HIP_OK) return rc;
  if (flags & DVO_HIP_INGEST_DEFER) return fail(ctx, DVO_HIP_ERR_INVALID, who, "DVO_HIP_INGEST_DEFER: a render is not recorded");
  rc = check_frames_at_level(ctx, n_frames, frames, 0, 1, kMaxBlocks, /*budget_early=*/false, who, [&](int, const dvo_hip_frame* f) -> int {
    if (!(f->lens_on || f->rig_on || f->filter_on)) return DVO_HIP_OK;
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame that carries a lens, a depth rig or a depth filter takes raw sensor planes; rendered planes are rectified, registered and free of sensor noise already");
  });
  if (rc != DVO_HIP_OK) return rc;
  const CameraGeom* cam = frames[0]->cam;
  const int width = frames[0]->lv[0].w, height = frames[0]->lv[0].h;
  RenderArgs args;
  rc = check_render(ctx, map, n_frames, width, height, cam->K[0], poses, params, &args, who);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the planes the frames ingest: scratch of the context.  Its last readers are the builds of the previous call's frames, which the main
  // stream waits for at the end of that call
  const size_t pixels = size_t(width) * size_t(height), plane = (pixels * 4 + 255) & ~size_t(255);
  std::vector<void*> planes;
  rc = reserve_plane_pairs(ctx, ctx->render_frame_planes, plane, n_frames, &planes);
  if (rc != DVO_HIP_OK) return rc;
  std::vector<const void*> ci, cz;
  for (size_t k = 0; k < planes.size(); ++k) (k % 2 ? cz : ci).push_back(planes[k]);
  IngestSource src{ci.data(), DVO_HIP_PIXEL_F32, 0, cz.data(), 1.0f, DVO_HIP_DEPTH_F32, 0};
  IngestSource probe = src;
  rc = check_ingest(ctx, who, n_frames, frames, &probe, /*plain_ok=*/true, role, cfg);   // (role, cfg, one camera: before anything is launched)
  if (rc != DVO_HIP_OK) return rc;
  rc = upload_views(ctx, n_frames, width, height, cam->K[0], poses, planes.data());
  if (rc != DVO_HIP_OK) return rc;
  launch_map_render(ctx->stream, map_table(map), render_views(ctx), render_outs(ctx, n_frames), n_frames, (long long)pixels, args,
                    ctx->scratch_words.as<unsigned long long>(), /*colour=*/false);
  DVO_HIP_TRY(ctx, hipGetLastError());
  DVO_HIP_TRY(ctx, hipEventRecord(ctx->render_done, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamWaitEvent(ctx->build_stream, ctx->render_done, 0));
  ctx->map_renders += n_frames;
  rc = ingest(ctx, who, n_frames, frames, src, /*host_planes=*/false, /*plain_ok=*/true, role, cfg, 0, (flags & DVO_HIP_INGEST_NO_RAW_COPY) ? 0 : 1);
  if (rc != DVO_HIP_OK) return rc;
  return wait_for_build(ctx, n_frames, frames);              // (the next render into the scratch planes runs behind this ingest)
}

int dvo_hip_time_map_render(dvo_hip_context* ctx, dvo_hip_map* map, int n_views, int width, int height, const float K[4], const double* poses,
                            const dvo_hip_render_params* params, int reps, float ms[3]) {
  DVO_ENTER(ctx);
  RenderArgs args;
  int rc = check_render(ctx, map, n_views, width, height, K, poses, params, &args, "time_map_render");
  if (rc != DVO_HIP_OK) return rc;
  if (reps < 1 || reps > 1000 || !ms) return fail(ctx, DVO_HIP_ERR_INVALID, "time_map_render: bad argument");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t pixels = size_t(width) * size_t(height), plane = (pixels * 4 + 255) & ~size_t(255);
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->build_stream));   // (the scratch planes may still be read by an ingest)
  std::vector<void*> planes;
  rc = reserve_plane_pairs(ctx, ctx->render_frame_planes, plane, n_views, &planes);
  if (rc == DVO_HIP_OK) rc = upload_views(ctx, n_views, width, height, K, poses, planes.data());
  if (rc != DVO_HIP_OK) return rc;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (hipEvent_t& x : ev)
    if (e == hipSuccess) e = hipEventCreate(&x);
  std::vector<float> t[3];
  unsigned long long* zbuf = ctx->scratch_words.as<unsigned long long>();
  const MapTable table = map_table(map);
  for (int r = 0; r < reps && e == hipSuccess; ++r) {
    e = hipEventRecord(ev[0], ctx->stream);
    launch_render_fill(ctx->stream, zbuf, (long long)pixels * n_views);
    if (e == hipSuccess) e = hipEventRecord(ev[1], ctx->stream);
    launch_render_splat(ctx->stream, table, render_views(ctx), n_views, args, zbuf, /*colour=*/false);
    if (e == hipSuccess) e = hipEventRecord(ev[2], ctx->stream);
    launch_render_resolve(ctx->stream, zbuf, render_outs(ctx, n_views), n_views, (long long)pixels, /*colour=*/false);
    if (e == hipSuccess) e = hipEventRecord(ev[3], ctx->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventSynchronize(ev[3]);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) {
      float one = 0.0f;
      e = hipEventElapsedTime(&one, ev[k], ev[k + 1]);
      t[k].push_back(one);
    }
  }
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  DVO_HIP_TRY(ctx, e);
  for (int k = 0; k < 3; ++k) {
    std::sort(t[k].begin(), t[k].end());
    ms[k] = t[k][t[k].size() / 2];
  }
  return DVO_HIP_OK;
}
