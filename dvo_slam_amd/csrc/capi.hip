// capi.hip -- host side of libdvo_hip.so: contexts, device-resident frame pyramids and the batched
// coarse-to-fine Gauss-Newton driver behind the C-ABI of include/dvo_hip.h.
//
// The host never touches pixels or poses: it uploads two raw planes per frame, enqueues kernels on the
// context's HIP stream and polls one integer ("pairs still iterating") every few iterations.
#include <hip/hip_runtime.h>
#ifdef DVO_WITH_ROCTX
#include <rocprofiler-sdk-roctx/roctx.h>
#endif
#include <xmmintrin.h>

#include <algorithm>
#include <functional>
#include <climits>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <atomic>
#include <chrono>
#include <thread>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dvo_hip.h"
#include "device_types.h"
#include "batch_policy.h"
#include "colour.h"
#include "sensor_formats.h"
#include "launch.h"
#include "keyframe_codes.h"
#include "pose_graph.h"
#include "ref_order.h"
#include "selection.h"

using namespace dvo_hip;

namespace {

std::string g_create_error;

// Bumped whenever device memory goes back to the allocator: what the small-table cache (PinnedRing) knows about the contents of
// device addresses is only good until an address can have been handed out again.
std::atomic<unsigned long long> g_free_epoch{1};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) {
      (void)hipFree(p);
      g_free_epoch.fetch_add(1, std::memory_order_relaxed);
    }
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  void release() {
    if (p) {
      (void)hipFree(p);
      g_free_epoch.fetch_add(1, std::memory_order_relaxed);
    }
    p = nullptr;
    bytes = 0;
  }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};

struct PinnedBuf {               // host memory the device can write (mapped, coherent), grown on demand
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t n) {
    if (n <= bytes) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocCoherent | hipHostMallocMapped);
    if (e == hipSuccess) bytes = n;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};

struct CameraGeom {             // RgbdCameraPyramid: per-level size, intrinsics and the point-cloud template
  int w0 = 0, h0 = 0, levels = 0;
  float K0[4] = {0, 0, 0, 0};
  int w[kMaxLevels], h[kMaxLevels];
  float K[kMaxLevels][4];
  float* tx[kMaxLevels];
  float* ty[kMaxLevels];
  DevBuf tables;
};

struct FrameLevel {
  int w = 0, h = 0;
  float* I = nullptr;
  float* Z = nullptr;
  float4* A = nullptr;
  float2* B = nullptr;
  float2* R = nullptr;
  float2* C = nullptr;         // {I, Z} of a current frame for the window sweep (null: not kept at this level)
  int cur_have = 0;            // flavours of the current-frame role that are built: kCurAB (A, B) | kCurC (C)
  bool selected = false;       // R / count built for (ithr, dthr) (reference role)
  bool q3 = false;             // ... and its last selected pixel cleared if the count is odd (option "ref_order", ref_order.hip)
  bool explicit_sel = false;   // ... or R / count hold an accepted set the caller handed over (dvo_hip_frame_set_level_selection)
  float ithr = 0, dthr = 0;
};

}  // namespace

struct dvo_hip_frame {
  int levels = 0;
  const CameraGeom* cam = nullptr;
  FrameLevel lv[kMaxLevels];
  DevBuf pool;
  int* sel_count = nullptr;    // device, one int per level
  unsigned long long built_seq = 0;   // ticket of the last build-stream work that wrote this frame (0 = none pending)
  int deferred = 0;                   // named by a recorded, not yet executed ingest (option "defer_ingest")
  // Frames ingested from raw sensor planes have no float I / Z planes at level 0 (k_build_from_raw writes the role planes
  // straight from the raw data).  What level 0 can later be derived from: the current-role planes A + B if they exist (they
  // hold everything), else the 3-B copy of the raw planes in the frame's staging area.
  bool raw0 = false;
  bool raw_copy = false;
  float depth_scale = 0.0f;
  // The caller selection of the reference role (dvo_hip_frames_set_selection): the frame's own copy of the level-0 mask (w0 bytes per
  // row) and the depth range, applied by k_apply_selection wherever a plane R is built.  Kept across re-ingests.
  bool sel_on = false;
  bool sel_has_mask = false;
  float sel_min = 0.0f, sel_max = INFINITY;
  DevBuf sel_mask;
  unsigned long long sel_visit = 0;   // (apply_selection: the call that last listed the frame)
  // The lens of the frame's camera (dvo_hip_frames_set_lens, lens.h): every later ingest rectifies the caller's planes into the frame's
  // float planes of level 0 first (lens_stage).  The frame's, not the camera's: CameraGeom describes the rectified image.
  bool lens_on = false;
  dvo_hip_lens lens = {};
  // The depth rig of the frame's sensors (dvo_hip_frames_set_depth_rig, depth_rig.h): every later ingest takes its depth plane as the depth
  // sensor's own image and registers it into the frame's float plane Z of level 0 first (rig_stage), ahead of the lens pass.
  bool rig_on = false;
  dvo_hip_depth_rig rig = {};
  // The depth filter of the frame (dvo_hip_frames_set_depth_filter, depth_filter.h): every later ingest conditions the depth plane the
  // other stages hand on -- flying pixels and hole borders rejected, noise smoothed -- into filter_plane first (filter_stage, the last
  // stage), and the ingest reads THAT plane.  The plane (w x h floats) is allocated when the filter is set and freed when it is cleared:
  // a steady-state ingest allocates nothing.
  bool filter_on = false;
  dvo_hip_depth_filter filter = {};
  DevBuf filter_plane;
  // The colour of the frame (dvo_hip_frames_set_colour, cloud_colour.h): its own level-0 plane of packed pixels, w0 * h0 dwords, written
  // and read on the main stream only.  A property like the lens: kept across re-ingests until it is replaced or cleared.
  bool colour_on = false;
  DevBuf colour;
};

// Small host -> device transfers (pointer tables, initial guesses) go through slots of pinned memory: from a pageable
// source the runtime stages the bytes itself and may hold the calling thread while it does; from a pinned slot the upload is a
// plain asynchronous copy and the host goes on enqueueing.  (No measurable difference in the benchmark loop, whose host side
// is dominated by the caller; kept because it takes a host-side wait out of the enqueue path.)  A slot is reused only after
// the copy that read it has completed (one event per slot).
// Small tables go from the pinned ring to device memory with a copy KERNEL, not with a copy command: copy commands of every stream
// share the DMA engine, where a few hundred bytes of table queue behind whatever is in flight -- behind 1.9 GB of raw planes when a
// caller streams 1024 pairs per step from host memory (the match then started 33 ms late, every step).
__global__ void k_copy_table(unsigned long long* __restrict__ dst, const unsigned long long* __restrict__ src, size_t n8) {
  const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n8) dst[i] = src[i];
}

// Waiting for a stream on the paths where the wait is part of a match's or a frame's latency: polling keeps the thread on its core
// instead of parking it in the driver; a wait that lasts longer than 20 ms falls back to the sleeping kind.
hipError_t sync_stream(hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess) return hipSuccess;
    if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();   // "still running" is not an error to keep
    if (q != hipErrorNotReady) return q;
    if ((spins & 0xff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) return hipStreamSynchronize(s);
  }
}

struct PinnedRing {
  static const int kSlots = 48;
  char* base = nullptr;
  size_t slot_bytes = 0;
  hipEvent_t done[kSlots] = {};
  bool in_flight[kSlots] = {};
  unsigned next = 0;

  // A streaming caller hands over the same frame sets step after step: the tables of a step (plane pointers of the frames to build,
  // of the pairs to align, identity initial guesses) are then the very bytes the device already holds at the very address.  The ring
  // remembers what it last sent to an address (a host copy) and sends nothing when it is asked for the same bytes again, on the same
  // stream, with no device memory freed in between (round 5: a 128-pair step of bench.py spent ~150 us of host time on ten such
  // uploads before its first alignment kernel was enqueued, and two dependent copy kernels at the head of the chain).
  struct Sent {
    void* dst = nullptr;
    hipStream_t stream = nullptr;
    unsigned long long epoch = 0, used = 0;
    std::vector<char> bytes;
  };
  static const int kSent = 24;
  Sent sent[kSent];
  unsigned long long clock = 0;
  long long skipped = 0;            // uploads answered from the cache (counter "table_uploads_skipped")
  bool cache = true;

  hipError_t upload(hipStream_t stream, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    Sent* slot = nullptr;
    if (cache) {
      const unsigned long long epoch = g_free_epoch.load(std::memory_order_relaxed);
      Sent* oldest = &sent[0];
      for (Sent& c : sent) {
        if (c.dst == dst) { slot = &c; break; }
        if (c.used < oldest->used) oldest = &c;
      }
      if (slot && slot->stream == stream && slot->epoch == epoch && slot->bytes.size() == bytes && std::memcmp(slot->bytes.data(), src, bytes) == 0) {
        slot->used = ++clock;
        skipped += 1;
        return hipSuccess;
      }
      if (!slot) slot = oldest;
      slot->dst = nullptr;                                       // (valid again once the copy below is enqueued)
      // Whatever else the cache believes about bytes of [dst, dst + bytes) is about to be overwritten: the slices of one table buffer
      // (ensure_roles) lie at offsets that depend on the batch size, so uploads of different batches overlap without sharing a start
      // address (round-5 advisor finding: batches of 3, 2, 3 pairs with a re-ingest between them left the 3-pair slice's entry alive
      // over the 2-pair slices' bytes, and the third upload was skipped).
      const char* lo = static_cast<const char*>(dst);
      for (Sent& c : sent)
        if (c.dst && static_cast<const char*>(c.dst) < lo + bytes && lo < static_cast<const char*>(c.dst) + c.bytes.size()) c.dst = nullptr;
    }
    const hipError_t e_up = upload_now(stream, dst, src, bytes);
    if (slot && e_up == hipSuccess) {
      slot->dst = dst;
      slot->stream = stream;
      slot->epoch = g_free_epoch.load(std::memory_order_relaxed);
      slot->used = ++clock;
      slot->bytes.assign(static_cast<const char*>(src), static_cast<const char*>(src) + bytes);
    }
    return e_up;
  }

  // which of `k` device buffers already holds exactly these bytes (sent on this stream, nothing freed since); -1: none
  int holder(DevBuf* candidates, int k, hipStream_t stream, const void* src, size_t bytes) const {
    if (!cache) return -1;
    const unsigned long long epoch = g_free_epoch.load(std::memory_order_relaxed);
    for (int i = 0; i < k; ++i)
      for (const Sent& c : sent)
        if (c.dst && c.dst == candidates[i].p && c.stream == stream && c.epoch == epoch && c.bytes.size() == bytes && std::memcmp(c.bytes.data(), src, bytes) == 0)
          return i;
    return -1;
  }

  void forget(const void* dst) {                                  // somebody else wrote to this address
    for (Sent& c : sent)
      if (c.dst == dst) c.dst = nullptr;
  }

  hipError_t upload_now(hipStream_t stream, void* dst, const void* src, size_t bytes) {
    if (bytes > slot_bytes) {                      // grow: wait for every copy in flight, then one new block
      hipError_t e = drain();
      if (e != hipSuccess) return e;
      if (base) (void)hipHostFree(base);
      base = nullptr;
      slot_bytes = 0;
      size_t want = 64 * 1024;
      while (want < bytes) want *= 2;
      e = hipHostMalloc(reinterpret_cast<void**>(&base), want * kSlots, hipHostMallocMapped);
      if (e != hipSuccess) return e;
      slot_bytes = want;
    }
    const unsigned k = next++ % kSlots;
    hipError_t e = hipSuccess;
    if (!done[k]) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
    if (e == hipSuccess && in_flight[k]) e = hipEventSynchronize(done[k]);
    if (e != hipSuccess) return e;
    std::memcpy(base + slot_bytes * k, src, bytes);
    if (bytes % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 8 == 0) {     // (every table here is pointers or doubles)
      const size_t n8 = bytes / 8;
      k_copy_table<<<dim3(unsigned((n8 + 255) / 256)), dim3(256), 0, stream>>>(
          static_cast<unsigned long long*>(dst), reinterpret_cast<const unsigned long long*>(base + slot_bytes * k), n8);
      e = hipGetLastError();
    } else {
      e = hipMemcpyAsync(dst, base + slot_bytes * k, bytes, hipMemcpyHostToDevice, stream);
    }
    if (e == hipSuccess) e = hipEventRecord(done[k], stream);
    in_flight[k] = e == hipSuccess;
    return e;
  }
  hipError_t drain() {
    for (int k = 0; k < kSlots; ++k)
      if (in_flight[k]) {
        const hipError_t e = hipEventSynchronize(done[k]);
        if (e != hipSuccess) return e;
        in_flight[k] = false;
      }
    return hipSuccess;
  }
  void release() {
    (void)drain();
    for (hipEvent_t& ev : done)
      if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    if (base) (void)hipHostFree(base);
    base = nullptr;
    slot_bytes = 0;
  }
};

// What the slow lane of a batch keeps from one batch to the next (capi_lane.inc, option "overlap_tails"): the stragglers of the levels run on
// a stream of their own beside the batch's chain, with partial rows, residual pairs and log-likelihood sums of their own (two levels index
// those by different tile counts), the pairs' flag bytes and the lane's two lists of them.  (Here and not in capi_lane.inc: the
// workspace holds one, and the lane's code needs the context, which holds the workspace.)
struct LaneResources {
  hipStream_t stream = nullptr;
  hipEvent_t split = nullptr;                  // the chain has marked its stragglers
  hipEvent_t end[2] = {nullptr, nullptr};      // per list: the launches given it so far are through (the current list's: all of the lane's)
  DevBuf partials, scratch, ll, flags, lists;
  hipError_t quiesce() { return stream ? hipStreamSynchronize(stream) : hipSuccess; }
  void release() {
    for (DevBuf* b : {&partials, &scratch, &ll, &flags, &lists}) b->release();
    if (!stream) return;
    (void)quiesce();
    (void)hipStreamDestroy(stream);
    for (hipEvent_t e : {split, end[0], end[1]}) (void)hipEventDestroy(e);
    stream = nullptr;
  }
};

// The batch workspace: one HIP stream, device scratch and the pinned poll words of the Gauss-Newton loop.
// (Splitting a batch into concurrently iterating pair groups on several streams was measured and dropped: the coarse
// levels are bound by the host's launch rate, which more streams only divide -- profiles/r01_d_groups.txt.)
struct Workspace {
  hipStream_t stream = nullptr;
  DevBuf states, partials, scratch, ll_partials, lvl_stats, it_stats, results, t_init, counters, pair_sums;
  // the pairs' plane-pointer table, in one of a few buffers picked by the batch's first frames: a caller that alternates between two
  // or three frame sets finds each set's table where it left it (PinnedRing's cache of what was sent where)
  static const int kTableSlots = 4;
  DevBuf pair_ptrs[kTableSlots];
  unsigned pair_ptrs_next = 0;
  DevBuf win_fallbacks;          // one 64-bit counter: lanes of the window sweep whose taps were fetched from memory (align_window.hip)
  int* f16_range_flag = nullptr; // pinned, one word per pair of the batch: raised by a workgroup of the f16 Gram schedule whose Jacobian left the f16 range (gram_f16.h)
  size_t f16_range_words = 0;
  PinnedRing* tables = nullptr;  // the context's ring for small uploads
  int* host_status = nullptr;    // pinned: one word per Gauss-Newton step of a batch, written by the device (k_solver_step)
  size_t host_status_words = 0;
  std::string err;
  bool created = false;
  // resident match kernel: the exchange rows of the workgroup groups and the sequence numbers used so far
  DevBuf exchange;
  unsigned resident_sequence = 0;
  long long exchange_shape = -1;   // pairs x group of the launch the exchange buffer was last cleared for
  // ... and, when it runs a whole match of a small batch, where it leaves results and statistics: pinned host memory the host
  // thread reads as soon as the kernel has counted the pairs done (no copy command, no stream synchronisation)
  PinnedBuf direct_results, direct_levels, direct_iters, direct_done;
  bool needs_drain = false;        // a batch ended early: the stream is drained before buffers are reused
  bool device_may_lag = true;      // the last batch returned without waiting for the stream (the resident kernel's direct path)
  int resident_error_word = 0;     // index of the current resident launch's error word in host_status (a ring, see kResidentErrorWords)
  unsigned resident_launch_counter = 0;
  LaneResources lane;              // the slow lane of a batch (capi_lane.inc)
  DevBuf chain_list;               // option "tail_lists": the pairs the chain's last steps of a level cover (capi_schedule.inc, chain_level)
  // option "ref_order": the rows' records of a pass (RefOrderSeg, the largest level's height per pair) and the pairs' RefOrderPair
  DevBuf ref_rows, ref_pairs;
};

// a helper thread of the concurrent pair groups (dvo_hip_context::opt_batch_groups) and the slice of the caller's batch it aligns
struct GroupWorker {
  dvo_hip_context* twin = nullptr;
  std::thread thread;
  std::mutex m;
  std::condition_variable cv;
  bool has_job = false, done = false, quit = false;
  // the job: a slice of the caller's batch
  int n = 0;
  dvo_hip_frame* const* refs = nullptr;
  dvo_hip_frame* const* curs = nullptr;
  const dvo_hip_config* cfg = nullptr;
  dvo_hip_result* results = nullptr;
  dvo_hip_level_stats* levels = nullptr;
  dvo_hip_iteration_stats* iters = nullptr;
  int cap_levels = 0, cap_iters = 0;
  hipEvent_t after = nullptr;                                  // the twin's stream waits for it (the role planes are ready)
  int rc = DVO_HIP_OK;
};


struct dvo_hip_context {
  // The reference hands one current pyramid to two trackers on two threads (dvo_slam/src/local_tracker.cpp:180-184) and runs
  // thread-local validators over shared keyframes (keyframe_graph.cpp:576-593): calls on one context from several host threads
  // are serialised here (recursive: dvo_hip_match -> dvo_hip_match_batch).  Contexts never share a lock.
  std::recursive_mutex mutex;
  int device = 0;
  hipStream_t stream = nullptr;    // == ws[0].stream
  std::string err;
  int opt_rows_per_wave = 0;
  int opt_iters_per_sync = 0;
  // Rendezvous of single-pair matches (dvo_hip_match): the reference's LocalTracker aligns every new image against two reference
  // frames from two threads at once (tbb::parallel_invoke, dvo_slam/src/local_tracker.cpp:180-184).  Two such calls with the same
  // current frame and the same configuration leave as ONE two-pair batch (one resident launch: 0.19 ms for both instead of 2 x 0.18
  // one after the other).  A caller waits for a partner only on a context where concurrent callers have been seen.
  struct MatchRequest {
    dvo_hip_frame* reference; dvo_hip_frame* current; const dvo_hip_config* cfg; dvo_hip_result* result;
    dvo_hip_level_stats* levels; int cap_levels; dvo_hip_iteration_stats* iters; int cap_iters;
    std::atomic<int> state{0};       // 0: waiting for a partner, 1: taken by one, 2: done (rc valid)
    int rc = 0;
  };
  std::mutex rendezvous_mutex;
  MatchRequest* rendezvous_waiting = nullptr;
  dvo_hip_frame* rendezvous_busy_current = nullptr;   // the current frame of the single-pair match that is running right now (null: none)
  int rendezvous_expect = 0;          // > 0: a lone caller waits (briefly) for a partner; refreshed whenever two callers met or collided
  int opt_rendezvous = 1;
  long long rendezvous_pairs = 0;     // two-pair batches formed (counter "rendezvous_pairs")
  long long f16_range_repeats = 0; // batches repeated with the f32 Gram because a Jacobian left the f16 range (counter "f16_range_repeats")
  long long strip_ingests = 0;     // frames ingested by the strip kernel (ingest_strips.hip), counter "strip_ingests"
  long long colour_ingests = 0;    // frames ingested from an 8-bit colour plane (colour.h), counter "colour_ingests"
  long long sensor_ingests = 0;    // frames ingested from a raw sensor plane (sensor_formats.h), counter "sensor_ingests"
  long long f32_ingests = 0;       // frames ingested from a float depth plane (DVO_HIP_DEPTH_F32), counter "f32_ingests"
  long long lens_ingests = 0;      // frames rectified at ingest (dvo_hip_frames_set_lens), counter "lens_ingests"
  long long depth_filter_ingests = 0;  // frames whose depth was filtered at ingest (dvo_hip_frames_set_depth_filter), counter "depth_filter_ingests"
  long long depth_registrations = 0;   // frames whose depth was registered at ingest (dvo_hip_frames_set_depth_rig), counter "depth_registrations"
  long long map_inserts = 0, map_points = 0, map_dropped = 0;   // frames / points a keyframe map took, points it dropped (dvo_hip_map_insert); counters of the same names
  long long map_removes = 0, map_rehashes = 0;   // frames subtracted from a keyframe map (dvo_hip_map_remove, dvo_hip_map_move), tables rebuilt (dvo_hip_map_rehash); counters of the same names
  // option "graph_resident": dvo_hip_graph_optimize hands a resident-sized graph to the resident kernel (capi_graph.inc); counter
  // "graph_resident_solves": graphs that kernel has optimised, by that way or by dvo_hip_graph_optimize_batch
  int opt_graph_resident = 0;
  long long graph_resident_solves = 0;
  long long map_renders = 0;       // views rendered out of a keyframe map (dvo_hip_map_render, dvo_hip_map_render_frames), counter "map_renders"
  long long frame_warps = 0;       // items warped (dvo_hip_frames_warp_inverse, dvo_hip_frames_warp_forward), counter "frame_warps"
  long long covisibility_pairs = 0;   // pairs counted (dvo_hip_frames_covisibility), counter "covisibility_pairs"
  long long codebook_encoded = 0;  // frames encoded (dvo_hip_frames_encode, dvo_hip_codebook_add_frames, _query_frames), counter "codebook_encoded"
  long long codebook_queries = 0;  // queries answered (dvo_hip_codebook_query_*), counter "codebook_queries"
  // Option "defer_ingest": a batched re-ingest (dvo_hip_frames_update_raw_device_as) is only recorded, and carried out by the next
  // dvo_hip_match_batch right behind the first launches of its first level (or by whatever entry point comes first).  A streaming
  // caller re-ingests the next batch and then aligns the current one: enqueueing the ingest first keeps the alignment's stream idle
  // for the ~0.1 ms (128 pairs) to ~0.5 ms (1024 pairs) of host time it takes -- this way the host does that work while the device
  // is already on the coarsest level.
  struct DeferredIngest {
    std::vector<dvo_hip_frame*> frames;
    std::vector<const void*> planes, depth;   // (an IngestSource's arrays, copied; its format and resolved pitch)
    int format = 0;
    size_t pitch = 0;
    int depth_format = 0;
    size_t depth_pitch = 0;
    float depth_scale;
    int role;
    dvo_hip_config cfg;
    bool keep_raw_copy;
  };
  std::vector<DeferredIngest> deferred;
  int opt_defer_ingest = 0;
  int opt_defer_ingest_pixels = 0; // a recorded ingest waits until the launch chain is on a level of at least this many pixels (0: the chain's first launches)
  int opt_keep_raw_copy = 1;       // 0: a frame ingested straight into the reference role keeps no copy of its raw planes (option "keep_raw_copy")
  long long deferred_ingests = 0;  // ingests carried out behind the first launches of a match (counter "deferred_ingests")
  int opt_build_workgroups = 0;    // cap on the workgroups of a build-stream kernel (0 = one per tile): background builds
  int opt_stream_policy = 1;       // build-stream strip kernels stream raw planes and levels 0-1 non-temporally (option "stream_policy")
  int opt_tail_speculation = 0;    // 1: always enqueue the step ahead of the poll, also on the tail of a level whose empty step is costly (measurement)
  int opt_solver_waves = 0;        // wavefronts of a solver-step workgroup: 0 = by level and batch size, 2, 4
  int opt_ll_blocks = 0;           // workgroups per pair of the log-likelihood pass (0 = by batch size)
  int opt_compact_residuals = 1;   // the contracted window sweep stores only the residual pairs of constraints, packed (LevelGeom::compact)
  int opt_gram_lo_parts = 1;       // 1 (default since round 6): every Gram operand keeps its f16 low part on every level; 0: LevelGeom::gram_hi_j on the large ones
  int opt_min_workgroups = 0;      // tile-height heuristic: smallest launch that still counts as filling the chip
  int opt_condition_number = 0;    // results carry |lambda_max / lambda_min| of the information matrix
  int opt_fused_ll_pixels = 0;     // largest level (pixels) whose log-likelihood sweep runs inside the solver workgroup (0 = by batch size)
  float last_sel_ithr = 0.0f, last_sel_dthr = 0.0f;   // selection thresholds of the last match on this context
  int f32_gram_hold = 0;           // batches that still run with the f32 Gram after one left the f16 range (run_batch)
  long long warmup_wait_us = 0;    // longest of the waits dvo_hip_context_create made on the context's streams
  int opt_variant = 8;             // schedule of the sweep: 8 = current-frame window staged in LDS, contracted arithmetic + f16 hi/lo Gram on the matrix pipe where the level allows (7: residuals bit-identical to the oracle's)
                                   // (width a multiple of 64), else 5 = gathering sweep with the f32 Gram on the matrix cores
  // the resident match kernel (align_resident.hip): -1 = levels whose sweep is short enough for the groups that fit (default),
  // 0 = never (launches per iteration only), 1 = every level
  int opt_resident = -1;
  int opt_resident_rows = 0;       // "short enough": segments per wavefront and iteration at most (0 = kResidentRowsDefault)
  int opt_resident_group = 0;      // workgroups per pair (0 = as many as fit, up to kResidentMaxGroup)
  int resident_timeouts = 0;       // batches that had to be repeated because a group timed out (see run_batch)
  long long resident_launches = 0;
  long long resident_levels = 0;   // pyramid levels those launches ran (counter "resident_levels")
  // where the host thread's time of dvo_hip_match_batch goes (ns, accumulated): before the first launch of the batch, enqueueing,
  // waiting for the device, after the device is done
  long long host_ns[4] = {0, 0, 0, 0};
  long long host_batches = 0;
  std::chrono::steady_clock::time_point batch_entry;
  int opt_resident_flags = 0;      // kResidentFlag* (measurement and test hooks)
  // 1: on the levels whose log-likelihood pass fits the solver step, the step runs in the sweep's launch (solver_step.h).  Default 0:
  // measured slower in round 6 (profiles/r06_sweep_tail.txt) -- the step's serial float64 lane needs ~180 registers, the sweep it rides
  // in is built for 96 (five workgroups per compute unit), and the spilled step takes 40-50 us instead of 15
  int opt_sweep_tail = 0;
  long long tail_steps = 0;        // Gauss-Newton steps enqueued as ONE launch (sweep with a tail)
  // The overlapped tail of a level (round 6, capi_lane.inc): once at most opt_overlap_fraction-th of a large batch's pairs is still on a level, the
  // others begin the next level and the stragglers finish theirs beside it, on a stream of their own -- each pair leaves its level
  // independently, like the reference's match() calls do (dense_tracking.cpp:357).  0: off; 1: on (levels whose log-likelihood pass
  // runs inside the solver step, batches beyond the solver steps' hand-over).
  int opt_overlap_tails = 0;
  int opt_overlap_fraction = 8;
  // Active-pair lists (round 6): where an empty step is expensive (kCostlyEmptyStepWorkgroups) and at most 1/8 of the pairs is left on the
  // level, the steps that follow are launched over a LIST of those pairs -- tiles x active workgroups instead of tiles x pairs that
  // all but a few leave at once.  1: on.
  int opt_tail_lists = 0;
  long long listed_steps = 0;      // steps launched over an active-pair list (counter "listed_steps")
  long long overlapped_tails = 0;  // levels whose tail ran beside the next level (counter "overlapped_tails")
  long long overlapped_steps = 0;  // Gauss-Newton steps enqueued on the tail stream (counter "overlapped_steps")
  long long tail_drains = 0;       // batches that ended with a slow lane (counter "tail_drains") ...
  long long tail_wait_ns = 0;      // ... and how long the host waited for it behind the chain's last step (counter "tail_wait_us")
  // Concurrent pair groups (round 6): a large batch is aligned as two or three sub-batches at once -- the caller's thread runs the first
  // on this context, helper threads the others on TWIN contexts (same device, own stream, own scratch), like the reference spreads
  // independent match() calls over the workers of a tbb::parallel_reduce (dvo_slam/src/keyframe_graph.cpp:576-593).  Option
  // "batch_groups": 0 / 1 = one group (the default: see batch_groups_of for what was measured), 2 .. 4 = that many.
  int opt_batch_groups = 0;
  bool is_twin = false;            // a helper's context: never splits, never owns frames
  std::vector<GroupWorker*> group_workers;
  hipEvent_t roles_ready = nullptr;   // recorded behind ensure_batch_roles: the twins' streams wait for it
  long long grouped_batches = 0;
  // 1: levels small enough for LDS run align_small.hip under the default schedule; 0 (default): the gathering sweep.  Measured level: an
  // 80 x 60 launch of 1024 pairs 45-50 us against 46-48, of 128 pairs 10.2-11.3 against 9.0-9.5 -- three 53-KB workgroups per compute unit
  // hide a row's latencies no better than the gathering sweep's eight wavefronts per SIMD hide its taps' 
  int opt_small_sweep = 0;
  int opt_small_tiles = 0;         // its workgroups per pair (0 = BatchPolicy::small_level_tiles)
  int opt_coarse = 0;              // the fused coarse-level kernel (align_coarse.hip): 0 = off (default: measured and lost), 1 = whenever the levels admit it
  int opt_codebook_round_kb = 256 * 1024;   // staging for one round's distance matrix (capi_codes.inc, run_query), option "codebook_round_kb"
  int opt_coarse_pixels = 0;       // levels of up to this many pixels run in it (0 = kCoarseMaxPixels)
  int opt_coarse_wgs = 0;          // its workgroups per compute unit: 0 / 4 (128 registers) or 3 (168)
  long long coarse_launches = 0, coarse_levels = 0;
  int opt_deterministic = 0;       // a pair's record does not depend on the batch it is aligned in (see dvo_hip.h, option "deterministic")
  int opt_ref_compat = 0;          // projection and weights multiply with the HOST CPU's _mm_rcp_ps like the reference does
  int opt_ref_order = 0;           // the reference's rank-dependent quirks Q3, Q6, Q7 (ref_order.hip; option "ref_order")
  long long ref_order_passes = 0;  // steps enqueued with its scale passes (counter "ref_order_passes")
  DevBuf ref_order_planes;         // the RefOrderPlane table of the Q3 edit
  DevBuf rcp_table;                // ... from this table, dumped from the instruction itself when the option is first switched on
  int rcp_shift = 0;
  int rcp_packed = 0;              // a 16-bit copy of the table lies behind it (LevelGeom::rcp_packed)
  int opt_resident_cooperative = 0; // launch groups through hipLaunchCooperativeKernel (a separate hardware queue: +0.1 ms per launch)
  int compute_units = 0;
  std::vector<CameraGeom*> cameras;
  // Device blocks of destroyed frames, kept for the next frame of the same size: a tracking loop creates and destroys one frame per
  // image, and hipMalloc + hipFree (which waits for the device) cost more than building the frame (0.36 vs 0.13 ms at 640x480).
  // Reuse is safe without waiting: what still reads a destroyed frame can only be build-stream work queued before the next
  // frame's build (same stream, in order); main-stream readers are matches, and those have returned.
  struct PooledBlock { void* p; size_t bytes; };
  std::vector<PooledBlock> frame_pool;
  size_t frame_pool_bytes = 0;
  static constexpr size_t kFramePoolMaxBytes = size_t(1) << 30;
  static constexpr size_t kFramePoolMaxBlocks = 64;
  Workspace ws[1];
  DevBuf misc, role_tbl_cur, role_tbl_ref, prep_tbl_cur, prep_tbl_ref;
  DevBuf sel_tbl_main, sel_tbl_build;                 // tables of the caller-selection apply pass, one per stream (apply_selection)
  unsigned long long sel_visits = 0;
  DevBuf lens_tbl;                                    // table of the rectify pass (lens_stage; allocated by the first lens ingest)
  DevBuf sensor_tbl;                                  // table of the sensor-format pass (sensor_stage; allocated by the first sensor ingest)
  DevBuf graph_jobs, graph_outs;                      // the job records and results of a resident pose-graph launch (capi_graph.inc)
  DevBuf filter_tbl;                                  // table of the filter pass (filter_stage; allocated by the first filtered ingest)
  DevBuf rig_tbl;                                     // table of the register pass (rig_stage; allocated by the first rig ingest)
  DevBuf colour_tbl, colour_stage;                    // the plane table of a k_colour_pack launch and the staging area of host colour planes (capi_colour.inc)
  // The scratch of the calls that read frames at a level (capi_frame_calls.inc) and of the map's own calls.  Every use is a launch or a
  // copy on the main stream, and every such call ends in a wait for that stream (a render to device planes excepted, behind which the
  // next launch that reuses a buffer follows on the same stream): no call finds a buffer still in use, and may reallocate it.
  //   frame_tbl      the launch's table (upload_block_table): MapFrame of every such call; MapMergeEntry of the merges
  //   result_stage   results on their way to host memory (stage_results): map read-outs, world points and normals, renders, warps,
  //                  covisibility records, codes, query rows and -- in front of them -- a query's distance matrix; host records on
  //                  their way into a merge; a colour level (dvo_hip_frame_download_colour)
  //   side_tbl       the launch's second table: a render's views and planes, a warp's planes, covisibility's pairs, a query's ids and
  //                  skipped intervals
  //   scratch_words  device-only words: the z-buffers of renders and forward warps, a query's codes
  //   render_frame_planes  the planes a render hands to the frames' ingest (dvo_hip_map_render_frames, dvo_hip_time_map_render); read
  //                  on the build stream, which that call waits for
  DevBuf frame_tbl, result_stage, side_tbl, scratch_words, render_frame_planes;
  hipEvent_t render_done = nullptr;                   // recorded behind a render on the main stream: the build stream's ingest waits for it
  static const int kTableSlots = 4;
  DevBuf build_tbl[kTableSlots];   // (a few, picked by the list's first frame: see Workspace::pair_ptrs)
  DevBuf* build_tbl_cur = nullptr; // the one that holds the table of build_tbl_frames
  unsigned build_tbl_next = 0;
  PinnedRing tables;
  // build_tbl holds, in build-stream order, the table of exactly these frames (frames_build): the per-level launches of an
  // eager prepare of the same list reuse it instead of uploading the same bytes again
  std::vector<dvo_hip_frame*> build_tbl_frames;
  // Frame construction (ingest, pyramid, eagerly prepared role planes) runs on its own stream so that the next batch of
  // frames can be built while the current batch is being aligned: the build is bandwidth-bound, the coarse pyramid levels
  // of an alignment are latency-bound, and the two overlap.  Every build call takes a ticket and records an event; an
  // alignment makes the main stream wait for the newest ticket among ITS frames only.
  hipStream_t build_stream = nullptr;
  static const int kBuildRing = 16;
  hipEvent_t build_events[kBuildRing] = {};
  unsigned long long build_seq = 0;          // last ticket issued
  unsigned long long main_waited_seq = 0;    // newest ticket the main stream already waits behind
  // Host -> device transfers of raw planes (dvo_hip_frames_update_raw) have a stream of their own, so that the DMA of batch
  // k+2 runs while batch k+1 is being built and batch k aligned.
  // The planes land in one of kUploadRing contiguous device buffers (not in the frames' own staging areas), so that host planes
  // that are adjacent in memory move in ONE transfer: a 0.9 MB copy per frame reaches ~30 GB/s, a whole batch per copy the link rate.
  hipStream_t upload_stream = nullptr;
  hipEvent_t upload_done = nullptr;
  static const int kUploadRing = 3;
  DevBuf upload_buf[kUploadRing];
  unsigned long long upload_buf_seq[kUploadRing] = {};   // ticket of the build that reads the buffer's current contents
  unsigned upload_next = 0;
  unsigned long long upload_waited_seq = 0;  // newest build ticket the upload stream already waits behind
};

namespace {
int flush_deferred(dvo_hip_context* ctx);
}

// carry out the recorded ingests, if any (under the context's lock): nothing overtakes a recorded ingest
#define DVO_FLUSH_DEFERRED(ctx)                                     \
  do {                                                              \
    if ((ctx) && !(ctx)->deferred.empty()) {                        \
      const int rc_deferred__ = flush_deferred(ctx);                \
      if (rc_deferred__ != DVO_HIP_OK) return rc_deferred__;        \
    }                                                               \
  } while (0)

// How an entry point begins.  DVO_LOCK: the context's lock for the rest of the function, if there is a context (a null one is refused by
// the argument check that follows).  DVO_ENTER: the same, then the recorded ingests -- every entry point that works on frames or streams.
#define DVO_LOCK(ctx)                                               \
  std::unique_lock<std::recursive_mutex> guard;                     \
  if (ctx) guard = std::unique_lock<std::recursive_mutex>((ctx)->mutex)
#define DVO_ENTER(ctx) \
  DVO_LOCK(ctx);       \
  DVO_FLUSH_DEFERRED(ctx)

namespace {

// roctx ranges with the phase names of the reference's own (commented-out) stopwatches inside match()
// (dvo_core/src/dense_tracking.cpp:154-158, 222, 246, 309, 325, 349): "prep" = per-level set-up, "err" = passes 1-4 (the sweep and
// the log-likelihood pass), "linsys" = pass 5 + solve (the solver step); plus "build" for the frame construction.  They bracket
// the ENQUEUE of a phase on the host (rocprofv3 --marker-trace shows them next to the kernel trace); free when no tool listens.
// (marker ranges are a profiling aid: a ROCm installation without rocprofiler-sdk builds the library with WITH_ROCTX=0, Makefile)
struct Range {
#ifdef DVO_WITH_ROCTX
  explicit Range(const char* name) { roctxRangePushA(name); }
  ~Range() { roctxRangePop(); }
#else
  explicit Range(const char*) {}
#endif
};

#define DVO_HIP_TRY(ctx, expr)                                                                   \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess) {                                                                      \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                            \
      return DVO_HIP_ERR_HIP;                                                                     \
    }                                                                                             \
  } while (0)

#define DVO_WS_TRY(ws, expr)                                                                     \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess) {                                                                      \
      (ws).err = std::string(#expr) + ": " + hipGetErrorString(e__);                              \
      return DVO_HIP_ERR_HIP;                                                                     \
    }                                                                                             \
  } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int workspace_create(dvo_hip_context* ctx, int g) {
  Workspace& w = ctx->ws[g];
  if (w.created) return DVO_HIP_OK;
  // the alignment stream outranks the build stream: its short, dependent kernels must not queue behind the wide
  // elementwise kernels of a concurrent frame build
  int prio_least = 0, prio_greatest = 0;
  DVO_HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  DVO_HIP_TRY(ctx, hipStreamCreateWithPriority(&w.stream, hipStreamNonBlocking, prio_greatest));
  w.created = true;
  return DVO_HIP_OK;
}

void workspace_destroy(Workspace& w) {
  if (!w.created) return;
  (void)hipStreamSynchronize(w.stream);
  for (DevBuf& b : w.pair_ptrs) b.release();
  for (DevBuf* b : {&w.states, &w.partials, &w.scratch, &w.ll_partials, &w.lvl_stats, &w.it_stats, &w.results,
                    &w.t_init, &w.counters, &w.exchange, &w.win_fallbacks, &w.pair_sums, &w.chain_list, &w.ref_rows, &w.ref_pairs})
    b->release();
  w.lane.release();
  if (w.host_status) (void)hipHostFree(w.host_status);
  w.host_status = nullptr;
  w.host_status_words = 0;
  if (w.f16_range_flag) (void)hipHostFree(w.f16_range_flag);
  w.f16_range_flag = nullptr;
  w.f16_range_words = 0;
  for (PinnedBuf* b : {&w.direct_results, &w.direct_levels, &w.direct_iters, &w.direct_done}) b->release();
  (void)hipStreamDestroy(w.stream);
  w.created = false;
}

int fail(dvo_hip_context* ctx, int code, const char* msg) {
  if (ctx) ctx->err = msg;
  return code;
}
// (... "<entry point>: <rule>")
int fail(dvo_hip_context* ctx, int code, const char* who, const char* rule) {
  if (ctx) ctx->err = std::string(who) + ": " + rule;
  return code;
}

// The checks of a list of frames that every entry point shares; `who` names the entry point in the error text.  The list itself
// (others: the call's other mandatory pointers are there) ...
int check_frame_count(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const char* who, bool others = true) {
  if (!ctx || n_frames < 1 || !frames || !others) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  return DVO_HIP_OK;
}
// ... one frame of it (own_context: it must be a frame of a camera of this context) ...
int check_frame(dvo_hip_context* ctx, const dvo_hip_frame* f, const char* who, bool own_context = false) {
  if (!f) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null frame");
  if (own_context && std::find(ctx->cameras.begin(), ctx->cameras.end(), f->cam) == ctx->cameras.end())
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "a frame of another context");
  return DVO_HIP_OK;
}
// ... and both, for an entry point that checks nothing in between
int check_frame_list(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const char* who, bool own_context = false) {
  int rc = check_frame_count(ctx, n_frames, frames, who);
  for (int i = 0; i < n_frames && rc == DVO_HIP_OK; ++i) rc = check_frame(ctx, frames[i], who, own_context);
  return rc;
}

// The table of a launch whose workgroups find their entry by bisecting first_block (map_device.h), into `tbl` on the main stream: `host`
// holds the launch's entries, their first_block set, and one more, which becomes the end of the list at total_blocks.
template <typename Entry>
int upload_block_table(dvo_hip_context* ctx, DevBuf& tbl, std::vector<Entry>& host, int total_blocks) {
  std::memset(&host.back(), 0, sizeof(Entry));
  host.back().first_block = total_blocks;
  const size_t bytes = host.size() * sizeof(Entry);
  DVO_HIP_TRY(ctx, tbl.reserve(bytes));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, tbl.p, host.data(), bytes));
  return DVO_HIP_OK;
}

// The raw planes of a batch of frames (capi_ingest.inc), in host or in device memory: an 8-bit intensity or colour plane and a u16 depth
// plane per frame, one format and one row pitch for all of them
struct IngestSource {
  const void* const* planes;   // image planes
  int format;                  // 0 = grey, one byte per pixel; else DVO_HIP_PIXEL_* (DVO_HIP_PIXEL_F32: one float per pixel)
  size_t pitch;                // bytes from one row of an image plane to the next (as the caller gave it, 0 = tight, until check_ingest resolves it)
  const void* const* depth;    // depth planes: u16, tight; or float (DVO_HIP_DEPTH_F32) with a pitch of their own
  float depth_scale;
  int depth_format = DVO_HIP_DEPTH_U16;
  size_t depth_pitch = 0;      // float depth: bytes from one row to the next, 0 = tight until check_ingest resolves it (u16 depth: unused)
};

#include "capi_frames.inc"     // cameras, frame allocation and build, role planes (ensure_roles)
#include "capi_schedule.inc"   // batch plan, buffers, waits, resident / coarse plans, run_batch in parts (and, in front of those, capi_lane.inc)

// The Gram schedule of a batch, decided ONCE, before the planes of the roles are prepared for it (round-4 advisor finding: deciding it
// inside run_batch prepared two flavours of the current role for every new frame).  The default accumulates on the f16 matrix pipe
// from exact high + low operand pairs, which cannot represent a Jacobian component beyond +-65504; pairs that meet one are repeated
// with the f32 Gram (run_batch).  Two cases take the f32 Gram from the start: option "deterministic" (a pair's bits must not depend
// on whether ANOTHER pair of its batch left the f16 range), and the batches right after a batch MOST of whose pairs left it (a
// tracking sequence with a close depth step would otherwise pay twice on every frame; this makes the arithmetic of those batches
// depend on the context's history -- documented in dvo_hip.h, reset by option "variant").
struct EffectiveVariantScope {
  dvo_hip_context* c; int keep;
  explicit EffectiveVariantScope(dvo_hip_context* ctx) : c(ctx), keep(ctx->opt_variant) {
    if (c->opt_variant >= 7 && (c->opt_deterministic || c->f32_gram_hold > 0)) {
      if (c->f32_gram_hold > 0) c->f32_gram_hold -= 1;
      c->opt_variant = 6;
    }
  }
  ~EffectiveVariantScope() { c->opt_variant = keep; }
};

#include "capi_groups.inc"   // concurrent pair groups (option "batch_groups"): run_batch_grouped, destroy_group_workers

// preparation for the parity / measurement entry points
int prepare_single(dvo_hip_context* ctx, int n, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, const dvo_hip_config* cfg, BatchPlan& bp) {
  int rc = validate_batch(ctx, n, refs, curs, cfg);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_batch_roles(ctx, n, refs, curs, cfg, /*launch_path_only=*/true);
  if (rc != DVO_HIP_OK) return rc;
  make_plan(ctx, refs[0]->cam, cfg, n, bp);
  rc = prepare_buffers(ctx->ws[0], cfg, refs, curs, bp);
  if (rc == DVO_HIP_OK && sync_stream(ctx->stream) != hipSuccess) rc = DVO_HIP_ERR_HIP;
  if (rc != DVO_HIP_OK) ctx->err = ctx->ws[0].err;
  return rc;
}

}  // namespace

extern "C" {

int dvo_hip_get_counter(dvo_hip_context* ctx, const char* key, long long* value);   // (capi_options.inc, below)

const char* dvo_hip_version(void) { return "dvo_hip 0.1 (gfx950)"; }

namespace {
// The host CPU's _mm_rcp_ps as a table (option "ref_compat").  The instruction's result is probed, not assumed: over all 2^23
// mantissas of [1, 2) the smallest k is found for which the result depends on the leading k mantissa bits only (11 on the Intel
// Xeon this was developed on, 12 on the EPYC 9575F of the MI355X box), and the exact scaling with the exponent is checked on a
// sample.  A CPU whose instruction does not have that form (k > 16) is refused.
int build_rcp_table(dvo_hip_context* ctx) {
  auto rcp = [](float x) { return _mm_cvtss_f32(_mm_rcp_ss(_mm_set_ss(x))); };
  auto at = [](unsigned m) { unsigned b = 0x3f800000u | m; float x; std::memcpy(&x, &b, 4); return x; };
  // change points of the result along the mantissa: their common alignment gives k
  unsigned all_changes = 0;
  float prev = rcp(at(0));
  for (unsigned m = 1; m < (1u << 23); ++m) {
    const float r = rcp(at(m));
    if (r != prev) { all_changes |= m; prev = r; }
  }
  int shift = 0;
  while (shift < 23 && !((all_changes >> shift) & 1u)) ++shift;     // every change point is a multiple of 2^shift
  const int k = 23 - shift;
  if (k > 16) return fail(ctx, DVO_HIP_ERR_INVALID, "ref_compat: this CPU's _mm_rcp_ps is not a table on at most 16 mantissa bits");
  for (unsigned m = 0; m < (1u << 23); m += 4099)
    for (int e = -24; e <= 24; e += 3) {
      const float s = std::ldexp(1.0f, e);
      if (rcp(at(m) * s) != rcp(at(m)) / s) return fail(ctx, DVO_HIP_ERR_INVALID, "ref_compat: this CPU's _mm_rcp_ps does not scale exactly with the exponent");
    }
  std::vector<float> table(size_t(1) << k);
  for (unsigned i = 0; i < table.size(); ++i) table[i] = rcp(at(i << shift));
  // a 16-bit copy for the sweep that keeps the table in LDS: every value is in (0.5, 1], i.e. bits in [0x3f000000, 0x3f800000]; an
  // instruction with 11-12 bits of precision leaves the low mantissa bits zero (0x3f7ff800 is the OR of all results on the Intel Xeon
  // this was developed on).  Checked, not assumed; a table that does not pack, or one of more than 2^12 entries, is used from memory.
  bool packs = k <= 12;
  std::vector<uint16_t> packed(table.size());
  for (size_t i = 0; i < table.size() && packs; ++i) {
    unsigned b;
    std::memcpy(&b, &table[i], 4);
    packs = b >= 0x3f000000u && b <= 0x3f800000u && ((b - 0x3f000000u) & 0xffu) == 0;
    packed[i] = uint16_t((b - 0x3f000000u) >> 8);
  }
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, ctx->rcp_table.reserve(table.size() * (sizeof(float) + sizeof(uint16_t))));
  DVO_HIP_TRY(ctx, hipMemcpy(ctx->rcp_table.p, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
  if (packs)
    DVO_HIP_TRY(ctx, hipMemcpy(ctx->rcp_table.as<float>() + table.size(), packed.data(), packed.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  ctx->rcp_shift = shift;
  ctx->rcp_packed = packs ? 1 : 0;
  return DVO_HIP_OK;
}
}  // namespace

int dvo_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dvo_hip_context_create(int device, dvo_hip_context** out) {
  if (!out) return DVO_HIP_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_error = "no HIP device available (libdvo_hip has no CPU fallback)";
    return DVO_HIP_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    g_create_error = "device index out of range";
    return DVO_HIP_ERR_INVALID;
  }
  e = hipSetDevice(device);
  if (e != hipSuccess) {
    g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
    return DVO_HIP_ERR_HIP;
  }
  dvo_hip_context* ctx = new dvo_hip_context();
  ctx->device = device;
  if (hipDeviceGetAttribute(&ctx->compute_units, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ctx->compute_units = 0;
  int rc = workspace_create(ctx, 0);
  if (rc != DVO_HIP_OK) {
    g_create_error = "context setup: " + ctx->err;
    workspace_destroy(ctx->ws[0]);
    delete ctx;
    return DVO_HIP_ERR_HIP;
  }
  ctx->stream = ctx->ws[0].stream;
  ctx->ws[0].tables = &ctx->tables;
  int prio_least = 0, prio_greatest = 0;
  e = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->build_stream, hipStreamNonBlocking, prio_least);
  for (int i = 0; i < dvo_hip_context::kBuildRing && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ctx->build_events[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->upload_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->upload_done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->render_done, hipEventDisableTiming);
  if (e != hipSuccess) {
    g_create_error = std::string("context setup (build stream): ") + hipGetErrorString(e);
    dvo_hip_context_destroy(ctx);
    return DVO_HIP_ERR_HIP;
  }
  // Warm-up of the wait path.  In the FIRST GPU process on a fresh box the first stream wait of a batch has been seen to return 14-24 ms
  // after the device had finished (19 us by its own time stamps; DESIGN.md section 8: not under the profiler, not in later
  // processes, with polling as with hipStreamSynchronize, and skipping one wait only moved it to the next) -- a one-time cost of the
  // runtime's host-side wait machinery, not of this engine.  Every stream of the context therefore waits three times on a
  // trivial command here, where no caller is timing; the longest of those waits is kept (counter "warmup_wait_us"), so that a stall
  // that still shows up in a first match can be told from one that was absorbed here.
  {
    long long longest = 0;
    unsigned char scratch_byte[8] = {0};
    void* dev = nullptr;
    if (hipMalloc(&dev, 64) == hipSuccess) {
      for (hipStream_t st : {ctx->stream, ctx->build_stream, ctx->upload_stream})
        for (int rep = 0; rep < 3; ++rep) {
          (void)hipMemsetAsync(dev, 0, 64, st);
          (void)hipMemcpyAsync(scratch_byte, dev, 8, hipMemcpyDeviceToHost, st);
          const auto t0 = std::chrono::steady_clock::now();
          (void)hipStreamSynchronize(st);
          longest = std::max<long long>(longest, std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
        }
      (void)hipFree(dev);
    }
    ctx->warmup_wait_us = longest;
  }
  // DVO_HIP_REF_COMPAT=1: the reference-compatible arithmetic for callers that cannot set options -- the reference's own, unmodified
  // programs linked against the facade (tests/dropin)
  if (const char* env = std::getenv("DVO_HIP_REF_COMPAT"))
    if (env[0] == '1' && dvo_hip_set_option(ctx, "ref_compat", 1) != DVO_HIP_OK) {
      g_create_error = ctx->err;
      dvo_hip_context_destroy(ctx);
      return DVO_HIP_ERR_INVALID;
    }
  // DVO_HIP_REF_ORDER=1: the same for option "ref_order"
  if (const char* env = std::getenv("DVO_HIP_REF_ORDER"))
    if (env[0] == '1' && dvo_hip_set_option(ctx, "ref_order", 1) != DVO_HIP_OK) {
      g_create_error = ctx->err;
      dvo_hip_context_destroy(ctx);
      return DVO_HIP_ERR_INVALID;
    }
  *out = ctx;
  return DVO_HIP_OK;
}

void dvo_hip_context_destroy(dvo_hip_context* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  ctx->deferred.clear();                                       // (nobody is left to read what a recorded ingest would build)
  destroy_group_workers(ctx);
  if (ctx->upload_stream) (void)hipStreamSynchronize(ctx->upload_stream);
  if (ctx->build_stream) (void)hipStreamSynchronize(ctx->build_stream);
  for (Workspace& w : ctx->ws) workspace_destroy(w);
  if (ctx->upload_done) (void)hipEventDestroy(ctx->upload_done);
  if (ctx->upload_stream) (void)hipStreamDestroy(ctx->upload_stream);
  for (hipEvent_t ev : ctx->build_events)
    if (ev) (void)hipEventDestroy(ev);
  if (ctx->build_stream) (void)hipStreamDestroy(ctx->build_stream);
  for (DevBuf& b : ctx->build_tbl) b.release();
  for (DevBuf* b : {&ctx->misc, &ctx->role_tbl_cur, &ctx->role_tbl_ref, &ctx->prep_tbl_cur, &ctx->prep_tbl_ref, &ctx->rcp_table, &ctx->ref_order_planes,
                    &ctx->sel_tbl_main, &ctx->sel_tbl_build, &ctx->lens_tbl, &ctx->sensor_tbl, &ctx->rig_tbl, &ctx->filter_tbl, &ctx->graph_jobs, &ctx->graph_outs, &ctx->frame_tbl, &ctx->result_stage, &ctx->colour_tbl, &ctx->colour_stage, &ctx->side_tbl, &ctx->scratch_words, &ctx->render_frame_planes}) b->release();
  if (ctx->render_done) (void)hipEventDestroy(ctx->render_done);
  for (DevBuf& b : ctx->upload_buf) b.release();
  for (const dvo_hip_context::PooledBlock& b : ctx->frame_pool) (void)hipFree(b.p);
  ctx->frame_pool.clear();
  ctx->tables.release();
  for (CameraGeom* c : ctx->cameras) {
    c->tables.release();
    delete c;
  }
  delete ctx;
}

const char* dvo_hip_last_error(const dvo_hip_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void* dvo_hip_context_stream(dvo_hip_context* ctx) { return ctx ? static_cast<void*>(ctx->stream) : nullptr; }

int dvo_hip_context_device(const dvo_hip_context* ctx) { return ctx ? ctx->device : -1; }

#include "capi_options.inc"   // dvo_hip_get_counter, dvo_hip_set_option

namespace {

// role and cfg of dvo_hip_frames_prepare and of a role-aware ingest, against the frames; `who` names the entry point in the error text
int check_prepare_args(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int role, const dvo_hip_config* cfg, const char* who) {
  if (!ctx || n_frames < 1 || !frames || !cfg || (role != DVO_HIP_ROLE_CURRENT && role != DVO_HIP_ROLE_REFERENCE))
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (cfg->first_level < cfg->last_level || cfg->last_level < 0 || cfg->first_level >= kMaxLevels)
    return fail(ctx, DVO_HIP_ERR_INVALID, who, "need 0 <= last_level <= first_level < DVO_HIP_MAX_LEVELS");
  for (int i = 0; i < n_frames; ++i) {
    if (!frames[i]) return fail(ctx, DVO_HIP_ERR_INVALID, who, "null entry");
    if (frames[i]->cam != frames[0]->cam || frames[i]->levels <= cfg->first_level)
      return fail(ctx, DVO_HIP_ERR_INVALID, who, "frames must share the camera and have first_level + 1 levels");
  }
  return DVO_HIP_OK;
}

// role planes of levels cfg->last_level .. cfg->first_level on the build stream (what is already there is skipped)
int prepare_roles(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int role, const dvo_hip_config* cfg) {
  const bool ref = role == DVO_HIP_ROLE_REFERENCE;
  int want[kMaxLevels];
  for (int l = 0; l < kMaxLevels; ++l) want[l] = l < frames[0]->cam->levels ? eager_current_flavor(ctx, frames[0]->cam, l, n_frames) : kCurAB;
  float ithr = ref ? cfg->intensity_derivative_threshold : 0.0f, dthr = ref ? cfg->depth_derivative_threshold : 0.0f;
  std::vector<dvo_hip_frame*> speculative;
  if (ref && (ithr < 0.0f || dthr < 0.0f)) {
    // A negative threshold asks for a SPECULATIVE preparation (a caller that does not know the tracker the frame will meet: the facade's
    // buildAccelerationStructure): with the thresholds of the context's last match, and only for frames that hold no selection at
    // all -- a frame selected for other thresholds keeps its planes instead of alternating between two selections.
    ithr = ctx->last_sel_ithr; dthr = ctx->last_sel_dthr;
    for (int i = 0; i < n_frames; ++i) {
      bool any = false;
      for (int l = cfg->last_level; l <= cfg->first_level; ++l) any |= frames[i]->lv[l].selected;
      if (!any) speculative.push_back(frames[i]);
    }
    if (speculative.empty()) return DVO_HIP_OK;
    n_frames = int(speculative.size());
    frames = speculative.data();
  }
  const int rc = ensure_roles(ctx, n_frames, frames, ref ? 1 : 0, cfg->last_level, cfg->first_level, ithr, dthr, /*eager=*/true, want);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipGetLastError());
  return DVO_HIP_OK;
}

}  // namespace

#include "capi_ingest.inc"   // the raw-frame ingest: dvo_hip_frame_create_*, dvo_hip_frames_update_*, dvo_hip_flush_deferred
#include "capi_frame_calls.inc"   // calls that read frames at a level: the check of their frames, the frame table, results to the caller
#include "capi_map.inc"      // the keyframe map: dvo_hip_map_*, dvo_hip_frames_world_points, dvo_hip_map_render*
#include "capi_colour.inc"   // the colour of frames: dvo_hip_frames_set_colour, dvo_hip_frames_clear_colour, dvo_hip_frame_download_colour
#include "capi_normal.inc"   // surface normals: dvo_hip_frames_normals, dvo_hip_map_extract_normals, dvo_hip_map_render_normals
#include "capi_warp.inc"     // frames warped under a pose: dvo_hip_frames_warp_inverse, dvo_hip_frames_warp_forward
#include "capi_covis.inc"    // keyframe covisibility: dvo_hip_frames_covisibility
#include "capi_codes.inc"    // keyframes retrieved by appearance: dvo_hip_codebook_*, dvo_hip_frames_encode
#include "capi_graph.inc"    // the keyframe pose graph: dvo_hip_graph_*

int dvo_hip_upload_wait(dvo_hip_context* ctx) {
  DVO_ENTER(ctx);
  if (!ctx) return DVO_HIP_ERR_INVALID;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
  return DVO_HIP_OK;
}

int dvo_hip_host_alloc(dvo_hip_context* ctx, size_t bytes, void** out) {
  DVO_LOCK(ctx);
  if (!ctx || !out || bytes == 0) return fail(ctx, DVO_HIP_ERR_INVALID, "host_alloc: bad argument");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return DVO_HIP_OK;
}

void dvo_hip_host_free(dvo_hip_context* ctx, void* p) {
  DVO_LOCK(ctx);
  if (!p) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  (void)hipHostFree(p);
}

int dvo_hip_frames_prepare(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, int role, const dvo_hip_config* cfg) {
  DVO_ENTER(ctx);
  const int rc = check_prepare_args(ctx, n_frames, frames, role, cfg, "frames_prepare");
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return prepare_roles(ctx, n_frames, frames, role, cfg);
}

void dvo_hip_frame_destroy(dvo_hip_context* ctx, dvo_hip_frame* frame) {
  DVO_LOCK(ctx);
  if (!frame) return;
  if (ctx && !ctx->deferred.empty()) (void)flush_deferred(ctx);   // (a recorded ingest may name this frame)
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    ctx->build_tbl_frames.clear();   // a later frame may be given the same address
    if (frame->pool.p && ctx->frame_pool.size() < dvo_hip_context::kFramePoolMaxBlocks &&
        ctx->frame_pool_bytes + frame->pool.bytes <= dvo_hip_context::kFramePoolMaxBytes) {
      ctx->frame_pool.push_back({frame->pool.p, frame->pool.bytes});   // kept for the next frame of this size (see frame_pool)
      ctx->frame_pool_bytes += frame->pool.bytes;
      frame->pool.p = nullptr;
      frame->pool.bytes = 0;
    } else {
      (void)hipStreamSynchronize(ctx->stream);
      if (ctx->upload_stream) (void)hipStreamSynchronize(ctx->upload_stream);
      if (ctx->build_stream) (void)hipStreamSynchronize(ctx->build_stream);
    }
  }
  frame->sel_mask.release();
  frame->filter_plane.release();
  frame->colour.release();
  frame->pool.release();
  delete frame;
}

int dvo_hip_frame_info(const dvo_hip_frame* frame, int level, int* width, int* height, float K[4]) {
  if (!frame || level < 0 || level >= frame->levels) return DVO_HIP_ERR_INVALID;
  if (width) *width = frame->lv[level].w;
  if (height) *height = frame->lv[level].h;
  if (K) std::memcpy(K, frame->cam->K[level], 16);
  return DVO_HIP_OK;
}

int dvo_hip_frame_device_planes(const dvo_hip_frame* frame, int level, void** intensity_dev, void** depth_dev) {
  if (!frame || level < 0 || level >= frame->levels) return DVO_HIP_ERR_INVALID;
  if (intensity_dev) *intensity_dev = frame->lv[level].I;
  if (depth_dev) *depth_dev = frame->lv[level].Z;
  return DVO_HIP_OK;
}

int dvo_hip_frame_download_plane(dvo_hip_context* ctx, dvo_hip_frame* frame, int level, int plane, float* out) {
  DVO_ENTER(ctx);
  if (!ctx || !frame || !out || level < 0 || level >= frame->levels || plane < 0 || plane > 5)
    return fail(ctx, DVO_HIP_ERR_INVALID, "frame_download_plane: bad argument");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  dvo_hip_frame* one[1] = {frame};
  int rc = wait_for_build(ctx, 1, one);
  if (rc == DVO_HIP_OK) rc = ensure_roles(ctx, 1, one, 0, level, level, 0.0f, 0.0f);
  if (rc != DVO_HIP_OK) return rc;
  const FrameLevel& L = frame->lv[level];
  const size_t n = size_t(L.w) * L.h;
  DVO_HIP_TRY(ctx, ctx->misc.reserve(n * 4));
  launch_unpack_plane(ctx->stream, L.A, L.B, int(n), plane, ctx->misc.as<float>());
  DVO_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->misc.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}

int dvo_hip_frame_select(dvo_hip_context* ctx, dvo_hip_frame* frame, int level, float ithr, float dthr, int* n_selected,
                         uint8_t* mask_or_null) {
  DVO_ENTER(ctx);
  if (!ctx || !frame || level < 0 || level >= frame->levels) return fail(ctx, DVO_HIP_ERR_INVALID, "frame_select: bad argument");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = size_t(frame->lv[level].w) * frame->lv[level].h;
  uint8_t* mask_dev = nullptr;
  if (mask_or_null) {
    DVO_HIP_TRY(ctx, ctx->misc.reserve(n));
    mask_dev = ctx->misc.as<uint8_t>();
  }
  dvo_hip_frame* one[1] = {frame};
  if (frame->lv[level].explicit_sel) frame->lv[level].selected = false;   // (a selection for thresholds replaces an explicit one)
  int rc = wait_for_build(ctx, 1, one);
  if (rc == DVO_HIP_OK) rc = ensure_roles(ctx, 1, one, 1, level, level, ithr, dthr);
  if (rc == DVO_HIP_OK && mask_dev) rc = ensure_roles(ctx, 1, one, 0, level, level, 0.0f, 0.0f);
  if (rc != DVO_HIP_OK) return rc;
  if (mask_dev) {   // the mask is not kept on the device: recompute it from the sampling planes
    FrameLevel& L = frame->lv[level];
    DVO_HIP_TRY(ctx, hipMemsetAsync(frame->sel_count + level, 0, sizeof(int), ctx->stream));
    launch_select_pack(ctx->stream, L.A, L.B, L.w * L.h, ithr, dthr, L.R, frame->sel_count + level, mask_dev);
    mark_selected(L, ithr, dthr);
    rc = apply_selection(ctx, ctx->stream, 1, one, level, level, 0, mask_dev);
    if (rc != DVO_HIP_OK) return rc;
  }
  int count = 0;
  DVO_HIP_TRY(ctx, hipMemcpyAsync(&count, frame->sel_count + level, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (mask_or_null) DVO_HIP_TRY(ctx, hipMemcpyAsync(mask_or_null, mask_dev, n, hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (n_selected) *n_selected = count;
  return DVO_HIP_OK;
}

int dvo_hip_frames_set_selection(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const uint8_t* const* masks,
                                 size_t mask_pitch, int masks_on_device, float min_depth, float max_depth) {
  DVO_ENTER(ctx);
  int rc = check_frame_count(ctx, n_frames, frames, "frames_set_selection");
  if (rc != DVO_HIP_OK) return rc;
  if (!(min_depth <= max_depth)) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_selection: need min_depth <= max_depth (no NaN)");
  for (int i = 0; i < n_frames; ++i) {
    rc = check_frame(ctx, frames[i], "frames_set_selection");
    if (rc != DVO_HIP_OK) return rc;
    const size_t w0 = size_t(frames[i]->lv[0].w);
    if (masks && masks[i] && mask_pitch != 0 && mask_pitch < w0) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_selection: mask_pitch < width");
  }
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t bs = ctx->build_stream;
  bool any_mask = false, any_host = false;
  for (int i = 0; i < n_frames; ++i) {
    dvo_hip_frame* f = frames[i];
    const uint8_t* m = masks ? masks[i] : nullptr;
    const size_t w0 = size_t(f->lv[0].w), h0 = size_t(f->lv[0].h);
    if (m) {
      DVO_HIP_TRY(ctx, f->sel_mask.reserve(w0 * h0));
      // on the build stream: behind every build that may still read the frame's previous mask, ahead of every later one
      DVO_HIP_TRY(ctx, hipMemcpy2DAsync(f->sel_mask.p, w0, m, mask_pitch ? mask_pitch : w0, w0, h0,
                                        masks_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, bs));
      any_mask = true;
      any_host = any_host || !masks_on_device;
    }
    f->sel_has_mask = m != nullptr;
    f->sel_min = min_depth;
    f->sel_max = max_depth;
    f->sel_on = f->sel_has_mask || selection_range_on(min_depth, max_depth);
    invalidate_reference_role(f);
  }
  if (any_mask) {
    rc = stamp_build(ctx, n_frames, frames);
    if (rc != DVO_HIP_OK) return rc;
  }
  if (any_host) DVO_HIP_TRY(ctx, hipStreamSynchronize(bs));   // (the caller may reuse a host mask at once)
  return DVO_HIP_OK;
}

int dvo_hip_frames_clear_selection(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames) {
  DVO_ENTER(ctx);
  const int rc = check_frame_list(ctx, n_frames, frames, "frames_clear_selection");
  if (rc != DVO_HIP_OK) return rc;
  for (int i = 0; i < n_frames; ++i) {
    dvo_hip_frame* f = frames[i];
    if (!f->sel_on) continue;
    f->sel_on = f->sel_has_mask = false;
    f->sel_min = 0.0f;
    f->sel_max = INFINITY;
    invalidate_reference_role(f);   // (the mask buffer is kept for the next selection)
  }
  return DVO_HIP_OK;
}

int dvo_hip_frames_set_lens(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const dvo_hip_lens* lens) {
  DVO_ENTER(ctx);                                              // (a recorded ingest of these frames is carried out with the lens it was recorded under)
  int rc = check_frame_count(ctx, n_frames, frames, "frames_set_lens", lens != nullptr);
  if (rc != DVO_HIP_OK) return rc;
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(lens->K_raw[k])) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_lens: K_raw is not finite");
  for (int k = 0; k < 8; ++k)
    if (!std::isfinite(lens->D[k])) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_lens: D is not finite");
  if (!(lens->K_raw[0] > 0.0f) || !(lens->K_raw[1] > 0.0f)) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_lens: need fx_raw > 0 and fy_raw > 0");
  for (int i = 0; i < n_frames && rc == DVO_HIP_OK; ++i) rc = check_frame(ctx, frames[i], "frames_set_lens");
  if (rc != DVO_HIP_OK) return rc;
  // (a depth rig projects into the rectified pinhole K: its output is rectified depth already)
  for (int i = 0; i < n_frames; ++i)
    if (frames[i]->rig_on && lens->rectify_depth != 0)
      return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_lens: a frame that carries a depth rig takes a lens with rectify_depth = 0 only");
  for (int i = 0; i < n_frames; ++i) {
    dvo_hip_frame* f = frames[i];
    f->lens_on = true;
    std::memcpy(f->lens.K_raw, lens->K_raw, sizeof f->lens.K_raw);
    std::memcpy(f->lens.D, lens->D, sizeof f->lens.D);
    f->lens.rectify_depth = lens->rectify_depth != 0 ? 1 : 0;   // (lenses are compared bytewise: one spelling of "on", reserved ignored)
    f->lens.reserved = 0;
  }
  return DVO_HIP_OK;
}

int dvo_hip_frames_clear_lens(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames) {
  DVO_ENTER(ctx);
  const int rc = check_frame_list(ctx, n_frames, frames, "frames_clear_lens");
  if (rc != DVO_HIP_OK) return rc;
  for (int i = 0; i < n_frames; ++i) {
    frames[i]->lens_on = false;
    frames[i]->lens = dvo_hip_lens{};
  }
  return DVO_HIP_OK;
}

int dvo_hip_frames_set_depth_rig(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const dvo_hip_depth_rig* rig) {
  DVO_ENTER(ctx);                                              // (a recorded ingest of these frames is carried out with the rig it was recorded under)
  int rc = check_frame_count(ctx, n_frames, frames, "frames_set_depth_rig", rig != nullptr);
  if (rc != DVO_HIP_OK) return rc;
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(rig->K_depth[k])) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_depth_rig: K_depth is not finite");
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(rig->T[k])) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_depth_rig: T is not finite");
  if (!(rig->K_depth[0] > 0.0f) || !(rig->K_depth[1] > 0.0f)) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_depth_rig: need fx_d > 0 and fy_d > 0");
  if (rig->reserved[0] != 0 || rig->reserved[1] != 0) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_depth_rig: reserved must be 0");
  for (int i = 0; i < n_frames && rc == DVO_HIP_OK; ++i) rc = check_frame(ctx, frames[i], "frames_set_depth_rig");
  if (rc != DVO_HIP_OK) return rc;
  for (int i = 0; i < n_frames; ++i)
    if (frames[i]->lens_on && frames[i]->lens.rectify_depth != 0)
      return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_depth_rig: the frame's lens rectifies depth (a rig's output is rectified already: rectify_depth = 0)");
  for (int i = 0; i < n_frames; ++i) {
    frames[i]->rig_on = true;
    frames[i]->rig = *rig;                                     // (rigs are compared bytewise: reserved is 0, there is no padding)
  }
  return DVO_HIP_OK;
}

int dvo_hip_frames_clear_depth_rig(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames) {
  DVO_ENTER(ctx);
  const int rc = check_frame_list(ctx, n_frames, frames, "frames_clear_depth_rig");
  if (rc != DVO_HIP_OK) return rc;
  for (int i = 0; i < n_frames; ++i) {
    frames[i]->rig_on = false;
    frames[i]->rig = dvo_hip_depth_rig{};
  }
  return DVO_HIP_OK;
}

dvo_hip_depth_filter dvo_hip_depth_filter_default(void) { return depth_filter_default_params(); }

int dvo_hip_frames_set_depth_filter(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames, const dvo_hip_depth_filter* filter) {
  DVO_ENTER(ctx);                                              // (a recorded ingest of these frames is carried out with the filter it was recorded under)
  int rc = check_frame_count(ctx, n_frames, frames, "frames_set_depth_filter", filter != nullptr);
  if (rc != DVO_HIP_OK) return rc;
  if (const char* wrong = depth_filter_check(*filter)) return fail(ctx, DVO_HIP_ERR_INVALID, "frames_set_depth_filter", wrong);
  for (int i = 0; i < n_frames && rc == DVO_HIP_OK; ++i) rc = check_frame(ctx, frames[i], "frames_set_depth_filter");
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // every plane first: a frame whose plane cannot be had leaves every frame's filter as it was
  for (int i = 0; i < n_frames; ++i)
    DVO_HIP_TRY(ctx, frames[i]->filter_plane.reserve(size_t(frames[i]->lv[0].w) * frames[i]->lv[0].h * 4));
  for (int i = 0; i < n_frames; ++i) {
    frames[i]->filter_on = true;
    frames[i]->filter = *filter;                               // (filters are compared bytewise: reserved is 0, there is no padding)
  }
  return DVO_HIP_OK;
}

int dvo_hip_frames_clear_depth_filter(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames) {
  DVO_ENTER(ctx);
  const int rc = check_frame_list(ctx, n_frames, frames, "frames_clear_depth_filter");
  if (rc != DVO_HIP_OK) return rc;
  bool any = false;
  for (int i = 0; i < n_frames; ++i) any = any || frames[i]->filter_plane.p != nullptr;
  // (the build stream may still read a plane that is about to go back to the allocator)
  if (any && ctx->build_stream) DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->build_stream));
  for (int i = 0; i < n_frames; ++i) {
    frames[i]->filter_on = false;
    frames[i]->filter = dvo_hip_depth_filter{};
    frames[i]->filter_plane.release();
  }
  return DVO_HIP_OK;
}

int dvo_hip_frame_set_level_selection(dvo_hip_context* ctx, dvo_hip_frame* frame, int level, const uint8_t* accepted) {
  DVO_ENTER(ctx);
  if (!ctx || !frame || level < 0 || level >= frame->levels) return fail(ctx, DVO_HIP_ERR_INVALID, "frame_set_level_selection: bad argument");
  if (!accepted) {                                           // drop the level's explicit set: the next use selects by thresholds again
    FrameLevel& L = frame->lv[level];
    if (L.explicit_sel) L.selected = L.explicit_sel = L.q3 = false;
    return DVO_HIP_OK;
  }
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  dvo_hip_frame* one[1] = {frame};
  int rc = wait_for_build(ctx, 1, one);
  if (rc == DVO_HIP_OK) rc = ensure_roles(ctx, 1, one, 0, level, level, 0.0f, 0.0f);   // (plane A holds the level's {I, Z})
  if (rc != DVO_HIP_OK) return rc;
  FrameLevel& L = frame->lv[level];
  const size_t n = size_t(L.w) * L.h;
  DVO_HIP_TRY(ctx, ctx->misc.reserve(n));
  DVO_HIP_TRY(ctx, hipMemcpyAsync(ctx->misc.p, accepted, n, hipMemcpyHostToDevice, ctx->stream));
  DVO_HIP_TRY(ctx, hipMemsetAsync(frame->sel_count + level, 0, sizeof(int), ctx->stream));
  launch_pack_accepted(ctx->stream, L.A, ctx->misc.as<uint8_t>(), int(n), L.R, frame->sel_count + level);
  DVO_HIP_TRY(ctx, hipGetLastError());
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  mark_selected(L, 0.0f, 0.0f);
  L.explicit_sel = true;
  return DVO_HIP_OK;
}

int dvo_hip_match_batch(dvo_hip_context* ctx, int n_pairs, dvo_hip_frame* const* references, dvo_hip_frame* const* currents,
                        const dvo_hip_config* cfg, dvo_hip_result* results, dvo_hip_level_stats* levels, int cap_levels,
                        dvo_hip_iteration_stats* iters, int cap_iters) {
  DVO_LOCK(ctx);
  if (!results) return fail(ctx, DVO_HIP_ERR_INVALID, "match: results is null");
  int rc = validate_batch(ctx, n_pairs, references, currents, cfg);
  if (rc != DVO_HIP_OK) return rc;
  if (cfg->use_initial_estimate)
    for (int i = 0; i < n_pairs; ++i)
      for (int k = 0; k < 16; ++k)
        if (!std::isfinite(results[i].transformation[k]))
          return fail(ctx, DVO_HIP_ERR_INVALID, "match: provided initialization is NaN (dense_tracking.cpp:139)");
  ctx->batch_entry = std::chrono::steady_clock::now();
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // a recorded ingest (option "defer_ingest") of frames this batch aligns comes first; of other frames: behind the first launches (run_batch)
  if (!ctx->deferred.empty()) {
    bool mine = false;
    for (int i = 0; i < n_pairs && !mine; ++i) mine = references[i]->deferred || currents[i]->deferred;
    if (mine) DVO_FLUSH_DEFERRED(ctx);
  }
  EffectiveVariantScope effective_variant_scope(ctx);
  rc = ensure_batch_roles(ctx, n_pairs, references, currents, cfg);
  if (rc != DVO_HIP_OK) return rc;

  const int groups = batch_groups_of(ctx, n_pairs);
  if (groups > 1) {
    rc = run_batch_grouped(ctx, groups, n_pairs, references, currents, cfg, results, levels, cap_levels, iters, cap_iters);
  } else {
    rc = run_batch(ctx, n_pairs, references, currents, cfg, results, levels, cap_levels, iters, cap_iters);
    if (rc != DVO_HIP_OK) ctx->err = ctx->ws[0].err;
  }
  if (!ctx->deferred.empty()) {                                // (a path without launches to hide it behind, or a batch that ended early)
    const int rc_deferred = flush_deferred(ctx);
    if (rc == DVO_HIP_OK) rc = rc_deferred;
  }
  return rc;
}

int dvo_hip_match(dvo_hip_context* ctx, dvo_hip_frame* reference, dvo_hip_frame* current, const dvo_hip_config* cfg,
                  dvo_hip_result* result, dvo_hip_level_stats* levels, int cap_levels, dvo_hip_iteration_stats* iters, int cap_iters) {
  auto alone = [&]() {
    dvo_hip_frame* r[1] = {reference};
    dvo_hip_frame* c[1] = {current};
    return dvo_hip_match_batch(ctx, 1, r, c, cfg, result, levels, cap_levels, iters, cap_iters);
  };
  if (!ctx || !reference || !current || !cfg || !result || !ctx->opt_rendezvous) return alone();
  typedef dvo_hip_context::MatchRequest Request;
  constexpr int kExpectCalls = 16;                             // lone calls that still wait after the last meeting / collision (each
                                                               // wait is up to 60 us against a 0.18-0.36 ms match: 64 was too many)
  auto same_config = [](const dvo_hip_config& a, const dvo_hip_config& b) {   // (field by field: the padding bytes of a caller's struct are not its business)
    return a.first_level == b.first_level && a.last_level == b.last_level && a.max_iterations_per_level == b.max_iterations_per_level &&
           a.use_initial_estimate == b.use_initial_estimate && a.precision == b.precision && a.mu == b.mu &&
           a.intensity_derivative_threshold == b.intensity_derivative_threshold && a.depth_derivative_threshold == b.depth_derivative_threshold;
  };
  constexpr auto kPartnerWait = std::chrono::microseconds(60);
  Request me;
  me.reference = reference; me.current = current; me.cfg = cfg; me.result = result;
  me.levels = levels; me.cap_levels = cap_levels; me.iters = iters; me.cap_iters = cap_iters;
  Request* partner = nullptr;
  bool waiting = false;
  {
    std::lock_guard<std::mutex> lock(ctx->rendezvous_mutex);
    Request* w = ctx->rendezvous_waiting;
    if (w && w->current == current && same_config(*w->cfg, *cfg)) {
      partner = w;
      ctx->rendezvous_waiting = nullptr;
      w->state.store(1, std::memory_order_release);
      ctx->rendezvous_expect = kExpectCalls;
    } else if (ctx->rendezvous_busy_current == current) {
      ctx->rendezvous_expect = kExpectCalls;                   // a collision: the other caller of this frame is already on the device
    } else if (!w && ctx->rendezvous_expect > 0) {
      ctx->rendezvous_expect -= 1;
      ctx->rendezvous_waiting = &me;
      waiting = true;
    }
  }
  if (partner) {
    // this thread runs both: the partner's pair first (it arrived first), one batch, statistics through a common stride
    dvo_hip_frame* r[2] = {partner->reference, reference};
    dvo_hip_frame* c[2] = {partner->current, current};
    dvo_hip_result res[2] = {*partner->result, *result};
    const bool want_levels = (partner->levels && partner->cap_levels > 0) || (levels && cap_levels > 0);
    const bool want_iters = (partner->iters && partner->cap_iters > 0) || (iters && cap_iters > 0);
    const int cl = want_levels ? cfg->first_level - cfg->last_level + 1 : 0;
    const int ci = want_iters ? cl * std::max(cfg->max_iterations_per_level, 1) : 0;
    std::vector<dvo_hip_level_stats> lv(size_t(2) * std::max(cl, 0));
    std::vector<dvo_hip_iteration_stats> it(size_t(2) * std::max(ci, 0));
    int rc = dvo_hip_match_batch(ctx, 2, r, c, cfg, res, want_levels ? lv.data() : nullptr, cl, want_iters ? it.data() : nullptr, ci);
    Request* both[2] = {partner, &me};
    int rcs[2] = {rc, rc};
    if (rc != DVO_HIP_OK && rc != DVO_HIP_ERR_CAPACITY && rc != DVO_HIP_ERR_INVALID) {
      // a HIP or device error: both callers get it at once (two more attempts would only double the time to report a dead device)
      partner->rc = rc;
      partner->state.store(2, std::memory_order_release);
      return rc;
    }
    if (rc == DVO_HIP_ERR_INVALID) {
      // the merged batch was refused (one request's initial estimate is not finite, a frame of another context, ...): each request
      // runs alone and gets ITS OWN status -- a valid match does not fail because of the partner it happened to meet
      for (int k = 0; k < 2; ++k) {
        Request* q = both[k];
        dvo_hip_frame* r1[1] = {q->reference};
        dvo_hip_frame* c1[1] = {q->current};
        rcs[k] = dvo_hip_match_batch(ctx, 1, r1, c1, q->cfg, q->result, q->levels, q->cap_levels, q->iters, q->cap_iters);
      }
      partner->rc = rcs[0];
      partner->state.store(2, std::memory_order_release);
      return rcs[1];
    }
    for (int k = 0; k < 2; ++k) {
      Request* q = both[k];
      *q->result = res[k];
      rcs[k] = DVO_HIP_OK;
      if (q->levels && q->cap_levels > 0) {
        const int nl = std::min(res[k].n_levels, std::min(q->cap_levels, cl));
        std::memcpy(q->levels, lv.data() + size_t(k) * cl, size_t(std::max(nl, 0)) * sizeof(dvo_hip_level_stats));
        if (res[k].n_levels > q->cap_levels) rcs[k] = DVO_HIP_ERR_CAPACITY;
      }
      if (q->iters && q->cap_iters > 0) {
        const int ni = std::min(res[k].n_iterations_total, std::min(q->cap_iters, ci));
        std::memcpy(q->iters, it.data() + size_t(k) * ci, size_t(std::max(ni, 0)) * sizeof(dvo_hip_iteration_stats));
        if (res[k].n_iterations_total > q->cap_iters) rcs[k] = DVO_HIP_ERR_CAPACITY;
      }
    }
    {
      std::lock_guard<std::mutex> lock(ctx->rendezvous_mutex);
      ctx->rendezvous_pairs += 1;
    }
    partner->rc = rcs[0];
    partner->state.store(2, std::memory_order_release);
    return rcs[1];
  }
  if (waiting) {
    const auto t0 = std::chrono::steady_clock::now();
    while (me.state.load(std::memory_order_acquire) == 0) {
      if (std::chrono::steady_clock::now() - t0 > kPartnerWait) {
        std::lock_guard<std::mutex> lock(ctx->rendezvous_mutex);
        if (ctx->rendezvous_waiting == &me) {
          ctx->rendezvous_waiting = nullptr;
          waiting = false;                                     // nobody came: alone after all
        }
        break;                                                 // (else: taken in this very moment)
      }
    }
    if (waiting) {
      while (me.state.load(std::memory_order_acquire) != 2) std::this_thread::yield();   // the partner's thread runs the batch
      return me.rc;
    }
  }
  {
    std::lock_guard<std::mutex> lock(ctx->rendezvous_mutex);
    ctx->rendezvous_busy_current = current;
  }
  const int rc = alone();
  {
    std::lock_guard<std::mutex> lock(ctx->rendezvous_mutex);
    if (ctx->rendezvous_busy_current == current) ctx->rendezvous_busy_current = nullptr;
  }
  return rc;
}

int dvo_hip_level_iteration(dvo_hip_context* ctx, dvo_hip_frame* reference, dvo_hip_frame* current, int level, float ithr,
                            float dthr, const float T34[12], const float P_prev[4], int first_iteration_on_level,
                            dvo_hip_iteration_out* out, float* residuals_or_null) {
  DVO_ENTER(ctx);
  if (!ctx || !reference || !current || !T34 || !P_prev || !out) return fail(ctx, DVO_HIP_ERR_INVALID, "level_iteration: null argument");
  dvo_hip_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.first_level = level;
  cfg.last_level = level;
  cfg.max_iterations_per_level = 1;
  cfg.intensity_derivative_threshold = ithr;
  cfg.depth_derivative_threshold = dthr;
  if (level < 0 || level >= reference->levels || level >= current->levels) return fail(ctx, DVO_HIP_ERR_INVALID, "level_iteration: bad level");
  dvo_hip_frame* r[1] = {reference};
  dvo_hip_frame* c[1] = {current};
  BatchPlan bp;
  int rc = prepare_single(ctx, 1, r, c, &cfg, bp);
  if (rc != DVO_HIP_OK) return rc;
  hipStream_t s = ctx->stream;
  LevelGeom g = bp.geom[level];
  if (residuals_or_null) g.compact = 0;                        // (by pixel: one pair at every pixel's place)
  Workspace& w0 = ctx->ws[0];
  RefOrderPair* ref_order = ctx->opt_ref_order ? w0.ref_pairs.as<RefOrderPair>() : nullptr;   // (prepare_buffers: reserved under the option)
  const size_t npx = size_t(g.w) * g.h;
  DVO_HIP_TRY(ctx, ctx->misc.reserve(256 + sizeof(dvo_hip_iteration_out)));
  float* d_T = ctx->misc.as<float>();
  float* d_P = d_T + 12;
  dvo_hip_iteration_out* d_out = reinterpret_cast<dvo_hip_iteration_out*>(ctx->misc.as<char>() + 256);
  DVO_HIP_TRY(ctx, hipMemcpyAsync(d_T, T34, 48, hipMemcpyHostToDevice, s));
  DVO_HIP_TRY(ctx, hipMemcpyAsync(d_P, P_prev, 16, hipMemcpyHostToDevice, s));
  PairState* states = ctx->ws[0].states.as<PairState>();
  DVO_HIP_TRY(ctx, hipMemsetAsync(states, 0, sizeof(PairState), s));
  launch_set_fixed_state(s, states, g, d_T, d_P, first_iteration_on_level ? 1 : 0);
  // the sweep, the passes of option "ref_order", the log-likelihood pass (`range_flag`: where an f16 Gram schedule reports that it left its range)
  auto sweep_and_passes = [&](int* range_flag) {                // (by the plan's choice of the moment)
    launch_residual_reduce(s, bp.choice[level], bp.rpw[level], level == 0, g, bp.pair_ptrs + size_t(level), states, 1, w0.partials.as<float>(), w0.scratch.as<float2>(),
                           w0.win_fallbacks.as<unsigned long long>(), range_flag);
    if (ref_order) launch_ref_order(s, g, states, 1, w0.scratch.as<float2>(), w0.ref_rows.as<RefOrderSeg>(), ref_order);
    launch_loglik(s, g, states, 1, w0.partials.as<float>(), w0.scratch.as<float2>(), w0.ll_partials.as<double>(), kLlBlocksPerPair, false, ref_order);
  };
  sweep_and_passes(w0.f16_range_flag);
  int n_sel = 0;
  DVO_HIP_TRY(ctx, hipMemcpyAsync(&n_sel, reference->sel_count + level, sizeof(int), hipMemcpyDeviceToHost, s));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(s));
  if (*static_cast<volatile int*>(ctx->ws[0].f16_range_flag) != 0) {   // (see run_batch: beyond the f16 range, again with the f32 Gram)
    *static_cast<volatile int*>(ctx->ws[0].f16_range_flag) = 0;
    ctx->f16_range_repeats += 1;
    // geometry and plane flavours of the f32 schedule (a level whose width is no multiple of 64 is the gathering sweep's there)
    const int keep_variant = ctx->opt_variant;
    ctx->opt_variant = 6;
    rc = prepare_single(ctx, 1, r, c, &cfg, bp);
    ctx->opt_variant = keep_variant;
    if (rc != DVO_HIP_OK) return rc;
    g = bp.geom[level];
    sweep_and_passes(nullptr);
    DVO_HIP_TRY(ctx, hipStreamSynchronize(s));
  }
  launch_single_shot_out(s, g, ctx->ws[0].partials.as<float>(), ctx->ws[0].ll_partials.as<double>(), kLlBlocksPerPair, n_sel, d_out, ref_order);
  if (ref_order) ctx->ref_order_passes += 1;
  DVO_HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(dvo_hip_iteration_out), hipMemcpyDeviceToHost, s));
  if (residuals_or_null) DVO_HIP_TRY(ctx, hipMemcpyAsync(residuals_or_null, ctx->ws[0].scratch.p, npx * sizeof(float2), hipMemcpyDeviceToHost, s));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(s));
  DVO_HIP_TRY(ctx, hipGetLastError());
  if (residuals_or_null) {
    // a pixel without a constraint is a NaN PAIR on this boundary; the contracted sweep marks it in the first component only (which
    // is what the log-likelihood pass tests)
    float* r = reinterpret_cast<float*>(residuals_or_null);
    for (size_t i = 0; i < npx; ++i)
      if (r[2 * i] != r[2 * i]) r[2 * i + 1] = r[2 * i];
  }
  return DVO_HIP_OK;
}

int dvo_hip_time_residual_kernel(dvo_hip_context* ctx, int n_pairs, dvo_hip_frame* const* references, dvo_hip_frame* const* currents,
                                 int level, int warm_iterations, int reps, float* avg_ms) {
  DVO_ENTER(ctx);
  if (!avg_ms || reps < 1 || warm_iterations < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "time_residual_kernel: bad argument");
  dvo_hip_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.first_level = level;
  cfg.last_level = level;
  cfg.max_iterations_per_level = warm_iterations + 2;
  cfg.precision = 0.0;                                      // the warm-up iterations are never cut short by the stopping rule
  BatchPlan bp;
  int rc = prepare_single(ctx, n_pairs, references, currents, &cfg, bp);
  if (rc != DVO_HIP_OK) return rc;
  Workspace& w = ctx->ws[0];
  rc = ensure_host_status(w, 8);
  if (rc != DVO_HIP_OK) { ctx->err = w.err; return rc; }
  hipStream_t s = ctx->stream;
  const LevelGeom& g = bp.geom[level];
  const PairPtrs* pp = bp.pair_ptrs + size_t(level) * bp.n;
  std::vector<double> tinit(size_t(bp.n) * 16, 0.0);
  for (int i = 0; i < bp.n; ++i)
    for (int k = 0; k < 4; ++k) tinit[size_t(i) * 16 + k * 5] = 1.0;
  DVO_HIP_TRY(ctx, hipMemcpyAsync(w.t_init.p, tinit.data(), tinit.size() * sizeof(double), hipMemcpyHostToDevice, s));
  ctx->tables.forget(w.t_init.p);
  PairState* states = w.states.as<PairState>();
  launch_init_pairs(s, states, bp.n, bp.prm, w.t_init.as<double>());
  launch_level_begin(s, states, bp.n, bp.prm, g, level, pp, w.lvl_stats.as<dvo_hip_level_stats>());
  auto sweep = [&]() {
    launch_residual_reduce(s, bp.choice[level], bp.rpw[level], level == 0, g, pp, states, bp.n, w.partials.as<float>(), w.scratch.as<float2>(),
                           w.win_fallbacks.as<unsigned long long>());
  };
  // `warm_iterations` Gauss-Newton steps first: the timed sweeps then run where the sweeps of a match run -- at the transform
  // the solver moved to, with the t-distribution weights on (first = 0) -- instead of at the identity with unit weights
  for (int it = 0; it < warm_iterations; ++it) {
    sweep();
    launch_loglik(s, g, states, bp.n, w.partials.as<float>(), w.scratch.as<float2>(), w.ll_partials.as<double>(), kLlBlocksPerPair);
    DVO_HIP_TRY(ctx, hipMemsetAsync(w.counters.p, 0, sizeof(unsigned long long), s));
    launch_solver_step(s, states, bp.n, bp.prm, g, w.partials.as<float>(), w.ll_partials.as<double>(), kLlBlocksPerPair, nullptr,
                       w.lvl_stats.as<dvo_hip_level_stats>(), w.it_stats.as<dvo_hip_iteration_stats>(), w.counters.as<unsigned long long>(),
                       w.host_status);
  }
  // a pair whose last warm-up step was rejected (log-likelihood not improved) left the level: the timed sweeps cover every pair
  if (warm_iterations > 0) launch_force_active(s, states, bp.n);
  hipEvent_t e0, e1;
  DVO_HIP_TRY(ctx, hipEventCreate(&e0));
  DVO_HIP_TRY(ctx, hipEventCreate(&e1));
  sweep();   // warm
  DVO_HIP_TRY(ctx, hipEventRecord(e0, s));
  for (int r = 0; r < reps; ++r) sweep();
  DVO_HIP_TRY(ctx, hipEventRecord(e1, s));
  DVO_HIP_TRY(ctx, hipEventSynchronize(e1));
  float ms = 0;
  DVO_HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  DVO_HIP_TRY(ctx, hipGetLastError());
  *avg_ms = ms / float(reps);
  return DVO_HIP_OK;
}

int dvo_hip_time_stream_mix(dvo_hip_context* ctx, int n_pairs, dvo_hip_frame* const* references, dvo_hip_frame* const* currents,
                            int level, int with_write, int reps, float* avg_ms) {
  DVO_ENTER(ctx);
  if (!avg_ms || reps < 1) return fail(ctx, DVO_HIP_ERR_INVALID, "time_stream_mix: bad argument");
  dvo_hip_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.first_level = level;
  cfg.last_level = level;
  cfg.max_iterations_per_level = 1;
  BatchPlan bp;
  int rc = prepare_single(ctx, n_pairs, references, currents, &cfg, bp);
  if (rc != DVO_HIP_OK) return rc;
  hipStream_t s = ctx->stream;
  const LevelGeom& g = bp.geom[level];
  const PairPtrs* pp = bp.pair_ptrs + size_t(level) * bp.n;
  // without the write the kernel folds what it read into one float per workgroup (the partials buffer is large enough)
  float2* scratch = with_write ? ctx->ws[0].scratch.as<float2>() : nullptr;
  float* sink = ctx->ws[0].partials.as<float>();
  hipEvent_t e0, e1;
  DVO_HIP_TRY(ctx, hipEventCreate(&e0));
  DVO_HIP_TRY(ctx, hipEventCreate(&e1));
  const bool window_planes = bp.choice[level].reads_c;   // the planes the level's sweep really reads
  launch_stream_mix(s, pp, bp.n, g.w * g.h, scratch, sink, window_planes);   // warm
  DVO_HIP_TRY(ctx, hipEventRecord(e0, s));
  for (int r = 0; r < reps; ++r) launch_stream_mix(s, pp, bp.n, g.w * g.h, scratch, sink, window_planes);
  DVO_HIP_TRY(ctx, hipEventRecord(e1, s));
  DVO_HIP_TRY(ctx, hipEventSynchronize(e1));
  float ms = 0;
  DVO_HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  DVO_HIP_TRY(ctx, hipGetLastError());
  *avg_ms = ms / float(reps);
  return DVO_HIP_OK;
}

}  // extern "C"
