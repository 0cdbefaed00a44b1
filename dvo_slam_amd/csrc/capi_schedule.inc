// capi_schedule.inc -- how a batch is run: its plan (levels, tiles, buffers), the waits on the device's status words, which levels the resident
// and the fused coarse-level kernels take, and run_batch, the coarse-to-fine Gauss-Newton driver of a batch on the launch path, in parts:
// preparation, the one-launch prefixes, one level of the chain, the way out, the repeats.  The slow lane of a batch's stragglers is a unit
// of its own, capi_lane.inc, included in front of those parts.  Textually included by capi.hip inside its anonymous namespace, behind
// capi_frames.inc.
struct BatchPlan {
  int n = 0, nlev = 0, cap_levels = 0, cap_iters = 0;
  SolverParams prm;
  const CameraGeom* cam = nullptr;
  std::vector<int> rpw;          // per absolute level
  std::vector<LevelGeom> geom;   // per absolute level
  SweepOptions sweep;            // the options the choices were made under (sweep_options at make_plan's time)
  std::vector<SweepChoice> choice;   // per absolute level: which sweep runs it (sweep_choice.h); geom and rpw follow from it
  PairPtrs* pair_ptrs = nullptr; // device [levels][n] (null when the table only travels in kernel arguments)
  std::vector<PairPtrs> host_ptrs;   // the same table on the host
  int coarse_levels = 0;         // leading levels (first_level, first_level - 1, ...) the fused coarse-level kernel runs (plan_coarse)
  bool ref_order = false;        // option "ref_order": every level on the launch path, with the passes of ref_order.hip
};

int validate_batch(dvo_hip_context* ctx, int n, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, const dvo_hip_config* cfg) {
  if (!ctx || n < 1 || !refs || !curs || !cfg) return fail(ctx, DVO_HIP_ERR_INVALID, "match: null argument");
  if (cfg->first_level < cfg->last_level || cfg->last_level < 0 || cfg->first_level >= kMaxLevels)   // Config::IsSane, DT.cpp:74
    return fail(ctx, DVO_HIP_ERR_INVALID, "match: need 0 <= last_level <= first_level < DVO_HIP_MAX_LEVELS");
  if (cfg->max_iterations_per_level < 1) return fail(ctx, DVO_HIP_ERR_INVALID, "match: max_iterations_per_level < 1");
  const int need_levels = cfg->first_level + 1;   // Config::getNumLevels
  const CameraGeom* cam = refs[0] ? refs[0]->cam : nullptr;
  for (int i = 0; i < n; ++i) {
    if (!refs[i] || !curs[i]) return fail(ctx, DVO_HIP_ERR_INVALID, "match: null frame");
    if (refs[i]->levels < need_levels || curs[i]->levels < need_levels)
      return fail(ctx, DVO_HIP_ERR_INVALID, "match: frame pyramid has fewer levels than first_level + 1");
    if (refs[i]->cam != cam || curs[i]->cam != cam)
      return fail(ctx, DVO_HIP_ERR_INVALID, "match: all frames of a batch must share size and intrinsics");
  }
  return DVO_HIP_OK;
}

void make_plan(const dvo_hip_context* ctx, const CameraGeom* cam, const dvo_hip_config* cfg, int n, BatchPlan& bp) {
  const int need_levels = cfg->first_level + 1;
  bp.n = n;
  bp.cam = cam;
  bp.nlev = cfg->first_level - cfg->last_level + 1;
  bp.cap_levels = bp.nlev;
  bp.cap_iters = bp.nlev * cfg->max_iterations_per_level;
  bp.prm.max_iterations = cfg->max_iterations_per_level;
  bp.prm.first_level = cfg->first_level;
  bp.prm.last_level = cfg->last_level;
  bp.prm.use_initial_estimate = cfg->use_initial_estimate;
  bp.prm.precision = cfg->precision;
  bp.prm.mu = cfg->mu;
  bp.ref_order = ctx->opt_ref_order != 0;
  bp.prm.cap_iters = bp.cap_iters;
  bp.prm.cap_levels = bp.cap_levels;
  bp.prm.max_points_level0 = cam->w0 * cam->h0;
  bp.prm.want_condition_number = ctx->opt_condition_number;
  bp.prm.record_prefilled = 0;
  bp.rpw.assign(need_levels, 1);
  bp.geom.resize(need_levels);
  bp.sweep = sweep_options(ctx);
  bp.choice.resize(need_levels);
  for (int l = cfg->last_level; l <= cfg->first_level; ++l) {
    bp.choice[l] = choose_sweep(bp.sweep, cam->w[l], cam->h[l]);
    bp.rpw[l] = pick_rows_per_wave(ctx, cam, l, n, bp.choice[l]);
    bp.geom[l] = make_geom(ctx, cam, l, bp.rpw[l], bp.choice[l]);
  }
}

// buildAccelerationStructure for the current frames, PointSelection::select for the reference frames (both cached per
// frame and level); enqueued on the context's main stream
// `launch_path_only`: the caller runs every level on the launch-per-step path (the parity / measurement entry points)
int resident_levels_of(const dvo_hip_context* ctx, const dvo_hip_config* cfg, BatchPlan& bp, dvo_hip_frame* const* curs);

// Option "ref_order", Q3 (ref_order.hip::k_ref_order_drop_last): the reference planes R of a batch's levels lose the last selected pixel of
// an odd selection, once per build of the plane (FrameLevel::q3).  The edit keeps the pixel it cleared in the frame's block of selection
// counts and a match without the option puts it back (k_ref_order_restore): no plane is built again -- a reference frame ingested without
// a copy of its raw planes could not be.
int ref_order_planes(dvo_hip_context* ctx, int n, dvo_hip_frame* const* refs, const dvo_hip_config* cfg) {
  const bool edit = ctx->opt_ref_order != 0;
  std::vector<RefOrderPlane> host;
  for (int i = 0; i < n; ++i)
    for (int l = cfg->last_level; l <= cfg->first_level; ++l) {
      FrameLevel& L = refs[i]->lv[l];
      if (L.q3 == edit) continue;                              // (also the second visit of a frame listed twice)
      L.q3 = edit;
      RefOrderPlane p;
      p.R = L.R;
      p.count = refs[i]->sel_count + l;
      p.saved = ref_order_saved_slot(refs[i]->sel_count, l);
      p.npx = L.w * L.h;
      p.pad = 0;
      host.push_back(p);
    }
  if (host.empty()) return DVO_HIP_OK;
  DVO_HIP_TRY(ctx, ctx->ref_order_planes.reserve(host.size() * sizeof(RefOrderPlane)));
  DVO_HIP_TRY(ctx, ctx->tables.upload(ctx->stream, ctx->ref_order_planes.p, host.data(), host.size() * sizeof(RefOrderPlane)));
  if (edit) launch_ref_order_drop_last(ctx->stream, ctx->ref_order_planes.as<RefOrderPlane>(), int(host.size()));
  else launch_ref_order_restore(ctx->stream, ctx->ref_order_planes.as<RefOrderPlane>(), int(host.size()));
  DVO_HIP_TRY(ctx, hipGetLastError());
  return DVO_HIP_OK;
}

int ensure_batch_roles(dvo_hip_context* ctx, int n, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, const dvo_hip_config* cfg,
                       bool launch_path_only = false) {
  Range range("build");
  ctx->last_sel_ithr = cfg->intensity_derivative_threshold;   // (what a speculative reference preparation will assume, prepare_roles)
  ctx->last_sel_dthr = cfg->depth_derivative_threshold;
  int rc = wait_for_build(ctx, n, refs);
  if (rc == DVO_HIP_OK) rc = wait_for_build(ctx, n, curs);
  if (rc != DVO_HIP_OK) return rc;
  // the flavour of the current role each level is read in: the resident kernel and the gathering sweep read the taps A + B, the
  // window sweep the 8-byte plane C
  BatchPlan bp;
  make_plan(ctx, curs[0]->cam, cfg, n, bp);
  const int resident = launch_path_only ? 0 : resident_levels_of(ctx, cfg, bp, curs);
  int want[kMaxLevels];
  for (int l = 0; l < kMaxLevels; ++l)   // (ensure_roles looks at the batch's levels only)
    want[l] = l < cfg->last_level || l > cfg->first_level - resident || !bp.choice[l].reads_c ? kCurAB : kCurC;
  rc = ensure_roles(ctx, n, curs, 0, cfg->last_level, cfg->first_level, 0.0f, 0.0f, /*eager=*/false, want);
  if (rc == DVO_HIP_OK)
    rc = ensure_roles(ctx, n, refs, 1, cfg->last_level, cfg->first_level, cfg->intensity_derivative_threshold, cfg->depth_derivative_threshold);
  if (rc == DVO_HIP_OK) rc = ref_order_planes(ctx, n, refs, cfg);
  return rc;
}

// Device scratch for n pairs + the per-level pointer tables
int prepare_buffers(Workspace& w, const dvo_hip_config* cfg, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, BatchPlan& bp,
                    bool upload_table = true) {
  const int n = bp.n, need_levels = cfg->first_level + 1;
  size_t max_tiles = 1;
  for (int l = cfg->last_level; l <= cfg->first_level; ++l) max_tiles = std::max(max_tiles, size_t(bp.geom[l].tiles_x) * bp.geom[l].tiles_y);
  size_t npx = 0;                                             // residual entries per pair: the largest level's (packed ones own whole tiles)
  for (int l = cfg->last_level; l <= cfg->first_level; ++l) npx = std::max(npx, residual_entries(bp.geom[l]));
  DVO_WS_TRY(w, w.states.reserve(size_t(n) * sizeof(PairState)));

  DVO_WS_TRY(w, w.partials.reserve(size_t(n) * max_tiles * kAccStride * sizeof(float)));
  DVO_WS_TRY(w, w.scratch.reserve(size_t(n) * npx * sizeof(float2)));
  DVO_WS_TRY(w, w.ll_partials.reserve(size_t(n) * kLlBlocksPerPair * sizeof(double)));
  DVO_WS_TRY(w, w.lvl_stats.reserve(size_t(n) * bp.cap_levels * sizeof(dvo_hip_level_stats)));
  DVO_WS_TRY(w, w.it_stats.reserve(size_t(n) * bp.cap_iters * sizeof(dvo_hip_iteration_stats)));
  DVO_WS_TRY(w, w.results.reserve(size_t(n) * sizeof(dvo_hip_result)));
  DVO_WS_TRY(w, w.pair_sums.reserve(size_t(n) * kPairSumsStride * sizeof(double)));
  if (bp.ref_order) {
    int max_h = 1;
    for (int l = cfg->last_level; l <= cfg->first_level; ++l) max_h = std::max(max_h, bp.geom[l].h);
    DVO_WS_TRY(w, w.ref_rows.reserve(size_t(n) * max_h * sizeof(RefOrderSeg)));
    DVO_WS_TRY(w, w.ref_pairs.reserve(size_t(n) * sizeof(RefOrderPair)));
  }
  DVO_WS_TRY(w, w.t_init.reserve(size_t(n) * 16 * sizeof(double)));
  // per-step tallies, and behind them one arrival word per pair (the sweeps' tail, solver_step.h): cleared together at the start of a batch
  DVO_WS_TRY(w, w.counters.reserve(size_t(bp.cap_iters + 8 + kResidentErrorWords) * sizeof(unsigned long long) + align_up(size_t(n) * sizeof(int), 8)));
  if (!w.win_fallbacks.p) {
    DVO_WS_TRY(w, w.win_fallbacks.reserve(64));
    DVO_WS_TRY(w, hipMemsetAsync(w.win_fallbacks.p, 0, 64, w.stream));
  }
  if (w.f16_range_words < size_t(n)) {
    // (the words are only ever written by sweeps of a batch that is over by the time the next one is prepared: a larger array can
    // replace the old one here once the stream has drained)
    if (w.f16_range_flag) {
      DVO_WS_TRY(w, hipStreamSynchronize(w.stream));
      (void)hipHostFree(w.f16_range_flag);
      w.f16_range_flag = nullptr;
      w.f16_range_words = 0;
    }
    const size_t words = std::max<size_t>(64, size_t(n));
    DVO_WS_TRY(w, hipHostMalloc(reinterpret_cast<void**>(&w.f16_range_flag), words * sizeof(int), hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(w.f16_range_flag, 0, words * sizeof(int));
    w.f16_range_words = words;
  }
  std::vector<PairPtrs>& host = bp.host_ptrs;
  host.assign(size_t(n) * need_levels, PairPtrs());
  for (int l = cfg->last_level; l <= cfg->first_level; ++l)
    for (int i = 0; i < n; ++i) {
      PairPtrs& p = host[size_t(l) * n + i];
      p.refR = refs[i]->lv[l].R;
      p.curA = curs[i]->lv[l].A;
      p.curB = curs[i]->lv[l].B;
      p.n_selected = refs[i]->sel_count + l;
      p.curC = curs[i]->lv[l].C;
    }
  bp.pair_ptrs = nullptr;
  if (upload_table) {
    int slot = w.tables->holder(w.pair_ptrs, Workspace::kTableSlots, w.stream, host.data(), host.size() * sizeof(PairPtrs));
    if (slot < 0) slot = int(w.pair_ptrs_next++ % Workspace::kTableSlots);
    DevBuf& pair_ptrs = w.pair_ptrs[slot];
    DVO_WS_TRY(w, pair_ptrs.reserve(size_t(n) * need_levels * sizeof(PairPtrs)));
    DVO_WS_TRY(w, w.tables->upload(w.stream, pair_ptrs.p, host.data(), host.size() * sizeof(PairPtrs)));
    bp.pair_ptrs = pair_ptrs.as<PairPtrs>();
  }
  return DVO_HIP_OK;
}

// Spin on the pinned status word the device writes when the last workgroup of a step is through (publish_step in
// solver_kernels.hip).  A host-memory poll sees the word ~2 us after the store; an event synchronisation took ~10 us.
int step_wait_check(Workspace& w, std::chrono::steady_clock::time_point t0) {
  const hipError_t q = hipStreamQuery(w.stream);
  if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();   // "still running" is not an error to keep
  if (q != hipSuccess && q != hipErrorNotReady) {
    w.err = std::string("match: stream failed while waiting for a Gauss-Newton step: ") + hipGetErrorString(q);
    return DVO_HIP_ERR_HIP;
  }
  if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
    w.err = "match: timed out waiting for a Gauss-Newton step";
    return DVO_HIP_ERR_HIP;
  }
  return DVO_HIP_OK;
}

int wait_for_step(Workspace& w, int step, int* active) {
  volatile int* word = w.host_status + step;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    const int v = *word;
    if (v & kStepDoneFlag) {
      *active = v & ~kStepDoneFlag;
      return DVO_HIP_OK;
    }
    if ((spins & 0xfffff) == 0) {                            // every ~1M polls: has the stream died, or are we stuck?
      const int rc = step_wait_check(w, t0);
      if (rc != DVO_HIP_OK) return rc;
    }
  }
}

// The direct path of the resident kernel: spin on the pinned word in which the kernel counts the pairs whose results (and statistics)
// are complete in pinned host memory; a group that timed out raises the error word instead (the caller repeats the batch).
int wait_for_direct(Workspace& w, int n_pairs) {
  volatile int* done = w.direct_done.as<int>();
  volatile int* error_word = w.host_status + w.resident_error_word;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    if (*error_word != 0) return DVO_HIP_OK;                 // (looked at first: an error raised in this launch is reported by this launch)
    if (*done >= n_pairs) {
      std::atomic_thread_fence(std::memory_order_acquire);
      return DVO_HIP_OK;
    }
    if ((spins & 0xfffff) == 0) {
      const hipError_t q = hipStreamQuery(w.stream);
      if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();
      if (q == hipSuccess && *done < n_pairs && *error_word == 0) {   // the kernel is gone and has not reported: it never ran
        w.err = "match: the resident kernel ended without reporting its pairs";
        return DVO_HIP_ERR_HIP;
      }
      if (q != hipSuccess && q != hipErrorNotReady) {
        w.err = std::string("match: stream failed while the resident kernel ran: ") + hipGetErrorString(q);
        return DVO_HIP_ERR_HIP;
      }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
        w.err = "match: timed out waiting for the resident kernel";
        return DVO_HIP_ERR_HIP;
      }
    }
  }
}

// pinned status words the device writes (publish_step): coherent + mapped, so that a system-scope store is visible to the
// polling host thread whatever HIP_HOST_COHERENT says
int ensure_host_status(Workspace& w, size_t n_steps) {
  if (w.host_status_words < n_steps) {
    if (w.host_status) (void)hipHostFree(w.host_status);
    w.host_status = nullptr;
    w.host_status_words = 0;
    DVO_WS_TRY(w, hipHostMalloc(reinterpret_cast<void**>(&w.host_status), n_steps * sizeof(int), hipHostMallocCoherent | hipHostMallocMapped));
    w.host_status_words = n_steps;
  }
  return DVO_HIP_OK;
}

// ---- the resident kernel: which levels, how many workgroups per pair ------------------------------------------------------------
// Workgroups of a group wait for each other, so all groups in flight on a device must be on it together.  Contexts of one process
// (one per host thread, like the reference's one DenseTracker per TBB worker, keyframe_graph.cpp:576-593) share a per-device budget
// of compute units: launches with groups run SIDE BY SIDE as long as their workgroups fit the device together (one 512-thread
// workgroup per compute unit), and wait for each other beyond that.  (Round 2 let only one such launch run at a time: side by side,
// one launch in seven had timed out.  The cause was the exchange's missing flow control towards idle workgroups -- fixed in
// align_resident.hip, "Flow control" -- which a second launch on the device, delaying some workgroups' start, merely exposed.)
// Another PROCESS on the same device is not seen here; there a group can time out, and the batch is repeated on the launch path.
struct ResidentBudget {
  std::mutex m;
  std::condition_variable cv;
  int in_flight = 0;
  static ResidentBudget& of(int device) {
    static ResidentBudget budgets[64];
    return budgets[device >= 0 && device < 64 ? device : 63];
  }
  struct Hold {
    ResidentBudget* b = nullptr;
    int n = 0;
    Hold() = default;
    Hold(const Hold&) = delete;
    Hold& operator=(const Hold&) = delete;
    void take(ResidentBudget& budget, int workgroups, int capacity) {
      std::unique_lock<std::mutex> lock(budget.m);
      budget.cv.wait(lock, [&] { return budget.in_flight == 0 || budget.in_flight + workgroups <= capacity; });
      budget.in_flight += workgroups;
      b = &budget;
      n = workgroups;
    }
    ~Hold() {
      if (!b) return;
      {
        std::lock_guard<std::mutex> lock(b->m);
        b->in_flight -= n;
      }
      b->cv.notify_all();
    }
  };
};

constexpr int kResidentRowsDefault = 24;      // segments per wavefront and iteration up to which a level runs resident


struct ResidentPlan {
  int group = 1;                               // workgroups per pair
  int levels = 0;                              // leading levels (first_level, first_level - 1, ...) that run resident
  bool direct = false;                         // the whole match of a small batch: results and statistics land in pinned host memory
};

constexpr size_t kResidentDirectStatsBytes = size_t(64) << 20;

// `taps_missing`: current frames of the batch hold plane C but not the taps A + B on the level below the first one (they were ingested
// straight into their role in a batch of an eighth as many frames as compute units or more, eager_current_flavor): the resident kernel
// would have to have the taps derived for it first
bool window_taps_missing(const dvo_hip_config* cfg, const BatchPlan& bp, dvo_hip_frame* const* curs) {
  const int level = cfg->first_level - 1;
  if (level < cfg->last_level || !bp.choice[level].windowed()) return false;
  for (int i = 0; i < bp.n; ++i) {
    const int have = curs[i]->lv[level].cur_have;
    if ((have & kCurC) && !(have & kCurAB)) return true;
  }
  return false;
}

ResidentPlan plan_resident(const dvo_hip_context* ctx, const dvo_hip_config* cfg, const BatchPlan& bp, bool taps_missing) {
  ResidentPlan rp;
  // (deterministic: one path whatever the batch size, and that is the launch path; ref_order: its passes are the launch path's)
  if (ctx->opt_resident == 0 || ctx->opt_deterministic || ctx->opt_ref_order) return rp;
  const int cus = ctx->compute_units > 0 ? ctx->compute_units : 256;
  // more pairs than compute units: the workgroups would run in shifts, and the launch path, which gives every phase the whole chip,
  // is as fast (measured: 256 pairs -3 %, 512 pairs +1.6 % against it).  (Not with a pinned group size: the caller asks for
  // records that do not depend on the batch size, so the choice of path must not either.)
  // (round 3: with the f16 Gram and the short tiles the launch path is level with or ahead of ONE workgroup per pair as well -- 192 / 256
  // pairs: screening stage 0.278 / 0.306 vs 0.293 / 0.341 ms, levels 3 -> 1 0.82 / 0.95 vs 0.87 / 1.01, full match equal; the resident
  // kernel is kept for batches that get at least two workgroups per pair -- with launches limited to half the chip that is
  // pairs <= compute units / 4.  Measured at the end of round 3, 96 / 128 pairs with ONE workgroup each: full match 1.63 / 1.93 ms
  // resident against 1.61 / 1.90 on the launch path, levels 3 -> 1 0.60 / 0.67 against 0.57 / 0.65, and a streaming step of 128 pairs
  // beside its background ingest 2.50 against 2.41 ms; at 64 pairs (two workgroups each) resident still wins, 1.19 against 1.26.)
  // (round 5: up to 7/16 as many pairs as compute units the FIRST level alone -- 18 of a streaming step's 34 iterations in BASELINE
  // config 4, each a sweep and a solver launch of 11 + 12 us -- is still quicker resident with two workgroups per pair, which leave
  // an eighth of the chip to the background ingest: streaming step of 72 / 80 / 96 / 112 pairs 1.215 / 1.283 / 1.440 / 1.634 ->
  // 1.172 / 1.232 / 1.378 / 1.587 ms.  128 pairs: two workgroups each 1.808 against 1.776, one 1.748 on one box and level on two
  // others -- left on the launch path; with the second level resident as well 1.59 at 96 pairs.  Only a level the launch path
  // reads through the taps too: its planes exist.)
  // (the same from an eighth of the compute units on when the batch came from a streaming ingest that left the taps out -- see
  // eager_current_flavor; frames that hold them, or nothing yet, get the coarse levels resident as before: a match of 64 prepared pairs
  // 0.96 ms against 1.02 with the first level alone)
  const BatchPolicy policy(ctx->compute_units);
  const bool first_level_only = ctx->opt_resident < 0 && ctx->opt_resident_group == 0 &&
                                (!policy.resident_takes_coarse_levels(bp.n) || (policy.taps_missing_prefers_first_level_only(bp.n) && taps_missing));
  if (first_level_only && (!policy.resident_first_level_fits(bp.n) || bp.choice[cfg->first_level].windowed())) return rp;
  // all workgroups of a launch with groups must be resident at once: one workgroup (8 wavefronts, up to 256 registers) per compute unit
  int group = 1;
  while (group * 2 <= kResidentMaxGroup && bp.n * group * 2 <= cus) group *= 2;
  if (ctx->opt_resident_group > 0) group = std::min(group, ctx->opt_resident_group);
  if (first_level_only) {                                       // the groups leave an eighth of the chip free
    group = 1;
    while (group * 2 <= kResidentMaxGroup && bp.n * group * 2 * 8 <= cus * 7) group *= 2;
  }
  rp.group = group;
  const int rows_max = ctx->opt_resident_rows > 0 ? ctx->opt_resident_rows : kResidentRowsDefault;
  for (int level = cfg->first_level; level >= cfg->last_level; --level) {
    const int segments = (bp.cam->w[level] * bp.cam->h[level] + kTileW - 1) / kTileW;
    const int rows = (segments + group * kResidentSweepers - 1) / (group * kResidentSweepers);
    if (ctx->opt_resident != 1 && rows > rows_max) break;
    if (first_level_only && rp.levels == 1) break;
    if (size_t(bp.cam->w[level]) * bp.cam->h[level] >= (size_t(1) << 24)) break;   // the kernel locates a pixel with one float multiply
    rp.levels += 1;
  }
  static const bool trace_plan = std::getenv("DVO_HIP_TRACE_PLAN") != nullptr;     // (stderr: which plan a batch got)
  if (trace_plan)
    std::fprintf(stderr, "plan_resident: %d pairs, taps missing %d -> %s, %d workgroup(s) per pair, %d level(s) resident\n", bp.n, int(taps_missing),
                 first_level_only ? "first level only" : "coarse levels", rp.group, rp.levels);
  rp.direct = rp.levels == cfg->first_level - cfg->last_level + 1 && bp.n <= policy.resident_direct_max_pairs() &&
              size_t(bp.n) * bp.cap_iters * sizeof(dvo_hip_iteration_stats) <= kResidentDirectStatsBytes;   // (pinned, if asked for)
  return rp;
}

// ---- the fused coarse-level kernel (align_coarse.hip): which levels -----------------------------------------------------------------
// One workgroup per pair runs the leading levels of the match to their termination in ONE launch (sweep over all tiles, reduction,
// log-likelihood, loop body), with the launch path's device functions on the launch path's data layout: the records are the launch
// path's bit for bit.  The levels: from the first one down, as long as the level is small (kCoarseMaxPixels) and the kernel has an
// instantiation for it (coarse_kernel_takes).  OPT-IN (option "coarse" 1): measured in round 6 against the launch path at 128 / 256 /
// 512 / 1024 pairs per step and slower at every size (1.80 -> 3.08, 3.16 -> 4.43, 6.0 -> 7.2, 11.5 -> 12.5 ms per streaming step): a
// workgroup walks the 10 + 34 tiles of levels 3 and 2 one after the other -- 60 / 200 us per iteration where the launch path, which
// spreads the tiles of an iteration over the chip, needs 25 / 40 -- and with as many pairs as workgroup slots (1024 = 256 compute units x
// 4) the launch lasts as long as its slowest pair (15 + 9 iterations against a mean of 8 + 5).  It pays where pairs outnumber the slots
// several times over; kept for that case and as the bit-exact cross-check of the launch path's hand-over logic.
constexpr int kCoarseMaxPixels = 160 * 120;

void plan_coarse(const dvo_hip_context* ctx, const dvo_hip_config* cfg, BatchPlan& bp, const ResidentPlan& rp) {
  bp.coarse_levels = 0;
  if (ctx->opt_coarse == 0 || rp.levels > 0 || bp.sweep.variant != 8 || ctx->opt_ref_order) return;
  const int max_pixels = ctx->opt_coarse_pixels > 0 ? ctx->opt_coarse_pixels : kCoarseMaxPixels;
  for (int level = cfg->first_level; level >= cfg->last_level; --level) {
    if (bp.cam->w[level] * bp.cam->h[level] > max_pixels) break;
    const SweepChoice& choice = bp.choice[level];
    const int rpw = choice.tile_rows > 0 ? choice.tile_rows : kCoarseRowsPerWave;
    if (choice.tile_rows == 0 && ctx->opt_rows_per_wave > 0 && ctx->opt_rows_per_wave != rpw) break;   // (a tile height asked for by name stays)
    const LevelGeom g = make_geom(ctx, bp.cam, level, rpw, choice);
    if (!coarse_kernel_takes(choice, g)) break;
    bp.rpw[level] = rpw;
    bp.geom[level] = g;
    bp.coarse_levels += 1;
  }
}

// which of the two one-launch kernels takes the leading levels of a batch, if any
ResidentPlan plan_paths(const dvo_hip_context* ctx, const dvo_hip_config* cfg, BatchPlan& bp, bool taps_missing) {
  ResidentPlan rp = plan_resident(ctx, cfg, bp, taps_missing);
  if (ctx->opt_coarse == 1) {                                  // (option "coarse" 1: the fused coarse-level kernel wherever the levels admit it)
    const ResidentPlan none;
    plan_coarse(ctx, cfg, bp, none);
    if (bp.coarse_levels > 0) rp = none;
  } else {
    plan_coarse(ctx, cfg, bp, rp);
  }
  return rp;
}

int resident_levels_of(const dvo_hip_context* ctx, const dvo_hip_config* cfg, BatchPlan& bp, dvo_hip_frame* const* curs) {
  return plan_paths(ctx, cfg, bp, window_taps_missing(cfg, bp, curs)).levels;
}

int run_resident(dvo_hip_context* ctx, Workspace& w, const dvo_hip_config* cfg, const BatchPlan& bp, const ResidentPlan& rp,
                 const double* tinit, bool want_stats) {
  hipStream_t s = w.stream;
  ResidentArgs args;
  std::memset(&args, 0, sizeof(args));
  for (int l = cfg->last_level; l <= cfg->first_level; ++l) args.geom[l] = bp.geom[l];
  args.pair_ptrs = bp.pair_ptrs;
  args.states = w.states.as<PairState>();
  args.levels = w.lvl_stats.as<dvo_hip_level_stats>();
  args.iters = w.it_stats.as<dvo_hip_iteration_stats>();
  args.T_init = w.t_init.as<double>();
  args.scratch = w.scratch.as<float2>();
  args.error_word = w.host_status + w.resident_error_word;
  args.prm = bp.prm;
  args.n_pairs = bp.n;
  args.group = rp.group;
  args.first_level = cfg->first_level;
  args.last_level = cfg->first_level - rp.levels + 1;
  args.flags = ctx->opt_resident_flags;
  args.results = args.last_level == cfg->last_level ? w.results.as<dvo_hip_result>() : nullptr;
  if (bp.n <= kResidentInline) {                               // no table in device memory, no copy commands in front of the launch
    args.use_inline = 1;
    for (int l = cfg->last_level; l <= cfg->first_level; ++l)
      for (int i = 0; i < bp.n; ++i) args.inline_ptrs[l * bp.n + i] = bp.host_ptrs[size_t(l) * bp.n + i];
    std::memcpy(args.inline_T, tinit, size_t(bp.n) * 16 * sizeof(double));
  }
  if (rp.direct) {
    DVO_WS_TRY(w, w.direct_results.reserve(size_t(bp.n) * sizeof(dvo_hip_result)));
    DVO_WS_TRY(w, w.direct_done.reserve(64));
    args.results = w.direct_results.as<dvo_hip_result>();
    args.done_word = w.direct_done.as<int>();
    *static_cast<volatile int*>(args.done_word) = 0;
    if (want_stats) {
      DVO_WS_TRY(w, w.direct_levels.reserve(size_t(bp.n) * bp.cap_levels * sizeof(dvo_hip_level_stats)));
      DVO_WS_TRY(w, w.direct_iters.reserve(size_t(bp.n) * bp.cap_iters * sizeof(dvo_hip_iteration_stats)));
      args.host_levels = w.direct_levels.as<dvo_hip_level_stats>();
      args.host_iters = w.direct_iters.as<dvo_hip_iteration_stats>();
    }
  }
  ctx->resident_launches += 1;
  ctx->resident_levels += rp.levels;
  if (rp.group > 1) {
    // the rows of every group, and behind them one heartbeat word per workgroup (align_resident.hip, "Flow control")
    const size_t bytes = size_t(bp.n) * rp.group * kResidentRing * kResidentSlots * sizeof(unsigned long long) + align_up(size_t(bp.n) * rp.group * sizeof(unsigned), 256);
    const bool grown = bytes > w.exchange.bytes;
    DVO_WS_TRY(w, w.exchange.reserve(bytes));
    // sequence numbers never repeat between launches; when they would wrap (or the rows are new / in doubt) the rows are cleared
    const unsigned long long need64 = 2ull * unsigned(rp.levels) * unsigned(cfg->max_iterations_per_level) + 4ull;
    const unsigned need = need64 < 0x40000000ull ? unsigned(need64) : 0x40000000u;   // (more exchanges than that do not happen)
    // (... or the batch has another shape than the last one: the heartbeat words live BEHIND the rows, at an offset that follows pairs x
    // group, and a word that was a row slot of the previous launch -- the float half of a slot, 0x3f800000, reads as a beat far ahead --
    // would let a workgroup skip the wait the heartbeat exists for)
    const long long shape = (long long)bp.n * rp.group;
    if (grown || shape != w.exchange_shape || need64 >= 0x40000000ull || w.resident_sequence > 0xffffffffu - need - 1u) {
      DVO_WS_TRY(w, hipMemsetAsync(w.exchange.p, 0, w.exchange.bytes, s));
      w.resident_sequence = 0;
      w.exchange_shape = shape;
    }
    args.exchange = w.exchange.as<unsigned long long>();
    args.sequence_base = w.resident_sequence;
    w.resident_sequence += need;
  }
  DVO_WS_TRY(w, launch_match_resident(s, args, ctx->opt_resident_cooperative != 0));
  return DVO_HIP_OK;
}

int run_coarse(dvo_hip_context* ctx, Workspace& w, const dvo_hip_config* cfg, const BatchPlan& bp) {
  CoarseArgs args;
  std::memset(&args, 0, sizeof(args));
  for (int l = cfg->last_level; l <= cfg->first_level; ++l) args.geom[l] = bp.geom[l];
  args.pair_ptrs = bp.pair_ptrs;
  args.states = w.states.as<PairState>();
  args.levels = w.lvl_stats.as<dvo_hip_level_stats>();
  args.iters = w.it_stats.as<dvo_hip_iteration_stats>();
  args.T_init = w.t_init.as<double>();
  args.partials = w.partials.as<float>();
  args.scratch = w.scratch.as<float2>();
  args.fallback_count = w.win_fallbacks.as<unsigned long long>();
  args.f16_range_flag = w.f16_range_flag;
  args.prm = bp.prm;
  args.n_pairs = bp.n;
  args.first_level = cfg->first_level;
  args.last_level = cfg->first_level - bp.coarse_levels + 1;
  for (int l = args.last_level; l <= args.first_level; ++l) {   // (prepare_buffers sized both buffers for the largest level of the match)
    args.max_tiles = std::max(args.max_tiles, bp.geom[l].tiles_x * bp.geom[l].tiles_y);
    args.max_entries = std::max(args.max_entries, residual_entries(bp.geom[l]));
  }
  args.results = args.last_level == cfg->last_level ? w.results.as<dvo_hip_result>() : nullptr;
  ctx->coarse_launches += 1;
  ctx->coarse_levels += bp.coarse_levels;
  DVO_WS_TRY(w, launch_match_coarse(w.stream, args, ctx->opt_coarse_wgs == 3 ? 3 : 4));
  return DVO_HIP_OK;
}

std::mutex g_rare_path_mutex;   // (see run_batch: the repeat of pairs that left the f16 range)

constexpr int kF32GramHoldBatches = 32;   // after a batch left the f16 range of the Gram operands: this many batches go straight to the f32 Gram

// ---- run_batch, the coarse-to-fine Gauss-Newton driver of a batch, in parts ----------------------------------------------------------
// What the parts share: the batch as the caller gave it, what was planned for it, the typed device pointers of its buffers and the
// count of the steps enqueued so far.
struct BatchRun {
  dvo_hip_context* const ctx;
  Workspace& w;
  const hipStream_t s;
  const dvo_hip_config* const cfg;
  const int n;
  const BatchPolicy policy;                                    // every batch-size threshold below: batch_policy.h
  BatchPlan bp;
  ResidentPlan rp;
  std::vector<double> tinit;                                   // the initial guesses, 16 doubles per pair
  size_t main_steps = 0, n_steps = 0;                          // status words and tallies: the chain's, and with the slow lane's behind them
  int level_from = 0;                                          // the launch chain's first level (the one-launch kernels take those above it)
  PairState* states = nullptr;
  dvo_hip_level_stats* d_levels = nullptr;
  dvo_hip_iteration_stats* d_iters = nullptr;
  float* partials = nullptr;
  float2* scratch = nullptr;
  double* ll_partials = nullptr;
  RefOrderPair* ref_order = nullptr;                           // (option "ref_order")
  unsigned long long* tallies = nullptr;
  int* arrivals = nullptr;
  int per_level = 0, per_sync = 1;
  int step = kResidentErrorWords;                              // the first status words belong to the resident kernel's launches
  BatchRun(dvo_hip_context* c, const dvo_hip_config* config, int n_pairs)
      : ctx(c), w(c->ws[0]), s(c->ws[0].stream), cfg(config), n(n_pairs), policy(c->compute_units) {}
};

// How the launches of one iteration on `level` are put together; the chain and the slow lane run their pairs by the same rule.
struct LevelSchedule {
  bool fused_ll = false, two_waves = false;
  int ll_blocks = 0;
};
LevelSchedule schedule_of(const BatchRun& b, int level) {
  const dvo_hip_context* ctx = b.ctx;
  const LevelGeom& g = b.bp.geom[level];
  LevelSchedule ls;
  const int fuse_opt = ctx->opt_fused_ll_pixels;
  // levels this small run the log-likelihood sweep inside the solver workgroup (one launch less per iteration)
  // (measured, scripts/ab_match.py fused_ll_pixels: 128 pairs 2.152 -> 2.117 ms with level 1 fused; 16 pairs 0.756 -> 0.799, one
  // pair 0.524 -> 0.547: a lone workgroup per pair is slower than 32 blocks when the chip is empty)
  // (round 5, packed residual pairs, the streaming step beside its ingest, scripts/r5_midsize.py: level 1 in a launch of its own
  // 64 pairs 1.456 -> 1.378 ms, 128 pairs 1.939 -> 1.908, 256 pairs 3.308 -> 3.286, 512 pairs 5.859 -> 5.880: fused from 512 pairs)
  // (option "ref_order": the log-likelihood pass of its own on every level, k_loglik with the pairs' RefOrderPair)
  ls.fused_ll = !b.bp.ref_order && g.w * g.h <= (fuse_opt > 0 ? fuse_opt : (b.policy.fused_loglik_on_large_levels(b.n) && !ctx->opt_deterministic ? kFusedLoglikMaxPixelsBatch : kFusedLoglikMaxPixels));
  // workgroups per pair of the log-likelihood pass: each begins by reducing the pair's scale sums (a latency chain of ~10 us), which
  // a batch that fills the device anyway pays once per workgroup for nothing -- fewer, longer ones then (option ll_blocks to override)
  // (round 5, mid-size batches, scripts/r5_midsize.py: 16 instead of 32 workgroups per pair 64 / 128 / 200 pairs 1.179 -> 1.173 /
  // 1.775 -> 1.760 / 2.558 -> 2.538 ms per step; 8: 1.183 / 1.760 / 2.546)
  ls.ll_blocks = ctx->opt_ll_blocks > 0 ? std::min(ctx->opt_ll_blocks, kLlBlocksPerPair)
                 : (!g.compact || ctx->opt_deterministic ? kLlBlocksPerPair : b.policy.loglik_blocks(b.n));
  // the solver step of the smallest levels in two-wavefront workgroups (four per compute unit instead of two): a batch that otherwise
  // needs two goes of 512 resident workgroups (option solver_waves 2 / 4 to force; the records do not depend on it).  Measured at
  // 1024 pairs (scripts/r4_trace.sh): 80 x 60 46 -> 36 us per step; 160 x 120 with packed residuals 77 -> 90 (two wavefronts walk
  // its 96 slots in six rounds instead of three), 320 x 240 and the finest level level: those keep four.
  ls.two_waves = ctx->opt_solver_waves == 2 ||
                 (ctx->opt_solver_waves == 0 && ls.fused_ll && !g.compact && g.tiles_x * g.tiles_y <= 32 && b.policy.solver_two_waves(b.n));
  return ls;
}

#include "capi_lane.inc"       // the slow lane of a batch (SlowLane): needs the above, and the chain below needs it

// DVO_HIP_TRACE_SLOW=<ms>: where the host thread spent the time before the first launch of a batch whose preparation took longer (stderr).
// prepare_batch sets the marks: 0 roles ensured (dvo_hip_match_batch), 1 plan + buffers + tables, 2 initial guesses + drain, 3 status
// words, 4 stream wait + reset.
hipEvent_t g_trace_ev[2] = {nullptr, nullptr};   // device time stamps around a batch's preparation
struct PrepTrace {
  const dvo_hip_context* ctx;
  hipStream_t s;
  double limit_ms;
  double ms[5] = {0, 0, 0, 0, 0};
  PrepTrace(const dvo_hip_context* c, hipStream_t stream) : ctx(c), s(stream) {
    static const double trace_slow_ms = std::getenv("DVO_HIP_TRACE_SLOW") ? std::atof(std::getenv("DVO_HIP_TRACE_SLOW")) : 0.0;
    limit_ms = trace_slow_ms;
    mark(0);
    if (limit_ms > 0.0) {
      if (!g_trace_ev[0]) { (void)hipEventCreate(&g_trace_ev[0]); (void)hipEventCreate(&g_trace_ev[1]); }
      (void)hipEventRecord(g_trace_ev[0], s);
    }
  }
  void mark(int k) { if (limit_ms > 0.0) ms[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ctx->batch_entry).count(); }
  void before_stream_wait() { if (limit_ms > 0.0) (void)hipEventRecord(g_trace_ev[1], s); }
  void after_stream_wait() {
    if (limit_ms <= 0.0) return;
    mark(4);
    float gpu_ms = -1.0f;
    if (ms[4] - ms[3] > limit_ms && hipEventElapsedTime(&gpu_ms, g_trace_ev[0], g_trace_ev[1]) == hipSuccess)
      std::fprintf(stderr, "dvo_hip: the stream wait took %.3f ms on the host; on the device %.3f ms passed between the batch's first and last command so far\n",
                   ms[4] - ms[3], gpu_ms);
  }
  void report(int n) {
    mark(4);
    if (limit_ms > 0.0 && ms[4] > limit_ms)
      std::fprintf(stderr, "dvo_hip: slow preparation of a %d-pair batch: roles %.3f, plan + buffers + tables %.3f, initial guesses + drain %.3f, status words %.3f, "
                   "stream wait + reset %.3f ms\n", n, ms[0], ms[1] - ms[0], ms[2] - ms[1], ms[3] - ms[2], ms[4] - ms[3]);
  }
};

// Preparation: the plan, the buffers, the initial guesses, the drain of a batch that ended early, the status words and their reset.
int prepare_batch(BatchRun& b, SlowLane& lane, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, const dvo_hip_result* results) {
  dvo_hip_context* ctx = b.ctx;
  Workspace& w = b.w;
  const dvo_hip_config* cfg = b.cfg;
  const int n = b.n;
  BatchPlan& bp = b.bp;
  PrepTrace trace(ctx, b.s);
  make_plan(ctx, refs[0]->cam, cfg, n, bp);
  // The coarse levels -- for a small batch every level -- run inside ONE launch (align_resident.hip): no launch per iteration, no
  // host poll, the pairs of a batch do not wait for each other.
  b.rp = plan_paths(ctx, cfg, bp, window_taps_missing(cfg, bp, curs));
  const bool tables_inline = b.rp.direct && n <= kResidentInline;   // plane pointers and initial guesses travel as kernel arguments
  int rc = prepare_buffers(w, cfg, refs, curs, bp, !tables_inline);
  if (rc != DVO_HIP_OK) return rc;
  trace.mark(1);

  // initial guesses (Result.Transformation is in/out, dense_tracking.cpp:137-147)
  b.tinit.resize(size_t(n) * 16);
  for (int i = 0; i < n; ++i) std::memcpy(&b.tinit[size_t(i) * 16], results[i].transformation, 16 * sizeof(double));
  if (!tables_inline) DVO_WS_TRY(w, w.tables->upload(b.s, w.t_init.p, b.tinit.data(), b.tinit.size() * sizeof(double)));
  // per-step tallies (device) and status words (pinned host memory the device writes, see publish_step)
  b.main_steps = size_t(bp.cap_iters) + 8 + kResidentErrorWords;
  rc = lane.reserve();                                         // the slow lane of the batch (option "overlap_tails"), where it gets one
  if (rc != DVO_HIP_OK) return rc;
  b.n_steps = b.main_steps + lane.steps_cap();                 // (the lane's status words and tallies lie behind the main chain's)
  // (option "tail_lists": the chain's own active-pair list, chain_level)
  if (ctx->opt_tail_lists) DVO_WS_TRY(w, w.chain_list.reserve(align_up(size_t(n), 64) * sizeof(int)));
  // a batch that ended early (time-out, HIP error) may have left steps queued: nothing of it may still be running when the
  // status words and tallies are reset
  if (w.needs_drain) {
    DVO_WS_TRY(w, w.lane.quiesce());
    DVO_WS_TRY(w, sync_stream(b.s));
    // ... and the f16 range words it may have raised are nobody's business any more (they are cleared where they are read, at a batch's
    // regular end: left standing, the next batch would repeat unrelated pairs at the same indices -- round-5 advisor finding)
    if (w.f16_range_flag) std::memset(w.f16_range_flag, 0, w.f16_range_words * sizeof(int));
  }
  w.needs_drain = true;                                        // until this batch has come to its regular end
  trace.mark(2);
  rc = ensure_host_status(w, b.n_steps);
  if (rc != DVO_HIP_OK) return rc;
  trace.mark(3);
  w.resident_error_word = int(w.resident_launch_counter++ % kResidentErrorWords);
  if (b.rp.direct) {
    w.host_status[w.resident_error_word] = 0;
  } else {
    // (the previous batch may have ended on the host's side before the device was through with the step words: the direct path)
    // (only then: a batch that ended with a stream wait left nothing behind, and a wait for the table uploads just enqueued has been
    // seen to return 14-24 ms after the device was done with them -- 19 microseconds by its own time stamps: r03, the validator's
    // 128-pair batches in the first process on a box, never under the profiler)
    trace.before_stream_wait();
    if (w.device_may_lag) DVO_WS_TRY(w, sync_stream(b.s));
    w.device_may_lag = false;
    trace.after_stream_wait();
    std::memset(w.host_status, 0, b.n_steps * sizeof(int));
    DVO_WS_TRY(w, hipMemsetAsync(w.counters.p, 0, b.n_steps * sizeof(unsigned long long) + align_up(size_t(n) * sizeof(int), 8), b.s));
  }

  b.states = w.states.as<PairState>();
  b.d_levels = w.lvl_stats.as<dvo_hip_level_stats>();
  b.d_iters = w.it_stats.as<dvo_hip_iteration_stats>();
  b.partials = w.partials.as<float>();
  b.scratch = w.scratch.as<float2>();
  b.ll_partials = w.ll_partials.as<double>();
  b.ref_order = bp.ref_order ? w.ref_pairs.as<RefOrderPair>() : nullptr;
  b.tallies = w.counters.as<unsigned long long>();
  b.arrivals = reinterpret_cast<int*>(b.tallies + b.n_steps);
  b.per_level = cfg->max_iterations_per_level;
  b.per_sync = ctx->opt_iters_per_sync > 0 ? ctx->opt_iters_per_sync : 1;
  trace.report(n);
  return DVO_HIP_OK;
}

// A recorded ingest of the caller's next batch (option "defer_ingest") is carried out now, behind what this batch has enqueued so far;
// the text of its error becomes the batch's.
int flush_recorded_ingest(BatchRun& b) {
  if (b.ctx->deferred.empty()) return DVO_HIP_OK;
  const int rc_deferred = flush_deferred(b.ctx);
  if (rc_deferred != DVO_HIP_OK) b.w.err = b.ctx->err;
  return rc_deferred;
}

// The one-launch prefixes: the leading levels of the match in the resident kernel or in the fused coarse-level kernel, where the plan
// gave them any; the launch chain begins behind them (level_from).
int run_prefixes(BatchRun& b, bool want_stats) {
  const dvo_hip_config* cfg = b.cfg;
  b.level_from = cfg->first_level;
  if (b.rp.levels > 0) {
    Range range("resident");
    int rc = run_resident(b.ctx, b.w, cfg, b.bp, b.rp, b.tinit.data(), want_stats);
    if (rc == DVO_HIP_OK) rc = flush_recorded_ingest(b);       // (see the launch path, chain_level)
    if (rc != DVO_HIP_OK) return rc;
    b.level_from = cfg->first_level - b.rp.levels;
  }
  if (b.bp.coarse_levels > 0) {
    // the coarse levels of every pair in ONE launch, a workgroup per pair (align_coarse.hip): nothing to poll -- the host goes on to
    // enqueue the first steps of the level behind them
    Range range("coarse");
    int rc = run_coarse(b.ctx, b.w, cfg, b.bp);
    if (rc == DVO_HIP_OK) rc = flush_recorded_ingest(b);
    if (rc != DVO_HIP_OK) return rc;
    b.level_from = cfg->first_level - b.bp.coarse_levels;
  }
  return DVO_HIP_OK;
}

// ---- one level of the launch chain ---------------------------------------------------------------------------------------------------
const char* const kRangePrep[kMaxLevels] = {"prep L0", "prep L1", "prep L2", "prep L3", "prep L4", "prep L5", "prep L6", "prep L7"};
const char* const kRangeErr[kMaxLevels] = {"err L0", "err L1", "err L2", "err L3", "err L4", "err L5", "err L6", "err L7"};
const char* const kRangeLinsys[kMaxLevels] = {"linsys L0", "linsys L1", "linsys L2", "linsys L3", "linsys L4", "linsys L5", "linsys L6", "linsys L7"};

// what the chain's launches of a level share
struct LevelRun {
  int level = 0;
  LevelGeom g;                                                 // every pair of the batch but the slow lane's
  const PairPtrs* pp = nullptr;
  NextLevel next;                                              // where the solver steps hand a pair that has left the level over to
  LevelSchedule schedule;
  bool tail = false;                                           // the step runs in the sweep's launch
  double* pair_sums = nullptr;                                 // ... its wide half only (option "sweep_tail" 2)
  // what the launches cover: every pair, or -- the level's last steps, see "hold" in chain_level -- the list of those still active
  LevelGeom g_run;
  int n_run = 0;
};

// One step in the sweep's launch (round 6): where the log-likelihood pass runs inside the solver step anyway and the level's sweep
// has the instantiation, the workgroup that completes a pair's last tile runs the pair's step -- ONE launch per iteration
// (option 2: the WIDE half of the step -- reduction and log-likelihood, its memory round trips -- in the sweep's tail, the serial half
// in a one-wavefront launch behind it)
void enqueue_step_in_sweep(BatchRun& b, const LevelRun& L) {
  Workspace& w = b.w;
  Range range(kRangeErr[L.level]);
  const SolverStepArgs a = make_solver_step_args(b.states, b.n, b.bp.prm, b.partials, b.ll_partials, L.schedule.ll_blocks, b.scratch, b.d_levels, b.d_iters, b.tallies + b.step,
                                                 w.host_status + b.step, b.cfg->first_level - L.level, &L.next, b.arrivals, L.pair_sums);
  launch_residual_reduce(b.s, b.bp.choice[L.level], b.bp.rpw[L.level], L.level == 0, L.g, L.pp, b.states, b.n, b.partials, b.scratch, w.win_fallbacks.as<unsigned long long>(),
                         w.f16_range_flag, &a);
  if (L.pair_sums) {
    Range range2(kRangeLinsys[L.level]);
    launch_solver_serial(b.s, b.n, L.g, a);
  }
  b.ctx->tail_steps += 1;
}

// One step of the plain chain: the sweep, the passes of option "ref_order", the log-likelihood pass where it is a launch of its own, the
// solver step
void enqueue_step(BatchRun& b, const LevelRun& L) {
  dvo_hip_context* ctx = b.ctx;
  Workspace& w = b.w;
  const bool fused_ll = L.schedule.fused_ll;
  {
    Range range(kRangeErr[L.level]);
    launch_residual_reduce(b.s, b.bp.choice[L.level], b.bp.rpw[L.level], L.level == 0, L.g_run, L.pp, b.states, L.n_run, b.partials, b.scratch, w.win_fallbacks.as<unsigned long long>(),
                           w.f16_range_flag);
    if (b.ref_order) {
      launch_ref_order(b.s, L.g_run, b.states, L.n_run, b.scratch, w.ref_rows.as<RefOrderSeg>(), b.ref_order);
      ctx->ref_order_passes += 1;
    }
    if (!fused_ll) launch_loglik(b.s, L.g_run, b.states, L.n_run, b.partials, b.scratch, b.ll_partials, L.schedule.ll_blocks, ctx->opt_deterministic != 0, b.ref_order);
  }
  if (L.g_run.pair_list) ctx->listed_steps += 1;
  Range range(kRangeLinsys[L.level]);
  launch_solver_step(b.s, b.states, L.n_run, b.bp.prm, L.g_run, b.partials, b.ll_partials, L.schedule.ll_blocks, fused_ll ? b.scratch : nullptr, b.d_levels, b.d_iters,
                     b.tallies + b.step, w.host_status + b.step, L.schedule.two_waves, b.cfg->first_level - L.level, &L.next, b.ref_order);   // (the level record every pair on this level is at: fetched with the state)
}

void enqueue_chunk(BatchRun& b, const LevelRun& L, int count) {
  for (int c = 0; c < count; ++c, ++b.step) {
    if (L.tail) enqueue_step_in_sweep(b, L);
    else enqueue_step(b, L);
  }
}

// The level's pairs begin it (by a launch, or the solver steps of the level before have done it), and what its steps share is put together.
LevelRun begin_level(BatchRun& b, SlowLane& lane, int level) {
  const dvo_hip_context* ctx = b.ctx;
  const dvo_hip_config* cfg = b.cfg;
  const BatchPlan& bp = b.bp;
  const int n = b.n;
  LevelRun L;
  L.level = level;
  L.g = bp.geom[level];
  if (lane.skip_flags()) L.g.skip_flags = lane.skip_flags();   // (the lane's pairs are not this chain's any more)
  L.pp = bp.pair_ptrs + size_t(level) * n;
  // Batches of up to 256 pairs: every level but the launch path's first is begun pair by pair by the solver steps of the level before
  // it, and the results are written by the steps behind the last level (NextLevel) -- no launch between two levels, none at the end:
  // builds alternated on one box, 16 / 64 / 128 pairs 0.558 -> 0.553 / 1.196 -> 1.187 / 1.825 -> 1.807 ms per step; 256 and 1024
  // pairs level, 512 pairs 5.79 -> 5.88 (the launches k_level_begin / k_finish stay there)
  const bool hand_over = b.policy.level_hand_over(n);
  if (level == b.level_from || !hand_over) {
    Range range(kRangePrep[level]);
    // (the slow lane's pairs begin their levels there)
    launch_level_begin(b.s, b.states, n, bp.prm, L.g, level, L.pp, b.d_levels, level == cfg->first_level ? b.w.t_init.as<double>() : nullptr,
                       lane.skip_flags(), 0);
  }
  std::memset(&L.next, 0, sizeof(L.next));
  if (hand_over && level > cfg->last_level) {
    const LevelGeom& gn = bp.geom[level - 1];
    L.next.valid = 1;
    L.next.level = level - 1;
    L.next.fx = gn.fx; L.next.fy = gn.fy; L.next.ox = gn.ox; L.next.oy = gn.oy;
    L.next.pairs = bp.pair_ptrs + size_t(level - 1) * n;
  } else if (hand_over) {
    L.next.results = b.w.results.as<dvo_hip_result>();         // the last level: a pair that has left it gets its result written
  }
  L.schedule = schedule_of(b, level);
  L.tail = ctx->opt_sweep_tail != 0 && L.schedule.fused_ll && sweep_has_tail(bp.choice[level], bp.rpw[level], L.g.rcp_table != nullptr, L.g.gram_hi_j != 0);   // (enqueue_step_in_sweep)
  L.pair_sums = L.tail && ctx->opt_sweep_tail == 2 ? b.w.pair_sums.as<double>() : nullptr;
  L.g_run = L.g;
  L.n_run = n;
  return L;
}

// One level of the chain: its steps go out until no pair is left on it, or the slow lane has taken the last ones.
int chain_level(BatchRun& b, SlowLane& lane, int level) {
  dvo_hip_context* ctx = b.ctx;
  const dvo_hip_config* cfg = b.cfg;
  const int n = b.n, per_sync = b.per_sync, per_level = b.per_level;
  lane.chain_enters(level);
  LevelRun L = begin_level(b, lane, level);
  const LevelGeom& g = L.g;
  const bool hand_over = b.policy.level_hand_over(n);
  // Chunks of `per_sync` iterations are enqueued ONE AHEAD of the poll: while the host waits for the status word of
  // chunk k, chunk k+1 is already queued, so the GPU never idles for a host round trip.  Iterations enqueued past the
  // end of the level are no-ops (workgroups exit on !active).
  int enqueued = std::min(per_sync, per_level);
  enqueue_chunk(b, L, enqueued);
  // (option "defer_ingest_pixels": not before the chain has reached a level of that many pixels -- the frame build is bound by memory, and
  // beside it the latency-bound sweeps and steps of the SMALL levels run 30-50 % longer (80 x 60: 52 -> 77 us, 160 x 120: 159 -> 212 us per
  // 1024-pair launch), the issue-bound sweeps of the large ones 2 %: a large batch's ingest belongs beside levels 1 and 0)
  const bool flush_here = ctx->opt_defer_ingest_pixels <= 0 || g.w * g.h >= ctx->opt_defer_ingest_pixels || level == cfg->last_level;
  if (!ctx->deferred.empty() && flush_here) {
    // A recorded ingest of the caller's next batch (option "defer_ingest") is carried out now, behind the first launches of this
    // batch.  It is ~0.1-0.5 ms of host time during which nothing more would be enqueued here: where the level's steps are short,
    // a few more of them go out first (a pair needs more than four passes on its first level; a step too many exits at once).
    // (how many: the ingest of 2 n frames is ~0.3 us of host time per frame, a step of a small level ~20 us -- measured, builds
    // alternated on one box: seven instead of three more 256 pairs 3.288 -> 3.216 ms per step, 128 pairs 1.837 -> 1.856, 64 pairs
    // 1.199 -> 1.210)
    if (size_t(g.tiles_x) * g.tiles_y * size_t(n) < 65536) {
      const int lead = std::min(b.policy.deferred_ingest_lead(n) * per_sync, per_level - enqueued);
      if (lead > 0) {
        enqueue_chunk(b, L, lead);
        enqueued += lead;
      }
    }
    const int rc_deferred = flush_recorded_ingest(b);
    if (rc_deferred != DVO_HIP_OK) return rc_deferred;
  }
  int watched = b.step - 1;                                  // last step of the chunk whose outcome is awaited
  // (the slow lane: every level but the last may shed its stragglers to it -- on the last one nothing follows that they could run beside)
  const bool list_tails = ctx->opt_tail_lists != 0 && !b.bp.ref_order && !L.tail && !hand_over && b.bp.choice[level].pair_list;
  const bool may_shed = lane.on() && level > cfg->last_level && !L.tail && b.bp.choice[level].pair_list;
  // Where an EMPTY step is expensive -- the dispatcher needs 95 us for the 307 200 workgroups of a 1024-pair finest-level sweep
  // that all exit at once, 114 us with its log-likelihood and solver launches -- the step ahead of the poll is not enqueued once
  // only a few pairs are left on the level: the host then waits for the outcome first (a bubble of ~15 us if another step is
  // needed).  Elsewhere the speculative step is cheaper than the bubble.
  const bool empty_step_is_costly = size_t(g.tiles_x) * g.tiles_y * size_t(n) >= (ctx->opt_tail_speculation >= 2 ? size_t(ctx->opt_tail_speculation) : kCostlyEmptyStepWorkgroups) && ctx->opt_tail_speculation != 1;
  int last_active = n;
  for (;;) {
    const bool hold = empty_step_is_costly && last_active * 8 <= n;
    int more = hold ? 0 : std::min(per_sync, per_level - enqueued);
    if (more > 0) {
      enqueue_chunk(b, L, more);
      enqueued += more;
    }
    int active = 0;
    int rc = lane.wait(watched, &active);
    if (rc != DVO_HIP_OK) return rc;
    last_active = active;
    if (may_shed && active > 0 && size_t(active) * size_t(ctx->opt_overlap_fraction) <= size_t(n)) {
      // the pairs still on the level (at most `active`: the steps enqueued ahead of this poll only take some away) go to the slow lane
      rc = lane.shed(level, active);
      if (rc != DVO_HIP_OK) return rc;
      break;
    }
    if (hold && active > 0) {                                // (the held-back step is needed after all)
      // ... by `active` pairs, none of whose steps is in flight: from here on the launches cover the list of them
      if (list_tails && !L.g_run.pair_list) {
        int* const own_list = b.w.chain_list.as<int>();
        launch_mark_stragglers(b.s, b.states, n, level, lane.skip_flags(), own_list, active, true);
        L.g_run.pair_list = own_list;
        L.n_run = active;
      }
      more = std::min(per_sync, per_level - enqueued);
      if (more > 0) {
        enqueue_chunk(b, L, more);
        enqueued += more;
      }
    }
    if (active == 0 || more <= 0) break;                     // every pair left this level (or the iteration cap is reached)
    watched = b.step - 1;
  }
  // The pairs that ended the level in the step just awaited are handed over (NextLevel) by the step that was enqueued ahead of the poll.
  // If there is none -- the step was held back, or the iteration cap is reached -- one solver launch does nothing else.
  if (hand_over && b.step - 1 <= watched) {
    Range range(kRangeLinsys[level]);
    launch_solver_step(b.s, b.states, n, b.bp.prm, g, b.partials, b.ll_partials, L.schedule.ll_blocks, nullptr, b.d_levels, b.d_iters, b.tallies + b.step, b.w.host_status + b.step,
                       L.schedule.two_waves, cfg->first_level - level, &L.next, b.ref_order);
    ++b.step;
  }
  return DVO_HIP_OK;
}

// ---- the way out -------------------------------------------------------------------------------------------------------------------------
// where the batch's records are on the host once the device is through, and when the host got there
struct CopyOut {
  std::vector<dvo_hip_level_stats> hl;
  std::vector<dvo_hip_iteration_stats> hi;
  const dvo_hip_level_stats* hl_src = nullptr;
  const dvo_hip_iteration_stats* hi_src = nullptr;
  std::chrono::steady_clock::time_point t_enqueued, t_done;
};

// The results into the caller's array, the statistics to where copy_statistics finds them: straight out of pinned memory (the resident
// kernel's direct path) or by copies on the stream behind the last launch; the batch is over on the device when this returns.
int copy_out(BatchRun& b, dvo_hip_result* results, bool want_levels, bool want_iters, CopyOut& out) {
  Workspace& w = b.w;
  const int n = b.n;
  if (b.rp.direct) {
    // the kernel writes results (and statistics) into pinned host memory and counts the pairs done: the host thread watches that
    // word -- no copy command, no stream synchronisation on the way out
    out.t_enqueued = std::chrono::steady_clock::now();
    const int rc = wait_for_direct(w, n);
    w.device_may_lag = true;
    if (rc != DVO_HIP_OK) return rc;
    out.t_done = std::chrono::steady_clock::now();
    if (w.host_status[w.resident_error_word] == 0) {
      std::memcpy(results, w.direct_results.p, size_t(n) * sizeof(dvo_hip_result));
      if (want_levels) out.hl_src = w.direct_levels.as<dvo_hip_level_stats>();
      if (want_iters) out.hi_src = w.direct_iters.as<dvo_hip_iteration_stats>();
    } else {
      DVO_WS_TRY(w, sync_stream(b.s));                         // every group has to be gone before the batch is repeated
    }
    return DVO_HIP_OK;
  }
  if (b.level_from >= b.cfg->last_level && b.policy.finish_launch(n)) launch_finish(b.s, b.states, n, b.bp.prm, b.d_levels, b.d_iters, w.results.as<dvo_hip_result>());
  // (else the results are in place: written by the resident launch, or by the solver steps behind the pairs' last level)
  DVO_WS_TRY(w, hipMemcpyAsync(results, w.results.p, size_t(n) * sizeof(dvo_hip_result), hipMemcpyDeviceToHost, b.s));
  if (want_levels) {
    out.hl.resize(size_t(n) * b.bp.cap_levels);
    DVO_WS_TRY(w, hipMemcpyAsync(out.hl.data(), b.d_levels, out.hl.size() * sizeof(dvo_hip_level_stats), hipMemcpyDeviceToHost, b.s));
    out.hl_src = out.hl.data();
  }
  if (want_iters) {
    out.hi.resize(size_t(n) * b.bp.cap_iters);
    DVO_WS_TRY(w, hipMemcpyAsync(out.hi.data(), b.d_iters, out.hi.size() * sizeof(dvo_hip_iteration_stats), hipMemcpyDeviceToHost, b.s));
    out.hi_src = out.hi.data();
  }
  out.t_enqueued = std::chrono::steady_clock::now();
  DVO_WS_TRY(w, sync_stream(b.s));
  DVO_WS_TRY(w, hipGetLastError());
  out.t_done = std::chrono::steady_clock::now();
  return DVO_HIP_OK;
}

// every pair's statistics into the caller's arrays, as far as those reach; true: some did not fit
bool copy_statistics(const BatchRun& b, const CopyOut& out, const dvo_hip_result* results, dvo_hip_level_stats* levels, int cap_levels,
                     dvo_hip_iteration_stats* iters, int cap_iters) {
  bool truncated = false;
  for (int i = 0; i < b.n; ++i) {
    if (out.hl_src) {
      const int nl = std::min(results[i].n_levels, std::min(cap_levels, b.bp.cap_levels));
      std::memcpy(levels + size_t(i) * cap_levels, out.hl_src + size_t(i) * b.bp.cap_levels, size_t(nl) * sizeof(dvo_hip_level_stats));
      truncated |= results[i].n_levels > cap_levels;
    }
    if (out.hi_src) {
      const int ni = std::min(results[i].n_iterations_total, std::min(cap_iters, b.bp.cap_iters));
      std::memcpy(iters + size_t(i) * cap_iters, out.hi_src + size_t(i) * b.bp.cap_iters, size_t(ni) * sizeof(dvo_hip_iteration_stats));
      truncated |= results[i].n_iterations_total > cap_iters;
    }
  }
  return truncated;
}

int run_batch(dvo_hip_context* ctx, int n, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, const dvo_hip_config* cfg,
              dvo_hip_result* results, dvo_hip_level_stats* levels, int cap_levels, dvo_hip_iteration_stats* iters, int cap_iters);

// What the three repeats of a batch share: `m` pairs of it (pair k is the batch's pair which[k]; null: all of them, in place) get their
// initial guesses back, the roles are ensured again (another path or sweep may read another flavour of the current planes), and the
// pairs run as a batch.  What makes the second run another one -- an option, the Gram schedule -- the caller has set.
int run_again(const BatchRun& b, int m, const int* which, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, dvo_hip_result* results,
              dvo_hip_level_stats* levels, int cap_levels, dvo_hip_iteration_stats* iters, int cap_iters) {
  for (int k = 0; k < m; ++k) std::memcpy(results[k].transformation, &b.tinit[size_t(which ? which[k] : k) * 16], 16 * sizeof(double));
  int rc = ensure_batch_roles(b.ctx, m, refs, curs, b.cfg);
  if (rc == DVO_HIP_OK) rc = run_batch(b.ctx, m, refs, curs, b.cfg, results, levels, cap_levels, iters, cap_iters);
  return rc;
}

// the pairs whose word in the f16 range array a sweep has raised; the words are cleared
std::vector<int> take_out_of_range(const BatchRun& b) {
  std::vector<int> out_of_range;
  if (b.ctx->opt_variant >= 7)
    for (int i = 0; i < b.n; ++i)
      if (static_cast<volatile int*>(b.w.f16_range_flag)[i] != 0) {
        static_cast<volatile int*>(b.w.f16_range_flag)[i] = 0;
        out_of_range.push_back(i);
      }
  return out_of_range;
}

// the flagged pairs again, f32 Gram, as a batch of their own; their records replace the ones just copied out.  DVO_HIP_ERR_CAPACITY:
// their statistics did not fit either (the results are valid).
int repeat_out_of_range(const BatchRun& b, const std::vector<int>& out_of_range, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs,
                        dvo_hip_result* results, dvo_hip_level_stats* levels, int cap_levels, dvo_hip_iteration_stats* iters, int cap_iters) {
  dvo_hip_context* ctx = b.ctx;
  const int m = int(out_of_range.size());
  ctx->f16_range_repeats += m;
  std::vector<dvo_hip_frame*> r2(m), c2(m);
  std::vector<dvo_hip_result> res2(m);
  for (int k = 0; k < m; ++k) {
    const int i = out_of_range[k];
    r2[k] = refs[i];
    c2[k] = curs[i];
    res2[k] = results[i];
  }
  const bool want_l = levels && cap_levels > 0, want_i = iters && cap_iters > 0;
  std::vector<dvo_hip_level_stats> l2(want_l ? size_t(m) * cap_levels : 0);
  std::vector<dvo_hip_iteration_stats> i2(want_i ? size_t(m) * cap_iters : 0);
  ctx->opt_variant = 6;                                        // (restored by run_batch's variant_scope)
  const int rc = run_again(b, m, out_of_range.data(), r2.data(), c2.data(), res2.data(), want_l ? l2.data() : nullptr, cap_levels, want_i ? i2.data() : nullptr, cap_iters);
  if (rc != DVO_HIP_OK && rc != DVO_HIP_ERR_CAPACITY) return rc;
  for (int k = 0; k < m; ++k) {
    const int i = out_of_range[k];
    results[i] = res2[k];
    if (want_l) std::memcpy(levels + size_t(i) * cap_levels, l2.data() + size_t(k) * cap_levels, size_t(cap_levels) * sizeof(dvo_hip_level_stats));
    if (want_i) std::memcpy(iters + size_t(i) * cap_iters, i2.data() + size_t(k) * cap_iters, size_t(cap_iters) * sizeof(dvo_hip_iteration_stats));
  }
  return rc;
}

// The coarse-to-fine Gauss-Newton driver of a batch (dense_tracking.cpp:131-376 for every pair at once).
int run_batch(dvo_hip_context* ctx, int n, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, const dvo_hip_config* cfg,
              dvo_hip_result* results, dvo_hip_level_stats* levels, int cap_levels, dvo_hip_iteration_stats* iters, int cap_iters) {
  // (the Gram schedule of the batch -- f16 high + low operand pairs or f32 -- was decided by the caller, effective_variant_scope; what
  // this function changes for a repeat is undone when it returns)
  struct VariantScope {
    dvo_hip_context* c; int keep;
    ~VariantScope() { c->opt_variant = keep; }
  } variant_scope{ctx, ctx->opt_variant};
  BatchRun b(ctx, cfg, n);
  Workspace& w = b.w;
  SlowLane lane(b);
  int rc = prepare_batch(b, lane, refs, curs, results);
  if (rc != DVO_HIP_OK) return rc;
  const auto t_launch = std::chrono::steady_clock::now();
  const bool want_levels = levels && cap_levels > 0, want_iters = iters && cap_iters > 0;
  ResidentBudget::Hold compute_units;                          // released when this batch is through with the device
  if (b.rp.levels > 0 && b.rp.group > 1)
    compute_units.take(ResidentBudget::of(ctx->device), n * b.rp.group, ctx->compute_units > 0 ? ctx->compute_units : 256);
  rc = run_prefixes(b, want_levels || want_iters);
  if (rc != DVO_HIP_OK) return rc;
  lane.begin(b.level_from);
  for (int level = b.level_from; level >= cfg->last_level; --level) {
    rc = chain_level(b, lane, level);
    if (rc != DVO_HIP_OK) return rc;
  }
  rc = lane.drain();
  if (rc != DVO_HIP_OK) return rc;
  CopyOut out;
  rc = copy_out(b, results, want_levels, want_iters, out);
  if (rc != DVO_HIP_OK) return rc;
  if (b.rp.levels > 0 && w.host_status[w.resident_error_word] != 0) {
    // A group of the resident kernel gave up waiting for its peers: its workgroups were not all on the device at once (the
    // device is shared with another process that does the same, or a compute-unit mask shrank it).  Nothing is wrong with the
    // batch: it runs again, one launch per step, and the context stops using groups.
    w.resident_sequence = 0xffffffffu;                       // the exchange rows are in an unknown state: cleared before the next use
    ctx->resident_timeouts += 1;
    // (not after a single incident: a launch that started late once -- the device busy with another process for a moment -- is no
    // reason to give up the latency path for the rest of the context's life)
    if (ctx->resident_timeouts >= 3) ctx->opt_resident_group = 1;
    const int keep = ctx->opt_resident;
    ctx->opt_resident = 0;
    w.needs_drain = true;
    rc = run_again(b, n, nullptr, refs, curs, results, levels, cap_levels, iters, cap_iters);   // (the launch path may read another flavour of the current planes)
    ctx->opt_resident = keep;
    return rc;
  }
  // Pairs in which a Jacobian component of some pixel was beyond +-65504: the f16 high / low split of the Gram operands (variants 7-9)
  // does not represent it, the sweep's epilogue has raised the pair's word.  Those pairs run again with the f32 Gram of the same sweep
  // family (variant 6): the whole batch when most of it is concerned (one chain of launches either way; the batches that follow then
  // start on the f32 Gram, kF32GramHoldBatches), otherwise ONLY the flagged pairs, as a batch of their own, behind the copy-out below
  // (round 5: a single close depth step used to repeat all 1024 pairs of a batch).
  const std::vector<int> out_of_range = take_out_of_range(b);
  // (the repeats below prepare role planes and run another batch: two groups of one batch -- dvo_hip_match_batch -- do not do that at once)
  std::unique_lock<std::mutex> rare_path;
  if (!out_of_range.empty()) rare_path = std::unique_lock<std::mutex>(g_rare_path_mutex);
  if (!out_of_range.empty() && out_of_range.size() * 2 >= size_t(n)) {
    ctx->f16_range_repeats += (long long)out_of_range.size();
    ctx->f32_gram_hold = kF32GramHoldBatches;
    ctx->opt_variant = 6;                                      // (restored by variant_scope)
    return run_again(b, n, nullptr, refs, curs, results, levels, cap_levels, iters, cap_iters);   // (another sweep, maybe another flavour of the current planes)
  }
  bool truncated = copy_statistics(b, out, results, levels, cap_levels, iters, cap_iters);
  {
    using std::chrono::duration_cast;
    using std::chrono::nanoseconds;
    ctx->host_ns[0] += duration_cast<nanoseconds>(t_launch - ctx->batch_entry).count();
    ctx->host_ns[1] += duration_cast<nanoseconds>(out.t_enqueued - t_launch).count();
    ctx->host_ns[2] += duration_cast<nanoseconds>(out.t_done - out.t_enqueued).count();
    ctx->host_ns[3] += duration_cast<nanoseconds>(std::chrono::steady_clock::now() - out.t_done).count();
    ctx->host_batches += 1;
  }
  w.needs_drain = false;
  if (!out_of_range.empty()) {
    rc = repeat_out_of_range(b, out_of_range, refs, curs, results, levels, cap_levels, iters, cap_iters);
    if (rc != DVO_HIP_OK && rc != DVO_HIP_ERR_CAPACITY) return rc;
    truncated |= rc == DVO_HIP_ERR_CAPACITY;
  }
  if (truncated) {
    w.err = "match: statistics arrays too small (results are valid)";
    return DVO_HIP_ERR_CAPACITY;
  }
  return DVO_HIP_OK;
}
