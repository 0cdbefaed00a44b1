// capi_lane.inc -- the slow lane of a batch (round 6, option "overlap_tails").  Textually included by capi_schedule.inc between what the lane
// shares with the batch's chain (BatchRun, schedule_of, the waits on the status words) and the chain itself; what the lane keeps from one
// batch to the next is LaneResources (capi.hip, a member of the workspace).
//
// The pairs of a batch need different numbers of passes on a level, and the launch chain runs a level until its LAST pair has left it: on
// the bench's 1024-pair batches 11 of a step's 32 iterations are such tail launches, a few dozen pairs each, while the chip waits (1.1 ms
// of 11).  In the reference every match() runs on its own from start to end (dense_tracking.cpp:200-357).  Here, once at most 1/8 of
// the pairs is still on a level, those pairs leave the batch's chain for good: they get a flag byte and a place in a list
// (k_mark_stragglers), the chain goes on to the next level without them (LevelGeom::skip_flags), and a SLOW LANE -- a second stream, its
// own partial rows and residual pairs, its own status words -- runs them to the end of the match with launches over the list
// (LevelGeom::pair_list): the rest of that level, then level after level behind the main chain, taking up the stragglers the chain
// sheds on the way.  The lane works on one level at a time and never gets ahead of the chain: it leaves a level when none of its members is
// active on it AND the chain has left it (so nobody can still arrive there).  The batch ends when both have.  A pair's arithmetic does
// not know in which launch it runs: the records are the synchronous chain's bit for bit (tests/test_gpu_overlap.py).
//
// The lane of ONE batch.  The chain (run_batch, chain_level) calls the public members and nothing else of it: on(), reserve(), begin(),
// chain_enters(), skip_flags(), shed(), wait(), drain().
class SlowLane {
 public:
  explicit SlowLane(BatchRun& run) : b(run), r(run.w.lane) {}

  bool on() const { return on_; }
  size_t steps_cap() const { return steps_cap_; }              // status words and tallies of the lane: they lie behind the chain's

  // Decides whether the batch gets a lane and, if so, reserves what it needs.  Batches whose levels are begun by launches (beyond the solver
  // steps' hand-over), the plain launch chain (no step in the sweep's tail), more than one level on this path.
  int reserve() {
    dvo_hip_context* ctx = b.ctx;
    const dvo_hip_config* cfg = b.cfg;
    const BatchPlan& bp = b.bp;
    const int n = b.n;
    on_ = ctx->opt_overlap_tails != 0 && !ctx->opt_ref_order && !b.policy.level_hand_over(n) && ctx->opt_sweep_tail == 0 && b.rp.levels == 0 && bp.coarse_levels == 0 &&
          cfg->first_level > cfg->last_level;
    for (int l = cfg->last_level; l <= cfg->first_level; ++l)   // (the lane passes through every level: each one's sweep must take a list of pairs)
      on_ = on_ && bp.choice[l].pair_list;
    steps_cap_ = on_ ? size_t(bp.cap_iters) + 12 * size_t(bp.nlev) + 8 : 0;   // (per level: the passes of its slowest pair, and up to eight steps enqueued ahead of what is known)
    if (!on_) return DVO_HIP_OK;
    size_t t_tiles = 1, t_entries = 0;
    for (int l = cfg->last_level; l <= cfg->first_level; ++l) {
      t_tiles = std::max(t_tiles, size_t(bp.geom[l].tiles_x) * bp.geom[l].tiles_y);
      t_entries = std::max(t_entries, residual_entries(bp.geom[l]));
    }
    DVO_WS_TRY(b.w, r.partials.reserve(size_t(n) * t_tiles * kAccStride * sizeof(float)));
    DVO_WS_TRY(b.w, r.scratch.reserve(size_t(n) * t_entries * sizeof(float2)));
    DVO_WS_TRY(b.w, r.flags.reserve(align_up(size_t(n), 256)));
    DVO_WS_TRY(b.w, r.ll.reserve(size_t(n) * kLlBlocksPerPair * sizeof(double)));
    DVO_WS_TRY(b.w, r.lists.reserve(2 * list_stride() * sizeof(int)));   // (the list in use and the one being made)
    DVO_WS_TRY(b.w, b.w.counters.reserve((b.main_steps + steps_cap_) * sizeof(unsigned long long) + align_up(size_t(n) * sizeof(int), 8)));
    if (!r.stream) {
      int prio_least = 0, prio_greatest = 0;
      DVO_WS_TRY(b.w, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
      DVO_WS_TRY(b.w, hipStreamCreateWithPriority(&r.stream, hipStreamNonBlocking, prio_greatest));
      DVO_WS_TRY(b.w, hipEventCreateWithFlags(&r.split, hipEventDisableTiming));
      for (hipEvent_t& e : r.end) DVO_WS_TRY(b.w, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return DVO_HIP_OK;
  }

  // in front of the chain's first level
  void begin(int level_from) {
    main_level = level_from;
    if (on_) launch_clear_flags(b.s, flags(), b.n);
  }
  void chain_enters(int level) { main_level = level; }
  // what the chain's launches must skip (the lane's pairs are not the chain's any more); null: nothing
  unsigned char* skip_flags() const { return live ? flags() : nullptr; }

  // the chain sheds the pairs still active on `level` (at most `active` of them) to the lane
  int shed(int level, int active) {
    Range range("shed");
    const int next_sel = live ? list_sel ^ 1 : 0;
    const int new_cap = std::min(b.n, cap + active);
    // The list written now is the one the lane left at the previous shed.  The launches that read it are on the lane's stream, which nothing
    // orders against the chain's: the chain's stream waits, on the device, for the last of them (r.end of that list, recorded behind every
    // run of launches that were given it) before k_mark_stragglers writes.  A batch's first two sheds write a list each that nobody has read.
    if (sheds >= 2) DVO_WS_TRY(b.w, hipStreamWaitEvent(b.s, r.end[next_sel], 0));
    launch_mark_stragglers(b.s, b.states, b.n, level, flags(), list(next_sel), new_cap);
    DVO_WS_TRY(b.w, hipEventRecord(r.split, b.s));
    DVO_WS_TRY(b.w, hipStreamWaitEvent(r.stream, r.split, 0));
    cap = new_cap;
    list_sel = next_sel;
    sheds += 1;
    if (!live) {
      live = true;
      this->level = level;
    }
    valid_from = next;                                         // (whatever level the lane is on: its launches read the new list from here on)
    last_active = -1;
    enqueue(3);
    b.ctx->overlapped_tails += 1;
    return DVO_HIP_OK;
  }

  // the chain's wait for a step, looking after the lane meanwhile
  int wait(int idx, int* active) {
    if (!live || done) return wait_for_step(b.w, idx, active);
    volatile int* word = b.w.host_status + idx;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
      const int v = *word;
      if (v & kStepDoneFlag) {
        *active = v & ~kStepDoneFlag;
        service();
        return DVO_HIP_OK;
      }
      if ((spins & 0x3f) == 0) service();
      if ((spins & 0xfffff) == 0) {
        const int rc_check = step_wait_check(b.w, t0);
        if (rc_check != DVO_HIP_OK) return rc_check;
      }
    }
  }

  // the chain is through; the slow lane runs its pairs to the end of the match (from here on it may leave any level)
  int drain() {
    if (!live) return DVO_HIP_OK;
    main_level = b.cfg->last_level - 1;
    const auto t_wait = std::chrono::steady_clock::now();
    service();
    while (!done) {
      if (next == 0 || size_t(next) >= steps_cap_) {
        b.w.err = "match: the slow lane of the batch ran out of steps";
        return DVO_HIP_ERR_HIP;
      }
      int unused = 0;
      const int rc = wait_for_step(b.w, int(b.main_steps) + next - 1, &unused);
      if (rc != DVO_HIP_OK) return rc;
      service();
    }
    b.ctx->tail_drains += 1;
    b.ctx->tail_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_wait).count();
    DVO_WS_TRY(b.w, hipStreamWaitEvent(b.s, r.end[list_sel], 0));   // (k_finish and the copies of the results follow the lane's last step)
    return DVO_HIP_OK;
  }

 private:
  BatchRun& b;
  LaneResources& r;
  bool on_ = false;
  size_t steps_cap_ = 0;
  bool live = false, done = false;
  int level = -1;                    // the level its launches work on
  int cap = 0;                       // entries of the current list: an upper bound of the flagged pairs
  int list_sel = 0;                  // which of the two list buffers is the current one (the other may still be read by launches in flight)
  int sheds = 0;                     // sheds of this batch so far: from the third on a shed writes a list that launches have read
  int seen = 0;                      // status words of the lane read so far (they complete in order: one stream)
  int valid_from = 0;                // steps before this one say nothing about the lane's level as it is now (another level, or members have arrived since)
  int last_active = -1;
  int next = 0;                      // steps of the lane enqueued in this batch (index of its next status word, behind the chain's)
  int main_level = 0;                // the level the batch's own chain works on (below last_level: through)

  unsigned char* flags() const { return r.flags.as<unsigned char>(); }
  size_t list_stride() const { return align_up(size_t(b.n), 64); }
  int* list(int sel) const { return r.lists.as<int>() + size_t(sel) * list_stride(); }

  // `count` more steps of the lane's level over its current list (as far as its status words reach)
  void enqueue(int count) {
    dvo_hip_context* ctx = b.ctx;
    const BatchPlan& bp = b.bp;
    const LevelSchedule ls = schedule_of(b, level);
    LevelGeom g = bp.geom[level];
    g.pair_list = list(list_sel);
    const PairPtrs* pp = bp.pair_ptrs + size_t(level) * b.n;
    float* lp = r.partials.as<float>();
    float2* lscr = r.scratch.as<float2>();
    double* lll = r.ll.as<double>();
    for (int c = 0; c < count && size_t(next) < steps_cap_; ++c, ++next) {
      const size_t idx = b.main_steps + size_t(next);
      launch_residual_reduce(r.stream, bp.choice[level], bp.rpw[level], level == 0, g, pp, b.states, cap, lp, lscr, b.w.win_fallbacks.as<unsigned long long>(),
                             b.w.f16_range_flag);
      if (!ls.fused_ll) launch_loglik(r.stream, g, b.states, cap, lp, lscr, lll, ls.ll_blocks, ctx->opt_deterministic != 0);
      launch_solver_step(r.stream, b.states, cap, bp.prm, g, lp, lll, ls.ll_blocks, ls.fused_ll ? lscr : nullptr, b.d_levels, b.d_iters,
                         b.tallies + idx, b.w.host_status + idx, false, b.cfg->first_level - level, nullptr);
      ctx->overlapped_steps += 1;
    }
    (void)hipEventRecord(r.end[list_sel], r.stream);           // (the batch's end waits for the latest record: everything enqueued so far)
  }

  // what the lane's status words say by now, and what follows from it (never waits)
  void service() {
    if (!live || done) return;
    while (seen < next) {
      const int v = static_cast<volatile int*>(b.w.host_status)[b.main_steps + size_t(seen)];
      if (!(v & kStepDoneFlag)) break;
      if (seen >= valid_from) last_active = v & ~kStepDoneFlag;
      seen += 1;
    }
    if (seen > valid_from && last_active == 0) {               // nobody of the lane is active on its level
      if (level <= main_level) return;                         // (the chain is still on it: its stragglers may yet arrive)
      if (level == b.cfg->last_level) {
        done = true;
        return;
      }
      // on to the next level: the members that have left this one begin it (those that arrived further down are on theirs already)
      const int lv = level - 1;
      launch_level_begin(r.stream, b.states, b.n, b.bp.prm, b.bp.geom[lv], lv, b.bp.pair_ptrs + size_t(lv) * b.n, b.d_levels, nullptr, flags(), 1, level);
      level = lv;
      valid_from = next;
      last_active = -1;
      enqueue(3);
      return;
    }
    if (next - seen < 2) enqueue(2);
  }
};
