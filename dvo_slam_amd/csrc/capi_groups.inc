// capi_groups.inc -- concurrent pair groups: a batch aligned as several sub-batches at once, the caller's thread on its context, helper
// threads on twin contexts of the same device (option "batch_groups").  Textually included by capi.hip inside its anonymous namespace,
// behind run_batch.
// ---- concurrent pair groups (dvo_hip_context::opt_batch_groups) -----------------------------------------------------------------------
// the options a group's twin context aligns with: the owner's, as they are in effect for this batch
void mirror_options(const dvo_hip_context* from, dvo_hip_context* to) {
#define DVO_MIRROR(f) to->f = from->f
  DVO_MIRROR(opt_rows_per_wave); DVO_MIRROR(opt_iters_per_sync); DVO_MIRROR(opt_tail_speculation); DVO_MIRROR(opt_solver_waves);
  DVO_MIRROR(opt_ll_blocks); DVO_MIRROR(opt_compact_residuals); DVO_MIRROR(opt_gram_lo_parts); DVO_MIRROR(opt_min_workgroups);
  DVO_MIRROR(opt_condition_number); DVO_MIRROR(opt_fused_ll_pixels); DVO_MIRROR(opt_variant); DVO_MIRROR(opt_resident);
  DVO_MIRROR(opt_resident_rows); DVO_MIRROR(opt_resident_group); DVO_MIRROR(opt_resident_flags); DVO_MIRROR(opt_resident_cooperative);
  DVO_MIRROR(opt_sweep_tail); DVO_MIRROR(opt_coarse); DVO_MIRROR(opt_coarse_pixels); DVO_MIRROR(opt_coarse_wgs);
  DVO_MIRROR(opt_deterministic); DVO_MIRROR(opt_ref_order); DVO_MIRROR(opt_small_sweep); DVO_MIRROR(opt_small_tiles); DVO_MIRROR(compute_units);
  DVO_MIRROR(opt_overlap_tails); DVO_MIRROR(opt_overlap_fraction); DVO_MIRROR(opt_tail_lists); DVO_MIRROR(opt_defer_ingest_pixels);
#undef DVO_MIRROR
}

void group_worker_main(GroupWorker* gw) {
  (void)hipSetDevice(gw->twin->device);
  for (;;) {
    std::unique_lock<std::mutex> lock(gw->m);
    gw->cv.wait(lock, [&] { return gw->has_job || gw->quit; });
    if (gw->quit) return;
    gw->has_job = false;
    lock.unlock();
    dvo_hip_context* t = gw->twin;
    t->batch_entry = std::chrono::steady_clock::now();
    int rc = DVO_HIP_OK;
    if (hipStreamWaitEvent(t->stream, gw->after, 0) != hipSuccess) {
      t->err = "match: a pair group could not wait for the batch's role planes";
      rc = DVO_HIP_ERR_HIP;
    }
    if (rc == DVO_HIP_OK) {
      rc = run_batch(t, gw->n, gw->refs, gw->curs, gw->cfg, gw->results, gw->levels, gw->cap_levels, gw->iters, gw->cap_iters);
      if (rc != DVO_HIP_OK) t->err = t->ws[0].err;
    }
    lock.lock();
    gw->rc = rc;
    gw->done = true;
    lock.unlock();
    gw->cv.notify_all();
  }
}

// how many groups a batch of n pairs is aligned in
int batch_groups_of(const dvo_hip_context* ctx, int n) {
  if (ctx->is_twin || ctx->opt_ref_compat || ctx->opt_deterministic || ctx->opt_ref_order) return 1;   // (the reciprocal table lives in the owner; one schedule per pair)
  // Asked for by name only.  Measured (round 6, streaming loop, one box): 1024 pairs 11.75 -> 11.1-11.9 ms per step with two groups,
  // 11.4-12.0 with three -- groups that start together stay in phase, and two sweeps of the same level side by side gain nothing; the
  // gain of several contexts on one GPU comes from running OUT of phase, which a streaming caller gets from lanes
  // (dvo_slam_amd/apps/stream_pipeline.cpp, dvo_stream_lanes_*: 11.3 -> 10.8).
  return ctx->opt_batch_groups > 1 ? std::min(ctx->opt_batch_groups, std::max(1, n / 64)) : 1;
}

int ensure_group_workers(dvo_hip_context* ctx, int groups) {
  while (int(ctx->group_workers.size()) < groups - 1) {
    dvo_hip_context* twin = nullptr;
    const int rc = dvo_hip_context_create(ctx->device, &twin);
    if (rc != DVO_HIP_OK) return fail(ctx, rc, "match: could not create a pair group's context");
    twin->is_twin = true;
    GroupWorker* gw = new GroupWorker();
    gw->twin = twin;
    gw->thread = std::thread(group_worker_main, gw);
    ctx->group_workers.push_back(gw);
  }
  if (!ctx->roles_ready) DVO_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->roles_ready, hipEventDisableTiming));
  return DVO_HIP_OK;
}

void destroy_group_workers(dvo_hip_context* ctx) {
  for (GroupWorker* gw : ctx->group_workers) {
    {
      std::lock_guard<std::mutex> lock(gw->m);
      gw->quit = true;
    }
    gw->cv.notify_all();
    if (gw->thread.joinable()) gw->thread.join();
    dvo_hip_context_destroy(gw->twin);
    delete gw;
  }
  ctx->group_workers.clear();
  if (ctx->roles_ready) (void)hipEventDestroy(ctx->roles_ready);
  ctx->roles_ready = nullptr;
}

// the batch as `groups` sub-batches at once: pairs [0, n_0) on the caller's thread and context, the other slices on the helpers
int run_batch_grouped(dvo_hip_context* ctx, int groups, int n, dvo_hip_frame* const* refs, dvo_hip_frame* const* curs, const dvo_hip_config* cfg,
                      dvo_hip_result* results, dvo_hip_level_stats* levels, int cap_levels, dvo_hip_iteration_stats* iters, int cap_iters) {
  int rc = ensure_group_workers(ctx, groups);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, hipEventRecord(ctx->roles_ready, ctx->stream));
  const int base = n / groups, extra = n % groups;             // slice g: base pairs, the first `extra` slices one more
  const int n0 = base + (extra > 0 ? 1 : 0);
  int at = n0;
  for (int g = 1; g < groups; ++g) {
    GroupWorker* gw = ctx->group_workers[g - 1];
    const int m = base + (g < extra ? 1 : 0);
    mirror_options(ctx, gw->twin);
    {
      std::lock_guard<std::mutex> lock(gw->m);
      gw->n = m;
      gw->refs = refs + at; gw->curs = curs + at; gw->cfg = cfg; gw->results = results + at;
      gw->levels = levels && cap_levels > 0 ? levels + size_t(at) * cap_levels : nullptr;
      gw->iters = iters && cap_iters > 0 ? iters + size_t(at) * cap_iters : nullptr;
      gw->cap_levels = cap_levels; gw->cap_iters = cap_iters;
      gw->after = ctx->roles_ready;
      gw->done = false;
      gw->has_job = true;
    }
    gw->cv.notify_all();
    at += m;
  }
  ctx->grouped_batches += 1;
  rc = run_batch(ctx, n0, refs, curs, cfg, results, levels, cap_levels, iters, cap_iters);
  if (rc != DVO_HIP_OK) ctx->err = ctx->ws[0].err;
  for (int g = 1; g < groups; ++g) {                          // every helper is awaited whatever the outcome: its slice of the caller's arrays is in use
    GroupWorker* gw = ctx->group_workers[g - 1];
    std::unique_lock<std::mutex> lock(gw->m);
    gw->cv.wait(lock, [&] { return gw->done; });
    if (gw->rc != DVO_HIP_OK && (rc == DVO_HIP_OK || rc == DVO_HIP_ERR_CAPACITY)) {
      rc = gw->rc;
      ctx->err = gw->twin->err;
    }
    ctx->f16_range_repeats += gw->twin->f16_range_repeats;
    gw->twin->f16_range_repeats = 0;
  }
  return rc;
}

