// capi_options.inc -- dvo_hip_get_counter / dvo_hip_set_option: the string-keyed options and counters of a context (documented in
// include/dvo_hip.h; tests/test_capi.py checks that every key parsed here is).  Textually included by capi.hip inside its extern "C" block.
int dvo_hip_get_counter(dvo_hip_context* ctx, const char* key, long long* value) {
  if (!ctx || !key || !value) return DVO_HIP_ERR_INVALID;
  std::unique_lock<std::recursive_mutex> guard(ctx->mutex);
  if (std::strcmp(key, "resident_launches") == 0) *value = ctx->resident_launches;
  else if (std::strcmp(key, "resident_levels") == 0) *value = ctx->resident_levels;
  else if (std::strcmp(key, "resident_timeouts") == 0) *value = ctx->resident_timeouts;
  else if (std::strcmp(key, "grouped_batches") == 0) *value = ctx->grouped_batches;
  // (what the batch-size policy says for this context's device, for callers that stream: batch_policy.h)
  else if (std::strcmp(key, "compute_units") == 0) *value = BatchPolicy(ctx->compute_units).cus;
  else if (std::strcmp(key, "defer_ingest_max_pairs") == 0) *value = BatchPolicy(ctx->compute_units).defer_ingest_max_pairs();
  else if (std::strcmp(key, "background_build_workgroups") == 0) *value = BatchPolicy(ctx->compute_units).background_build_workgroups();
  else if (std::strcmp(key, "tail_steps") == 0) {
    *value = ctx->tail_steps;
    for (const GroupWorker* gw : ctx->group_workers) *value += gw->twin->tail_steps;
  }
  else if (std::strcmp(key, "overlapped_tails") == 0) *value = ctx->overlapped_tails;
  else if (std::strcmp(key, "overlapped_steps") == 0) *value = ctx->overlapped_steps;
  else if (std::strcmp(key, "listed_steps") == 0) *value = ctx->listed_steps;
  else if (std::strcmp(key, "tail_drains") == 0) *value = ctx->tail_drains;
  else if (std::strcmp(key, "tail_wait_us") == 0) *value = ctx->tail_wait_ns / 1000;
  else if (std::strcmp(key, "ref_order_passes") == 0) *value = ctx->ref_order_passes;
  else if (std::strcmp(key, "coarse_launches") == 0) *value = ctx->coarse_launches;
  else if (std::strcmp(key, "coarse_levels") == 0) *value = ctx->coarse_levels;
  else if (std::strcmp(key, "window_fallbacks") == 0) {
    unsigned long long v = 0;
    if (ctx->ws[0].win_fallbacks.p) {
      DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      DVO_HIP_TRY(ctx, hipMemcpy(&v, ctx->ws[0].win_fallbacks.p, sizeof(v), hipMemcpyDeviceToHost));
    }
    *value = (long long)v;
  }
  else if (std::strcmp(key, "strip_ingests") == 0) *value = ctx->strip_ingests;
  else if (std::strcmp(key, "colour_ingests") == 0) *value = ctx->colour_ingests;
  else if (std::strcmp(key, "sensor_ingests") == 0) *value = ctx->sensor_ingests;
  else if (std::strcmp(key, "f32_ingests") == 0) *value = ctx->f32_ingests;
  else if (std::strcmp(key, "lens_ingests") == 0) *value = ctx->lens_ingests;
  // (frames whose depth plane went through a depth rig, rig_stage; and the bytes of the pass's pointer table: 0 until the first one)
  else if (std::strcmp(key, "depth_registrations") == 0) *value = ctx->depth_registrations;
  // (frames whose depth plane went through a depth filter, filter_stage)
  else if (std::strcmp(key, "depth_filter_ingests") == 0) *value = ctx->depth_filter_ingests;
  else if (std::strcmp(key, "depth_rig_table_bytes") == 0) *value = (long long)ctx->rig_tbl.bytes;
  // (the keyframe map, capi_map.inc: frames inserted, points the maps took, points they dropped)
  else if (std::strcmp(key, "map_inserts") == 0) *value = ctx->map_inserts;
  else if (std::strcmp(key, "map_removes") == 0) *value = ctx->map_removes;
  else if (std::strcmp(key, "map_rehashes") == 0) *value = ctx->map_rehashes;
  else if (std::strcmp(key, "map_renders") == 0) *value = ctx->map_renders;
  else if (std::strcmp(key, "frame_warps") == 0) *value = ctx->frame_warps;
  else if (std::strcmp(key, "covisibility_pairs") == 0) *value = ctx->covisibility_pairs;
  else if (std::strcmp(key, "codebook_encoded") == 0) *value = ctx->codebook_encoded;
  else if (std::strcmp(key, "codebook_queries") == 0) *value = ctx->codebook_queries;
  else if (std::strcmp(key, "map_points") == 0) *value = ctx->map_points;
  else if (std::strcmp(key, "map_dropped") == 0) *value = ctx->map_dropped;
  else if (std::strcmp(key, "graph_resident_solves") == 0) *value = ctx->graph_resident_solves;
  else if (std::strcmp(key, "warmup_wait_us") == 0) *value = ctx->warmup_wait_us;
  else if (std::strcmp(key, "rendezvous_pairs") == 0) {
    std::lock_guard<std::mutex> lock(ctx->rendezvous_mutex);
    *value = ctx->rendezvous_pairs;
  }
  else if (std::strcmp(key, "f16_range_repeats") == 0) *value = ctx->f16_range_repeats;
  else if (std::strcmp(key, "table_uploads_skipped") == 0) *value = ctx->tables.skipped;
  else if (std::strcmp(key, "deferred_ingests") == 0) *value = ctx->deferred_ingests;
  else if (std::strcmp(key, "host_batches") == 0) *value = ctx->host_batches;
  else if (std::strcmp(key, "host_ns_prepare") == 0) *value = ctx->host_ns[0];
  else if (std::strcmp(key, "host_ns_enqueue") == 0) *value = ctx->host_ns[1];
  else if (std::strcmp(key, "host_ns_wait") == 0) *value = ctx->host_ns[2];
  else if (std::strcmp(key, "host_ns_finish") == 0) *value = ctx->host_ns[3];
  else return fail(ctx, DVO_HIP_ERR_INVALID, "unknown counter");
  return DVO_HIP_OK;
}

int dvo_hip_set_option(dvo_hip_context* ctx, const char* key, int value) {
  DVO_LOCK(ctx);
  if (!ctx || !key) return DVO_HIP_ERR_INVALID;
  if (std::strcmp(key, "rows_per_wave") == 0) {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8 && value != 16)
      return fail(ctx, DVO_HIP_ERR_INVALID, "rows_per_wave must be 0,1,2,4,8,16");
    ctx->opt_rows_per_wave = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "iters_per_sync") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "iters_per_sync must be >= 0");
    ctx->opt_iters_per_sync = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "variant") == 0) {
    if (value != 0 && (value < 5 || value > 9))
      return fail(ctx, DVO_HIP_ERR_INVALID, "variant must be 0 (all-VALU schedule), 5 (matrix-core schedule), 6 or 7 (current-frame window staged in LDS, residuals bit-identical to the oracle's), 8 or 9 (the same with contracted arithmetic)");
    if (ctx->opt_ref_order && value != 7 && value != 8) return fail(ctx, DVO_HIP_ERR_INVALID, "ref_order runs under variant 7 or 8");
    ctx->opt_variant = value;
    ctx->f32_gram_hold = 0;                                    // (a schedule asked for by name starts without history)
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "rendezvous") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "rendezvous must be 0 or 1");
    ctx->opt_rendezvous = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "ref_order") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "ref_order must be 0 or 1");
    if (value && ctx->opt_variant != 7 && ctx->opt_variant != 8) return fail(ctx, DVO_HIP_ERR_INVALID, "ref_order runs under variant 7 or 8");
    ctx->opt_ref_order = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "deterministic") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "deterministic must be 0 or 1");
    ctx->opt_deterministic = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "ref_compat") == 0) {
    if (value < 0 || value > 2) return fail(ctx, DVO_HIP_ERR_INVALID, "ref_compat must be 0, 1 or 2 (2: as 1, the table read through memory by every sweep)");
    if (value && !ctx->rcp_table.p) {
      const int rc = build_rcp_table(ctx);
      if (rc != DVO_HIP_OK) return rc;
    }
    ctx->opt_ref_compat = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "resident") == 0) {
    if (value < -1 || value > 1) return fail(ctx, DVO_HIP_ERR_INVALID, "resident must be -1 (automatic), 0 (off) or 1 (every level)");
    ctx->opt_resident = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "small_sweep") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "small_sweep must be 0 or 1");
    ctx->opt_small_sweep = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "small_tiles") == 0) {
    if (value < 0 || value > 32) return fail(ctx, DVO_HIP_ERR_INVALID, "small_tiles must be 0 (by batch size) .. 32");
    ctx->opt_small_tiles = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "batch_groups") == 0) {
    if (value < 0 || value > 4) return fail(ctx, DVO_HIP_ERR_INVALID, "batch_groups must be 0 or 1 (one group) .. 4");
    ctx->opt_batch_groups = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "solver_occupancy") == 0) {
    if (value != 0 && value != 3) return fail(ctx, DVO_HIP_ERR_INVALID, "solver_occupancy must be 0 or 3");
    g_solver_occupancy = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "sweep_tail") == 0) {
    if (value < 0 || value > 2) return fail(ctx, DVO_HIP_ERR_INVALID, "sweep_tail must be 0, 1 (the whole step in the sweep's tail) or 2 (its wide half; the serial half in a launch behind it)");
    ctx->opt_sweep_tail = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "overlap_tails") == 0) {
    if (value < 0 || value > 1) return fail(ctx, DVO_HIP_ERR_INVALID, "overlap_tails must be 0 (off) or 1 (a level's stragglers finish beside the next level)");
    ctx->opt_overlap_tails = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "defer_ingest_pixels") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "defer_ingest_pixels must be >= 0");
    ctx->opt_defer_ingest_pixels = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "tail_lists") == 0) {
    if (value < 0 || value > 1) return fail(ctx, DVO_HIP_ERR_INVALID, "tail_lists must be 0 or 1 (the last steps of a costly level are launched over the list of pairs still on it)");
    ctx->opt_tail_lists = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "overlap_fraction") == 0) {
    if (value < 2 || value > 64) return fail(ctx, DVO_HIP_ERR_INVALID, "overlap_fraction must be in [2, 64]: a level's tail is split off once at most 1/value of the pairs is on it");
    ctx->opt_overlap_fraction = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "coarse") == 0) {
    if (value < 0 || value > 1) return fail(ctx, DVO_HIP_ERR_INVALID, "coarse must be 0 (off) or 1 (whenever the levels admit it)");
    ctx->opt_coarse = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "codebook_round_kb") == 0) {
    if (value < 1) return fail(ctx, DVO_HIP_ERR_INVALID, "codebook_round_kb must be >= 1");
    ctx->opt_codebook_round_kb = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "coarse_pixels") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "coarse_pixels must be >= 0");
    ctx->opt_coarse_pixels = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "coarse_workgroups") == 0) {
    if (value != 0 && value != 3 && value != 4) return fail(ctx, DVO_HIP_ERR_INVALID, "coarse_workgroups must be 0, 3 or 4");
    ctx->opt_coarse_wgs = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "resident_flags") == 0) {
    ctx->opt_resident_flags = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "resident_cooperative") == 0) {
    ctx->opt_resident_cooperative = value != 0;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "resident_rows") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "resident_rows must be >= 0");
    ctx->opt_resident_rows = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "resident_group") == 0) {
    if (value < 0 || value > kResidentMaxGroup || (value & (value - 1))) return fail(ctx, DVO_HIP_ERR_INVALID, "resident_group must be 0 or a power of two <= 64");
    ctx->opt_resident_group = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "build_workgroups") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "build_workgroups must be >= 0");
    ctx->opt_build_workgroups = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "tail_speculation") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "tail_speculation must be >= 0");
    ctx->opt_tail_speculation = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "solver_waves") == 0) {
    if (value != 0 && value != 2 && value != 4) return fail(ctx, DVO_HIP_ERR_INVALID, "solver_waves must be 0, 2 or 4");
    ctx->opt_solver_waves = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "ll_blocks") == 0) {
    if (value < 0 || value > kLlBlocksPerPair) return fail(ctx, DVO_HIP_ERR_INVALID, "ll_blocks must be 0..32");
    ctx->opt_ll_blocks = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "gram_lo_parts") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "gram_lo_parts must be 0 or 1");
    ctx->opt_gram_lo_parts = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "compact_residuals") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "compact_residuals must be 0 or 1");
    ctx->opt_compact_residuals = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "min_workgroups") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "min_workgroups must be >= 0");
    ctx->opt_min_workgroups = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "condition_number") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "condition_number must be 0 or 1");
    ctx->opt_condition_number = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "defer_ingest") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "defer_ingest must be 0 or 1");
    ctx->opt_defer_ingest = value;
    if (!value) DVO_FLUSH_DEFERRED(ctx);
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "stream_policy") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "stream_policy must be 0 or 1");
    ctx->opt_stream_policy = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "keep_raw_copy") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "keep_raw_copy must be 0 or 1");
    ctx->opt_keep_raw_copy = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "table_cache") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "table_cache must be 0 or 1");
    ctx->tables.cache = value != 0;
    for (PinnedRing::Sent& c : ctx->tables.sent) c.dst = nullptr;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "graph_resident") == 0) {
    if (value != 0 && value != 1) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_resident must be 0 or 1 (dvo_hip_graph_optimize runs a resident-sized graph in one launch)");
    ctx->opt_graph_resident = value;
    return DVO_HIP_OK;
  }
  if (std::strcmp(key, "fused_ll_pixels") == 0) {
    if (value < 0) return fail(ctx, DVO_HIP_ERR_INVALID, "fused_ll_pixels must be >= 0");
    ctx->opt_fused_ll_pixels = value;
    return DVO_HIP_OK;
  }
  return fail(ctx, DVO_HIP_ERR_INVALID, "unknown option");
}
