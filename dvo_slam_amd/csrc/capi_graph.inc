// capi_graph.inc -- the keyframe pose graph behind the C-ABI (include/dvo_hip.h, dvo_hip_graph_*; arithmetic and schedule: pose_graph.h;
// kernels: pose_graph.hip).  Every launch runs on the context's main stream; arguments are checked before anything is launched or
// changed.  Two schedules of the same statements.  The launch path: the host enqueues one Levenberg-Marquardt trial -- the start of the
// solve, cg_max_iterations pairs of launches that return at once when the solve has ended, the step, the cost at the stepped poses --
// reads one small record, and judges the trial with pg_lm_judge.  The resident path (dvo_hip_graph_optimize_batch; dvo_hip_graph_optimize
// under option "graph_resident"): graphs of at most kPgResidentMaxVertices vertices and kPgResidentMaxEdges edges, one workgroup each, in
// ONE launch of k_pg_resident that judges its trials itself; one read afterwards.  The same bits either way.  Textually included by
// capi.hip inside its extern "C" block.
struct dvo_hip_graph {
  dvo_hip_context* ctx = nullptr;
  int n = 0, m = 0;
  bool any_free = false;               // a vertex that is neither fixed nor without an edge
  int cur = 0;                         // poses[cur] is the estimate, the other buffer takes a trial's stepped poses
  std::vector<unsigned char> fixed_host;
  DevBuf poses[2], fixed, from, to, Z, omega, delta, inc_start, inc, E, V, partials, record;
};

namespace {

// what the host reads per trial: the solve's state and the two sums of launch_pg_reduce
struct PgRecord {
  PgCgState cg;
  double sums[2];
};

int graph_vertex_blocks(const dvo_hip_graph* g) { return (g->n + kPgBlock - 1) / kPgBlock; }
int graph_edge_blocks(const dvo_hip_graph* g) { return (g->m + kPgBlock - 1) / kPgBlock; }

// the partials: rz (two rows of vertex blocks) | pAp | vertex scalar (largest diagonal entry, scale) | cost (edge blocks)
struct PgPartials {
  double *rz, *pap, *vertex, *cost;
};
PgPartials graph_partials(const dvo_hip_graph* g) {
  const size_t nb = size_t(graph_vertex_blocks(g));
  double* p = g->partials.as<double>();
  return PgPartials{p, p + 2 * nb, p + 3 * nb, p + 4 * nb};
}

PgGraph graph_view(const dvo_hip_graph* g) {
  PgGraph v;
  v.n = g->n;
  v.m = g->m;
  v.fixed = g->fixed.as<unsigned char>();
  v.from = g->from.as<int>();
  v.to = g->to.as<int>();
  v.Z = g->Z.as<double>();
  v.omega = g->omega.as<double>();
  v.delta = g->delta.as<double>();
  v.inc_start = g->inc_start.as<int>();
  v.inc = g->inc.as<int>();
  v.E = g->E.as<double>();
  v.V = g->V.as<double>();
  return v;
}

int check_graph(dvo_hip_context* ctx, const dvo_hip_graph* g, const char* who) {
  if (!ctx || !g) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  if (g->ctx != ctx) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a graph of another context");
  return DVO_HIP_OK;
}

bool all_finite(const double* a, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!pg_finite(a[i])) return false;
  return true;
}

int graph_upload(dvo_hip_context* ctx, DevBuf& buf, const void* host, size_t bytes) {
  if (bytes == 0) return DVO_HIP_OK;
  DVO_HIP_TRY(ctx, buf.reserve(bytes));
  DVO_HIP_TRY(ctx, hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the host arrays are the caller's, or locals)
  return DVO_HIP_OK;
}

// the vertex incidence lists of m edges: a counting sort by vertex, which leaves every list in ascending edge index
int graph_set_incidence(dvo_hip_context* ctx, dvo_hip_graph* g, int m, const int32_t* from, const int32_t* to) {
  std::vector<int> start(size_t(g->n) + 1, 0), inc(size_t(m) * 2);
  for (int k = 0; k < m; ++k) {
    start[size_t(from[k]) + 1] += 1;
    start[size_t(to[k]) + 1] += 1;
  }
  for (int v = 0; v < g->n; ++v) start[size_t(v) + 1] += start[size_t(v)];
  std::vector<int> at(start.begin(), start.end() - 1);
  for (int k = 0; k < m; ++k) {
    inc[size_t(at[size_t(from[k])]++)] = k * 2;
    inc[size_t(at[size_t(to[k])]++)] = k * 2 + 1;
  }
  g->any_free = false;
  for (int v = 0; v < g->n; ++v) g->any_free = g->any_free || (!g->fixed_host[size_t(v)] && start[size_t(v) + 1] > start[size_t(v)]);
  int rc = graph_upload(ctx, g->inc_start, start.data(), start.size() * sizeof(int));
  if (rc == DVO_HIP_OK) rc = graph_upload(ctx, g->inc, inc.data(), inc.size() * sizeof(int));
  return rc;
}

int graph_read_record(dvo_hip_context* ctx, dvo_hip_graph* g, PgRecord* out) {
  DVO_HIP_TRY(ctx, hipMemcpyAsync(out, g->record.p, sizeof(PgRecord), hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}

// every edge's record at poses[which] and the cost there
int graph_linearise(dvo_hip_context* ctx, dvo_hip_graph* g, int which, bool with_blocks, double* cost) {
  const PgPartials p = graph_partials(g);
  launch_pg_linearise(ctx->stream, graph_view(g), g->poses[which].as<double>(), with_blocks, p.cost);
  launch_pg_reduce(ctx->stream, p.cost, graph_edge_blocks(g), nullptr, 0, reinterpret_cast<PgRecord*>(g->record.p)->sums);
  DVO_HIP_TRY(ctx, hipGetLastError());
  PgRecord r;
  const int rc = graph_read_record(ctx, g, &r);
  if (rc == DVO_HIP_OK) *cost = r.sums[0];
  return rc;
}

// D and b of every vertex; the largest diagonal entry of H
int graph_gather(dvo_hip_context* ctx, dvo_hip_graph* g, double* max_diagonal) {
  const PgPartials p = graph_partials(g);
  launch_pg_gather(ctx->stream, graph_view(g), p.vertex);
  DVO_HIP_TRY(ctx, hipGetLastError());
  std::vector<double> tops(size_t(graph_vertex_blocks(g)));
  DVO_HIP_TRY(ctx, hipMemcpyAsync(tops.data(), p.vertex, tops.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *max_diagonal = 0.0;
  for (double t : tops) *max_diagonal = t > *max_diagonal ? t : *max_diagonal;
  return DVO_HIP_OK;
}

// per-vertex or per-edge components [first, first + comps) of a component-major device array of `count` columns, row-major to the host
int graph_download_rows(dvo_hip_context* ctx, const double* device, int count, int first, int comps, double* out) {
  if (!out || count == 0) return DVO_HIP_OK;
  std::vector<double> t(size_t(count) * comps);
  DVO_HIP_TRY(ctx, hipMemcpyAsync(t.data(), device + size_t(first) * count, t.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < count; ++i)
    for (int c = 0; c < comps; ++c) out[size_t(i) * comps + c] = t[size_t(c) * count + i];
  return DVO_HIP_OK;
}

// the rules of a parameter set, for both schedules
bool graph_params_ok(const dvo_hip_graph_params& prm) {
  return prm.max_iterations >= 0 && prm.cg_max_iterations >= 1 && prm.cg_max_iterations <= 100000 && prm.cg_tolerance > 0.0 && prm.cg_tolerance < 1.0 &&
         prm.min_relative_decrease >= 0.0 && pg_finite(prm.min_relative_decrease) && prm.initial_damping_scale > 0.0 &&
         pg_finite(prm.initial_damping_scale);
}
const char* const kGraphParamRules = "need max_iterations >= 0, 1 <= cg_max_iterations <= 100000, 0 < cg_tolerance < 1, "
                                     "min_relative_decrease >= 0 and initial_damping_scale > 0";

bool graph_resident_sized(const dvo_hip_graph* g) { return g->n <= kPgResidentMaxVertices && g->m <= kPgResidentMaxEdges; }

static_assert(sizeof(PgResidentIteration) == sizeof(dvo_hip_graph_iteration), "k_pg_resident writes the records as the caller reads them");

// The resident schedule (k_pg_resident): every graph optimised from start to end by one workgroup of ONE launch, then one
// synchronisation and one read.  The arguments have been checked: resident-sized graphs of this context, each once, good parameters.
// params: one per graph.  records (may be null): max_records per graph.
int graph_optimize_resident(dvo_hip_context* ctx, int n_graphs, dvo_hip_graph* const* graphs, const dvo_hip_graph_params* params,
                            dvo_hip_graph_report* reports, dvo_hip_graph_iteration* records, int max_records) {
  int stride = 0;                                                   // records the kernel keeps per graph: no trial beyond max_iterations is run
  for (int i = 0; i < n_graphs; ++i) stride = params[i].max_iterations > stride ? params[i].max_iterations : stride;
  stride = stride < max_records ? stride : max_records;
  std::vector<PgResidentJob> jobs(static_cast<size_t>(n_graphs));
  for (int i = 0; i < n_graphs; ++i) {
    const dvo_hip_graph* g = graphs[i];
    PgResidentJob& job = jobs[size_t(i)];
    job.g = graph_view(g);
    job.poses[0] = g->poses[0].as<double>();
    job.poses[1] = g->poses[1].as<double>();
    job.cur = g->cur;
    job.any_free = g->any_free ? 1 : 0;
    job.max_iterations = params[i].max_iterations;
    job.cg_max_iterations = params[i].cg_max_iterations;
    job.cg_tolerance = params[i].cg_tolerance;
    job.min_relative_decrease = params[i].min_relative_decrease;
    job.initial_damping_scale = params[i].initial_damping_scale;
  }
  const size_t job_bytes = jobs.size() * sizeof(PgResidentJob), out_bytes = jobs.size() * sizeof(PgResidentOut);
  const size_t record_bytes = jobs.size() * size_t(stride) * sizeof(PgResidentIteration);
  DVO_HIP_TRY(ctx, ctx->graph_jobs.reserve(job_bytes));
  DVO_HIP_TRY(ctx, ctx->graph_outs.reserve(out_bytes + record_bytes));
  PgResidentOut* outs = ctx->graph_outs.as<PgResidentOut>();
  PgResidentIteration* device_records = reinterpret_cast<PgResidentIteration*>(outs + n_graphs);
  DVO_HIP_TRY(ctx, hipMemcpyAsync(ctx->graph_jobs.p, jobs.data(), job_bytes, hipMemcpyHostToDevice, ctx->stream));
  size_t stage_bytes = 0;                                           // the LDS of a workgroup: what the largest graph that fits needs
  for (int i = 0; i < n_graphs; ++i) {
    const size_t need = graphs[i]->m > 0 ? pg_resident_stage_bytes(graphs[i]->n, graphs[i]->m) : 0;
    if (need <= size_t(kPgResidentStageBytes) && need > stage_bytes) stage_bytes = need;
  }
  launch_pg_resident(ctx->stream, ctx->graph_jobs.as<PgResidentJob>(), n_graphs, outs, device_records, stride, stage_bytes);
  DVO_HIP_TRY(ctx, hipGetLastError());
  std::vector<unsigned char> host(out_bytes + record_bytes);
  DVO_HIP_TRY(ctx, hipMemcpyAsync(host.data(), ctx->graph_outs.p, host.size(), hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < n_graphs; ++i) {
    PgResidentOut o;
    std::memcpy(&o, host.data() + size_t(i) * sizeof(PgResidentOut), sizeof o);
    dvo_hip_graph_report& r = reports[i];
    std::memset(&r, 0, sizeof r);
    r.status = o.status;
    r.iterations = o.iterations;
    r.accepted = o.accepted;
    r.cg_iterations = o.cg_iterations;
    r.initial_cost = o.initial_cost;
    r.final_cost = o.final_cost;
    r.final_damping = o.final_damping;
    graphs[i]->cur = o.cur & 1;
    const int kept = o.iterations < stride ? o.iterations : stride;
    if (kept > 0)
      std::memcpy(records + size_t(i) * size_t(max_records), host.data() + out_bytes + size_t(i) * size_t(stride) * sizeof(PgResidentIteration),
                  size_t(kept) * sizeof(PgResidentIteration));
  }
  ctx->graph_resident_solves += n_graphs;
  return DVO_HIP_OK;
}

}  // namespace

int dvo_hip_graph_create(dvo_hip_context* ctx, dvo_hip_graph** out) {
  DVO_LOCK(ctx);
  if (!ctx || !out) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_create: bad argument");
  dvo_hip_graph* g = new dvo_hip_graph();
  g->ctx = ctx;
  *out = g;
  return DVO_HIP_OK;
}

void dvo_hip_graph_destroy(dvo_hip_context* ctx, dvo_hip_graph* g) {
  DVO_LOCK(ctx);
  if (!g) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  for (DevBuf* b : {&g->poses[0], &g->poses[1], &g->fixed, &g->from, &g->to, &g->Z, &g->omega, &g->delta, &g->inc_start, &g->inc, &g->E, &g->V,
                    &g->partials, &g->record})
    b->release();
  delete g;
}

int dvo_hip_graph_set_vertices(dvo_hip_context* ctx, dvo_hip_graph* g, int n, const double* poses, const unsigned char* fixed) {
  DVO_LOCK(ctx);
  int rc = check_graph(ctx, g, "graph_set_vertices");
  if (rc != DVO_HIP_OK) return rc;
  if (n <= 0 || n > kPgMaxVertices || !poses) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_vertices: need 1 <= n <= 2^20 poses");
  if (!all_finite(poses, size_t(n) * 16)) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_vertices: a pose has a non-finite entry");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  g->n = n;
  g->m = 0;
  g->cur = 0;
  g->fixed_host.assign(size_t(n), 0);
  if (fixed)
    for (int v = 0; v < n; ++v) g->fixed_host[size_t(v)] = fixed[v] ? 1 : 0;
  const size_t nb = size_t(graph_vertex_blocks(g));
  rc = graph_upload(ctx, g->poses[0], poses, size_t(n) * 16 * sizeof(double));
  if (rc == DVO_HIP_OK) rc = graph_upload(ctx, g->fixed, g->fixed_host.data(), size_t(n));
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, g->poses[1].reserve(size_t(n) * 16 * sizeof(double)));
  DVO_HIP_TRY(ctx, g->V.reserve(size_t(n) * kPgVertexComps * sizeof(double)));
  DVO_HIP_TRY(ctx, g->partials.reserve((4 * nb + size_t(kPgMaxEdges / kPgBlock)) * sizeof(double)));
  DVO_HIP_TRY(ctx, g->record.reserve(sizeof(PgRecord)));
  return graph_set_incidence(ctx, g, 0, nullptr, nullptr);
}

int dvo_hip_graph_set_poses(dvo_hip_context* ctx, dvo_hip_graph* g, int n, const double* poses) {
  DVO_LOCK(ctx);
  const int rc = check_graph(ctx, g, "graph_set_poses");
  if (rc != DVO_HIP_OK) return rc;
  if (n <= 0 || n != g->n || !poses) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_poses: need the poses of the graph's n vertices");
  if (!all_finite(poses, size_t(n) * 16)) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_poses: a pose has a non-finite entry");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return graph_upload(ctx, g->poses[g->cur], poses, size_t(n) * 16 * sizeof(double));
}

int dvo_hip_graph_set_edges(dvo_hip_context* ctx, dvo_hip_graph* g, int m, const int32_t* from, const int32_t* to, const double* measurements,
                            const double* information, const double* delta) {
  DVO_LOCK(ctx);
  int rc = check_graph(ctx, g, "graph_set_edges");
  if (rc != DVO_HIP_OK) return rc;
  if (g->n <= 0) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_edges: set the vertices first");
  if (m < 0 || m > kPgMaxEdges || (m > 0 && (!from || !to || !measurements || !information)))
    return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_edges: need 0 <= m <= 2^22 edges");
  for (int k = 0; k < m; ++k) {
    if (from[k] < 0 || from[k] >= g->n || to[k] < 0 || to[k] >= g->n) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_edges: a vertex index out of range");
    if (from[k] == to[k]) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_edges: an edge from a vertex to itself");
    if (delta && !(delta[k] >= 0.0 && pg_finite(delta[k]))) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_edges: need a finite delta >= 0");
  }
  if (m > 0 && !(all_finite(measurements, size_t(m) * 16) && all_finite(information, size_t(m) * 36)))
    return fail(ctx, DVO_HIP_ERR_INVALID, "graph_set_edges: a measurement or an information matrix has a non-finite entry");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<double> no_kernel;
  if (!delta) no_kernel.assign(size_t(m), 0.0);
  g->m = 0;                                                         // (until everything below has arrived)
  rc = graph_upload(ctx, g->from, from, size_t(m) * sizeof(int32_t));
  if (rc == DVO_HIP_OK) rc = graph_upload(ctx, g->to, to, size_t(m) * sizeof(int32_t));
  if (rc == DVO_HIP_OK) rc = graph_upload(ctx, g->Z, measurements, size_t(m) * 16 * sizeof(double));
  if (rc == DVO_HIP_OK) rc = graph_upload(ctx, g->omega, information, size_t(m) * 36 * sizeof(double));
  if (rc == DVO_HIP_OK) rc = graph_upload(ctx, g->delta, delta ? delta : no_kernel.data(), size_t(m) * sizeof(double));
  if (rc == DVO_HIP_OK) rc = graph_set_incidence(ctx, g, m, from, to);
  if (rc != DVO_HIP_OK) return rc;
  DVO_HIP_TRY(ctx, g->E.reserve(size_t(m) * kPgEdgeComps * sizeof(double)));
  g->m = m;
  return DVO_HIP_OK;
}

dvo_hip_graph_params dvo_hip_graph_params_default(void) {
  dvo_hip_graph_params p;
  std::memset(&p, 0, sizeof p);
  p.max_iterations = 50;
  p.cg_max_iterations = 200;
  p.cg_tolerance = 1e-8;
  p.min_relative_decrease = 1e-9;
  p.initial_damping_scale = 1e-5;
  return p;
}

int dvo_hip_graph_optimize(dvo_hip_context* ctx, dvo_hip_graph* g, const dvo_hip_graph_params* params, dvo_hip_graph_report* out,
                           dvo_hip_graph_iteration* records, int max_records) {
  DVO_LOCK(ctx);
  int rc = check_graph(ctx, g, "graph_optimize");
  if (rc != DVO_HIP_OK) return rc;
  const dvo_hip_graph_params prm = params ? *params : dvo_hip_graph_params_default();
  if (!out || g->n <= 0 || max_records < 0 || (max_records > 0 && !records)) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_optimize: bad argument");
  if (!graph_params_ok(prm)) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_optimize", kGraphParamRules);
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->opt_graph_resident && graph_resident_sized(g)) return graph_optimize_resident(ctx, 1, &g, &prm, out, records, max_records);
  std::memset(out, 0, sizeof *out);
  out->status = DVO_HIP_GRAPH_NOTHING_TO_DO;
  if (g->m == 0) return DVO_HIP_OK;
  double cost = 0.0, top = 0.0;
  rc = graph_linearise(ctx, g, g->cur, true, &cost);
  if (rc != DVO_HIP_OK) return rc;
  out->initial_cost = out->final_cost = cost;
  if (!g->any_free) return DVO_HIP_OK;
  rc = graph_gather(ctx, g, &top);
  if (rc != DVO_HIP_OK) return rc;
  PgLm lm;
  pg_lm_begin(lm, cost, prm.initial_damping_scale, top);
  const PgPartials p = graph_partials(g);
  PgRecord* record = reinterpret_cast<PgRecord*>(g->record.p);
  out->status = DVO_HIP_GRAPH_ITERATION_CAP;
  for (int it = 0; it < prm.max_iterations; ++it) {
    const PgGraph view = graph_view(g);
    const double lambda = lm.lambda, before = lm.cost;
    const int other = g->cur ^ 1;
    DVO_HIP_TRY(ctx, hipMemsetAsync(g->record.p, 0, sizeof(PgRecord), ctx->stream));
    launch_pg_cg_init(ctx->stream, view, &record->cg, lambda, p.rz);
    for (int k = 0; k < prm.cg_max_iterations; ++k) {
      launch_pg_multiply(ctx->stream, view, &record->cg, p.rz, p.pap, k, lambda, prm.cg_tolerance, false);
      launch_pg_cg_update(ctx->stream, view, &record->cg, p.pap, p.rz, k);
    }
    launch_pg_apply(ctx->stream, view, lambda, g->poses[g->cur].as<double>(), g->poses[other].as<double>(), p.vertex);
    launch_pg_linearise(ctx->stream, view, g->poses[other].as<double>(), false, p.cost);
    launch_pg_reduce(ctx->stream, p.cost, graph_edge_blocks(g), p.vertex, graph_vertex_blocks(g), record->sums);
    DVO_HIP_TRY(ctx, hipGetLastError());
    PgRecord r;
    rc = graph_read_record(ctx, g, &r);
    if (rc != DVO_HIP_OK) return rc;
    const int cg_status = r.cg.stop_multiply != kPgCgRunning ? r.cg.stop_multiply : kPgCgIterationCap;
    int stop = -1;
    const bool accepted = pg_lm_judge(lm, r.sums[0], r.sums[1], cg_status, prm.min_relative_decrease, &stop);
    if (it < max_records) {
      dvo_hip_graph_iteration& rec = records[it];
      std::memset(&rec, 0, sizeof rec);
      rec.cost_before = before;
      rec.cost_after = r.sums[0];
      rec.damping = lambda;
      rec.cg_iterations = r.cg.iterations;
      rec.cg_status = cg_status;
      rec.accepted = accepted ? 1 : 0;
    }
    out->iterations += 1;
    out->cg_iterations += r.cg.iterations;
    if (accepted) {
      out->accepted += 1;
      g->cur = other;
    }
    if (stop >= 0) {
      out->status = stop;
      break;
    }
    if (accepted && it + 1 < prm.max_iterations) {                 // (a rejected trial leaves the linearisation as it is)
      double again = 0.0;
      rc = graph_linearise(ctx, g, g->cur, true, &again);
      if (rc == DVO_HIP_OK) rc = graph_gather(ctx, g, &top);
      if (rc != DVO_HIP_OK) return rc;
    }
  }
  out->final_cost = lm.cost;
  out->final_damping = lm.lambda;
  return DVO_HIP_OK;
}

int dvo_hip_graph_optimize_batch(dvo_hip_context* ctx, int n_graphs, dvo_hip_graph* const* graphs, const dvo_hip_graph_params* params,
                                 dvo_hip_graph_report* reports, dvo_hip_graph_iteration* records, int max_records) {
  DVO_LOCK(ctx);
  const char* who = "graph_optimize_batch";
  if (!ctx) return dvo_hip_device_count() > 0 ? DVO_HIP_ERR_INVALID : DVO_HIP_ERR_NO_DEVICE;
  if (n_graphs <= 0 || !graphs || !reports || max_records < 0 || (max_records > 0 && !records)) return fail(ctx, DVO_HIP_ERR_INVALID, who, "bad argument");
  for (int i = 0; i < n_graphs; ++i) {
    const int rc = check_graph(ctx, graphs[i], who);
    if (rc != DVO_HIP_OK) return rc;
    if (graphs[i]->n <= 0) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a graph without vertices");
    if (!graph_resident_sized(graphs[i])) return fail(ctx, DVO_HIP_ERR_INVALID, who, "a graph beyond 1024 vertices or 4096 edges: dvo_hip_graph_optimize takes it");
  }
  std::vector<const dvo_hip_graph*> sorted(graphs, graphs + n_graphs);
  std::sort(sorted.begin(), sorted.end(), std::less<const dvo_hip_graph*>());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(ctx, DVO_HIP_ERR_INVALID, who, "the same graph twice");
  std::vector<dvo_hip_graph_params> prm(static_cast<size_t>(n_graphs), dvo_hip_graph_params_default());
  if (params) prm.assign(params, params + n_graphs);
  for (int i = 0; i < n_graphs; ++i)
    if (!graph_params_ok(prm[size_t(i)])) return fail(ctx, DVO_HIP_ERR_INVALID, who, kGraphParamRules);
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  return graph_optimize_resident(ctx, n_graphs, graphs, prm.data(), reports, records, max_records);
}

int dvo_hip_graph_get_poses(dvo_hip_context* ctx, dvo_hip_graph* g, int n, double* poses_out) {
  DVO_LOCK(ctx);
  const int rc = check_graph(ctx, g, "graph_get_poses");
  if (rc != DVO_HIP_OK) return rc;
  if (n <= 0 || n != g->n || !poses_out) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_get_poses: need room for the graph's n poses");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  DVO_HIP_TRY(ctx, hipMemcpyAsync(poses_out, g->poses[g->cur].p, size_t(n) * 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  DVO_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DVO_HIP_OK;
}

int dvo_hip_graph_linearise(dvo_hip_context* ctx, dvo_hip_graph* g, double* error_out, double* chi2_out, double* weight_out, double* blocks_out,
                            double* gradient_out, double* cost_out) {
  DVO_LOCK(ctx);
  int rc = check_graph(ctx, g, "graph_linearise");
  if (rc != DVO_HIP_OK) return rc;
  if (g->n <= 0) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_linearise: set the vertices first");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  double cost = 0.0;
  if (g->m > 0) rc = graph_linearise(ctx, g, g->cur, true, &cost);
  const double* E = g->E.as<double>();
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, E, g->m, kPgE, 6, error_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, E, g->m, kPgS, 1, chi2_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, E, g->m, kPgW, 1, weight_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, E, g->m, kPgAii, 108, blocks_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, E, g->m, kPgGi, 12, gradient_out);
  if (rc == DVO_HIP_OK && cost_out) *cost_out = cost;
  return rc;
}

int dvo_hip_graph_edge_stats(dvo_hip_context* ctx, dvo_hip_graph* g, int m, double* chi2_out, double* weight_out) {
  DVO_LOCK(ctx);
  int rc = check_graph(ctx, g, "graph_edge_stats");
  if (rc != DVO_HIP_OK) return rc;
  if (m != g->m || g->n <= 0) return fail(ctx, DVO_HIP_ERR_INVALID, "graph_edge_stats: need room for the graph's m edges");
  if (m == 0) return DVO_HIP_OK;
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  double cost = 0.0;
  rc = graph_linearise(ctx, g, g->cur, false, &cost);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, g->E.as<double>(), m, kPgS, 1, chi2_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, g->E.as<double>(), m, kPgW, 1, weight_out);
  return rc;
}

int dvo_hip_graph_multiply(dvo_hip_context* ctx, dvo_hip_graph* g, double damping, const double* p_in, double* y_out, double* pty_out,
                           double* diagonal_out, double* rhs_out, double* inverse_out) {
  DVO_LOCK(ctx);
  int rc = check_graph(ctx, g, "graph_multiply");
  if (rc != DVO_HIP_OK) return rc;
  if (g->n <= 0 || !p_in || !(damping >= 0.0 && pg_finite(damping)) || !all_finite(p_in, size_t(g->n) * 6))
    return fail(ctx, DVO_HIP_ERR_INVALID, "graph_multiply: need vertices, a finite p of n x 6 and a finite damping >= 0");
  DVO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int n = g->n;
  const PgPartials p = graph_partials(g);
  PgRecord* record = reinterpret_cast<PgRecord*>(g->record.p);
  double cost = 0.0, top = 0.0;
  if (g->m > 0) rc = graph_linearise(ctx, g, g->cur, true, &cost);
  if (rc == DVO_HIP_OK) rc = graph_gather(ctx, g, &top);
  if (rc != DVO_HIP_OK) return rc;
  std::vector<double> t(size_t(n) * 6);
  for (int v = 0; v < n; ++v)
    for (int c = 0; c < 6; ++c) t[size_t(c) * n + v] = p_in[size_t(v) * 6 + c];
  double* V = g->V.as<double>();
  DVO_HIP_TRY(ctx, hipMemsetAsync(g->record.p, 0, sizeof(PgRecord), ctx->stream));
  launch_pg_cg_init(ctx->stream, graph_view(g), &record->cg, damping, p.rz);
  DVO_HIP_TRY(ctx, hipMemcpyAsync(V + size_t(kPgP0) * n, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_pg_multiply(ctx->stream, graph_view(g), &record->cg, p.rz, p.pap, 0, damping, 0.5, true);
  launch_pg_reduce(ctx->stream, p.pap, graph_vertex_blocks(g), nullptr, 0, record->sums);
  DVO_HIP_TRY(ctx, hipGetLastError());
  PgRecord r;
  rc = graph_read_record(ctx, g, &r);
  if (rc == DVO_HIP_OK && pty_out) *pty_out = r.sums[0];
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, V, n, kPgY, 6, y_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, V, n, kPgD, 36, diagonal_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, V, n, kPgB, 6, rhs_out);
  if (rc == DVO_HIP_OK) rc = graph_download_rows(ctx, V, n, kPgMinv, 36, inverse_out);
  return rc;
}
