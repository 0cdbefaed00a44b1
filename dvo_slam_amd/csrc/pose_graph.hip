// pose_graph.hip -- the kernels of the pose-graph optimiser (arithmetic and order of every sum: pose_graph.h; driver: capi_graph.inc).
// One lane per edge (k_pg_linearise) or per vertex (the others), kPgBlock of them per workgroup: a workgroup's LDS tree is one subtree
// of a scalar's adjacent-pair tree, and the kernel that needs the scalar walks the rest of the tree over the workgroups' partials
// itself -- every workgroup the same adds, so all of them reach the same decision.  No atomics, no grid-wide wait; a launch reads the
// stop word the launch BEFORE it wrote and returns at once when the solve has ended.
// k_pg_resident is the other schedule of the same statements: a resident-sized graph (kPgResidentMaxVertices, kPgResidentMaxEdges)
// optimised from start to end by ONE workgroup in ONE launch, a batch of graphs by one workgroup each.
#include <hip/hip_runtime.h>

#include "global_ptr.h"
#include "launch.h"
#include "pose_graph.h"

namespace dvo_hip {
namespace {

// the adjacent-pair tree over the workgroup's kPgBlock values; every lane gets the sum
__device__ double block_tree(double v, double* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int stride = 1; stride < kPgBlock; stride *= 2) {
    if ((t & (2 * stride - 1)) == 0) lds[t] += lds[t + stride];
    __syncthreads();
  }
  const double sum = lds[0];
  __syncthreads();
  return sum;
}

// pg_tree_sum over `count` partials: a lane takes padded / kPgBlock adjacent ones, the workgroup's tree the rest
__device__ double partials_tree(const double* partials, int count, double* lds) {
  const size_t padded = pg_pad_pow2(size_t(count)), chunk = padded > size_t(kPgBlock) ? padded / kPgBlock : 1;
  const size_t lo = size_t(threadIdx.x) * chunk;
  double v = 0.0;
  if (lo < size_t(count)) v = pg_tree_raw(partials + lo, size_t(count) - lo < chunk ? size_t(count) - lo : chunk, chunk);
  return block_tree(v, lds) + 0.0;
}

__global__ __launch_bounds__(kPgBlock) void k_pg_linearise(PgGraph g, const double* poses, int with_blocks, double* cost_partials) {
  __shared__ double lds[kPgBlock];
  const int k = blockIdx.x * kPgBlock + threadIdx.x;
  const double rho = k < g.m ? pg_linearise_edge(g, poses, k, with_blocks != 0) : 0.0;
  const double sum = block_tree(rho, lds);
  if (threadIdx.x == 0) cost_partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kPgBlock) void k_pg_gather(PgGraph g, double* max_partials) {
  __shared__ double lds[kPgBlock];
  const int v = blockIdx.x * kPgBlock + threadIdx.x, t = threadIdx.x;
  lds[t] = v < g.n ? pg_gather_vertex(g, v) : 0.0;
  __syncthreads();
  for (int stride = kPgBlock / 2; stride > 0; stride /= 2) {
    if (t < stride) lds[t] = lds[t + stride] > lds[t] ? lds[t + stride] : lds[t];
    __syncthreads();
  }
  if (t == 0) max_partials[blockIdx.x] = lds[0];
}

// (st was cleared by the driver; a failed factorisation is stored by whichever lanes met one: the same word, the same value)
__global__ __launch_bounds__(kPgBlock) void k_pg_cg_init(PgGraph g, PgCgState* st, double lambda, double* rz_partials) {
  __shared__ double lds[kPgBlock];
  const int v = blockIdx.x * kPgBlock + threadIdx.x;
  bool ok = true;
  const double rz = v < g.n ? pg_cg_init_vertex(g, v, lambda, &ok) : 0.0;
  if (!ok) st->cholesky_failed = 1;
  const double sum = block_tree(rz, lds);
  if (threadIdx.x == 0) rz_partials[blockIdx.x] = sum;
}

// Multiply `it` of a solve.  rz_partials: two rows of n_blocks, row it & 1 holds r^T z as cg_init (it == 0) or the vector kernel of
// iteration it - 1 left it.  mode kPgDirGiven: the test hook, p as stored at kPgP0, no state.
__global__ __launch_bounds__(kPgBlock) void k_pg_multiply(PgGraph g, PgCgState* st, const double* rz_partials, double* pap_partials, int n_blocks,
                                                          int it, double lambda, double tolerance, int given) {
  __shared__ double lds[kPgBlock];
  __shared__ int stopped;
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  int mode = kPgDirGiven;
  double beta = 0.0;
  if (!given) {
    if (threadIdx.x == 0) stopped = st->stop_multiply;
    __syncthreads();
    if (stopped != 0) {
      if (writer) st->stop_vector = stopped;
      return;
    }
    const double rz = partials_tree(rz_partials + size_t(it & 1) * n_blocks, n_blocks, lds);
    PgCgState s = {};                                               // (only the words no workgroup of THIS launch writes)
    s.rz0 = it == 0 ? rz : st->rz0;
    if (it > 0) s.rz[(it - 1) & 1] = st->rz[(it - 1) & 1];
    s.cholesky_failed = st->cholesky_failed;
    const int status = pg_cg_before_multiply(s, it, rz, tolerance, &beta);
    if (writer) {
      st->stop_vector = status;
      if (status == kPgCgRunning) {
        if (it == 0) st->rz0 = rz;
        st->rz[it & 1] = rz;
        st->iterations = it + 1;
      }
    }
    if (status != kPgCgRunning) return;
    mode = it == 0 ? kPgDirFirst : kPgDirNext;
  }
  const int v = blockIdx.x * kPgBlock + threadIdx.x;
  const int p_new = given || (it & 1) == 0 ? kPgP0 : kPgP1, p_old = p_new == kPgP0 ? kPgP1 : kPgP0;
  const double py = v < g.n ? pg_multiply_vertex(g, v, lambda, mode, beta, p_old, p_new) : 0.0;
  const double sum = block_tree(py, lds);
  if (threadIdx.x == 0) pap_partials[blockIdx.x] = sum;
}

// The vector kernel of iteration `it`: x, r, z and the partials of the next r^T z.
__global__ __launch_bounds__(kPgBlock) void k_pg_cg_update(PgGraph g, PgCgState* st, const double* pap_partials, double* rz_partials, int n_blocks, int it) {
  __shared__ double lds[kPgBlock];
  __shared__ int stopped;
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (threadIdx.x == 0) stopped = st->stop_vector;
  __syncthreads();
  if (stopped != 0) {
    if (writer) st->stop_multiply = stopped;
    return;
  }
  const double pAp = partials_tree(pap_partials, n_blocks, lds);
  double alpha;
  const int status = pg_cg_step_length(st->rz[it & 1], pAp, &alpha);
  if (writer) st->stop_multiply = status;
  if (status != kPgCgRunning) return;
  const int v = blockIdx.x * kPgBlock + threadIdx.x;
  const double rz = v < g.n ? pg_cg_update_vertex(g, v, alpha, (it & 1) == 0 ? kPgP0 : kPgP1) : 0.0;
  const double sum = block_tree(rz, lds);
  if (threadIdx.x == 0) rz_partials[size_t((it + 1) & 1) * n_blocks + blockIdx.x] = sum;
}

__global__ __launch_bounds__(kPgBlock) void k_pg_apply(PgGraph g, double lambda, const double* poses, double* out, double* scale_partials) {
  __shared__ double lds[kPgBlock];
  const int v = blockIdx.x * kPgBlock + threadIdx.x;
  const double scale = v < g.n ? pg_apply_vertex(g, v, lambda, poses, out) : 0.0;
  const double sum = block_tree(scale, lds);
  if (threadIdx.x == 0) scale_partials[blockIdx.x] = sum;
}

// one workgroup: out[0] = the tree over a, out[1] = the tree over b (n_b may be 0)
__global__ __launch_bounds__(kPgBlock) void k_pg_reduce(const double* a, int n_a, const double* b, int n_b, double* out) {
  __shared__ double lds[kPgBlock];
  const double sa = partials_tree(a, n_a, lds);
  const double sb = n_b > 0 ? partials_tree(b, n_b, lds) : 0.0;
  if (threadIdx.x == 0) {
    out[0] = sa;
    out[1] = sb;
  }
}

// ---- the resident schedule: one workgroup optimises one graph from its first linearisation to its report -------------------------------
// The same statements in the same order as dvo_hip_graph_optimize's launches (capi_graph.inc), the same adds in every scalar's tree: a
// block's subtree as block_tree forms it, the tree over the blocks' partials as pg_tree_sum walks it.  Every lane holds the scalars and
// takes the decisions, so the control flow is uniform; phases are separated by __syncthreads() alone.

static_assert(kPgBlock == 256, "resident_tree: four wavefronts of 64");
static_assert(kPgResidentMaxVertices % kPgBlock == 0 && kPgResidentMaxEdges % kPgBlock == 0 && kPgResidentMaxVertices <= kPgResidentMaxEdges, "resident limits");
constexpr int kPgResidentPartials = kPgResidentMaxEdges / kPgBlock;

struct PgResidentLds {
  double waves[kPgBlock / 64];
  double part[kPgResidentPartials];
};

// block_tree's adds: the six levels inside a wavefront across its lanes (lane t takes lane t + stride where block_tree's lds[t] does),
// the last two over the four wavefronts' sums; every lane gets the sum
__device__ double resident_tree(double v, PgResidentLds& lds) {
  const int lane = threadIdx.x & 63;
  for (int stride = 1; stride < 64; stride *= 2) {
    const double other = __shfl_down(v, stride, 64);
    if ((lane & (2 * stride - 1)) == 0) v = v + other;
  }
  if (lane == 0) lds.waves[threadIdx.x >> 6] = v;
  __syncthreads();
  const double sum = (lds.waves[0] + lds.waves[1]) + (lds.waves[2] + lds.waves[3]);
  __syncthreads();
  return sum;
}

// the scalar of `blocks` partials left in lds.part: pg_tree_sum's adds -- the adjacent-pair tree over the partials padded with zeros to a
// power of two, plus 0.0 -- from registers (pg_tree_raw's stack of levels would live in scratch memory)
__device__ double resident_finish(int blocks, PgResidentLds& lds) {
  static_assert(kPgResidentPartials == 16, "four levels");
  __syncthreads();
  double a[16], b[8], c[4], d[2];
  for (int i = 0; i < 16; ++i) a[i] = i < blocks ? lds.part[i] : 0.0;
  for (int i = 0; i < 8; ++i) b[i] = a[2 * i] + a[2 * i + 1];
  for (int i = 0; i < 4; ++i) c[i] = b[2 * i] + b[2 * i + 1];
  for (int i = 0; i < 2; ++i) d[i] = c[2 * i] + c[2 * i + 1];
  const double sum = blocks <= 1 ? a[0] : blocks <= 2 ? b[0] : blocks <= 4 ? c[0] : blocks <= 8 ? d[0] : d[0] + d[1];
  __syncthreads();
  return sum + 0.0;
}

// A pointer out of the job record, as a pointer into the global address space: what pose_graph.h's functions reach through it becomes
// global_load / global_store, many in flight, where a pointer read from memory is a flat address with one access in flight
// (global_ptr.h).  The slot's bits are read as an integer, so that no flat pointer exists that the cast could be folded back into.
template <typename T> __device__ __forceinline__ T* global_pointer_at(T* const* slot) {
  unsigned long long bits;
  __builtin_memcpy(&bits, slot, sizeof bits);
  return (T*)(Global<T>)bits;
}

// One graph from its first linearisation to its report.  kStaged: the graph's vertex records (kPgVertexComps x n), the off-diagonal
// blocks of its edges (36 x m) and its index arrays lie in the workgroup's LDS from the first gather on -- what a CG iteration reads
// and writes never leaves the compute unit -- and the records in g.V are not touched.  The statements and their order are the same.
template <bool kStaged>
__device__ __forceinline__ void resident_optimise(const PgGraph& g, double* const (&pose_buffers)[2], const PgResidentJob& job, PgResidentLds& lds,
                                                  double* stage, PgResidentOut* outs, PgResidentIteration* records, int max_records) {
  PgGraph gg = g, gc = g;                                           // the gather's view and the solve's: where V, the blocks B and the indices lie
  double* staged_blocks = nullptr;
  if constexpr (kStaged) {
    const size_t n = size_t(g.n), m = size_t(g.m);
    double* V = stage;
    staged_blocks = V + size_t(kPgVertexComps) * n;
    int* inc_start = reinterpret_cast<int*>(staged_blocks + 36 * m);
    int* inc = inc_start + (n + 1);
    int* from = inc + 2 * m;
    int* to = from + m;
    unsigned char* fixed = reinterpret_cast<unsigned char*>(to + m);
    for (size_t i = threadIdx.x; i < n + 1; i += kPgBlock) inc_start[i] = g.inc_start[i];
    for (size_t i = threadIdx.x; i < 2 * m; i += kPgBlock) inc[i] = g.inc[i];
    for (size_t i = threadIdx.x; i < m; i += kPgBlock) {
      from[i] = g.from[i];
      to[i] = g.to[i];
    }
    for (size_t i = threadIdx.x; i < n; i += kPgBlock) fixed[i] = g.fixed[i];
    __syncthreads();
    gg.V = V;
    gg.fixed = fixed;
    gg.inc_start = inc_start;
    gg.inc = inc;
    gc = gg;
    gc.from = from;
    gc.to = to;
    gc.E = staged_blocks - size_t(kPgAij) * m;                      // (the solve reads the components kPgAij .. kPgAij + 35 of an edge record, no others)
  }
  const int t = threadIdx.x;
  const int vertex_blocks = (g.n + kPgBlock - 1) / kPgBlock, edge_blocks = (g.m + kPgBlock - 1) / kPgBlock;
  PgResidentOut out = {};
  out.status = kPgNothingToDo;
  out.cur = job.cur;
  PgLm lm = {};
  bool begun = false;
  // (the host admits resident-sized graphs only: lds.part holds no more partials)
  bool run = g.m > 0 && g.n <= kPgResidentMaxVertices && g.m <= kPgResidentMaxEdges;
  int it = 0, which = job.cur, cg_status = kPgCgRunning, cg_iterations = 0;
  bool blocks = true;                                               // the pending linearisation: at the estimate, with blocks; or at a trial's poses
  double lambda = 0.0, before = 0.0, scale = 0.0;
  while (run) {
    for (int b = 0; b < edge_blocks; ++b) {
      const int k = b * kPgBlock + t;
      const double rho = k < g.m ? pg_linearise_edge(g, which ? pose_buffers[1] : pose_buffers[0], k, blocks) : 0.0;
      const double sum = resident_tree(rho, lds);
      if (t == 0) lds.part[b] = sum;
    }
    const double cost = resident_finish(edge_blocks, lds);
    if (blocks) {
      if (!begun) {
        out.initial_cost = out.final_cost = cost;
        if (!job.any_free) break;
      }
      if constexpr (kStaged)
        for (size_t i = threadIdx.x; i < 36 * size_t(g.m); i += kPgBlock) staged_blocks[i] = g.E[size_t(kPgAij) * size_t(g.m) + i];
      double top = 0.0;
      for (int b = 0; b < vertex_blocks; ++b) {
        const int v = b * kPgBlock + t;
        const double d = v < g.n ? pg_gather_vertex(gg, v) : 0.0;
        top = d > top ? d : top;
      }
      for (int stride = 32; stride > 0; stride /= 2) {            // (the largest entry is the same in any order)
        const double other = __shfl_down(top, stride, 64);
        top = other > top ? other : top;
      }
      if ((t & 63) == 0) lds.waves[t >> 6] = top;
      __syncthreads();
      top = 0.0;
      for (int w = 0; w < kPgBlock / 64; ++w) top = lds.waves[w] > top ? lds.waves[w] : top;
      __syncthreads();
      if (!begun) {
        pg_lm_begin(lm, cost, job.initial_damping_scale, top);
        begun = true;
        out.status = kPgIterationCap;
        if (job.max_iterations <= 0) break;
      }
    } else {
      int stop = -1;
      const bool accepted = pg_lm_judge(lm, cost, scale, cg_status, job.min_relative_decrease, &stop);
      if (t == 0 && it < max_records) {
        PgResidentIteration rec = {};
        rec.cost_before = before;
        rec.cost_after = cost;
        rec.damping = lambda;
        rec.cg_iterations = cg_iterations;
        rec.cg_status = cg_status;
        rec.accepted = accepted ? 1 : 0;
        records[size_t(blockIdx.x) * size_t(max_records) + size_t(it)] = rec;
      }
      out.iterations += 1;
      out.cg_iterations += cg_iterations;
      if (accepted) {
        out.accepted += 1;
        out.cur = which;
      }
      if (stop >= 0) {
        out.status = stop;
        break;
      }
      it += 1;
      if (it >= job.max_iterations) break;
      if (accepted) {                                               // (a rejected trial leaves the linearisation as it is)
        which = out.cur;
        blocks = true;
        continue;
      }
    }
    // one trial: the solve, the step into the other pose buffer; its cost is the next linearisation
    lambda = lm.lambda;
    before = lm.cost;
    PgCgState s = {};
    int failed = 0;
    for (int b = 0; b < vertex_blocks; ++b) {
      const int v = b * kPgBlock + t;
      bool ok = true;
      const double rz = v < g.n ? pg_cg_init_vertex(gc, v, lambda, &ok) : 0.0;
      failed |= __syncthreads_or(ok ? 0 : 1);
      const double sum = resident_tree(rz, lds);
      if (t == 0) lds.part[b] = sum;
    }
    s.cholesky_failed = failed ? 1 : 0;
    double rz = resident_finish(vertex_blocks, lds);
    int status = kPgCgRunning;
    for (int k = 0; k < job.cg_max_iterations; ++k) {
      double beta, alpha;
      if (k == 0) s.rz0 = rz;
      status = pg_cg_before_multiply(s, k, rz, job.cg_tolerance, &beta);
      if (status != kPgCgRunning) break;
      s.rz[k & 1] = rz;
      s.iterations = k + 1;
      const int p_new = (k & 1) == 0 ? kPgP0 : kPgP1, p_old = p_new == kPgP0 ? kPgP1 : kPgP0;
      for (int b = 0; b < vertex_blocks; ++b) {
        const int v = b * kPgBlock + t;
        const double py = v < g.n ? pg_multiply_vertex(gc, v, lambda, k == 0 ? kPgDirFirst : kPgDirNext, beta, p_old, p_new) : 0.0;
        const double sum = resident_tree(py, lds);
        if (t == 0) lds.part[b] = sum;
      }
      const double pAp = resident_finish(vertex_blocks, lds);
      status = pg_cg_step_length(s.rz[k & 1], pAp, &alpha);
      if (status != kPgCgRunning) break;
      for (int b = 0; b < vertex_blocks; ++b) {
        const int v = b * kPgBlock + t;
        const double r = v < g.n ? pg_cg_update_vertex(gc, v, alpha, p_new) : 0.0;
        const double sum = resident_tree(r, lds);
        if (t == 0) lds.part[b] = sum;
      }
      rz = resident_finish(vertex_blocks, lds);
    }
    cg_iterations = s.iterations;
    cg_status = status == kPgCgRunning ? kPgCgIterationCap : status;
    which = out.cur ^ 1;
    for (int b = 0; b < vertex_blocks; ++b) {
      const int v = b * kPgBlock + t;
      const double x = v < g.n ? pg_apply_vertex(gc, v, lambda, out.cur ? pose_buffers[1] : pose_buffers[0], which ? pose_buffers[1] : pose_buffers[0]) : 0.0;
      const double sum = resident_tree(x, lds);
      if (t == 0) lds.part[b] = sum;
    }
    scale = resident_finish(vertex_blocks, lds);
    blocks = false;
  }
  if (begun) {
    out.final_cost = lm.cost;
    out.final_damping = lm.lambda;
  }
  if (t == 0) outs[blockIdx.x] = out;
}

__global__ __launch_bounds__(kPgBlock) void k_pg_resident(const PgResidentJob* __restrict__ jobs, PgResidentOut* outs, PgResidentIteration* records, int max_records,
                                                          unsigned stage_bytes) {
  extern __shared__ __attribute__((aligned(16))) double pg_stage[];
  __shared__ PgResidentLds lds;
  const PgResidentJob& record = jobs[blockIdx.x];
  PgGraph g;
  g.n = record.g.n;
  g.m = record.g.m;
  g.fixed = global_pointer_at(&record.g.fixed);
  g.from = global_pointer_at(&record.g.from);
  g.to = global_pointer_at(&record.g.to);
  g.Z = global_pointer_at(&record.g.Z);
  g.omega = global_pointer_at(&record.g.omega);
  g.delta = global_pointer_at(&record.g.delta);
  g.inc_start = global_pointer_at(&record.g.inc_start);
  g.inc = global_pointer_at(&record.g.inc);
  g.E = global_pointer_at(&record.g.E);
  g.V = global_pointer_at(&record.g.V);
  double* const pose_buffers[2] = {global_pointer_at(&record.poses[0]), global_pointer_at(&record.poses[1])};
  PgResidentJob job = {};                                           // (the scalars)
  job.cur = record.cur;
  job.any_free = record.any_free;
  job.max_iterations = record.max_iterations;
  job.cg_max_iterations = record.cg_max_iterations;
  job.cg_tolerance = record.cg_tolerance;
  job.min_relative_decrease = record.min_relative_decrease;
  job.initial_damping_scale = record.initial_damping_scale;
  // (a graph whose working set the launch's LDS does not hold runs from memory: the same result, more slowly)
  const bool staged = g.n > 0 && g.m > 0 && g.n <= kPgResidentMaxVertices && g.m <= kPgResidentMaxEdges && pg_resident_stage_bytes(g.n, g.m) <= size_t(stage_bytes);
  if (staged) resident_optimise<true>(g, pose_buffers, job, lds, pg_stage, outs, records, max_records);
  else resident_optimise<false>(g, pose_buffers, job, lds, pg_stage, outs, records, max_records);
}

int blocks_of(int count) { return (count + kPgBlock - 1) / kPgBlock; }

}  // namespace

void launch_pg_linearise(hipStream_t s, const PgGraph& g, const double* poses, bool with_blocks, double* cost_partials) {
  hipLaunchKernelGGL(k_pg_linearise, dim3(blocks_of(g.m)), dim3(kPgBlock), 0, s, g, poses, with_blocks ? 1 : 0, cost_partials);
}
void launch_pg_gather(hipStream_t s, const PgGraph& g, double* max_partials) {
  hipLaunchKernelGGL(k_pg_gather, dim3(blocks_of(g.n)), dim3(kPgBlock), 0, s, g, max_partials);
}
void launch_pg_cg_init(hipStream_t s, const PgGraph& g, PgCgState* st, double lambda, double* rz_partials) {
  hipLaunchKernelGGL(k_pg_cg_init, dim3(blocks_of(g.n)), dim3(kPgBlock), 0, s, g, st, lambda, rz_partials);
}
void launch_pg_multiply(hipStream_t s, const PgGraph& g, PgCgState* st, const double* rz_partials, double* pap_partials, int it, double lambda,
                        double tolerance, bool given) {
  hipLaunchKernelGGL(k_pg_multiply, dim3(blocks_of(g.n)), dim3(kPgBlock), 0, s, g, st, rz_partials, pap_partials, blocks_of(g.n), it, lambda, tolerance,
                     given ? 1 : 0);
}
void launch_pg_cg_update(hipStream_t s, const PgGraph& g, PgCgState* st, const double* pap_partials, double* rz_partials, int it) {
  hipLaunchKernelGGL(k_pg_cg_update, dim3(blocks_of(g.n)), dim3(kPgBlock), 0, s, g, st, pap_partials, rz_partials, blocks_of(g.n), it);
}
void launch_pg_apply(hipStream_t s, const PgGraph& g, double lambda, const double* poses, double* out, double* scale_partials) {
  hipLaunchKernelGGL(k_pg_apply, dim3(blocks_of(g.n)), dim3(kPgBlock), 0, s, g, lambda, poses, out, scale_partials);
}
void launch_pg_reduce(hipStream_t s, const double* a, int n_a, const double* b, int n_b, double* out) {
  hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(kPgBlock), 0, s, a, n_a, b, n_b, out);
}
void launch_pg_resident(hipStream_t s, const PgResidentJob* jobs, int n_graphs, PgResidentOut* outs, PgResidentIteration* records, int max_records,
                        size_t stage_bytes) {
  static bool raised[64] = {};                                      // the attribute is per device (callers hold their context's lock)
  int device = 0;
  if (stage_bytes > 32768 && hipGetDevice(&device) == hipSuccess && device >= 0 && device < 64 && !raised[device])
    raised[device] = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pg_resident), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         int(kPgResidentStageBytes)) == hipSuccess;
  if (stage_bytes > 32768 && !(device >= 0 && device < 64 && raised[device])) stage_bytes = 32768;     // (the limit stayed: fewer graphs are staged)
  if (stage_bytes > size_t(kPgResidentStageBytes)) stage_bytes = size_t(kPgResidentStageBytes);
  hipLaunchKernelGGL(k_pg_resident, dim3(n_graphs), dim3(kPgBlock), stage_bytes, s, jobs, outs, records, max_records, unsigned(stage_bytes));
}

}  // namespace dvo_hip
