// pose_graph.hip -- the kernels of the pose-graph optimiser (arithmetic and order of every sum: pose_graph.h; driver: capi_graph.inc).
// One lane per edge (k_pg_linearise) or per vertex (the others), kPgBlock of them per workgroup: a workgroup's LDS tree is one subtree
// of a scalar's adjacent-pair tree, and the kernel that needs the scalar walks the rest of the tree over the workgroups' partials
// itself -- every workgroup the same adds, so all of them reach the same decision.  No atomics, no grid-wide wait; a launch reads the
// stop word the launch BEFORE it wrote and returns at once when the solve has ended.
#include <hip/hip_runtime.h>

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

}  // namespace dvo_hip
