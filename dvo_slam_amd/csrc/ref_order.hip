// ref_order.hip -- option "ref_order": the reference's rank-dependent quirks Q6 (paired scale sums) and Q7 (log-likelihood tail) on the
// launch path, and the plane edit behind Q3 (the last selected pixel of an odd selection).  The algebra is ref_order.h.
//
// Per Gauss-Newton pass, behind the sweep (which stores one residual pair per pixel, NaN where there is no constraint):
//   k_ref_order_rows     grid (row blocks, pairs): a wavefront per row reads the row's residual pairs once, recomputes the weights with
//                        the previous pass' precision exactly as the sweep does, and writes the row's RefOrderSeg;
//   k_ref_order_combine  a workgroup per pair: joins the rows' records in row order (their counts give every row's first rank), forms
//                        n, S and the precision, and sums the log-likelihood terms of the ranks Q7 drops (the last n mod 50) by walking
//                        the last rows.  k_loglik and the solver step take n, S and that sum from its RefOrderPair.
#include "align_common.h"
#include "ref_order.h"

namespace dvo_hip {

constexpr int kRefOrderRowsPerBlock = kWavesPerBlock;   // one row per wavefront
constexpr int kRefOrderSegLoads = 8;                    // residual pairs a lane loads per round of its run

__device__ __forceinline__ RefOrderSeg shfl_down_seg(const RefOrderSeg& s, int off) {
  RefOrderSeg o;
  for (int i = 0; i < 3; ++i) {
    o.se[i] = __shfl_down(s.se[i], off, 64);
    o.so[i] = __shfl_down(s.so[i], off, 64);
    o.rr_last[i] = __shfl_down(s.rr_last[i], off, 64);
  }
  o.w_first = __shfl_down(s.w_first, off, 64);
  o.c = __shfl_down(s.c, off, 64);
  o.pad = 0;
  return o;
}

__global__ __launch_bounds__(kBlock) void k_ref_order_rows(const LevelGeom g, const PairState* __restrict__ states, const float2* __restrict__ scratch,
                                                           RefOrderSeg* __restrict__ rows) {
  const int pair = pair_of_launch_index(g, blockIdx.y);
  if (pair < 0) return;
  const PairState& st = states[pair];
  if (!st.active || st.level != g.level) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int v = blockIdx.x * kRefOrderRowsPerBlock + wave;
  if (v >= g.h) return;                                      // (wavefront-uniform; no barrier below)
  float Pp[4];
  for (int i = 0; i < 4; ++i) Pp[i] = st.P_prev[i];
  const bool first = st.first != 0;
  // lane l owns the run of pixels [l K, (l + 1) K) of the row: its constraints are consecutive ranks, folded into the run's record
  // one by one (ref_order_push: the two parities' sums in registers), and the 64 runs are joined in lane order
  const int K = (g.w + 63) / 64;
  const int u0 = min(lane * K, g.w), u1 = min(u0 + K, g.w);
  const float2* row = scratch + size_t(pair) * g.w * g.h + size_t(v) * g.w;
  RefOrderSeg s = ref_order_empty();
  for (int u = u0; u < u1; u += kRefOrderSegLoads) {
    float2 r[kRefOrderSegLoads];
#pragma unroll
    for (int k = 0; k < kRefOrderSegLoads; ++k) r[k] = row[min(u + k, u1 - 1)];
#pragma unroll
    for (int k = 0; k < kRefOrderSegLoads; ++k)
      if (u + k < u1 && r[k].x == r[k].x)
        ref_order_push(s, r[k].x, r[k].y, ref_order_weight(first, g.rcp_table, g.rcp_shift, r[k].x, r[k].y, Pp));
  }
  // the 64 runs joined in lane order: lane l ends up holding lanes [l, l + 2 off) wherever l is a multiple of 2 off
  for (int off = 1; off < 64; off <<= 1) {
    const RefOrderSeg o = shfl_down_seg(s, off);
    if ((lane & (2 * off - 1)) == 0) s = ref_order_join(s, o);
  }
  if (lane == 0) rows[size_t(pair) * g.h + v] = s;
}

__global__ __launch_bounds__(kBlock) void k_ref_order_combine(const LevelGeom g, const PairState* __restrict__ states, const float2* __restrict__ scratch,
                                                              const RefOrderSeg* __restrict__ rows, RefOrderPair* __restrict__ out) {
  const int pair = pair_of_launch_index(g, blockIdx.x);
  if (pair < 0) return;
  if (!states[pair].active || states[pair].level != g.level) return;
  __shared__ RefOrderSeg seg[kBlock];
  __shared__ int first_tail_row, first_tail_rank;
  const int t = threadIdx.x;
  const RefOrderSeg* mine = rows + size_t(pair) * g.h;
  // thread t joins the rows [t R, (t + 1) R)
  const int R = (g.h + kBlock - 1) / kBlock;
  const int r0 = min(t * R, g.h), r1 = min(r0 + R, g.h);
  RefOrderSeg s = ref_order_empty();
  for (int r = r0; r < r1; ++r) s = ref_order_join(s, mine[r]);
  seg[t] = s;
  if (t == 0) first_tail_row = g.h;
  __syncthreads();
  // the runs' first ranks: an exclusive scan of the counts (every thread reads the counts before it; kBlock ints)
  int start = 0;
  for (int k = 0; k < t; ++k) start += seg[k].c;
  int n = start + s.c;
  for (int k = t + 1; k < kBlock; ++k) n += seg[k].c;
  const int kept = ref_order_ll_kept(n);
  // the row holding rank `kept` (the first whose constraints Q7 drops): in the run that covers that rank
  if (kept < n && start <= kept && kept < start + s.c) {
    int at = start;
    for (int r = r0; r < r1; ++r) {
      const int c = mine[r].c;
      if (at + c > kept) {
        first_tail_row = r;
        first_tail_rank = at;
        break;
      }
      at += c;
    }
  }
  __syncthreads();
  // the runs joined in thread order
  for (int off = 1; off < kBlock; off <<= 1) {
    if ((t & (2 * off - 1)) == 0) seg[t] = ref_order_join(seg[t], seg[t + off]);
    __syncthreads();
  }
  const RefOrderSeg total = seg[0];
  float C[3], P[4];
  const double d = double(total.c) - 3.0;
  scale_to_precision(total.se[0] / d, total.se[1] / d, total.se[2] / d, C, P);   // (the step's and k_loglik's P, from the same n and S)
  if (t >= 64) return;
  // wavefront 0: the dropped terms -- every constraint of rank >= kept, rows first_tail_row .. in order (k_loglik adds them only
  // where n >= 6; so does this)
  const int lane = t;
  double tail = 0.0;
  if (total.c >= 6) {
    int rank = first_tail_rank;
    for (int v = first_tail_row; v < g.h && rank < total.c; ++v) {
      const int c = mine[v].c;
      if (c == 0) continue;
      const float2* row = scratch + size_t(pair) * g.w * g.h + size_t(v) * g.w;
      int before = 0;                                        // constraints of the row left of this 64-pixel chunk
      for (int u0 = 0; u0 < g.w; u0 += 64) {
        const int u = u0 + lane;
        const float2 r = u < g.w ? row[u] : make_float2(__builtin_nanf(""), 0.0f);
        const bool valid = r.x == r.x;
        const unsigned long long ballot = __ballot(valid);
        const int k = rank + before + __popcll(ballot & ((1ull << lane) - 1ull));
        if (valid && k >= kept) tail += log1p(0.2 * double(mahalanobis(r.x, r.y, P)));
        before += __popcll(ballot);
      }
      rank += c;
    }
  }
  tail = wave_sum_double(tail);
  if (lane == 0) {
    RefOrderPair o;
    o.n = double(total.c);
    for (int i = 0; i < 3; ++i) o.S[i] = total.se[i];
    o.ll_tail = tail;
    o.pad[0] = o.pad[1] = o.pad[2] = 0.0;
    out[pair] = o;
  }
}

void launch_ref_order(hipStream_t s, const LevelGeom& g, const PairState* states, int n_pairs, const float2* scratch, RefOrderSeg* rows, RefOrderPair* out) {
  k_ref_order_rows<<<dim3((g.h + kRefOrderRowsPerBlock - 1) / kRefOrderRowsPerBlock, n_pairs), dim3(kBlock), 0, s>>>(g, states, scratch, rows);
  k_ref_order_combine<<<dim3(n_pairs), dim3(kBlock), 0, s>>>(g, states, scratch, rows, out);
}

// Q3: a reference plane {Zsel, I} whose level selected an odd number N of pixels (the frame's counter) loses its last selected pixel in
// raster order (Zsel = NaN): it gives no constraint, no scale term, no log-likelihood term, no row of the normal equations.  One
// workgroup per plane, scanning back from the end in 1024-pixel chunks; the pixel and its Zsel go to the plane's slot
// (k_ref_order_restore puts them back when the frame is next matched without the option).
constexpr int kDropThreads = 1024;

__global__ __launch_bounds__(kDropThreads) void k_ref_order_drop_last(const RefOrderPlane* __restrict__ planes) {
  const RefOrderPlane p = planes[blockIdx.x];
  if ((*p.count & 1) == 0) {
    if (threadIdx.x == 0) p.saved[0] = -1;
    return;
  }
  __shared__ int last;
  if (threadIdx.x == 0) last = -1;
  __syncthreads();
  for (int base = p.npx - kDropThreads; base > -kDropThreads; base -= kDropThreads) {
    const int i = base + int(threadIdx.x);
    if (i >= 0 && p.R[i].x == p.R[i].x) atomicMax(&last, i);
    __syncthreads();
    if (last >= 0) break;                                    // (uniform: read after the barrier, written before the next one)
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    p.saved[0] = last;
    if (last >= 0) {
      p.saved[1] = __float_as_int(p.R[last].x);
      p.R[last].x = __builtin_nanf("");
    }
  }
}

__global__ void k_ref_order_restore(const RefOrderPlane* __restrict__ planes, int n_planes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_planes) return;
  const RefOrderPlane p = planes[i];
  const int at = p.saved[0];
  if (at >= 0 && at < p.npx) p.R[at].x = __int_as_float(p.saved[1]);
  p.saved[0] = -1;
}

void launch_ref_order_drop_last(hipStream_t s, const RefOrderPlane* planes, int n_planes) {
  if (n_planes > 0) k_ref_order_drop_last<<<dim3(n_planes), dim3(kDropThreads), 0, s>>>(planes);
}

void launch_ref_order_restore(hipStream_t s, const RefOrderPlane* planes, int n_planes) {
  if (n_planes > 0) k_ref_order_restore<<<dim3((n_planes + 63) / 64), dim3(64), 0, s>>>(planes, n_planes);
}

}  // namespace dvo_hip
