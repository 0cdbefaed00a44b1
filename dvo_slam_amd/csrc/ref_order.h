// ref_order.h -- the algebra of option "ref_order" (SURVEY.md Q3, Q6, Q7), shared by the kernels of ref_order.hip and, compiled for
// the host, by the CPU tier (tests/emul/ref_order_emul.cpp).
//
// The reference's point list is the selected pixels in raster order (point_selection.cpp:119-140); a constraint's place in it is its
// RANK k among the valid constraints of the linearisation in raster order.  Two of its quirks depend on that rank:
//   Q6 (dense_tracking_impl.cpp:590-638): the scale sums pair the constraints (k, k + 1) and use the first residual of a pair twice,
//        S = sum_{k even} w_k r_k r_k^T + sum_{k odd} w_k r_{k-1} r_{k-1}^T   (an odd n: the last, even, rank pairs with nobody);
//   Q7 (dense_tracking_impl.cpp:406-425): the log-likelihood sum drops its last n mod 50 terms, n does not.
// A run of consecutive constraints -- a lane's pixels, a row, a block of rows -- is summarised by a RefOrderSeg that holds its terms
// for both parities of its first rank; two adjacent runs join into one (an associative join, ref_order_join), so rows are summed
// independently and combined by a scan of their counts.  Every sum is float64.
#pragma once

#include "pixel_math.h"

namespace dvo_hip {

struct RefOrderSeg {
  double se[3];        // the run's terms of S if its first constraint has an even rank (00, 01, 11)
  double so[3];        // ... an odd one
  double rr_last[3];   // r r^T of its last constraint
  double w_first;      // weight of its first constraint
  int c;               // constraints in the run
  int pad;
};

// what the combine writes per pair: n, S (the bracket of Q6, before the division by n - 3) and the dropped log-likelihood terms
struct RefOrderPair {
  double n;
  double S[3];
  double ll_tail;      // sum over the ranks [50 floor(n / 50), n) of log(1 + 0.2 r^T P r), P = ((S / (n - 3)) as float)^-1
  double pad[3];
};

// a reference plane {Zsel, I} of one frame level and the level's selection count N (Q3: the last selected pixel goes if N is odd), and
// where the edit keeps what it cleared -- {pixel index or -1, bits of its Zsel} -- so that it can be put back (in the frame's own
// block of selection counts: ref_order_saved_slot)
struct RefOrderPlane {
  float2* R;
  const int* count;
  int* saved;
  int npx;
  int pad;
};

// the frame's selection counters take one int per level at the start of a 256-byte block; behind them, from int 16 on, the Q3 slots
DVO_HD int* ref_order_saved_slot(int* sel_count, int level) { return sel_count + 16 + 2 * level; }

constexpr int kRefOrderLlGroup = 50;   // Q7: the reference adds its log-likelihood terms in groups of 50

DVO_HD RefOrderSeg ref_order_empty() {
  RefOrderSeg s;
  for (int i = 0; i < 3; ++i) s.se[i] = s.so[i] = s.rr_last[i] = 0.0;
  s.w_first = 0.0;
  s.c = 0;
  s.pad = 0;
  return s;
}

// one constraint with residual (r0, r1) and weight w
DVO_HD RefOrderSeg ref_order_leaf(float r0, float r1, float w) {
  RefOrderSeg s;
  const double a = double(r0), b = double(r1), wd = double(w);
  s.rr_last[0] = a * a; s.rr_last[1] = a * b; s.rr_last[2] = b * b;
  for (int i = 0; i < 3; ++i) {
    s.se[i] = wd * s.rr_last[i];
    s.so[i] = 0.0;
  }
  s.w_first = wd;
  s.c = 1;
  s.pad = 0;
  return s;
}

// the run `a` followed by the run `b`
DVO_HD RefOrderSeg ref_order_join(const RefOrderSeg& a, const RefOrderSeg& b) {
  if (a.c == 0) return b;
  if (b.c == 0) return a;
  const bool a_odd = (a.c & 1) != 0;
  RefOrderSeg s;
  for (int i = 0; i < 3; ++i) {
    const double cross = b.w_first * a.rr_last[i];     // the pair (a's last, b's first), if a's last has an even rank
    // first rank even: b begins on the parity of a.c, a's last rank (a.c - 1) is even iff a.c is odd
    s.se[i] = a.se[i] + (a_odd ? b.so[i] + cross : b.se[i]);
    // first rank odd: b begins on the parity of a.c + 1, a's last rank (a.c) is even iff a.c is even
    s.so[i] = a.so[i] + (a_odd ? b.se[i] : b.so[i] + cross);
    s.rr_last[i] = b.rr_last[i];
  }
  s.w_first = a.w_first;
  s.c = a.c + b.c;
  s.pad = 0;
  return s;
}

// the run `s` followed by one constraint: ref_order_join(s, ref_order_leaf(r0, r1, w)) bit for bit, without forming the leaf (the
// rows kernel's per-pixel step)
DVO_HD void ref_order_push(RefOrderSeg& s, float r0, float r1, float w) {
  const double a = double(r0), b = double(r1), wd = double(w);
  const double rr[3] = {a * a, a * b, b * b};
  const bool odd = (s.c & 1) != 0;                     // the new constraint's rank parity under an even first rank
  for (int i = 0; i < 3; ++i) {
    // even start: an even rank adds w r r^T, an odd one w r_prev r_prev^T; odd start: the other way round (the first constraint's
    // partner lies in the run before: rr_last is still zero then, and the join adds that term)
    s.se[i] += wd * (odd ? s.rr_last[i] : rr[i]);
    s.so[i] += wd * (odd ? rr[i] : s.rr_last[i]);
    s.rr_last[i] = rr[i];
  }
  if (s.c == 0) s.w_first = wd;
  s.c += 1;
}

// the weight of the sweeps (align_kernels.hip, k_residual_reduce): 1 on a level's first pass (Q11), else the t-distribution weight with
// the previous pass' precision, with the host CPU's reciprocal under option "ref_compat" (rcp_table non-null)
DVO_HD float ref_order_weight(bool first, const float* rcp_table, int rcp_shift, float r0, float r1, const float* P_prev) {
  if (first) return 1.0f;
  if (rcp_table) return 7.0f * rcp_like_the_host(rcp_table, rcp_shift, 5.0f + mahalanobis(r0, r1, P_prev));
  return tdist_weight(r0, r1, P_prev);
}

// the ranks [ref_order_ll_kept(n), n) are left out of the log-likelihood sum (Q7)
DVO_HD int ref_order_ll_kept(int n) { return (n / kRefOrderLlGroup) * kRefOrderLlGroup; }

}  // namespace dvo_hip
