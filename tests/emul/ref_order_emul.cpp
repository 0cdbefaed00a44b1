// Host build of the algebra of option "ref_order" (dvo_slam_amd/csrc/ref_order.h) in the order ref_order.hip joins it: per row 64
// lane runs of ceil(w / 64) pixels, joined as a tree in lane order; the rows in 256 runs of ceil(h / 256), joined as a tree.  Test-only
// (tests/test_ref_order.py), never linked into the library.
#include <xmmintrin.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../dvo_slam_amd/csrc/ref_order.h"

using namespace dvo_hip;

namespace {

RefOrderSeg tree(std::vector<RefOrderSeg> v) {
  for (size_t off = 1; off < v.size(); off <<= 1)
    for (size_t t = 0; t + off < v.size(); t += 2 * off) v[t] = ref_order_join(v[t], v[t + off]);
  return v[0];
}

float weight(bool first, bool host_rcp, float r0, float r1, const float* P) {
  if (!first && host_rcp) return 7.0f * _mm_cvtss_f32(_mm_rcp_ss(_mm_set_ss(5.0f + mahalanobis(r0, r1, P))));   // (option "ref_compat")
  return ref_order_weight(first, nullptr, 0, r0, r1, P);
}

}  // namespace

extern "C" {

// res: h x w residual pairs, NaN in the first component where there is no constraint.  host_rcp: the weights with this CPU's _mm_rcp_ss
// (what the table of option "ref_compat" reproduces).  out: n, S00, S01, S11, the log-likelihood sum over all constraints, the dropped
// tail (Q7), -ll as the solver step forms it; C (3) and P (4) as float.
void ref_order_emul(const float* res, int w, int h, const float* P_prev, int first, int host_rcp, double* out, float* C, float* P) {
  const int K = (w + 63) / 64;
  std::vector<RefOrderSeg> rows(h);
  for (int v = 0; v < h; ++v) {
    std::vector<RefOrderSeg> lanes(64, ref_order_empty());
    for (int l = 0; l < 64; ++l)
      for (int u = std::min(l * K, w); u < std::min(l * K + K, w); ++u) {
        const float r0 = res[(size_t(v) * w + u) * 2], r1 = res[(size_t(v) * w + u) * 2 + 1];
        if (r0 == r0) ref_order_push(lanes[l], r0, r1, weight(first != 0, host_rcp != 0, r0, r1, P_prev));
      }
    rows[v] = tree(lanes);
  }
  const int R = (h + 255) / 256;
  std::vector<RefOrderSeg> runs(256, ref_order_empty());
  for (int t = 0; t < 256; ++t)
    for (int r = std::min(t * R, h); r < std::min(t * R + R, h); ++r) runs[t] = ref_order_join(runs[t], rows[r]);
  const RefOrderSeg total = tree(runs);
  const double d = double(total.c) - 3.0;
  scale_to_precision(total.se[0] / d, total.se[1] / d, total.se[2] / d, C, P);
  const int kept = ref_order_ll_kept(total.c);
  double all = 0.0, tail = 0.0;
  int k = 0;
  for (int i = 0; i < w * h; ++i) {
    const float r0 = res[2 * i], r1 = res[2 * i + 1];
    if (r0 != r0) continue;
    const double t = std::log1p(0.2 * double(mahalanobis(r0, r1, P)));
    all += t;
    if (k++ >= kept) tail += t;
  }
  if (total.c < 6) all = tail = 0.0;
  const double det = double(P[0]) * double(P[3]) - double(P[1]) * double(P[2]);
  out[0] = total.c;
  for (int i = 0; i < 3; ++i) out[1 + i] = total.se[i];
  out[4] = all;
  out[5] = tail;
  out[6] = -double(float(0.5 * double(total.c) * std::log(det) - 3.5 * (all - tail)));
}

}  // extern "C"
