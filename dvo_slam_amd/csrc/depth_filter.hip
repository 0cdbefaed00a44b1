// depth_filter.hip -- the filter pass of the ingest (depth_filter.h; include/dvo_hip.h, dvo_hip_frames_set_depth_filter): the depth planes
// of n frames -> one tight float plane per frame (the frame's filter plane), flying pixels and hole borders rejected, noise smoothed.
// One launch on the build stream, the LAST stage of frames_build; the float-depth ingest (DVO_HIP_DEPTH_F32, ingest_strips.hip /
// k_build_from_raw) then reads that plane.  Never in place: the source may be the frame's own level-0 plane Z (behind a rig or a lens),
// and a stencil must not write what its neighbours still read.
//
// A workgroup of four wavefronts takes a 64 x 16 tile and stages it with a halo of H = max(radius, edge_radius, hole_radius) <= 3 in
// LDS, converted at load (depth_of_u16 / depth_of_f32): a valid depth as itself, an in-image hole as the quiet NaN, a cell outside the
// image as -1 ("no tap", distinct from "hole": the image border erodes nothing).  The range table wr (64 floats) goes to LDS too; the
// spatial table ws is read from the kernel argument with compile-time indices (scalar loads).  A lane owns a RUN of four pixels of one
// column: it walks the 4 + 2 H rows of its window strip once, holds a row's 2 H + 1 taps in registers and feeds them to every pixel of
// the run that the row belongs to -- (4 + 2 H)(2 H + 1) / 4 LDS words per pixel instead of (2 H + 1)^2, 17.5 against 49 at H = 3.  For
// each pixel the taps still arrive row-major over dy, dx, the order depth_filter.h states, so the sums are the yardstick's bit for bit.
// Lanes of a wavefront read consecutive LDS words (rows of 64 + 2 H floats): no bank conflicts; the table lookups hit 64 words.
// Templated on R = radius, E = max(edge_radius, hole_radius) (the two radii themselves are wave-uniform run-time values), ZF = float
// depth, else u16, NT = the source is read with the non-temporal policy ("stream_policy"); the plane is written with it.
#include "dispatch.h"
#include "global_ptr.h"
#include "launch.h"
#include "depth_filter.h"

namespace dvo_hip {

namespace {

constexpr int kFiltW = 64, kFiltH = 16, kFiltRun = 4;
constexpr float kFiltNoTap = -1.0f;

template <int R, int E, bool ZF, bool NT>
__global__ __launch_bounds__(256) void k_depth_filter(const DepthFilterPtrs* __restrict__ tbl, DepthFilterArgs a, int tiles_x, int tiles_y, int n_frames) {
#pragma clang fp contract(off)
  constexpr int H = R > E ? R : E;
  constexpr int LW = kFiltW + 2 * H, LH = kFiltH + 2 * H;
  constexpr int M = kDepthFilterMaxRadius;
  __shared__ float tile[LH * LW];
  __shared__ float wr[kDepthFilterBins];
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int per_frame = tiles_x * tiles_y, total = per_frame * n_frames;
  const int w = a.w, h = a.h;
  const int er = a.P.edge_radius, hr = a.P.hole_radius;
  const float hole = depth_filter_hole();
  if (threadIdx.x < kDepthFilterBins) wr[threadIdx.x] = a.P.wr[threadIdx.x];
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    const int frame = i / per_frame, t = i - frame * per_frame;
    const int bx = t % tiles_x, by = t / tiles_x;
    const DepthFilterPtrs& f = tbl[frame];
    const auto depth = (Global<const uint8_t>)global_ptr(f.depth);
    const auto out = global_ptr(f.out);
    const size_t zpitch = size_t(a.depth_pitch);
    __syncthreads();                                         // (the previous tile has been read)
    for (int c = threadIdx.x; c < LH * LW; c += 256) {
      const int cy = c / LW, cx = c - cy * LW;
      const int gx = bx * kFiltW - H + cx, gy = by * kFiltH - H + cy;
      float z = kFiltNoTap;
      if (gx >= 0 && gy >= 0 && gx < w && gy < h) {
        const auto p = depth + size_t(gy) * zpitch + size_t(gx) * (ZF ? 4 : 2);
        if constexpr (ZF) z = depth_of_f32(gld<NT>((Global<const float>)p), a.depth_scale);
        else z = depth_of_u16(gld<NT>((Global<const uint16_t>)p), a.depth_scale);
        if (!depth_filter_valid(z)) z = hole;
      }
      tile[c] = z;
    }
    __syncthreads();
    const int u = bx * kFiltW + lx, v0 = by * kFiltH + ly * kFiltRun;
    float zc[kFiltRun], tau[kFiltRun], inv[kFiltRun], acc_w[kFiltRun], acc_d[kFiltRun];
    bool rejected[kFiltRun];
#pragma unroll
    for (int p = 0; p < kFiltRun; ++p) {
      zc[p] = tile[(ly * kFiltRun + p + H) * LW + lx + H];
      tau[p] = depth_filter_tau(a.P, zc[p]);
      inv[p] = depth_filter_inv(a.P, zc[p]);
      acc_w[p] = 0.0f;
      acc_d[p] = 0.0f;
      rejected[p] = false;
    }
    if constexpr (H > 0) {
#pragma unroll
      for (int r = 0; r < kFiltRun + 2 * H; ++r) {
        float tap[2 * H + 1];
#pragma unroll
        for (int k = 0; k < 2 * H + 1; ++k) tap[k] = tile[(ly * kFiltRun + r) * LW + lx + k];
#pragma unroll
        for (int p = 0; p < kFiltRun; ++p) {
          const int dy = r - p - H;
          if (dy < -H || dy > H) continue;
#pragma unroll
          for (int dx = -H; dx <= H; ++dx) {
            const float zn = tap[dx + H];
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const int cheb = ax > ay ? ax : ay;
            if (cheb <= E && cheb > 0) {
              if (zn != zn) {
                if (cheb <= hr) rejected[p] = true;
              } else if (zn > 0.0f && cheb <= er && depth_filter_edge(zn, zc[p], tau[p])) {
                rejected[p] = true;
              }
            }
            if (cheb <= R && zn > 0.0f) depth_filter_tap(zn, zc[p], inv[p], a.P.ws[dy + M][dx + M], wr, &acc_w[p], &acc_d[p]);
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < kFiltRun; ++p) {
      const int v = v0 + p;
      if (u >= w || v >= h) continue;
      float o = hole;
      if (depth_filter_valid(zc[p]) && !rejected[p]) o = R == 0 ? zc[p] : depth_filter_result(zc[p], acc_w[p], acc_d[p]);
      gst<NT>(out + (size_t(v) * w + u), o);
    }
  }
}

}  // namespace

void launch_depth_filter(hipStream_t s, const DepthFilterPtrs* tbl, int n_frames, const DepthFilterArgs& a, bool depth_f32, int max_workgroups,
                         bool stream_nt) {
  const int tx = (a.w + kFiltW - 1) / kFiltW, ty = (a.h + kFiltH - 1) / kFiltH;
  const long long total = (long long)tx * ty * n_frames;
  const dim3 grid(capped_grid(total, max_workgroups)), block(256);
  const int reject = a.P.edge_radius > a.P.hole_radius ? a.P.edge_radius : a.P.hole_radius;
  with_value<0, 1, 2, 3>(a.P.radius, [&](auto R) {
    with_value<0, 1, 2>(reject, [&](auto E) {
      with_bool(depth_f32, [&](auto ZF) {
        with_bool(stream_nt, [&](auto NT) {
          k_depth_filter<decltype(R)::value, decltype(E)::value, decltype(ZF)::value, decltype(NT)::value><<<grid, block, 0, s>>>(tbl, a, tx, ty,
                                                                                                                                 n_frames);
        });
      });
    });
  });
}

}  // namespace dvo_hip
