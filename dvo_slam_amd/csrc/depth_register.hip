// depth_register.hip -- the register pass of the ingest (depth_rig.h; include/dvo_hip.h, dvo_hip_frames_set_depth_rig): the depth sensor's
// planes of n frames -> the tight float plane Z of level 0 of each frame, seen from the colour camera.  Two launches on the build stream
// at the head of frames_build, ahead of the lens pass; the float-depth ingest (DVO_HIP_DEPTH_F32, ingest_strips.hip / k_build_from_raw)
// then reads Z where it lies.
//
// k_depth_fill stores the hole pattern (kDepthRigHole, a quiet NaN above every finite float as an unsigned) into every z-buffer: 16 B per
// lane, grid-stride over frames x quads, and a scalar tail for planes whose pixel count is no multiple of 4 (odd widths).
// k_depth_register is the forward scatter: a wavefront takes 64 consecutive SOURCE pixels of one row, a workgroup of four wavefronts a
// 64 x 16 tile (rows w, w + 4, ...), as in rectify.hip.  The map is smooth, so the 64 targets of a wavefront fall into one or two lines
// of the z-buffer, and the rows of a tile meet again in the cache.  The minimum is a vector memory atomic whose return value is not
// used (unsigned minimum on the float's bits, relaxed, agent scope), at the DEFAULT cache policy: the ingest reads the plane back at
// once.  Source planes are read with the non-temporal policy when the build stream's launches are ("stream_policy").  The result does
// not depend on the order of the atomics.  ZF = float depth, else u16.  No LDS, no barriers, 256-thread workgroups.
#include "dispatch.h"
#include "global_ptr.h"
#include "launch.h"
#include "depth_rig.h"

namespace dvo_hip {

namespace {

constexpr int kRegW = 64, kRegH = 16;
typedef unsigned GlobalU32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_depth_fill(const DepthRigPtrs* __restrict__ tbl, int n_frames, int pixels) {
  const int quads = pixels >> 2, tail = pixels & 3;
  const long long total = (long long)quads * n_frames;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const GlobalU32x4 hole = {kDepthRigHole, kDepthRigHole, kDepthRigHole, kDepthRigHole};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int frame = int(i / quads), q = int(i - (long long)frame * quads);
    const auto Z = (Global<GlobalU32x4>)global_ptr(tbl[frame].Z);   // (planes are 256-byte aligned: frame_alloc)
    Z[q] = hole;
  }
  // the tail: the last pixels % 4 elements of every plane, one lane each
  const long long tails = (long long)tail * n_frames;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < tails; i += stride) {
    const int frame = int(i / tail), k = int(i - (long long)frame * tail);
    const auto Z = (Global<unsigned>)global_ptr(tbl[frame].Z);
    Z[size_t(quads) * 4 + k] = kDepthRigHole;
  }
}

template <bool ZF, bool NT>
__global__ __launch_bounds__(256) void k_depth_register(const DepthRigPtrs* __restrict__ tbl, DepthRigArgs a, int tiles_x, int tiles_y, int n_frames) {
#pragma clang fp contract(off)
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int per_frame = tiles_x * tiles_y, total = per_frame * n_frames;
  const int w = a.w, h = a.h;
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    const int frame = i / per_frame, t = i - frame * per_frame;
    const int bx = t % tiles_x, by = t / tiles_x;
    const DepthRigPtrs& f = tbl[frame];
    const auto depth = (Global<const uint8_t>)global_ptr(f.depth);
    const auto Z0 = (Global<unsigned>)global_ptr(f.Z);
    const size_t zpitch = size_t(a.depth_pitch);
    const int u = bx * kRegW + lx;
#pragma unroll
    for (int k = 0; k < kRegH / 4; ++k) {
      const int v = by * kRegH + ly + 4 * k;
      if (u >= w || v >= h) continue;
      const auto p = depth + size_t(v) * zpitch + size_t(u) * (ZF ? 4 : 2);
      float z;
      if constexpr (ZF) z = depth_of_f32(gld<NT>((Global<const float>)p), a.depth_scale);
      else z = depth_of_u16(gld<NT>((Global<const uint16_t>)p), a.depth_scale);
      int at;
      uint32_t bits;
      if (!depth_rig_project(a.map, w, h, u, v, z, &at, &bits)) continue;   // (at lies inside the plane: xi, yi are clamped)
      (void)__hip_atomic_fetch_min(Z0 + at, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

void launch_depth_register(hipStream_t s, const DepthRigPtrs* tbl, int n_frames, const DepthRigArgs& a, bool depth_f32, int max_workgroups,
                           bool stream_nt) {
  const int pixels = a.w * a.h;
  const long long fill_items = ((long long)(pixels >> 2) * n_frames + 255) / 256;
  const long long fill_blocks = fill_items < 1 ? 1 : fill_items;
  const dim3 block(256);
  k_depth_fill<<<dim3(capped_grid(fill_blocks, max_workgroups)), block, 0, s>>>(tbl, n_frames, pixels);
  const int tx = (a.w + kRegW - 1) / kRegW, ty = (a.h + kRegH - 1) / kRegH;
  const long long total = (long long)tx * ty * n_frames;
  const dim3 grid(capped_grid(total, max_workgroups));
  with_bool(depth_f32, [&](auto ZF) {
    with_bool(stream_nt, [&](auto NT) {
      k_depth_register<decltype(ZF)::value, decltype(NT)::value><<<grid, block, 0, s>>>(tbl, a, tx, ty, n_frames);
    });
  });
}

}  // namespace dvo_hip
