// frame_warp.hip -- frames warped under a pose on the device (frame_warp.h; include/dvo_hip.h, dvo_hip_frames_warp_inverse and
// dvo_hip_frames_warp_forward).  Both kernels read the frames through the frame table of the keyframe-map launches (MapFrame: the {I, Z}
// pairs of the level, 8 B apart in plane C or 16 B apart in the taps A, the level's K, and the item's transform as MapFrame::pose).
//
// k_warp_inverse: a lane per raster pixel, a wavefront 64 consecutive pixels of the raster; the item is the grid's y, walked where there
// are more items than the grid is high; the grid's x strides over the item's pixels.  A lane loads its own Z_R (with the difference plane
// the whole pair {I_R, Z_R}: one 8-byte load), and -- where the projection lands inside the sampled image -- the four {I_S, Z_S} pairs of
// its taps with plain cached 8-byte loads: neighbouring lanes hit neighbouring taps under any small motion, so the taps of a wavefront
// lie in a few cache lines of two rows; no window is staged in LDS.  Two or three coalesced 4-byte stores per lane.
// k_warp_forward: a lane per source pixel, the same grid.  One 8-byte load of the pair, the projection in registers, and the footprint loop
// -- constant bounds kWarpMaxFootprint with an early break, as k_map_render's -- issues one 64-bit vector memory atomic per covered
// pixel (unsigned minimum, relaxed, agent scope) whose return value is not used.  Nothing waits or retries; the minimum over integers
// does not depend on the order of arrival.  The z-buffers are the context's render scratch: filled by k_render_fill and resolved by
// k_render_resolve<false> (map_render.hip) on the same stream, so warps and map renders are ordered with each other.
// No LDS, no barriers, 256-thread workgroups.
#include "global_ptr.h"
#include "launch.h"
#include "frame_warp.h"

namespace dvo_hip {

namespace {

__global__ __launch_bounds__(256) void k_warp_inverse(const MapFrame* __restrict__ tbl, const WarpPlanes* __restrict__ outs, int n, float margin) {
#pragma clang fp contract(off)
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (int item = int(blockIdx.y); item < n; item += int(gridDim.y)) {
    const MapFrame& R = tbl[2 * item];                           // (item < n: entries 2 item and 2 item + 1 lie inside the table of 2n + 1)
    const MapFrame& S = tbl[2 * item + 1];
    const int w = R.w, h = R.h;                                  // (S.w == w and S.h == h: checked before the launch)
    const long long pixels = (long long)w * h;
    const size_t rs = size_t(R.stride), ss = size_t(S.stride);
    const auto Rp = (Global<const float>)global_ptr(R.iz);
    const auto Sp = (Global<const float>)global_ptr(S.iz);
    const WarpPlanes o = outs[item];                             // (item < n: inside the table of planes)
    const auto Iout = (Global<float>)global_ptr(o.I);
    const auto Zout = (Global<float>)global_ptr(o.Z);
    const auto Dout = (Global<float>)global_ptr(o.D);
    const bool difference = o.D != nullptr;                      // (uniform over the item)
    const MapPose T = R.pose;
    const float KR[4] = {R.K[0], R.K[1], R.K[2], R.K[3]}, KS[4] = {S.K[0], S.K[1], S.K[2], S.K[3]};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {   // (i < w * h: inside R's level and the item's planes)
      float IR = 0.0f, z;
      if (difference) {
        const GlobalF32x2 iz = *(Global<const GlobalF32x2>)(Rp + size_t(i) * rs);
        IR = iz.x;
        z = iz.y;
      } else {
        z = Rp[size_t(i) * rs + 1];
      }
      // the taps: warp_inverse_pixel asks only for 0 <= xx <= w - 1 and 0 <= yy <= h - 1, so yy * w + xx < w * h: inside S's level
      const auto taps = [&](int xx, int yy) {
        const GlobalF32x2 t = *(Global<const GlobalF32x2>)(Sp + (size_t(yy) * size_t(w) + size_t(xx)) * ss);
        return WarpTap{t.x, t.y};
      };
      float Iw, Zw;
      warp_inverse_pixel(T, KR, KS, w, h, int(i % w), int(i / w), z, margin, taps, &Iw, &Zw);
      Iout[i] = Iw;
      Zout[i] = Zw;
      if (difference) Dout[i] = warp_difference(Iw, IR);
    }
  }
}

__global__ __launch_bounds__(256) void k_warp_forward(const MapFrame* __restrict__ tbl, int n, long long pixels, int mode, float min_depth,
                                                      float max_depth, unsigned long long* __restrict__ zbuf) {
#pragma clang fp contract(off)
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (int item = int(blockIdx.y); item < n; item += int(gridDim.y)) {
    const MapFrame& f = tbl[item];                               // (item < n: inside the table)
    const int w = f.w, h = f.h;                                  // (w * h == pixels: checked before the launch)
    unsigned long long* plane = zbuf + (size_t)item * (size_t)pixels;   // (item < n: the item's own pixels elements of the n * pixels)
    const size_t fs = size_t(f.stride);
    const auto Fp = (Global<const float>)global_ptr(f.iz);
    const MapPose T = f.pose;
    const float K[4] = {f.K[0], f.K[1], f.K[2], f.K[3]};
    const WarpSplat s = warp_splat_prepare(T, K);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {   // (i < w * h: inside the frame's level)
      const GlobalF32x2 iz = *(Global<const GlobalF32x2>)(Fp + size_t(i) * fs);
      WarpFootprint fp;
      if (!warp_forward_pixel(T, s, K, w, h, mode, min_depth, max_depth, int(i % w), int(i / w), iz.x, iz.y, &fp)) continue;
      // fp lies inside the image (warp_axis clips, NEAREST tests): 0 <= u0 < u1 <= w, 0 <= v0 < v1 <= h, at most kWarpMaxFootprint a side
      const int nu = fp.u1 - fp.u0, nv = fp.v1 - fp.v0;
      for (int dy = 0; dy < kWarpMaxFootprint; ++dy) {
        if (dy >= nv) break;
        unsigned long long* row = plane + (size_t)(fp.v0 + dy) * (size_t)w + (size_t)fp.u0;
        for (int dx = 0; dx < kWarpMaxFootprint; ++dx) {
          if (dx >= nu) break;
          (void)__hip_atomic_fetch_min(row + dx, (unsigned long long)fp.value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
}

// x: grid-stride over the pixels of one item, y: the items (at most 1024 rows; the kernels walk the rest)
dim3 warp_grid(long long pixels, int n) {
  long long blocks = (pixels + 255) / 256;
  const int rows = n < 1024 ? n : 1024;
  const long long cap = 8192 / rows > 64 ? 8192 / rows : 64;
  blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
  return dim3(unsigned(blocks), unsigned(rows));
}

}  // namespace

void launch_warp_inverse(hipStream_t s, const MapFrame* tbl, const WarpPlanes* outs, int n, long long max_pixels, float margin) {
  k_warp_inverse<<<warp_grid(max_pixels, n), dim3(256), 0, s>>>(tbl, outs, n, margin);
}

void launch_warp_forward(hipStream_t s, const MapFrame* tbl, int n, long long pixels, int mode, float min_depth, float max_depth,
                         unsigned long long* zbuf) {
  k_warp_forward<<<warp_grid(pixels, n), dim3(256), 0, s>>>(tbl, n, pixels, mode, min_depth, max_depth, zbuf);
}

}  // namespace dvo_hip
