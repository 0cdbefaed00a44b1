// rectify.hip -- the rectifying pass of the ingest (lens.h; include/dvo_hip.h, dvo_hip_frames_set_lens): raw camera planes of n frames
// -> the tight float planes I / Z of level 0 of each frame, undistorted.  One launch on the build stream at the head of frames_build;
// the float ingest (DVO_HIP_PIXEL_F32 + DVO_HIP_DEPTH_F32, ingest_strips.hip / k_build_from_raw) then reads those planes where they
// lie and builds the role planes and the pyramid as for any float frame.
//
// The map is computed per lane in registers (lens_map: ~30 float operations and two divisions), never read from a table: the pass
// writes 8 B per pixel and reads 3-8 B, a tabulated map would add 8 B more.  A wavefront takes 64 consecutive pixels of one row, a
// workgroup of four wavefronts a 64 x 16 tile (rows w, w + 4, ...): the map is smooth, so the taps of a wavefront are the neighbours of
// its neighbours' -- two source rows, a few cache lines per load instruction -- and the rows of a tile meet again in the CU's cache.
// Raw planes are read with the non-temporal policy when the build stream's launches are ("stream_policy", like k_ingest_strips), the
// float planes written with it: they are read back once, by the ingest behind this pass, and must not displace the coarse levels.
// Templated on the caller's formats: CH = 0 grey8, 3 / 4 a colour format (byte order is a wave-uniform choice of weights), kChF32 a
// float image; ZF = float depth, else u16.  Pitches as the ingest takes them.  No LDS, no barriers, 256-thread workgroups.
#include "dispatch.h"
#include "global_ptr.h"
#include "launch.h"
#include "lens.h"

namespace dvo_hip {

namespace {

constexpr int kRectW = 64, kRectH = 16;

template <int CH, bool ZF, bool NT>
__global__ __launch_bounds__(256) void k_rectify(const RectifyPtrs* __restrict__ tbl, RectifyArgs a, int tiles_x, int tiles_y, int n_frames) {
#pragma clang fp contract(off)
  constexpr bool IF = CH == kChF32, COL = CH == 3 || CH == 4;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int per_frame = tiles_x * tiles_y, total = per_frame * n_frames;
  const GreyWeights gw = grey_weights(a.red_first != 0);
  const int w = a.w, h = a.h;
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    const int frame = i / per_frame, t = i - frame * per_frame;
    const int bx = t % tiles_x, by = t / tiles_x;
    const RectifyPtrs& f = tbl[frame];
    // (global_ptr.h: every plane pointer read once, as a pointer into the global address space; rows are addressed in bytes)
    const auto image = (Global<const uint8_t>)global_ptr(f.image);
    const auto depth = (Global<const uint8_t>)global_ptr(f.depth);
    const auto I0 = global_ptr(f.I), Z0 = global_ptr(f.Z);
    const size_t pitch = size_t(a.image_pitch), zpitch = size_t(a.depth_pitch);
    auto image_tap = [&](int x, int y) -> float {
      const auto p = image + size_t(y) * pitch + size_t(x) * (IF ? 4 : COL ? CH : 1);
      if (IF) return gld<NT>((Global<const float>)p);
      if (COL) return float(grey_of(gld<NT>(p), gld<NT>(p + 1), gld<NT>(p + 2), gw));
      return float(gld<NT>(p));
    };
    auto depth_tap = [&](int x, int y) -> float {
      const auto p = depth + size_t(y) * zpitch + size_t(x) * (ZF ? 4 : 2);
      if (ZF) return depth_of_f32(gld<NT>((Global<const float>)p), a.depth_scale);
      return depth_of_u16(gld<NT>((Global<const uint16_t>)p), a.depth_scale);
    };
    const int u = bx * kRectW + lx;
#pragma unroll
    for (int k = 0; k < kRectH / 4; ++k) {
      const int v = by * kRectH + ly + 4 * k;
      if (u >= w || v >= h) continue;
      float iv, zv;
      lens_rectify_pixel(a.map, w, h, u, v, a.rectify_depth != 0, image_tap, depth_tap, &iv, &zv);
      const size_t at = size_t(v) * w + u;
      gst<NT>(I0 + at, iv);
      gst<NT>(Z0 + at, zv);
    }
  }
}

}  // namespace

void launch_rectify(hipStream_t s, const RectifyPtrs* tbl, int n_frames, const RectifyArgs& a, int channels, bool depth_f32, int max_workgroups,
                    bool stream_nt) {
  const int tx = (a.w + kRectW - 1) / kRectW, ty = (a.h + kRectH - 1) / kRectH;
  const long long total = (long long)tx * ty * n_frames;
  const dim3 grid(capped_grid(total, max_workgroups)), block(256);
  with_value<kChF32, 3, 4, 0>(channels, [&](auto CH) {
    with_bool(depth_f32 || channels == kChF32, [&](auto ZF) {   // (a float image comes with float depth)
      with_bool(stream_nt, [&](auto NT) {
        constexpr int kCh = decltype(CH)::value;
        constexpr bool kZf = decltype(ZF)::value;
        if constexpr (kCh != kChF32 || kZf) k_rectify<kCh, kZf, decltype(NT)::value><<<grid, block, 0, s>>>(tbl, a, tx, ty, n_frames);
      });
    });
  });
}

}  // namespace dvo_hip
