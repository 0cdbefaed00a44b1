// pyramid_kernels.hip -- device-resident image data model, batched over frames.
//
// What the reference does on the host per frame and per level
//   ingest        dvo_benchmark/src/benchmark_slam.cpp:46-93, dvo_core/src/core/surface_pyramid.cpp:65-105
//   pyr-down      dvo_core/src/core/rgbd_image.cpp:38-55 (2x2 mean), :127-139 (depth subsample), :156-172
//   derivatives   dvo_core/src/core/rgbd_image.cpp:419-489, rgbd_image_sse.cpp:241-284
//   accel struct  dvo_core/src/core/rgbd_image.cpp:534-543   (8 interleaved float channels, 32 B/pixel)
//   selection     dvo_core/src/core/point_selection.cpp:89-152, point_selection.h:49-67
// is done here on the GPU, one launch per pyramid level for a whole batch of frames (blockIdx.z = frame),
// so a frame upload is two raw planes and every derived plane stays in HBM.  The per-pixel arithmetic (mean, subsample, differences,
// predicate) is image_model.h's; the kernels here only lay it out.  Layout (all float32):
//   I, Z          planar, 4 B/pixel each (pyr-down and derivative source; built when the frame is ingested)
//   A             float4 {I, Z, Idx, Idy}  current-side sampling plane, one 16-B tap per bilinear corner
//   B             float2 {Zdx, Zdy}        current-side sampling plane,  8-B tap
//   R             float4 {Zsel, I, Idx, Idy} reference-side stream; Zsel = NaN where the selection
//                 predicate rejects the pixel, so the reduce kernel needs no separate mask or list
// These are bandwidth-trivial elementwise kernels; they are written for coalescing only.
#include "colour.h"
#include "dispatch.h"
#include "global_ptr.h"
#include "image_model.h"
#include "launch.h"
#include "selection.h"

namespace dvo_hip {

// Work distribution of the frame-build kernels: a linear index over (tile, frame) walked with a grid stride.  Launched with
// one workgroup per tile this is the plain one-tile-per-workgroup kernel; launched with FEWER workgroups (option
// "build_workgroups") the same kernel becomes a background job that leaves most wave slots of every CU free, so the
// short dependent kernels of an alignment running concurrently on the other stream are dispatched at once instead of queueing
// behind tens of thousands of elementwise workgroups.
template <typename Body>
__device__ __forceinline__ void for_each_tile(int tiles_x, int tiles_y, int n_frames, Body body) {
  const int per_frame = tiles_x * tiles_y, total = per_frame * n_frames;
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    const int frame = i / per_frame, t = i - frame * per_frame;
    body(t % tiles_x, t / tiles_x, frame);
  }
}

// The selection count of a tile of a 4-wavefront workgroup: `count` is wave-uniform; one LDS word per wavefront, added in a fixed order,
// ONE atomic per tile (one per wavefront-row serialised a whole kernel on 128 addresses).  Holds one barrier; the caller puts another
// between this and its next call (the words are rewritten).  The counter must have been zeroed on the stream before.
__device__ __forceinline__ void add_tile_count(int count, int wave, int lane, int* counter) {
  __shared__ int wave_counts[4];
  if (lane == 0) wave_counts[wave] = count;
  __syncthreads();
  if (wave == 0 && lane == 0) {
    const int total = (wave_counts[0] + wave_counts[1]) + (wave_counts[2] + wave_counts[3]);
    if (total) atomicAdd(counter, total);
  }
}

// Level 0 straight from the raw planes, in the role the frame is about to play, plus pyramid levels 1-3: one pass over
// 3 B per pixel instead of  raw -> float I, Z (8 B written)  followed by  I, Z (+ halo) -> role planes (8 B read again).
// A 32 x 8 workgroup owns a 64 x 16 tile; the tile and its one-pixel border are converted into LDS pixel by pixel (rows that
// allow wider loads take the strip ingest, ingest_strips.hip), border coordinates clamped like the reference's derivative
// code (image_model.h), so pixels past the image edge hold the edge value.  Then every thread derives its 2 x 2
// quad from LDS and folds pyramid levels 1-3 (2 x 2 means through LDS).  Float I / Z planes
// of level 0 are never written:
// a frame built this way keeps either its current-role planes (which hold everything) or a 3-B copy of the raw planes
// (keep_grey / keep_raw) from which the other role can be derived later by the same kernel.
// ROLE: -1 = none (copy + pyramid only), 0 = current (A, B), 1 = reference (R + selection count, counter zeroed before).
// Arithmetic = the reference's ingest (surface_pyramid.cpp:65-105) and image_model.h: bit-identical planes.
// CH = 3 / 4: the grey value of a pixel comes from the frame's colour plane (colour.h) -- odd widths, unaligned
// colour planes and padded pitches the strip ingest does not take; keep_grey receives the converted grey.
// CH = kChF32 / ZF: a float image plane / a float depth plane (ingest_strips.hip's float sources) at odd widths and
// rows that are not 8-byte aligned; with ZF the raw copy goes to the float planes I / Z of level 0 (keep_planes).
constexpr int kB0W = 64, kB0H = 16, kB0Stride = 68;

template <int ROLE, int CH = 0, bool ZF = false>
__global__ __launch_bounds__(256) void k_build_from_raw(const FrameBuildPtrs* __restrict__ tbl, float scale, int w0, int h0, int levels,
                                                        float ithr, float dthr, int tiles_x, int tiles_y, int n_frames, int cur_flavor) {
#pragma clang fp contract(off)
  static_assert(CH != kChF32 || ZF, "a float image comes with float depth");
  constexpr bool IF = CH == kChF32, COL = CH == 3 || CH == 4;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8 threads, one 2 x 2 quad each
  const int w1 = w0 >> 1, h1 = h0 >> 1;
  const int w2 = w1 >> 1, h2 = h1 >> 1, w3 = w2 >> 1, h3 = h2 >> 1;
  __shared__ float sI[kB0H + 2][kB0Stride];
  __shared__ float sZ[kB0H + 2][kB0Stride];
  __shared__ float s1[8][32];
  __shared__ float s2[4][16];
  const float nanv = __builtin_nanf("");
  for_each_tile(tiles_x, tiles_y, n_frames, [&](int bx, int by, int frame) {
    const FrameBuildPtrs& f = tbl[frame];
    // (global_ptr.h: every plane pointer read once, as a pointer into the global address space)
    const auto grey = global_ptr(f.grey);
    const auto raw = global_ptr(f.raw);
    const auto keep_grey = global_ptr(f.keep_grey);
    const auto keep_raw = global_ptr(f.keep_raw);
    const auto colour = global_ptr(f.colour);                   // (CH > 0 only)
    const size_t pitch = size_t(f.colour_pitch);
    const GreyWeights gw = grey_weights(pixel_red_first(f.colour_format));
    auto colour_grey = [&](int y, int x) -> uint8_t {          // (CH = 3 / 4 only)
      const auto p = colour + size_t(y) * pitch + size_t(x) * (COL ? CH : 0);
      return uint8_t(grey_of(p[0], p[1], p[2], gw));
    };
    const auto depth_f = (Global<const uint8_t>)global_ptr(f.depth_f32);   // (ZF only; rows are addressed in bytes)
    const size_t zpitch = size_t(f.depth_pitch);
    const bool keep_planes = ZF && f.keep_planes != 0;
    const auto I0 = global_ptr(f.I[0]), Z0 = global_ptr(f.Z[0]);
    const auto A0 = global_ptr(f.A[0]);
    const auto B0 = global_ptr(f.B[0]);
    const auto C0 = global_ptr(f.C[0]);
    const auto R0 = global_ptr(f.R[0]);
    const auto I1 = global_ptr(f.I[1]), I2 = global_ptr(f.I[2]), I3 = global_ptr(f.I[3]);
    const auto Z1 = global_ptr(f.Z[1]), Z2 = global_ptr(f.Z[2]), Z3 = global_ptr(f.Z[3]);
    const int x0 = bx * kB0W, y0 = by * kB0H;
    auto depth_of = [&](uint16_t d) { return d == 0 ? nanv : float(d) * scale; };
    // ---- tile + border into LDS (column c of the slab = image column x0 - 1 + c, row r = image row y0 - 1 + r, clamped) ----
    for (int i = threadIdx.x; i < (kB0H + 2) * (kB0W + 2); i += 256) {
      const int r = i / (kB0W + 2), c = i - r * (kB0W + 2);
      const int yy = y0 - 1 + r, xx = x0 - 1 + c;
      const int y = clamp_index(yy, h0), x = clamp_index(xx, w0);
      const bool own = yy == y && xx == x && r >= 1 && r <= kB0H && c >= 1 && c <= kB0W;   // a pixel of this tile, not of its border
      const uint8_t gv = COL ? colour_grey(y, x) : IF ? uint8_t(0) : grey[size_t(y) * (ZF ? pitch : size_t(w0)) + x];   // (with float depth: a grey plane has a pitch)
      const float iv = IF ? *(Global<const float>)(colour + size_t(y) * pitch + size_t(x) * 4) : float(gv);
      sI[r][c] = iv;
      if (ZF) {
        const float zv = depth_of_f32(*(Global<const float>)(depth_f + size_t(y) * zpitch + size_t(x) * 4), scale);   // (colour.h)
        sZ[r][c] = zv;
        if (keep_planes && own) {
          I0[size_t(y) * w0 + x] = iv;
          Z0[size_t(y) * w0 + x] = zv;
        }
      } else {
        const uint16_t dv = raw[size_t(y) * w0 + x];
        sZ[r][c] = depth_of(dv);
        if (keep_grey && own) {
          keep_grey[size_t(y) * w0 + x] = gv;
          keep_raw[size_t(y) * w0 + x] = dv;
        }
      }
    }
    __syncthreads();
    // ---- level 0 in the frame's role ----
    // wavefront w writes rows w, w + 4, ... of the tile, lane = column: every store instruction covers 64 consecutive pixels
    // (1 KiB of A or R, 512 B of B) instead of every other pixel of two rows
    const int x1 = bx * 32 + tx, y1 = by * 8 + ty;              // level-1 pixel = level-0 quad (pyramid part below)
    int count = 0;
    if (ROLE >= 0) {
      const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
#pragma unroll
      for (int k = 0; k < kB0H / 4; ++k) {
        const int x = x0 + lx, y = y0 + ly + 4 * k;
        const int r = ly + 4 * k + 1, c = lx + 1;
        bool ok = false;
        if (x < w0 && y < h0) {
          const float i0 = sI[r][c], z0 = sZ[r][c];
          const float idx = central_difference(sI[r][c - 1], sI[r][c + 1]), idy = central_difference(sI[r - 1][c], sI[r + 1][c]);
          const float zdx = central_difference(sZ[r][c - 1], sZ[r][c + 1]), zdy = central_difference(sZ[r - 1][c], sZ[r + 1][c]);
          const size_t at = size_t(y) * w0 + x;
          if (ROLE == 0) {
            // the current role comes in two flavours (device_types.h kCurAB / kCurC): the gathered taps of the gathering sweep and
            // the resident kernel, and / or the 8-byte {I, Z} plane the window sweep stages in LDS (align_window.hip)
            if (cur_flavor & kCurAB) {
              gstore(A0 + at, make_float4(i0, z0, idx, idy));
              gstore(B0 + at, make_float2(zdx, zdy));
            }
            if (cur_flavor & kCurC) gstore(C0 + at, make_float2(i0, z0));
          } else {
            ok = selects(z0, idx, idy, zdx, zdy, ithr, dthr);
            gstore(R0 + at, make_float2(ok ? z0 : nanv, i0));
          }
        }
        if (ROLE == 1) count += __popcll(__ballot(ok));         // wave-uniform
      }
    }
    // ---- pyramid levels 1-3 (16 x 4 and 8 x 2 pixels of levels 2 and 3 per tile; an out-of-image quad is never written) ----
    const int r = 2 * ty + 1, c = 2 * tx + 1;
    const float i1 = mean_2x2(sI[r][c], sI[r][c + 1], sI[r + 1][c], sI[r + 1][c + 1]);
    const float z00 = depth_subsample(sZ[r][c]);
    if (levels >= 2 && x1 < w1 && y1 < h1) {
      I1[size_t(y1) * w1 + x1] = i1;
      Z1[size_t(y1) * w1 + x1] = z00;
    }
    s1[ty][tx] = i1;
    // (one barrier either way: s1 complete, sI / sZ free for the next tile)
    if (ROLE == 1) add_tile_count(count, threadIdx.x >> 6, threadIdx.x & 63, f.sel_count);
    else __syncthreads();
    const int x2 = x1 >> 1, y2 = y1 >> 1;
    if ((tx & 1) == 0 && (ty & 1) == 0) {
      const float i2 = mean_2x2(s1[ty][tx], s1[ty][tx + 1], s1[ty + 1][tx], s1[ty + 1][tx + 1]);
      if (levels >= 3 && x2 < w2 && y2 < h2) {
        I2[size_t(y2) * w2 + x2] = i2;
        Z2[size_t(y2) * w2 + x2] = z00;
      }
      s2[ty >> 1][tx >> 1] = i2;
    }
    __syncthreads();
    if (levels >= 4 && (tx & 3) == 0 && (ty & 3) == 0) {
      const int x3 = x1 >> 2, y3 = y1 >> 2, cx = tx >> 1, cy = ty >> 1;
      if (x3 < w3 && y3 < h3) {
        I3[size_t(y3) * w3 + x3] = mean_2x2(s2[cy][cx], s2[cy][cx + 1], s2[cy + 1][cx], s2[cy + 1][cx + 1]);
        Z3[size_t(y3) * w3 + x3] = z00;
      }
    }
    __syncthreads();                                             // s1, s2, the tile count's words free for the next tile of this workgroup
  });
}

__global__ void k_pyr_down(const FrameBuildPtrs* __restrict__ tbl, int level, int w, int h) {
#pragma clang fp contract(off)
  const FrameBuildPtrs& f = tbl[blockIdx.z];
  const auto I = global_ptr<const float>(f.I[level - 1]);       // (global_ptr.h: read once, global address space)
  const auto Z = global_ptr<const float>(f.Z[level - 1]);
  const auto outI = global_ptr(f.I[level]);
  const auto outZ = global_ptr(f.Z[level]);
  const int ow = w >> 1, oh = h >> 1;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= ow || y >= oh) return;
  const auto r0 = I + size_t(2 * y) * w + 2 * x;
  const auto r1 = r0 + w;
  outI[size_t(y) * ow + x] = mean_2x2(r0[0], r0[1], r1[0], r1[1]);
  outZ[size_t(y) * ow + x] = depth_subsample(Z[size_t(2 * y) * w + 2 * x]);
}

// The pixel sources of derive_at (image_model.h: clamped central differences): the planar float planes I / Z of a level, or the
// interleaved {I, Z} plane C of a frame that has been a current frame of the window sweep.  The derived planes are built per ROLE, like
// the reference builds them lazily: a frame that is only ever a current frame gets A + B (buildAccelerationStructure,
// rgbd_image.cpp:534-543), a frame that is only ever a reference gets R + the selection count (PointSelection::select,
// point_selection.cpp:89-152).
struct PlanarSource {
  Global<const float> I, Z;
  int w;
  __device__ __forceinline__ float2 operator()(int x, int y) const { return make_float2(I[size_t(y) * w + x], Z[size_t(y) * w + x]); }
};
struct InterleavedSource {
  Global<const float2> C;
  int w;
  __device__ __forceinline__ float2 operator()(int x, int y) const { return gload(C + size_t(y) * w + x); }
};

// A frame that holds only one flavour of the current role at a level gets the other: the taps A + B from the {I, Z} plane C
// (derive_at over the interleaved plane: bit-identical planes), or C from A.  MODE 2: the reference role
// (R + selection count, counter zeroed before) from C -- PointSelection over a frame that has been a current frame of the window
// sweep so far.
template <int MODE>
__global__ void k_from_current_plane(const FrameBuildPtrs* __restrict__ tbl, int level, int w, int h, float ithr, float dthr,
                                     int tiles_x, int tiles_y, int n_frames) {
  for_each_tile(tiles_x, tiles_y, n_frames, [&](int bx, int by, int frame) {
    const FrameBuildPtrs& f = tbl[frame];
    const auto A = global_ptr(f.A[level]);                      // (global_ptr.h: read once, global address space)
    const auto B = global_ptr(f.B[level]);
    const auto R = global_ptr(f.R[level]);
    const auto Cw = global_ptr(f.C[level]);
    const int x = bx * 64 + threadIdx.x;
    const int y = by * 4 + threadIdx.y;
    bool ok = false;
    if (x < w && y < h) {
      const size_t at = size_t(y) * w + x;
      if (MODE == 1) {
        const float4 a = gload((Global<const float4>)(A + at));
        gstore(Cw + at, make_float2(a.x, a.y));
      } else {
        const Derivs d = derive_at(InterleavedSource{global_ptr<const float2>(f.C[level]), w}, w, h, x, y);
        if (MODE == 0) {
          gstore(A + at, make_float4(d.i0, d.z0, d.idx, d.idy));
          gstore(B + at, make_float2(d.zdx, d.zdy));
        } else {
          ok = selects(d.z0, d.idx, d.idy, d.zdx, d.zdy, ithr, dthr);
          gstore(R + at, make_float2(ok ? d.z0 : __builtin_nanf(""), d.i0));
        }
      }
    }
    if (MODE == 2) {
      add_tile_count(__popcll(__ballot(ok)), threadIdx.y, threadIdx.x, f.sel_count + level);
      __syncthreads();                                          // the tile count's words are rewritten by the next tile
    }
  });
}

// The role planes of SEVERAL pyramid levels of a set of frames in one launch (a single camera frame: levels 1-3 are 6000 pixels
// together; one launch per level, each with its table upload and counter reset, is 9-12 launches of 4 microseconds of work and 8 of
// launch latency each -- the largest item of a tracking front end's frame after the match itself); with a one-level span, the path of
// a level of odd width, which the strips (ingest_strips.hip) do not take.  A workgroup takes a 64 x 16 tile of one level of one frame.
// ROLE 0: current, the two sampling planes (flavour per level: LevelSpan::flavor).  ROLE 1: reference, the streamed plane with the
// selection predicate folded into Z, and the count of selected pixels (counters of the levels zeroed before).
template <int ROLE>
__global__ __launch_bounds__(256) void k_derive_levels(const FrameBuildPtrs* __restrict__ tbl, const LevelSpan span, int n_frames, float ithr, float dthr) {
  const int per_frame = span.tile0[span.l1 + 1], total = per_frame * n_frames;
  for (int gi = blockIdx.x; gi < total; gi += gridDim.x) {
    const int frame = gi / per_frame, t = gi - frame * per_frame;
    int level = span.l0;
    while (level < span.l1 && t >= span.tile0[level + 1]) ++level;
    const int w = span.w[level], h = span.h[level], tiles_x = (w + 63) / 64;
    const int tile = t - span.tile0[level], bx = tile % tiles_x, by = tile / tiles_x;
    const FrameBuildPtrs& f = tbl[frame];
    const auto I = global_ptr<const float>(f.I[level]);
    const auto Z = global_ptr<const float>(f.Z[level]);
    const auto A = global_ptr(f.A[level]);
    const auto B = global_ptr(f.B[level]);
    const auto C = global_ptr(f.C[level]);
    const auto R = global_ptr(f.R[level]);
    const int flavor = span.flavor[level];
    const int x = bx * 64 + threadIdx.x;
    int count = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = (by * 4 + r) * 4 + threadIdx.y;
      bool ok = false;
      if (x < w && y < h) {
        const size_t at = size_t(y) * w + x;
        if (ROLE == 0 && flavor == kCurC) {                     // (uniform) only the {I, Z} pair: no neighbours to read
          gstore(C + at, make_float2(I[at], Z[at]));
        } else {
          const Derivs d = derive_at(PlanarSource{I, Z, w}, w, h, x, y);
          if (ROLE == 0) {
            gstore(A + at, make_float4(d.i0, d.z0, d.idx, d.idy));
            gstore(B + at, make_float2(d.zdx, d.zdy));
            if (flavor & kCurC) gstore(C + at, make_float2(d.i0, d.z0));
          } else {
            ok = selects(d.z0, d.idx, d.idy, d.zdx, d.zdy, ithr, dthr);
            gstore(R + at, make_float2(ok ? d.z0 : __builtin_nanf(""), d.i0));
          }
        }
      }
      if (ROLE == 1) count += __popcll(__ballot(ok));           // wave-uniform
    }
    if (ROLE == 1) {
      add_tile_count(count, threadIdx.y, threadIdx.x, f.sel_count + level);
      __syncthreads();                                          // the tile count's words are rewritten by the next tile
    }
  }
}

__global__ void k_zero_counts_levels(const FrameBuildPtrs* __restrict__ tbl, int n_frames, int l0, int l1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_frames)
    for (int l = l0; l <= l1; ++l) tbl[i].sel_count[l] = 0;
}

// re-selection with other thresholds (PointSelection with a different predicate), one frame
__global__ void k_select_pack(const float4* __restrict__ A, const float2* __restrict__ B, int n, float ithr, float dthr,
                              float2* __restrict__ R, int* __restrict__ count, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const float4 a = A[i];
    const float2 b = B[i];
    ok = selects(a.y, a.z, a.w, b.x, b.y, ithr, dthr);
    R[i] = make_float2(ok ? a.y : __builtin_nanf(""), a.x);
    if (mask) mask[i] = ok ? 1 : 0;
  }
  const unsigned long long ballot = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(count, __popcll(ballot));
}

// The caller selection of reference frames (selection.h) over their freshly built planes R: a selected pixel the mask or the depth
// range rejects gets Zsel = NaN -- the sweeps already treat that as unselected -- and leaves the level's count.  A workgroup takes 512
// pixels of one level of one frame (span.tile0: block offsets), a lane two of them, read 16 B at a time; stores only where a pixel
// leaves.  The ref_order saved slots beside the counts are not touched (the pass always follows a fresh build, never a Q3 edit).
__global__ __launch_bounds__(256) void k_apply_selection(const SelectionApply* __restrict__ tbl, const LevelSpan span, int n_frames) {
  const int per_frame = span.tile0[span.l1 + 1], total = per_frame * n_frames;
  for (int gi = blockIdx.x; gi < total; gi += gridDim.x) {
    const int frame = gi / per_frame, t = gi - frame * per_frame;
    int level = span.l0;
    while (level < span.l1 && t >= span.tile0[level + 1]) ++level;
    const int w = span.w[level], npx = w * span.h[level];
    const SelectionApply& f = tbl[frame];
    float2* R = f.R[level];
    const int i0 = (t - span.tile0[level]) * 512 + int(threadIdx.x) * 2;
    bool gone[2] = {false, false};
    if (i0 < npx) {
      float z[2];
      if (i0 + 1 < npx) {                                       // (R is 256-byte aligned and i0 even: a 16-byte load)
        const float4 two = *reinterpret_cast<const float4*>(R + i0);
        z[0] = two.x; z[1] = two.z;
      } else {
        z[0] = R[i0].x; z[1] = __builtin_nanf("");
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int i = i0 + k;
        if (z[k] == z[k]) {                                     // selected so far (a selected pixel has a finite depth)
          const int y = i / w, x = i - y * w;
          if (!selection_keeps(f.mask, size_t(f.pitch), level, x, y, z[k], f.range_on != 0, f.min_depth, f.max_depth)) {
            R[i].x = __builtin_nanf("");
            if (f.report) f.report[i] = 0;
            gone[k] = true;
          }
        }
      }
    }
    const int removed = __popcll(__ballot(gone[0])) + __popcll(__ballot(gone[1]));   // wave-uniform
    if ((threadIdx.x & 63) == 0 && removed) atomicSub(f.sel_count + level, removed);
  }
}

__global__ void k_pack_accepted(const float4* __restrict__ A, const uint8_t* __restrict__ accepted, int n, float2* __restrict__ R,
                                int* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const float4 a = A[i];
    ok = accepted[i] != 0;
    R[i] = make_float2(ok ? a.y : __builtin_nanf(""), a.x);
  }
  const unsigned long long ballot = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(count, __popcll(ballot));
}

__global__ void k_unpack_plane(const float4* __restrict__ A, const float2* __restrict__ B, int n, int plane, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v;
  switch (plane) {
    case 0: v = A[i].x; break;
    case 1: v = A[i].y; break;
    case 2: v = A[i].z; break;
    case 3: v = A[i].w; break;
    case 4: v = B[i].x; break;
    default: v = B[i].y; break;
  }
  out[i] = v;
}

static void zero_counts(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int l0, int l1) {
  k_zero_counts_levels<<<dim3((n_frames + 63) / 64), dim3(64), 0, s>>>(tbl, n_frames, l0, l1);
}

LevelSpan level_span(int l0, int l1, const int* w, const int* h, bool pixel_blocks) {
  LevelSpan span{};
  span.l0 = l0; span.l1 = l1;
  int units = 0;
  for (int l = l0; l <= l1; ++l) {
    span.w[l] = w[l]; span.h[l] = h[l];
    span.tile0[l] = units;
    units += pixel_blocks ? (w[l] * h[l] + 511) / 512 : ((w[l] + 63) / 64) * ((h[l] + 15) / 16);
  }
  span.tile0[l1 + 1] = units;
  return span;
}

// one level of k_derive_levels: the form of launch_derive_current / launch_derive_reference at odd widths
static LevelSpan one_level_span(int level, int w, int h, int flavor) {
  int ws[kMaxLevels] = {}, hs[kMaxLevels] = {};
  ws[level] = w; hs[level] = h;
  LevelSpan span = level_span(level, level, ws, hs);
  span.flavor[level] = flavor;
  return span;
}

void launch_build_from_raw(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, float scale, int w0, int h0, int levels, int role, bool strips,
                           float ithr, float dthr, int max_workgroups, int cur_flavor, int c_levels, int colour_channels, bool stream_nt,
                           bool depth_f32) {
  depth_f32 = depth_f32 || colour_channels == kChF32;
  if (role == 1) zero_counts(s, tbl, n_frames, 0, 0);
  if (strips) {
    launch_ingest_strips(s, tbl, n_frames, scale, w0, h0, levels, role, ithr, dthr, max_workgroups, cur_flavor, c_levels, colour_channels, stream_nt,
                         depth_f32);
    return;
  }
  const int tx = (w0 + kB0W - 1) / kB0W, ty = (h0 + kB0H - 1) / kB0H;
  const dim3 grid(capped_grid((long long)tx * ty * n_frames, max_workgroups)), block(256);
  const int lv = levels < 4 ? levels : 4;
  with_value<0, 1, -1>(role, [&](auto ROLE) {
    with_value<3, 4, kChF32, 0>(colour_channels, [&](auto CH) {
      with_bool(depth_f32, [&](auto ZF) {
        constexpr int kCh = decltype(CH)::value;
        constexpr bool kZf = decltype(ZF)::value;
        if constexpr (kCh != kChF32 || kZf)
          k_build_from_raw<decltype(ROLE)::value, kCh, kZf><<<grid, block, 0, s>>>(tbl, scale, w0, h0, lv, ithr, dthr, tx, ty, n_frames, cur_flavor);
      });
    });
  });
}

void launch_pyr_down(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h) {
  const int ow = w / 2, oh = h / 2;
  k_pyr_down<<<dim3((ow + 63) / 64, (oh + 3) / 4, n_frames), dim3(64, 4), 0, s>>>(tbl, level, w, h);
}

// (even widths: the strip form, ingest_strips.hip; odd ones: k_derive_levels over the one level)
void launch_derive_current(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, int max_workgroups, int cur_flavor,
                           bool stream_nt) {
  if (derive_strips_supports(w)) {
    launch_derive_strips(s, tbl, n_frames, level, w, h, 0, 0.0f, 0.0f, max_workgroups, cur_flavor, stream_nt);
    return;
  }
  launch_derive_levels(s, tbl, n_frames, one_level_span(level, w, h, cur_flavor), 0, 0.0f, 0.0f, max_workgroups);
}

void launch_from_current_plane(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, int mode, float ithr, float dthr,
                               int max_workgroups) {
  const int tx = (w + 63) / 64, ty = (h + 3) / 4;
  const dim3 grid(capped_grid((long long)tx * ty * n_frames, max_workgroups)), block(64, 4);
  if (mode == 2) zero_counts(s, tbl, n_frames, level, level);
  with_value<0, 1, 2>(mode, [&](auto MODE) {
    k_from_current_plane<decltype(MODE)::value><<<grid, block, 0, s>>>(tbl, level, w, h, ithr, dthr, tx, ty, n_frames);
  });
}

void launch_derive_levels(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, const LevelSpan& span, int role, float ithr, float dthr,
                          int max_workgroups) {
  const int total = span.tile0[span.l1 + 1] * n_frames;
  const dim3 grid(capped_grid(total, max_workgroups)), block(64, 4);
  if (role == 1) zero_counts(s, tbl, n_frames, span.l0, span.l1);
  with_value<1, 0>(role, [&](auto ROLE) { k_derive_levels<decltype(ROLE)::value><<<grid, block, 0, s>>>(tbl, span, n_frames, ithr, dthr); });
}

void launch_derive_reference(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, float ithr, float dthr,
                             int max_workgroups, bool stream_nt) {
  if (derive_strips_supports(w)) {
    zero_counts(s, tbl, n_frames, level, level);
    launch_derive_strips(s, tbl, n_frames, level, w, h, 1, ithr, dthr, max_workgroups, 0, stream_nt);
    return;
  }
  launch_derive_levels(s, tbl, n_frames, one_level_span(level, w, h, 0), 1, ithr, dthr, max_workgroups);
}

void launch_select_pack(hipStream_t s, const float4* A, const float2* B, int n, float ithr, float dthr, float2* R, int* count, uint8_t* mask) {
  k_select_pack<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(A, B, n, ithr, dthr, R, count, mask);
}

void launch_apply_selection(hipStream_t s, const SelectionApply* tbl, int n_frames, const LevelSpan& span, int max_workgroups) {
  const int total = span.tile0[span.l1 + 1] * n_frames;
  k_apply_selection<<<dim3(capped_grid(total, max_workgroups)), dim3(256), 0, s>>>(tbl, span, n_frames);
}

void launch_pack_accepted(hipStream_t s, const float4* A, const uint8_t* accepted, int n, float2* R, int* count) {
  k_pack_accepted<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(A, accepted, n, R, count);
}

void launch_unpack_plane(hipStream_t s, const float4* A, const float2* B, int n, int plane, float* out) {
  k_unpack_plane<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(A, B, n, plane, out);
}

}  // namespace dvo_hip
