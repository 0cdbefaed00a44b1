// ingest_strips.hip -- the ingest of raw sensor planes (level 0 in the frame's role + pyramid levels 1-3) with one 128 x 8 pixel
// strip per WAVEFRONT, everything in registers: no LDS, no barriers.
//
// Same arithmetic as k_build_from_raw (pyramid_kernels.hip), which remains the path for odd widths and unaligned planes -- the
// reference's ingest (dvo_core/src/core/surface_pyramid.cpp:65-105) and, from image_model.h, the 2x2-mean pyr-down, the depth
// subsampling, the clamped central differences and the selection predicate: bit-identical planes.  What differs is how the work is
// laid out on the machine.
// k_build_from_raw gives a 64 x 16 tile to a 256-thread workgroup that converts it into LDS and meets at three barriers; a
// workgroup has 3 KB of loads in flight in two dependent rounds and the kernel moves 14 B per pixel at 1.7 of the 8 TB/s (1024
// frames of 640 x 480: 2.6 ms, the largest single item of a bench step after the finest-level sweeps).  Here
//   lane l of a wavefront owns pixel columns 2l, 2l + 1 of the strip and all 8 (+ 2 halo) rows: 16-20 independent loads per lane are
//     issued before the first is used (6 KB in flight per wavefront, 100+ KB per CU);
//   a lane's pixel pair is 16 B of every 8-B-per-pixel plane (R, C, B): one 16-B store per lane and row, 1 KiB per instruction;
//   the horizontal neighbours of a pair are the adjacent lanes' registers (DPP wave shifts; lanes 0 and 63 load the strip's edge
//     columns), the vertical ones the lane's own rows; the 2 x 2 means of levels 1-3 are in-lane sums and DPP row shifts;
//   the four wavefronts of a workgroup take four vertically adjacent strips, so their shared halo rows meet in the CU's cache.
// A current frame that is only read by the window sweep (plane C = {I, Z}, align_window.hip) needs no neighbours at all: TAPS = false
// drops the halo rows, the edge columns and the differences.
// CH = 3 / 4: the frame's 8-bit colour plane takes the grey plane's place (colour.h).  A lane reads its pixel pair as the 8 bytes of one
// 4-byte-aligned window (3 channels: 6 bytes at an even offset, the window starts 2 bytes early when x % 4 == 2 and otherwise ends inside
// pixel x + 2, never outside the row; 4 channels: 8 aligned bytes), converts it to the same two grey bytes the grey plane would hold,
// and everything after that is the grey ingest's code.  BGR against RGB order is a wave-uniform choice of weights, not a variant.
// Float sources: CH = kChF32 reads the image as one float per pixel (0..255, taken as is), ZF the depth as float metres (NaN = hole,
// stored as z * scale, rounded on its own).  A lane's pixel pair is then ONE 8-byte load per float plane and row (512 B per wavefront
// and instruction, rows 8-byte aligned) instead of 2 + 4 bytes; the conversion is the only difference, everything behind it is shared.
// A float-depth frame's raw copy is its own float planes I / Z of level 0 (FrameBuildPtrs::keep_planes), written with the NT policy
// like the u8 / u16 copy.
#include "colour.h"
#include "dispatch.h"
#include "global_ptr.h"
#include "image_model.h"
#include "launch.h"

namespace dvo_hip {

namespace {

constexpr int kStripW = 128, kStripH = 8, kStripsPerGroup = 4;
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138, kDppRowShl1 = 0x101, kDppRowShl2 = 0x102;

// lane i <- lane i + 1 of the wavefront; lane 63 keeps `edge`
__device__ __forceinline__ float from_next_lane(float v, float edge) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), kDppWaveShl1, 0xf, 0xf, false));
}
// lane i <- lane i - 1 of the wavefront; lane 0 keeps `edge`
__device__ __forceinline__ float from_previous_lane(float v, float edge) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), kDppWaveShr1, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ float row_shifted(float v) {   // within a row of 16 lanes; the lanes that use it always have a source lane
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// the 8 bytes that hold pixels x, x + 1 (x even) of a colour row with CH bytes per pixel (see the head of the file); two dword loads
// the compiler merges into one 8-byte load (the window is 4-byte aligned only)
template <int CH, bool NT>
__device__ __forceinline__ unsigned long long colour_pair_bits(Global<const uint8_t> row, int x) {
  const Global<const unsigned> at = (Global<const unsigned>)(row + ((CH * x) & ~3));
  return (unsigned long long)gld<NT>(at + 1) << 32 | gld<NT>(at);
}
// the grey bytes of pixels x, x + 1 from colour_pair_bits: grey(x) | grey(x + 1) << 8, as a grey plane's 16-bit load would give them
template <int CH>
__device__ __forceinline__ unsigned colour_pair_grey(unsigned long long bits, int x, GreyWeights w) {
  const int s = CH == 3 ? (x & 2) * 8 : 0;
  return grey_at_bits(bits, s, w) | grey_at_bits(bits, s + 8 * CH, w) << 8;
}

}  // namespace

// The role planes of a strip's 8 rows from its register rows: I / Z[j] = image row y0 + kFirst + j (clamped), kFirst = -1 with TAPS;
// eI / eZ[r]: the strip's edge columns (lane 0: the column left of the strip, lane 63: the column right of it).  Returns the number of
// selected pixels of the wavefront (ROLE 1).
template <int ROLE, bool TAPS, bool NT>
__device__ __forceinline__ int strip_role_planes(const float (&I)[TAPS ? kStripH + 2 : kStripH][2], const float (&Z)[TAPS ? kStripH + 2 : kStripH][2],
                                                 const float (&eI)[kStripH], const float (&eZ)[kStripH], int x, int y0, int w0, int h0, bool in_x,
                                                 Global<float2> R0, Global<float4> A0, Global<float2> B0, Global<float2> C0, int cur_flavor,
                                                 float ithr, float dthr) {
#pragma clang fp contract(off)
  constexpr int kFirst = TAPS ? -1 : 0;
  const float nanv = __builtin_nanf("");
  int count = 0;
#pragma unroll
      for (int r = 0; r < kStripH; ++r) {
        const int j = r - kFirst, y = y0 + r;
        const bool inside = in_x && y < h0;
        const size_t at = size_t(y) * w0 + x;
        const float i0 = I[j][0], i1 = I[j][1], z0 = Z[j][0], z1 = Z[j][1];
        if (TAPS) {
          // column x - 1 of the pair's first pixel: the previous lane's second pixel (lane 0: the edge column); at the image border the
          // pixel itself, which is what the clamped index reads (image_model.h); column x + 2 of the second pixel likewise
          const float ie = eI[r], ze = eZ[r];
          const float il_n = from_previous_lane(i1, ie), zl_n = from_previous_lane(z1, ze);
          const float ir_n = from_next_lane(i0, ie), zr_n = from_next_lane(z0, ze);
          const float il = x > 0 ? il_n : i0, zl = x > 0 ? zl_n : z0;
          const float ir = x + 2 < w0 ? ir_n : i1, zr = x + 2 < w0 ? zr_n : z1;
          const float idx0 = central_difference(il, i1), idx1 = central_difference(i0, ir);
          const float zdx0 = central_difference(zl, z1), zdx1 = central_difference(z0, zr);
          const float idy0 = central_difference(I[j - 1][0], I[j + 1][0]), idy1 = central_difference(I[j - 1][1], I[j + 1][1]);
          const float zdy0 = central_difference(Z[j - 1][0], Z[j + 1][0]), zdy1 = central_difference(Z[j - 1][1], Z[j + 1][1]);
          if (ROLE == 1) {
            const bool ok0 = inside && selects(z0, idx0, idy0, zdx0, zdy0, ithr, dthr);
            const bool ok1 = inside && selects(z1, idx1, idy1, zdx1, zdy1, ithr, dthr);
            if (inside) gstore_pair<NT>(R0 + at, make_float4(ok0 ? z0 : nanv, i0, ok1 ? z1 : nanv, i1));
            count += __popcll(__ballot(ok0)) + __popcll(__ballot(ok1));   // wave-uniform
          } else if (inside) {
            if (cur_flavor & kCurAB) {
              gstore<NT>(A0 + at, make_float4(i0, z0, idx0, idy0));
              gstore<NT>(A0 + at + 1, make_float4(i1, z1, idx1, idy1));
              gstore_pair<NT>(B0 + at, make_float4(zdx0, zdy0, zdx1, zdy1));
            }
            if (cur_flavor & kCurC) gstore_pair<NT>(C0 + at, make_float4(i0, z0, i1, z1));
          }
        } else if (inside) {
          gstore_pair<NT>(C0 + at, make_float4(i0, z0, i1, z1));
        }
      }
  return count;
}

// ROLE: -1 = none (raw copy + pyramid only), 0 = current, 1 = reference (R + selection count, counter zeroed before).
// TAPS: level 0 needs the central differences (reference role; current role with the gathered taps A + B).
// c_levels: bit l set = pyramid level l (1-3) also gets the current role's {I, Z} plane C.
// CH: 0 = the grey plane f.grey, 3 / 4 = the colour plane f.colour with 3 / 4 bytes per pixel,
// kChF32 = the float image plane in f.colour (8-byte aligned rows of f.colour_pitch bytes).
// NT: the raw planes are read, and the planes of levels 0-1 and the raw copy written, with the non-temporal policy (global_ptr.h): a
// background build beside the coarse levels of a match then leaves their planes in the Infinity Cache.  Levels 2-3 keep the default.
// ZF: the depth plane is f.depth_f32 (float metres, 8-byte aligned rows of f.depth_pitch bytes) instead of the u16 plane f.raw.
template <int ROLE, bool TAPS, int CH = 0, bool NT = false, bool ZF = false>
__global__ __launch_bounds__(256) void k_ingest_strips(const FrameBuildPtrs* __restrict__ tbl, float scale, int w0, int h0, int levels,
                                                       float ithr, float dthr, int groups_x, int groups_y, int n_frames, int cur_flavor, int c_levels) {
#pragma clang fp contract(off)
  static_assert(ROLE != 1 || TAPS, "the selection predicate needs the differences");
  static_assert(CH != kChF32 || ZF, "a float image comes with float depth");
  constexpr bool IF = CH == kChF32, COL = CH == 3 || CH == 4;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w1 = w0 >> 1, h1 = h0 >> 1, w2 = w1 >> 1, h2 = h1 >> 1, w3 = w2 >> 1, h3 = h2 >> 1;
  const float nanv = __builtin_nanf("");
  const int per_frame = groups_x * groups_y, total = per_frame * n_frames;
  for (int gi = blockIdx.x; gi < total; gi += gridDim.x) {
    const int frame = gi / per_frame, t = gi - frame * per_frame;
    const int sx = t % groups_x, sy = (t / groups_x) * kStripsPerGroup + wave;
    const int y0 = sy * kStripH;
    if (y0 >= h0) continue;                                     // (wave-uniform; nothing below synchronises the workgroup)
    const FrameBuildPtrs& f = tbl[frame];
    const auto grey = global_ptr(f.grey);
    const auto raw = global_ptr(f.raw);
    const auto keep_grey = global_ptr(f.keep_grey);
    const auto keep_raw = global_ptr(f.keep_raw);
    const auto colour = global_ptr(f.colour);                  // (CH > 0 only)
    const size_t pitch = size_t(f.colour_pitch);
    const GreyWeights gw = grey_weights(pixel_red_first(f.colour_format));
    const auto depth_f = (Global<const uint8_t>)global_ptr(f.depth_f32);   // (ZF only; rows are addressed in bytes)
    const size_t zpitch = size_t(f.depth_pitch);
    const bool keep_planes = ZF && f.keep_planes != 0;
    const auto I0 = global_ptr(f.I[0]), Z0 = global_ptr(f.Z[0]);
    // (the pointers of every plane the strip writes, read before the loads are issued: a scalar load further down would wait behind them)
    const auto R0 = global_ptr(f.R[0]);
    const auto A0 = global_ptr(f.A[0]);
    const auto B0 = global_ptr(f.B[0]);
    const auto C0 = global_ptr(f.C[0]);
    const auto I1 = global_ptr(f.I[1]), I2 = global_ptr(f.I[2]), I3 = global_ptr(f.I[3]);
    const auto Z1 = global_ptr(f.Z[1]), Z2 = global_ptr(f.Z[2]), Z3 = global_ptr(f.Z[3]);
    const auto C1 = global_ptr(f.C[1]), C2 = global_ptr(f.C[2]), C3 = global_ptr(f.C[3]);
    const bool want_c1 = (c_levels & 2) && C1, want_c2 = (c_levels & 4) && C2, want_c3 = (c_levels & 8) && C3;   // (a frame without the plane: skipped)
    const auto sel_count = global_ptr(f.sel_count);
    const int x = sx * kStripW + 2 * lane;
    const bool in_x = x < w0;                                   // widths are even here: the pair is inside or outside as a whole
    const int xl = in_x ? x : w0 - 2;                           // lanes past the right border load the last pair (and store nothing)
    auto depth_of = [&](unsigned d) { return d == 0 ? nanv : float(d) * scale; };

    // ---- every load of the strip, before anything is used ----
    constexpr int kFirst = TAPS ? -1 : 0, kRows = TAPS ? kStripH + 2 : kStripH;   // register row j = image row y0 + kFirst + j (clamped)
    unsigned g[kRows], d[kRows];
    unsigned long long cb[COL ? kRows : 1];                     // (colour: the pixel pair's bytes, converted once every load is issued)
    GlobalF32x2 fi[IF ? kRows : 1], fz[ZF ? kRows : 1];         // (float planes: the pixel pair itself)
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const int y = min(max(y0 + kFirst + j, 0), h0 - 1);       // (scalar)
      const size_t row = size_t(y) * w0;
      if (COL) cb[j] = colour_pair_bits<CH, NT>(colour + size_t(y) * pitch, xl);
      else if (IF) fi[j] = gld<NT>((Global<const GlobalF32x2>)(colour + size_t(y) * pitch + size_t(xl) * 4));
      else g[j] = gld<NT>((Global<const uint16_t>)(grey + (ZF ? size_t(y) * pitch : row) + xl));   // (with float depth: a grey plane has a pitch)
      if (ZF) fz[j] = gld<NT>((Global<const GlobalF32x2>)(depth_f + size_t(y) * zpitch + size_t(xl) * 4));
      else d[j] = gld<NT>((Global<const uint32_t>)(raw + row + xl));
    }
    unsigned ge[kStripH], de[kStripH];                          // the strip's edge columns, rows y0 .. y0 + 7: lane 0 left, the others right
    unsigned long long cbe[COL && TAPS ? kStripH : 1];          // (colour: the bytes of the pair that holds the edge column)
    float fie[IF && TAPS ? kStripH : 1], fze[ZF && TAPS ? kStripH : 1];
    const int xe = lane == 0 ? max(sx * kStripW - 1, 0) : min(sx * kStripW + kStripW, w0 - 1);
    if (TAPS) {
      const bool edge_lane = lane == 0 || lane == 63;
#pragma unroll
      for (int r = 0; r < kStripH; ++r) {
        const size_t row = size_t(min(y0 + r, h0 - 1)) * w0;
        const size_t ye = size_t(min(y0 + r, h0 - 1));
        ge[r] = 0u; de[r] = 0u;
        if (COL) cbe[r] = 0ull;
        if (IF) fie[r] = 0.0f;
        if (ZF) fze[r] = 0.0f;
        if (edge_lane) {
          if (COL) cbe[r] = colour_pair_bits<CH, NT>(colour + ye * pitch, xe & ~1);
          else if (IF) fie[r] = gld<NT>((Global<const float>)(colour + ye * pitch + size_t(xe) * 4));
          else ge[r] = gld<NT>(grey + (ZF ? ye * pitch : row) + xe);
          if (ZF) fze[r] = gld<NT>((Global<const float>)(depth_f + ye * zpitch + size_t(xe) * 4));
          else de[r] = gld<NT>(raw + row + xe);
        }
      }
    }
    if (COL) {
#pragma unroll
      for (int j = 0; j < kRows; ++j) g[j] = colour_pair_grey<CH>(cb[j], xl, gw);
      if (TAPS) {
#pragma unroll
        for (int r = 0; r < kStripH; ++r) ge[r] = colour_pair_grey<CH>(cbe[r], xe & ~1, gw) >> (8 * (xe & 1)) & 0xffu;
      }
    }
    if (!ZF && keep_grey && in_x) {                             // the frame's own copy of its raw planes (for the other role, later)
#pragma unroll
      for (int r = 0; r < kStripH; ++r) {
        const int y = y0 + r;
        if (y < h0) {
          const size_t at = size_t(y) * w0 + x;
          gst<NT>((Global<uint16_t>)(keep_grey + at), uint16_t(g[r - kFirst]));
          gst<NT>((Global<uint32_t>)(keep_raw + at), d[r - kFirst]);
        }
      }
    }
    float I[kRows][2], Z[kRows][2];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (IF) { I[j][0] = fi[j].x; I[j][1] = fi[j].y; }
      else { I[j][0] = float(g[j] & 0xffu); I[j][1] = float(g[j] >> 8); }
      if (ZF) { Z[j][0] = depth_of_f32(fz[j].x, scale); Z[j][1] = depth_of_f32(fz[j].y, scale); }   // (colour.h)
      else { Z[j][0] = depth_of(d[j] & 0xffffu); Z[j][1] = depth_of(d[j] >> 16); }
    }
    if (ZF && keep_planes && in_x) {                            // float depth: the frame's raw copy is its float planes I / Z of level 0
#pragma unroll
      for (int r = 0; r < kStripH; ++r) {
        const int y = y0 + r;
        if (y < h0) {
          const size_t at = size_t(y) * w0 + x;
          gst<NT>((Global<GlobalF32x2>)(I0 + at), GlobalF32x2{I[r - kFirst][0], I[r - kFirst][1]});
          gst<NT>((Global<GlobalF32x2>)(Z0 + at), GlobalF32x2{Z[r - kFirst][0], Z[r - kFirst][1]});
        }
      }
    }

    // ---- level 0 in the frame's role ----
    float eI[kStripH], eZ[kStripH];
    if (TAPS) {
#pragma unroll
      for (int r = 0; r < kStripH; ++r) {
        eI[r] = IF ? fie[r] : float(ge[r]);
        eZ[r] = ZF ? depth_of_f32(fze[r], scale) : depth_of(de[r]);
      }
    }
    const int count = ROLE >= 0 ? strip_role_planes<ROLE, TAPS, NT>(I, Z, eI, eZ, x, y0, w0, h0, in_x, R0, A0, B0, C0, cur_flavor, ithr, dthr) : 0;
    if (ROLE == 1 && lane == 0 && count) atomicAdd((int*)sel_count, count);

    // ---- pyramid levels 1-3: 64 x 4, 32 x 2 and 16 x 1 pixels per strip; an out-of-image quad is never written ----
    if (levels < 2) continue;
    const int x1 = sx * (kStripW / 2) + lane;
    float m1[4], z1v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = 2 * k - kFirst, y1 = sy * 4 + k;
      m1[k] = mean_2x2(I[j][0], I[j][1], I[j + 1][0], I[j + 1][1]);
      z1v[k] = depth_subsample(Z[j][0]);
      if (x1 < w1 && y1 < h1) {
        const size_t at = size_t(y1) * w1 + x1;
        gst<NT>(I1 + at, m1[k]);
        gst<NT>(Z1 + at, z1v[k]);
        if (want_c1) gstore<NT>(C1 + at, make_float2(m1[k], z1v[k]));
      }
    }
    if (levels < 3) continue;
    const int x2 = x1 >> 1;
    float m2[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int y2 = sy * 2 + m;
      m2[m] = mean_2x2(m1[2 * m], row_shifted<kDppRowShl1>(m1[2 * m]), m1[2 * m + 1], row_shifted<kDppRowShl1>(m1[2 * m + 1]));
      if ((lane & 1) == 0 && x2 < w2 && y2 < h2) {
        const size_t at = size_t(y2) * w2 + x2;
        I2[at] = m2[m];
        Z2[at] = z1v[2 * m];
        if (want_c2) gstore(C2 + at, make_float2(m2[m], z1v[2 * m]));
      }
    }
    if (levels < 4) continue;
    const int x3 = x1 >> 2, y3 = sy;
    const float m3 = mean_2x2(m2[0], row_shifted<kDppRowShl2>(m2[0]), m2[1], row_shifted<kDppRowShl2>(m2[1]));
    if ((lane & 3) == 0 && x3 < w3 && y3 < h3) {
      const size_t at = size_t(y3) * w3 + x3;
      I3[at] = m3;
      Z3[at] = z1v[0];
      if (want_c3) gstore(C3 + at, make_float2(m3, z1v[0]));
    }
  }
}

// The role planes of ONE pyramid level from the float planes I / Z (levels >= 1, and level 0 of frames created from float planes): the
// same strips, the same role code, 8-byte loads of pixel pairs instead of the raw planes' 2 + 4 bytes.  Takes the batches; odd widths
// and a single camera frame's levels (one launch for all of them) go through k_derive_levels (one pixel per thread, ten scattered
// 4-byte loads each: 3 TB/s).
// NT: loads and stores with the non-temporal policy (the ingest's NT, for level 1 of a background build).
template <int ROLE, bool TAPS, bool NT = false>
__global__ __launch_bounds__(256) void k_derive_strips(const FrameBuildPtrs* __restrict__ tbl, int level, int w0, int h0, float ithr, float dthr,
                                                       int groups_x, int groups_y, int n_frames, int cur_flavor) {
#pragma clang fp contract(off)
  static_assert(ROLE == 0 || ROLE == 1, "current or reference");
  static_assert(ROLE != 1 || TAPS, "the selection predicate needs the differences");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int per_frame = groups_x * groups_y, total = per_frame * n_frames;
  for (int gi = blockIdx.x; gi < total; gi += gridDim.x) {
    const int frame = gi / per_frame, t = gi - frame * per_frame;
    const int sx = t % groups_x, sy = (t / groups_x) * kStripsPerGroup + wave;
    const int y0 = sy * kStripH;
    if (y0 >= h0) continue;
    const FrameBuildPtrs& f = tbl[frame];
    const auto Ip = global_ptr<const float>(f.I[level]);
    const auto Zp = global_ptr<const float>(f.Z[level]);
    const auto Rl = global_ptr(f.R[level]);
    const auto Al = global_ptr(f.A[level]);
    const auto Bl = global_ptr(f.B[level]);
    const auto Cl = global_ptr(f.C[level]);
    const auto sel_count = global_ptr(f.sel_count);
    const int x = sx * kStripW + 2 * lane;
    const bool in_x = x < w0;
    const int xl = in_x ? x : w0 - 2;
    constexpr int kFirst = TAPS ? -1 : 0, kRows = TAPS ? kStripH + 2 : kStripH;
    float I[kRows][2], Z[kRows][2];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const int y = min(max(y0 + kFirst + j, 0), h0 - 1);
      const size_t row = size_t(y) * w0;
      const GlobalF32x2 iv = gld<NT>((Global<const GlobalF32x2>)(Ip + row + xl));
      const GlobalF32x2 zv = gld<NT>((Global<const GlobalF32x2>)(Zp + row + xl));
      I[j][0] = iv.x; I[j][1] = iv.y;
      Z[j][0] = zv.x; Z[j][1] = zv.y;
    }
    float eI[kStripH], eZ[kStripH];
    if (TAPS) {
      const int xe = lane == 0 ? max(sx * kStripW - 1, 0) : min(sx * kStripW + kStripW, w0 - 1);
      const bool edge_lane = lane == 0 || lane == 63;
#pragma unroll
      for (int r = 0; r < kStripH; ++r) {
        const size_t row = size_t(min(y0 + r, h0 - 1)) * w0;
        eI[r] = 0.0f; eZ[r] = 0.0f;
        if (edge_lane) {
          eI[r] = gld<NT>(Ip + row + xe);
          eZ[r] = gld<NT>(Zp + row + xe);
        }
      }
    }
    const int count = strip_role_planes<ROLE, TAPS, NT>(I, Z, eI, eZ, x, y0, w0, h0, in_x, Rl, Al, Bl, Cl, cur_flavor, ithr, dthr);
    if (ROLE == 1 && lane == 0 && count) atomicAdd((int*)sel_count + level, count);
  }
}

bool derive_strips_supports(int w) { return w % 2 == 0 && w >= 4; }

// role 0: current (flavours cur_flavor), role 1: reference (the level's counters zeroed before by the caller)
// stream_nt: the non-temporal policy at levels 0-1 (launch.h)
void launch_derive_strips(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, int level, int w, int h, int role, float ithr, float dthr,
                          int max_workgroups, int cur_flavor, bool stream_nt) {
  const int gx = (w + kStripW - 1) / kStripW, gy = (h + kStripH * kStripsPerGroup - 1) / (kStripH * kStripsPerGroup);
  const long long total = (long long)gx * gy * n_frames;
  const dim3 grid(capped_grid(total, max_workgroups)), block(256);
  auto launch = [&](auto ROLE, auto TAPS) {
    with_bool(stream_nt && level <= 1, [&](auto NT) {
      k_derive_strips<decltype(ROLE)::value, decltype(TAPS)::value, decltype(NT)::value>
          <<<grid, block, 0, s>>>(tbl, level, w, h, ithr, dthr, gx, gy, n_frames, cur_flavor);
    });
  };
  if (role == 1) launch(std::integral_constant<int, 1>{}, std::true_type{});
  else with_bool((cur_flavor & kCurAB) != 0, [&](auto TAPS) { launch(std::integral_constant<int, 0>{}, TAPS); });
}

// (a float image with float depth: every even width; the 8-bit planes' loads want rows of 4 pixels)
bool ingest_strips_supports(int w0, bool wide, bool f32_image) { return wide && w0 % (f32_image ? 2 : 4) == 0; }

// (a float plane: the lanes' 8-byte pixel pairs)
bool f32_strips_aligned(const void* plane, size_t pitch) { return reinterpret_cast<uintptr_t>(plane) % 8 == 0 && pitch % 8 == 0; }

// (a colour plane: 3-byte pixels need 4-byte aligned rows, 4-byte pixels 8-byte aligned ones, see colour_pair_bits)
bool colour_strips_aligned(const void* colour, size_t pitch, int channels) {
  const size_t a = channels == 4 ? 8 : 4;
  return reinterpret_cast<uintptr_t>(colour) % a == 0 && pitch % a == 0;
}

void launch_ingest_strips(hipStream_t s, const FrameBuildPtrs* tbl, int n_frames, float scale, int w0, int h0, int levels, int role,
                          float ithr, float dthr, int max_workgroups, int cur_flavor, int c_levels, int colour_channels, bool stream_nt,
                          bool depth_f32) {
  const int gx = (w0 + kStripW - 1) / kStripW, gy = (h0 + kStripH * kStripsPerGroup - 1) / (kStripH * kStripsPerGroup);
  const long long total = (long long)gx * gy * n_frames;
  const dim3 grid(capped_grid(total, max_workgroups)), block(256);
  const int lv = levels < 4 ? levels : 4;
  // TAPS follows the role: the reference role always, the current role with the gathered taps, never without a role
  with_value<1, 0, -1>(role, [&](auto ROLE) {
    constexpr int kRole = decltype(ROLE)::value;
    auto launch = [&](auto TAPS) {
      with_value<3, 4, kChF32, 0>(colour_channels, [&](auto CH) {
        with_bool(depth_f32 || colour_channels == kChF32, [&](auto ZF) {
          with_bool(stream_nt, [&](auto NT) {
            constexpr int kCh = decltype(CH)::value;
            constexpr bool kZf = decltype(ZF)::value;
            if constexpr (kCh != kChF32 || kZf)
              k_ingest_strips<kRole, decltype(TAPS)::value, kCh, decltype(NT)::value, kZf>
                  <<<grid, block, 0, s>>>(tbl, scale, w0, h0, lv, ithr, dthr, gx, gy, n_frames, cur_flavor, c_levels);
          });
        });
      });
    };
    if constexpr (kRole == 1) launch(std::true_type{});
    else if constexpr (kRole == -1) launch(std::false_type{});
    else with_bool((cur_flavor & kCurAB) != 0, launch);
  });
}

}  // namespace dvo_hip
