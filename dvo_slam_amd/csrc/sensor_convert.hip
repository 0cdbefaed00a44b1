// sensor_convert.hip -- the sensor-format pass (sensor_formats.h; include/dvo_hip.h, DVO_HIP_PIXEL_BAYER_* / _YUYV8 / _UYVY8): the raw
// sensor planes of n frames of one size -> a tight plane of 8-bit grey each (OUT 0: one launch on the build stream at the head of
// frames_build, in front of the rig pass, the lens pass and the ingest, which then read a grey8 source) or of packed pixels 0x00RRGGBB
// (OUT 1: dvo_hip_frames_set_colour, straight into the frame's colour plane where k_colour_pack writes).
//
// A bandwidth kernel: grey mode reads 1 (Bayer) or 2 (YUV) B per pixel and writes 1.  A lane owns 4 consecutive pixels of a row, a
// wavefront 256 pixels of 4 consecutive rows, a workgroup of four wavefronts a 256 x 16 tile; the tiles are walked with a grid stride
// (option "build_workgroups" caps the grid like launch_rectify's).  No LDS, no barriers, no atomics, 256-thread workgroups.
//   loads    the lane's 4 (Bayer) or 8 (YUV) bytes of a row as aligned dwords where every plane's address and the pitch are 4-byte
//            aligned (SensorArgs::src_dwords, chosen per launch); else, and in the lane that holds a row's ragged end, byte by byte.  A
//            Bayer wavefront loads 6 rows for its 4 (the halo rows of neighbouring wavefronts meet in the CU's cache) and takes each
//            row's two halo columns from the neighbouring lanes' dwords; only a wavefront's first and last lane, and the lane at the
//            row's end, load theirs.  Every index is reflected / clamped into [0, w) x [0, h) BEFORE the address is formed: nothing is
//            read outside a plane's w x h pixels, not even a row's padding.
//   mosaic   a lane's x is a multiple of 4 and a wavefront's y too, so a site's phase is its position in the lane's 4 x 4 block against the
//            two wave-uniform pattern bits: the four patterns are one code path with selects (bayer_site).
//   stores   one dword of grey, or 16 bytes of packed pixels, per lane and row where w % 4 == 0 and the destination is aligned
//            (SensorArgs::dst_wide); else element by element.
// NT: planes read, and the converted plane written, with the non-temporal policy when the build stream's launches are ("stream_policy"):
// the plane is read back once, by the pass behind this one.
#include "dispatch.h"
#include "global_ptr.h"
#include "launch.h"
#include "sensor_formats.h"

namespace dvo_hip {

namespace {

constexpr int kSensorW = 256, kSensorRows = 4, kSensorH = 4 * kSensorRows;
typedef unsigned SensorU32x4 __attribute__((ext_vector_type(4)));

// index i of n samples reflected about the edge sample, and clamped: lanes and rows past the image address its last samples
__device__ __forceinline__ int sensor_index(int i, int n) {
  const int r = i < 0 ? -i : i >= n ? 2 * n - 2 - i : i;
  return min(max(r, 0), n - 1);
}

// the converted pixels x0 .. x0 + 3 of row y: one store where the plane allows it
template <int OUT, bool NT>
__device__ __forceinline__ void sensor_store(Global<uint8_t> dst, int w, int x0, int y, const SensorBgr (&c)[4], bool wide) {
  const size_t at = size_t(y) * size_t(w) + size_t(x0);
  if (OUT == 0) {
    unsigned g[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) g[m] = sensor_grey(c[m]);
    if (wide) {
      gst<NT>((Global<uint32_t>)(dst + at), uint32_t(g[0] | g[1] << 8 | g[2] << 16 | g[3] << 24));
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (x0 + m < w) gst<NT>(dst + at + m, uint8_t(g[m]));
    }
  } else {
    const auto out = (Global<uint32_t>)dst + at;
    if (wide) {
      gst<NT>((Global<SensorU32x4>)out, SensorU32x4{sensor_packed(c[0]), sensor_packed(c[1]), sensor_packed(c[2]), sensor_packed(c[3])});
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (x0 + m < w) gst<NT>(out + m, sensor_packed(c[m]));
    }
  }
}

// FMT: 0 = a Bayer mosaic, 1 = YUV 4:2:2 (pattern and byte order: a.format, wave-uniform).  OUT: 0 = grey8, 1 = packed pixels.
template <int FMT, int OUT, bool NT>
__global__ __launch_bounds__(256) void k_sensor_convert(const SensorPtrs* __restrict__ tbl, SensorArgs a, int tiles_x, int tiles_y, int n_frames) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int per_frame = tiles_x * tiles_y, total = per_frame * n_frames;
  const int w = a.w, h = a.h;
  const size_t pitch = size_t(a.pitch);
  const int red_x = bayer_red_x(a.format), red_y = bayer_red_y(a.format);
  const bool luma_first = yuv_luma_first(a.format);
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    const int frame = i / per_frame, t = i - frame * per_frame;
    const int bx = t % tiles_x, by = t / tiles_x;
    const int y0 = by * kSensorH + wave * kSensorRows;
    if (y0 >= h) continue;                                      // (wave-uniform; nothing below synchronises the workgroup)
    const SensorPtrs& f = tbl[frame];
    const auto src = global_ptr(f.src);
    const auto dst = (Global<uint8_t>)global_ptr(static_cast<uint8_t*>(f.dst));
    const int x0 = bx * kSensorW + 4 * lane;
    const bool whole = x0 + 3 < w;                              // the lane's 4 pixels lie inside the row
    const bool dwords = a.src_dwords != 0 && whole, wide = a.dst_wide != 0 && whole;
    SensorBgr c[4];
    if (FMT == 0) {
      // rows y0 - 1 .. y0 + 4 (reflected), columns x0 - 1 .. x0 + 4 (reflected): B(j, t) = the byte of register row j at column x0 - 1 + t
      int xs[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) xs[k] = sensor_index(x0 - 1 + k, w);
      unsigned mid[kSensorRows + 2], left[kSensorRows + 2], right[kSensorRows + 2];
      const bool left_lane = lane > 0, right_lane = lane < 63 && x0 + 4 < w;   // the halo column is a neighbouring lane's pixel
#pragma unroll
      for (int j = 0; j < kSensorRows + 2; ++j) {
        const auto row = src + size_t(sensor_index(y0 - 1 + j, h)) * pitch;   // (scalar)
        if (dwords) {
          mid[j] = gld<NT>((Global<const uint32_t>)(row + x0));
        } else {
          mid[j] = unsigned(gld<NT>(row + xs[1])) | unsigned(gld<NT>(row + xs[2])) << 8 | unsigned(gld<NT>(row + xs[3])) << 16 |
                   unsigned(gld<NT>(row + xs[4])) << 24;
        }
        left[j] = 0u;
        right[j] = 0u;
        if (!left_lane) left[j] = gld<NT>(row + xs[0]);
        if (!right_lane) right[j] = gld<NT>(row + xs[5]);
      }
#pragma unroll
      for (int j = 0; j < kSensorRows + 2; ++j) {
        const unsigned up = __shfl_up(mid[j], 1), down = __shfl_down(mid[j], 1);
        if (left_lane) left[j] = up >> 24;
        if (right_lane) right[j] = down & 0xffu;
      }
      auto B = [&](int j, int k) -> unsigned { return k == 0 ? left[j] : k == 5 ? right[j] : (mid[j] >> (8 * (k - 1))) & 0xffu; };
#pragma unroll
      for (int r = 0; r < kSensorRows; ++r) {
        const int y = y0 + r;
        if (y >= h) break;                                      // (wave-uniform)
#pragma unroll
        for (int m = 0; m < 4; ++m)                              // (x0 and y0 are multiples of 4: the site's phase is (m & 1, r & 1))
          c[m] = bayer_site((m & 1) ^ red_x, (r & 1) ^ red_y, B(r + 1, m + 1), B(r, m + 1), B(r + 2, m + 1), B(r + 1, m), B(r + 1, m + 2), B(r, m),
                            B(r, m + 2), B(r + 2, m), B(r + 2, m + 2));
        if (x0 < w) sensor_store<OUT, NT>(dst, w, x0, y, c, wide);
      }
    } else {
      // the lane's two pixel pairs of rows y0 .. y0 + 3 (w is even: a pair is inside or outside as a whole)
      unsigned p0[kSensorRows], p1[kSensorRows];
      const int xa = sensor_index(x0, w) & ~1, xb = sensor_index(x0 + 2, w) & ~1;
#pragma unroll
      for (int r = 0; r < kSensorRows; ++r) {
        const auto row = src + size_t(min(y0 + r, h - 1)) * pitch;   // (scalar)
        if (dwords) {
          p0[r] = gld<NT>((Global<const uint32_t>)(row + size_t(x0) * 2));
          p1[r] = gld<NT>((Global<const uint32_t>)(row + size_t(x0) * 2 + 4));
        } else {
          const auto a0 = row + size_t(xa) * 2, a1 = row + size_t(xb) * 2;
          p0[r] = unsigned(gld<NT>(a0)) | unsigned(gld<NT>(a0 + 1)) << 8 | unsigned(gld<NT>(a0 + 2)) << 16 | unsigned(gld<NT>(a0 + 3)) << 24;
          p1[r] = unsigned(gld<NT>(a1)) | unsigned(gld<NT>(a1 + 1)) << 8 | unsigned(gld<NT>(a1 + 2)) << 16 | unsigned(gld<NT>(a1 + 3)) << 24;
        }
      }
      const int sl = luma_first ? 0 : 8, sc = luma_first ? 8 : 0;   // bit of the first luma byte and of U in a pair's dword
#pragma unroll
      for (int r = 0; r < kSensorRows; ++r) {
        const int y = y0 + r;
        if (y >= h) break;                                      // (wave-uniform)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const unsigned p = m < 2 ? p0[r] : p1[r];
          c[m] = yuv_pixel(int(p >> (sl + 16 * (m & 1)) & 0xffu), int(p >> sc & 0xffu), int(p >> (sc + 16) & 0xffu));
        }
        if (x0 < w) sensor_store<OUT, NT>(dst, w, x0, y, c, wide);
      }
    }
  }
}

}  // namespace

bool sensor_src_dwords(const void* plane, size_t pitch) { return reinterpret_cast<uintptr_t>(plane) % 4 == 0 && pitch % 4 == 0; }

void launch_sensor_convert(hipStream_t s, const SensorPtrs* tbl, int n_frames, const SensorArgs& a, bool packed, int max_workgroups, bool stream_nt) {
  const int tx = (a.w + kSensorW - 1) / kSensorW, ty = (a.h + kSensorH - 1) / kSensorH;
  const long long total = (long long)tx * ty * n_frames;
  const dim3 grid(capped_grid(total, max_workgroups)), block(256);
  with_value<0, 1>(sensor_is_bayer(a.format) ? 0 : 1, [&](auto FMT) {
    with_bool(packed, [&](auto OUT) {
      with_bool(stream_nt, [&](auto NT) {
        k_sensor_convert<decltype(FMT)::value, int(decltype(OUT)::value), decltype(NT)::value><<<grid, block, 0, s>>>(tbl, a, tx, ty, n_frames);
      });
    });
  });
}

}  // namespace dvo_hip
