// map_render.hip -- views of the keyframe map on the device (map_render.h; include/dvo_hip.h, dvo_hip_map_render and
// dvo_hip_map_render_frames): the table of a map -> tight float planes I and Z of n views, the nearest voxel per pixel.  Three launches
// on the context's main stream.
//
// k_render_fill stores ~0 into the z-buffers of all views, which lie behind one another in one block: 16 B per lane (two elements),
// grid-stride, and one lane for the odd element at the end.
// k_map_render is the splat: the grid's y is the view, its x strides over the table; a lane owns one slot of the table in one view, a
// wavefront 64 consecutive slots.  An empty slot costs its 8-byte key; an occupied one the other
// 24 bytes, the extraction of its record (double, as k_map_extract) and the projection, all in registers.  The footprint loop -- at most
// max_splat x max_splat pixels, bounded by kRenderMaxSplat -- issues one 64-bit vector memory atomic per covered pixel whose return
// value is not used (unsigned minimum, relaxed, agent scope), as k_depth_register does with 32 bits.  Nothing waits or retries; the
// minimum over integers does not depend on the order of arrival.  PRELOAD (DVO_RENDER_PRELOAD=1 at build time; off by default, not
// measured) reads the element first with a plain load and skips the atomic when it is already smaller or equal: an element only falls,
// so a stale value can only send a lane to the atomic, which decides.
// k_render_resolve turns the z-buffer into the planes: 8 B read, 4 B stored to I and 4 B to Z per pixel, a lane per pixel, a wavefront
// 64 consecutive pixels (256 contiguous bytes per plane), the view again in the grid's y.  No LDS, no barriers, 256-thread workgroups.
// A colour view (cloud_colour.h; dvo_hip_map_render_colour) runs the COLOUR instantiations: the splat reads 16 more bytes per live voxel
// (the side table's sums) and puts the voxel's colour where the intensity's bits were -- the depth half of the element, the footprint and
// the atomic are the grey view's -- and the resolve stores the colour word in place of I.
// A normals view (cloud_normal.h; dvo_hip_map_render_normals) runs the NORMALS instantiation of the splat: 16 more bytes per live voxel
// (the normal side table's sums), the voxel's quantised world normal where the intensity's bits were; k_render_resolve_normals rotates
// it into the view and stores one 16-byte record per pixel beside Z.
#include "global_ptr.h"
#include "launch.h"
#include "map_render.h"
#include "cloud_normal.h"

#ifndef DVO_RENDER_PRELOAD
#define DVO_RENDER_PRELOAD 0
#endif

namespace dvo_hip {

namespace {

typedef unsigned GlobalU32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_render_fill(unsigned long long* __restrict__ zbuf, long long elements) {
  const long long pairs = elements >> 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const GlobalU32x4 empty = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  const auto Z = (Global<GlobalU32x4>)global_ptr(reinterpret_cast<GlobalU32x4*>(zbuf));   // (the block is 256-byte aligned: hipMalloc)
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += stride) Z[i] = empty;
  // the tail: the last element of an odd count
  if ((elements & 1) && blockIdx.x == 0 && threadIdx.x == 0) zbuf[elements - 1] = kRenderEmpty;
}

template <bool PRELOAD, bool COLOUR, bool NORMALS = false>
__global__ __launch_bounds__(256) void k_map_render(MapTable m, const MapView* __restrict__ views, int n_views, RenderArgs a,
                                                    unsigned long long* __restrict__ zbuf) {
#pragma clang fp contract(off)
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  const int max_splat = a.max_splat < kRenderMaxSplat ? a.max_splat : kRenderMaxSplat;
  // the grid's y is the view (no division per slot); more views than the grid is high are walked
  for (int view = int(blockIdx.y); view < n_views; view += int(gridDim.y)) {
    const MapView& v = views[view];                            // (view < n_views: inside the table of views)
    unsigned long long* plane = zbuf + (size_t)view * ((size_t)v.w * (size_t)v.h);
    for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; at < m.capacity; at += stride) {   // (at < capacity: inside the table)
      const auto words = (Global<const GlobalU32x2>)global_ptr(reinterpret_cast<const GlobalU32x2*>(m.slots + at));
      const GlobalU32x2 k = words[0];
      const unsigned long long key = (unsigned long long)k.x | (unsigned long long)k.y << 32;
      if (key == kMapEmptyKey) continue;
      const GlobalU32x2 ns = words[1], yz = words[2], ip = words[3];   // n sx | sy sz | si pad
      RenderFootprint f;
      if (!map_render_voxel(v, a, key, ns.x, ns.y, yz.x, yz.y, ip.x, &f)) continue;
      if constexpr (COLOUR) {
        const GlobalU32x4 t = *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.colour + at));   // sr sg sb pad
        f.value = colour_render_value(f.value, colour_extract(ns.x, t.x, t.y, t.z));   // (drawn: n >= min_points >= 1)
      }
      if constexpr (NORMALS) {
        const GlobalU32x4 t = *(Global<const GlobalU32x4>)global_ptr(reinterpret_cast<const GlobalU32x4*>(m.normals + at));   // snx sny snz nn
        f.value = normal_render_value(f.value, t.x, t.y, t.z, t.w);
      }
      // f lies inside the image (map_render_axis clips): 0 <= u0 <= u1 <= w - 1, 0 <= v0 <= v1 <= h - 1
      const int nu = f.u1 - f.u0 + 1, nv = f.v1 - f.v0 + 1;
      for (int dy = 0; dy < max_splat; ++dy) {
        if (dy >= nv) break;
        unsigned long long* row = plane + (size_t)(f.v0 + dy) * (size_t)v.w + (size_t)f.u0;
        for (int dx = 0; dx < max_splat; ++dx) {
          if (dx >= nu) break;
          if constexpr (PRELOAD) {
            if (__hip_atomic_load(row + dx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= f.value) continue;
          }
          (void)__hip_atomic_fetch_min(row + dx, (unsigned long long)f.value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
}

template <bool COLOUR>
__global__ __launch_bounds__(256) void k_render_resolve(const unsigned long long* __restrict__ zbuf, const RenderPlanes* __restrict__ out, int n_views,
                                                        long long pixels) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (int view = int(blockIdx.y); view < n_views; view += int(gridDim.y)) {   // (view < n_views: inside the tables)
    const auto E = (Global<const GlobalU32x2>)global_ptr(reinterpret_cast<const GlobalU32x2*>(zbuf + (size_t)view * (size_t)pixels));
    const auto Iout = (Global<float>)global_ptr(out[view].I);
    const auto Zout = (Global<float>)global_ptr(out[view].Z);
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += stride) {   // (p < pixels: inside the view's planes)
      const GlobalU32x2 e = E[p];
      if constexpr (COLOUR) {
        uint32_t rgba, z;
        colour_render_resolve((unsigned long long)e.x | (unsigned long long)e.y << 32, &rgba, &z);
        Iout[p] = __uint_as_float(rgba);                       // (the plane is the caller's uint32 plane: the bits are stored as they are)
        Zout[p] = __uint_as_float(z);
      } else {
        float I, Z;
        map_render_resolve((unsigned long long)e.x | (unsigned long long)e.y << 32, &I, &Z);
        Iout[p] = I;
        Zout[p] = Z;
      }
    }
  }
}

// the normals view's resolve: 8 B read, one 16-byte record {n.x, n.y, n.z, has} (the view's camera coordinates) and 4 B of Z stored per pixel
__global__ __launch_bounds__(256) void k_render_resolve_normals(const unsigned long long* __restrict__ zbuf, const MapView* __restrict__ views,
                                                                const RenderPlanes* __restrict__ out, int n_views, long long pixels) {
#pragma clang fp contract(off)
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (int view = int(blockIdx.y); view < n_views; view += int(gridDim.y)) {   // (view < n_views: inside the tables)
    const MapView& v = views[view];
    const auto E = (Global<const GlobalU32x2>)global_ptr(reinterpret_cast<const GlobalU32x2*>(zbuf + (size_t)view * (size_t)pixels));
    const auto Nout = (Global<GlobalF32x4>)global_ptr(reinterpret_cast<GlobalF32x4*>(out[view].I));
    const auto Zout = (Global<float>)global_ptr(out[view].Z);
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += stride) {   // (p < pixels: inside the view's planes)
      const GlobalU32x2 e = E[p];
      float n[4];
      uint32_t z;
      normal_render_resolve((unsigned long long)e.x | (unsigned long long)e.y << 32, v, n, &z);
      const GlobalF32x4 rec = {n[0], n[1], n[2], n[3]};
      Nout[p] = rec;
      Zout[p] = __uint_as_float(z);
    }
  }
}

// x: grid-stride over the items of one view, y: the views (at most 1024 rows; the kernels walk the rest)
dim3 view_grid(long long items, int n_views) {
  long long blocks = (items + 255) / 256;
  const int rows = n_views < 1024 ? n_views : 1024;
  const long long cap = 8192 / rows > 64 ? 8192 / rows : 64;
  blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
  return dim3(unsigned(blocks), unsigned(rows));
}

}  // namespace

void launch_render_fill(hipStream_t s, unsigned long long* zbuf, long long elements) {
  k_render_fill<<<dim3(stride_grid(elements >> 1)), dim3(256), 0, s>>>(zbuf, elements);
}

void launch_render_splat(hipStream_t s, const MapTable& m, const MapView* views, int n_views, const RenderArgs& a, unsigned long long* zbuf, bool colour) {
  const dim3 grid = view_grid((long long)m.capacity, n_views), block(256);
  if (colour) k_map_render<DVO_RENDER_PRELOAD != 0, true><<<grid, block, 0, s>>>(m, views, n_views, a, zbuf);
  else k_map_render<DVO_RENDER_PRELOAD != 0, false><<<grid, block, 0, s>>>(m, views, n_views, a, zbuf);
}

void launch_render_resolve(hipStream_t s, const unsigned long long* zbuf, const RenderPlanes* out, int n_views, long long pixels, bool colour) {
  const dim3 grid = view_grid(pixels, n_views), block(256);
  if (colour) k_render_resolve<true><<<grid, block, 0, s>>>(zbuf, out, n_views, pixels);
  else k_render_resolve<false><<<grid, block, 0, s>>>(zbuf, out, n_views, pixels);
}

void launch_map_render(hipStream_t s, const MapTable& m, const MapView* views, const RenderPlanes* out, int n_views, long long pixels, const RenderArgs& a,
                       unsigned long long* zbuf, bool colour) {
  launch_render_fill(s, zbuf, pixels * n_views);
  launch_render_splat(s, m, views, n_views, a, zbuf, colour);
  launch_render_resolve(s, zbuf, out, n_views, pixels, colour);
}

void launch_map_render_normals(hipStream_t s, const MapTable& m, const MapView* views, const RenderPlanes* out, int n_views, long long pixels,
                               const RenderArgs& a, unsigned long long* zbuf) {
  launch_render_fill(s, zbuf, pixels * n_views);
  k_map_render<DVO_RENDER_PRELOAD != 0, false, true><<<view_grid((long long)m.capacity, n_views), dim3(256), 0, s>>>(m, views, n_views, a, zbuf);
  k_render_resolve_normals<<<view_grid(pixels, n_views), dim3(256), 0, s>>>(zbuf, views, out, n_views, pixels);
}

bool map_render_preloads() { return DVO_RENDER_PRELOAD != 0; }

}  // namespace dvo_hip
