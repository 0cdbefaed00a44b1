"""CPU tier: surface normals in the keyframe map (dvo_slam_amd/csrc/cloud_normal.h), without a GPU.
  * cloud_normal.h with cloud_map.h, cloud_colour.h and map_render.h compiled for the host with g++ -Werror and -ffp-contract=off;
    frame_normals() and NormalHostMap below are the yardstick of tests/test_gpu_map_normals.py: a table and its side tables in host
    memory, filled, emptied, extracted and rendered with the headers' own functions;
  * analytic planes (an outside truth): every interior pixel has a normal, no border pixel has one, the frame normals lie within 1e-3 rad
    of the plane's and a voxel's extracted normal within 2.5e-3 rad (asin(sqrt(3) / (2 * 511)) = 1.7e-3 of quantisation plus the
    arithmetic); the sign, and that the world normal turns with the pose;
  * pixels without a normal (a NaN neighbour, a depth step) are still inserted; a thin wall seen from both sides has agreement near 0;
    the extremes of the sums; insert then remove restores the side table; the table does not depend on the pixel order;
  * the normals view's depth plane equals the grey view's, holes and normal-less voxels resolve to zeros;
  * the Python wrappers refuse before the library is reached; the header declares DVO_HIP_MAP_NORMALS 4u; the facade check compiles.
  * merge: a plain merge of two sub-maps equals the single build; a posed merge followed by a posed subtraction restores the destination;
    a posed merge under a quarter turn turns the extracted normals within the quantisation."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import test_cloud_map as tcm
import test_map_render as tmr
from dvo_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")
INF = float("inf")
HOLE = 0x7FC00000
FRAME_TOL = 1e-3            # rad: the issue's bound on a frame normal of an analytic plane
VOXEL_TOL = 2.5e-3          # rad: ... and on a voxel's extracted normal

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include <vector>
#include "cloud_colour.h"
#include "cloud_normal.h"
#include "map_render.h"
using namespace dvo_hip;
namespace {
// the world normal of pixel i as k_frame_normals and k_map_insert form it: neighbours are read only for an interior, usable pixel
bool pixel_normal(const MapPose& pose, const float* K, int w, int h, const float* Z, int i, bool usable, float N[3]) {
  N[0] = N[1] = N[2] = 0.0f;
  const int u = i % w, v = i / w;
  if (!usable || !normal_interior(w, h, u, v)) return false;
  float n[3];
  if (!normal_camera(K, u, v, Z[i], Z[i - 1], Z[i + 1], Z[i - w], Z[i + w], n)) return false;
  normal_world(pose, n, N);
  return true;
}
}
extern "C" {
int normals_host_slot_bytes() { return int(sizeof(MapNormalSlot)); }
float normals_host_min_cos() { return kNormalMinCos; }
uint32_t normals_host_quantise(float x) { return normal_quantise(x); }
float normals_host_dequantise(uint32_t q) { return normal_dequantise(q); }
void normals_host_extract_one(uint32_t snx, uint32_t sny, uint32_t snz, uint32_t nn, float* out) { normal_extract(snx, sny, snz, nn, out); }
uint64_t normals_host_render_value(uint64_t grey, uint32_t snx, uint32_t sny, uint32_t snz, uint32_t nn) { return normal_render_value(grey, snx, sny, snz, nn); }
// the organised normal plane {N.x, N.y, N.z, has} of a level
void normals_host_frame(const float* K, const double* T16, int w, int h, const float* Z, float min_depth, float max_depth, float* out) {
  const MapPose pose = map_pose_prepare(T16);
  for (int i = 0; i < w * h; ++i) {
    float P[3], N[3];
    const bool usable = map_world_point(pose, K, i % w, i / w, Z[i], min_depth, max_depth, P);
    const bool has = pixel_normal(pose, K, w, h, Z, i, usable, N);
    out[4 * i + 0] = N[0]; out[4 * i + 1] = N[1]; out[4 * i + 2] = N[2]; out[4 * i + 3] = has ? 1.0f : 0.0f;
  }
}
void normals_host_clear(MapSlot* slots, MapColourSlot* colour, MapNormalSlot* normals, uint64_t capacity, uint64_t* counters) {
  for (uint64_t i = 0; i < capacity; ++i) {
    std::memset(&slots[i], 0, sizeof(MapSlot));
    if (colour) std::memset(&colour[i], 0, sizeof(MapColourSlot));
    std::memset(&normals[i], 0, sizeof(MapNormalSlot));
    slots[i].key = kMapEmptyKey;
  }
  for (int i = 0; i < 8; ++i) counters[i] = 0;
}
// One frame into (sign +1) or out of (sign -1) the table, word by word as k_map_insert does it: {n, sx}, {sy, sz}, {sr, sg}, {snx, sny} and
// {snz, nn} as 64-bit two's-complement adds, si and sb as 32-bit ones.  colour / plane0 null: a map without colour.  counters: 0 usable
// points in range of the frames added, 1 dropped, 2 out of range, 3 unusable, 5 occupied slots, 6 points to remove, 7 of them unmatched.
void normals_host_update(MapSlot* slots, MapColourSlot* colour, MapNormalSlot* normals, uint64_t capacity, uint64_t* counters, float leaf,
                         const float* K, const double* T16, int w, int h, const float* I, const float* Z, const uint32_t* plane0, int w0, int shift,
                         float min_depth, float max_depth, int sign, int reverse) {
  const MapPose pose = map_pose_prepare(T16);
  const bool minus = sign < 0;
  for (int k = 0; k < w * h; ++k) {
    const int i = reverse ? w * h - 1 - k : k;
    float P[3], N[3];
    uint64_t key;
    uint32_t q[4];
    if (!map_world_point(pose, K, i % w, i / w, Z[i], min_depth, max_depth, P)) { counters[3] += minus ? uint64_t(0) - 1 : 1; continue; }
    if (!map_key_of(P, I[i], leaf, &key, q)) { counters[2] += minus ? uint64_t(0) - 1 : 1; continue; }
    counters[minus ? 6 : 0] += 1;
    const uint32_t c = colour ? colour_level(plane0, w0, i % w, i / w, shift) : 0u;
    const bool has = pixel_normal(pose, K, w, h, Z, i, true, N);
    uint64_t at = map_hash(key, capacity);
    bool placed = false;
    for (int p = 0; p < kMapMaxProbes && !placed; ++p, at = (at + 1) & (capacity - 1)) {
      MapSlot& s = slots[at];
      if (s.key == kMapEmptyKey) {
        if (minus) break;
        s.key = key;
        counters[5] += 1;
      }
      if (s.key != key) continue;
      uint64_t words[2], add[2] = {map_word(1u, q[0]), map_word(q[1], q[2])};
      std::memcpy(words, &s.n, 16);
      for (int j = 0; j < 2; ++j) words[j] += minus ? map_negate(add[j]) : add[j];
      std::memcpy(&s.n, words, 16);
      s.si += minus ? 0u - q[3] : q[3];
      if (colour) {
        uint64_t cw;
        std::memcpy(&cw, &colour[at], 8);
        const uint64_t ca = colour_word(colour_r(c), colour_g(c));
        cw += minus ? map_negate(ca) : ca;
        std::memcpy(&colour[at], &cw, 8);
        colour[at].sb += minus ? 0u - colour_b(c) : colour_b(c);
      }
      if (has) {
        uint64_t nw[2];
        const uint64_t na[2] = {normal_word(normal_quantise(N[0]), normal_quantise(N[1])), normal_word(normal_quantise(N[2]), 1u)};
        std::memcpy(nw, &normals[at], 16);
        for (int j = 0; j < 2; ++j) nw[j] += minus ? map_negate(na[j]) : na[j];
        std::memcpy(&normals[at], nw, 16);
      }
      placed = true;
    }
    if (!placed) counters[minus ? 7 : 1] += 1;
  }
}
// live slots in table order; returns their number.  rgba null: not wanted (or no colour)
uint64_t normals_host_extract(const MapSlot* slots, const MapColourSlot* colour, const MapNormalSlot* normals, uint64_t capacity, float leaf,
                              float* xyzi, float* nrm, uint32_t* rgba, uint32_t* counts, uint64_t* keys, uint32_t* nn) {
  uint64_t n = 0;
  for (uint64_t i = 0; i < capacity; ++i) {
    const MapSlot& s = slots[i];
    if (!map_slot_live(s.key, s.n)) continue;
    map_extract_voxel(s.key, s.n, s.sx, s.sy, s.sz, s.si, leaf, xyzi + 4 * n);
    normal_extract(normals[i].snx, normals[i].sny, normals[i].snz, normals[i].nn, nrm + 4 * n);
    if (rgba) rgba[n] = colour_extract(s.n, colour[i].sr, colour[i].sg, colour[i].sb);
    counts[n] = s.n;
    keys[n] = s.key;
    nn[n] = normals[i].nn;
    ++n;
  }
  return n;
}
// `count` records (a table: its capacity) into (sign +1) or out of (-1) the table, as k_map_merge does in its NORMALS instantiations; T16
// null: a plain merge; else posed, the records binned with leaf_src.  carry_oor / carry_unusable: the counts a plain merge from a MAP
// carries along.  src_colour null: no colour.
void normals_host_merge(MapSlot* slots, MapColourSlot* colour, MapNormalSlot* normals, uint64_t capacity, uint64_t* counters, float leaf,
                        const MapSlot* src, const MapColourSlot* src_colour, const MapNormalSlot* src_normals, uint64_t count, float leaf_src, int sign,
                        const double* T16, uint64_t carry_oor, uint64_t carry_unusable) {
  const bool minus = sign < 0;
  MapPose pose;
  std::memset(&pose, 0, sizeof pose);
  if (T16) pose = map_pose_prepare(T16);
  counters[2] += minus ? uint64_t(0) - carry_oor : carry_oor;
  counters[3] += minus ? uint64_t(0) - carry_unusable : carry_unusable;
  for (uint64_t i = 0; i < count; ++i) {
    const MapSlot& r = src[i];
    if (!map_slot_live(r.key, r.n)) continue;
    uint64_t key = r.key;
    uint32_t add[5] = {r.n, r.sx, r.sy, r.sz, r.si};
    if (T16) {
      const int how = map_pose_record(pose, r.key, r.n, r.sx, r.sy, r.sz, r.si, leaf_src, leaf, &key, add);
      if (how == kMapPoseUnusable) { counters[3] += minus ? uint64_t(0) - r.n : uint64_t(r.n); continue; }
      if (how == kMapPoseOutOfRange) { counters[2] += minus ? uint64_t(0) - r.n : uint64_t(r.n); continue; }
    }
    uint32_t facing[4] = {src_normals[i].snx, src_normals[i].sny, src_normals[i].snz, src_normals[i].nn};
    if (T16 && facing[3] != 0u) normal_pose_sums(pose, facing[0], facing[1], facing[2], facing[3], facing);
    counters[minus ? 6 : 0] += r.n;
    uint64_t at = map_hash(key, capacity);
    bool placed = false;
    for (int p = 0; p < kMapMaxProbes && !placed; ++p, at = (at + 1) & (capacity - 1)) {
      MapSlot& s = slots[at];
      if (s.key == kMapEmptyKey) {
        if (minus) break;
        s.key = key;
        counters[5] += 1;
      }
      if (s.key != key) continue;
      uint64_t words[2], a2[2] = {map_word(add[0], add[1]), map_word(add[2], add[3])};
      std::memcpy(words, &s.n, 16);
      for (int j = 0; j < 2; ++j) words[j] += minus ? map_negate(a2[j]) : a2[j];
      std::memcpy(&s.n, words, 16);
      s.si += minus ? 0u - add[4] : add[4];
      if (colour) {
        uint64_t cw;
        std::memcpy(&cw, &colour[at], 8);
        const uint64_t ca = colour_word(src_colour[i].sr, src_colour[i].sg);
        cw += minus ? map_negate(ca) : ca;
        std::memcpy(&colour[at], &cw, 8);
        colour[at].sb += minus ? 0u - src_colour[i].sb : src_colour[i].sb;
      }
      uint64_t nw[2];
      const uint64_t na[2] = {normal_word(facing[0], facing[1]), normal_word(facing[2], facing[3])};
      std::memcpy(nw, &normals[at], 16);
      for (int j = 0; j < 2; ++j) nw[j] += minus ? map_negate(na[j]) : na[j];
      std::memcpy(&normals[at], nw, 16);
      placed = true;
    }
    if (!placed) counters[minus ? 7 : 1] += r.n;
  }
}
void normals_host_pose_sums(const double* T16, uint32_t snx, uint32_t sny, uint32_t snz, uint32_t nn, uint32_t* out) {
  normal_pose_sums(map_pose_prepare(T16), snx, sny, snz, nn, out);
}
// the normals views of the table: what k_map_render (NORMALS) and k_render_resolve_normals do
void normals_host_render(const MapSlot* slots, const MapNormalSlot* normals, uint64_t capacity, const RenderArgs* a, const float* K, int w, int h,
                         const double* poses, int n_views, float* nrm, uint32_t* Z) {
  for (int k = 0; k < n_views; ++k) {
    const MapView view = map_view_prepare(poses + 16 * k, K, w, h);
    std::vector<uint64_t> z(size_t(w) * h, kRenderEmpty);
    for (uint64_t j = 0; j < capacity; ++j) {
      const MapSlot& s = slots[j];
      RenderFootprint f;
      if (s.key == kMapEmptyKey || !map_render_voxel(view, *a, s.key, s.n, s.sx, s.sy, s.sz, s.si, &f)) continue;
      const uint64_t value = normal_render_value(f.value, normals[j].snx, normals[j].sny, normals[j].snz, normals[j].nn);
      for (int v = f.v0; v <= f.v1; ++v)
        for (int u = f.u0; u <= f.u1; ++u) {
          uint64_t& e = z[size_t(v) * w + u];
          if (value < e) e = value;
        }
    }
    for (size_t i = 0; i < z.size(); ++i) normal_render_resolve(z[i], view, nrm + 4 * (size_t(k) * w * h + i), Z + size_t(k) * w * h + i);
  }
}
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    """cloud_normal.h compiled for the host: g++, every warning an error, no contraction"""
    tmp = tempfile.mkdtemp(prefix="map_normals_host_")
    src, out = os.path.join(tmp, "map_normals_host.cpp"), os.path.join(tmp, "map_normals_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    fp, dp, vp, u64, u32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p, C.c_uint64, C.c_uint32
    L.normals_host_min_cos.restype = C.c_float
    L.normals_host_quantise.argtypes = [C.c_float]
    L.normals_host_quantise.restype = u32
    L.normals_host_dequantise.argtypes = [u32]
    L.normals_host_dequantise.restype = C.c_float
    L.normals_host_extract_one.argtypes = [u32, u32, u32, u32, vp]
    L.normals_host_extract_one.restype = None
    L.normals_host_render_value.argtypes = [u64, u32, u32, u32, u32]
    L.normals_host_render_value.restype = u64
    L.normals_host_frame.argtypes = [fp, dp, C.c_int, C.c_int, fp, C.c_float, C.c_float, vp]
    L.normals_host_frame.restype = None
    L.normals_host_clear.argtypes = [vp, vp, vp, u64, vp]
    L.normals_host_clear.restype = None
    L.normals_host_update.argtypes = [vp, vp, vp, u64, vp, C.c_float, fp, dp, C.c_int, C.c_int, fp, fp, vp, C.c_int, C.c_int, C.c_float, C.c_float,
                                      C.c_int, C.c_int]
    L.normals_host_update.restype = None
    L.normals_host_extract.argtypes = [vp, vp, vp, u64, C.c_float, vp, vp, vp, vp, vp, vp]
    L.normals_host_extract.restype = u64
    L.normals_host_merge.argtypes = [vp, vp, vp, u64, vp, C.c_float, vp, vp, vp, u64, C.c_float, C.c_int, dp, u64, u64]
    L.normals_host_merge.restype = None
    L.normals_host_pose_sums.argtypes = [dp, u32, u32, u32, u32, vp]
    L.normals_host_pose_sums.restype = None
    L.normals_host_render.argtypes = [vp, vp, u64, C.POINTER(tmr.RenderArgs), fp, C.c_int, C.c_int, dp, C.c_int, vp, vp]
    L.normals_host_render.restype = None
    assert L.normals_host_slot_bytes() == 16
    return L


def frame_normals(Z, K, T, min_depth=0.0, max_depth=INF):
    """the organised plane [h, w, 4] {N.x, N.y, N.z, has} of the level's depth plane Z with intrinsics K under pose T, as cloud_normal.h
    defines it, computed on the host"""
    h, w = Z.shape
    out = np.empty((h, w, 4), np.float32)
    (ki, kp), (ti, tp), (zi, zp) = tcm._f(K), tcm._d(T), tcm._f(Z)
    host_lib().normals_host_frame(kp, tp, w, h, zp, min_depth, max_depth, out.ctypes.data)
    return out


class NormalHostMap:
    """the yardstick of a map with normals (colour=True: and with colour): the tables of cloud_map.h, cloud_colour.h and cloud_normal.h
    in host memory"""

    def __init__(self, leaf, capacity, colour=False):
        self.leaf = float(np.float32(leaf))
        self.capacity = 64
        while self.capacity < capacity:
            self.capacity *= 2
        self.slots = np.empty(self.capacity * 32, np.uint8)
        self.colour = np.empty(self.capacity * 4, np.uint32) if colour else None
        self.normals = np.empty(self.capacity * 4, np.uint32)
        self.counters = np.zeros(8, np.uint64)
        self.clear()

    def _colour_ptr(self):
        return self.colour.ctypes.data if self.colour is not None else None

    def clear(self):
        host_lib().normals_host_clear(self.slots.ctypes.data, self._colour_ptr(), self.normals.ctypes.data, self.capacity, self.counters.ctypes.data)

    def update(self, I, Z, K, T, plane0=None, level=0, sign=1, min_depth=0.0, max_depth=INF, reverse=False):
        """the level's planes I, Z [h, w] with intrinsics K under pose T; a map with colour: coloured from the LEVEL-0 plane plane0"""
        h, w = Z.shape
        assert (plane0 is not None) == (self.colour is not None)
        pp, w0 = None, 0
        if plane0 is not None:
            plane0 = np.ascontiguousarray(plane0, np.uint32)
            assert plane0.shape[0] >> level == h and plane0.shape[1] >> level == w
            pp, w0 = plane0.ctypes.data, plane0.shape[1]
        (ki, kp), (ti, tp), (ii, ip), (zi, zp) = tcm._f(K), tcm._d(T), tcm._f(I), tcm._f(Z)
        host_lib().normals_host_update(self.slots.ctypes.data, self._colour_ptr(), self.normals.ctypes.data, self.capacity, self.counters.ctypes.data,
                                       self.leaf, kp, tp, w, h, ip, zp, pp, w0, level, min_depth, max_depth, sign, 1 if reverse else 0)
        return self

    def insert(self, *args, **kw):
        return self.update(*args, sign=1, **kw)

    def remove(self, *args, **kw):
        return self.update(*args, sign=-1, **kw)

    def stats(self):
        c = [int(x) for x in self.counters]
        return dict(points=c[0] - c[1] - (c[6] - c[7]), dropped=c[1], out_of_range=c[2], unusable=c[3], occupied=c[5], removed=c[6] - c[7],
                    unmatched=c[7], capacity=self.capacity)

    def extract(self, with_nn=False):
        """(xyzi, counts, keys[, rgba], normals) of the live voxels, sorted by key -- what KeyframeMap.extract(sort=True, normals=True
        [, colour=True]) returns; with_nn: and nn [n] uint32, the points that had a normal, last"""
        n = self.capacity
        xyzi, nrm, rgba = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32), np.empty(n, np.uint32)
        counts, keys, nn = np.empty(n, np.uint32), np.empty(n, np.uint64), np.empty(n, np.uint32)
        got = int(host_lib().normals_host_extract(self.slots.ctypes.data, self._colour_ptr(), self.normals.ctypes.data, self.capacity, self.leaf,
                                                  xyzi.ctypes.data, nrm.ctypes.data, rgba.ctypes.data if self.colour is not None else None,
                                                  counts.ctypes.data, keys.ctypes.data, nn.ctypes.data))
        order = np.argsort(keys[:got], kind="stable")
        out = [xyzi[:got][order], counts[:got][order], keys[:got][order]]
        if self.colour is not None:
            out.append(rgba[:got][order])
        out.append(nrm[:got][order])
        if with_nn:
            out.append(nn[:got][order])
        return tuple(out)

    def render(self, K, w, h, poses, **params):
        """(normals [n, h, w, 4] float32, Z [n, h, w] float32) of the normals views"""
        K, T = tmr._views(K, poses)
        nrm, Z = np.empty((len(T), h, w, 4), np.float32), np.empty((len(T), h, w), np.float32)
        a = tmr._args(self.leaf, params)
        host_lib().normals_host_render(self.slots.ctypes.data, self.normals.ctypes.data, self.capacity, C.byref(a), K.ctypes.data_as(C.POINTER(C.c_float)),
                                       w, h, T.ctypes.data_as(C.POINTER(C.c_double)), len(T), nrm.ctypes.data, Z.ctypes.data)
        return nrm, Z

    def merge(self, src, sign=1, pose=None):
        """another NormalHostMap's table into (sign +1) or out of (-1) this one: plain (pose None; the source's out-of-range and unusable
        counts come along), or posed under the 4 x 4 pose"""
        assert (src.colour is None) == (self.colour is None)
        tp = None if pose is None else tcm._d(pose)[1]
        carry = (0, 0) if pose is not None else (int(src.counters[2]), int(src.counters[3]))
        host_lib().normals_host_merge(self.slots.ctypes.data, self._colour_ptr(), self.normals.ctypes.data, self.capacity, self.counters.ctypes.data,
                                      self.leaf, src.slots.ctypes.data, src._colour_ptr(), src.normals.ctypes.data, src.capacity, src.leaf, sign, tp,
                                      carry[0], carry[1])
        return self

    def records(self):
        """(records, colour records or None, normal records) of the live voxels, sorted by key: what KeyframeMap.export() returns, sorted"""
        rec = self.slots.view(np.dtype(_lib.MAP_RECORD))
        live = (rec["key"] != np.uint64(0xFFFFFFFFFFFFFFFF)) & (rec["n"] > 0)
        order = np.argsort(rec["key"][live], kind="stable")
        colour = None if self.colour is None else self.colour.view(np.dtype(_lib.MAP_COLOUR_RECORD))[live][order]
        return rec[live][order], colour, self.normals.view(np.dtype(_lib.MAP_NORMAL_RECORD))[live][order]

    def grey_table(self):
        """the slot table as a tests/test_cloud_map.py HostMap (what a map without the flag fed the same frames holds)"""
        m = tcm.HostMap(self.leaf, self.capacity)
        m.slots[:] = self.slots
        m.counters[:6] = [self.counters[0], self.counters[1], self.counters[2], self.counters[3], 0, self.counters[5]]
        return m


def assert_normal_maps_identical(a, b, what=""):
    """two sorted extractions with normals (xyzi, counts, keys, ..., normals): identical bit for bit"""
    tcm.assert_maps_identical(a, b, what)
    assert len(a) == len(b)
    for x, y in zip(a[3:], b[3:]):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype.itemsize == 4 and np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: the side tables' records differ" % (what,)


# ---- analytic planes ----------------------------------------------------------------------------------------------------------------------

W, H = 64, 48
K_PLANE = np.array([0.8 * W, 0.8 * W, W / 2 - 0.5, H / 2 - 0.5], np.float32)
AXIS = np.array([0.6, 0.8, 0.0])                            # oblique, in the image plane


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def plane_depth(tilt_deg, w=W, h=H, K=K_PLANE, dist=1.5):
    """(Z [h, w] float32, n [3] float64): the depth plane of a plane through (0, 0, dist) whose normal is (0, 0, -1) tilted about AXIS, and
    that normal (facing the camera), in float64"""
    n = rotation(AXIS, np.deg2rad(tilt_deg)) @ np.array([0.0, 0.0, -1.0])
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    K = K.astype(np.float64)
    rays = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], -1)
    Z = (n[2] * dist) / (rays @ n)
    cos = -(rays @ n) / np.linalg.norm(rays, axis=-1)
    assert np.degrees(np.arccos(cos.min())) < 80.0             # every ray meets the plane at under 80 degrees
    return Z.astype(np.float32), n


def angle_to(N, n):
    """the angle [rad] between the rows of N and the unit vector n, accurate near 0"""
    N = np.asarray(N, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(N, n), axis=-1), N @ n)


def pose_of(R=np.eye(3), t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


@pytest.mark.parametrize("tilt", [0, 20, 40])
def test_analytic_plane_every_interior_pixel_has_the_planes_normal(tilt):
    Z, n = plane_depth(tilt)
    rec = frame_normals(Z, K_PLANE, np.eye(4))
    has = rec[..., 3]
    assert set(np.unique(has)) <= {0.0, 1.0}
    assert np.all(has[1:-1, 1:-1] == 1.0)                        # none may be left out
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert np.all(has[border] == 0.0) and np.all(rec[border][:, :3] == 0.0)
    err = angle_to(rec[1:-1, 1:-1, :3].reshape(-1, 3), n)
    print("tilt %d: frame normals within %.3g rad of the plane's (bound %.3g)" % (tilt, err.max(), FRAME_TOL))
    assert err.max() < FRAME_TOL
    assert np.all(rec[1:-1, 1:-1, 2] < 0)                        # facing the camera
    assert np.abs(np.linalg.norm(rec[1:-1, 1:-1, :3].astype(np.float64), axis=-1) - 1).max() < 1e-6
    # the extracted normal of every voxel that holds one
    m = NormalHostMap(0.05, 1 << 14).insert(np.full((H, W), 100.0, np.float32), Z, K_PLANE, np.eye(4))
    xyzi, counts, keys, nrm, nn = m.extract(with_nn=True)
    assert int(nn.sum()) == (H - 2) * (W - 2) and int(counts.sum()) == H * W
    held = nn > 0
    assert held.sum() > 100
    verr = angle_to(nrm[held, :3], n)
    print("tilt %d: voxel normals within %.3g rad (bound %.3g), agreement %.5f .. %.5f" % (tilt, verr.max(), VOXEL_TOL, nrm[held, 3].min(), nrm[held, 3].max()))
    assert verr.max() < VOXEL_TOL
    assert np.all(np.abs(nrm[held, 3] - 1.0) < 4e-3)             # a flat patch: agreement 1 within the quantisation
    assert np.all(nrm[~held] == 0.0)


def test_sign_and_the_world_normal_turns_with_the_pose():
    Z, n = plane_depth(20)
    cam = frame_normals(Z, K_PLANE, np.eye(4))[1:-1, 1:-1, :3].reshape(-1, 3)
    assert np.all(cam[:, 2] < 0)
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])                    # the camera turned by 90 degrees about y
    world = frame_normals(Z, K_PLANE, pose_of(R, (0.3, -0.2, 0.1)))[1:-1, 1:-1, :3].reshape(-1, 3)
    assert angle_to(world, R @ n).max() < FRAME_TOL
    # an axis permutation is exact in float: N = (n.z, n.y, -n.x), the translation does not enter
    assert np.array_equal(world[:, 0], cam[:, 2]) and np.array_equal(world[:, 1], cam[:, 1]) and np.array_equal(world[:, 2], -cam[:, 0])


def test_pixels_without_a_normal_are_still_inserted():
    Z, n = plane_depth(0)
    Zh = Z.copy()
    Zh[20, 30] = np.nan
    rec = frame_normals(Zh, K_PLANE, np.eye(4))
    gone = [(20, 30), (20, 29), (20, 31), (19, 30), (21, 30)]                             # the hole and its four neighbours
    for v in range(1, H - 1):
        for u in range(1, W - 1):
            assert (rec[v, u, 3] == 0.0) == ((v, u) in gone), (v, u)
    m = NormalHostMap(8.0, 64).insert(np.zeros((H, W), np.float32), Zh, K_PLANE, pose_of(t=(4.0, 4.0, 1.0)))
    xyzi, counts, keys, nrm, nn = m.extract(with_nn=True)
    assert len(keys) == 1 and counts[0] == H * W - 1 and nn[0] == (H - 2) * (W - 2) - 5 and nn[0] < counts[0]
    # a neighbour out of the DEPTH RANGE still serves: the range is applied to the pixel itself only
    Zr = Z.copy()
    Zr[20, 30] = 1.5 * 1.001
    rec = frame_normals(Zr, K_PLANE, np.eye(4), 0.5, 1.5005)
    assert rec[20, 30, 3] == 0.0 and rec[20, 29, 3] == 1.0 and rec[19, 30, 3] == 1.0


def test_a_depth_step_of_thirty_per_cent_gives_no_normal():
    # (the focal length of a 640-wide level 0, where a step above roughly 4 % of the depth looks like a surface seen at over 84 degrees;
    # with the 51-pixel focal length of K_PLANE two pixels are so far apart that a 30 % step is a 81-degree slope and keeps its normal)
    K_step = np.array([525.0, 525.0, W / 2 - 0.5, H / 2 - 0.5], np.float32)
    Z = np.full((H, W), 1.0, np.float32)
    Z[:, 32:] = 1.3
    assert frame_normals(Z, K_PLANE, np.eye(4))[20, 31, 3] == 1.0
    rec = frame_normals(Z, K_step, np.eye(4))
    assert np.all(rec[1:-1, 31:33, 3] == 0.0)                   # the two columns whose stencil straddles the step
    assert np.all(rec[1:-1, 1:31, 3] == 1.0) and np.all(rec[1:-1, 33:-1, 3] == 1.0)
    assert abs(host_lib().normals_host_min_cos() - 0.1) < 1e-8


def test_a_thin_wall_seen_from_both_sides_has_agreement_near_zero():
    Z = np.full((H, W), 1.0, np.float32)
    I = np.zeros((H, W), np.float32)
    front = pose_of(t=(4.0, 4.0, 0.0))
    back = pose_of(np.diag([-1.0, 1.0, -1.0]), (4.0, 4.0, 2.0))                           # half a turn about y: the same wall from behind
    one = NormalHostMap(8.0, 64).insert(I, Z, K_PLANE, front)
    both = NormalHostMap(8.0, 64).insert(I, Z, K_PLANE, front).insert(I, Z, K_PLANE, back)
    a = one.extract(with_nn=True)
    b = both.extract(with_nn=True)
    assert len(a[2]) == 1 and len(b[2]) == 1 and b[1][0] == 2 * H * W and b[4][0] == 2 * (H - 2) * (W - 2)
    assert a[3][0, 3] > 0.999 and a[3][0, 2] < -0.999
    assert b[3][0, 3] < 0.01


def test_extremes_of_the_sums():
    L = host_lib()
    out = np.empty(4, np.float32)
    n = 1 << 20
    L.normals_host_extract_one(1022 * n, 511 * n, 511 * n, n, out.ctypes.data)            # 2^20 points facing +x: nothing wraps
    assert 1022 * n < 1 << 30 and out.tolist() == [1.0, 0.0, 0.0, 1.0]
    L.normals_host_extract_one(1022 * n, 1022 * n, 1022 * n, n, out.ctypes.data)
    assert np.allclose(out[:3], 1 / np.sqrt(3), atol=1e-7)
    L.normals_host_extract_one(1022, 511, 511, 1, out.ctypes.data)                        # one point
    assert out.tolist() == [1.0, 0.0, 0.0, 1.0]
    L.normals_host_extract_one(0, 511, 511, 1, out.ctypes.data)
    assert out.tolist() == [-1.0, 0.0, 0.0, 1.0]
    L.normals_host_extract_one(0, 0, 0, 0, out.ctypes.data)                               # no point with a normal
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0]
    L.normals_host_extract_one(511 * 2, 511 * 2, 511 * 2, 2, out.ctypes.data)             # opposite normals: no direction left
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0]
    # the quantisation: biased, clamped, symmetric; a NaN is 0
    assert [L.normals_host_quantise(x) for x in (-1.0, 0.0, 1.0, -7.0, 7.0, float("nan"))] == [0, 511, 1022, 0, 1022, 0]
    assert L.normals_host_quantise(0.5 / 511) == 512 and L.normals_host_quantise(-0.5 / 511 - 1e-6) == 510
    assert [L.normals_host_dequantise(q) for q in (0, 511, 1022)] == [-1.0, 0.0, 1.0]
    # the view payload: the depth half is kept, a voxel without a normal carries 0
    grey = 0x3f80000012345678
    assert L.normals_host_render_value(grey, 0, 0, 0, 0) == 0x3f80000000000000
    assert L.normals_host_render_value(grey, 1022, 511, 511, 1) == 0x3f80000000000000 | 1 << 30 | 1022 << 20 | 511 << 10 | 511


def scene_views(w, h):
    return tcm.float_views(w, h)


def test_insert_then_remove_restores_the_side_table():
    K, views = scene_views(102, 78)
    m = NormalHostMap(0.02, 1 << 16)
    for I, Z, T in views:
        m.insert(I, Z, K, T)
    slots, normals = m.slots.copy(), m.normals.copy()
    before = m.extract()
    assert (before[3][:, 3] > 0).sum() > 500 and (before[3][:, 3] == 0).sum() > 10        # voxels with a normal, and without
    I, Z, T = views[0]
    T = T @ tcm.scenes.se3_exp([0.03, -0.02, 0.01, 0.01, -0.02, 0.015])
    m.insert(I, Z, K, T)
    assert not np.array_equal(m.normals, normals)
    m.remove(I, Z, K, T)
    s = m.stats()
    assert s["unmatched"] == 0 and s["removed"] > 1000
    assert np.array_equal(m.normals, normals)                    # every word, vacant slots (zeros) included
    live = m.slots.view(np.uint32).reshape(-1, 8)[:, 2] > 0
    assert np.array_equal(m.slots.reshape(-1, 32)[live], slots.reshape(-1, 32)[live])
    assert_normal_maps_identical(m.extract(), before, "after the removal")


@pytest.mark.parametrize("level", [0, 1])
def test_the_table_does_not_depend_on_the_pixel_order(level):
    K, views = scene_views(102, 78)
    Kl = np.array(K, np.float32) / np.float32(1 << level) if level else K
    s = 1 << level
    planes = [(np.ascontiguousarray(I[::s, ::s][:78 >> level, :102 >> level]), np.ascontiguousarray(Z[::s, ::s][:78 >> level, :102 >> level]), T)
              for I, Z, T in views]
    fwd, rev = NormalHostMap(0.05, 1 << 14), NormalHostMap(0.05, 1 << 14)
    for I, Z, T in planes:
        fwd.insert(I, Z, Kl, T)
    for I, Z, T in reversed(planes):
        rev.insert(I, Z, Kl, T, reverse=True)
    a, b = fwd.extract(with_nn=True), rev.extract(with_nn=True)
    assert len(a[2]) > 300 and (a[1] > 1).sum() > 50 and (a[4] > 1).sum() > 50
    assert_normal_maps_identical(a, b, "forward against reversed")
    # the slots are those of a map without the flag fed the same frames
    grey = tcm.HostMap(0.05, 1 << 14)
    for I, Z, T in planes:
        grey.insert(I, Z, Kl, T)
    tcm.assert_maps_identical(a, grey.extract(), "the map without normals")


# ---- merge --------------------------------------------------------------------------------------------------------------------------------

def test_a_plain_merge_of_two_sub_maps_equals_the_single_build():
    K, views = scene_views(102, 78)
    single, a, b, dst = (NormalHostMap(0.02, 1 << 16) for _ in range(4))
    for I, Z, T in views:
        single.insert(I, Z, K, T)
    a.insert(*views[0][:2], K, views[0][2])
    b.insert(*views[1][:2], K, views[1][2])
    dst.merge(a).merge(b)
    assert_normal_maps_identical(dst.extract(with_nn=True), single.extract(with_nn=True), "a + b against the single build")
    assert dst.stats() == single.stats()
    for x, y in zip(dst.records(), single.records()):
        assert (x is None and y is None) or np.array_equal(x, y)
    # ... and taking one out again leaves the other, word for word in the side table
    dst.merge(b, sign=-1)
    assert_normal_maps_identical(dst.extract(with_nn=True), a.extract(with_nn=True), "(a + b) - b")
    live = dst.slots.view(np.uint32).reshape(-1, 8)[:, 2] > 0
    assert np.all(dst.normals.reshape(-1, 4)[~live] == 0)


def test_a_posed_merge_and_its_subtraction_restore_the_destination():
    K, views = scene_views(102, 78)
    dst, sub = NormalHostMap(0.02, 1 << 16), NormalHostMap(0.03, 1 << 16)
    dst.insert(*views[0][:2], K, views[0][2])
    sub.insert(*views[1][:2], K, np.eye(4))                     # a sub-map in its anchor's coordinates
    slots, normals, before = dst.slots.copy(), dst.normals.copy(), dst.extract(with_nn=True)
    pose = views[1][2]
    dst.merge(sub, pose=pose)
    assert not np.array_equal(dst.normals, normals) and dst.stats()["points"] > int(before[1].sum())
    twice = NormalHostMap(0.02, 1 << 16)
    twice.insert(*views[0][:2], K, views[0][2]).merge(sub, pose=pose)
    assert np.array_equal(twice.normals, dst.normals) and np.array_equal(twice.slots, dst.slots)   # deterministic
    dst.merge(sub, sign=-1, pose=pose)
    assert dst.stats()["unmatched"] == 0
    assert np.array_equal(dst.normals, normals)
    live = dst.slots.view(np.uint32).reshape(-1, 8)[:, 2] > 0
    assert np.array_equal(dst.slots.reshape(-1, 32)[live], slots.reshape(-1, 32)[live])
    assert_normal_maps_identical(dst.extract(with_nn=True), before, "after the posed subtraction")


def test_a_posed_merge_under_a_quarter_turn_turns_the_normals():
    Z, n = plane_depth(20)
    sub = NormalHostMap(0.05, 1 << 14).insert(np.full((H, W), 100.0, np.float32), Z, K_PLANE, np.eye(4))
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    dst = NormalHostMap(0.05, 1 << 14).merge(sub, pose=pose_of(R, (0.5, 0.25, -0.125)))
    xyzi, counts, keys, nrm, nn = dst.extract(with_nn=True)
    assert int(counts.sum()) == H * W and int(nn.sum()) == (H - 2) * (W - 2)
    held = nn > 0
    assert held.sum() > 100 and angle_to(nrm[held, :3], R @ n).max() < VOXEL_TOL
    # a quarter turn permutes the sums exactly: s' = (snz, sny, 1022 nn - snx)
    out = np.empty(3, np.uint32)
    host_lib().normals_host_pose_sums(tcm._d(pose_of(R))[1], 700, 600, 400, 2, out.ctypes.data)
    assert out.tolist() == [400, 600, 2 * 1022 - 700]
    host_lib().normals_host_pose_sums(tcm._d(pose_of(3.0 * np.eye(3)))[1], 2044, 0, 1022, 2, out.ctypes.data)   # clamped into [0, 1022 nn]
    assert out.tolist() == [2044, 0, 1022]


def test_normals_view_shares_the_depth_plane_and_zeroes_holes_and_normal_less_voxels():
    K, views = scene_views(102, 78)
    m = NormalHostMap(0.02, 1 << 16)
    for I, Z, T in views:
        m.insert(I, Z, K, T)
    Kv = np.array([70.0, 70.0, 39.5, 29.5], np.float32)
    poses = np.stack([views[0][2], views[1][2]])
    for params in ({}, dict(max_splat=1)):
        nrm, Z = m.render(Kv, 80, 60, poses, **params)
        I_grey, Z_grey = tmr.render_host_map(m.grey_table(), Kv, 80, 60, poses, **params)
        assert np.array_equal(Z.view(np.uint32), Z_grey.view(np.uint32))
        hole = Z.view(np.uint32) == HOLE
        assert hole.any() and (~hole).sum() > 1000
        assert np.all(nrm[hole] == 0.0)
        has = nrm[..., 3]
        assert set(np.unique(has)) <= {0.0, 1.0} and (has == 1.0).sum() > 500
        bare = ~hole & (has == 0.0)
        assert bare.any() and np.all(nrm[bare] == 0.0)           # voxels none of whose points had a normal are drawn, with their Z
        length = np.linalg.norm(nrm[has == 1.0][:, :3].astype(np.float64), axis=-1)
        assert np.abs(length - 1).max() < np.sqrt(3) / (2 * 511) + 1e-6
    # seen from the poses the frames were taken at, most normals face the camera
    nrm, Z = m.render(Kv, 80, 60, poses, max_splat=1)
    seen = nrm[nrm[..., 3] == 1.0]
    assert (seen[:, 2] < 0).mean() > 0.95


def test_a_view_turns_the_normal_into_its_camera():
    Z, n = plane_depth(20)
    R = rotation([0.0, 1.0, 0.0], 0.3)
    T = pose_of(R, (0.2, 0.0, -0.1))
    m = NormalHostMap(0.02, 1 << 14).insert(np.full((H, W), 50.0, np.float32), Z, K_PLANE, T)
    nrm, Zv = m.render(K_PLANE, W, H, T[None], max_splat=1)
    seen = nrm[0][nrm[0, ..., 3] == 1.0][:, :3]
    assert len(seen) > 500
    # world normal R n, back through the view's R^T: n again, to the voxel tolerance plus the payload's quantisation
    assert angle_to(seen, n).max() < VOXEL_TOL + np.sqrt(3) / (2 * 511)


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------------

CTX = "ctx"


class FakeCamera:
    def __init__(self, w, h):
        self.width, self.height = w, h


class FakePyr:
    """enough of a pyramid for the argument checks; a call that reached the library would fail on ctx"""

    def __init__(self, w=64, h=48, ctx=CTX):
        self.camera, self.ctx, self.ptr, self.levels = FakeCamera(w, h), ctx, None, 3


def fake_map(normals, colour=False):
    m = object.__new__(d.KeyframeMap)
    m.coloured, m.with_normals, m.ptr, m.ctx = colour, normals, None, CTX
    return m


def test_a_map_without_normals_asked_for_them_refuses_before_the_library():
    m = fake_map(False)
    with pytest.raises(ValueError):
        m.extract(normals=True)
    with pytest.raises(ValueError):
        m.render_normals([60, 60, 31.5, 23.5], 64, 48, np.eye(4))
    with pytest.raises(TypeError):
        d.KeyframeMap(ctx="ctx", normals=1)
    with pytest.raises(TypeError):
        d.KeyframeMap(ctx="ctx", colour=False, normals="yes")
    with_normals = fake_map(True)
    with pytest.raises(ValueError):
        with_normals.extract(colour=True, normals=True)                                   # no colour in this one
    with pytest.raises(ValueError):
        with_normals.render_normals([60, 60, 31.5, 23.5], 64, 48, np.eye(4), max_splat=2)
    with pytest.raises(ValueError):
        with_normals.render_normals([60, -60, 31.5, 23.5], 64, 48, np.eye(4))
    with pytest.raises(ValueError):
        with_normals.render_normals([60, 60, 31.5, 23.5], 64, 0, np.eye(4))
    with pytest.raises(ValueError):
        with_normals.render_normals([60, 60, 31.5, 23.5], 64, 48, np.eye(3))
    with pytest.raises(TypeError):
        with_normals.render_normals([60, 60, 31.5, 23.5], 64, 48, np.eye(4), reserved=1)


def test_normals_batch_rejects_bad_arguments_before_the_library():
    p = FakePyr()
    with pytest.raises(ValueError):
        d.normals_batch([], np.zeros((0, 4, 4)))
    with pytest.raises(ValueError):
        d.normals_batch([p], np.eye(3)[None])
    with pytest.raises(ValueError):
        d.normals_batch([p, FakePyr()], np.eye(4)[None])
    with pytest.raises(ValueError):
        d.normals_batch([p], np.eye(4)[None], level=3)
    with pytest.raises(TypeError):
        d.normals_batch([p], np.eye(4)[None], level=1.0)
    with pytest.raises(ValueError):
        d.normals_batch([p], np.eye(4)[None], min_depth=2.0, max_depth=1.0)
    with pytest.raises(ValueError):
        d.normals_batch([p], np.eye(4)[None], min_depth=float("nan"))
    with pytest.raises(ValueError):
        d.normals_batch([p, FakePyr(ctx="other")], np.stack([np.eye(4)] * 2))


def test_sub_map_wrappers_refuse_mismatched_maps_and_records_before_the_library():
    m, other, plain = fake_map(True), fake_map(True), fake_map(False)
    for x in (m, other, plain):
        x.leaf, x.ptr = 0.01, C.c_void_p(1)                      # (open maps; a call that reached the library would fail on ctx)
    rec = np.zeros(1, np.dtype(_lib.MAP_RECORD))
    nrec = np.zeros(1, np.dtype(_lib.MAP_NORMAL_RECORD))
    for call in (lambda: plain.merge([other]), lambda: m.merge([plain]), lambda: m.move_submaps([plain], np.eye(4)[None], np.eye(4)[None]),
                 lambda: m.absorb(rec), lambda: plain.absorb(rec, normals=nrec), lambda: m.absorb(rec, normals=np.zeros(2, np.dtype(_lib.MAP_NORMAL_RECORD)))):
        with pytest.raises(ValueError, match="normal"):
            call()
    with pytest.raises(TypeError):
        m.absorb(rec, normals=np.zeros(1, np.dtype(_lib.MAP_COLOUR_RECORD)))                # not the normal record's fields
    with pytest.raises(TypeError):
        m.absorb(rec, normals=np.zeros((1, 4), np.uint32))


def test_header_and_bindings_declare_the_normals_entry_points():
    text = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    for name in ("dvo_hip_frames_normals", "dvo_hip_map_extract_normals", "dvo_hip_map_render_normals", "dvo_hip_map_export_ex",
                 "dvo_hip_map_merge_records_ex"):
        assert "int %s(dvo_hip_context* ctx" % name in text and name in _lib.EXPORTS
    assert "#define DVO_HIP_MAP_NORMALS 4u" in text and _lib.MAP_NORMALS == 4
    assert "#define DVO_HIP_MAP_COLOUR 1u" in text
    # flags = 2 stays an unknown flag that is refused, and the header says so at the define
    at = text.index("#define DVO_HIP_MAP_NORMALS 4u")
    assert "flags = 2" in text[at - 400:at] and "refused" in text[at - 400:at]
    capi = open(os.path.join(CSRC, "capi_map.inc")).read()
    assert 'flags & ~(DVO_HIP_MAP_COLOUR | DVO_HIP_MAP_NORMALS)) return fail(ctx, DVO_HIP_ERR_INVALID, "map_create: unknown flag")' in capi
    assert (_lib.MAP_COLOUR | _lib.MAP_NORMALS) & 2 == 0
    # dvo_hip_render_params is unchanged: five fields and three reserved words
    assert C.sizeof(_lib.RenderParams) == 32
    d.build()
    L = C.CDLL(d.LIB_PATH)
    for name in _lib.EXPORTS:
        assert hasattr(L, name), name


# ---- the C++ facade -----------------------------------------------------------------------------------------------------------------------

def build_map_normals_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "map_normals_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "map_normals_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_normals_classes_compile():
    d.build()
    assert os.path.exists(build_map_normals_facade_check())
