"""CPU tier: views of the keyframe map (dvo_slam_amd/csrc/map_render.h), without a GPU.
  * map_render.h (the functions k_map_render and k_render_resolve inline) compiled for the host with g++ -Werror and -ffp-contract=off,
    with the HostMap of tests/test_cloud_map.py as the table; render_host() below is the yardstick of tests/test_gpu_map_render.py;
  * the planes do not depend on the order the voxels are visited in, nor on the order the map was filled in;
  * a fronto-parallel plane is rendered without holes, at its depth;
  * the nearer of two surfaces wins, and of two voxels at one depth the one with the lower intensity;
  * a single voxel covers exactly the pixels the header defines: the empty range, the cap, the four image edges, the skipped voxels;
  * accuracy on the project's scene: coverage and depth error of a render against the view it was built from; tracking a frame against
    the rendered model with the oracle, against the true pose;
  * the Python wrappers reject bad arguments before anything reaches the library; the C++ facade compiles
    (tests/cpp/map_render_facade_check.cpp)."""
import ctypes as C
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import scenes
import test_cloud_map as tcm
from dvo_slam_amd import tracker
from test_cloud_map import HostMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")
INF = float("inf")
HOLE = 0x7FC00000
DEFAULTS = dict(min_depth=0.0, max_depth=INF, splat=2.0, max_splat=7, min_points=1)

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include <vector>
#include "map_render.h"
using namespace dvo_hip;
namespace {
uint64_t splat(std::vector<uint64_t>& z, int w, const RenderFootprint& f) {
  uint64_t updates = 0;
  for (int v = f.v0; v <= f.v1; ++v)
    for (int u = f.u0; u <= f.u1; ++u, ++updates) {
      uint64_t& e = z[size_t(v) * w + u];
      if (f.value < e) e = f.value;
    }
  return updates;
}
void resolve(const std::vector<uint64_t>& z, float* I, float* Z) {
  for (size_t i = 0; i < z.size(); ++i) map_render_resolve(z[i], I + i, Z + i);
}
}
extern "C" {
// n records {x, y, z, I} with their point counts, visited in the order `order` (n indexes), into n_views views; returns the number of
// covered-pixel updates (every pixel of every footprint)
uint64_t render_host_records(const float* xyzi, const uint32_t* counts, const int64_t* order, uint64_t n, const RenderArgs* a, const float* K, int w, int h,
                             const double* poses, int n_views, float* I, float* Z) {
  uint64_t updates = 0;
  for (int k = 0; k < n_views; ++k) {
    const MapView view = map_view_prepare(poses + 16 * k, K, w, h);
    std::vector<uint64_t> z(size_t(w) * h, kRenderEmpty);
    for (uint64_t j = 0; j < n; ++j) {
      RenderFootprint f;
      const int64_t i = order[j];
      if (map_render_record(view, *a, xyzi + 4 * i, counts[i], &f)) updates += splat(z, w, f);
    }
    resolve(z, I + size_t(k) * w * h, Z + size_t(k) * w * h);
  }
  return updates;
}
// the same from the table itself, its slots visited in the order `order` (capacity indexes): what k_map_render does
uint64_t render_host_table(const MapSlot* slots, const int64_t* order, uint64_t capacity, const RenderArgs* a, const float* K, int w, int h,
                           const double* poses, int n_views, float* I, float* Z) {
  uint64_t updates = 0;
  for (int k = 0; k < n_views; ++k) {
    const MapView view = map_view_prepare(poses + 16 * k, K, w, h);
    std::vector<uint64_t> z(size_t(w) * h, kRenderEmpty);
    for (uint64_t j = 0; j < capacity; ++j) {
      const MapSlot& s = slots[order[j]];
      RenderFootprint f;
      if (s.key != kMapEmptyKey && map_render_voxel(view, *a, s.key, s.n, s.sx, s.sy, s.sz, s.si, &f)) updates += splat(z, w, f);
    }
    resolve(z, I + size_t(k) * w * h, Z + size_t(k) * w * h);
  }
  return updates;
}
int render_host_args_bytes() { return int(sizeof(RenderArgs)); }
int render_host_max_splat() { return kRenderMaxSplat; }
}
"""


class RenderArgs(C.Structure):
    _fields_ = [("min_depth", C.c_float), ("max_depth", C.c_float), ("splat", C.c_float), ("leaf", C.c_float), ("max_splat", C.c_int),
                ("min_points", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def host_lib():
    """map_render.h compiled for the host: g++, every warning an error, no contraction (what the header's pragma says to clang)"""
    tmp = tempfile.mkdtemp(prefix="map_render_host_")
    src, out = os.path.join(tmp, "map_render_host.cpp"), os.path.join(tmp, "map_render_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    fp, dp, vp, u64 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p, C.c_uint64
    L.render_host_records.argtypes = [vp, vp, vp, u64, C.POINTER(RenderArgs), fp, C.c_int, C.c_int, dp, C.c_int, vp, vp]
    L.render_host_records.restype = u64
    L.render_host_table.argtypes = [vp, vp, u64, C.POINTER(RenderArgs), fp, C.c_int, C.c_int, dp, C.c_int, vp, vp]
    L.render_host_table.restype = u64
    assert L.render_host_args_bytes() == C.sizeof(RenderArgs) and L.render_host_max_splat() == 15
    return L


def _args(leaf, params):
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **params)
    return RenderArgs(p["min_depth"], p["max_depth"], p["splat"], float(np.float32(leaf)), p["max_splat"], p["min_points"])


def _views(K, poses):
    K = np.ascontiguousarray(K, np.float32).reshape(4)
    T = np.ascontiguousarray(poses, np.float64)
    if T.ndim == 2:
        T = T[None]
    assert T.shape[1:] == (4, 4)
    return K, T


def render_host(xyzi, counts, leaf, K, w, h, poses, order=None, want_updates=False, **params):
    """render_host(): the planes (I, Z) [n, h, w] of the records (xyzi [m, 4], counts [m]) -- a map's extraction -- seen from the poses,
    as map_render.h defines them, computed on the host; order: the order the records are visited in"""
    xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
    assert len(xyzi) == len(counts)
    order = np.arange(len(counts), dtype=np.int64) if order is None else np.ascontiguousarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(len(counts)))
    K, T = _views(K, poses)
    I, Z = np.empty((len(T), h, w), np.float32), np.empty((len(T), h, w), np.float32)
    a = _args(leaf, params)
    updates = host_lib().render_host_records(xyzi.ctypes.data, counts.ctypes.data, order.ctypes.data, len(counts), C.byref(a),
                                             K.ctypes.data_as(C.POINTER(C.c_float)), w, h, T.ctypes.data_as(C.POINTER(C.c_double)), len(T),
                                             I.ctypes.data, Z.ctypes.data)
    return (I, Z, int(updates)) if want_updates else (I, Z)


def render_host_map(m, K, w, h, poses, order=None, **params):
    """... of a HostMap's table, its slots visited in `order`"""
    order = np.arange(m.capacity, dtype=np.int64) if order is None else np.ascontiguousarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(m.capacity))
    K, T = _views(K, poses)
    I, Z = np.empty((len(T), h, w), np.float32), np.empty((len(T), h, w), np.float32)
    a = _args(m.leaf, params)
    host_lib().render_host_table(m.slots.ctypes.data, order.ctypes.data, m.capacity, C.byref(a), K.ctypes.data_as(C.POINTER(C.c_float)), w, h,
                                 T.ctypes.data_as(C.POINTER(C.c_double)), len(T), I.ctypes.data, Z.ctypes.data)
    return I, Z


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def holes(Z):
    return Z.view(np.uint32) == HOLE


# ---- 1. order independence ------------------------------------------------------------------------------------------------------------

def test_planes_do_not_depend_on_the_order_of_the_voxels_or_of_the_insertions():
    K, views = tcm.float_views(128, 96)
    leaf, cap = 0.02, 1 << 16
    forward, backward = HostMap(leaf, cap), HostMap(leaf, cap)
    for I, Z, T in views:
        forward.insert(I, Z, K, T)
    for I, Z, T in reversed(views):
        backward.insert(I, Z, K, T, reverse=True)
    poses = np.stack([views[0][2], views[1][2] @ scenes.se3_exp([0.03, -0.02, 0.01, 0.02, -0.03, 0.015])])
    want = render_host_map(forward, K, 128, 96, poses)
    assert holes(want[1]).any() and (~holes(want[1])).sum() > 0.5 * want[1].size
    assert np.all(want[0][holes(want[1])] == 0.0) and np.all(want[1][~holes(want[1])] > 0)
    n = forward.capacity
    shuffled = np.random.default_rng(7).permutation(n)
    for what, m, order in (("backwards", forward, np.arange(n)[::-1]), ("shuffled", forward, shuffled), ("filled in another order", backward, None),
                           ("filled in another order, shuffled", backward, shuffled)):
        assert same_bits(render_host_map(m, K, 128, 96, poses, order), want), what
    # the records of the extraction are what the table's slots give: the GPU tier's yardstick is fed the device map's extraction
    xyzi, counts, keys, over = forward.extract()
    assert same_bits(render_host(xyzi, counts, leaf, K, 128, 96, poses), want)
    assert same_bits(render_host(xyzi, counts, leaf, K, 128, 96, poses, order=np.random.default_rng(8).permutation(len(counts))), want)
    # two views in one call are the two single calls
    for k in range(2):
        one = render_host(xyzi, counts, leaf, K, 128, 96, poses[k])
        assert same_bits((one[0][0], one[1][0]), (want[0][k], want[1][k]))


# ---- 2. a fronto-parallel plane -------------------------------------------------------------------------------------------------------

def test_a_fronto_parallel_plane_has_no_holes_and_its_depth():
    """A plane at depth d = 2, inserted from the identity pose at 64 x 48 (fx = fy = 50), leaf 0.08, rendered from the identity with the
    default parameters.  L = leaf * fx / d = 2 pixels is the leaf's size in the image, the pixels' points lie d / fx = 0.04 = leaf / 2
    apart in X and in Y and all at z = d.

    No hole.  Along an axis the voxels form a row of cells of L pixels, and every cell that a pixel's point falls into is occupied.  Its
    centroid (cloud_map.h: the mean of the offsets truncated to leaf / 1024, plus half a step) lies inside the cell, so two neighbouring
    centroids project less than 2 L apart; the footprints are hx = splat * 0.5 * L = L wide on each side with the default splat = 2, so
    consecutive footprints [u' - hx, u' + hx] overlap (2 hx = 2 L > the gap), and their union is one interval.  It starts left of pixel
    0: pixel 0's point lies in the first occupied cell, whose other points lie to its right by less than L, so the first centroid
    projects to u' < 0 + L and u' - hx < 0; likewise on the right.  Every pixel centre in the image therefore lies in some footprint
    -- provided no footprint is cut by max_splat: a footprint covers at most floor(2 hx) + 1 = 5 <= 7 pixels.  The claim needs
    splat >= 2 when the centroids may lie anywhere in their cells, which is the default; the issue's border of ceil(hx) pixels is not
    needed (asserted: no hole at all), and is granted to the assertion on the interior.  Rounding: u' is computed in float32 with an
    error of a few 1e-6 pixels, far below the overlap, which is at least 2 L / 1024 (the centroid cannot reach the cell's faces).

    Depth.  All points have z = d, so per voxel the z offsets are one value q, and the extracted z = (iz + (q + 0.5) / 1024) * leaf lies
    within leaf / 2048 of d (truncation to leaf / 1024, half a step added back), rounded to float32 once: plus one ulp of d.  From the
    identity p.z = ((0 x + 0 y) + 1 z) + (-0) = z exactly."""
    w, h, d_, leaf = 64, 48, 2.0, 0.08
    K = np.array([50.0, 50.0, 31.5, 23.5], np.float32)
    y, x = np.mgrid[0:h, 0:w]
    I = ((x * 3 + y * 7) % 256).astype(np.float32)
    m = HostMap(leaf, 1 << 12).insert(I, np.full((h, w), d_, np.float32), K, np.eye(4))
    assert m.stats()["dropped"] == 0 and m.stats()["points"] == w * h
    Ir, Zr = render_host_map(m, K, w, h, np.eye(4))
    hx = DEFAULTS["splat"] * 0.5 * leaf * float(K[0]) / d_
    assert math.floor(2 * hx) + 1 <= DEFAULTS["max_splat"]
    b = math.ceil(hx)
    assert not holes(Zr[0])[b:h - b, b:w - b].any()
    assert not holes(Zr[0]).any()
    tol = float(np.float32(leaf)) / 2048 + float(np.spacing(np.float32(d_)))
    assert np.abs(Zr[0].astype(np.float64) - d_).max() <= tol
    assert Ir[0].min() >= 0.0 and Ir[0].max() <= 255.0 and np.unique(Ir[0]).size > 50
    # a footprint much narrower than the leaf leaves holes on the same map: one pixel per voxel, where a voxel spans two
    assert holes(render_host_map(m, K, w, h, np.eye(4), splat=0.4)[1]).any()


# ---- 3. occlusion ---------------------------------------------------------------------------------------------------------------------

def records(points):
    """records (xyzi, counts) of hand-made voxels [(x, y, z, I, n)]"""
    p = np.array(points, np.float64).reshape(-1, 5)
    return p[:, :4].astype(np.float32), p[:, 4].astype(np.uint32)


def test_the_near_surface_wins_and_equal_depths_go_to_the_lower_intensity():
    w, h, leaf, d_ = 64, 48, 0.08, 1.5
    K = np.array([50.0, 50.0, 31.5, 23.5], np.float32)
    near, far = HostMap(leaf, 1 << 12), HostMap(leaf, 1 << 12)
    both = HostMap(leaf, 1 << 12)
    Zn = np.full((h, w), np.nan, np.float32)
    Zn[:, :40] = d_                                                 # the near plane covers the left of the image
    Zf = np.full((h, w), 2 * d_, np.float32)
    In, If = np.full((h, w), 200.0, np.float32), np.full((h, w), 50.0, np.float32)
    for m, planes in ((near, [(In, Zn)]), (far, [(If, Zf)]), (both, [(If, Zf), (In, Zn)])):
        for I, Z in planes:
            m.insert(I, Z, K, np.eye(4))
    (_, zn), (_, zf), (ib, zb) = (render_host_map(m, K, w, h, np.eye(4)) for m in (near, far, both))
    covered = ~holes(zn[0])
    assert covered.sum() > 30 * h and (~covered).sum() > 15 * h and not holes(zf[0]).any()
    assert np.array_equal(zb[0][covered], zn[0][covered]) and np.all(ib[0][covered] == 200.0)      # near wins wherever both land
    assert np.array_equal(zb[0][~covered], zf[0][~covered]) and np.all(ib[0][~covered] == 50.0)
    assert np.all(zb[0][covered] < 1.6) and np.all(zb[0][~covered] > 2.9)
    # equal depths: the lower intensity wins, whatever the order; a negative intensity counts as 0 and a NaN too
    for lo, hi in ((10.0, 20.0), (0.0, 0.5), (-3.0, 1.0)):
        xyzi, counts = records([(0.0, 0.0, 2.0, hi, 1), (0.01, 0.0, 2.0, lo, 1)])
        a = render_host(xyzi, counts, leaf, K, w, h, np.eye(4))
        b_ = render_host(xyzi, counts, leaf, K, w, h, np.eye(4), order=[1, 0])
        assert same_bits(a, b_)
        shared = (a[1][0] == 2.0)
        assert shared.sum() >= 4 and np.all(a[0][0][shared] == max(lo, 0.0))
    xyzi, counts = records([(0.0, 0.0, 2.0, np.nan, 1)])
    a = render_host(xyzi, counts, leaf, K, w, h, np.eye(4))
    assert np.all(a[0][0][a[1][0] == 2.0] == 0.0) and (a[1][0] == 2.0).sum() >= 4


# ---- 4. the footprint -----------------------------------------------------------------------------------------------------------------

def footprint(uc, vc, z, leaf, K, w, h, **params):
    """the pixels [(u, v)] one voxel leaves, placed so that it projects to (uc, vc) at depth z from the identity pose"""
    K = np.asarray(K, np.float32)
    x = (np.float64(uc) - K[2]) * z / K[0]
    y = (np.float64(vc) - K[3]) * z / K[1]
    xyzi, counts = records([(x, y, z, 7.0, params.pop("n", 1))])
    I, Z = render_host(xyzi, counts, leaf, K, w, h, np.eye(4), **params)
    vs, us = np.nonzero(~holes(Z[0]))
    assert np.all(Z[0][vs, us] == np.float32(z)) and np.all(I[0][vs, us] == 7.0) and np.all(I[0][holes(Z[0])] == 0.0)
    return sorted(zip(us.tolist(), vs.tolist()))


def box(u0, u1, v0, v1):
    return sorted((u, v) for u in range(u0, u1 + 1) for v in range(v0, v1 + 1))


def test_a_single_voxel_covers_exactly_the_pixels_of_the_definition():
    """K = (64, 64, 16, 12), z = 2, leaf 1 / 16: hx = splat * 0.5 * leaf * fx / z = splat exactly, and every quantity below is a
    dyadic fraction: the voxel's position, its projection and the bounds are exact in float32."""
    K, w, h, leaf = [64.0, 64.0, 16.0, 12.0], 32, 24, 1.0 / 16
    f = functools.partial(footprint, z=2.0, leaf=leaf, K=K, w=w, h=h)
    # splat 2: hx = 2.  u' = 10.25: [ceil(8.25), floor(12.25)] = 9 .. 12; v' = 6: [4, 8] (a centre on the footprint's edge is covered)
    assert f(10.25, 6.0) == box(9, 12, 4, 8)
    assert f(10.5, 6.5) == box(9, 12, 5, 8)
    # splat 0.25: hx = 0.25.  u' = 10.5: [ceil(10.25), floor(10.75)] is empty -> the nearest pixel floor(11.0) = 11; v' = 6.25: [6, 6]
    assert f(10.5, 6.25, splat=0.25) == [(11, 6)]
    assert f(10.4375, 6.75, splat=0.25) == [(10, 7)]              # empty on both axes: floor(10.9375) = 10, [6.5, 7] -> 7
    # the cap: splat 4 -> hx = 4, 9 pixels a side uncut; max_splat 7, 3, 1 keep 7, 3, 1 around the nearest pixel
    assert f(10.0, 6.0, splat=4.0, max_splat=9) == box(6, 14, 2, 10)
    assert f(10.0, 6.0, splat=4.0) == box(7, 13, 3, 9)
    assert f(10.0, 6.0, splat=4.0, max_splat=3) == box(9, 11, 5, 7)
    assert f(10.25, 6.75, splat=4.0, max_splat=1) == [(10, 7)]
    assert f(10.75, 6.0, splat=2.0, max_splat=3) == box(10, 12, 5, 7)      # [9, 12] cut to 11 - 1 .. 11 + 1
    assert f(10.0, 6.0, z=1.0 / 64, splat=4.0, max_splat=15) == box(3, 17, 0, 13)   # hx = 512: the cap alone bounds the loop
    # clipping at the four edges, and just outside them
    assert f(0.0, 6.0) == box(0, 2, 4, 8) and f(31.0, 6.0) == box(29, 31, 4, 8)
    assert f(10.0, 0.0) == box(8, 12, 0, 2) and f(10.0, 23.0) == box(8, 12, 21, 23)
    assert f(-1.5, -1.0) == box(0, 0, 0, 1) and f(33.0, 25.0) == box(31, 31, 23, 23)
    assert f(-2.5, 6.0) == [] and f(10.0, 26.5) == [] and f(34.5, 6.0) == [] and f(10.0, -3.0) == []
    assert f(-0.75, 6.0, splat=0.25) == [] and f(-0.5, 6.0, splat=0.25) == [(0, 6)]    # nearest pixel -1: clipped away; floor(0.0) = 0
    assert f(1e6, 6.0) == [] and f(10.0, -1e6) == []
    # nothing is left by a voxel behind the camera, at depth 0, beyond the range or under min_points
    xyzi, counts = records([(0.0, 0.0, -2.0, 7.0, 1), (0.0, 0.0, 0.0, 7.0, 1), (np.nan, 0.0, 2.0, 7.0, 1), (0.0, 0.0, np.inf, 7.0, 1)])
    assert holes(render_host(xyzi, counts, leaf, K, w, h, np.eye(4))[1]).all()
    assert f(10.0, 6.0, min_depth=2.5, max_depth=3.0) == [] and f(10.0, 6.0, min_depth=0.0, max_depth=1.5) == []
    assert f(10.0, 6.0, min_depth=2.0, max_depth=2.0) == box(8, 12, 4, 8)
    assert f(10.0, 6.0, n=2, min_points=3) == [] and f(10.0, 6.0, n=3, min_points=3) == box(8, 12, 4, 8)
    assert f(10.0, 6.0, n=(1 << 20) + 1) == [] and f(10.0, 6.0, n=1 << 20) == box(8, 12, 4, 8)
    # a view from another pose: the inverse is applied (the camera moved 0.5 to the right sees the voxel 16 pixels to the left)
    T = np.eye(4)
    T[0, 3] = 0.5
    xyzi, counts = records([(0.0, 0.0, 2.0, 7.0, 1)])
    Z = render_host(xyzi, counts, leaf, K, w, h, T)[1][0]
    vs, us = np.nonzero(~holes(Z))
    assert sorted(set(us.tolist())) == [0, 1, 2] and sorted(set(vs.tolist())) == [10, 11, 12, 13, 14]     # u' = 16 - 16 = 0, v' = 12
    # ... and a rotation about y by 90 degrees: the camera at the origin looking along +x sees the point (2, 0, 0) in its centre
    R = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    xyzi, counts = records([(2.0, 0.0, 0.0, 7.0, 1)])
    Z = render_host(xyzi, counts, leaf, K, w, h, R)[1][0]
    vs, us = np.nonzero(~holes(Z))
    assert sorted(set(us.tolist())) == [14, 15, 16, 17, 18] and np.all(Z[vs, us] == 2.0)


# ---- 5. accuracy on the project's scene -----------------------------------------------------------------------------------------------

# measured with this file on the CPU (profiles/map_render.md): views 0 and 1 of float_views(128, 96), leaf 0.02, default parameters
MEASURED_COVERAGE, MEASURED_MEDIAN, MEASURED_P95 = 1.0, 0.0021163225, 3.0912928820
MEASURED_P90, MEASURED_TOO_NEAR = 0.0591878891, 0.0659012837     # the 90th percentile; the share of pixels more than 0.1 m too near


def scene_map():
    K, views = tcm.float_views(128, 96)
    m = HostMap(0.02, 1 << 16)
    for I, Z, T in views[:2]:
        m.insert(I, Z, K, T)
    assert m.stats()["dropped"] == 0
    return K, views, m


def scene_accuracy():
    K, views, m = scene_map()
    Ir, Zr = render_host_map(m, K, 128, 96, views[0][2])
    Z0 = views[0][1]
    valid0, filled = np.isfinite(Z0) & (Z0 > 0), ~holes(Zr[0])
    diff = (Zr[0].astype(np.float64) - Z0.astype(np.float64))[valid0 & filled]
    err = np.abs(diff)
    return (float((valid0 & filled).sum() / valid0.sum()), float(np.median(err)), float(np.percentile(err, 95)), float(np.percentile(err, 90)),
            float((diff < -0.1).mean()), float((diff > 0.1).mean()))


def test_accuracy_on_the_projects_scene():
    """Coverage (the share of view 0's valid pixels the render fills) and the median and 95th percentile of |Z_render - Z_view0| over
    the pixels valid in both, for the map of views 0 and 1 at 128 x 96 under their true poses, leaf 0.02, rendered at view 0's pose.
    On slanted surfaces and at depth edges these follow from no closed form; they were measured here on the CPU (MEASURED_* above):
    coverage 1.0, median 2.1 mm, 95th percentile 3.09 m.  The percentile lies in the tail the flat square splat is known for: the
    scene's nearest objects stand 0.32 m from the camera in front of a background metres away, a 2 cm voxel there is 6.5 pixels wide,
    and its footprint (cut to 7 pixels) grows the foreground silhouette by up to 3 pixels -- 6.6 % of the pixels show the foreground
    where view 0 saw the background, none the other way round (profiles/map_render.md has the breakdown).
    Asserted: the errors at most twice the measured ones, and the shortfall of the coverage from 1 at most half the measured shortfall,
    which is 0: every valid pixel of view 0 is filled.  A broken projection loses coverage at once.
    Twice 3.09 m constrains little on a scene a few metres deep, so two figures that lie below the silhouette tail are held to the same
    factor of two: the 90th percentile (measured 5.9 cm) and the share of pixels more than 0.1 m too NEAR (measured 6.6 %) -- a footprint
    that grows, or a cap that stops cutting, moves both.  No pixel is more than 0.1 m too FAR: the z-buffer keeps the nearest voxel, and
    every valid pixel of view 0 put its own point into the map, so something at its depth or nearer covers it."""
    coverage, median, p95, p90, too_near, too_far = scene_accuracy()
    print("coverage %.6f median %.6g p95 %.6g p90 %.6g too near %.6g too far %.6g" % (coverage, median, p95, p90, too_near, too_far))
    assert MEASURED_COVERAGE > 0.5 and MEASURED_MEDIAN > 0 and MEASURED_P95 > MEASURED_MEDIAN
    assert 1.0 - coverage <= 0.5 * (1.0 - MEASURED_COVERAGE)
    assert median <= 2.0 * MEASURED_MEDIAN and p95 <= 2.0 * MEASURED_P95
    assert p90 <= 2.0 * MEASURED_P90 and too_near <= 2.0 * MEASURED_TOO_NEAR and too_far == 0.0


# parameters profiles/map_render.md and include/dvo_hip.h name for model views to TRACK against
TRACKING_PARAMS = [dict(max_splat=1), dict(splat=1.0, min_depth=0.6)]


def oracle_tracking_error(I, Z, K, views, levels=3):
    """view 1 aligned against the planes (I, Z) at view 0's pose by the oracle (MATH mode, the default config cut to the levels 128 x 96
    has): the max-abs twist between its transformation and the true relative pose"""
    import common as cm
    from oracle import pyoracle as po
    cfg = d.Config()
    cfg.FirstLevel, cfg.LastLevel = min(cfg.FirstLevel, levels - 1), min(cfg.LastLevel, levels - 1)
    ref = po.Pyramid(np.ascontiguousarray(I), np.ascontiguousarray(Z), K, levels)
    cur = po.Pyramid(views[1][0], views[1][1], K, levels)
    o = po.match(ref, cur, cm.oracle_config_from(cfg, po.MATH))
    assert not np.isnan(o["T"]).any()
    true = np.linalg.inv(views[0][2]) @ views[1][2]
    return float(cm.twist_matrix_error(o["T"], true)), float(np.abs(po.se3_log(true)).max())


def test_tracking_against_the_model_on_the_cpu():
    """The headline use, on the CPU: view 1 aligned by the oracle against the model of views 0 and 1 rendered at view 0's pose, its
    distance to the TRUE relative pose beside that of aligning against view 0's own planes.  Measured (profiles/map_render.md): the
    motion is 0.021; keyframe 0.0089; the default view 0.054 -- the grown foreground silhouettes mislead the alignment, so the
    defaults are NOT for tracking on such a scene, which is a record here and stated where the use is advertised; max_splat = 1 gives
    0.0088 and splat = 1 with min_depth = 0.6 gives 0.0071.
    Asserted for the parameters named for tracking: the result is nearer to the truth than the identity is (an estimate farther off
    than the motion itself is worse than none), and not farther than twice the keyframe's own distance (the model holds the keyframe's
    points and view 1's; a correct view of it cannot be much worse than the keyframe alone, and the factor allows for the holes a
    one-pixel splat leaves)."""
    K, views, m = scene_map()
    baseline, motion = oracle_tracking_error(views[0][0], views[0][1], K, views)
    I, Z = render_host_map(m, K, 128, 96, views[0][2])
    default, _ = oracle_tracking_error(I[0], Z[0], K, views)
    print("motion %.4g keyframe %.4g default view %.4g" % (motion, baseline, default))
    assert baseline < motion
    for params in TRACKING_PARAMS:
        I, Z = render_host_map(m, K, 128, 96, views[0][2], **params)
        err, _ = oracle_tracking_error(I[0], Z[0], K, views)
        print(params, "%.4g" % err)
        assert err < motion and err <= 2.0 * baseline, (params, err)


# ---- 6. the Python wrappers and the C++ facade ----------------------------------------------------------------------------------------

class FakeCamera:
    width, height = 64, 48


class FakePyramid:
    def __init__(self, ctx, camera, levels=3):
        self.ctx, self.camera, self.levels, self.ptr = ctx, camera, levels, None


def test_python_wrappers_reject_bad_arguments_before_the_library():
    ctx, cam = object(), FakeCamera()
    m = d.KeyframeMap.__new__(d.KeyframeMap)                       # (no library behind it: every refusal below comes first)
    m.ctx, m.ptr, m.leaf = ctx, None, 0.01
    K, eye = [50.0, 50.0, 31.5, 23.5], np.eye(4)
    good = tracker._render_view_args(K, 64, 48, eye, "t")
    assert good[0].dtype == np.float32 and good[1:3] == (64, 48) and good[3].shape == (1, 4, 4) and good[3].dtype == np.float64
    assert tracker._render_view_args(K, 64, 48, np.stack([eye, eye, eye]), "t")[3].shape == (3, 4, 4)
    p = d.render_params_struct()
    assert (p.min_depth, p.max_depth, p.splat, p.max_splat, p.min_points, list(p.reserved)) == (0.0, INF, 2.0, 7, 1, [0, 0, 0])
    assert C.sizeof(d._lib.RenderParams) == 32
    bad_views = [dict(K=[50.0, 50.0, 31.5]), dict(K=[0.0, 50.0, 31.5, 23.5]), dict(K=[50.0, -1.0, 31.5, 23.5]), dict(K=[50.0, 50.0, np.nan, 23.5]),
                 dict(K=[INF, 50.0, 31.5, 23.5]), dict(width=0), dict(height=-3), dict(width=(1 << 24) + 1), dict(poses=np.zeros((2, 3, 4))),
                 dict(poses=np.zeros((0, 4, 4))), dict(poses=np.zeros(16)), dict(width=1 << 16, height=1 << 16)]
    for bad in bad_views:
        with pytest.raises(ValueError):
            m.render(**dict(dict(K=K, width=64, height=48, poses=eye), **bad))
    for bad in (dict(width=64.0), dict(height=True), dict(K="abcd"), dict(poses=[["a"] * 4] * 4)):
        with pytest.raises(TypeError):
            m.render(**dict(dict(K=K, width=64, height=48, poses=eye), **bad))
    bad_params = [dict(splat=0.0), dict(splat=-1.0), dict(splat=4.5), dict(splat=float("nan")), dict(max_splat=0), dict(max_splat=6), dict(max_splat=17),
                  dict(max_splat=-1), dict(min_points=0), dict(min_depth=2.0, max_depth=1.0), dict(min_depth=float("nan")), dict(max_depth=float("nan"))]
    two = [FakePyramid(ctx, cam), FakePyramid(ctx, cam)]
    for bad in bad_params:
        with pytest.raises(ValueError):
            m.render(K, 64, 48, eye, **bad)
        with pytest.raises(ValueError):
            m.render_into(two, np.stack([eye, eye]), **bad)
    for bad in (dict(max_splat=7.0), dict(min_points=True), dict(spat=2.0)):
        with pytest.raises(TypeError):
            m.render(K, 64, 48, eye, **bad)
    for pyramids, poses in (([], np.zeros((0, 4, 4))), (two, eye), (two, np.stack([eye] * 3)), (two, np.zeros((2, 16))),
                            ([two[0], FakePyramid(object(), cam)], np.stack([eye, eye])), ([two[0], FakePyramid(ctx, FakeCamera())], np.stack([eye, eye]))):
        with pytest.raises(ValueError):
            m.render_into(pyramids, poses)
    lensed, rigged = FakePyramid(ctx, cam), FakePyramid(ctx, cam)
    lensed._lens, rigged._depth_rig = ([1.0] * 4, [0.0] * 8, True), ([1.0] * 4, [0.0] * 12)
    for p in (lensed, rigged):
        with pytest.raises(ValueError):
            m.render_into([p], eye)
    with pytest.raises(ValueError):
        m.render_into(two, np.stack([eye, eye]), flags=d._lib.INGEST_DEFER)
    with pytest.raises(ValueError):
        m.render_into(two, np.stack([eye, eye]), role="keyframe", config=d.Config())
    with pytest.raises(ValueError):
        m.render_into(two, np.stack([eye, eye]), role="current")   # a role needs a config


def build_render_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "map_render_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "map_render_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_render_compiles():
    d.build()
    assert os.path.exists(build_render_facade_check())
