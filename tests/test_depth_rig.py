"""CPU tier: the depth rig of the registering ingest, without a GPU.
  * dvo_slam_amd/csrc/depth_rig.h (the projection k_depth_register inlines) compiled for the host with g++ -Werror and
    -ffp-contract=off; reg() below registers whole planes with it and is the yardstick of tests/test_gpu_depth_rig.py;
  * the identity rig reproduces a plane of positive finite depths bit for bit; zeros (u16), NaN, negative values and infinities are holes;
  * a numpy float64 restatement of the model agrees with the yardstick except where float32 rounding of u' + 0.5 decides a pixel;
  * hand-made planes: the nearer of two sources wins in either order, the -0.5 / w - 0.5 borders, a point behind the camera, occlusion
    and the band of holes behind a depth step;
  * it matters: on a synthetic pair whose depth is rendered from the shifted sensor, the oracle's pose error is smaller on the
    registered pair than on the unregistered one (numbers: profiles/depth_registration.md);
  * the Python wrappers reject bad arguments before anything reaches the library; the C++ facade's setDepthRig / clearDepthRig compile
    (tests/cpp/depth_rig_facade_check.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import scenes
from dvo_slam_amd import _lib
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")
FR1_K = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
SCALE = 1.0 / 5000.0

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include "depth_rig.h"
using namespace dvo_hip;
namespace {
float converted(const unsigned char* depth, int depth_format, size_t pitch, float scale, int u, int v) {
  const unsigned char* p = depth + size_t(v) * pitch + size_t(u) * (depth_format == DVO_HIP_DEPTH_F32 ? 4 : 2);
  if (depth_format == DVO_HIP_DEPTH_F32) { float f; std::memcpy(&f, p, 4); return depth_of_f32(f, scale); }
  uint16_t r; std::memcpy(&r, p, 2);
  return depth_of_u16(r, scale);
}
dvo_hip_depth_rig rig_of(const float* K_depth, const float* T) {
  dvo_hip_depth_rig rig;
  std::memcpy(rig.K_depth, K_depth, sizeof rig.K_depth);
  std::memcpy(rig.T, T, sizeof rig.T);
  rig.reserved[0] = rig.reserved[1] = 0;
  return rig;
}
}
extern "C" {
// depth_format: DVO_HIP_DEPTH_*; pitch in bytes; Z: the z-buffer as uint32; reverse != 0: the source pixels last to first
void rig_host_register(const float* K, const float* K_depth, const float* T, int w, int h, const unsigned char* depth, int depth_format, size_t pitch,
                       float scale, uint32_t* Z, int reverse) {
  const DepthRigMap m = depth_rig_prepare(K, rig_of(K_depth, T));
  for (int i = 0; i < w * h; ++i) Z[i] = kDepthRigHole;
  for (int k = 0; k < w * h; ++k) {
    const int i = reverse ? w * h - 1 - k : k;
    const int u = i % w, v = i / w;
    int at;
    uint32_t bits;
    if (!depth_rig_project(m, w, h, u, v, converted(depth, depth_format, pitch, scale, u, v), &at, &bits)) continue;
    if (bits < Z[at]) Z[at] = bits;
  }
}
// per SOURCE pixel: where it lands (-1: skipped) and the bits it offers
void rig_host_project(const float* K, const float* K_depth, const float* T, int w, int h, const unsigned char* depth, int depth_format, size_t pitch,
                      float scale, int* at, uint32_t* bits) {
  const DepthRigMap m = depth_rig_prepare(K, rig_of(K_depth, T));
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) {
      const int i = v * w + u;
      if (!depth_rig_project(m, w, h, u, v, converted(depth, depth_format, pitch, scale, u, v), &at[i], &bits[i])) at[i] = -1, bits[i] = 0;
    }
}
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    """depth_rig.h compiled for the host: g++, every warning an error, no contraction (what the header's pragma says to clang)"""
    tmp = tempfile.mkdtemp(prefix="depth_rig_host_")
    src, out = os.path.join(tmp, "depth_rig_host.cpp"), os.path.join(tmp, "depth_rig_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    fp, vp, ip, up = C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    L.rig_host_register.argtypes = [fp, fp, fp, C.c_int, C.c_int, vp, C.c_int, C.c_size_t, C.c_float, up, C.c_int]
    L.rig_host_register.restype = None
    L.rig_host_project.argtypes = [fp, fp, fp, C.c_int, C.c_int, vp, C.c_int, C.c_size_t, C.c_float, ip, up]
    L.rig_host_project.restype = None
    return L


def _f(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _format(depth):
    assert depth.dtype in (np.float32, np.uint16) and depth.strides[1] == depth.itemsize
    return _lib.DEPTH_F32 if depth.dtype == np.float32 else _lib.DEPTH_U16


def reg(depth, K, K_depth, T, depth_scale=SCALE, reverse=False):
    """reg(P): the registered float plane Z of the depth sensor's plane P as depth_rig.h defines it, computed on the host.  depth: [h, w]
    uint16 or float32, rows may be padded (the array's own stride is the pitch); T: 3 x 4 [R | t]."""
    h, w = depth.shape
    Z = np.empty((h, w), np.uint32)
    (_, k), (_, kd), (_, t) = _f(K), _f(K_depth), _f(np.asarray(T, np.float32)[:3])
    host_lib().rig_host_register(k, kd, t, w, h, depth.ctypes.data, _format(depth), depth.strides[0], depth_scale,
                                 Z.ctypes.data_as(C.POINTER(C.c_uint32)), 1 if reverse else 0)
    return Z.view(np.float32)


def project(depth, K, K_depth, T, depth_scale=SCALE):
    """per source pixel: (target index or -1, offered bits) as depth_rig.h computes them"""
    h, w = depth.shape
    at, bits = np.empty((h, w), np.int32), np.empty((h, w), np.uint32)
    (_, k), (_, kd), (_, t) = _f(K), _f(K_depth), _f(np.asarray(T, np.float32)[:3])
    host_lib().rig_host_project(k, kd, t, w, h, depth.ctypes.data, _format(depth), depth.strides[0], depth_scale,
                                at.ctypes.data_as(C.POINTER(C.c_int)), bits.ctypes.data_as(C.POINTER(C.c_uint32)))
    return at, bits


IDENTITY_T = np.eye(4, dtype=np.float32)[:3]


def kinect_rig(K):
    """a Kinect-like rig over the colour camera K: the depth sensor 25 mm beside it, turned by 0.6 degrees, with a 10 % longer focal length"""
    K = np.asarray(K, np.float32)
    K_depth = (K.astype(np.float64) * np.array([1.10, 1.10, 1.004, 0.993])).astype(np.float32)
    T = scenes.se3_exp([0, 0, 0] + list(np.deg2rad(0.6) * np.array([0.3, 0.9, 0.316]) / np.linalg.norm([0.3, 0.9, 0.316])))[:3].copy()
    T[:, 3] = [-0.025, 0.001, 0.003]
    return K_depth, T.astype(np.float32)


def scaled_K(w):
    return (FR1_K * (w / 640.0)).astype(np.float32)


def smooth_depth(w, h, seed=0):
    """a slanted, gently curved surface at 1-3 m as float64 metres: no two neighbours at the same depth"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 6.28, 2)
    return 1.6 + 0.9 * x / w + 0.4 * y / h + 0.08 * np.sin(x / 23.0 + ph[0]) * np.cos(y / 31.0 + ph[1])


# ---- 1. the identity rig ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(102, 78), (321, 240)])
def test_identity_rig_reproduces_the_plane_bit_for_bit(w, h):
    K = scaled_K(w)
    z = smooth_depth(w, h)
    u16 = np.rint(z * 5000).astype(np.uint16)
    f32 = z.astype(np.float32)
    assert np.array_equal(reg(u16, K, K, IDENTITY_T).view(np.uint32), (u16.astype(np.float32) * np.float32(SCALE)).view(np.uint32))
    assert np.array_equal(reg(f32, K, K, IDENTITY_T, 1.0).view(np.uint32), f32.view(np.uint32))
    assert np.array_equal(reg(f32, K, K, IDENTITY_T, 0.5), f32 * np.float32(0.5))
    # padded rows are the same plane
    pad = np.zeros((h, w + 3), np.float32)
    pad[:, :w] = f32
    assert np.array_equal(reg(pad[:, :w], K, K, IDENTITY_T, 1.0), f32)
    # what is no measurement comes out NaN, everything else as it was
    rng = np.random.default_rng(1)
    bad = rng.random((h, w)) < 0.1
    holes = u16.copy()
    holes[bad] = 0
    Z = reg(holes, K, K, IDENTITY_T)
    assert np.isnan(Z[bad]).all() and np.array_equal(Z[~bad], u16[~bad].astype(np.float32) * np.float32(SCALE))
    assert np.all(Z[bad].view(np.uint32) == 0x7FC00000)
    special = f32.copy()
    special[bad] = rng.choice(np.array([np.nan, -1.5, -0.0, 0.0, np.inf, -np.inf], np.float32), int(bad.sum()))
    Z = reg(special, K, K, IDENTITY_T, 1.0)
    assert np.isnan(Z[bad]).all() and np.array_equal(Z[~bad], f32[~bad])


# ---- 2. the float64 model ---------------------------------------------------------------------------------------------------------------

def model_f64(depth, K, K_depth, T, depth_scale):
    """The model as include/dvo_hip.h states it, in float64 from the float32 parameters and the float32 converted depth.  Per source
    pixel: the target index (-1: skipped), P'.z, u', v'."""
    h, w = depth.shape
    fx, fy, ox, oy = (float(v) for v in np.asarray(K, np.float32))
    fxd, fyd, oxd, oyd = (float(v) for v in np.asarray(K_depth, np.float32))
    T = np.asarray(T, np.float32).astype(np.float64)
    if depth.dtype == np.uint16:
        z = np.where(depth == 0, np.float32(np.nan), depth.astype(np.float32) * np.float32(depth_scale)).astype(np.float64)
    else:
        z = (depth * np.float32(depth_scale)).astype(np.float64)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.isfinite(z) & (z > 0)
        X, Y = (u - oxd) / fxd * z, (v - oyd) / fyd * z
        P = np.stack([T[i, 0] * X + T[i, 1] * Y + T[i, 2] * z + T[i, 3] for i in range(3)])
        ok &= np.isfinite(P[2]) & (P[2] > 0)
        tu, tv = fx * P[0] / P[2] + ox, fy * P[1] / P[2] + oy
        ok &= (tu >= -0.5) & (tu < w - 0.5) & (tv >= -0.5) & (tv < h - 0.5)
        xi = np.clip(np.floor(np.where(ok, tu, 0) + 0.5), 0, w - 1).astype(np.int64)
        yi = np.clip(np.floor(np.where(ok, tv, 0) + 0.5), 0, h - 1).astype(np.int64)
    return np.where(ok, yi * w + xi, -1), P[2], tu, tv


@pytest.mark.parametrize("w,h,fmt", [(321, 240, "u16"), (102, 78, "f32"), (640, 480, "u16")])
def test_yardstick_equals_the_float64_model_up_to_rounding_boundaries(w, h, fmt):
    """A target pixel DIFFERS when the float64 model's winning source does not offer, in float32, that very pixel the value the
    yardstick holds there, when only one of the two has a value, or when the values differ by more than 1e-6 z.  Asserted: at most
    0.5 % of the pixels differ, and for every one of them a source whose float32 and float64 targets disagree lies within 1e-3 pixels
    of a rounding boundary (u' + 0.5 or v' + 0.5 an integer).  Measured with the yardstick on the smooth scene under the Kinect-like
    rig: 0 of 77 040 pixels at 321 x 240 (u16), 0 of 7 956 at 102 x 78 (f32) and 9 of 307 200 = 0.0029 % at 640 x 480 (u16) -- float32
    carries u' to a few 1e-5 pixels at these widths, and the share of pixels that close to a boundary in u or v is of that order."""
    K = scaled_K(w)
    K_depth, T = kinect_rig(K)
    z = smooth_depth(w, h, 2)
    depth = np.rint(z * 5000).astype(np.uint16) if fmt == "u16" else z.astype(np.float32)
    scale = SCALE if fmt == "u16" else 1.0
    Z32 = reg(depth, K, K_depth, T, scale).reshape(-1)
    at32, bits32 = (a.reshape(-1) for a in project(depth, K, K_depth, T, scale))
    at64, pz, tu, tv = (a.reshape(-1) for a in model_f64(depth, K, K_depth, T, scale))
    # the float64 z-buffer: per target the source of the smallest P'.z
    src = np.flatnonzero(at64 >= 0)
    order = src[np.lexsort((pz[src], at64[src]))]
    first = np.concatenate([[True], at64[order][1:] != at64[order][:-1]])
    winner = np.full(w * h, -1, np.int64)
    winner[at64[order][first]] = order[first]
    Z64 = np.where(winner >= 0, pz[np.maximum(winner, 0)], np.nan)
    have32, have64 = ~np.isnan(Z32), winner >= 0
    assert have64.mean() > 0.7 and (~have64).mean() > 0.05       # (a longer focal length: the depth image covers a part of the colour image)
    wi = np.maximum(winner, 0)
    differs = have32 != have64
    both = have32 & have64
    differs |= both & ((at32[wi] != np.arange(w * h)) | (bits32[wi] != Z32.view(np.uint32)))
    with np.errstate(invalid="ignore"):
        differs |= both & (np.abs(Z32.astype(np.float64) - Z64) > 1e-6 * Z64)
    share = differs.mean()
    print("%d x %d %s: %d of %d target pixels differ (%.4f %%)" % (w, h, fmt, differs.sum(), w * h, 100 * share))
    assert share <= 0.005
    # every differing pixel is explained by a source that float32 and float64 send to different pixels, at a rounding boundary
    moved = np.flatnonzero(at32 != at64)
    with np.errstate(invalid="ignore"):
        near = np.minimum(np.abs(tu + 0.5 - np.rint(tu + 0.5)), np.abs(tv + 0.5 - np.rint(tv + 0.5))) < 1e-3
    assert near[moved].all()
    explained = np.zeros(w * h, bool)
    for a in (at32[moved], at64[moved]):
        explained[a[a >= 0]] = True
    assert not (differs & ~explained).any()


# ---- 3. hand-made planes ----------------------------------------------------------------------------------------------------------------

def test_the_nearer_of_two_sources_wins_in_either_order():
    w, h = 16, 8
    K = np.array([10.0, 10.0, 4.0, 4.0], np.float32)
    K_depth = np.array([20.0, 20.0, 8.0, 8.0], np.float32)        # u' = u / 2 exactly: sources 3 and 4 (1.5 and 2.0) both land on pixel 2
    for near, far in ((3, 4), (4, 3)):
        depth = np.zeros((h, w), np.float32)
        depth[6, near], depth[6, far] = 1.0, 2.0                  # (row 6 -> v' = 3.0)
        at, _ = project(depth, K, K_depth, IDENTITY_T, 1.0)
        assert at[6, 3] == at[6, 4] == 3 * w + 2
        for reverse in (False, True):
            Z = reg(depth, K, K_depth, IDENTITY_T, 1.0, reverse)
            assert Z[3, 2] == 1.0 and np.isfinite(Z).sum() == 1


def test_borders_and_points_behind_the_camera():
    w, h = 16, 8
    K = np.array([16.0, 16.0, 4.0, 4.0], np.float32)
    depth = np.full((h, w), 2.0, np.float32)
    # the depth sensor's centre half a pixel to the right: u' = u - 0.5 exactly.  Source 0 lies at -0.5: kept, in pixel 0
    Kd = K + np.array([0, 0, 0.5, 0], np.float32)
    at, _ = project(depth, K, Kd, IDENTITY_T, 1.0)
    assert np.array_equal(at[2], 2 * w + np.arange(w))            # floor(u - 0.5 + 0.5) = u
    assert np.isfinite(reg(depth, K, Kd, IDENTITY_T, 1.0)).all()
    # ... half a pixel to the left: u' = u + 0.5, the last source lies at w - 0.5: dropped; the others land one pixel to the right
    Kd = K - np.array([0, 0, 0.5, 0], np.float32)
    at, _ = project(depth, K, Kd, IDENTITY_T, 1.0)
    assert np.all(at[:, w - 1] == -1) and np.array_equal(at[2, :w - 1], 2 * w + 1 + np.arange(w - 1))
    Z = reg(depth, K, Kd, IDENTITY_T, 1.0)
    assert np.isnan(Z[:, 0]).all() and np.all(Z[:, 1:] == 2.0)
    # the same in v
    Kd = K - np.array([0, 0, 0, 0.5], np.float32)
    at, _ = project(depth, K, Kd, IDENTITY_T, 1.0)
    assert np.all(at[h - 1] == -1) and np.all(at[:h - 1] >= 0)
    Kd = K + np.array([0, 0, 0, 0.5], np.float32)
    assert np.all(project(depth, K, Kd, IDENTITY_T, 1.0)[0] >= 0)
    # behind the colour camera, and exactly in its plane: skipped
    for tz in (-5.0, -2.0):
        T = IDENTITY_T.copy()
        T[2, 3] = tz
        assert np.isnan(reg(depth, K, K, T, 1.0)).all()
    # an overflowing product is no depth
    T = IDENTITY_T.copy()
    T[2, 2] = 3e38
    assert np.isnan(reg(np.full((h, w), 4.0, np.float32), K, K, T, 1.0)).all()


def step_scene(w=64, h=48):
    """a foreground slab at 1 m in columns [24, 44) before a wall at 3 m, seen by a sensor 24 mm to the left of the colour camera"""
    K = np.array([500.0, 500.0, 31.5, 23.5], np.float32)
    depth = np.full((h, w), 15000, np.uint16)
    depth[:, 24:44] = 5000
    T = IDENTITY_T.copy()
    T[0, 3] = -0.024
    return K, depth, T


def test_occlusion_and_the_band_of_holes_behind_a_depth_step():
    K, depth, T = step_scene()
    Z = reg(depth, K, K, T)
    near, far = np.float32(5000) * np.float32(SCALE), np.float32(15000) * np.float32(SCALE)
    assert set(np.unique(Z[np.isfinite(Z)]).tolist()) == {float(near), float(far)}     # never a mixture
    # the slab moves by fx t / z = -12 pixels, the wall by -4: the slab covers columns 12-31 ...
    assert np.all(Z[:, 12:32] == near)
    # ... among them the wall's sources 16-23, which land on 12-19: occluded, gone; to the left the wall as it was
    assert np.all(Z[:, :12] == far)
    # behind the slab's far side nothing was seen: a band of holes 8 pixels wide, then the wall again, to its last source (63 -> 59)
    assert np.isnan(Z[:, 32:40]).all() and np.all(Z[:, 40:60] == far) and np.isnan(Z[:, 60:]).all()
    assert np.array_equal(Z, reg(depth, K, K, T, reverse=True), equal_nan=True)


# ---- 4. it matters ----------------------------------------------------------------------------------------------------------------------

MATTERS = dict(seed=3, w=320, h=240, levels=3)


@functools.lru_cache(maxsize=None)
def matters_pair():
    """scenes.edge_scene with the depth planes rendered again from the depth sensor of the Kinect-like rig: (the pair as the colour
    camera alone would see it, the pair with the depth sensor's planes, K_depth, T)"""
    seed, w, h = MATTERS["seed"], MATTERS["w"], MATTERS["h"]
    pair = scenes.edge_scene(seed, w, h)
    scene = scenes._Scene(np.random.default_rng([seed, w, h]))    # (the scene is the first thing edge_scene draws from its generator)
    K_depth, T = kinect_rig(pair["K"])
    fxd, fyd, oxd, oyd = (float(v) for v in K_depth)
    T4 = np.vstack([T.astype(np.float64), [0, 0, 0, 1]])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rays = np.stack([(xx - oxd) / fxd, (yy - oyd) / fyd, np.ones_like(xx)], -1)
    # the recovered scene IS the pair's: cast from the colour camera, it gives the pair's reference depth wherever no hole was punched
    fx, fy, ox, oy = (float(v) for v in pair["K"])
    own, _, _ = scene.cast(np.zeros(3), np.stack([(xx - ox) / fx, (yy - oy) / fy, np.ones_like(xx)], -1))
    seen = pair["depth_ref"] != 0
    assert seen.mean() > 0.5 and np.array_equal(scenes._quantise_depth(own)[seen], pair["depth_ref"][seen])
    raw = dict(pair)
    for view, M in (("ref", np.eye(4)), ("cur", scenes.se3_exp(pair["xi_true"]))):
        S = M @ T4                                                # depth sensor of that view -> reference colour camera
        s, _, _ = scene.cast(S[:3, 3], rays @ S[:3, :3].T)
        raw["depth_" + view] = scenes._quantise_depth(s)
    return pair, raw, K_depth, T


def pose_error(T, xi_true):
    return float(np.abs(po.se3_log(np.linalg.inv(po.se3_exp(xi_true)) @ T)).max())


def registered_pyramids(raw, K, K_depth, T, levels):
    return tuple(po.Pyramid(raw["grey_" + v].astype(np.float32), reg(raw["depth_" + v], K, K_depth, T), K, levels) for v in ("ref", "cur"))


def test_registration_matters_to_the_oracle():
    pair, raw, K_depth, T = matters_pair()
    levels = MATTERS["levels"]
    cfg = po.make_config(first_level=levels - 1, last_level=0, mode=po.MATH)
    e_raw = pose_error(po.match(*po.pyramids_from_pair(raw, levels), cfg)["T"], pair["xi_true"])
    e_reg = pose_error(po.match(*registered_pyramids(raw, pair["K"], K_depth, T, levels), cfg)["T"], pair["xi_true"])
    print("pose error (largest twist component against the scene's true warp): depth sensor's planes as they are e_raw = %.3e, "
          "registered e_reg = %.3e" % (e_raw, e_reg))
    assert e_reg < e_raw


# ---- 5. wrappers and facade -------------------------------------------------------------------------------------------------------------

class _NoLibrary:
    """stands in for a context: any use of the library is a test failure"""
    ptr = None

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


class _Pyramid:
    def __init__(self):
        self.ctx, self.ptr = _NoLibrary(), None


def test_wrappers_reject_bad_arguments_before_the_library():
    pyrs = [_Pyramid(), _Pyramid()]
    K = [570.3, 570.3, 319.5, 239.5]
    T = np.eye(4)[:3]
    bad_T = np.eye(4)
    bad_T[3, 0] = 0.1
    nan_T = T.copy()
    nan_T[1, 2] = np.nan
    bad = [
        (ValueError, (K[:3], T)),                                  # K_depth: four numbers
        (ValueError, (np.zeros((2, 2)), T)),
        (ValueError, (K, np.eye(3))),                              # T: 3 x 4, 4 x 4 or 12 values
        (ValueError, (K, np.zeros(11))),
        (ValueError, (K, bad_T)),                                  # (a 4 x 4 whose last row is not 0 0 0 1)
        (ValueError, (K, nan_T)),                                  # finite
        (ValueError, ([np.inf, 500, 300, 200], T)),
        (ValueError, (K, T * 1e39)),                               # (infinite as float32)
        (ValueError, ([0.0, 500, 300, 200], T)),                   # positive focal lengths
        (ValueError, ([500, -1.0, 300, 200], T)),
        (TypeError, (K, np.array([["a"] * 4] * 3))),               # numbers
        (TypeError, (np.array([1 + 2j, 1, 1, 1]), T)),
        (TypeError, (K, None)),
        (TypeError, (None, T)),
    ]
    for exc, (k, t) in bad:
        with pytest.raises(exc):
            d.set_depth_rig_batch(pyrs, k, t)
        with pytest.raises(exc):
            d.RgbdImagePyramid.set_depth_rig(pyrs[0], k, t)
    with pytest.raises(ValueError):
        d.set_depth_rig_batch([], K, T)
    with pytest.raises(ValueError):
        d.clear_depth_rig_batch([])
    M = np.arange(12, dtype=np.float64).reshape(3, 4) / 8
    for t in (M, np.vstack([M, [0, 0, 0, 1]]), M.reshape(-1), M.tolist()):
        rig = d.depth_rig_struct(K, t)
        assert list(rig.T) == M.reshape(-1).tolist() and list(rig.reserved) == [0, 0]
        assert list(rig.K_depth) == [float(np.float32(v)) for v in K]
    assert C.sizeof(_lib.DepthRig) == 72


def test_header_declares_the_depth_rig():
    text = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    assert "typedef struct {\n  float K_depth[4];" in text and "} dvo_hip_depth_rig;" in text
    for name in ("dvo_hip_frames_set_depth_rig", "dvo_hip_frames_clear_depth_rig"):
        assert "int %s(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames" % name in text
        assert name in _lib.EXPORTS
    assert '"depth_registrations"' in text and "dvo_ros/src/camera_base.cpp:30-33" in text
    comment = open(os.path.join(CSRC, "depth_rig.h")).read()
    assert "depth_image_proc/register" in comment and "WITHOUT hole filling" in comment and "orthonormality" in comment


def build_depth_rig_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "depth_rig_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "depth_rig_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_depth_rig_methods_compile():
    d.build()
    assert os.path.exists(build_depth_rig_facade_check())
