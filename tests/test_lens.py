"""CPU tier: the lens model of the rectifying ingest, without a GPU.
  * dvo_slam_amd/csrc/lens.h (the map and the per-pixel rectifier k_rectify inlines) compiled for the host with g++ -Werror and
    -ffp-contract=off: the map against a float64 restatement of the OpenCV forward model written here, within the float32 rounding
    of the chain; D = 0 with K_raw = K maps every pixel exactly onto itself;
  * the same host build rectifies whole planes -- rectify() below is the yardstick rect(P) of tests/test_gpu_lens_ingest.py --
    checked against a numpy float32 restatement of the blend and on hand-made planes (edge semantics);
  * it matters: on a synthetic pair distorted on the CPU, the oracle's pose error is several times larger on the unrectified pair
    than on the rectified one (numbers: profiles/lens_ingest.md);
  * the Python wrappers reject bad arguments before anything reaches the library; the C++ facade's setLens / clearLens compile
    (tests/cpp/lens_facade_check.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common as cm
import dvo_slam_amd as d
from dvo_slam_amd import _lib, tum
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")

# lenses: fr1-like plumb-bob (the TUM fr1 calibration's magnitudes), an 8-coefficient rational set, and none
FR1_D = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633, 0.0, 0.0, 0.0], np.float32)
RATIONAL_D = np.array([0.31, -0.42, 0.0013, -0.0021, 0.18, 0.12, 0.07, 0.03], np.float32)
ZERO_D = np.zeros(8, np.float32)
FORMATS = dict(_lib.MIXED_PIXEL_FORMATS, f32=_lib.PIXEL_F32)

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include "lens.h"
using namespace dvo_hip;
extern "C" {
void lens_host_map(const float* K, const float* K_raw, const float* D, int w, int h, float* sx, float* sy) {
  const LensMap m = lens_prepare(K, K_raw, D);
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) lens_map(m, u, v, &sx[size_t(v) * w + u], &sy[size_t(v) * w + u]);
}
// format: 0 grey8, DVO_HIP_PIXEL_* colour, DVO_HIP_PIXEL_F32; depth_format: DVO_HIP_DEPTH_*; pitches in bytes
int lens_host_rectify(const float* K, const float* K_raw, const float* D, int rectify_depth, int w, int h, const unsigned char* image, int format,
                      size_t pitch, const unsigned char* depth, int depth_format, size_t depth_pitch, float depth_scale, float* I, float* Z) {
  const int ch = format == 0 ? 1 : format == DVO_HIP_PIXEL_F32 ? 4 : pixel_channels(format);
  if (ch == 0) return -1;
  const LensMap m = lens_prepare(K, K_raw, D);
  const GreyWeights gw = grey_weights(pixel_red_first(format));
  auto image_tap = [&](int x, int y) -> float {
    const unsigned char* p = image + size_t(y) * pitch + size_t(x) * ch;
    if (format == DVO_HIP_PIXEL_F32) { float f; std::memcpy(&f, p, 4); return f; }
    if (format == 0) return float(p[0]);
    return float(grey_of(p[0], p[1], p[2], gw));
  };
  auto depth_tap = [&](int x, int y) -> float {
    const unsigned char* p = depth + size_t(y) * depth_pitch + size_t(x) * (depth_format == DVO_HIP_DEPTH_F32 ? 4 : 2);
    if (depth_format == DVO_HIP_DEPTH_F32) { float f; std::memcpy(&f, p, 4); return depth_of_f32(f, depth_scale); }
    uint16_t r; std::memcpy(&r, p, 2);
    return depth_of_u16(r, depth_scale);
  };
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u)
      lens_rectify_pixel(m, w, h, u, v, rectify_depth != 0, image_tap, depth_tap, &I[size_t(v) * w + u], &Z[size_t(v) * w + u]);
  return 0;
}
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    """lens.h compiled for the host: g++, every warning an error, no contraction (what the header's pragma says to clang)"""
    tmp = tempfile.mkdtemp(prefix="lens_host_")
    src, out = os.path.join(tmp, "lens_host.cpp"), os.path.join(tmp, "lens_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    L.lens_host_map.argtypes = [fp, fp, fp, C.c_int, C.c_int, fp, fp]
    L.lens_host_map.restype = None
    L.lens_host_rectify.argtypes = [fp, fp, fp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_size_t, vp, C.c_int, C.c_size_t, C.c_float, fp, fp]
    return L


def _f(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _d8(D):
    D = np.asarray(D, np.float32)
    return np.concatenate([D, np.zeros(8 - D.shape[0], np.float32)])


def header_map(K, K_raw, D, w, h):
    """(sx, sy) of every pixel as lens.h computes them (float32)"""
    sx, sy = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    (_, k), (_, kr), (_, dd) = _f(K), _f(K_raw), _f(_d8(D))
    host_lib().lens_host_map(k, kr, dd, w, h, sx.ctypes.data_as(C.POINTER(C.c_float)), sy.ctypes.data_as(C.POINTER(C.c_float)))
    return sx, sy


def rectify(image, depth, K, K_raw, D, rectify_depth=True, fmt="grey8", depth_scale=1.0 / 5000.0):
    """rect(P): the rectified float pair (I, Z) of the raw planes P = (image, depth) as lens.h defines it, computed on the host.
    image: [h, w] uint8 (grey8), [h, w, c] uint8 (a colour format) or [h, w] float32 (f32); depth: [h, w] uint16 or float32; rows may be
    padded (the arrays' own strides are the pitches)."""
    h, w = depth.shape
    channels = image.shape[2] if image.ndim == 3 else 1
    assert image.shape[:2] == (h, w) and image.strides[1] == image.itemsize * channels and depth.strides[1] == depth.itemsize
    assert channels == 1 or image.strides[2] == 1
    I, Z = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    (_, k), (_, kr), (_, dd) = _f(K), _f(K_raw), _f(_d8(D))
    zf = _lib.DEPTH_F32 if depth.dtype == np.float32 else _lib.DEPTH_U16
    assert depth.dtype in (np.float32, np.uint16) and image.dtype == (np.float32 if fmt == "f32" else np.uint8)
    rc = host_lib().lens_host_rectify(k, kr, dd, 1 if rectify_depth else 0, w, h, image.ctypes.data, FORMATS[fmt], image.strides[0],
                                      depth.ctypes.data, zf, depth.strides[0], depth_scale, I.ctypes.data_as(C.POINTER(C.c_float)),
                                      Z.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return I, Z


def model_f64(K, K_raw, D, w, h):
    """the forward model as include/dvo_hip.h states it, in float64, from the float32 parameters"""
    fx, fy, ox, oy = (float(v) for v in np.asarray(K, np.float32))
    fxr, fyr, oxr, oyr = (float(v) for v in np.asarray(K_raw, np.float32))
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in _d8(D))
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (u - ox) / fx, (v - oy) / fy
    r2 = x * x + y * y
    radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fxr * xd + oxr, fyr * yd + oyr


def map_bound(K, K_raw, D, w, h):
    """How far the float32 chain of lens.h may lie from model_f64, per axis, in pixels: running error analysis of the chain as the
    header orders it, every rounding at most eps = 2^-24 of the value it produces (1 + eps factors of second order dropped; the 11 and
    the 8 below leave room for them).
      x, y          (u - ox) / fx: two roundings, 2 eps each; x^2, y^2, x y: 5 eps; r2 = x^2 + y^2 (positive terms): 6 eps;
      N = r2 (d1 + r2 (d2 + r2 d3)), d_j = fl(k_j - k_(j+3)): r2's 6 eps reach N through r2 N'(r2), at most 6 eps (|d1| r2 + 2 |d2| r2^2
                    + 3 |d3| r2^3); the chain's own seven roundings (d_j, three products, two sums, and one spare) act on partial sums
                    of at most N_abs = |d1| r2 + |d2| r2^2 + |d3| r2^3: 7 eps N_abs.  The denominator 1 + r2 (k4 + ...) likewise;
      q = N / Den   err(N) / |Den| + |N| err(Den) / Den^2 + eps |q|;
      dx            |x| err(q) + 11 eps T, T = |x| N_abs / |Den| + 2 |p1| |x y| + |p2| (r2 + 2 x^2): the factors' own errors (x: 2, x y: 5, r2 +
                    2 x^2: 7), the products and the two sums; the scale by fxr adds one more (inside the 11);
      pinhole part  fl(fl(u s) + c), s = fl(fxr / fx), c = fl(oxr - fl(ox s)): s's rounding acts on (u - ox) s, then the products u s
                    and ox s, c and the sum: eps (|(u - ox) s| + |u s| + |ox s| + |c| + |u s + c|);
      the last sum  eps |sx|.
    It comes out at a few ulp of the largest coordinate (up to ~11 at the corners of the plumb-bob set) -- the caller prints it and
    checks that it is no more than that."""
    eps = 2.0 ** -24
    D8 = [float(v) for v in _d8(D)]
    k1, k2, p1, p2, k3, k4, k5, k6 = D8
    d = [float(np.float32(a) - np.float32(b)) for a, b in ((k1, k4), (k2, k5), (k3, k6))]
    Kf, Kr = [float(v) for v in np.asarray(K, np.float32)], [float(v) for v in np.asarray(K_raw, np.float32)]
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = np.abs((u - Kf[2]) / Kf[0]), np.abs((v - Kf[3]) / Kf[1])
    r2 = x * x + y * y
    n_abs = abs(d[0]) * r2 + abs(d[1]) * r2 ** 2 + abs(d[2]) * r2 ** 3
    n = np.abs(d[0] * r2 + d[1] * r2 ** 2 + d[2] * r2 ** 3)
    err_n = eps * (6 * (abs(d[0]) * r2 + 2 * abs(d[1]) * r2 ** 2 + 3 * abs(d[2]) * r2 ** 3) + 7 * n_abs)
    den_abs = 1 + abs(k4) * r2 + abs(k5) * r2 ** 2 + abs(k6) * r2 ** 3
    den = np.abs(1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    err_den = eps * (6 * (abs(k4) * r2 + 2 * abs(k5) * r2 ** 2 + 3 * abs(k6) * r2 ** 3) + 7 * den_abs)
    err_q = err_n / den + n * err_den / den ** 2 + eps * n / den
    sx, sy = model_f64(K, K_raw, D, w, h)
    out = []
    for a, b, f, fr, o, orr, coord, pa, pb, s64 in ((x, y, Kf[0], Kr[0], Kf[2], Kr[2], u, p1, p2, sx), (y, x, Kf[1], Kr[1], Kf[3], Kr[3], v, p2, p1, sy)):
        s = fr / f
        pin = np.abs((coord - o) * s) + coord * s + abs(o * s) + abs(orr - o * s) + np.abs(coord * s + (orr - o * s))
        T = a * n_abs / den + 2 * abs(pa) * a * b + abs(pb) * (r2 + 2 * a * a)
        out.append(eps * pin + fr * (a * err_q + 11 * eps * T) + eps * np.abs(s64))
    return out[0], out[1]


FR1_K = np.array([517.3, 516.5, 318.6, 255.3], np.float32)


def raw_K(K):
    """a raw camera matrix near K, not equal to it (a rectified camera seldom keeps the raw one's numbers)"""
    return (np.asarray(K, np.float64) * np.array([1.013, 1.009, 0.994, 1.011])).astype(np.float32)


# ---- 1. the model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(640, 480), (321, 243)])
@pytest.mark.parametrize("lens", ["plumb_bob", "rational", "zeros"])
def test_map_equals_the_float64_model_within_float32_rounding(w, h, lens):
    K = (FR1_K * (w / 640.0)).astype(np.float32)
    K_raw = K if lens == "zeros" else raw_K(K)
    D = dict(plumb_bob=FR1_D, rational=RATIONAL_D, zeros=ZERO_D)[lens]
    sx, sy = header_map(K, K_raw, D, w, h)
    wx, wy = model_f64(K, K_raw, D, w, h)
    bx, by = map_bound(K, K_raw, D, w, h)
    ex, ey = np.abs(sx.astype(np.float64) - wx), np.abs(sy.astype(np.float64) - wy)
    largest = max(np.abs(wx).max(), np.abs(wy).max(), w, h)
    ulp = float(np.spacing(np.float32(largest)))
    print("lens %s %dx%d: max error %.3e / %.3e px, bound %.3e / %.3e px, ulp of the largest coordinate (%.1f) %.3e"
          % (lens, w, h, ex.max(), ey.max(), bx.max(), by.max(), largest, ulp))
    # the worst case of the chain is a few ulp of the largest coordinate (about 11 for the plumb-bob set, whose alternating coefficients
    # cancel at the corners; the errors met are 1-2 ulp): a bound of another order would mean the derivation is wrong
    assert bx.max() <= 16 * ulp and by.max() <= 16 * ulp
    assert np.all(ex <= bx) and np.all(ey <= by)
    if lens == "zeros":                                           # K_raw = K, D = 0: the identity, exactly
        v, u = np.mgrid[0:h, 0:w].astype(np.float32)
        assert np.array_equal(sx, u) and np.array_equal(sy, v)
    else:                                                         # ... and the lenses are no toys: pixels move at the corners
        v, u = np.mgrid[0:h, 0:w]
        assert np.hypot(wx - u, wy - v).max() > 4.0 * w / 640.0


def test_map_against_opencv_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    w, h = 640, 480
    K, K_raw = FR1_K, raw_K(FR1_K)
    for D in (FR1_D, RATIONAL_D):
        cam = np.array([[K_raw[0], 0, K_raw[2]], [0, K_raw[1], K_raw[3]], [0, 0, 1]], np.float64)
        new = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float64)
        m1, m2 = cv2.initUndistortRectifyMap(cam, D.astype(np.float64), None, new, (w, h), cv2.CV_32FC1)
        sx, sy = header_map(K, K_raw, D, w, h)
        assert np.abs(sx - m1).max() < 1e-3 and np.abs(sy - m2).max() < 1e-3    # (OpenCV's own map is float32 from a float64 chain)


# ---- 2. the host rectifier ------------------------------------------------------------------------------------------------------------

def planes(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    grey = np.clip(np.rint(127 + 70 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0) + rng.uniform(-20, 20, (h, w))), 0, 255).astype(np.uint8)
    depth = np.rint(5000 * (1.2 + 0.002 * x + 0.001 * y + 0.5 * (x > w * 0.6))).astype(np.uint16)
    depth[rng.random((h, w)) < 0.05] = 0
    return grey, depth


def tinted(grey, seed):
    rng = np.random.default_rng(seed)
    return np.clip(grey[..., None].astype(np.int32) + rng.integers(-40, 41, grey.shape + (3,)), 0, 255).astype(np.uint8)


def in_format(bgr, fmt):
    c = bgr if fmt.startswith("bgr") else bgr[..., ::-1]
    if fmt.endswith("a8"):
        c = np.concatenate([c, np.random.default_rng(7).integers(0, 256, bgr.shape[:2] + (1,), dtype=np.uint8)], -1)
    return np.ascontiguousarray(c)


def blend_f32(taps, depth_f, sx, sy, rectify_depth=True):
    """numpy restatement of lens_rectify_pixel from the header's own (sx, sy): float32 operations one at a time"""
    h, w = taps.shape
    one = np.float32(1)
    with np.errstate(invalid="ignore"):
        valid = (sx >= 0) & (sx <= np.float32(w - 1)) & (sy >= 0) & (sy <= np.float32(h - 1))
    sxv, syv = np.where(valid, sx, 0).astype(np.float32), np.where(valid, sy, 0).astype(np.float32)
    x0, y0 = np.minimum(sxv.astype(np.int32), w - 2), np.minimum(syv.astype(np.int32), h - 2)
    ax, ay = sxv - x0.astype(np.float32), syv - y0.astype(np.float32)
    bx, by = one - ax, one - ay
    t00, t10, t01, t11 = taps[y0, x0], taps[y0, x0 + 1], taps[y0 + 1, x0], taps[y0 + 1, x0 + 1]
    top, bottom = bx * t00 + ax * t10, bx * t01 + ax * t11
    I = by * top + ay * bottom
    assert I.dtype == np.float32
    if rectify_depth:
        Z = depth_f[(syv + np.float32(0.5)).astype(np.int32), (sxv + np.float32(0.5)).astype(np.int32)]
    else:
        Z = depth_f
    return np.where(valid, I, np.float32(0)), np.where(valid, Z, np.float32(np.nan)), valid


@pytest.mark.parametrize("w,h", [(64, 48), (37, 23)])
@pytest.mark.parametrize("D", [FR1_D, RATIONAL_D], ids=["plumb_bob", "rational"])
@pytest.mark.parametrize("rectify_depth", [True, False])
def test_host_rectifier_every_format_equals_the_numpy_restatement(w, h, D, rectify_depth):
    K = np.array([0.8 * w, 0.8 * w, 0.5 * w - 0.7, 0.5 * h + 0.4], np.float32)
    K_raw = raw_K(K)
    grey, depth = planes(w, h, 3)
    bgr = tinted(grey, 4)
    grey_of_bgr = tum.bgr_to_grey(bgr)
    assert np.array_equal(po.bgr_to_grey(bgr), grey_of_bgr.astype(np.float32))
    sx, sy = header_map(K, K_raw, D, w, h)
    scale = np.float32(1.0 / 5000.0)
    z_u16 = np.where(depth == 0, np.float32(np.nan), depth.astype(np.float32) * scale).astype(np.float32)
    z_f32 = (depth.astype(np.float32) * np.float32(2e-4) + np.float32(1e-5)).astype(np.float32)
    z_f32[depth == 0] = np.nan
    fimg = (grey.astype(np.float32) + np.float32(0.37)).astype(np.float32)
    want_grey = blend_f32(grey.astype(np.float32), z_u16, sx, sy, rectify_depth)
    assert want_grey[2].any() and not want_grey[2].all()          # the lens leaves an invalid border
    cases = [("grey8", grey, grey.astype(np.float32)), ("f32", fimg, fimg)]
    cases += [(fmt, in_format(bgr, fmt), grey_of_bgr.astype(np.float32)) for fmt in ("bgr8", "rgb8", "bgra8", "rgba8")]
    for fmt, image, taps in cases:
        for zplane, zf, zscale in ((depth, z_u16, float(scale)), (z_f32, (z_f32 * np.float32(0.5)).astype(np.float32), 0.5)):
            if fmt == "f32" and zplane.dtype != np.float32:
                continue                                          # (a float image comes with float depth)
            I, Z = rectify(image, zplane, K, K_raw, D, rectify_depth, fmt, zscale)
            wi, wz, _ = blend_f32(taps, zf, sx, sy, rectify_depth)
            assert np.array_equal(I.view(np.uint32), wi.view(np.uint32)), (fmt, zplane.dtype)
            assert np.array_equal(Z, wz, equal_nan=True), (fmt, zplane.dtype)
    # padded rows are the same planes
    pad = np.zeros((h, w + 5, 3), np.uint8)
    pad[:, :w] = bgr
    zpad = np.zeros((h, w + 3), np.float32)
    zpad[:, :w] = z_f32
    a = rectify(pad[:, :w], zpad[:, :w], K, K_raw, D, rectify_depth, "bgr8", 1.0)
    b = rectify(bgr, z_f32, K, K_raw, D, rectify_depth, "bgr8", 1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def test_edge_semantics_on_hand_made_planes():
    w, h = 16, 12
    K = np.array([20.0, 20.0, 7.5, 5.5], np.float32)
    rng = np.random.default_rng(0)
    fimg = rng.uniform(0, 255, (h, w)).astype(np.float32)
    depth = rng.integers(1, 60000, (h, w)).astype(np.uint16)
    fdepth = rng.uniform(0.5, 4.0, (h, w)).astype(np.float32)
    # the identity lens: every pixel is its own tap, the last column and row included (a tap exactly on w - 1 / h - 1)
    I, Z = rectify(fimg, fdepth, K, K, ZERO_D, True, "f32", 1.0)
    assert np.array_equal(I, fimg) and np.array_equal(Z, fdepth)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    I, Z = rectify(g, depth, K, K, ZERO_D, True, "grey8", 0.0002)
    assert np.array_equal(I, g.astype(np.float32)) and np.array_equal(Z, depth.astype(np.float32) * np.float32(0.0002))
    # a raw camera whose centre lies half a pixel to the right: sx = u + 0.5 exactly, so the last column is just outside
    K_half = K + np.array([0, 0, 0.5, 0], np.float32)
    sx, sy = header_map(K, K_half, ZERO_D, w, h)
    v, u = np.mgrid[0:h, 0:w].astype(np.float32)
    assert np.array_equal(sx, u + np.float32(0.5)) and np.array_equal(sy, v)
    I, Z = rectify(g, depth, K, K_half, ZERO_D, True, "grey8", 0.0002)
    assert np.all(I[:, w - 1] == 0) and np.isnan(Z[:, w - 1]).all()                     # outside: I = 0, Z = NaN
    assert np.array_equal(I[:, :w - 1], (g[:, :-1].astype(np.float32) + g[:, 1:].astype(np.float32)) * np.float32(0.5))
    assert np.array_equal(Z[:, :w - 1], depth[:, 1:].astype(np.float32) * np.float32(0.0002))   # nearest of u + 0.5: int(u + 1.0) = u + 1
    # a coordinate a hair outside the last column, and a hair inside
    for shift, inside in ((np.float32(1e-4), False), (np.float32(-1e-4), True)):
        Ks = K + np.array([0, 0, shift, 0], np.float32)
        sx, _ = header_map(K, Ks, ZERO_D, w, h)
        assert (sx[0, w - 1] <= w - 1) == inside
        I, Z = rectify(fimg, fdepth, K, Ks, ZERO_D, True, "f32", 1.0)
        assert np.isnan(Z[:, w - 1]).all() != inside and (np.all(I[:, w - 1] == 0) != inside)
    # a u16 0 under the nearest tap is a hole
    holes = depth.copy()
    holes[3, 5] = 0
    _, Z = rectify(g, holes, K, K, ZERO_D, True, "grey8", 0.0002)
    assert np.isnan(Z[3, 5]) and np.isnan(Z).sum() == 1
    # rectify_depth = 0: depth pixel for pixel where the image pixel is valid, NaN where it is not
    I, Z = rectify(g, depth, K, K_half, ZERO_D, False, "grey8", 0.0002)
    assert np.array_equal(Z[:, :w - 1], depth[:, :w - 1].astype(np.float32) * np.float32(0.0002)) and np.isnan(Z[:, w - 1]).all()
    # NaN coordinates are invalid (a lens whose denominator vanishes somewhere)
    I, Z = rectify(g, depth, K, K, np.array([0, 0, 0, 0, 0, -1.0 / 0.0625, 0, 0], np.float32), True, "grey8", 0.0002)
    assert np.isfinite(I).all()


def test_depth_is_the_nearest_pixel_never_a_mixture():
    w, h = 64, 48
    K = np.array([50.0, 50.0, 31.5, 23.5], np.float32)
    depth = np.full((h, w), 5000, np.uint16)
    depth[:, 29:] = 15000                                         # a step from 1 m to 3 m
    depth[20:, :] += 2500
    grey = np.zeros((h, w), np.uint8)
    for D in (FR1_D, RATIONAL_D):
        _, Z = rectify(grey, depth, K, raw_K(K), D, True, "grey8", 1.0 / 5000.0)
        values = set(np.unique(Z[np.isfinite(Z)]).tolist())
        source = set((np.unique(depth).astype(np.float32) * np.float32(1.0 / 5000.0)).tolist())
        assert values <= source and len(values) == 4


# ---- 3. it matters --------------------------------------------------------------------------------------------------------------------

def undistort_points_f64(K, K_raw, D, w, h, iterations=40):
    """For every RAW pixel (sx, sy) the rectified coordinate (u, v) the model maps onto it: the model inverted in float64 by fixed-point
    iteration on the normalised coordinates (cv::undistortPoints' scheme)."""
    fx, fy, ox, oy = (float(v) for v in np.asarray(K, np.float32))
    fxr, fyr, oxr, oyr = (float(v) for v in np.asarray(K_raw, np.float32))
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in _d8(D))
    sy, sx = np.mgrid[0:h, 0:w].astype(np.float64)
    xd, yd = (sx - oxr) / fxr, (sy - oyr) / fyr
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) / radial, (yd - dy) / radial
    return x * fx + ox, y * fy + oy


def distort_pair(pair, K_raw, D):
    """the pair as a camera with that lens would have delivered it: every raw pixel looks up the pinhole images where the inverted model
    says (grey: bilinear, rounded to u8; depth: nearest, 0 stays 0)"""
    h, w = pair["grey_ref"].shape
    u, v = undistort_points_f64(pair["K"], K_raw, D, w, h)
    assert u.min() >= 0 and u.max() <= w - 1 and v.min() >= 0 and v.max() <= h - 1   # (the lens magnifies: every raw pixel has a source)
    x0, y0 = np.minimum(np.floor(u).astype(int), w - 2), np.minimum(np.floor(v).astype(int), h - 2)
    ax, ay = u - x0, v - y0
    out = dict(pair)
    for view in ("ref", "cur"):
        g = pair["grey_" + view].astype(np.float64)
        blend = (1 - ay) * ((1 - ax) * g[y0, x0] + ax * g[y0, x0 + 1]) + ay * ((1 - ax) * g[y0 + 1, x0] + ax * g[y0 + 1, x0 + 1])
        out["grey_" + view] = np.clip(np.rint(blend), 0, 255).astype(np.uint8)
        out["depth_" + view] = np.ascontiguousarray(pair["depth_" + view][np.rint(v).astype(int), np.rint(u).astype(int)])
    return out


# the pair of the end-to-end checks (CPU: here; GPU: tests/test_gpu_lens_ingest.py): chosen on the CPU so that the oracle alone shows
# the effect -- a smooth synthetic scene at 320 x 240 under the fr1-like lens
MATTERS = dict(seed=42, w=320, h=240, levels=3, D=FR1_D)


@functools.lru_cache(maxsize=None)
def matters_pair():
    pair = cm.synth(MATTERS["seed"], MATTERS["w"], MATTERS["h"])
    K_raw = raw_K(pair["K"])
    return pair, distort_pair(pair, K_raw, MATTERS["D"]), K_raw


def rectified_pyramids(raw, K, K_raw, D, levels):
    return tuple(po.Pyramid(*rectify(raw["grey_" + v], raw["depth_" + v], K, K_raw, D), K, levels) for v in ("ref", "cur"))


def pose_error(T, xi_true):
    return float(np.abs(po.se3_log(np.linalg.inv(po.se3_exp(xi_true)) @ T)).max())


def test_rectification_matters_to_the_oracle():
    pair, raw, K_raw = matters_pair()
    levels = MATTERS["levels"]
    cfg = po.make_config(first_level=levels - 1, last_level=0, mode=po.MATH)
    e0 = pose_error(po.match(*po.pyramids_from_pair(pair, levels), cfg)["T"], pair["xi_true"])
    e1 = pose_error(po.match(*rectified_pyramids(raw, pair["K"], K_raw, MATTERS["D"], levels), cfg)["T"], pair["xi_true"])
    e_raw = pose_error(po.match(*po.pyramids_from_pair(raw, levels), cfg)["T"], pair["xi_true"])
    print("pose error (largest twist component against the scene's true warp): original pair e0 = %.3e, distorted pair rectified "
          "e1 = %.3e, distorted pair as it is e_raw = %.3e" % (e0, e1, e_raw))
    assert e_raw > 3 * e1


# ---- 4. wrappers and facade -------------------------------------------------------------------------------------------------------------

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
    K = [517.3, 516.5, 318.6, 255.3]
    bad = [
        (ValueError, (K[:3], FR1_D)),                              # K_raw: four numbers
        (ValueError, (np.zeros((2, 2)), FR1_D)),
        (ValueError, (K, FR1_D[:3])),                              # D: 4, 5 or 8
        (ValueError, (K, FR1_D[:6])),
        (ValueError, (K, np.zeros((2, 4)))),
        (ValueError, (K, [0.1, np.nan, 0, 0])),                    # finite
        (ValueError, ([np.inf, 500, 300, 200], FR1_D)),
        (ValueError, (K, [1e39, 0, 0, 0])),                        # (infinite as float32)
        (ValueError, ([0.0, 500, 300, 200], FR1_D)),               # positive focal lengths
        (ValueError, ([500, -1.0, 300, 200], FR1_D)),
        (TypeError, (K, np.array(["a", "b", "c", "d"]))),          # numbers
        (TypeError, (np.array([1 + 2j, 1, 1, 1]), FR1_D)),
        (TypeError, (K, None)),
    ]
    for exc, (k, dd) in bad:
        with pytest.raises(exc):
            d.set_lens_batch(pyrs, k, dd)
        with pytest.raises(exc):
            d.RgbdImagePyramid.set_lens(pyrs[0], k, dd)
    with pytest.raises(TypeError):
        d.set_lens_batch(pyrs, K, FR1_D, rectify_depth="yes")
    with pytest.raises(ValueError):
        d.set_lens_batch([], K, FR1_D)
    with pytest.raises(ValueError):
        d.clear_lens_batch([])
    for n in (4, 5, 8):                                            # D is padded with zeros
        lens = d.lens_struct(K, FR1_D[:n], rectify_depth=False)
        assert list(lens.D) == [float(v) for v in FR1_D[:n]] + [0.0] * (8 - n) and lens.rectify_depth == 0 and lens.reserved == 0
        assert list(lens.K_raw) == [float(np.float32(v)) for v in K]
    assert C.sizeof(_lib.Lens) == 56
    assert d.lens_struct(K, FR1_D).rectify_depth == 1


def test_header_declares_the_lens():
    text = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    assert "typedef struct {\n  float K_raw[4];" in text and "} dvo_hip_lens;" in text
    for name in ("dvo_hip_frames_set_lens", "dvo_hip_frames_clear_lens"):
        assert "int %s(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames" % name in text
        assert name in _lib.EXPORTS
    assert '"lens_ingests"' in text


def build_lens_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "lens_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "lens_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_lens_methods_compile():
    d.build()
    assert os.path.exists(build_lens_facade_check())
