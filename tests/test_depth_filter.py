"""CPU tier: the depth filter of the ingest (include/dvo_hip.h, dvo_hip_frames_set_depth_filter).
  * dvo_slam_amd/csrc/depth_filter.h (the rule k_depth_filter inlines) compiled for the host with g++ -Wall -Werror
    -ffp-contract=off: filt(P, params) is the yardstick the device planes are held to bit for bit (tests/test_gpu_depth_filter.py);
  * its tables against numpy's float64 exp, and a numpy float32 restatement of the per-pixel rule against it, bit for bit;
  * hand-made planes: constant, radius 0, a step, an outlier, a hole, the gate;
  * noise on a slanted plane is lower after filtering; mixed pixels of a step scene are gone and little else;
  * the oracle's pose error on a noisy pair with and without the filter: printed and recorded (profiles/depth_filter.md), not asserted;
  * the Python wrappers reject bad arguments before anything reaches the library; the C++ facade's setDepthFilter / clearDepthFilter
    compile (tests/cpp/depth_filter_facade_check.cpp)."""
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
SCALE = 1.0 / 5000.0
HOLE_BITS = 0x7FC00000

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include <vector>
#include "depth_filter.h"
using namespace dvo_hip;
extern "C" {
// null: acceptable, else what depth_filter_check says
const char* filt_host_check(const dvo_hip_depth_filter* f) { return depth_filter_check(*f); }
void filt_host_default(dvo_hip_depth_filter* f) { *f = depth_filter_default_params(); }
int filt_host_prepared_bytes() { return int(sizeof(DepthFilterPrepared)); }
void filt_host_tables(const dvo_hip_depth_filter* f, float* ws49, float* wr64) {
  const DepthFilterPrepared P = depth_filter_prepare(*f);
  std::memcpy(ws49, P.ws, sizeof P.ws);
  std::memcpy(wr64, P.wr, sizeof P.wr);
}
// depth_format: DVO_HIP_DEPTH_*; pitch in bytes; out: w * h floats, tight
void filt_host(const dvo_hip_depth_filter* f, int w, int h, const unsigned char* depth, int depth_format, size_t pitch, float scale, float* out) {
  const DepthFilterPrepared P = depth_filter_prepare(*f);
  std::vector<float> z(size_t(w) * h);
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) {
      const unsigned char* p = depth + size_t(v) * pitch + size_t(u) * (depth_format == DVO_HIP_DEPTH_F32 ? 4 : 2);
      if (depth_format == DVO_HIP_DEPTH_F32) { float x; std::memcpy(&x, p, 4); z[size_t(v) * w + u] = depth_of_f32(x, scale); }
      else { uint16_t r; std::memcpy(&r, p, 2); z[size_t(v) * w + u] = depth_of_u16(r, scale); }
    }
  depth_filter_plane(P, z.data(), w, h, w, out);
}
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    """depth_filter.h compiled for the host: g++, every warning an error, no contraction (what the header's pragma says to clang)"""
    tmp = tempfile.mkdtemp(prefix="depth_filter_host_")
    src, out = os.path.join(tmp, "depth_filter_host.cpp"), os.path.join(tmp, "depth_filter_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    fp, vp, pp = C.POINTER(C.c_float), C.c_void_p, C.POINTER(_lib.DepthFilter)
    L.filt_host_check.argtypes = [pp]
    L.filt_host_check.restype = C.c_char_p
    L.filt_host_default.argtypes = [pp]
    L.filt_host_tables.argtypes = [pp, fp, fp]
    L.filt_host.argtypes = [pp, C.c_int, C.c_int, vp, C.c_int, C.c_size_t, C.c_float, fp]
    for f in (L.filt_host_default, L.filt_host_tables, L.filt_host):
        f.restype = None
    return L


def _format(depth):
    assert depth.dtype in (np.float32, np.uint16) and depth.strides[1] == depth.itemsize
    return _lib.DEPTH_F32 if depth.dtype == np.float32 else _lib.DEPTH_U16


def filt(depth, params, depth_scale=1.0):
    """filt(P): the filtered float plane of the depth plane P as depth_filter.h defines it, computed on the host.  depth: [h, w] uint16 or
    float32, rows may be padded (the array's own stride is the pitch); params: the keyword arguments of set_depth_filter."""
    h, w = depth.shape
    out = np.empty((h, w), np.float32)
    s = d.depth_filter_struct(**params)
    host_lib().filt_host(C.byref(s), w, h, depth.ctypes.data, _format(depth), depth.strides[0], depth_scale, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def tables(params):
    ws, wr = np.empty((7, 7), np.float32), np.empty(64, np.float32)
    s = d.depth_filter_struct(**params)
    host_lib().filt_host_tables(C.byref(s), ws.ctypes.data_as(C.POINTER(C.c_float)), wr.ctypes.data_as(C.POINTER(C.c_float)))
    return ws, wr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def is_hole(a):
    return bits(a) == HOLE_BITS


# parameter sets the tests walk: the defaults, every reach at its largest, the edge rule alone, erosion alone, a narrow gate
PARAMS = [
    dict(),
    dict(radius=3, sigma_space=2.0, edge_radius=2, hole_radius=2),
    dict(radius=0, edge_radius=2, hole_radius=0),
    dict(radius=1, sigma_space=0.7, edge_radius=0, hole_radius=1),
    dict(radius=2, gate=1.5, noise_a=0.004, noise_b=0.0, edge_radius=1, edge_abs=0.02, edge_rel=0.0, hole_radius=1),
]


# ---- 1. the tables ----------------------------------------------------------------------------------------------------------------------

def ulps(a, b):
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.mark.parametrize("params", PARAMS[:2] + PARAMS[3:])
def test_tables_agree_with_float64_exp(params):
    p = dict(d.depth_filter_default(), **params)
    ws, wr = tables(params)
    dy, dx = np.mgrid[-3:4, -3:4].astype(np.float64)
    want_ws = np.exp(-(dx * dx + dy * dy) / (2.0 * float(np.float32(p["sigma_space"])) ** 2)).astype(np.float32)
    r = p["radius"]
    inside = (np.abs(dx) <= r) & (np.abs(dy) <= r)
    assert ulps(ws[inside], want_ws[inside]).max() <= 1
    assert np.all(ws[~inside] == 0.0) and ws[3, 3] == 1.0
    b = np.arange(64, dtype=np.float64)
    want_wr = np.exp(-0.5 * ((b + 0.5) * float(np.float32(p["gate"])) / 64.0) ** 2).astype(np.float32)
    assert ulps(wr, want_wr).max() <= 1 and np.all(np.diff(wr) < 0) and wr[0] < 1.0
    assert host_lib().filt_host_prepared_bytes() < 512


# ---- 2. a numpy float32 restatement ------------------------------------------------------------------------------------------------------

def shifted(z, dy, dx):
    """(the plane moved so that element [y, x] is z[y + dy, x + dx], which of its elements lie in the image)"""
    h, w = z.shape
    out = np.full((h, w), np.nan, np.float32)
    inside = np.zeros((h, w), bool)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    yt, xt = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
    out[ys, xs] = z[yt, xt]
    inside[ys, xs] = True
    return out, inside


def filt_numpy(z, params):
    """the per-pixel rule of depth_filter.h on a plane of CONVERTED depths, every operation a float32 numpy operation of its own, fed the
    host build's tables"""
    p = dict(d.depth_filter_default(), **params)
    f32 = np.float32
    ws, wr = tables(params)
    z = np.ascontiguousarray(z, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        valid = np.isfinite(z) & (z > 0)
        tau = f32(p["edge_abs"]) + f32(p["edge_rel"]) * z
        rejected = np.zeros(z.shape, bool)
        reach = max(p["edge_radius"], p["hole_radius"])
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                zn, inside = shifted(z, dy, dx)
                vn = inside & np.isfinite(zn) & (zn > 0)
                cheb = max(abs(dx), abs(dy))
                if cheb <= p["hole_radius"]:
                    rejected |= inside & ~vn
                if cheb <= p["edge_radius"]:
                    rejected |= vn & (np.abs(zn - z) > tau)
        out = z.copy()
        r = p["radius"]
        if r > 0:
            inv = f32(64.0) / (f32(p["gate"]) * (f32(p["noise_a"]) + f32(p["noise_b"]) * (z * z)))
            acc_w, acc_d = np.zeros(z.shape, f32), np.zeros(z.shape, f32)
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    zn, inside = shifted(z, dy, dx)
                    dd = zn - z
                    t = np.abs(dd) * inv
                    take = inside & np.isfinite(zn) & (zn > 0) & (t < f32(64.0))
                    bin_ = np.where(take, t, 0).astype(np.int32)
                    wgt = ws[dy + 3, dx + 3] * wr[bin_]
                    acc_w = np.where(take, acc_w + wgt, acc_w)
                    acc_d = np.where(take, acc_d + wgt * dd, acc_d)
            out = z + acc_d / acc_w
            assert out.dtype == np.float32 and acc_w.dtype == np.float32
    out = bits(out).copy()
    out[~valid | rejected] = HOLE_BITS
    return out.view(np.float32)


def busy_plane(w, h, seed=0):
    """u16 depth with everything in it: a slanted wall, two foreground slabs (steps), mixed pixels at one slab's border, holes of every
    size, sensor noise growing with z * z"""
    rng = np.random.default_rng([seed, w, h])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 1.8 + 1.6 * x / w + 0.5 * y / h
    z[h // 5:3 * h // 5, w // 4:w // 2] = 0.9 + 0.1 * x[h // 5:3 * h // 5, w // 4:w // 2] / w
    z[h // 2:, 2 * w // 3:2 * w // 3 + max(3, w // 10)] = 1.2
    z[h // 5 - 1, w // 4:w // 2] = 0.5 * (z[h // 5 - 2, w // 4:w // 2] + z[h // 5, w // 4:w // 2])        # a row of flying pixels
    z += rng.normal(0, 1, (h, w)) * (0.0012 + 0.0019 * z * z)
    raw = np.rint(z * 5000).astype(np.uint16)
    raw[rng.random((h, w)) < 0.02] = 0
    for _ in range(4):
        x0, y0, rw, rh = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(1, 9)), int(rng.integers(1, 9))
        raw[y0:y0 + rh, x0:x0 + rw] = 0
    raw[0, : w // 3] = 0                                         # holes on the border and in a corner
    raw[h - 2:, w - 2:] = 0
    return raw


def converted(raw, scale=SCALE):
    z = raw.astype(np.float32) * np.float32(scale)
    z[raw == 0] = np.nan
    return z


@pytest.mark.parametrize("w,h", [(102, 78), (33, 9)])
@pytest.mark.parametrize("params", PARAMS)
def test_numpy_float32_restatement_equals_the_yardstick(w, h, params):
    raw = busy_plane(w, h)
    got = filt(raw, params, SCALE)
    want = filt_numpy(converted(raw), params)
    assert same_bits(got, want)
    p = dict(d.depth_filter_default(), **params)
    holes, kept = is_hole(got), ~is_hole(got)
    assert holes.any() and kept.any() and not np.isnan(got[kept]).any()
    if p["radius"] > 0:
        assert (bits(got)[kept] != bits(converted(raw))[kept]).any()
    if p["edge_radius"] > 0 or p["hole_radius"] > 0:
        assert (holes & (raw != 0)).any()
    # the float source of the same depths gives the same plane
    fz = np.where(raw == 0, np.nan, raw.astype(np.float32)).astype(np.float32)
    assert same_bits(filt(fz, params, SCALE), got)


# ---- 3. hand-made planes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", PARAMS)
def test_a_constant_plane_returns_its_own_bits(params):
    z = np.full((20, 31), 1.2345678, np.float32)
    assert same_bits(filt(z, params), z)


def test_radius_0_returns_the_bits_of_kept_pixels():
    raw = busy_plane(102, 78)
    for params in (dict(radius=0, edge_radius=0), dict(radius=0, edge_radius=2, hole_radius=1)):
        got = filt(raw, params, SCALE)
        kept = ~is_hole(got)
        assert kept.any() and np.array_equal(bits(got)[kept], bits(converted(raw))[kept])
    assert np.array_equal(~is_hole(filt(raw, dict(radius=0, edge_radius=0), SCALE)), raw != 0)


@pytest.mark.parametrize("edge_radius", [1, 2])
def test_a_vertical_step_loses_edge_radius_columns_on_each_side(edge_radius):
    z = np.full((24, 40), 1.0, np.float32)
    z[:, 20:] = 2.0                                              # |step| = 1 > tau(2.0) = 0.07 > tau(1.0)
    got = filt(z, dict(edge_radius=edge_radius))
    gone = is_hole(got)
    want = np.zeros_like(gone)
    want[:, 20 - edge_radius:20 + edge_radius] = True
    assert np.array_equal(gone, want)
    assert same_bits(got[~gone], z[~gone])                       # (the gate: no tap of the other side moves a kept pixel)


@pytest.mark.parametrize("edge_radius", [1, 2])
def test_an_isolated_outlier_goes_with_its_neighbours_within_edge_radius(edge_radius):
    z = np.full((21, 21), 1.5, np.float32)
    z[10, 10] = 1.9                                              # a flying pixel: 0.4 from the wall, tau(1.5) = 0.055, tau(1.9) = 0.067
    gone = is_hole(filt(z, dict(edge_radius=edge_radius)))
    want = np.zeros_like(gone)
    want[10 - edge_radius:11 + edge_radius, 10 - edge_radius:11 + edge_radius] = True      # the pixel and its Chebyshev ball
    assert np.array_equal(gone, want)
    # without the edge rule nothing goes, and the gate keeps the outlier out of every neighbour's mean
    got = filt(z, dict(edge_radius=0, radius=3, sigma_space=2.0))
    assert not is_hole(got).any() and same_bits(got, z)


@pytest.mark.parametrize("hole_radius", [0, 1, 2])
def test_a_hole_erodes_its_ring_and_the_border_erodes_nothing(hole_radius):
    z = np.full((19, 23), 2.0, np.float32)
    z[9, 11] = np.nan
    z[0, 0] = 0.0                                                # (an invalid value in the corner: not NaN, still a hole)
    gone = is_hole(filt(z, dict(hole_radius=hole_radius, edge_radius=0)))
    want = np.zeros_like(gone)
    want[9 - hole_radius:10 + hole_radius, 11 - hole_radius:12 + hole_radius] = True
    want[0:1 + hole_radius, 0:1 + hole_radius] = True
    assert np.array_equal(gone, want)
    clean = np.full((19, 23), 2.0, np.float32)
    assert not is_hole(filt(clean, dict(hole_radius=2, edge_radius=2, radius=3, sigma_space=1.0))).any()


def test_a_tap_across_a_step_never_moves_a_kept_pixel():
    rng = np.random.default_rng(11)
    near = (1.0 + rng.normal(0, 0.002, (30, 20))).astype(np.float32)
    far = (1.2 + rng.normal(0, 0.002, (30, 20))).astype(np.float32)          # 0.2 apart: 64 bins end at gate * sigma(1.0) = 0.0093
    both = np.concatenate([near, far], axis=1)
    params = dict(radius=3, sigma_space=2.0, edge_radius=0)
    got = filt(both, params)
    # every pixel further than the window from the step equals the filter of its own side alone; so does every pixel AT the step,
    # once the other side is replaced by holes (taps that do not count)
    alone = both.copy()
    alone[:, 20:] = np.nan
    assert same_bits(got[:, :20], filt(alone, params)[:, :20])
    assert (bits(got[:, :20]) != bits(near)).mean() > 0.9       # (and the filter did smooth)


# ---- 4. what it is for -------------------------------------------------------------------------------------------------------------------

def noise_sigma(z, p):
    return p["noise_a"] + p["noise_b"] * z * z


def test_noise_on_a_slanted_plane_is_lower_after_filtering():
    p = d.depth_filter_default()
    h, w = 120, 160
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    truth = 1.0 + 1.8 * x / w + 0.3 * y / h
    noisy = (truth + np.random.default_rng(2).normal(0, 1, (h, w)) * noise_sigma(truth, p)).astype(np.float32)
    got = filt(noisy, {})
    kept = ~is_hole(got)
    before = float(np.sqrt(np.mean((noisy[kept] - truth[kept]) ** 2)))
    after = float(np.sqrt(np.mean((got[kept].astype(np.float64) - truth[kept]) ** 2)))
    print("RMS error against the true plane: before %.4e m, after %.4e m, ratio %.3f, %.4f of the pixels kept" % (before, after, after / before, kept.mean()))
    assert kept.mean() > 0.5 and after < before


def mixed_step_scene(w=160, h=120):
    """a wall at 2 m with a slab at 1 m in front of it; the slab's outermost ring of pixels is MIXED: the mean of both surfaces"""
    z = np.full((h, w), 2.0, np.float32)
    x0, x1, y0, y1 = w // 4, 3 * w // 4, h // 4, 3 * h // 4
    z[y0:y1, x0:x1] = 1.5
    z[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = 1.0
    return z, (x1 - x0, y1 - y0)


def test_mixed_pixels_of_a_step_scene_are_gone_and_little_else():
    p = d.depth_filter_default()
    z, (bw, bh) = mixed_step_scene()
    n_mixed = int((z == 1.5).sum())
    assert n_mixed == 2 * (bw + bh) - 4

    def floating(plane):
        """valid pixels further than tau(z) from both surfaces"""
        v = ~is_hole(plane) & np.isfinite(plane)
        tau = p["edge_abs"] + p["edge_rel"] * plane
        with np.errstate(invalid="ignore"):
            return int((v & (np.abs(plane - 1.0) > tau) & (np.abs(plane - 2.0) > tau)).sum())

    assert floating(z) == n_mixed                                # without the filter: every mixed pixel hangs between the surfaces
    got = filt(z, dict(edge_radius=1))
    assert floating(got) == 0
    # the edge is a closed outline of 2 (bw + bh) - 4 pixels; with edge_radius 1 the rule removes that ring and at most one ring on
    # each side of it, 3 rings of at most 2 (bw + bh) + 4 pixels each (the outer one is the longest): the share of the image below
    share = 3.0 * (2 * (bw + bh) + 4) / z.size
    removed = int(is_hole(got).sum())
    print("removed %d of %d pixels (%.4f), bound %.4f" % (removed, z.size, removed / z.size, share))
    assert n_mixed <= removed < share * z.size and share < 0.07


NOISY = dict(seed=3, w=320, h=240, levels=3)


def pose_error(T, xi_true):
    return float(np.abs(po.se3_log(np.linalg.inv(po.se3_exp(xi_true)) @ T)).max())


def test_oracle_pose_error_with_and_without_the_filter_is_recorded():
    """Nobody has measured whether the filter improves the oracle's pose on a noisy pair: both errors are printed (and recorded in
    profiles/depth_filter.md), nothing is asserted about their order."""
    p = d.depth_filter_default()
    pair = scenes.edge_scene(NOISY["seed"], NOISY["w"], NOISY["h"])
    rng = np.random.default_rng(17)
    noisy = dict(pair)
    for v in ("ref", "cur"):
        z = pair["depth_" + v].astype(np.float64) * SCALE
        z = z + rng.normal(0, 1, z.shape) * noise_sigma(z, p)
        noisy["depth_" + v] = np.where(pair["depth_" + v] == 0, 0, np.clip(np.rint(z * 5000), 1, 65535)).astype(np.uint16)
    levels = NOISY["levels"]
    cfg = po.make_config(first_level=levels - 1, last_level=0, mode=po.MATH)
    e_clean = pose_error(po.match(*po.pyramids_from_pair(pair, levels), cfg)["T"], pair["xi_true"])
    e_noisy = pose_error(po.match(*po.pyramids_from_pair(noisy, levels), cfg)["T"], pair["xi_true"])
    filtered = tuple(po.Pyramid(noisy["grey_" + v].astype(np.float32), filt(noisy["depth_" + v], {}, SCALE), pair["K"], levels) for v in ("ref", "cur"))
    e_filt = pose_error(po.match(*filtered, cfg)["T"], pair["xi_true"])
    print("pose error (largest twist component against the scene's true warp): clean depth %.3e, noisy depth %.3e, noisy depth through "
          "the default filter %.3e" % (e_clean, e_noisy, e_filt))
    assert all(np.isfinite(e) for e in (e_clean, e_noisy, e_filt))


# ---- 5. wrappers and facade -------------------------------------------------------------------------------------------------------------

class _NoLibrary:
    """stands in for a context: any use of the library is a test failure"""
    ptr = None

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


class _Pyramid:
    def __init__(self):
        self.ctx, self.ptr = _NoLibrary(), None


BAD_PARAMS = [
    (ValueError, dict(radius=4)), (ValueError, dict(radius=-1)), (ValueError, dict(edge_radius=3)), (ValueError, dict(hole_radius=3)),
    (ValueError, dict(hole_radius=-1)), (ValueError, dict(sigma_space=0.0)), (ValueError, dict(sigma_space=-1.0)), (ValueError, dict(gate=0.0)),
    (ValueError, dict(gate=-3.0)), (ValueError, dict(noise_a=-1e-3)), (ValueError, dict(noise_b=-1e-3)), (ValueError, dict(edge_abs=-0.01)),
    (ValueError, dict(edge_rel=-0.01)), (ValueError, dict(noise_a=0.0, noise_b=0.0)), (ValueError, dict(gate=float("nan"))),
    (ValueError, dict(edge_abs=float("inf"))), (ValueError, dict(noise_b=1e39)), (TypeError, dict(radius=1.5)), (TypeError, dict(gate="3")),
    (TypeError, dict(sigma_space=None)), (TypeError, dict(sigma=1.0)), (TypeError, dict(edge_radius=True)),
]


def test_wrappers_reject_bad_arguments_before_the_library():
    pyrs = [_Pyramid(), _Pyramid()]
    for exc, params in BAD_PARAMS:
        with pytest.raises(exc):
            d.set_depth_filter_batch(pyrs, **params)
        with pytest.raises(exc):
            d.RgbdImagePyramid.set_depth_filter(pyrs[0], **params)
    with pytest.raises(ValueError):
        d.set_depth_filter_batch([])
    with pytest.raises(ValueError):
        d.clear_depth_filter_batch([])
    s = d.depth_filter_struct(radius=0, sigma_space=0.0)          # (sigma_space is not read without a window)
    assert s.radius == 0 and list(s.reserved) == [0, 0]
    assert C.sizeof(_lib.DepthFilter) == 44


def test_the_header_checks_what_the_wrapper_checks_and_shares_its_defaults():
    L = host_lib()
    s = _lib.DepthFilter()
    L.filt_host_default(C.byref(s))
    want = d.depth_filter_default()
    assert {k: getattr(s, k) for k in want} == {k: (v if isinstance(v, int) else float(np.float32(v))) for k, v in want.items()}
    assert list(s.reserved) == [0, 0] and L.filt_host_check(C.byref(s)) is None
    for exc, params in BAD_PARAMS:
        if exc is TypeError or "noise_b" in params and params["noise_b"] > 1:
            continue
        t = _lib.DepthFilter.from_buffer_copy(s)
        for k, v in params.items():
            setattr(t, k, v)
        assert L.filt_host_check(C.byref(t)) is not None, params
    t = _lib.DepthFilter.from_buffer_copy(s)
    t.reserved[1] = 1
    assert L.filt_host_check(C.byref(t)) is not None


def test_header_declares_the_depth_filter():
    text = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    assert "typedef struct {\n  int32_t radius;" in text and "} dvo_hip_depth_filter;" in text
    for name in ("dvo_hip_frames_set_depth_filter", "dvo_hip_frames_clear_depth_filter"):
        assert "int %s(dvo_hip_context* ctx, int n_frames, dvo_hip_frame* const* frames" % name in text
        assert name in _lib.EXPORTS
    assert '"depth_filter_ingests"' in text and "dvo_hip_depth_filter_default" in _lib.EXPORTS
    comment = open(os.path.join(CSRC, "depth_filter.h")).read()
    assert "NOT VERIFIED" in comment and "no decision cascades" in comment


def build_depth_filter_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "depth_filter_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "depth_filter_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_depth_filter_methods_compile():
    d.build()
    assert os.path.exists(build_depth_filter_facade_check())
