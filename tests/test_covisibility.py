"""Keyframe covisibility, CPU tier (dvo_slam_amd/csrc/covisibility.h; include/dvo_hip.h, dvo_hip_frames_covisibility).

covisibility.h is compiled for the host (g++, -ffp-contract=off) the way tests/test_frame_warp.py compiles frame_warp.h, and exposed as
covisibility_host(): the yardstick the device records are compared with in tests/test_gpu_covisibility.py.  Here it is held to an
independent numpy statement of the header's five steps, to hand-made planes that show every class alone, and the Python logic above
the device call (covisibility_matrix, overlap, loop_closure_candidates) runs with the host build in the call's place.
"""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cameras
import dvo_slam_amd as d
import scenes
from test_frame_warp import CSRC, K8, ROOT, TILT, FakeCamera, FakePyramid, _k, _plane, _t, flat, np_point, scene_pair, shift

INF = float("inf")
f32 = np.float32
FIELDS = ("valid", "in_view", "unknown", "occluded", "seen_through", "consistent", "photo")

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include "covisibility.h"
using namespace dvo_hip;
extern "C" {
// the record of one ordered pair over tight planes: a (wa x ha, Ka) as b (wb x hb, Kb) sees it under T16 (a's camera -> b's camera).
// The record is summed in the four 64-bit words the kernel adds in (covis_words) and copied out as they lie.
void covisibility_host(const float* Ia, const float* Za, const float* Ib, const float* Zb, const float* Ka, const float* Kb, int wa, int ha,
                       int wb, int hb, const double* T16, const dvo_hip_covis_params* par, dvo_hip_covis_record* out) {
  const MapPose T = map_pose_prepare(T16);
  const auto tap = [&](int xx, int yy) { return WarpTap{Ib[size_t(yy) * wb + xx], Zb[size_t(yy) * wb + xx]}; };
  uint64_t words[4] = {0, 0, 0, 0};
  for (int y = 0; y < ha; ++y)
    for (int x = 0; x < wa; ++x) {
      const size_t i = size_t(y) * wa + x;
      uint32_t q;
      const int c = covis_pixel(T, Ka, Kb, wb, hb, *par, x, y, Ia[i], Za[i], tap, &q);
      const CovisWords w = covis_words(c, q);
      for (int k = 0; k < 4; ++k) words[k] += w.w[k];
    }
  static_assert(sizeof(dvo_hip_covis_record) == sizeof words, "the record is four 64-bit words");
  std::memcpy(out, words, sizeof words);
}
unsigned covis_host_photo(float Ia, float Ib) { return covis_photo(Ia, Ib); }
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    """covisibility.h compiled for the host: g++, every warning an error, no contraction (what the header's pragma says to clang)"""
    tmp = tempfile.mkdtemp(prefix="covisibility_host_")
    src, out = os.path.join(tmp, "covisibility_host.cpp"), os.path.join(tmp, "covisibility_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.covisibility_host.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), vp, vp]
    L.covisibility_host.restype = None
    L.covis_host_photo.argtypes = [C.c_float, C.c_float]
    L.covis_host_photo.restype = C.c_uint
    return L


def covisibility_host(Ia, Za, Ib, Zb, Ka, Kb, T, depth_tolerance=0.05, depth_tolerance_rel=0.0, min_depth=0.0, max_depth=INF):
    """covisibility_host(): the record (a COVIS_DTYPE scalar) of planes Ia, Za as the camera of planes Ib, Zb sees them under T (a's
    camera -> b's camera), as covisibility.h defines it, computed on the host"""
    Za, Zb = _plane(Za), _plane(Zb)
    Ia, Ib, Ka, Kb, T = _plane(Ia, Za.shape), _plane(Ib, Zb.shape), _k(Ka), _k(Kb), _t(T)
    par = d.covis_params_struct(depth_tolerance, depth_tolerance_rel, min_depth, max_depth)
    out = np.zeros(1, d.COVIS_DTYPE)
    host_lib().covisibility_host(Ia.ctypes.data, Za.ctypes.data, Ib.ctypes.data, Zb.ctypes.data, Ka.ctypes.data, Kb.ctypes.data, Za.shape[1],
                                 Za.shape[0], Zb.shape[1], Zb.shape[0], T.ctypes.data_as(C.POINTER(C.c_double)), C.addressof(par), out.ctypes.data)
    return out[0]


def as_dict(r):
    return {k: int(r[k]) for k in FIELDS}


def holds_invariant(r):
    return r["in_view"] == r["unknown"] + r["occluded"] + r["seen_through"] + r["consistent"] and r["in_view"] <= r["valid"]


# ---- the numpy float32 statement of covisibility.h, steps 1-5 ---------------------------------------------------------------------------

def np_covisibility(Ia, Za, Ib, Zb, Ka, Kb, T, depth_tolerance=0.05, depth_tolerance_rel=0.0, min_depth=0.0, max_depth=INF):
    """whole planes at a time, every operation rounded to float32 on its own; returns the record as a dict"""
    Ia, Za, Ib, Zb, Ka, Kb, T = _plane(Ia), _plane(Za), _plane(Ib), _plane(Zb), _k(Ka), _k(Kb), _t(T)
    hb, wb = Zb.shape
    tol0, rel, lo, hi = f32(depth_tolerance), f32(depth_tolerance_rel), f32(min_depth), f32(max_depth)
    with np.errstate(all="ignore"):
        valid = np.isfinite(Za) & (Za > 0)                                                      # step 1
        if lo > 0 or not hi >= f32(3.402823466e+38):                                            # the range is on (selection.h)
            valid &= (Za >= lo) & (Za <= hi)
        X, Y, p = np_point(T, Ka, Za)                                                           # step 2
        front = valid & np.isfinite(p[2]) & (p[2] > 0)
        u, v = (p[0] * Kb[0]) / p[2] + Kb[2], (p[1] * Kb[1]) / p[2] + Kb[3]                     # step 3
        xr, yr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        in_view = front & (xr >= 0) & (xr < f32(wb)) & (yr >= 0) & (yr < f32(hb))
        xi, yi = np.where(in_view, xr, 0).astype(np.int64), np.where(in_view, yr, 0).astype(np.int64)
        zb, ib = Zb[yi, xi], Ib[yi, xi]                                                         # step 4
        known = in_view & np.isfinite(zb)
        tol = (tol0 + rel * p[2]).astype(f32)                                                   # step 5
        dz = (zb - p[2]).astype(f32)
        occluded = known & (dz < -tol)
        seen_through = known & (dz > tol)
        consistent = known & ~occluded & ~seen_through
        e = np.abs((Ia - ib).astype(f32))
        q = np.where(e < 4096, np.floor(np.where(e < 4096, e, 0) * f32(16.0) + f32(0.5)), 65535).astype(np.uint64)
    assert X.dtype == Y.dtype == p[2].dtype == u.dtype == xr.dtype == tol.dtype == f32
    return dict(valid=int(valid.sum()), in_view=int(in_view.sum()), unknown=int((in_view & ~known).sum()), occluded=int(occluded.sum()),
                seen_through=int(seen_through.sum()), consistent=int(consistent.sum()), photo=int(q[consistent].sum()))


# ---- 1. and 5. the host build equals the numpy statement, on scenes that exercise it ------------------------------------------------------

# small motions beside the pairs' own and TILT: a few centimetres and degrees
MOTIONS = {"tilt": TILT,
           "sway": scenes.se3_exp([0.03, 0.02, -0.02, -0.03, 0.04, 0.02]),
           "back": scenes.se3_exp([-0.02, 0.01, 0.06, 0.02, -0.02, -0.03])}


# The cases that do not meet the conditions of section 5 below (worked out on the host build, which they are conditions FOR): under TILT
# the tele camera's image moves by 48 of 128 pixels and a quarter of it stays in view; the camera whose principal point lies outside
# the image sees the scene in a third of its pixels, and of those none stays within 5 cm under `sway` and `back`, or at level 2.
LEFT_OUT = {("tele", "tilt"), ("outside", "sway"), ("outside", "back"), ("outside", "own", 2), ("outside", "own, backwards", 2)}


def equality_cases(name):
    """(label, level, (Ka, Ia, Za), (Kb, Ib, Zb), T) of scene pair `name`: the pair's own motion both ways at every level, and the
    reference view against the current one under each of MOTIONS composed with the pair's motion"""
    pyramid, T = scene_pair(name)
    for level, (K, ref, cur) in enumerate(pyramid):
        cases = [("own", (K,) + ref, (K,) + cur, T), ("own, backwards", (K,) + cur, (K,) + ref, np.linalg.inv(T))]
        cases += [(label, (K,) + ref, (K,) + cur, M @ T) for label, M in MOTIONS.items()]
        for label, A, B, M in cases:
            if (name, label) not in LEFT_OUT and (name, label, level) not in LEFT_OUT:
                yield label, level, A, B, M


@pytest.mark.parametrize("name", cameras.NAMES)
def test_host_build_equals_the_numpy_statement(name):
    for label, level, (Ka, Ia, Za), (Kb, Ib, Zb), T in equality_cases(name):
        for kw in (dict(), dict(depth_tolerance=0.01, depth_tolerance_rel=0.02, min_depth=0.7, max_depth=2.5)):
            want = np_covisibility(Ia, Za, Ib, Zb, Ka, Kb, T, **kw)
            got = covisibility_host(Ia, Za, Ib, Zb, Ka, Kb, T, **kw)
            assert as_dict(got) == want, (name, label, level, kw)
            assert holds_invariant(got)
        # 5. not a comparison of empty counts (the default parameters): conditions on the scene, met by every case listed
        want = np_covisibility(Ia, Za, Ib, Zb, Ka, Kb, T)
        assert want["in_view"] > 0.3 * Za.size, (name, label, level, want)
        assert min(want["unknown"], want["occluded"], want["consistent"]) >= 1, (name, label, level, want)


def test_two_sizes_and_cameras():
    """a at 128 x 96 under fr1, b at 64 x 48 under another camera model: the point lands in b's raster, by b's K"""
    (Ka, ref, _), T = scene_pair("fr1")[0][0], scene_pair("fr1")[1]
    small, _ = scene_pair("aniso", 5, 64, 48, 1)
    Kb, _, cur = small[0]
    for A, B, M in (((Ka,) + ref, (Kb,) + cur, T), ((Kb,) + cur, (Ka,) + ref, np.linalg.inv(T))):
        want = np_covisibility(A[1], A[2], B[1], B[2], A[0], B[0], M)
        assert as_dict(covisibility_host(A[1], A[2], B[1], B[2], A[0], B[0], M)) == want
        assert want["in_view"] > 0.1 * A[2].size and want["valid"] > want["in_view"], want


# ---- 2. the self pair under the identity -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cameras.NAMES)
def test_self_pair_under_the_identity(name):
    """every valid pixel lands on itself: floorf(u + 0.5f) is x whatever the last bit of u (u is within a fraction of a pixel of x)"""
    pyramid, _ = scene_pair(name)
    for level, (K, ref, cur) in enumerate(pyramid):
        for I, Z in (ref, cur):
            r = covisibility_host(I, Z, I, Z, K, K, np.eye(4))
            usable = int((np.isfinite(Z) & (Z > 0)).sum())
            assert r["valid"] == r["in_view"] == r["consistent"] == usable > 0.3 * Z.size, (name, level, as_dict(r))
            assert r["photo"] == 0 and r["unknown"] == r["occluded"] == r["seen_through"] == 0


# ---- 3. hand-made 8 x 8 planes: each class alone, then a mix ------------------------------------------------------------------------------

def record(Ia, Za, Ib, Zb, T=np.eye(4), Ka=K8, Kb=K8, **kw):
    return as_dict(covisibility_host(Ia, Za, Ib, Zb, Ka, Kb, T, **kw))


def only(**counts):
    """a record with these counts and zeros elsewhere"""
    return dict({k: 0 for k in FIELDS}, **counts)


def test_each_class_alone():
    I, Z = np.arange(64, dtype=f32).reshape(8, 8), flat(2.0)
    assert record(I, Z, I, Z) == only(valid=64, in_view=64, consistent=64)
    for T in (shift(9.0, 0.0), shift(-4.0, -9.0), shift(0.0, 8.0)):                     # a shift off the image
        assert record(I, Z, I, Z, T) == only(valid=64)
    assert record(I, Z, I, Z, np.diag([-1.0, 1.0, -1.0, 1.0])) == only(valid=64)        # a 180-degree turn about y: p.z = -z
    assert record(I, Z, I, flat(1.5)) == only(valid=64, in_view=64, occluded=64)        # a nearer plane in b
    assert record(I, Z, I, flat(2.5)) == only(valid=64, in_view=64, seen_through=64)    # a farther plane in b
    hole = flat(2.0)
    hole[2, 3] = np.nan
    hole[5, 5] = np.inf
    assert record(I, Z, I, hole) == only(valid=64, in_view=64, unknown=2, consistent=62)
    assert record(I, hole, I, Z) == only(valid=62, in_view=62, consistent=62)           # a hole in a is not valid
    # one column leaves to the left: the nearest pixel of u = -1 is outside, of u = 0 .. 6 inside
    assert record(I, Z, I, Z, shift(-1.0, 0.0)) == only(valid=64, in_view=56, consistent=56, photo=56 * 16)
    # half a pixel: integer coordinates are centres, u = x - 0.5 rounds to x (floor(x - 0.5 + 0.5)): nothing leaves
    assert record(I, Z, I, Z, shift(-0.5, 0.0))["in_view"] == 64 and record(I, Z, I, Z, shift(-0.75, 0.0))["in_view"] == 56
    assert record(I, Z, I, Z, shift(0.25, 0.0))["in_view"] == 64 and record(I, Z, I, Z, shift(0.5, 0.0))["in_view"] == 56


def test_tolerances_photo_and_depth_range():
    I = np.arange(64, dtype=f32).reshape(8, 8)
    # a near half (1 m) and a far half (4 m) of a; b lies 8 cm behind both
    Za = flat(1.0)
    Za[:, 4:] = 4.0
    Zb = (Za + f32(0.08)).astype(f32)
    assert record(I, Za, I, Zb) == only(valid=64, in_view=64, seen_through=64)
    # 2 % of the depth on top of 5 cm: 7 cm at 1 m (still seen through), 13 cm at 4 m (consistent)
    assert record(I, Za, I, Zb, depth_tolerance_rel=0.02) == only(valid=64, in_view=64, seen_through=32, consistent=32)
    assert record(I, Za, I, Zb, depth_tolerance=0.1) == only(valid=64, in_view=64, consistent=64)
    # the depth range skips pixels of a
    assert record(I, Za, I, Za, min_depth=2.0, max_depth=5.0) == only(valid=32, in_view=32, consistent=32)
    assert record(I, Za, I, Za, min_depth=0.0, max_depth=1.0) == only(valid=32, in_view=32, consistent=32)
    assert record(I, Za, I, Za, min_depth=1.5, max_depth=3.0) == only()
    # photo: sixteenths, rounded half up; NaN and anything from 4096 on give 65535
    Z = flat(2.0)
    assert record(I, Z, I + f32(0.25), Z)["photo"] == 64 * 4
    assert record(I, Z, I + f32(1.0 / 32), Z)["photo"] == 64 and record(I, Z, I + f32(1.0 / 64), Z)["photo"] == 0
    nan_I = I.copy()
    nan_I[1, 1] = np.nan
    assert record(I, Z, nan_I, Z) == only(valid=64, in_view=64, consistent=64, photo=65535)
    assert record(nan_I, Z, I, Z)["photo"] == 65535 and record(nan_I, Z, nan_I, Z)["photo"] == 65535
    L = host_lib()
    assert [L.covis_host_photo(0.0, x) for x in (4095.0, 4095.97, 4096.0, 1e30, INF)] == [65520, 65536, 65535, 65535, 65535]


def test_b_of_another_size_and_camera():
    """a is 8 x 8 under K8; b is 4 x 6 (w x h) under a camera of half the focal length: a's pixel (x, y) lands at ((x - 3.5) / 2 + 1.5,
    (y - 3.5) / 2 + 2.5), whose nearest pixels cover b's columns 0 .. 3 (from x = 0 .. 7: -0.25 .. 3.25) and rows 1 .. 4"""
    I, Z = np.arange(64, dtype=f32).reshape(8, 8), flat(2.0)
    Kb = np.array([32.0, 32.0, 1.5, 2.5], f32)
    Ib, Zb = np.zeros((6, 4), f32), np.full((6, 4), np.nan, f32)
    Zb[1:5, :] = 2.0
    assert record(I, Z, Ib, Zb, Kb=Kb) == only(valid=64, in_view=64, consistent=64, photo=int(I.sum()) * 16)
    Zb[1, :] = np.nan                                                                   # b's row 1 takes a's rows 0 and 1 (v = 0.75, 1.25)
    assert record(I, Z, Ib, Zb, Kb=Kb) == only(valid=64, in_view=64, unknown=16, consistent=48, photo=int(I[2:].sum()) * 16)
    # the other way round: b's pixel (x, y) lands at (2 x + 0.5, 2 y - 1.5) of a, nearest pixel (2 x + 1, 2 y - 1): rows 0 and 5 leave
    assert record(Ib, np.full((6, 4), 2.0, f32), I, Z, Ka=Kb, Kb=K8) == only(valid=24, in_view=16, consistent=16, photo=int(I[1::2, 1::2].sum()) * 16)


def test_a_mix_holds_the_invariant():
    """a flat at 2 m with four pixels without depth, moved one pixel right and two up; b's columns lie 30 cm nearer (column 4), 30 cm
    further (columns 3 and 7) or at 2 m, and three pixels of its row 3 are holes.  6 rows x 7 columns stay in view; of b's columns
    1 .. 7 there, column 4 occludes (6 - 1 hole), 3 and 7 are seen through (5 + 6), the other four agree (6 + 5 + 6 + 6)"""
    rng = np.random.default_rng(11)
    I, Ib = rng.uniform(0, 255, (8, 8)).astype(f32), rng.uniform(0, 255, (8, 8)).astype(f32)
    Za = flat(2.0)
    Za[0, :3] = np.nan
    Za[7, 7] = -1.0
    Zb = (flat(2.0) + np.array([-0.3, 0.0, 0.0, 0.3] * 2, f32)[None, :]).astype(f32)
    Zb[3, 2:5] = np.nan
    T = shift(1.0, -2.0)
    got = covisibility_host(I, Za, Ib, Zb, K8, K8, T)
    assert as_dict(got) == np_covisibility(I, Za, Ib, Zb, K8, K8, T) and holds_invariant(got)
    assert as_dict(got) == only(valid=60, in_view=42, unknown=3, occluded=5, seen_through=11, consistent=23, photo=int(got["photo"]))
    assert got["photo"] > 0


# ---- 4. overlap falls as the views turn apart ---------------------------------------------------------------------------------------------

def yaw(degrees):
    a = np.deg2rad(degrees)
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return T


def test_overlap_falls_as_the_yaw_grows():
    """one view against itself turned about the camera's y axis by 0, 10, 20 and 40 degrees (fr1 at 128 x 96: 62 degrees across)"""
    K, (I, Z), _ = scene_pair("fr1")[0][0]
    shares = []
    for degrees in (0.0, 10.0, 20.0, 40.0):
        ab = np.array([covisibility_host(I, Z, I, Z, K, K, yaw(degrees))])
        ba = np.array([covisibility_host(I, Z, I, Z, K, K, yaw(-degrees))])
        shares.append(float(d.overlap(ab, ba)[0]))
    assert shares[0] == 1.0 and all(x > y for x, y in zip(shares, shares[1:])) and shares[-1] < 0.5, shares


# ---- 6. the Python logic over the host build ---------------------------------------------------------------------------------------------

class HostPyramid:
    """a pyramid as covisibility_batch sees one, with the planes on the host"""
    def __init__(self, ctx, planes):
        self.ctx, self.planes, self.levels, self.ptr = ctx, planes, len(planes), None      # planes[level] = (K, I, Z)


def host_batch(pyramids, pairs, transforms, level=2, **kw):
    """covisibility_batch with the host build in the device call's place: the same checks first, then covisibility_host per pair"""
    P, T = d.tracker._covis_args(pyramids, pairs, transforms, level, "host_batch")
    out = np.zeros(P.shape[0], d.COVIS_DTYPE)
    for k, (a, b) in enumerate(P):
        (Ka, Ia, Za), (Kb, Ib, Zb) = pyramids[a].planes[level], pyramids[b].planes[level]
        out[k] = covisibility_host(Ia, Za, Ib, Zb, Ka, Kb, T[k], **kw)
    return out


@functools.lru_cache(maxsize=None)
def keyframes():
    """five keyframes and their poses (camera -> world): 0 and 1 are the two views of the fr1 pair under their true relative pose, 2 holds
    keyframe 0's planes five metres aside, 3 stands where 0 stands and has no depth at all, 4 holds keyframe 0's planes turned by
    35 degrees about the camera's y axis"""
    pyramid, T = scene_pair("fr1")
    ctx = object()
    ref = HostPyramid(ctx, [(K, r[0], r[1]) for K, r, c in pyramid])
    cur = HostPyramid(ctx, [(K, c[0], c[1]) for K, r, c in pyramid])
    empty = HostPyramid(ctx, [(K, r[0], np.full_like(r[1], np.nan)) for K, r, c in pyramid])
    # poses camera -> world with the reference camera as the world: T is reference -> current, so the current camera's pose is inv(T)
    far = np.eye(4)
    far[0, 3] = 5.0
    poses = np.stack([np.eye(4), np.linalg.inv(T), far, np.eye(4), yaw(35.0)])
    return [ref, cur, ref, empty, ref], poses


def test_matrix_and_overlap_over_the_host_build():
    pyramids, poses = keyframes()
    M = d.covisibility_matrix(pyramids, poses, level=1, batch=host_batch)
    assert M.shape == (5, 5) and M.dtype == d.COVIS_DTYPE
    (K, Ia, Za), (_, Ib, Zb) = pyramids[0].planes[1], pyramids[1].planes[1]
    assert M[0, 1] == covisibility_host(Ia, Za, Ib, Zb, K, K, np.linalg.inv(poses[1]) @ poses[0])
    assert M[1, 0] == covisibility_host(Ib, Zb, Ia, Za, K, K, np.linalg.inv(poses[0]) @ poses[1])
    assert all(M[k, k]["valid"] == M[k, k]["consistent"] for k in range(5)) and M[3, 3]["valid"] == 0
    S = d.overlap(M, M.T)
    assert S.dtype == np.float64 and np.array_equal(S, S.T)
    assert S[0, 0] == 1.0 and S[3, 3] == 0.0 and np.all(S[3] == 0.0)                       # valid == 0: no overlap, no division
    assert S[0, 1] == min(M[0, 1]["consistent"] / M[0, 1]["valid"], M[1, 0]["consistent"] / M[1, 0]["valid"]) > 0.3
    assert S[0, 2] == 0.0 and 0.0 < S[0, 4] < S[0, 1]                                       # five metres aside; turned away
    with pytest.raises(TypeError):
        d.overlap(np.zeros(3), M[0, :3])
    with pytest.raises(ValueError):
        d.overlap(M[0], M[:, :2])


def test_loop_closure_candidates_over_the_host_build():
    pyramids, poses = keyframes()
    calls = []

    def counted(*a, **kw):
        calls.append(len(a[1]))
        return host_batch(*a, **kw)

    S = d.overlap(*(lambda M: (M, M.T))(d.covisibility_matrix(pyramids, poses, level=1, batch=host_batch)))
    # the radius set: 0, 1, 3 and 4 stand within a metre of keyframe 0 (itself included, as in the reference), 2 does not
    assert d.radius_set(poses, 0, 1.0).tolist() == [0, 1, 3, 4] and d.radius_set(poses, 2, 1.0).tolist() == [2]
    assert d.radius_set(poses, 0, 5.0).tolist() == [0, 1, 2, 3, 4] and d.radius_set(poses, 0, 4.99).tolist() == [0, 1, 3, 4]   # <=
    got = d.loop_closure_candidates(pyramids, poses, 0, 1.0, level=1, batch=counted)
    assert calls == [8]                                                                     # both directions of four survivors: one call
    # ordered by overlap, descending; 3 (no valid pixel: overlap 0) still passes min_overlap = 0
    assert got.tolist() == [0, 1, 4, 3] and list(S[0, got]) == sorted(S[0, got], reverse=True)
    assert d.loop_closure_candidates(pyramids, poses, 0, 1.0, min_overlap=1e-9, level=1, batch=host_batch).tolist() == [0, 1, 4]
    assert d.loop_closure_candidates(pyramids, poses, 0, 1.0, min_overlap=float(S[0, 1]), level=1, batch=host_batch).tolist() == [0, 1]
    assert d.loop_closure_candidates(pyramids, poses, 0, 1.0, min_overlap=1.0, level=1, batch=host_batch).tolist() == [0]
    # ties go by index: keyframes 0 and 2 hold the same planes, so from 1 they overlap alike once they stand at the same place
    same = poses.copy()
    same[2] = same[0]
    tie = d.loop_closure_candidates(pyramids, same, 1, 1.0, level=1, batch=host_batch)
    assert tie.tolist() == [1, 0, 2, 4, 3]
    # the query from further away: the set is the query alone; a query that is no keyframe's neighbour at radius 0 still finds itself
    assert d.loop_closure_candidates(pyramids, poses, 2, 1.0, level=1, batch=host_batch).tolist() == [2]
    assert d.loop_closure_candidates(pyramids, poses, 3, 0.0, level=1, batch=host_batch).tolist() == [0, 3, 4]   # they share a place; all overlap 0: by index


# ---- 7. the wrappers' argument checks ----------------------------------------------------------------------------------------------------

def test_python_wrappers_reject_bad_arguments_before_the_library():
    """every pyramid here has no library behind it (ctx is a bare object): a call that got past the checks would fail with an
    AttributeError, not with the ValueError / TypeError asserted"""
    ctx, cam = object(), FakeCamera()
    two = [FakePyramid(ctx, cam), FakePyramid(ctx, cam)]
    eye2 = np.stack([np.eye(4), np.eye(4)])
    pairs = [(0, 1), (1, 0)]
    p = d.covis_params_struct()
    assert (p.depth_tolerance_rel, p.min_depth, p.max_depth, list(p.reserved)) == (0.0, 0.0, INF, [0, 0, 0, 0]) and p.depth_tolerance == f32(0.05)
    assert C.sizeof(d._lib.CovisParams) == 32 and d.COVIS_DTYPE.itemsize == 32 and d.COVIS_DTYPE.names == FIELDS
    assert d.COVIS_DTYPE.fields["photo"][1] == 24
    nan_T, inf_T = eye2.copy(), eye2.copy()
    nan_T[1, 0, 3], inf_T[0, 2, 2] = np.nan, np.inf
    for bad in [([], pairs, eye2), (two, [], np.zeros((0, 4, 4))), (two, [(0, 2), (1, 0)], eye2), (two, [(0, 1), (-1, 0)], eye2),
                (two, [(0, 1, 1), (1, 0, 0)], eye2), (two, [[(0, 1)], [(1, 0)]], eye2), (two, pairs, np.eye(4)), (two, pairs, np.stack([np.eye(4)] * 3)),
                (two, pairs, np.zeros((2, 16))), (two, pairs, nan_T), (two, pairs, inf_T), ([two[0], FakePyramid(object(), cam)], pairs, eye2)]:
        with pytest.raises(ValueError):
            d.covisibility_batch(*bad)
    for bad in ([(0.0, 1.0), (1.0, 0.0)], [("a", "b")] * 2, [(True, False)] * 2):
        with pytest.raises(TypeError):
            d.covisibility_batch(two, bad, eye2)
    with pytest.raises(ValueError):
        d.covisibility_batch(two, np.zeros(((1 << 22) + 1, 2), np.int32), eye2)
    for level in (-1, 3, 7):
        with pytest.raises(ValueError):
            d.covisibility_batch(two, pairs, eye2, level=level)
    with pytest.raises(ValueError):
        d.covisibility_batch([two[0], FakePyramid(ctx, cam, levels=1)], pairs, eye2, level=1)
    for level in (1.0, True, "0"):
        with pytest.raises(TypeError):
            d.covisibility_batch(two, pairs, eye2, level=level)
    for bad in (dict(depth_tolerance=-0.01), dict(depth_tolerance=float("nan")), dict(depth_tolerance_rel=-1.0), dict(depth_tolerance_rel=float("nan")),
                dict(min_depth=2.0, max_depth=1.0), dict(min_depth=float("nan")), dict(max_depth=float("nan"))):
        with pytest.raises(ValueError):
            d.covisibility_batch(two, pairs, eye2, **bad)
        with pytest.raises(ValueError):
            d.covisibility_matrix(two, eye2, **bad)
        with pytest.raises(ValueError):
            d.loop_closure_candidates(two, eye2, 0, 1.0, **bad)
    with pytest.raises(TypeError):
        d.covisibility_batch(two, pairs, eye2, depth_tolerance="wide")
    singular = eye2.copy()
    singular[1, :3, :3] = 0.0
    for poses in (np.eye(4), np.zeros((2, 3, 4)), nan_T, singular):
        with pytest.raises(ValueError):
            d.covisibility_matrix(two, poses)
        with pytest.raises(ValueError):
            d.loop_closure_candidates(two, poses, 0, 1.0)
    for query in (-1, 2):
        with pytest.raises(ValueError):
            d.loop_closure_candidates(two, eye2, query, 1.0)
    for query in (0.0, True, None):
        with pytest.raises(TypeError):
            d.loop_closure_candidates(two, eye2, query, 1.0)
    for kw in (dict(max_distance=-1.0), dict(max_distance=float("nan")), dict(max_distance=1.0, min_overlap=-0.1),
               dict(max_distance=1.0, min_overlap=1.5), dict(max_distance=1.0, min_overlap=float("nan"))):
        with pytest.raises(ValueError):
            d.loop_closure_candidates(two, eye2, 0, **kw)
    with pytest.raises(TypeError):
        d.loop_closure_candidates(two, eye2, 0, "near")


# ---- 8. the C++ facade -------------------------------------------------------------------------------------------------------------------

def build_covisibility_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "covisibility_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "covisibility_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_covisibility_compiles():
    d.build()
    assert os.path.exists(build_covisibility_facade_check())
