"""GPU tier: views of the keyframe map on the device (include/dvo_hip.h, dvo_hip_map_render and dvo_hip_map_render_frames; k_render_fill,
k_map_render, k_render_resolve).  The yardstick is render_host() of tests/test_map_render.py -- the host build of
dvo_slam_amd/csrc/map_render.h -- fed the device map's own extraction: the device planes equal it BIT FOR BIT, since every z-buffer
update is an integer atomic minimum and nothing depends on the order the device visits the voxels in.
  1. bit-for-bit equality at three shapes, at a keyframe's pose and off it, host and device output, two views in one call;
  2. contention: hundreds of voxels per pixel, the largest footprint; the same render twice;
  3. table shapes: 2^10 slots a third full, 64 slots;
  4. parameters: a depth range, min_points, a view that sees nothing;
  5. render_into: the frame's planes, its pyramid, a role-aware call;
  6. tracking a frame against the model, against the oracle;
  7. refusals, the counter, clear and re-insert, frames with a lens or a depth rig;
  8. the C++ facade's PointCloudAggregator::render against KeyframeMap.render."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import common as cm
import dvo_slam_amd as d
import scenes
import test_cloud_map as tcm
import test_depth_rig as tdr
import test_map_render as tmr
from dvo_slam_amd import _lib
from oracle import pyoracle as po
from test_gpu_cloud_map import SHAPES, facade_frame, frames_of, planes_of, roomy, yardstick
from test_gpu_f32_ingest import blank_frames, camera
from test_gpu_lens_ingest import lens_of
from test_map_render import holes, render_host, same_bits

pytestmark = pytest.mark.gpu
INF = float("inf")
LEAF = 0.02
TWIST_TOL = 1e-6     # tests/test_gpu_parity.py line 720: the final transform of a full match against the oracle at Precision 5e-7


def device_map(w, h, n, leaf=LEAF):
    """(ctx, pyramids, poses, K of level 0, the map of the n frames in a roomy table)"""
    ctx, pyramids, poses = frames_of(w, h, n)
    want, capacity = roomy(pyramids, poses, 0, leaf)
    m = d.KeyframeMap(ctx, leaf, capacity)
    m.insert(pyramids, poses)
    assert m.stats()["dropped"] == 0
    return ctx, pyramids, poses, planes_of(pyramids[0], 0)[2], m


def want_of(m, K, w, h, poses, **params):
    """the yardstick's planes of the device map's own extraction"""
    xyzi, counts, keys = m.extract(sort=True)
    return render_host(xyzi, counts, m.leaf, K, w, h, poses, **params)


def off(T, k=1):
    return T @ scenes.se3_exp([0.04 * k, -0.03, 0.02 * k, 0.03, -0.04 * k, 0.02])


# ---- 1. bit for bit -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,n", list(zip(SHAPES, (2, 3, 4))))
def test_render_equals_the_yardstick(shape, n):
    w, h = shape
    ctx, pyramids, poses, K, m = device_map(w, h, n)
    views = np.stack([poses[0], off(poses[1])])
    want = want_of(m, K, w, h, views)
    for k in range(2):
        assert holes(want[1][k]).any() and (~holes(want[1][k])).sum() > 0.3 * w * h, k      # holes and filled pixels are both present
    got = m.render(K, w, h, views)
    assert got[0].shape == (2, h, w) and same_bits(got, want), (w, h, "host")
    dev = m.render(K, w, h, views, device=True)
    torch.cuda.synchronize()
    assert same_bits([t.cpu().numpy() for t in dev], want), (w, h, "device")
    for k in range(2):                                              # two views in one call are the two single calls
        one = m.render(K, w, h, views[k])
        assert same_bits((one[0][0], one[1][0]), (want[0][k], want[1][k])), (w, h, k)
    # another camera than the keyframes': half the size, a principal point off the centre
    K2 = np.array([K[0] * 0.5, K[1] * 0.55, K[2] * 0.4, K[3] * 0.6], np.float32)
    assert same_bits(m.render(K2, w // 2 + 1, h // 2, views[1]), want_of(m, K2, w // 2 + 1, h // 2, views[1]))
    m.close()


def test_device_planes_of_views_whose_pixel_count_is_no_multiple_of_four():
    """101 x 77 = 7777 pixels: the device planes of two views cannot lie back to back and both be 16-byte aligned, so
    KeyframeMap.render pads each plane and returns strided tensors"""
    ctx, pyramids, poses, K, m = device_map(128, 96, 2)
    w, h = 101, 77
    K2 = (K * np.float32(w / 128.0)).astype(np.float32)
    views = np.stack([poses[0], off(poses[1]), off(poses[0], 2)])
    want = want_of(m, K2, w, h, views)
    assert holes(want[1]).any() and (~holes(want[1])).sum() > 0.3 * want[1].size
    dev = m.render(K2, w, h, views, device=True)
    torch.cuda.synchronize()
    assert all(t.shape == (3, h, w) and t[k].data_ptr() % 16 == 0 for t in dev for k in range(3))
    assert same_bits([t.cpu().numpy() for t in dev], want) and same_bits(m.render(K2, w, h, views), want)
    m.close()


# ---- 2. contention --------------------------------------------------------------------------------------------------------------------

def test_contention_and_the_largest_footprint():
    w, h = 321, 240
    ctx, pyramids, poses, K, m = device_map(w, h, 3)
    small = (K * np.float32(16.0 / w)).astype(np.float32)          # the same field of view on 16 x 12 pixels
    views = np.stack([poses[0], off(poses[0])])
    xyzi, counts, keys = m.extract(sort=True)
    want = render_host(xyzi, counts, m.leaf, small, 16, 12, views, want_updates=True)
    assert want[2] > 100 * 16 * 12 * 2                              # hundreds of voxels meet on every pixel
    first = m.render(small, 16, 12, views)
    assert same_bits(first, want[:2]) and same_bits(m.render(small, 16, 12, views), first)
    big = dict(max_splat=15, splat=4.0)
    want_big = render_host(xyzi, counts, m.leaf, small, 16, 12, views, want_updates=True, **big)
    assert want_big[2] > want[2]
    assert same_bits(m.render(small, 16, 12, views, **big), want_big[:2])
    # ... and at full size, where the footprints are 15 pixels wide close to the camera
    full = m.render(K, w, h, views, **big)
    assert same_bits(full, want_of(m, K, w, h, views, **big)) and same_bits(m.render(K, w, h, views, **big), full)
    m.close()


# ---- 3. table shapes ------------------------------------------------------------------------------------------------------------------

def test_small_tables():
    ctx, pyramids, poses = frames_of(128, 96, 2)
    K = planes_of(pyramids[0], 0)[2]
    want = yardstick(pyramids, poses, 0, 0.25, 1 << 10, 0.0, 5.0)
    assert 300 <= want.stats()["occupied"] <= 450 and 1 < want.longest_run() < tcm.MAX_PROBES
    m = d.KeyframeMap(ctx, 0.25, 1 << 10)
    m.insert(pyramids, poses, max_depth=5.0)
    views = np.stack([poses[0], off(poses[1])])
    got = m.render(K, 128, 96, views)
    assert same_bits(got, want_of(m, K, 128, 96, views)) and same_bits(got, tmr.render_host_map(want, K, 128, 96, views))
    assert (~holes(got[1])).sum() > 1000
    # 64 slots: a leaf so large that the scene fits
    coarse = yardstick(pyramids, poses, 0, 4.0, 64)
    assert coarse.stats()["dropped"] == 0 and 4 <= coarse.stats()["occupied"] < 64
    c = d.KeyframeMap(ctx, 4.0, 64)
    c.insert(pyramids, poses)
    got = c.render(K, 128, 96, views, splat=0.05)
    assert same_bits(got, tmr.render_host_map(coarse, K, 128, 96, views, splat=0.05)) and (~holes(got[1])).any()
    for x in (m, c):
        x.close()


# ---- 4. parameters --------------------------------------------------------------------------------------------------------------------

def test_depth_range_min_points_and_a_view_that_sees_nothing():
    w, h = 128, 96
    ctx, pyramids, poses, K, m = device_map(w, h, 2)
    plain = m.render(K, w, h, poses[0])
    lo, hi = (float(x) for x in np.nanpercentile(plain[1], [30, 70]))
    ranged = m.render(K, w, h, poses[0], min_depth=lo, max_depth=hi)
    assert same_bits(ranged, want_of(m, K, w, h, poses[0], min_depth=lo, max_depth=hi))
    seen = ranged[1][~holes(ranged[1])]
    assert 0 < seen.size < (~holes(plain[1])).sum() and seen.min() >= lo and seen.max() <= hi
    dense = m.render(K, w, h, poses[0], min_points=2)
    assert same_bits(dense, want_of(m, K, w, h, poses[0], min_points=2)) and not same_bits(dense, plain)
    away = poses[0] @ np.diag([-1.0, 1.0, -1.0, 1.0])               # turned by 180 degrees about y: the scene lies behind the camera
    for device in (False, True):
        I, Z = m.render(K, w, h, away, device=device)
        if device:
            torch.cuda.synchronize()
            I, Z = I.cpu().numpy(), Z.cpu().numpy()
        assert np.all(Z.view(np.uint32) == 0x7FC00000) and np.all(I.view(np.uint32) == 0)
    assert holes(want_of(m, K, w, h, away)[1]).all()
    m.close()


# ---- 5. render_into -------------------------------------------------------------------------------------------------------------------

def all_planes(p, levels):
    return [planes_of(p, l)[:2] for l in range(levels)]


def test_render_into_gives_the_frame_the_rendered_planes_make():
    w, h, levels = 128, 96, 3
    ctx, pyramids, poses, K, m = device_map(w, h, 2)
    cam = pyramids[0].camera
    views = np.stack([poses[0], off(poses[1])])
    I, Z = m.render(K, w, h, views)
    targets = blank_frames(cam, 2)
    m.render_into(targets, views)
    for k in range(2):
        made = cam.create(I[k], Z[k])                               # a frame created from the same float planes
        got, want = all_planes(targets[k], levels), all_planes(made, levels)
        assert same_bits(got[0], (I[k], Z[k])), k
        for l in range(levels):
            assert np.array_equal(got[l][0].view(np.uint32), want[l][0].view(np.uint32)) and np.array_equal(got[l][1].view(np.uint32), want[l][1].view(np.uint32)), (k, l)
    # a role-aware call followed by a match = a plain update followed by a match
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    tracker = d.DenseTracker(cfg, ctx)
    results = []
    for role in (None, "reference"):
        ref = blank_frames(cam, 1)
        m.render_into(ref, views[:1], role=role, config=cfg if role else None)
        r = d.Result()
        assert tracker.match(ref[0], pyramids[1], r) is True
        results.append(np.array(r.Transformation, copy=True))
    assert not np.isnan(results[0]).any() and np.array_equal(results[0], results[1])
    # rendering again into the same frames follows the new poses
    m.render_into(targets, views[::-1])
    assert same_bits(all_planes(targets[0], 1)[0], (I[1], Z[1])) and same_bits(all_planes(targets[1], 1)[0], (I[0], Z[0]))
    m.close()


# ---- 6. tracking against the model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [dict()] + tmr.TRACKING_PARAMS, ids=["defaults", "max_splat_1", "splat_1_min_depth"])
def test_tracking_a_frame_against_the_model(params):
    """View 1 aligned against the map of views 0 and 1 rendered at view 0's pose: the GPU's transformation against the oracle's MATH mode
    on the same float planes, within the twist tolerance of a full match (TWIST_TOL) -- with the default parameters and with those named
    for tracking.  For the latter the GPU's result is also held against the TRUE relative pose, by the bounds
    tests/test_map_render.py::test_tracking_against_the_model_on_the_cpu derives; with the defaults the distance to the truth is
    printed only (0.054 on the CPU: the grown silhouettes mislead the alignment, profiles/map_render.md)."""
    w, h, levels = 128, 96, 3
    ctx, pyramids, poses, K, m = device_map(w, h, 2)
    model = blank_frames(pyramids[0].camera, 1)
    m.render_into(model, poses[:1], **params)
    cfg = d.Config()
    cfg.FirstLevel = min(cfg.FirstLevel, levels - 1)                # the default config, cut to the levels this size has
    cfg.LastLevel = min(cfg.LastLevel, cfg.FirstLevel)
    r = d.Result()
    assert d.DenseTracker(cfg, ctx).match(model[0], pyramids[1], r) is True
    T_gpu = np.array(r.Transformation, copy=True)
    I, Z = m.render(K, w, h, poses[0], **params)
    I1, Z1, _ = planes_of(pyramids[1], 0)
    oref, ocur = po.Pyramid(I[0], Z[0], K, levels), po.Pyramid(I1, Z1, K, levels)
    o = po.match(oref, ocur, cm.oracle_config_from(cfg, po.MATH))
    assert not np.isnan(T_gpu).any() and not np.isnan(o["T"]).any()
    err = cm.twist_matrix_error(T_gpu, o["T"])
    true = np.linalg.inv(poses[0]) @ poses[1]
    to_truth, motion = cm.twist_matrix_error(T_gpu, true), float(np.abs(po.se3_log(true)).max())
    print("%s: GPU against the oracle %.3g; GPU / oracle against the true relative pose %.3g / %.3g; the motion %.3g"
          % (params, err, to_truth, cm.twist_matrix_error(o["T"], true), motion))
    assert err < TWIST_TOL, err
    if params:
        K_, views = tcm.float_views(w, h)
        baseline, _ = tmr.oracle_tracking_error(views[0][0], views[0][1], K_, views)
        assert to_truth < motion and to_truth <= 2.0 * baseline, (to_truth, motion, baseline)
    m.close()


# ---- 7. refusals, counter, lifetime ---------------------------------------------------------------------------------------------------

def test_refusals_change_nothing_and_the_counter_counts_views():
    w, h = 128, 96
    ctx, pyramids, poses, K, m = device_map(w, h, 2)
    L = ctx._lib
    c0 = ctx.counter("map_renders")
    m.render(K, w, h, np.stack([poses[0], poses[1], poses[0]]))
    assert ctx.counter("map_renders") - c0 == 3
    targets = blank_frames(pyramids[0].camera, 2)
    m.render_into(targets, poses)
    assert ctx.counter("map_renders") - c0 == 5
    before = [planes_of(t, 0)[:2] for t in targets]
    c1 = ctx.counter("map_renders")
    other = d.Context(0)
    foreign_map = d.KeyframeMap(other, LEAF, 1 << 10)
    foreign = camera(other, w, h, K, 3).create(*tcm.float_views(w, h)[1][0][:2])
    Kc = np.ascontiguousarray(K, np.float32)
    kp = Kc.ctypes.data_as(C.POINTER(C.c_float))
    T = np.ascontiguousarray(poses, np.float64)
    tp = T.ctypes.data_as(C.POINTER(C.c_double))
    out = [np.full((h, w), -7.0, np.float32) for _ in range(4)]
    oi, oz = (C.c_void_p * 2)(out[0].ctypes.data, out[1].ctypes.data), (C.c_void_p * 2)(out[2].ctypes.data, out[3].ctypes.data)
    nulled = (C.c_void_p * 2)(out[0].ctypes.data, None)
    handles = (C.c_void_p * 2)(targets[0].ptr, targets[1].ptr)
    mixed = (C.c_void_p * 2)(targets[0].ptr, foreign.ptr)
    nullf = (C.c_void_p * 2)(targets[0].ptr, None)
    good = d.render_params_struct()

    def params(**kw):
        p = d.render_params_struct()
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return C.byref(p)

    def K_of(*v):
        a = np.array(v, np.float32)
        return a.ctypes.data_as(C.POINTER(C.c_float)), a

    def render(map_=m.ptr, ctx_=ctx.ptr, n=2, w_=w, h_=h, k=kp, t=tp, p=C.byref(good), i=oi, z=oz, dev=0):
        return L.dvo_hip_map_render(ctx_, map_, n, w_, h_, k, t, p, i, z, dev)

    def frames(map_=m.ptr, ctx_=ctx.ptr, n=2, f=handles, t=tp, p=C.byref(good), role=-1, cfg=None, flags=0):
        return L.dvo_hip_map_render_frames(ctx_, map_, n, f, t, p, role, cfg, flags)

    bad_params = [dict(splat=0.0), dict(splat=4.5), dict(splat=float("nan")), dict(splat=-1.0), dict(max_splat=0), dict(max_splat=8), dict(max_splat=17),
                  dict(max_splat=-3), dict(min_points=0), dict(min_depth=2.0, max_depth=1.0), dict(min_depth=float("nan")), dict(max_depth=float("nan")),
                  dict(reserved=0), dict(reserved=2)]
    bad_K = [K_of(0.0, 100.0, 64.0, 48.0), K_of(100.0, -1.0, 64.0, 48.0), K_of(np.nan, 100.0, 64.0, 48.0), K_of(100.0, 100.0, INF, 48.0)]
    ccfg = d.Config(FirstLevel=2, LastLevel=0).to_c()
    calls = [lambda: render(map_=None), lambda: render(map_=foreign_map.ptr), lambda: render(ctx_=other.ptr), lambda: render(n=0), lambda: render(n=-1),
             lambda: render(w_=0), lambda: render(h_=-5), lambda: render(w_=(1 << 24) + 1, h_=1), lambda: render(k=None), lambda: render(t=None),
             lambda: render(i=None), lambda: render(z=None), lambda: render(i=nulled), lambda: render(z=nulled),
             lambda: render(i=(C.c_void_p * 2)(8, 16), z=(C.c_void_p * 2)(16, 32), dev=1),       # a device plane that is not 16-byte aligned
             lambda: frames(map_=None), lambda: frames(map_=foreign_map.ptr), lambda: frames(n=0), lambda: frames(f=None), lambda: frames(t=None),
             lambda: frames(f=mixed), lambda: frames(f=nullf), lambda: frames(flags=_lib.INGEST_DEFER),
             lambda: frames(role=7, cfg=C.byref(ccfg)), lambda: frames(role=_lib.ROLE_REFERENCE, cfg=None)]
    calls += [lambda b=b: render(p=params(**b)) for b in bad_params] + [lambda b=b: frames(p=params(**b)) for b in bad_params]
    calls += [lambda b=b: render(k=b[0]) for b in bad_K]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
    assert all(np.all(o == -7.0) for o in out) and ctx.counter("map_renders") == c1
    assert render() == 0 and not any(np.any(o == -7.0) for o in out)     # the same call with nothing wrong
    assert ctx.counter("map_renders") == c1 + 2
    assert all(same_bits(planes_of(t, 0)[:2], b) for t, b in zip(targets, before))
    # a frame with a lens or a depth rig is refused, by the library and by the wrapper
    lensed, rigged = blank_frames(pyramids[0].camera, 1), blank_frames(pyramids[0].camera, 1)
    d.set_lens_batch(lensed, *lens_of(K, "plumb_bob"))
    d.set_depth_rig_batch(rigged, *tdr.kinect_rig(K))
    for f in (lensed, rigged):
        assert frames(n=1, f=(C.c_void_p * 1)(f[0].ptr)) == _lib.ERR_INVALID
        with pytest.raises(ValueError):
            m.render_into(f, poses[:1])
    d.clear_lens_batch(lensed)
    m.render_into(lensed, poses[:1])                                # without the lens the frame takes the view
    assert same_bits(planes_of(lensed[0], 0)[:2], before[0])
    with pytest.raises(ValueError):
        m.render_into([foreign], poses[:1])
    assert ctx.counter("map_renders") == c1 + 3
    for x in (m, foreign_map):
        x.close()
    del foreign
    other.close()


def test_render_follows_clear_and_reinsert():
    w, h = 128, 96
    ctx, pyramids, poses, K, m = device_map(w, h, 2)
    first = m.render(K, w, h, poses[0])
    assert (~holes(first[1])).any()
    m.clear()
    cleared = m.render(K, w, h, poses[0])
    assert np.all(cleared[1].view(np.uint32) == 0x7FC00000) and np.all(cleared[0] == 0.0)
    moved = np.stack([off(T, 2) for T in poses])                    # after a pose-graph optimisation: the same frames under new poses
    m.insert(pyramids, moved)
    second = m.render(K, w, h, poses[0])
    assert same_bits(second, want_of(m, K, w, h, poses[0])) and not same_bits(second, first)
    assert same_bits(m.render(K, w, h, moved[0]), want_of(m, K, w, h, moved[0]))
    m.close()


# ---- 8. the C++ facade ----------------------------------------------------------------------------------------------------------------

def test_cpp_facade_render_equals_keyframe_map_render():
    d.build()
    exe = tmr.build_render_facade_check()
    n, w, h = 3, 64, 48
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "view.bin")
        out = subprocess.run([exe, str(n), path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, np.float32).reshape(2, h, w)
    ctx = d.default_context()
    K = np.array([60.0, 60.0, 31.5, 23.5], np.float32)
    cam = camera(ctx, w, h, K, 1)
    pyramids, poses = [], []
    for k in range(n):
        I, Z, T = facade_frame(k)
        pyramids.append(cam.create(I, Z))
        poses.append(T)
    m = d.KeyframeMap(ctx, 0.01, 1 << 20)
    m.insert(pyramids, np.stack(poses))
    pose = np.eye(4)
    pose[:3, 3] = [0.03, -0.02, -0.05]
    I, Z = m.render(K, w, h, pose)
    assert holes(Z).any() and (~holes(Z)).sum() > w * h // 2
    assert same_bits((got[0], got[1]), (I[0], Z[0]))
    m.close()
