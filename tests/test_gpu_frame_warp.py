"""GPU tier: frames warped under a pose on the device (include/dvo_hip.h, dvo_hip_frames_warp_inverse and dvo_hip_frames_warp_forward;
k_warp_inverse, k_warp_forward).  The yardstick is warp_inverse_host() / warp_forward_host() of tests/test_frame_warp.py -- the host build
of dvo_slam_amd/csrc/frame_warp.h -- fed the planes the device itself holds at the level: the device planes equal it BIT FOR BIT.
  1. bit-for-bit equality at 64 x 48 and 128 x 96, levels 0 to 2 (16 x 12: a raster narrower than a wavefront, a pixel count that is no
     multiple of 256), n = 1 and n = 5 distinct frames under 5 distinct transforms, host and device output, both forward modes;
     one call with more items than the grid is high; items of differing sizes;
  2. forward device planes fed to the float ingest give the frame the same planes give from the host;
  3. a warp issued after a deferred re-ingest sees the new planes;
  4. refusals, the counter;
  5. a map render, a forward warp and the same render again: the z-buffer scratch is shared;
  6. the C++ facade's RgbdImage::warp* against the Python wrappers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import scenes
import test_frame_warp as tfw
from dvo_slam_amd import _lib
from test_frame_warp import NEAREST, SPLAT, holes, same_bits, warp_forward_host, warp_inverse_host
from test_gpu_cloud_map import planes_of
from test_gpu_f32_ingest import blank_frames, camera

pytestmark = pytest.mark.gpu
INF = float("inf")
MODES = {"nearest": NEAREST, "splat": SPLAT}
GRID_ROWS = 1024                    # frame_warp.hip, warp_grid: the items beyond that many are walked by the kernels


def frames_of(w, h, n=5, levels=3):
    """(ctx, n pyramids of distinct planes of the (w, h) scenes, n distinct transforms of a few centimetres and degrees)"""
    ctx = d.default_context()
    pairs = [tfw.scene_pair("fr1", seed, w, h, 1)[0][0] for seed in (3, 5, 7)]
    cam = camera(ctx, w, h, pairs[0][0], levels)
    planes = [view for K, ref, cur in pairs for view in (ref, cur)][:n]
    pyramids = [cam.create(I, Z) for I, Z in planes]
    transforms = np.stack([scenes.se3_exp([0.02 * (k + 1), -0.015 * k, -0.03 * (k % 3), 0.02 * k, -0.015 * (k + 1), 0.01 * k]) for k in range(n)])
    return ctx, pyramids, transforms


def host_arrays(planes, device):
    if not device:
        return planes
    torch.cuda.synchronize()
    return [p.cpu().numpy() for p in planes]


def want_inverse(raster, sampled, T, level, **kw):
    (IR, ZR, KR), (IS, ZS, KS) = planes_of(raster, level), planes_of(sampled, level)
    return warp_inverse_host(IR, ZR, IS, ZS, KR, KS, T, difference=True, **kw)


def want_forward(pyramid, T, level, mode, **kw):
    I, Z, K = planes_of(pyramid, level)
    return warp_forward_host(I, Z, K, T, MODES[mode], **kw)


# ---- 1. bit for bit -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(64, 48), (128, 96)])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_warps_equal_the_host_build(shape, level):
    w, h = shape
    ctx, pyramids, T = frames_of(w, h)
    sampled = pyramids[1:] + pyramids[:1]                            # item k: frame k's raster, frame k + 1 sampled
    wl, hl = w >> level, h >> level
    for n in (1, 5):
        for device in (False, True):
            got = d.warp_inverse_batch(pyramids[:n], sampled[:n], T[:n], level=level, difference=True, device=device)
            assert len(got) == 3 and all(len(g) == n for g in got)
            for k in range(n):
                item = host_arrays([g[k] for g in got], device)
                assert item[0].shape == (hl, wl)
                want = want_inverse(pyramids[k], sampled[k], T[k], level)
                assert same_bits(item, want), (shape, level, n, device, k, "inverse")
                assert np.isfinite(want[0]).sum() > 0.3 * wl * hl and np.isnan(want[0]).any()
            two = d.warp_inverse_batch(pyramids[:n], sampled[:n], T[:n], level=level, occlusion_margin=0.01, device=device)
            assert len(two) == 2
            for k in range(n):
                assert same_bits(host_arrays([g[k] for g in two], device), want_inverse(pyramids[k], sampled[k], T[k], level, margin=0.01)[:2]), (k, "margin")
            for mode in MODES:
                got = d.warp_forward_batch(pyramids[:n], T[:n], level=level, mode=mode, device=device)
                for k in range(n):
                    want = want_forward(pyramids[k], T[k], level, mode)
                    assert same_bits(host_arrays([g[k] for g in got], device), want), (shape, level, n, device, k, mode)
                    assert (~holes(want[1])).sum() > 0.3 * wl * hl
    # a depth range on the forward warp
    near = d.warp_forward_batch(pyramids[:2], T[:2], level=level, mode="nearest", min_depth=0.8, max_depth=1.6)
    for k in range(2):
        want = want_forward(pyramids[k], T[k], level, "nearest", min_depth=0.8, max_depth=1.6)
        assert same_bits([g[k] for g in near], want) and not same_bits(want, want_forward(pyramids[k], T[k], level, "nearest")), k


def test_more_items_than_the_grid_is_high():
    """1030 items of 16 x 12 (level 2 of 64 x 48) over five frames, every item under a transform of its own: the launch's grid has
    1024 rows, the kernels walk the rest; an item index in the wrong place shows in the planes"""
    ctx, pyramids, _ = frames_of(64, 48)
    n, level = GRID_ROWS + 6, 2
    T = np.stack([scenes.se3_exp([0.0001 * k, -0.00005 * k, -0.00008 * k, 0.00004 * k, -0.00006 * k, 0.00002 * k]) for k in range(n)])
    raster, sampled = [pyramids[k % 5] for k in range(n)], [pyramids[(k + 2) % 5] for k in range(n)]
    planes = [planes_of(p, level) for p in pyramids]
    inv = d.warp_inverse_batch(raster, sampled, T, level=level, difference=True)
    fwd = d.warp_forward_batch(raster, T, level=level)
    for k in list(range(8)) + list(range(GRID_ROWS - 4, n)):
        (IR, ZR, K), (IS, ZS, _) = planes[k % 5], planes[(k + 2) % 5]
        assert same_bits([g[k] for g in inv], warp_inverse_host(IR, ZR, IS, ZS, K, K, T[k], difference=True)), k
        assert same_bits([g[k] for g in fwd], warp_forward_host(IR, ZR, K, T[k], SPLAT)), k
    assert not same_bits([g[n - 1] for g in fwd], [g[n - 6] for g in fwd])           # (the same frame under another transform: other planes)


def test_items_of_differing_sizes_share_a_call():
    ctx, small, Ts = frames_of(64, 48)
    _, large, Tl = frames_of(128, 96)
    raster, sampled = [small[0], large[0], small[2]], [small[1], large[1], small[3]]
    T = np.stack([Ts[0], Tl[1], Ts[2]])
    for device in (False, True):
        inv = d.warp_inverse_batch(raster, sampled, T, level=1, difference=True, device=device)
        for mode in MODES:
            fwd = d.warp_forward_batch(raster, T, level=1, mode=mode, device=device)
            for k in range(3):
                assert same_bits(host_arrays([g[k] for g in fwd], device), want_forward(raster[k], T[k], 1, mode)), (device, mode, k)
        for k in range(3):
            assert same_bits(host_arrays([g[k] for g in inv], device), want_inverse(raster[k], sampled[k], T[k], 1)), (device, k)


# ---- 2. predicted planes into frames --------------------------------------------------------------------------------------------------

def test_forward_device_planes_feed_the_float_ingest():
    w, h = 128, 96
    ctx, pyramids, T = frames_of(w, h, 2)
    cam = pyramids[0].camera
    I, Z = d.warp_forward_batch(pyramids, T, device=True)
    fed = blank_frames(cam, 2)
    d.update_f32_device_batch(fed, [t.data_ptr() for t in I], [t.data_ptr() for t in Z])
    Ih, Zh = d.warp_forward_batch(pyramids, T)
    from_host = blank_frames(cam, 2)
    d.update_f32_host_batch(from_host, Ih, Zh)
    d.upload_wait(ctx)
    for k in range(2):
        got, want = planes_of(fed[k], 0), planes_of(from_host[k], 0)
        assert same_bits(got[:2], want[:2]) and same_bits(got[:2], (Ih[k], Zh[k])), k
        assert same_bits(planes_of(fed[k], 1)[:2], planes_of(from_host[k], 1)[:2]), k
        assert (~holes(got[1])).sum() > 0.5 * w * h


# ---- 3. deferred ingests --------------------------------------------------------------------------------------------------------------

def test_a_warp_after_a_deferred_reingest_sees_the_new_planes():
    w, h = 64, 48
    ctx, pyramids, T = frames_of(w, h, 4)
    cam = pyramids[0].camera
    a, b = blank_frames(cam, 1)[0], blank_frames(cam, 1)[0]
    new = [planes_of(p, 0)[:2] for p in pyramids[2:4]]
    dev = [[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in pair] for pair in new]
    c0 = ctx.counter("deferred_ingests")
    d.update_f32_device_batch([a, b], [dev[0][0].data_ptr(), dev[1][0].data_ptr()], [dev[0][1].data_ptr(), dev[1][1].data_ptr()],
                              flags=_lib.INGEST_DEFER)
    inv = d.warp_inverse_batch([a], [b], T[:1], level=1, difference=True)
    assert ctx.counter("deferred_ingests") == c0 + 1                 # the recorded ingest (one call) was carried out, not dropped
    assert same_bits([g[0] for g in inv], want_inverse(pyramids[2], pyramids[3], T[0], 1))
    d.update_f32_device_batch([a], [dev[1][0].data_ptr()], [dev[1][1].data_ptr()], flags=_lib.INGEST_DEFER)
    fwd = d.warp_forward_batch([a], T[1:2], level=0)
    assert same_bits([g[0] for g in fwd], want_forward(pyramids[3], T[1], 0, "splat"))


# ---- 4. refusals and the counter ------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing_and_the_counter_counts_items():
    w, h = 64, 48
    ctx, pyramids, transforms = frames_of(w, h, 3)
    L = ctx._lib
    other = d.Context(0)
    K = planes_of(pyramids[0], 0)[2]
    foreign = camera(other, w, h, K, 3).create(*planes_of(pyramids[0], 0)[:2])
    larger = camera(ctx, 128, 96, K, 3).create(*tfw.scene_pair("fr1", 3, 128, 96, 1)[0][0][1])
    shallow = camera(ctx, w, h, K, 1).create(*planes_of(pyramids[0], 0)[:2])
    T = np.ascontiguousarray(transforms[:2], np.float64)
    tp = T.ctypes.data_as(C.POINTER(C.c_double))
    out = [np.full((h, w), -7.0, np.float32) for _ in range(6)]
    oi, oz, od = ((C.c_void_p * 2)(out[2 * k].ctypes.data, out[2 * k + 1].ctypes.data) for k in range(3))
    nulled = (C.c_void_p * 2)(out[0].ctypes.data, None)
    handles = lambda *p: (C.c_void_p * len(p))(*[x if x is None else x.ptr for x in p])      # noqa: E731
    fr, sa = handles(pyramids[0], pyramids[1]), handles(pyramids[1], pyramids[2])
    good = d.warp_params_struct()

    def params(**kw):
        p = d.warp_params_struct()
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return C.byref(p)

    def T_with(value, at):
        bad = T.copy()
        bad.reshape(-1)[at] = value
        return bad.ctypes.data_as(C.POINTER(C.c_double)), bad

    def inverse(ctx_=ctx.ptr, n=2, r=fr, s=sa, t=tp, level=0, p=C.byref(good), i=oi, z=oz, dd=od, dev=0):
        return L.dvo_hip_frames_warp_inverse(ctx_, n, r, s, t, level, p, i, z, dd, dev)

    def forward(ctx_=ctx.ptr, n=2, f=fr, t=tp, level=0, p=C.byref(good), i=oi, z=oz, dev=0):
        return L.dvo_hip_frames_warp_forward(ctx_, n, f, t, level, p, i, z, dev)

    bad_params = [dict(mode=2), dict(mode=-1), dict(occlusion_margin=-0.01), dict(occlusion_margin=float("nan")), dict(min_depth=2.0, max_depth=1.0),
                  dict(min_depth=float("nan")), dict(max_depth=float("nan")), dict(reserved=0), dict(reserved=3)]
    bad_T = [T_with(np.nan, 3), T_with(np.inf, 16 + 5), T_with(-np.inf, 11), T_with(np.nan, 31)]
    misaligned = (C.c_void_p * 2)(1 << 20 | 8, 1 << 21 | 4)
    aligned = (C.c_void_p * 2)(1 << 20, 1 << 21)
    c1 = ctx.counter("frame_warps")
    calls = [lambda: inverse(ctx_=other.ptr), lambda: inverse(n=0), lambda: inverse(n=-2), lambda: inverse(r=None), lambda: inverse(s=None),
             lambda: inverse(t=None), lambda: inverse(i=None), lambda: inverse(z=None), lambda: inverse(i=nulled), lambda: inverse(z=nulled),
             lambda: inverse(dd=nulled), lambda: inverse(r=handles(pyramids[0], None)), lambda: inverse(s=handles(pyramids[1], None)),
             lambda: inverse(r=handles(pyramids[0], foreign)), lambda: inverse(s=handles(foreign, pyramids[2])),
             lambda: inverse(level=3), lambda: inverse(level=-1), lambda: inverse(level=1, s=handles(pyramids[1], shallow)),
             lambda: inverse(s=handles(pyramids[1], larger)), lambda: inverse(r=handles(larger, pyramids[1])),
             lambda: inverse(i=misaligned, z=aligned, dd=None, dev=1), lambda: inverse(i=aligned, z=misaligned, dd=None, dev=1),
             lambda: inverse(i=aligned, z=aligned, dd=misaligned, dev=1),
             lambda: forward(ctx_=other.ptr), lambda: forward(n=0), lambda: forward(f=None), lambda: forward(t=None), lambda: forward(i=None),
             lambda: forward(z=None), lambda: forward(i=nulled), lambda: forward(z=nulled), lambda: forward(f=handles(pyramids[0], None)),
             lambda: forward(f=handles(foreign, pyramids[1])), lambda: forward(level=3), lambda: forward(level=-1),
             lambda: forward(level=1, f=handles(shallow, pyramids[1])), lambda: forward(i=misaligned, z=aligned, dev=1),
             lambda: forward(i=aligned, z=misaligned, dev=1)]
    calls += [lambda b=b: inverse(p=params(**b)) for b in bad_params] + [lambda b=b: forward(p=params(**b)) for b in bad_params]
    calls += [lambda b=b: inverse(t=b[0]) for b in bad_T] + [lambda b=b: forward(t=b[0]) for b in bad_T]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
    assert all(np.all(o == -7.0) for o in out) and ctx.counter("frame_warps") == c1
    # the same calls with nothing wrong
    assert inverse() == 0 and not any(np.any(o == -7.0) for o in out) and ctx.counter("frame_warps") == c1 + 2
    assert same_bits([out[0], out[2], out[4]], want_inverse(pyramids[0], pyramids[1], T[0], 0))
    assert same_bits([out[1], out[3], out[5]], want_inverse(pyramids[1], pyramids[2], T[1], 0))
    for o in out:
        o[...] = -7.0
    assert inverse(dd=None, p=None) == 0 and np.all(out[4] == -7.0) and np.all(out[5] == -7.0) and not np.any(out[0] == -7.0)
    for o in out:
        o[...] = -7.0
    assert forward(n=1) == 0 and ctx.counter("frame_warps") == c1 + 5 and np.all(out[1] == -7.0) and np.all(out[3] == -7.0)
    assert same_bits([out[0], out[2]], want_forward(pyramids[0], T[0], 0, "splat"))
    assert forward(p=None) == 0 and ctx.counter("frame_warps") == c1 + 7
    d.warp_forward_batch(pyramids, transforms, level=2)
    d.warp_inverse_batch(pyramids[:1], pyramids[1:2], transforms[:1])
    assert ctx.counter("frame_warps") == c1 + 11
    with pytest.raises(ValueError):
        d.warp_forward_batch([foreign, pyramids[0]], T)
    p = L.dvo_hip_warp_params_default()
    assert (p.mode, p.min_depth, p.max_depth, list(p.reserved)) == (SPLAT, 0.0, INF, [0] * 4) and p.occlusion_margin == np.float32(0.05)
    del foreign
    other.close()


# ---- 5. the shared z-buffer scratch ---------------------------------------------------------------------------------------------------

def test_a_forward_warp_between_two_renders_leaves_the_render_as_it_was():
    w, h = 128, 96
    ctx, pyramids, T = frames_of(w, h, 3)
    K = planes_of(pyramids[0], 0)[2]
    poses = np.stack([np.eye(4), T[0], T[1]])
    m = d.KeyframeMap(ctx, 0.02, 1 << 17)
    m.insert(pyramids, poses)
    views = np.stack([T[2], np.eye(4)])
    first = m.render(K, w, h, views)
    assert (~holes(first[1])).sum() > 0.5 * first[1].size
    fwd = d.warp_forward_batch(pyramids, T, level=0)                 # three z-buffers where the render had two
    again = m.render(K, w, h, views)
    assert same_bits(again, first)
    assert same_bits([g[1] for g in d.warp_forward_batch(pyramids, T, level=0)], [g[1] for g in fwd])   # ... and the other way round
    small = m.render(K, w // 2, h // 2, views[:1])                   # a smaller render, then the warp again
    assert small[1].shape == (1, h // 2, w // 2)
    for k in range(3):
        assert same_bits([g[k] for g in d.warp_forward_batch(pyramids, T, level=0)], want_forward(pyramids[k], T[k], 0, "splat")), k
    m.close()


# ---- 6. the C++ facade ----------------------------------------------------------------------------------------------------------------

def facade_frame(k, w=64, h=48):
    """frame k of tests/cpp/frame_warp_facade_check.cpp: integer-valued formulas, exact in float32 on both sides"""
    y, x = np.mgrid[0:h, 0:w]
    I = ((x * 7 + y * 13 + k * 5) % 256).astype(np.float32)
    Z = (1000 + (x * 3 + y * 5 + k * 11) % 512).astype(np.float32) * np.float32(0.001)
    Z[(x // 2 + 2 * (y // 2) + k) % 29 == 0] = np.nan
    return I, Z


def test_cpp_facade_warps_equal_the_python_wrappers():
    d.build()
    exe = tfw.build_warp_facade_check()
    w, h, level = 64, 48, 1
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "warps.bin")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, np.float32).reshape(6, h >> level, w >> level)
    ctx = d.default_context()
    cam = camera(ctx, w, h, np.array([60.0, 60.0, 31.5, 23.5], np.float32), 3)
    a, b = cam.create(*facade_frame(0)), cam.create(*facade_frame(1))
    T = np.eye(4)
    T[0, 2], T[2, 0] = 1.0 / 64, -1.0 / 64
    T[:3, 3] = [0.02, -0.01, -0.15]
    inv = d.warp_inverse_batch([a], [b], T, level=level)
    assert same_bits((got[0], got[1]), (inv[0][0], inv[1][0]))
    for k, mode in ((2, "nearest"), (4, "splat")):
        fwd = d.warp_forward_batch([a], T, level=level, mode=mode)
        assert same_bits((got[k], got[k + 1]), (fwd[0][0], fwd[1][0])), mode
