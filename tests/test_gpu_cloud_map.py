"""GPU tier: the keyframe map on the device (include/dvo_hip.h, dvo_hip_map_* and dvo_hip_frames_world_points; k_world_points,
k_map_insert, k_map_extract, k_map_clear).  The yardstick is the host build of dvo_slam_amd/csrc/cloud_map.h (tests/test_cloud_map.py,
world() and HostMap), fed the planes dvo_hip_frame_download_plane returns: the device results equal it BIT FOR BIT -- every accumulation
is an integer atomic, so nothing depends on the order the device visits the pixels in.
  1. the organised cloud, host and device output, levels 0 and 1, two frames under different poses in one call, holes;
  2. the map: keys, counts and xyzi of the sorted extraction, 2 to 4 overlapping frames, leaf 0.02;
  3. contention and run folding: a fronto-parallel plane at a 0.5 m leaf, a single-pixel hole inside a run, a checkerboard of holes;
  4. a table of 2^10 slots, a third full: probing;
  5. overflow is an error, not a hang: 64 slots; extract with too small a max_points writes nothing beyond it;
  6. flags and lifetime: deferred ingest, re-ingest, depth range, lens and depth rig, refusals, counters;
  7. the C++ facade's PointCloudAggregator against KeyframeMap."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import scenes
import test_cloud_map as tcm
import test_depth_rig as tdr
from dvo_slam_amd import _lib
from test_cloud_map import HostMap, assert_maps_identical, world
from test_gpu_f32_ingest import blank_frames, camera
from test_gpu_lens_ingest import SCALE, ingest, lens_of, raw_scene

pytestmark = pytest.mark.gpu
INF = float("inf")
SHAPES = [(128, 96), (321, 240), (102, 78)]      # a multiple of 64; an odd width: waves straddle rows; no multiple of 4 or 64


def frames_of(w, h, n, levels=3):
    """n pyramids of the (w, h) scene with their poses: views 0 and 1 under their true poses, further ones the same planes under poses a
    few centimetres and degrees off (overlapping, not coincident)"""
    K, views = tcm.float_views(w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    pyramids, poses = [], []
    for k in range(n):
        I, Z, T = views[k % 2]
        if k >= 2:
            T = T @ scenes.se3_exp([0.03 * k, -0.02, 0.01 * k, 0.01, -0.02 * k, 0.015])
        pyramids.append(cam.create(I, Z))
        poses.append(T)
    return ctx, pyramids, np.stack(poses)


def planes_of(pyramid, level):
    """(I, Z, K) of a level as dvo_hip_frame_download_plane returns them: what the map reads"""
    img = pyramid.level(level)
    return np.array(img.intensity, copy=True), np.array(img.depth, copy=True), np.array(img.K, copy=True)


def yardstick(pyramids, poses, level, leaf, capacity, min_depth=0.0, max_depth=INF):
    m = HostMap(leaf, capacity)
    for p, T in zip(pyramids, poses):
        I, Z, K = planes_of(p, level)
        m.insert(I, Z, K, T, min_depth, max_depth)
    return m


def roomy(pyramids, poses, level, leaf, min_depth=0.0, max_depth=INF):
    """the yardstick in a table at least four times its voxels, with the preconditions under which the device cannot drop: the set of
    occupied slots under linear probing does not depend on the insertion order, so the device's probe sequences are the yardstick's"""
    want = yardstick(pyramids, poses, level, leaf, 1 << 22, min_depth, max_depth)
    capacity = 64
    while capacity < 4 * want.stats()["occupied"]:
        capacity *= 2
    want = yardstick(pyramids, poses, level, leaf, capacity, min_depth, max_depth)
    assert want.stats()["dropped"] == 0 and capacity >= 4 * want.stats()["occupied"] and want.longest_run() < tcm.MAX_PROBES
    return want, capacity


def check_against(m, want, what):
    got = m.extract(sort=True)
    assert_maps_identical(got, want.extract(), what)
    s, ws = m.stats(), want.stats()
    for k in ("occupied", "points", "dropped", "out_of_range", "unusable", "capacity"):
        assert s[k] == ws[k], (what, k, s, ws)
    assert s["over_limit"] == 0 and 0 < s["updates"] <= s["points"]
    return got


# ---- 1. the organised cloud -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("level", [0, 1])
def test_world_points_equal_the_yardstick(w, h, level):
    ctx, pyramids, poses = frames_of(w, h, 2)
    want = []
    for p, T in zip(pyramids, poses):
        I, Z, K = planes_of(p, level)
        want.append(world(I, Z, K, T))
        assert np.isnan(want[-1][..., 0]).any() and np.isfinite(want[-1][..., 0]).any()          # holes present
    assert not np.array_equal(poses[0], poses[1])
    host = d.world_points_batch(pyramids, poses, level)
    dev = d.world_points_batch(pyramids, poses, level, device=True)
    torch.cuda.synchronize()
    for k in range(2):
        assert host[k].shape == want[k].shape
        assert np.array_equal(host[k].view(np.uint32), want[k].view(np.uint32)), (w, h, level, k, "host")
        assert np.array_equal(dev[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), (w, h, level, k, "device")
    I, Z, K = planes_of(pyramids[0], level)
    lo, hi = (float(x) for x in np.nanpercentile(Z, [30, 70]))
    ranged = d.world_points_batch(pyramids[:1], poses[:1], level, lo, hi)[0]
    assert np.array_equal(ranged.view(np.uint32), world(I, Z, K, poses[0], lo, hi).view(np.uint32))


# ---- 2. the map equals the yardstick ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,n", [(128, 96, 2), (321, 240, 3), (102, 78, 4)])
def test_map_equals_the_yardstick(w, h, n):
    ctx, pyramids, poses = frames_of(w, h, n)
    want, capacity = roomy(pyramids, poses, 0, 0.02)
    m = d.KeyframeMap(ctx, 0.02, capacity)
    m.insert(pyramids, poses)
    assert m.stats()["dropped"] == 0
    got = check_against(m, want, (w, h, n))
    assert (got[1] > 1).sum() > 50                                  # voxels that several pixels, and several frames, share
    # the device output, unsorted: the same records in some order
    xyzi, counts, keys = m.extract(device=True)
    torch.cuda.synchronize()
    order = np.argsort(keys.cpu().numpy().view(np.uint64), kind="stable")
    assert_maps_identical((xyzi.cpu().numpy()[order], counts.cpu().numpy().view(np.uint32)[order], keys.cpu().numpy().view(np.uint64)[order]), got, "device")
    # level 1, one frame per call: the same map as all frames in one call
    want1, capacity1 = roomy(pyramids, poses, 1, 0.02)
    one, each = d.KeyframeMap(ctx, 0.02, capacity1), d.KeyframeMap(ctx, 0.02, capacity1)
    one.insert(pyramids, poses, level=1)
    for p, T in zip(pyramids, poses):
        each.insert([p], T[None], level=1)
    check_against(one, want1, "level 1")
    assert_maps_identical(one.extract(sort=True), each.extract(sort=True), "frame by frame")
    for x in (m, one, each):
        x.close()


def test_frames_of_different_sizes_share_a_call():
    ctx, a, pa = frames_of(128, 96, 2)
    _, b, pb = frames_of(102, 78, 1)
    pyramids, poses = [a[0], b[0], a[1]], np.stack([pa[0], pb[0], pa[1]])
    want, capacity = roomy(pyramids, poses, 0, 0.05)
    m = d.KeyframeMap(ctx, 0.05, capacity)
    m.insert(pyramids, poses)
    check_against(m, want, "mixed sizes")
    clouds = d.world_points_batch(pyramids, poses)
    for p, T, got in zip(pyramids, poses, clouds):
        I, Z, K = planes_of(p, 0)
        assert np.array_equal(got.view(np.uint32), world(I, Z, K, T).view(np.uint32))
    m.close()


# ---- 3. contention and run folding ------------------------------------------------------------------------------------------------------

def plane_frame(w, h, holes):
    K = np.array([0.8 * w, 0.8 * w, w / 2 - 0.5, h / 2 - 0.5], np.float32)
    y, x = np.mgrid[0:h, 0:w]
    Z = np.full((h, w), 2.0, np.float32)
    I = ((x * 3 + y * 7) % 256).astype(np.float32) + np.float32(0.25)
    if holes == "single":
        Z[h // 2, w // 2] = np.nan                                  # one hole inside a run
        Z[3, 17] = np.nan
    elif holes == "checkerboard":
        Z[(x + y) % 2 == 1] = np.nan                                # every run has length 1
    ctx = d.default_context()
    return ctx, camera(ctx, w, h, K, 2).create(I, Z)


@pytest.mark.parametrize("holes", ["none", "single", "checkerboard"])
@pytest.mark.parametrize("w,h", [(321, 240), (128, 96)])
@pytest.mark.parametrize("leaf,tx", [(0.5, 0.1), (4.0, 2.0)])
def test_long_runs_and_contended_voxels(w, h, holes, leaf, tx):
    """the plane at Z = 2 m spans 2.5 m in X.  Leaf 0.5: a row falls into 5 or 6 voxels.  Leaf 4 with the plane moved to X in
    [0.75, 3.25]: a whole row lies in one x-voxel, so every run goes on over the row's end into the next row (two voxels in all, split
    in Y), at a width (321) where the row ends fall inside the wavefronts"""
    ctx, p = plane_frame(w, h, holes)
    T = np.eye(4)
    T[:3, 3] = [tx, -0.2, 0.3]                                      # fronto-parallel: whole rows fall into a handful of voxels
    want, capacity = roomy([p], [T], 0, leaf)
    assert want.stats()["occupied"] <= (40 if leaf == 0.5 else 2)
    if holes != "checkerboard":
        voxel = np.floor(world(*planes_of(p, 0), T)[..., :3].astype(np.float64) / leaf)
        crossing = int(np.all(voxel[:-1, -1] == voxel[1:, 0], axis=-1).sum())   # rows whose last pixel shares a voxel with the next row's first
        assert crossing == (0 if leaf == 0.5 else h - 2)            # (h - 2: one row end lies on the split in Y)
    m = d.KeyframeMap(ctx, leaf, capacity)
    m.insert([p], T[None])
    got = check_against(m, want, (w, h, holes))
    usable = int(np.isfinite(planes_of(p, 0)[1]).sum())
    assert int(got[1].sum()) == usable == m.stats()["points"] and got[1].max() > 200       # (hundreds of pixels contend for a voxel)
    m.close()


# ---- 4. a small table -------------------------------------------------------------------------------------------------------------------

def test_a_table_of_1024_slots_a_third_full():
    ctx, pyramids, poses = frames_of(128, 96, 2)
    want = yardstick(pyramids, poses, 0, 0.25, 1 << 10, 0.0, 5.0)
    assert 300 <= want.stats()["occupied"] <= 450 and want.stats()["dropped"] == 0 and 1 < want.longest_run() < tcm.MAX_PROBES
    m = d.KeyframeMap(ctx, 0.25, 1 << 10)
    m.insert(pyramids, poses, max_depth=5.0)
    check_against(m, want, "2^10 slots")
    m.close()


# ---- 5. overflow ------------------------------------------------------------------------------------------------------------------------

def test_overflow_is_an_error_not_a_hang():
    ctx, pyramids, poses = frames_of(128, 96, 2)
    assert yardstick(pyramids, poses, 0, 0.02, 1 << 20).stats()["occupied"] > 64
    m = d.KeyframeMap(ctx, 0.02, 64)
    c0 = ctx.counter("map_dropped")
    with pytest.raises(d.DvoHipError) as e:
        m.insert(pyramids, poses)
    assert e.value.code == _lib.ERR_CAPACITY
    s = m.stats()
    usable = sum(int((np.isfinite(planes_of(p, 0)[1]) & (planes_of(p, 0)[1] > 0)).sum()) for p in pyramids)
    assert s["capacity"] == 64 and s["dropped"] > 0 and s["occupied"] <= 64 and s["points"] + s["dropped"] == usable
    assert ctx.counter("map_dropped") - c0 == s["dropped"]
    assert int(m.extract()[1].sum()) == s["points"]                 # the map keeps what it took
    m.clear()
    assert m.stats()["occupied"] == 0 and m.stats()["dropped"] == 0 and len(m.extract()[2]) == 0
    # the map that overflowed, cleared, takes an insert that fits: a depth band that holds about 40 pixels of the two frames, which at
    # this leaf is fewer than 64 voxels (the probe bound exceeds the table: every key finds a slot)
    zs = np.sort(np.concatenate([planes_of(p, 0)[1].ravel() for p in pyramids]))
    zs = zs[np.isfinite(zs) & (zs > 0)]
    lo, hi = float(zs[len(zs) // 2 - 20]), float(zs[len(zs) // 2 + 19])
    fitting = yardstick(pyramids, poses, 0, 0.02, 64, lo, hi)
    assert fitting.stats()["dropped"] == 0 and 4 <= fitting.stats()["occupied"] < 64 and fitting.stats()["points"] >= 40
    m.insert(pyramids, poses, min_depth=lo, max_depth=hi)
    check_against(m, fitting, "the overflowed map after clear")
    # max_points too small: DVO_HIP_ERR_CAPACITY, nothing written beyond it (a guard band behind each array); a map with a leaf so large
    # that the whole scene fits the 64 slots
    want = yardstick(pyramids, poses, 0, 4.0, 64)
    assert want.stats()["dropped"] == 0 and 4 <= want.stats()["occupied"] < 64
    coarse = d.KeyframeMap(ctx, 4.0, 64)
    coarse.insert(pyramids, poses)
    check_against(coarse, want, "a 4 m leaf")
    n = want.stats()["occupied"]
    assert n >= 4
    take, guard = n - 2, 16
    xyzi, counts, keys = np.full((take + guard, 4), -7.0, np.float32), np.full(take + guard, 0xABCDABCD, np.uint32), np.full(take + guard, 77, np.uint64)
    got = C.c_size_t(0)
    rc = ctx._lib.dvo_hip_map_extract(ctx.ptr, coarse.ptr, take, xyzi.ctypes.data, counts.ctypes.data, keys.ctypes.data, 0, C.byref(got))
    assert rc == _lib.ERR_CAPACITY and got.value == take
    assert np.all(xyzi[take:] == -7.0) and np.all(counts[take:] == 0xABCDABCD) and np.all(keys[take:] == 77)
    assert set(keys[:take].tolist()) <= set(want.extract()[2].tolist()) and len(set(keys[:take].tolist())) == take
    dev = torch.full((take + guard, 4), -7.0, dtype=torch.float32, device="cuda")
    rc = ctx._lib.dvo_hip_map_extract(ctx.ptr, coarse.ptr, take, dev.data_ptr(), None, None, 1, C.byref(got))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_CAPACITY and got.value == take and bool((dev[take:] == -7.0).all()) and bool((dev[:take, 2] != -7.0).all())
    for x in (m, coarse):
        x.close()


# ---- 6. flags and lifetime --------------------------------------------------------------------------------------------------------------

def test_insert_after_a_deferred_ingest_and_a_reingest_and_with_a_depth_range():
    w, h, levels = 128, 96, 3
    K, views = raw_scene(w, h)
    ctx = d.default_context()
    frames = blank_frames(camera(ctx, w, h, K, levels), 2)
    poses = np.stack([np.eye(4), scenes.se3_exp([0.02, -0.01, 0.015, 0.01, 0.02, -0.01])])
    m = d.KeyframeMap(ctx, 0.05, 1 << 16)
    d0 = ctx.counter("deferred_ingests")
    keep = ingest(frames, [v["fimg"] for v in views], [v["fdepth"] for v in views], "f32", "f32", 0.5, "device", "current", levels, flags=_lib.INGEST_DEFER)
    assert ctx.counter("deferred_ingests") == d0
    m.insert(frames, poses)                                         # carries the recorded ingest out first
    assert ctx.counter("deferred_ingests") > d0
    first = check_against(m, yardstick(frames, poses, 0, 0.05, 1 << 16), "deferred")
    assert np.array_equal(planes_of(frames[0], 0)[1], views[0]["fdepth"] * np.float32(0.5), equal_nan=True)
    # the same frames re-ingested from other planes: after clear(), a new map
    keep += ingest(frames, [views[1]["grey"], views[0]["grey"]], [views[1]["depth"], views[0]["depth"]], "raw", "grey8", SCALE, "device", None, levels)
    m.clear()
    m.insert(frames, poses, level=1)
    second = check_against(m, yardstick(frames, poses, 1, 0.05, 1 << 16), "re-ingested")
    assert not np.array_equal(first[2], second[2])
    # a depth range
    _, Z, _ = planes_of(frames[0], 0)
    lo, hi = (float(x) for x in np.nanpercentile(Z, [20, 60]))
    m.clear()
    m.insert(frames, poses, min_depth=lo, max_depth=hi)
    ranged = yardstick(frames, poses, 0, 0.05, 1 << 16, lo, hi)
    check_against(m, ranged, "depth range")
    assert 0 < ranged.stats()["points"] < yardstick(frames, poses, 0, 0.05, 1 << 16).stats()["points"]
    m.close()
    del keep


def test_frames_with_a_lens_or_a_depth_rig_insert_their_own_planes():
    w, h, levels = 128, 96, 3
    K, views = raw_scene(w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    lensed, rigged = blank_frames(cam, 1), blank_frames(cam, 1)
    d.set_lens_batch(lensed, *lens_of(K, "plumb_bob"))
    d.set_depth_rig_batch(rigged, *tdr.kinect_rig(K))
    keep = ingest(lensed, [views[0]["grey"]], [views[0]["depth"]], "raw", "grey8", SCALE, "device", None, levels)
    keep += ingest(rigged, [views[1]["grey"]], [views[1]["depth"]], "raw", "grey8", SCALE, "host", "reference", levels)
    frames, poses = lensed + rigged, np.stack([np.eye(4), scenes.se3_exp([0.02, 0.0, 0.01, 0.0, 0.02, 0.0])])
    plain = blank_frames(cam, 1)
    keep += ingest(plain, [views[0]["grey"]], [views[0]["depth"]], "raw", "grey8", SCALE, "device", None, levels)
    assert not np.array_equal(planes_of(lensed[0], 0)[1], planes_of(plain[0], 0)[1], equal_nan=True)   # rectified, not the caller's plane
    want, capacity = roomy(frames, poses, 0, 0.05)
    m = d.KeyframeMap(ctx, 0.05, capacity)
    m.insert(frames, poses)
    check_against(m, want, "lens and rig")
    m.close()
    del keep


def test_refusals_change_nothing_and_counters_move_as_documented():
    ctx, pyramids, poses = frames_of(128, 96, 2)
    want, capacity = roomy(pyramids, poses, 0, 0.05)
    m = d.KeyframeMap(ctx, 0.05, capacity)
    names = ("map_inserts", "map_points", "map_dropped")
    c0 = [ctx.counter(k) for k in names]
    m.insert(pyramids, poses)
    s = m.stats()
    assert [ctx.counter(k) - a for k, a in zip(names, c0)] == [2, s["points"], 0]
    before = m.extract(sort=True)
    c1 = [ctx.counter(k) for k in names]
    other = d.Context(0)
    foreign = camera(other, 128, 96, pyramids[0].camera.K, 3).create(*tcm.float_views(128, 96)[1][0][:2])
    handles = (C.c_void_p * 2)(pyramids[0].ptr, pyramids[1].ptr)
    mixed = (C.c_void_p * 2)(pyramids[0].ptr, foreign.ptr)
    nulled = (C.c_void_p * 2)(pyramids[0].ptr, None)
    T = np.ascontiguousarray(poses, np.float64)
    tp = T.ctypes.data_as(C.POINTER(C.c_double))
    L = ctx._lib
    out = [np.full((96, 128, 4), -7.0, np.float32) for _ in range(2)]
    outs = (C.c_void_p * 2)(*[o.ctypes.data for o in out])
    calls = [
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 2, handles, tp, 3, 0.0, INF),          # a level the frames do not have
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 2, handles, tp, -1, 0.0, INF),
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 2, handles, None, 0, 0.0, INF),        # null poses
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 2, mixed, tp, 0, 0.0, INF),            # a frame of another context
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 2, nulled, tp, 0, 0.0, INF),
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 0, handles, tp, 0, 0.0, INF),
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 2, handles, tp, 0, 2.0, 1.0),
        lambda: L.dvo_hip_map_insert(ctx.ptr, m.ptr, 2, handles, tp, 0, float("nan"), 1.0),
        lambda: L.dvo_hip_map_insert(ctx.ptr, None, 2, handles, tp, 0, 0.0, INF),
        lambda: L.dvo_hip_map_insert(other.ptr, m.ptr, 2, handles, tp, 0, 0.0, INF),        # the map of another context
        lambda: L.dvo_hip_frames_world_points(ctx.ptr, 2, handles, tp, 3, 0.0, INF, outs, 0),
        lambda: L.dvo_hip_frames_world_points(ctx.ptr, 2, handles, None, 0, 0.0, INF, outs, 0),
        lambda: L.dvo_hip_frames_world_points(ctx.ptr, 2, mixed, tp, 0, 0.0, INF, outs, 0),
        lambda: L.dvo_hip_frames_world_points(ctx.ptr, 2, handles, tp, 0, 0.0, INF, None, 0),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
    assert all(np.all(o == -7.0) for o in out)
    assert [ctx.counter(k) for k in names] == c1 and m.stats() == s
    assert_maps_identical(m.extract(sort=True), before, "after the refusals")
    check_against(m, want, "after the refusals")
    ptr = C.c_void_p()
    for leaf in (0.0, -1.0, float("nan"), INF):
        assert L.dvo_hip_map_create(ctx.ptr, leaf, 1024, C.byref(ptr)) == _lib.ERR_INVALID and not ptr.value
    tiny = d.KeyframeMap(ctx, 0.05, 1)
    assert tiny.stats()["capacity"] == 64                           # rounded up to a power of two, at least 64
    odd = d.KeyframeMap(ctx, 0.05, 1000)
    assert odd.stats()["capacity"] == 1024
    with pytest.raises(ValueError):
        m.insert([foreign], np.eye(4)[None])                        # the Python wrapper refuses it first
    for x in (tiny, odd, m):
        x.close()
    del foreign
    other.close()


# ---- 7. the C++ facade ------------------------------------------------------------------------------------------------------------------

def facade_frame(k, w=64, h=48):
    """keyframe k of tests/cpp/map_facade_check.cpp: integer-valued formulas, exact in float32 on both sides"""
    y, x = np.mgrid[0:h, 0:w]
    I = ((x * 7 + y * 13 + k * 5) % 256).astype(np.float32)
    Z = (1000 + (x * 3 + y * 5 + k * 11) % 512).astype(np.float32) * np.float32(0.001)
    Z[(x + 2 * y + k) % 29 == 0] = np.nan
    T = np.eye(4)
    T[0, 2], T[2, 0] = k / 1024.0, -k / 1024.0                      # (applied as given; no trigonometry to round differently)
    T[:3, 3] = [0.01 * k, -0.005 * k, 0.002 * k]
    return I, Z, T


@pytest.mark.parametrize("n", [3, 120])
def test_cpp_facade_aggregator_equals_keyframe_map(n):
    d.build()
    exe = tcm.build_map_facade_check()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.bin")
        out = subprocess.run([exe, str(n), path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, np.float32).reshape(-1, 4)
    ctx = d.default_context()
    cam = camera(ctx, 64, 48, np.array([60.0, 60.0, 31.5, 23.5], np.float32), 1)
    step = max(n // 50, 1)
    names = sorted("kf%04d" % k for k in range(n))                  # the aggregator walks its keyframes in name order
    chosen = [int(name[2:]) for i, name in enumerate(names) if i % step == 0]
    assert len(chosen) == (3 if n == 3 else 60)
    pyramids, poses = [], []
    for k in chosen:
        I, Z, T = facade_frame(k)
        pyramids.append(cam.create(I, Z))
        poses.append(T)
    m = d.KeyframeMap(ctx, 0.01, 1 << 20)
    m.insert(pyramids, np.stack(poses))
    xyzi, counts, keys = m.extract(sort=True)
    assert len(xyzi) > 1000 and m.stats()["dropped"] == 0
    assert got.shape == xyzi.shape and np.array_equal(got.view(np.uint32), xyzi.view(np.uint32))
    m.close()
