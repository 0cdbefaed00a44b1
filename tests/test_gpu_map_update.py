"""GPU tier: a keyframe map that follows the pose graph (include/dvo_hip.h, dvo_hip_map_remove / _move / _rehash; k_map_insert over signed
frames, k_map_rehash, the vacant count of k_map_extract).  The yardstick in every case is the host map (tests/test_cloud_map.py, HostMap)
built from ONLY the frames that should remain, under the poses they should have, in a table sized by tests/test_gpu_cloud_map.py's
`roomy` rule: keys, counts and xyzi of the sorted extraction are identical bit for bit, and points, dropped, out_of_range and unusable
are those of the yardstick (a removal takes its frame's pixels out of all four).
  1. insert four, remove one -- each position in turn -- and two in one call; levels 0 and 1, 128 x 96 and 102 x 78, leaf 0.02 (a sparse
     table) and 0.5 (hundreds of pixels per voxel, 64-lane runs);
  2. move one frame, and all four by a small twist: the yardstick under the new poses, and remove + insert; an unchanged pose is skipped;
  3. a render after a removal equals the render of a map that never held the frame;
  4. rehash at the same capacity and to double; into 64 slots; growing a map that dropped points;
  5. refusals and counters;
  6. the C++ facade's incremental PointCloudAggregator (tests/cpp/map_update_facade_check.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import scenes
import test_cloud_map as tcm
import test_map_update as tmu
from dvo_slam_amd import _lib
from test_cloud_map import assert_maps_identical
from test_gpu_cloud_map import facade_frame, frames_of, planes_of, roomy, yardstick
from test_gpu_f32_ingest import camera

pytestmark = pytest.mark.gpu
INF = float("inf")
TWIST = [0.004, -0.003, 0.002, 0.001, -0.002, 0.0015]              # a pose-graph correction: millimetres and a tenth of a degree
STAT_KEYS = ("points", "dropped", "out_of_range", "unusable")


@functools.lru_cache(maxsize=None)
def four(w, h):
    """(ctx, pyramids, poses) of the four-frame set; built once per size and left unchanged"""
    return frames_of(w, h, 4)


def check_remaining(m, pyramids, poses, level, leaf, what, expect_vacant=None):
    """m against the yardstick built from these frames only; returns (the map's stats, the yardstick's)"""
    want, _ = roomy(pyramids, poses, level, leaf)
    assert_maps_identical(m.extract(sort=True), want.extract(), what)
    s, ws = m.stats(), want.stats()
    for k in STAT_KEYS:
        assert s[k] == ws[k], (what, k, s, ws)
    assert s["occupied"] - s["vacant"] == ws["occupied"] and s["over_limit"] == 0 and s["unmatched"] == 0, (what, s, ws)
    if expect_vacant is not None:
        assert (s["vacant"] > 0) == expect_vacant, (what, s)
    return s, ws


def capacity_for(pyramids, poses, level, leaf):
    return roomy(pyramids, poses, level, leaf)[1]


def without(items, gone):
    return [x for k, x in enumerate(items) if k not in gone]


# ---- 1. removal -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf", [0.02, 0.5])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("w,h", [(128, 96), (102, 78)])
def test_insert_four_remove_one_or_two(w, h, level, leaf):
    ctx, pyramids, poses = four(w, h)
    capacity = capacity_for(pyramids, poses, level, leaf)
    m = d.KeyframeMap(ctx, leaf, capacity)
    r0 = ctx.counter("map_removes")
    for gone in ([0], [1], [2], [3], [1, 3]):
        m.clear()
        m.insert(pyramids, poses, level=level)
        full = m.stats()
        assert full["vacant"] == full["removed"] == full["unmatched"] == 0
        m.remove([pyramids[k] for k in gone], poses[gone], level=level)
        s, ws = check_remaining(m, without(pyramids, gone), np.stack(without(list(poses), gone)), level, leaf, (w, h, level, leaf, gone), True)
        assert s["occupied"] == full["occupied"] and s["vacant"] == full["occupied"] - ws["occupied"]      # the keys stay in their slots
        assert s["removed"] == full["points"] - ws["points"] > 0 and s["capacity"] == capacity
    assert ctx.counter("map_removes") - r0 == 6
    m.close()


# ---- 2. moves ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf", [0.02, 0.5])
@pytest.mark.parametrize("w,h,level", [(128, 96, 0), (102, 78, 1)])
def test_move_equals_the_yardstick_under_the_new_poses_and_remove_plus_insert(w, h, level, leaf):
    ctx, pyramids, poses = four(w, h)
    for moving in ([2], [0, 1, 2, 3]):
        new = poses.copy()
        for k in moving:
            new[k] = poses[k] @ scenes.se3_exp([x * (k + 1) for x in TWIST])
        capacity = 4 * capacity_for(pyramids, new, level, leaf)     # (room for the slots the old poses leave vacant)
        moved, two_calls = d.KeyframeMap(ctx, leaf, capacity), d.KeyframeMap(ctx, leaf, capacity)
        for m in (moved, two_calls):
            m.insert(pyramids, poses, level=level)
        c0 = [ctx.counter(k) for k in ("map_removes", "map_inserts")]
        moved.move(pyramids, poses, new, level=level)               # all four are passed: those whose pose stays cost nothing
        assert [ctx.counter(k) - a for k, a in zip(("map_removes", "map_inserts"), c0)] == [len(moving), len(moving)]
        sel = [pyramids[k] for k in moving]
        two_calls.remove(sel, poses[moving], level=level)
        two_calls.insert(sel, new[moving], level=level)
        check_remaining(moved, pyramids, new, level, leaf, ("move", w, h, level, leaf, moving))
        assert_maps_identical(moved.extract(sort=True), two_calls.extract(sort=True), "remove + insert")
        assert moved.stats() == two_calls.stats()
        # ... and back again: the map of the first insertion
        moved.move(sel, new[moving], poses[moving], level=level)
        check_remaining(moved, pyramids, poses, level, leaf, ("moved back", moving))
        c1 = ctx.counter("map_removes")
        moved.move(pyramids, poses, poses, level=level)             # nothing moves: nothing is launched
        assert ctx.counter("map_removes") == c1
        for m in (moved, two_calls):
            m.close()


# ---- 3. rendering -----------------------------------------------------------------------------------------------------------------------

def test_a_render_after_a_removal_equals_the_render_of_a_map_that_never_held_the_frame():
    ctx, pyramids, poses = four(128, 96)
    capacity = capacity_for(pyramids, poses, 0, 0.02)
    held, never = d.KeyframeMap(ctx, 0.02, capacity), d.KeyframeMap(ctx, 0.02, capacity)
    held.insert(pyramids, poses)
    K = planes_of(pyramids[0], 0)[2]
    view = poses[2] @ scenes.se3_exp([0.01, 0.0, -0.01, 0.0, 0.01, 0.0])
    with_it = held.render(K, 128, 96, view)
    held.remove(pyramids[2:3], poses[2:3])
    never.insert(without(pyramids, [2]), np.stack(without(list(poses), [2])))
    assert held.stats()["vacant"] > 0
    got, want = held.render(K, 128, 96, view), never.render(K, 128, 96, view)
    for a, b, c in zip(got, want, with_it):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert not np.array_equal(a.view(np.uint32), c.view(np.uint32))          # the frame was seen in this view
    assert np.isfinite(got[1]).sum() > 1000
    for m in (held, never):
        m.close()


# ---- 4. rehash --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf", [0.02, 0.5])
def test_rehash_reclaims_vacant_slots_and_keeps_every_record(leaf):
    ctx, pyramids, poses = four(128, 96)
    capacity = capacity_for(pyramids, poses, 0, leaf)
    rest, rest_poses = without(pyramids, [2]), np.stack(without(list(poses), [2]))
    h0 = ctx.counter("map_rehashes")
    for new_capacity in (None, 2 * capacity):
        m = d.KeyframeMap(ctx, leaf, capacity)
        m.insert(pyramids, poses)
        m.remove(pyramids[2:3], poses[2:3])
        before, s0 = m.extract(sort=True), m.stats()
        assert s0["vacant"] > 0
        m.rehash(new_capacity)
        s = m.stats()
        assert_maps_identical(m.extract(sort=True), before, "rehash")
        assert s["vacant"] == 0 and s["occupied"] == len(before[2]) and s["capacity"] == (new_capacity or capacity) and s["dropped"] == 0
        for k in ("points", "removed", "unmatched", "out_of_range", "unusable", "updates", "over_limit"):
            assert s[k] == s0[k], k
        check_remaining(m, rest, rest_poses, 0, leaf, "rehashed", False)
        # a later insert and a later remove
        m.insert(pyramids[2:3], poses[2:3])
        check_remaining(m, pyramids, poses, 0, leaf, "rehashed + insert", False)
        m.remove(pyramids[:1], poses[:1])
        check_remaining(m, pyramids[1:], poses[1:], 0, leaf, "rehashed + insert + remove", True)
        m.close()
    assert ctx.counter("map_rehashes") - h0 == 2


def test_rehash_into_64_slots_and_growing_a_map_that_dropped_points():
    ctx, pyramids, poses = four(128, 96)
    capacity = capacity_for(pyramids, poses, 0, 0.02)
    m = d.KeyframeMap(ctx, 0.02, capacity)
    m.insert(pyramids, poses)
    before, s0, h0 = m.extract(sort=True), m.stats(), ctx.counter("map_rehashes")
    assert s0["occupied"] > 64
    with pytest.raises(d.DvoHipError) as e:
        m.rehash(64)
    assert e.value.code == _lib.ERR_CAPACITY and ctx.counter("map_rehashes") == h0
    assert m.stats() == s0
    assert_maps_identical(m.extract(sort=True), before, "after the failed rehash")
    m.remove(pyramids[3:], poses[3:])                               # the map is intact: it still takes a removal
    check_remaining(m, pyramids[:3], poses[:3], 0, 0.02, "after the failed rehash", True)
    for bad in (63, 1000, 32):
        assert ctx._lib.dvo_hip_map_rehash(ctx.ptr, m.ptr, bad) == _lib.ERR_INVALID
    m.close()
    # a map of 64 slots drops points: removals are refused until it has grown
    small = d.KeyframeMap(ctx, 0.02, 64)
    with pytest.raises(d.DvoHipError) as e:
        small.insert(pyramids[:1], poses[:1])
    assert e.value.code == _lib.ERR_CAPACITY
    s1, kept = small.stats(), small.extract(sort=True)
    assert s1["dropped"] > 0 and s1["occupied"] == 64
    r0 = ctx.counter("map_removes")
    with pytest.raises(d.DvoHipError) as e:
        small.remove(pyramids[:1], poses[:1])
    assert e.value.code == _lib.ERR_INVALID and "dropped" in str(e.value) and ctx.counter("map_removes") == r0
    with pytest.raises(d.DvoHipError):
        small.move(pyramids[:1], poses[:1], poses[1:2])
    assert small.stats() == s1
    assert_maps_identical(small.extract(sort=True), kept, "after the refused removal")
    small.rehash(1 << 12)
    s2 = small.stats()
    assert s2["dropped"] == 0 and s2["points"] == s1["points"] and s2["occupied"] == 64 and s2["capacity"] == 1 << 12
    assert_maps_identical(small.extract(sort=True), kept, "grown")
    # the refusal is lifted; the frame's dropped points are not in the table, so its removal leaves exactly those unmatched
    with pytest.raises(d.DvoHipError) as e:
        small.remove(pyramids[:1], poses[:1])
    s3 = small.stats()
    assert e.value.code == _lib.ERR_INVALID and str(s1["dropped"]) in str(e.value)
    assert s3["unmatched"] == s1["dropped"] and s3["removed"] == s1["points"] and s3["points"] == 0 and s3["vacant"] == 64
    assert len(small.extract()[2]) == 0
    small.close()


# ---- 5. refusals and counters -----------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing_and_a_wrong_pose_is_reported():
    ctx, pyramids, poses = four(128, 96)
    capacity = capacity_for(pyramids, poses, 0, 0.05)
    m = d.KeyframeMap(ctx, 0.05, capacity)
    m.insert(pyramids, poses)
    names = ("map_inserts", "map_removes", "map_rehashes", "map_points", "map_dropped")
    s, before, c0 = m.stats(), m.extract(sort=True), [ctx.counter(k) for k in names]
    other = d.Context(0)
    foreign = camera(other, 128, 96, pyramids[0].camera.K, 3).create(*tcm.float_views(128, 96)[1][0][:2])
    foreign_map = d.KeyframeMap(other, 0.05, 1 << 10)
    handles = (C.c_void_p * 2)(pyramids[0].ptr, pyramids[1].ptr)
    mixed = (C.c_void_p * 2)(pyramids[0].ptr, foreign.ptr)
    nulled = (C.c_void_p * 2)(pyramids[0].ptr, None)
    T = np.ascontiguousarray(poses[:2], np.float64)
    tp = T.ctypes.data_as(C.POINTER(C.c_double))
    L = ctx._lib
    calls = []
    for f in (lambda *a: L.dvo_hip_map_remove(*a[:5], *a[6:]), L.dvo_hip_map_move):      # (remove has no second pose array)
        calls += [
            lambda f=f: f(ctx.ptr, m.ptr, 2, handles, tp, tp, 3, 0.0, INF),             # a level the frames do not have
            lambda f=f: f(ctx.ptr, m.ptr, 2, handles, tp, tp, -1, 0.0, INF),
            lambda f=f: f(ctx.ptr, m.ptr, 2, handles, None, tp, 0, 0.0, INF),           # a null pose
            lambda f=f: f(ctx.ptr, m.ptr, 2, mixed, tp, tp, 0, 0.0, INF),               # a frame of another context
            lambda f=f: f(ctx.ptr, m.ptr, 2, nulled, tp, tp, 0, 0.0, INF),
            lambda f=f: f(ctx.ptr, m.ptr, 0, handles, tp, tp, 0, 0.0, INF),
            lambda f=f: f(ctx.ptr, m.ptr, 2, handles, tp, tp, 0, 2.0, 1.0),             # a bad range
            lambda f=f: f(ctx.ptr, m.ptr, 2, handles, tp, tp, 0, float("nan"), 1.0),
            lambda f=f: f(ctx.ptr, None, 2, handles, tp, tp, 0, 0.0, INF),
            lambda f=f: f(ctx.ptr, foreign_map.ptr, 2, handles, tp, tp, 0, 0.0, INF),   # a map of another context
        ]
    calls += [lambda: L.dvo_hip_map_move(ctx.ptr, m.ptr, 2, handles, tp, None, 0, 0.0, INF),
              lambda: L.dvo_hip_map_rehash(ctx.ptr, None, 0), lambda: L.dvo_hip_map_rehash(ctx.ptr, foreign_map.ptr, 0),
              lambda: L.dvo_hip_map_rehash(ctx.ptr, m.ptr, 100)]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
    assert [ctx.counter(k) for k in names] == c0 and m.stats() == s
    assert_maps_identical(m.extract(sort=True), before, "after the refusals")
    with pytest.raises(ValueError):
        m.remove([foreign], np.eye(4)[None])                        # the Python wrapper refuses it first
    # a removal under a wrong pose: ERR_INVALID with the count; the map keeps what the call did
    wrong = poses[1] @ scenes.se3_exp([0.3, 0.2, -0.2, 0.0, 0.1, 0.0])
    with pytest.raises(d.DvoHipError) as e:
        m.remove(pyramids[1:2], wrong[None])
    s1 = m.stats()
    assert e.value.code == _lib.ERR_INVALID and s1["unmatched"] > 0 and str(s1["unmatched"]) in str(e.value)
    one = yardstick(pyramids[1:2], poses[1:2], 0, 0.05, 1 << 16).stats()["points"]
    assert s1["points"] == s["points"] - s1["removed"] and s1["removed"] + s1["unmatched"] == one
    # (a point that meets a foreign voxel under the wrong pose is subtracted from it: what such a map extracts is not checked here)
    assert [ctx.counter(k) - a for k, a in zip(names, c0)] == [0, 1, 0, 0, 0]
    # counters of a remove, a move and a rehash that succeed
    m.clear()
    m.insert(pyramids, poses)
    c1 = [ctx.counter(k) for k in names]
    m.remove(pyramids[:2], poses[:2])
    m.move(pyramids[2:], poses[2:], np.stack([poses[2], poses[3] @ scenes.se3_exp(TWIST)]))      # one of the two stays
    m.rehash()
    taken = m.stats()
    assert [ctx.counter(k) - a for k, a in zip(names, c1)][:3] == [1, 3, 1] and ctx.counter("map_dropped") == c1[4]
    assert taken["removed"] > 0 and ctx.counter("map_points") - c1[3] == taken["points"] + taken["removed"] - s["points"]
    for x in (m, foreign_map):
        x.close()
    del foreign
    other.close()


# ---- 6. the C++ facade ------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_incremental_aggregator_equals_the_rebuild():
    exe = tmu.build_map_update_facade_check()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.bin")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, np.float32).reshape(-1, 4)
    # the cloud after "remove kf1, re-pose kf2" against KeyframeMap fed the keyframes that remain under the poses they have
    ctx = d.default_context()
    cam = camera(ctx, 64, 48, np.array([60.0, 60.0, 31.5, 23.5], np.float32), 1)
    pyramids, poses = [], []
    for k in (0, 2, 3, 4):
        I, Z, T = facade_frame(k)
        if k == 2:
            T[0, 3] += 0.013
            T[1, 2], T[2, 1] = 3.0 / 1024.0, -3.0 / 1024.0
        pyramids.append(cam.create(I, Z))
        poses.append(T)
    m = d.KeyframeMap(ctx, 0.01, 1 << 18)
    m.insert(pyramids, np.stack(poses))
    xyzi = m.extract(sort=True)[0]
    assert len(xyzi) > 1000 and got.shape == xyzi.shape and np.array_equal(got.view(np.uint32), xyzi.view(np.uint32))
    m.close()
