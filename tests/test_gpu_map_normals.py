"""GPU tier: surface normals in the keyframe map (include/dvo_hip.h, dvo_hip_frames_normals, DVO_HIP_MAP_NORMALS,
dvo_hip_map_extract_normals, dvo_hip_map_render_normals) against the CPU-tier yardstick of tests/test_map_normals.py -- the host build of
dvo_slam_amd/csrc/cloud_normal.h, fed the planes dvo_hip_frame_download_plane returns -- BIT FOR BIT, no tolerances:
  1. k_frame_normals: frames of 67 x 5 and 128 x 96 in one call, and 321 x 240, at every level they have, to the host and to the device;
  2. insert: the slots and both side tables through the sorted extraction at levels 0 and 1, with NORMALS alone and with COLOUR | NORMALS;
     the grey and colour extractions of such a map equal those of a map without the flag;
  3. the packed run sums at their worst: whole wavefronts folding into one voxel under poses that put a component at q = 1022, holes that
     make nn differ from n within a run, a 64-wide level;
  4. remove, move and rehash (one that fails included) carry the side table; a move with unchanged poses launches nothing;
  5. merge: plain, posed and move_submaps; export_ex to merge_records_ex round trips on host and device records; save / load; the
     sub-map refusals change nothing;
  6. normals views at 64 x 48 and 160 x 120 against the yardstick, Z against dvo_hip_map_render, holes included;
  7. every refusal changes nothing;
  8. the C++ facade's PointCloudAggregator with normals against KeyframeMap(normals=True)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import test_cloud_map as tcm
import test_gpu_cloud_map as tgcm
import test_map_colour as tmc
import test_map_normals as tmn
from dvo_slam_amd import _lib
from test_gpu_cloud_map import frames_of, planes_of
from test_gpu_f32_ingest import camera
from test_map_normals import NormalHostMap, assert_normal_maps_identical, frame_normals

pytestmark = pytest.mark.gpu
INF = float("inf")
HOLE = 0x7FC00000


def bits(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint32)


def colour_of(pyramids, seed=170):
    """random BGR colour attached to the pyramids in one call; returns their level-0 planes of packed pixels"""
    imgs = [tmc.random_image(p.camera.width, p.camera.height, 3, seed + k) for k, p in enumerate(pyramids)]
    d.set_colour_batch(pyramids, imgs, "bgr8")
    return [tmc.pack_plane(np.ascontiguousarray(img), "bgr8") for img in imgs]


def yardstick(pyramids, poses, level, leaf, capacity, planes=None, min_depth=0.0, max_depth=INF):
    m = NormalHostMap(leaf, capacity, colour=planes is not None)
    for k, (p, T) in enumerate(zip(pyramids, poses)):
        I, Z, K = planes_of(p, level)
        m.insert(I, Z, K, T, None if planes is None else planes[k], level=level, min_depth=min_depth, max_depth=max_depth)
    return m


def roomy(pyramids, poses, level, leaf, planes=None):
    """the yardstick in a table at least four times its voxels: the device cannot drop, its probe sequences are the yardstick's"""
    want = yardstick(pyramids, poses, level, leaf, 1 << 22, planes)
    capacity = 64
    while capacity < 4 * want.stats()["occupied"]:
        capacity *= 2
    want = yardstick(pyramids, poses, level, leaf, capacity, planes)
    assert want.stats()["dropped"] == 0 and want.grey_table().longest_run() < tcm.MAX_PROBES
    return want, capacity


def check_against(m, want, what):
    got = m.extract(sort=True, colour=want.colour is not None, normals=True)
    assert_normal_maps_identical(got, want.extract(), what)
    s, ws = m.stats(), want.stats()
    for k in ("occupied", "points", "dropped", "out_of_range", "unusable", "capacity", "removed", "unmatched"):
        assert s[k] == ws[k], (what, k, s, ws)
    assert s["over_limit"] == 0
    return got


# ---- 1. k_frame_normals ---------------------------------------------------------------------------------------------------------------------

def small_frame(ctx):
    """a 67 x 5 pyramid (levels 0 and 1) cut out of the 128 x 96 scene across a depth edge: wavefronts straddle its rows, and only three
    rows are interior"""
    K, views = tcm.float_views(128, 96)
    I, Z, T = views[0]
    Ks = np.array([K[0], K[1], 33.0, 2.0], np.float32)
    return camera(ctx, 67, 5, Ks, 2).create(np.ascontiguousarray(I[44:49, 30:97]), np.ascontiguousarray(Z[44:49, 30:97])), T


@pytest.mark.parametrize("device", [False, True])
def test_frame_normals_equal_the_yardstick(device):
    ctx, mid, mid_poses = frames_of(128, 96, 2)
    _, large, large_poses = frames_of(321, 240, 1)
    small, small_pose = small_frame(ctx)
    assert small.levels == 2 and mid[0].levels == 3 and large[0].levels == 3
    seen = 0
    for group, poses, levels in (([small, mid[0], mid[1]], np.stack([small_pose, mid_poses[0], mid_poses[1]]), (0, 1)),
                                 (mid, mid_poses, (2,)), (large, large_poses, (0, 1, 2))):
        for level in levels:
            for lo, hi in ((0.0, INF), (0.5, 5.0)):
                got = d.normals_batch(group, poses, level=level, min_depth=lo, max_depth=hi, device=device)
                if device:
                    torch.cuda.synchronize()
                    got = [g.cpu().numpy() for g in got]
                for p, T, g in zip(group, poses, got):
                    I, Z, K = planes_of(p, level)
                    want = frame_normals(Z, K, T, lo, hi)
                    assert g.shape == want.shape and np.array_equal(bits(g), bits(want)), (p.camera.width, level, lo, device)
                    has = want[..., 3] == 1.0
                    assert not has[0].any() and not has[-1].any() and not has[:, 0].any() and not has[:, -1].any()
                    seen += int(has.sum())
                    if level == 0 and Z.shape[0] > 20 and hi == INF:
                        assert has.sum() > has.size // 4 and (~has[1:-1, 1:-1]).sum() > 10     # normals, and holes and edges without
    assert seen > 20000
    # the 67 x 5 frame has normals in its three interior rows
    want = frame_normals(planes_of(small, 0)[1], planes_of(small, 0)[2], small_pose)
    assert (want[1:4, :, 3] == 1.0).sum() > 60


# ---- 2. insert ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("colour", [False, True])
def test_map_with_normals_equals_the_yardstick(colour, level):
    ctx, pyramids, poses = frames_of(128, 96, 3)
    planes = colour_of(pyramids) if colour else None
    want, capacity = roomy(pyramids, poses, level, 0.02, planes)
    m = d.KeyframeMap(ctx, 0.02, capacity, colour=colour, normals=True)
    assert m.info() == dict(leaf=float(np.float32(0.02)), colour=colour, normals=True, capacity=capacity)
    m.insert(pyramids, poses, level=level)
    got = check_against(m, want, (colour, level))
    nrm = got[-1]
    assert (got[1] > 1).sum() > 50 and (nrm[:, 3] > 0).sum() > 500 and (nrm[:, 3] == 0).sum() > 10
    # the grey and the colour extraction: what a map without the flag fed the same frames returns
    bare = d.KeyframeMap(ctx, 0.02, capacity, colour=colour)
    bare.insert(pyramids, poses, level=level)
    tcm.assert_maps_identical(m.extract(sort=True), bare.extract(sort=True), "grey extraction")
    if colour:
        tmc.assert_colour_maps_identical(m.extract(sort=True, colour=True), bare.extract(sort=True, colour=True), "colour extraction")
    assert m.stats() == bare.stats()
    # the device output, unsorted: the same records in some order
    out = m.extract(device=True, colour=colour, normals=True)
    torch.cuda.synchronize()
    host = [t.cpu().numpy() for t in out]
    order = np.argsort(host[2].view(np.uint64), kind="stable")
    dev = [host[0][order], host[1].view(np.uint32)[order], host[2].view(np.uint64)[order]] + [a[order] for a in host[3:]]
    if colour:
        dev[3] = dev[3].view(np.uint32)
    assert_normal_maps_identical(tuple(dev), got, "device")
    # frame by frame: the same map
    each = d.KeyframeMap(ctx, 0.02, capacity, colour=colour, normals=True)
    for p, T in zip(pyramids, poses):
        each.insert([p], T[None], level=level)
    assert_normal_maps_identical(each.extract(sort=True, colour=colour, normals=True), got, "frame by frame")
    for x in (m, bare, each):
        x.close()


def test_frames_of_different_sizes_share_an_insert():
    ctx, a, pa = frames_of(128, 96, 2)
    _, b, pb = frames_of(102, 78, 1)
    small, small_pose = small_frame(ctx)
    pyramids, poses = [a[0], small, b[0], a[1]], np.stack([pa[0], small_pose, pb[0], pa[1]])
    want, capacity = roomy(pyramids, poses, 0, 0.05)
    m = d.KeyframeMap(ctx, 0.05, capacity, normals=True)
    m.insert(pyramids, poses)
    check_against(m, want, "mixed sizes")
    m.close()


# ---- 3. the packed run sums at their worst --------------------------------------------------------------------------------------------------

TURNS = {"z": (np.diag([-1.0, 1.0, -1.0]), (2.0, 2.0, 5.0)),                                # the camera's (0, 0, -1) becomes (0, 0, +1)
         "x": (np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]), (5.0, 2.0, 2.0))}   # ... becomes (+1, 0, 0)


def plane_with_holes(w, h, holes):
    """a fronto-parallel plane at 2 m; holes "sparse": a NaN every seventh pixel of every third row, so that runs of valid lanes hold
    lanes with and without a normal (beside, above and below a hole)"""
    K = np.array([0.8 * w, 0.8 * w, w / 2 - 0.5, h / 2 - 0.5], np.float32)
    y, x = np.mgrid[0:h, 0:w]
    Z = np.full((h, w), 2.0, np.float32)
    if holes == "sparse":
        Z[(x % 7 == 3) & (y % 3 == 1)] = np.nan
    I = ((x * 3 + y * 7) % 256).astype(np.float32) + np.float32(0.25)
    ctx = d.default_context()
    return ctx, camera(ctx, w, h, K, 2).create(I, Z)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("holes", ["none", "sparse"])
@pytest.mark.parametrize("turn", ["z", "x"])
def test_whole_wavefronts_fold_into_one_voxel_at_the_largest_component(turn, holes, level):
    """128 x 96 and, at level 1, 64 x 48 -- a wavefront is exactly one row -- with leaf 4: every run of 64 lanes folds into one voxel,
    64 * 1022 = 65408 in a 16-bit field, one below a carry into the next"""
    ctx, p = plane_with_holes(128, 96, holes)
    R, t = TURNS[turn]
    T = tmn.pose_of(R, t)
    want, capacity = roomy([p], [T], level, 4.0)
    assert want.stats()["occupied"] == 1
    m = d.KeyframeMap(ctx, 4.0, capacity, normals=True)
    m.insert([p], T[None], level=level)
    got = check_against(m, want, (turn, holes, level))
    I, Z, K = planes_of(p, level)
    rec = frame_normals(Z, K, T)
    has = rec[..., 3] == 1.0
    assert np.all(rec[has][:, :3] == (R @ np.array([0.0, 0.0, -1.0])).astype(np.float32))   # every normal is the axis, q = 1022 in one component
    xyzi, counts, keys, nrm, nn = want.extract(with_nn=True)
    usable = int(np.isfinite(Z).sum())
    assert counts[0] == usable and nn[0] == has.sum() and 0 < nn[0] < counts[0]
    assert np.array_equal(got[3][0], np.append(R @ np.array([0.0, 0.0, -1.0]), 1.0).astype(np.float32))
    if holes == "none":
        assert m.stats()["updates"] <= usable // 32                 # runs were folded: far fewer updates than points
    else:
        assert (has[1:-1, 1:-1].sum() < np.isfinite(Z[1:-1, 1:-1]).sum()) or level == 1     # nn differs from n inside the runs
    m.remove([p], T[None], level=level)
    assert m.stats()["points"] == 0 and len(m.extract(normals=True)[2]) == 0
    m.insert([p], T[None], level=level)                             # the vacated slot holds zeros again: the same sums as at first
    assert_normal_maps_identical(m.extract(sort=True, normals=True), got, "inserted again")
    m.close()


# ---- 4. remove, move, rehash ----------------------------------------------------------------------------------------------------------------

VIEW_K = np.array([70.0, 70.0, 39.5, 29.5], np.float32)


def same_views(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("colour", [False, True])
def test_remove_move_and_rehash_carry_the_normals(colour):
    ctx, pyramids, poses = frames_of(128, 96, 3)
    planes = colour_of(pyramids) if colour else None
    kw = dict(colour=colour, normals=True)
    want_all, capacity = roomy(pyramids, poses, 0, 0.02, planes)
    m = d.KeyframeMap(ctx, 0.02, capacity, **kw)
    m.insert(pyramids, poses)
    everything = check_against(m, want_all, "three frames")
    # remove: the map that never held the frame
    m.remove(pyramids[1:2], poses[1:2])
    never = d.KeyframeMap(ctx, 0.02, capacity, **kw)
    never.insert([pyramids[0], pyramids[2]], poses[[0, 2]])
    two = never.extract(sort=True, **kw)
    assert_normal_maps_identical(m.extract(sort=True, **kw), two, "after remove")
    sub = None if planes is None else [planes[0], planes[2]]
    assert_normal_maps_identical(two, yardstick([pyramids[0], pyramids[2]], poses[[0, 2]], 0, 0.02, capacity, sub).extract(), "yardstick")
    views = poses[:2]
    assert same_views(m.render_normals(VIEW_K, 80, 60, views), never.render_normals(VIEW_K, 80, 60, views))
    s = m.stats()
    assert s["unmatched"] == 0 and s["vacant"] > 0 and len(two[2]) < len(everything[2])
    # a move with unchanged poses launches nothing
    before, moves = m.stats(), ctx.counter("map_inserts")
    m.move(pyramids[2:], poses[2:], poses[2:])
    assert m.stats() == before and ctx.counter("map_inserts") == moves
    # move = remove + insert
    new = poses[2] @ tcm.scenes.se3_exp([0.02, 0.01, -0.015, 0.01, 0.0, -0.01])
    m.move(pyramids[2:], poses[2:], new[None])
    never.remove(pyramids[2:], poses[2:])
    never.insert(pyramids[2:], new[None])
    moved = m.extract(sort=True, **kw)
    assert_normal_maps_identical(moved, never.extract(sort=True, **kw), "move")
    assert_normal_maps_identical(moved, yardstick([pyramids[0], pyramids[2]], [poses[0], new], 0, 0.02, capacity, sub).extract(), "move, yardstick")
    # rehash to a larger and to a smaller table keeps every record; the vacant slots go
    views_before = m.render_normals(VIEW_K, 80, 60, views)
    for cap in (capacity * 2, capacity // 2):
        m.rehash(cap)
        s = m.stats()
        assert s["capacity"] == cap and s["vacant"] == 0 and s["occupied"] == len(moved[2])
        assert_normal_maps_identical(m.extract(sort=True, **kw), moved, "rehash to %d" % cap)
        assert same_views(m.render_normals(VIEW_K, 80, 60, views), views_before)
    # ... and goes on working: the third frame back to where it was
    m.move(pyramids[2:], new[None], poses[2:])
    assert_normal_maps_identical(m.extract(sort=True, **kw), two, "after the rehashes")
    # a rehash that cannot fit leaves the map and its normals as they are
    stats = m.stats()
    with pytest.raises(d.DvoHipError) as err:
        m.rehash(64)
    assert err.value.code == _lib.ERR_CAPACITY and m.stats() == stats
    assert_normal_maps_identical(m.extract(sort=True, **kw), two, "after the failed rehash")
    m.clear()
    assert m.stats()["occupied"] == 0
    m.insert(pyramids[:1], poses[:1])
    first = None if planes is None else planes[:1]
    assert_normal_maps_identical(m.extract(sort=True, **kw), yardstick(pyramids[:1], poses[:1], 0, 0.02, capacity // 2, first).extract(), "after clear")
    for x in (m, never):
        x.close()


# ---- 5. merge -------------------------------------------------------------------------------------------------------------------------------

def sorted_records(rec):
    """what KeyframeMap.export() returned (host arrays, or device tensors of int32 words), sorted by key: NormalHostMap.records()'s order"""
    out = []
    for a, fields in zip(rec, (_lib.MAP_RECORD, _lib.MAP_COLOUR_RECORD, _lib.MAP_NORMAL_RECORD)):
        if a is not None and hasattr(a, "cpu"):
            a = np.ascontiguousarray(a.cpu().numpy()).view(np.dtype(fields)).reshape(-1)
        out.append(a)
    order = np.argsort(out[0]["key"], kind="stable")
    return [None if a is None else a[order] for a in out]


def assert_records_equal(got, want, what):
    for g, w in zip(sorted_records(got), want):
        assert (g is None and w is None) or np.array_equal(g, w), what


@pytest.mark.parametrize("colour", [False, True])
def test_plain_merge_of_sub_maps_equals_the_single_build(colour):
    ctx, pyramids, poses = frames_of(128, 96, 3)
    planes = colour_of(pyramids) if colour else None
    kw = dict(colour=colour, normals=True)
    want, capacity = roomy(pyramids, poses, 0, 0.02, planes)
    subs = []
    for k in range(3):
        sub = d.KeyframeMap(ctx, 0.02, capacity, **kw)
        sub.insert(pyramids[k:k + 1], poses[k:k + 1])
        subs.append(sub)
    dst = d.KeyframeMap(ctx, 0.02, capacity, **kw)
    dst.merge(subs)
    check_against(dst, want, "the sum of three sub-maps")
    assert_records_equal(dst.export(), want.records(), "export")
    # one leaves again: the map of the other two
    dst.subtract(subs[1])
    sub_planes = None if planes is None else [planes[0], planes[2]]
    two = yardstick([pyramids[0], pyramids[2]], poses[[0, 2]], 0, 0.02, capacity, sub_planes)
    assert_normal_maps_identical(dst.extract(sort=True, **kw), two.extract(), "after the subtraction")
    assert dst.stats()["unmatched"] == 0
    for x in subs + [dst]:
        x.close()


def test_posed_merge_subtraction_and_move_submaps_equal_the_yardstick():
    ctx, pyramids, poses = frames_of(128, 96, 3)
    eye = np.eye(4)
    # two sub-maps in their anchors' coordinates, a coarser leaf than the destination's
    subs, host_subs = [], []
    for k in (1, 2):
        sub = d.KeyframeMap(ctx, 0.03, 1 << 16, normals=True)
        sub.insert(pyramids[k:k + 1], eye[None])
        subs.append(sub)
        host_subs.append(yardstick(pyramids[k:k + 1], [eye], 0, 0.03, 1 << 16))
        assert_normal_maps_identical(sub.extract(sort=True, normals=True), host_subs[-1].extract(), "sub-map %d" % k)
    dst = d.KeyframeMap(ctx, 0.02, 1 << 17, normals=True)
    dst.insert(pyramids[:1], poses[:1])
    want = yardstick(pyramids[:1], poses[:1], 0, 0.02, 1 << 17)
    alone = want.extract()
    dst.merge(subs, poses=poses[1:])
    for h, T in zip(host_subs, poses[1:]):
        want.merge(h, pose=T)
    merged = check_against(dst, want, "posed merge")
    assert len(merged[2]) > len(alone[2]) and (merged[3][:, 3] > 0).sum() > (alone[3][:, 3] > 0).sum()
    # after a pose-graph optimisation: both sub-maps re-posed in one launch (one of them stays where it is)
    new = np.stack([poses[1] @ tcm.scenes.se3_exp([0.02, 0.01, -0.015, 0.01, 0.0, -0.01]), poses[2]])
    dst.move_submaps(subs, poses[1:], new)
    want.merge(host_subs[0], sign=-1, pose=poses[1]).merge(host_subs[0], pose=new[0])
    check_against(dst, want, "move_submaps")
    # the posed subtraction restores the destination
    dst.subtract(subs, poses=new)
    assert dst.stats()["unmatched"] == 0
    assert_normal_maps_identical(dst.extract(sort=True, normals=True), alone, "after the posed subtraction")
    for x in subs + [dst]:
        x.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("colour", [False, True])
def test_export_ex_merge_records_ex_save_and_load_round_trip(colour, device):
    ctx, pyramids, poses = frames_of(128, 96, 2)
    planes = colour_of(pyramids) if colour else None
    kw = dict(colour=colour, normals=True)
    want, capacity = roomy(pyramids, poses, 0, 0.02, planes)
    src = d.KeyframeMap(ctx, 0.02, capacity, **kw)
    src.insert(pyramids, poses)
    everything = src.extract(sort=True, **kw)
    rec = src.export(device=device)
    if device:
        torch.cuda.synchronize()
    assert len(rec) == 3 and (rec[1] is None) == (not colour)
    assert_records_equal(rec, want.records(), "export_ex")
    fresh = d.KeyframeMap(ctx, 0.02, capacity, **kw)
    fresh.absorb(rec[0], rec[1], normals=rec[2])
    assert_normal_maps_identical(fresh.extract(sort=True, **kw), everything, "absorbed")
    fresh.absorb(rec[0], rec[1], sign=-1, normals=rec[2])
    assert fresh.stats()["points"] == 0 and len(fresh.extract(**kw)[2]) == 0
    # a posed absorb equals the posed merge of the map itself
    T = tcm.scenes.se3_exp([0.1, -0.05, 0.02, 0.02, 0.3, -0.01])
    posed, posed_map = d.KeyframeMap(ctx, 0.025, capacity, **kw), d.KeyframeMap(ctx, 0.025, capacity, **kw)
    posed.absorb(rec[0], rec[1], leaf=0.02, pose=T, normals=rec[2])
    posed_map.merge([src], poses=T[None])
    assert_normal_maps_identical(posed.extract(sort=True, **kw), posed_map.extract(sort=True, **kw), "posed absorb")
    # the old export writes what it always wrote; the old merge_records cannot supply the normals and is refused
    L = ctx._lib
    n = len(everything[2])
    old = np.zeros(n, np.dtype(_lib.MAP_RECORD))
    got = C.c_size_t(0)
    assert L.dvo_hip_map_export(ctx.ptr, src.ptr, n, old.ctypes.data, None, 0, C.byref(got)) == _lib.OK and got.value == n
    assert np.array_equal(np.sort(old, order="key"), want.records()[0])
    before = fresh.stats()
    colour_rec = None if not colour else np.zeros(n, np.dtype(_lib.MAP_COLOUR_RECORD)).ctypes.data
    assert L.dvo_hip_map_merge_records(ctx.ptr, fresh.ptr, n, old.ctypes.data, colour_rec, 0, 0.02, 1, None) == _lib.ERR_INVALID
    assert b"normal" in L.dvo_hip_last_error(ctx.ptr) and fresh.stats() == before
    if not device:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "map.npz")
            src.save(path)
            loaded = d.KeyframeMap.load(path, ctx)
            assert loaded.info() == src.info() and loaded.info()["normals"]
            assert_normal_maps_identical(loaded.extract(sort=True, **kw), everything, "save, load")
            loaded.close()
            # a file of a map without normals loads as one
            bare = d.KeyframeMap(ctx, 0.02, capacity, colour=colour)
            bare.insert(pyramids, poses)
            bare.save(path)
            with np.load(path) as z:
                assert "normals" not in z.files
            loaded = d.KeyframeMap.load(path, ctx)
            assert "normals" not in loaded.info() and len(loaded.export()) == 2
            tcm.assert_maps_identical(loaded.extract(sort=True), everything, "a file without normals")
            for x in (loaded, bare):
                x.close()
    for x in (src, fresh, posed, posed_map):
        x.close()


def test_sub_map_refusals_change_nothing():
    ctx, pyramids, poses = frames_of(128, 96, 2)
    L = ctx._lib
    a, b, plain = d.KeyframeMap(ctx, 0.05, 1 << 16, normals=True), d.KeyframeMap(ctx, 0.05, 1 << 16, normals=True), d.KeyframeMap(ctx, 0.05, 1 << 16)
    a.insert(pyramids[:1], poses[:1])
    b.insert(pyramids[1:], poses[1:])
    plain.insert(pyramids[1:], poses[1:])
    before = [x.stats() for x in (a, b, plain)]
    records = a.extract(sort=True, normals=True)
    plain_records = plain.extract(sort=True)
    eye = np.ascontiguousarray(np.eye(4)[None], np.float64)
    ep = eye.ctypes.data_as(C.POINTER(C.c_double))
    rec = np.zeros(4, np.dtype(_lib.MAP_RECORD))
    rec["key"], rec["n"] = 5, 1
    nrec = np.zeros(4, np.dtype(_lib.MAP_NORMAL_RECORD))
    out, nout = np.full(64, 7, np.dtype(_lib.MAP_RECORD)), np.full(64, 7, np.dtype(_lib.MAP_NORMAL_RECORD))
    got = C.c_size_t(99)
    dev = torch.zeros(64 * 12 + 4, dtype=torch.int32, device="cuda:%d" % ctx.device)
    one = lambda m: (C.c_void_p * 1)(m.ptr)
    calls = [
        lambda: L.dvo_hip_map_merge(ctx.ptr, a.ptr, 1, one(plain), None, None),                      # with normals against without
        lambda: L.dvo_hip_map_merge(ctx.ptr, plain.ptr, 1, one(b), None, None),
        lambda: L.dvo_hip_map_merge(ctx.ptr, plain.ptr, 1, one(b), None, ep),
        lambda: L.dvo_hip_map_move_submaps(ctx.ptr, plain.ptr, 1, one(b), ep, ep),
        lambda: L.dvo_hip_map_move_submaps(ctx.ptr, a.ptr, 1, one(plain), ep, ep),
        lambda: L.dvo_hip_map_export_ex(ctx.ptr, plain.ptr, 64, out.ctypes.data, None, nout.ctypes.data, 0, C.byref(got)),   # no normals to export
        lambda: L.dvo_hip_map_export_ex(ctx.ptr, a.ptr, 64, dev.data_ptr(), None, dev.data_ptr() + 64 * 32 + 4, 1, C.byref(got)),   # unaligned
        lambda: L.dvo_hip_map_export_ex(ctx.ptr, a.ptr, 64, None, None, nout.ctypes.data, 0, C.byref(got)),
        lambda: L.dvo_hip_map_merge_records(ctx.ptr, a.ptr, 4, rec.ctypes.data, None, 0, 0.05, 1, None),     # cannot supply the normals
        lambda: L.dvo_hip_map_merge_records_ex(ctx.ptr, a.ptr, 4, rec.ctypes.data, None, None, 0, 0.05, 1, None),
        lambda: L.dvo_hip_map_merge_records_ex(ctx.ptr, plain.ptr, 4, rec.ctypes.data, None, nrec.ctypes.data, 0, 0.05, 1, None),
        lambda: L.dvo_hip_map_merge_records_ex(ctx.ptr, a.ptr, 4, rec.ctypes.data, None, nrec.ctypes.data, 0, 0.05, 2, None),
        lambda: L.dvo_hip_map_merge_records_ex(ctx.ptr, a.ptr, 4, rec.ctypes.data, None, nrec.ctypes.data, 0, 0.06, 1, None),   # plain: the leaf differs
        lambda: L.dvo_hip_map_merge_records_ex(ctx.ptr, a.ptr, 4, dev.data_ptr(), None, dev.data_ptr() + 4 * 32 + 4, 1, 0.05, 1, None),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
        assert L.dvo_hip_last_error(ctx.ptr), k
    torch.cuda.synchronize()
    assert [x.stats() for x in (a, b, plain)] == before and got.value == 99
    assert np.all(out["key"] == 7) and np.all(nout["nn"] == 7) and int(dev.abs().sum().item()) == 0
    assert_normal_maps_identical(a.extract(sort=True, normals=True), records, "after the refusals")
    tcm.assert_maps_identical(plain.extract(sort=True), plain_records, "the map without normals")
    for call in (lambda: a.merge([plain]), lambda: plain.merge([b]), lambda: a.absorb(rec), lambda: plain.absorb(rec, normals=nrec)):
        with pytest.raises(ValueError):
            call()
    for x in (a, b, plain):
        x.close()


# ---- 6. normals views -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [{}, dict(max_splat=1)])
@pytest.mark.parametrize("w,h", [(64, 48), (160, 120)])
def test_normals_views_equal_the_yardstick(w, h, params):
    ctx, pyramids, poses = frames_of(128, 96, 2)
    want, capacity = roomy(pyramids, poses, 0, 0.02)
    m = d.KeyframeMap(ctx, 0.02, capacity, normals=True)
    m.insert(pyramids, poses)
    Kv = np.array([0.9 * w, 0.9 * w, w / 2 - 0.5, h / 2 - 0.5], np.float32)
    views = np.stack([poses[0], poses[1] @ tcm.scenes.se3_exp([0.05, 0.0, -0.1, 0.0, 0.03, 0.0])])
    nrm, Z = m.render_normals(Kv, w, h, views, **params)
    want_nrm, want_Z = want.render(Kv, w, h, views, **params)
    assert nrm.dtype == np.float32 and nrm.shape == (2, h, w, 4) and Z.shape == (2, h, w)
    assert np.array_equal(bits(nrm), bits(want_nrm)) and np.array_equal(bits(Z), bits(want_Z))
    I_grey, Z_grey = m.render(Kv, w, h, views, **params)
    assert np.array_equal(bits(Z), bits(Z_grey))                    # bit for bit the grey view's depth
    hole = bits(Z) == HOLE
    assert hole.any() and (~hole).sum() > w * h // 4
    assert np.all(nrm[hole] == 0.0) and (nrm[..., 3] == 1.0).sum() > w * h // 8
    dev_nrm, dev_Z = m.render_normals(Kv, w, h, views, device=True, **params)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dev_nrm.cpu().numpy()), bits(nrm)) and np.array_equal(bits(dev_Z.cpu().numpy()), bits(Z))
    m.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing():
    ctx, pyramids, poses = frames_of(128, 96, 2)
    L = ctx._lib
    with_normals, plain = d.KeyframeMap(ctx, 0.05, 1 << 16, normals=True), d.KeyframeMap(ctx, 0.05, 1 << 16)
    with_normals.insert(pyramids, poses)
    plain.insert(pyramids, poses)
    before_n, before_p = with_normals.stats(), plain.stats()
    counters = {k: ctx.counter(k) for k in ("map_inserts", "map_points", "map_renders")}
    records = with_normals.extract(sort=True, normals=True)
    T = np.ascontiguousarray(poses, np.float64)
    tp = T.ctypes.data_as(C.POINTER(C.c_double))
    handles = (C.c_void_p * 2)(*[p.ptr for p in pyramids])
    xyzi, nrm, rgba, got = np.full((8, 4), -7.0, np.float32), np.full((8, 4), -7.0, np.float32), np.full(8, 7, np.uint32), C.c_size_t(99)
    plane_n, plane_z = np.full((60, 80, 4), -7.0, np.float32), np.full((60, 80), -7.0, np.float32)
    K = np.ascontiguousarray(VIEW_K)
    kp = K.ctypes.data_as(C.POINTER(C.c_float))
    outs_n, outs_z = (C.c_void_p * 1)(plane_n.ctypes.data), (C.c_void_p * 1)(plane_z.ctypes.data)
    frames_out = [np.full((96, 128, 4), -7.0, np.float32) for _ in range(2)]
    fo = (C.c_void_p * 2)(*[a.ctypes.data for a in frames_out])
    dev = torch.zeros(96 * 128 * 4 * 2 + 4, dtype=torch.float32, device="cuda:%d" % ctx.device)
    unaligned = (C.c_void_p * 2)(dev.data_ptr() + 4, dev.data_ptr() + 96 * 128 * 16)
    params = _lib.RenderParams()
    L.dvo_hip_render_params_default.restype = _lib.RenderParams
    params = L.dvo_hip_render_params_default()
    params.reserved[0] = 1
    calls = [
        lambda: L.dvo_hip_map_extract_normals(ctx.ptr, plain.ptr, 8, xyzi.ctypes.data, nrm.ctypes.data, None, None, None, 0, C.byref(got)),
        lambda: L.dvo_hip_map_extract_normals(ctx.ptr, with_normals.ptr, 8, xyzi.ctypes.data, None, None, None, None, 0, C.byref(got)),
        lambda: L.dvo_hip_map_extract_normals(ctx.ptr, with_normals.ptr, 8, xyzi.ctypes.data, nrm.ctypes.data, rgba.ctypes.data, None, None, 0, C.byref(got)),
        lambda: L.dvo_hip_map_extract_normals(ctx.ptr, with_normals.ptr, 8, xyzi.ctypes.data, nrm.ctypes.data, None, None, None, 0, None),
        lambda: L.dvo_hip_map_extract_normals(ctx.ptr, with_normals.ptr, 8, dev.data_ptr(), dev.data_ptr() + 4, None, None, None, 1, C.byref(got)),
        lambda: L.dvo_hip_map_render_normals(ctx.ptr, plain.ptr, 1, 80, 60, kp, tp, None, outs_n, outs_z, 0),
        lambda: L.dvo_hip_map_render_normals(ctx.ptr, with_normals.ptr, 1, 80, 60, kp, tp, None, None, outs_z, 0),
        lambda: L.dvo_hip_map_render_normals(ctx.ptr, with_normals.ptr, 1, 80, 60, kp, tp, None, outs_n, None, 0),
        lambda: L.dvo_hip_map_render_normals(ctx.ptr, with_normals.ptr, 1, 80, 60, kp, tp, None, (C.c_void_p * 1)(None), outs_z, 0),
        lambda: L.dvo_hip_map_render_normals(ctx.ptr, with_normals.ptr, 1, 80, 60, kp, tp, C.byref(params), outs_n, outs_z, 0),
        lambda: L.dvo_hip_map_render_normals(ctx.ptr, with_normals.ptr, 1, 80, 0, kp, tp, None, outs_n, outs_z, 0),
        lambda: L.dvo_hip_map_render_normals(ctx.ptr, with_normals.ptr, 1, 80, 60, kp, tp, None, (C.c_void_p * 1)(dev.data_ptr() + 4), (C.c_void_p * 1)(dev.data_ptr()), 1),
        lambda: L.dvo_hip_frames_normals(ctx.ptr, 2, handles, tp, 0, 0.0, INF, None, 0),
        lambda: L.dvo_hip_frames_normals(ctx.ptr, 2, handles, tp, 0, 0.0, INF, (C.c_void_p * 2)(frames_out[0].ctypes.data, None), 0),
        lambda: L.dvo_hip_frames_normals(ctx.ptr, 2, handles, tp, 0, 0.0, INF, unaligned, 1),
        lambda: L.dvo_hip_frames_normals(ctx.ptr, 2, handles, tp, 3, 0.0, INF, fo, 0),
        lambda: L.dvo_hip_frames_normals(ctx.ptr, 2, handles, tp, 0, 2.0, 1.0, fo, 0),
        lambda: L.dvo_hip_frames_normals(ctx.ptr, 2, handles, None, 0, 0.0, INF, fo, 0),
        lambda: L.dvo_hip_frames_normals(ctx.ptr, 0, handles, tp, 0, 0.0, INF, fo, 0),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
        assert L.dvo_hip_last_error(ctx.ptr), k
    torch.cuda.synchronize()
    ptr = C.c_void_p()
    for flags in (2, 6, 8):
        assert L.dvo_hip_map_create_ex(ctx.ptr, 0.05, 1024, flags, C.byref(ptr)) == _lib.ERR_INVALID and not ptr.value   # 2 stays an unknown flag
        assert b"unknown flag" in L.dvo_hip_last_error(ctx.ptr)
    assert with_normals.stats() == before_n and plain.stats() == before_p
    assert {k: ctx.counter(k) for k in counters} == counters
    assert got.value == 99 and np.all(xyzi == -7.0) and np.all(nrm == -7.0) and np.all(rgba == 7) and np.all(plane_n == -7.0) and np.all(plane_z == -7.0)
    assert all(np.all(a == -7.0) for a in frames_out) and float(dev.abs().sum().item()) == 0.0
    assert_normal_maps_identical(with_normals.extract(sort=True, normals=True), records, "after the refusals")
    with pytest.raises(ValueError):
        plain.extract(normals=True)
    with pytest.raises(ValueError):
        plain.render_normals(VIEW_K, 80, 60, poses[:1])
    # a frame of another context
    other = d.Context(0)
    foreign = camera(other, 128, 96, pyramids[0].camera.K, 3).create(*tcm.float_views(128, 96)[1][0][:2])
    assert L.dvo_hip_frames_normals(ctx.ptr, 1, (C.c_void_p * 1)(foreign.ptr), tp, 0, 0.0, INF, fo, 0) == _lib.ERR_INVALID
    assert L.dvo_hip_map_extract_normals(other.ptr, with_normals.ptr, 8, xyzi.ctypes.data, nrm.ctypes.data, None, None, None, 0, C.byref(got)) == _lib.ERR_INVALID
    assert all(np.all(a == -7.0) for a in frames_out) and np.all(nrm == -7.0)
    for x in (with_normals, plain):
        x.close()
    del foreign
    other.close()


# ---- 8. the C++ facade ----------------------------------------------------------------------------------------------------------------------

def facade_normals_frame(k, w=64, h=48):
    """keyframe k of tests/cpp/map_normals_facade_check.cpp: integer-valued formulas, exact in float32 on both sides"""
    y, x = np.mgrid[0:h, 0:w]
    I = ((x * 7 + y * 13 + k * 5) % 256).astype(np.float32)
    Z = (1000 + 4 * x + 2 * y + k).astype(np.float32) * np.float32(0.001)
    Z[(x + 2 * y + k) % 29 == 0] = np.nan
    T = np.eye(4)
    T[0, 2], T[2, 0] = k / 1024.0, -k / 1024.0
    T[:3, 3] = [0.01 * k, -0.005 * k, 0.002 * k]
    return I, Z, T


def test_cpp_facade_aggregator_with_normals_equals_keyframe_map():
    d.build()
    exe = tmn.build_map_normals_facade_check()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.bin")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        cloud = np.fromfile(path, np.float32).reshape(-1, 8)
    ctx = d.default_context()
    cam = camera(ctx, 64, 48, np.array([60.0, 60.0, 31.5, 23.5], np.float32), 1)
    pyramids, poses = [], []
    for k in range(3):
        I, Z, T = facade_normals_frame(k)
        pyramids.append(cam.create(I, Z))
        poses.append(T)
    m = d.KeyframeMap(ctx, 0.01, 1 << 20, normals=True)
    m.insert(pyramids, np.stack(poses))
    xyzi, counts, keys, nrm = m.extract(sort=True, normals=True)
    assert len(keys) == len(cloud) > 1000 and (nrm[:, 3] > 0).sum() > len(keys) // 2
    assert np.array_equal(bits(cloud[:, :4]), bits(xyzi)) and np.array_equal(bits(cloud[:, 4:]), bits(nrm))
    m.close()
