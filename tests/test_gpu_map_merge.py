"""GPU tier: keyframe sub-maps on the device (dvo_slam_amd/csrc/map_merge.hip: k_map_merge, k_map_export; C-ABI: dvo_hip_map_merge,
dvo_hip_map_move_submaps, dvo_hip_map_export, dvo_hip_map_merge_records, dvo_hip_map_info).  The yardstick is the host restatement of
tests/test_map_merge.py (MergeMap, compiled from dvo_slam_amd/csrc/cloud_map.h and cloud_colour.h without contraction): sorted raw
records, colour records and statistics are compared BIT FOR BIT.
  1. plain merge and subtract, posed merge and subtract, move_submaps against subtract-then-merge; grey and coloured;
  2. record arrays of 1, 63, 64, 65 and 257 records (the ragged last wavefront), from host and device memory, a dead record in the middle;
  3. three sources of 64, 256 and 1024 slots in one launch, one of them twice with opposite signs and different poses;
  4. end to end: sub-maps in anchor coordinates, a pose-graph optimisation, move_submaps; the render of the result;
  5. export and absorb: a fresh map, save / load, a second context, a merge of sub-maps built in two contexts;
  6. the 64-slot table and the refusals through the C-ABI;
  7. the C++ facade (tests/cpp/map_merge_facade_check.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import scenes
import test_gpu_map_colour as tgmc
import test_map_merge as tmm
from dvo_slam_amd import _lib
from test_gpu_cloud_map import frames_of, planes_of, yardstick
from test_gpu_f32_ingest import camera
from test_map_merge import COLOUR_RECORD, RECORD, MergeMap, assert_records_identical

pytestmark = pytest.mark.gpu
LEVEL, LEAF, SLOTS = 1, 0.02, 1 << 17                                # 64 x 48 pixels a keyframe; the tables stay at most a quarter full
STATS = ("points", "dropped", "out_of_range", "unusable", "over_limit", "occupied", "vacant", "removed", "unmatched")
POSES = [scenes.se3_exp(x) for x in ([0.31, -0.12, 0.07, 0.04, -0.09, 0.12], [-0.2, 0.05, 0.11, -0.03, 0.06, -0.08],
                                     [0.02, 0.4, -0.15, 0.1, 0.02, -0.05], [0.12, -0.3, 0.2, -0.07, -0.04, 0.09])]


def device_records(m):
    """(records, colour records or None) of a device map, sorted by key"""
    rec, tint = m.export()
    order = np.argsort(rec["key"], kind="stable")
    return rec[order], (None if tint is None else tint[order])


def check(m, want, what):
    """the device map m against the host restatement: records and statistics"""
    assert_records_identical(device_records(m), want.records(), what)
    s, ws = m.stats(), want.stats()
    for k in STATS:
        assert s[k] == ws[k], (what, k, s, ws)


def host_build(pyramids, poses, planes, leaf=LEAF, slots=SLOTS):
    """the host table of the keyframes' level under the poses (coloured where planes are given), as a MergeMap"""
    if planes is None:
        return MergeMap.of(yardstick(pyramids, poses, LEVEL, leaf, slots))
    return MergeMap.of(tgmc.yardstick(pyramids, poses, planes, LEVEL, leaf, slots))


def device_build(ctx, pyramids, poses, colour, leaf=LEAF, slots=SLOTS):
    m = d.KeyframeMap(ctx, leaf, slots, colour=colour)
    m.insert(pyramids, poses, level=LEVEL)
    return m


@functools.lru_cache(maxsize=None)
def world(colour):
    """Six keyframes in two groups of three, built once and left unchanged.  Per group g: `plain[g]` is its map under the world poses,
    `sub[g]` its sub-map in the coordinates of the group's first keyframe (insertion poses T_anchor^-1 T_i, leaf 0.03: another grid than
    the destination's), each as (device map, host restatement); `whole`: the host table of all six under the world poses."""
    ctx, pyramids, poses = frames_of(128, 96, 6)
    planes = tgmc.colour_of(pyramids) if colour else None
    w = dict(ctx=ctx, pyramids=pyramids, poses=poses, planes=planes, plain=[], sub=[], anchors=[])
    for g in (0, 1):
        ps, Ts = pyramids[3 * g:3 * g + 3], poses[3 * g:3 * g + 3]
        pl = None if planes is None else planes[3 * g:3 * g + 3]
        local = np.stack([np.linalg.inv(Ts[0]) @ T for T in Ts])
        w["anchors"].append(Ts[0])
        w["plain"].append((device_build(ctx, ps, Ts, colour), host_build(ps, Ts, pl)))
        w["sub"].append((device_build(ctx, ps, local, colour, leaf=0.03), host_build(ps, local, pl, leaf=0.03)))
    w["whole"] = host_build(pyramids, poses, planes)
    assert 4 * w["whole"].stats()["occupied"] <= SLOTS and w["whole"].stats()["dropped"] == 0
    return w


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [False, True])
def test_plain_merge_is_the_single_build_and_subtract_restores(colour):
    w = world(colour)
    (da, ha), (db, hb) = w["plain"]
    m, want = d.KeyframeMap(w["ctx"], LEAF, SLOTS, colour=colour), MergeMap(LEAF, SLOTS, colour)
    m.merge([da, db])
    want.merge(ha).merge(hb)
    check(m, want, "a + b")
    assert_records_identical(device_records(m), w["whole"].records(), "a + b against the single build")
    for k in ("points", "dropped", "out_of_range", "unusable", "over_limit"):
        assert m.stats()[k] == w["whole"].stats()[k], k
    if colour:
        whole = device_build(w["ctx"], w["pyramids"], w["poses"], True)
        tmm.assert_maps_identical(m.extract(sort=True), whole.extract(sort=True), "extraction")
        assert np.array_equal(m.extract(sort=True, colour=True)[3], whole.extract(sort=True, colour=True)[3])
        whole.close()
    m.subtract(db)
    check(m, want.subtract(hb), "a + b - b")
    assert_records_identical(device_records(m), ha.records(), "a + b - b against a")
    m.merge([da, db], signs=[-1, 1])                                 # both signs in one launch
    check(m, want.subtract(ha).merge(hb), "- a + b")
    m.close()


@pytest.mark.parametrize("colour", [False, True])
def test_posed_merge_subtract_and_move_submaps(colour):
    w = world(colour)
    (da, ha), (db, hb) = w["sub"]
    Ta, Tb = w["anchors"]
    Ta2 = Ta @ scenes.se3_exp([0.004, -0.003, 0.002, 0.001, -0.002, 0.0015])
    m, want = d.KeyframeMap(w["ctx"], LEAF, SLOTS, colour=colour), MergeMap(LEAF, SLOTS, colour)
    m.merge([da, db], poses=[Ta, Tb])
    want.merge(ha, pose=Ta).merge(hb, pose=Tb)
    check(m, want, "posed a + b")
    assert m.stats()["points"] == ha.stats()["points"] + hb.stats()["points"] > 5000
    before = m.stats()["updates"]
    m.move_submaps([da, db], [Ta, Tb], [Ta2, Tb])                    # b stays: left out of the launch
    want.subtract(ha, pose=Ta).merge(ha, pose=Ta2)
    check(m, want, "move_submaps against subtract, merge")
    assert m.stats()["updates"] - before == 2 * int(ha.live().sum())
    m.move_submaps([da, db], [Ta2, Tb], [Ta2, Tb])                   # nothing moves: nothing is launched
    assert m.stats()["updates"] - before == 2 * int(ha.live().sum())
    m.subtract([da], poses=[Ta2])
    check(m, want.subtract(ha, pose=Ta2), "posed a + b - a")
    only_b = MergeMap(LEAF, SLOTS, colour).merge(hb, pose=Tb)
    assert_records_identical(device_records(m), only_b.records(), "what is left is b under its pose")
    m.close()


# ---- 2. ragged record arrays ----------------------------------------------------------------------------------------------------------------

def to_device(a, words):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1, words).copy()).cuda()


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_record_arrays_with_a_ragged_last_wavefront(n, colour):
    w = world(colour)
    rec, tint = w["plain"][1][1].records()
    rec, tint = rec[100:100 + n].copy(), (None if tint is None else tint[100:100 + n].copy())
    assert len(rec) == n
    if n > 1:
        rec["n"][n // 2] = 0                                          # a record that is not live, in the middle
        rec["key"][n // 3] = tmm.EMPTY
    dead = 0 if n == 1 else 1 if n // 2 == n // 3 else 2
    for where in ("host", "device"):
        m, want = d.KeyframeMap(w["ctx"], LEAF, 1 << 10, colour=colour), MergeMap(LEAF, 1 << 10, colour)
        give = (lambda a, words: a) if where == "host" else to_device
        m.absorb(give(rec, 8), None if tint is None else give(tint, 4))
        check(m, want.absorb(rec, tint), "%s: plain" % where)
        assert m.stats()["occupied"] == n - dead
        m.absorb(give(rec, 8), None if tint is None else give(tint, 4), leaf=LEAF, pose=POSES[0])
        check(m, want.absorb(rec, tint, pose=POSES[0]), "%s: posed" % where)
        m.absorb(give(rec, 8), None if tint is None else give(tint, 4), sign=-1)
        check(m, want.absorb(rec, tint, sign=-1), "%s: plain out again" % where)
        m.close()


# ---- 3. several sources in one launch -----------------------------------------------------------------------------------------------------

def test_three_sources_of_different_sizes_and_one_of_them_twice():
    w = world(False)
    rec = w["plain"][0][1].records()[0]
    assert len(rec) > 1250
    parts = {64: rec[:20], 256: rec[500:560], 1024: rec[1000:1250]}   # (a 64-slot source: smaller than a workgroup)
    dev = {c: d.KeyframeMap(w["ctx"], LEAF, c) for c in parts}
    host = {c: MergeMap(LEAF, c) for c in parts}
    for c, r in parts.items():
        dev[c].absorb(r)
        host[c].absorb(r)
        check(dev[c], host[c], "source of %d slots" % c)
    m, want = d.KeyframeMap(w["ctx"], 0.025, 1 << 12), MergeMap(0.025, 1 << 12)
    m.merge([dev[256]], poses=[POSES[3]])
    want.merge(host[256], pose=POSES[3])
    # 256 leaves under the pose it has and enters under another, between the two others
    m.merge([dev[64], dev[256], dev[1024], dev[256]], signs=[1, -1, 1, 1], poses=[POSES[0], POSES[3], POSES[2], POSES[1]])
    want.merge(host[64], pose=POSES[0]).subtract(host[256], pose=POSES[3]).merge(host[1024], pose=POSES[2]).merge(host[256], pose=POSES[1])
    check(m, want, "four entries, one launch")
    assert m.stats()["points"] == sum(int(r["n"].sum()) for r in parts.values()) and m.stats()["unmatched"] == 0
    # ... and plain: sources of three capacities into a fourth
    p, pw = d.KeyframeMap(w["ctx"], LEAF, 1 << 11), MergeMap(LEAF, 1 << 11)
    p.merge([dev[1024], dev[64], dev[256], dev[64]])
    check(p, pw.merge(host[1024]).merge(host[64]).merge(host[256]).merge(host[64]), "plain, a source twice")
    for x in list(dev.values()) + [m, p]:
        x.close()


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------------

def test_submaps_follow_a_pose_graph_optimisation_and_render():
    w = world(False)
    ctx, truth = w["ctx"], w["poses"]
    (da, ha), (db, hb) = w["sub"]
    drifted = truth.copy()
    for k, xi in ((1, [0.02, -0.01, 0.015, 0.004, -0.003, 0.002]), (3, [-0.03, 0.02, 0.01, -0.002, 0.005, 0.003]), (4, [0.01, 0.01, -0.02, 0.003, 0.001, -0.004])):
        drifted[k] = truth[k] @ scenes.se3_exp(xi)
    m, want = d.KeyframeMap(ctx, LEAF, SLOTS), MergeMap(LEAF, SLOTS)
    m.merge([da, db], poses=[drifted[0], drifted[3]])                # the anchors are keyframes 0 and 3
    want.merge(ha, pose=drifted[0]).merge(hb, pose=drifted[3])
    graph = d.PoseGraph(ctx)
    graph.set_vertices(drifted, [True] + [False] * 5)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (0, 3), (1, 4)]
    graph.set_edges([a for a, _ in pairs], [b for _, b in pairs], [np.linalg.inv(truth[a]) @ truth[b] for a, b in pairs],
                    [np.diag([1e4] * 3 + [4e4] * 3)] * len(pairs))
    assert graph.optimize()["accepted"] >= 1
    new = graph.poses()
    graph.close()
    assert np.array_equal(new[0], drifted[0]) and not np.array_equal(new[3], drifted[3])
    m.move_submaps([da, db], [drifted[0], drifted[3]], [new[0], new[3]])
    want.subtract(hb, pose=drifted[3]).merge(hb, pose=new[3])
    check(m, want, "after the optimisation")
    # the render of the merged map is the render of the host-restated table, uploaded through absorb
    up = d.KeyframeMap(ctx, LEAF, SLOTS)
    up.absorb(want.slots)                                             # the raw table: empty and vacant slots among the records
    K, views = np.array([70.0, 70.0, 39.5, 29.5], np.float32), np.stack([new[0], new[4]])
    got, ref = m.render(K, 80, 60, views), up.render(K, 80, 60, views)
    for a, b in zip(got, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(got[1]).mean() > 0.05
    m.close()
    up.close()


# ---- 5. export and absorb -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [False, True])
def test_export_absorb_save_and_load_round_trips(colour):
    w = world(colour)
    src, host = w["plain"][0]
    sorted_extract = lambda m: m.extract(sort=True, colour=True) if colour else m.extract(sort=True)
    want = sorted_extract(src)
    rec, tint = src.export()
    assert rec.dtype == RECORD and len(rec) == int(host.live().sum()) and np.all(rec["pad"] == 0) and (tint is None) == (not colour)
    assert_records_identical(device_records(src), host.records(), "export")
    info = src.info()
    assert info == dict(leaf=float(np.float32(LEAF)), colour=colour, capacity=SLOTS)
    fresh = d.KeyframeMap(w["ctx"], LEAF, SLOTS, colour=colour)
    fresh.absorb(rec, tint)
    for a, b in zip(sorted_extract(fresh), want):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    # device to device, without the host
    drec, dtint = src.export(device=True)
    assert drec.is_cuda and drec.shape == (len(rec), 8)
    again = d.KeyframeMap(w["ctx"], LEAF, SLOTS * 2, colour=colour)
    again.absorb(drec, dtint)
    assert_records_identical(device_records(again), host.records(), "device records")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "map.npz")
        src.save(path)
        loaded = d.KeyframeMap.load(path, ctx=w["ctx"])
        assert loaded.info() == info
        assert_records_identical(device_records(loaded), host.records(), "save, load")
        loaded.close()
    # too small an array: the first max_records, and the capacity error
    got = C.c_size_t(0)
    few = np.zeros(10, RECORD)
    L, ctx = w["ctx"]._lib, w["ctx"]
    assert L.dvo_hip_map_export(ctx.ptr, src.ptr, 10, few.ctypes.data, None, 0, C.byref(got)) == _lib.ERR_CAPACITY and got.value == 10
    assert np.all(np.isin(few["key"], rec["key"])) and len(set(few["key"].tolist())) == 10
    fresh.close()
    again.close()


def test_submaps_built_in_two_contexts_merge_into_the_single_build():
    w = world(False)
    ctx2 = d.Context(w["ctx"].device)
    K = np.array(w["pyramids"][3].level(0).K, copy=True)
    cam2 = camera(ctx2, 128, 96, K, 3)
    theirs = [cam2.create(*planes_of(p, 0)[:2]) for p in w["pyramids"][3:]]
    other = device_build(ctx2, theirs, w["poses"][3:], False)
    rec, tint = other.export()                                        # to the host from one context ...
    assert_records_identical(device_records(other), w["plain"][1][1].records(), "the sub-map of the second context")
    m = d.KeyframeMap(w["ctx"], LEAF, SLOTS)
    with pytest.raises(ValueError):
        m.merge([other])                                              # (a map of another context is refused: records are the way)
    m.merge([w["plain"][0][0]])
    m.absorb(rec)                                                     # ... and into a map of the other
    assert_records_identical(device_records(m), w["whole"].records(), "two contexts")
    s, ws = m.stats(), w["whole"].stats()
    assert s["points"] == ws["points"] and s["dropped"] == 0 and s["over_limit"] == 0
    m.close()
    other.close()
    del theirs, cam2
    ctx2.close()


# ---- 6. capacity and refusals ---------------------------------------------------------------------------------------------------------------

def test_a_full_table_reports_and_refusals_change_nothing():
    w = world(False)
    ctx, L = w["ctx"], w["ctx"]._lib
    (da, ha), (db, hb) = w["plain"]
    small = d.KeyframeMap(ctx, LEAF, 64)
    with pytest.raises(d.DvoHipError) as e:
        small.merge([da])
    s = small.stats()
    assert e.value.code == _lib.ERR_CAPACITY and s["occupied"] == 64 and s["dropped"] > 0 and s["points"] + s["dropped"] == ha.stats()["points"]
    with pytest.raises(d.DvoHipError) as e:
        small.subtract([da])                                          # a map that has dropped points does not know what it holds
    assert e.value.code == _lib.ERR_INVALID and small.stats() == s
    small.close()

    m = d.KeyframeMap(ctx, LEAF, SLOTS)
    m.merge([da])
    coloured, other_leaf = d.KeyframeMap(ctx, LEAF, 64, colour=True), d.KeyframeMap(ctx, 0.03, 64)
    ctx2 = d.Context(ctx.device)
    foreign = d.KeyframeMap(ctx2, LEAF, 64)
    before, records = m.stats(), device_records(m)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    eye, nan = np.eye(4), np.eye(4)
    nan[0, 3] = np.nan
    maps = lambda *ms: (C.c_void_p * len(ms))(*[x.ptr if x is not None else None for x in ms])
    signs = lambda *s: (C.c_int * len(s))(*s)
    rec, tint = np.zeros(4, RECORD), np.zeros(4, COLOUR_RECORD)
    rec["key"], rec["n"] = [1, 2, 3, 4], 1
    merge = lambda dst, srcs, sg=None, T=None: L.dvo_hip_map_merge(ctx.ptr, dst.ptr, len(srcs), maps(*srcs), sg, None if T is None else T.ctypes.data_as(dp))
    absorb = lambda dst, n, r, c, leaf, sign, T=None: L.dvo_hip_map_merge_records(ctx.ptr, dst.ptr, n, r, c, 0, leaf, sign, None if T is None else T.ctypes.data_as(dp))
    refused = [
        merge(m, [m]), merge(m, [db, m]), merge(m, [None]), merge(m, [foreign]), merge(m, [coloured]), merge(coloured, [db]), merge(m, [other_leaf]),
        merge(m, [db], signs(0)), merge(m, [db], signs(2)), merge(m, [db], None, nan), merge(m, [db], signs(-1), nan),
        L.dvo_hip_map_merge(ctx.ptr, m.ptr, -1, maps(db), None, None), L.dvo_hip_map_merge(ctx.ptr, None, 1, maps(db), None, None),
        L.dvo_hip_map_merge(ctx.ptr, m.ptr, 1, None, None, None),
        L.dvo_hip_map_move_submaps(ctx.ptr, m.ptr, 1, maps(m), eye.ctypes.data_as(dp), eye.ctypes.data_as(dp)),
        L.dvo_hip_map_move_submaps(ctx.ptr, m.ptr, 1, maps(db), eye.ctypes.data_as(dp), nan.ctypes.data_as(dp)),
        L.dvo_hip_map_move_submaps(ctx.ptr, m.ptr, 1, maps(db), None, eye.ctypes.data_as(dp)),
        L.dvo_hip_map_move_submaps(ctx.ptr, m.ptr, 1, maps(coloured), eye.ctypes.data_as(dp), nan.ctypes.data_as(dp)),
        absorb(m, 4, rec.ctypes.data, tint.ctypes.data, LEAF, 1), absorb(coloured, 4, rec.ctypes.data, None, LEAF, 1), absorb(m, 4, rec.ctypes.data, None, 0.03, 1),
        absorb(m, 4, rec.ctypes.data, None, LEAF, 0), absorb(m, 4, rec.ctypes.data, None, LEAF, 1, nan), absorb(m, 4, None, None, LEAF, 1),
        absorb(m, (1 << 32) + 1, rec.ctypes.data, None, LEAF, 1), absorb(m, 4, rec.ctypes.data, None, float("nan"), 1, eye),
        L.dvo_hip_map_merge_records(ctx.ptr, m.ptr, 4, rec.ctypes.data + 8, None, 1, LEAF, 1, None),           # a device array off its alignment
        L.dvo_hip_map_export(ctx.ptr, m.ptr, 4, None, None, 0, C.byref(C.c_size_t())), L.dvo_hip_map_export(ctx.ptr, m.ptr, 4, rec.ctypes.data, None, 0, None),
        L.dvo_hip_map_export(ctx.ptr, m.ptr, 4, rec.ctypes.data, tint.ctypes.data, 0, C.byref(C.c_size_t())),  # colour records of a grey map
        L.dvo_hip_map_info(ctx.ptr, foreign.ptr, None, None, None),
    ]
    assert all(rc == _lib.ERR_INVALID for rc in refused), refused
    assert m.stats() == before and coloured.stats()["occupied"] == 0
    assert_records_identical(device_records(m), records, "after the refusals")
    # what is fine: nothing to do is no error; an unmatched subtraction is reported and counted
    assert merge(m, []) == _lib.OK and absorb(m, 0, None, None, LEAF, 1) == _lib.OK and m.stats() == before
    assert merge(m, [db], signs(-1)) == _lib.ERR_INVALID
    s = m.stats()
    assert s["unmatched"] > 0 and s["unmatched"] + s["removed"] == hb.stats()["points"]
    check(m, MergeMap(LEAF, SLOTS).merge(ha).subtract(hb), "a - b")
    for x in (m, coloured, other_leaf, foreign):
        x.close()
    ctx2.close()


# ---- 7. the C++ facade --------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_submaps():
    exe = tmm.build_map_merge_facade_check()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.bin")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, np.float32).reshape(-1, 4)
    assert len(got) > 1000 and np.all(np.isfinite(got))
