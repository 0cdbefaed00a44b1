"""Keyframe covisibility on the device (include/dvo_hip.h, dvo_hip_frames_covisibility; dvo_slam_amd/csrc/covisibility.hip).

The yardstick is covisibility_host() of tests/test_covisibility.py -- covisibility.h compiled for the host -- fed the planes the device
holds at the level (planes_of): the records are integers and must be EQUAL, whatever the order the workgroups add in.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import scenes
import test_covisibility as tcv
import test_frame_warp as tfw
from dvo_slam_amd import _lib
from test_covisibility import FIELDS, as_dict, covisibility_host, holds_invariant
from test_gpu_cloud_map import planes_of
from test_gpu_f32_ingest import blank_frames, camera
from test_gpu_frame_warp import facade_frame, frames_of

pytestmark = pytest.mark.gpu
INF = float("inf")
GRID_ROWS = 1024                    # covisibility.hip, covis_grid: the pairs beyond that many are walked by the kernel
OTHER = dict(depth_tolerance=0.01, depth_tolerance_rel=0.02, min_depth=0.7, max_depth=2.5)
# a self pair, both directions of one pair, and frame 0 in six of the seven
PAIRS7 = np.array([(0, 0), (0, 1), (1, 0), (2, 0), (3, 0), (0, 4), (2, 3)])


def small_motions(n, scale=1.0):
    return np.stack([scenes.se3_exp(scale * np.array([0.02 * (k + 1), -0.015 * k, -0.03 * (k % 3), 0.02 * k, -0.015 * (k + 1), 0.01 * k]))
                     for k in range(n)])


class Planes:
    """the planes the device holds, downloaded once per (pyramid, level)"""
    def __init__(self):
        self.seen = {}

    def __call__(self, pyramid, level):
        key = (id(pyramid), level)
        if key not in self.seen:
            self.seen[key] = planes_of(pyramid, level)
        return self.seen[key]


def want_records(planes, pyramids, pairs, T, level, **kw):
    out = np.zeros(len(pairs), d.COVIS_DTYPE)
    for k, (a, b) in enumerate(pairs):
        (Ia, Za, Ka), (Ib, Zb, Kb) = planes(pyramids[a], level), planes(pyramids[b], level)
        out[k] = covisibility_host(Ia, Za, Ib, Zb, Ka, Kb, T[k], **kw)
    return out


def as_records(got, device):
    if not device:
        assert got.dtype == d.COVIS_DTYPE
        return got
    assert got.dtype == torch.uint8 and got.shape[1] == 32 and got.is_cuda
    return got.cpu().numpy().view(d.COVIS_DTYPE).reshape(-1)


def host_batch_of(planes):
    """covisibility_batch with the host build in the device call's place, over the planes the device holds"""
    def batch(pyramids, pairs, transforms, level=2, **kw):
        P, T = d.tracker._covis_args(pyramids, pairs, transforms, level, "host_batch")
        return want_records(planes, pyramids, P, T, level, **kw)
    return batch


# ---- 1. records equal the host build ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(64, 48), (128, 96)])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_records_equal_the_host_build(shape, level):
    """level 2 of 64 x 48 is 16 x 12: narrower than a wavefront, and 192 pixels are no multiple of 256"""
    w, h = shape
    ctx, pyramids, _ = frames_of(w, h)
    planes = Planes()
    T = small_motions(7)
    T[0] = np.eye(4)                                                   # the self pair under the identity
    T[2] = np.linalg.inv(T[1])                                         # (1, 0) is (0, 1) backwards
    pixels = (w >> level) * (h >> level)
    for pairs, M in ((PAIRS7[1:2], T[1:2]), (PAIRS7, T)):
        for kw in (dict(), OTHER):
            want = want_records(planes, pyramids, pairs, M, level, **kw)
            for device in (False, True):
                got = as_records(d.covisibility_batch(pyramids, pairs, M, level=level, device=device, **kw), device)
                assert got.shape == (len(pairs),)
                assert [as_dict(r) for r in got] == [as_dict(r) for r in want], (shape, level, len(pairs), kw, device)
            assert all(holds_invariant(r) for r in want)
    # not a comparison of empty records: the self pair sees itself entirely, the two directions of (0, 1) keep a third of the image in view
    base = want_records(planes, pyramids, PAIRS7[:3], T[:3], level)
    assert base[0]["valid"] == base[0]["consistent"] == base[0]["in_view"] > 0.3 * pixels and base[0]["photo"] == 0
    assert base[1]["in_view"] > 0.3 * pixels and base[2]["in_view"] > 0.3 * pixels
    assert as_dict(base[1]) != as_dict(want_records(planes, pyramids, PAIRS7[1:2], T[1:2], level, **OTHER)[0])


# ---- 2. more pairs than the grid is high ------------------------------------------------------------------------------------------------

def test_more_pairs_than_the_grid_is_high():
    """1030 pairs of 16 x 12 (level 2 of 64 x 48) over five frames, every pair under a transform of its own: the launch's grid has 1024
    rows, the kernel walks the rest; a pair index in the wrong place shows in the records.  (The pair table of 1030 pairs also goes
    past the ring of pinned upload slots, capi_covis.inc.)"""
    ctx, pyramids, _ = frames_of(64, 48)
    n, level = GRID_ROWS + 6, 2
    T = np.stack([scenes.se3_exp([0.0004 * k, -0.0002 * k, -0.0003 * k, 0.0002 * k, -0.0003 * k, 0.0001 * k]) for k in range(n)])
    pairs = np.array([(k % 5, (k + 2) % 5) for k in range(n)])
    got = d.covisibility_batch(pyramids, pairs, T, level=level)
    pick = list(range(8)) + list(range(n - 10, n))
    want = want_records(Planes(), pyramids, pairs[pick], T[pick], level)
    assert [as_dict(r) for r in got[pick]] == [as_dict(r) for r in want]
    assert all(holds_invariant(r) and r["valid"] > 0 for r in got)
    assert as_dict(got[n - 1]) != as_dict(got[n - 6])                  # (the same two frames under another transform: another record)


# ---- 3. two sizes and cameras in one call -----------------------------------------------------------------------------------------------

def test_frames_of_two_sizes_and_cameras_share_a_call():
    ctx, large, _ = frames_of(128, 96, 2)
    (K, ref, cur), = tfw.scene_pair("aniso", 5, 64, 48, 1)[0]
    cam = camera(ctx, 64, 48, K, 3)
    small = [cam.create(*ref), cam.create(*cur)]
    pyramids = [large[0], small[0], large[1], small[1]]
    pairs = np.array([(0, 2), (1, 3), (0, 1), (3, 2), (1, 1), (2, 0)])               # (0, 1) and (3, 2): a and b differ in size and camera
    T = small_motions(6, 0.5)
    planes = Planes()
    for level in (0, 1):
        want = want_records(planes, pyramids, pairs, T, level)
        for device in (False, True):
            got = as_records(d.covisibility_batch(pyramids, pairs, T, level=level, device=device), device)
            assert [as_dict(r) for r in got] == [as_dict(r) for r in want], (level, device)
        assert want[2]["in_view"] > 0 and want[3]["in_view"] > 0 and want[2]["valid"] > want[3]["valid"] > 0


# ---- 4. deferred ingests ----------------------------------------------------------------------------------------------------------------

def test_a_call_after_a_deferred_reingest_sees_the_new_planes():
    w, h = 64, 48
    ctx, pyramids, T = frames_of(w, h, 4)
    cam = pyramids[0].camera
    a, b = blank_frames(cam, 1)[0], blank_frames(cam, 1)[0]
    new = [planes_of(p, 0)[:2] for p in pyramids[2:4]]
    dev = [[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in pair] for pair in new]
    c0 = ctx.counter("deferred_ingests")
    d.update_f32_device_batch([a, b], [dev[0][0].data_ptr(), dev[1][0].data_ptr()], [dev[0][1].data_ptr(), dev[1][1].data_ptr()],
                              flags=_lib.INGEST_DEFER)
    pairs = np.array([(0, 1), (1, 0)])
    got = d.covisibility_batch([a, b], pairs, T[:2], level=1)
    assert ctx.counter("deferred_ingests") == c0 + 1                  # the recorded ingest (one call) was carried out, not dropped
    want = want_records(Planes(), pyramids[2:4], pairs, T[:2], 1)
    assert [as_dict(r) for r in got] == [as_dict(r) for r in want] and want[0]["in_view"] > 0


# ---- 5. the same records again, and the shared scratch ----------------------------------------------------------------------------------

def test_identical_calls_and_calls_after_a_render_and_a_warp_give_identical_records():
    w, h = 128, 96
    ctx, pyramids, T = frames_of(w, h, 3)
    M = small_motions(7)
    pairs = PAIRS7 % 3
    first = d.covisibility_batch(pyramids, pairs, M, level=1)
    assert np.array_equal(d.covisibility_batch(pyramids, pairs, M, level=1), first)
    K = planes_of(pyramids[0], 0)[2]
    m = d.KeyframeMap(ctx, 0.02, 1 << 17)
    m.insert(pyramids, np.stack([np.eye(4), T[0], T[1]]))
    view = m.render(K, w, h, np.stack([T[2], np.eye(4)]))             # the view table and the staging area are the call's scratch too
    fwd = d.warp_forward_batch(pyramids, T, level=0)
    assert np.array_equal(d.covisibility_batch(pyramids, pairs, M, level=1), first)
    assert tfw.same_bits(m.render(K, w, h, np.stack([T[2], np.eye(4)])), view)      # ... and the other way round
    assert tfw.same_bits([g[1] for g in d.warp_forward_batch(pyramids, T, level=0)], [g[1] for g in fwd])
    assert np.array_equal(as_records(d.covisibility_batch(pyramids, pairs, M, level=1, device=True), True), first)
    m.close()


# ---- 6. refusals and the counter --------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_the_counter_counts_pairs():
    w, h = 64, 48
    ctx, pyramids, transforms = frames_of(w, h, 3)
    L = ctx._lib
    other = d.Context(0)
    K = planes_of(pyramids[0], 0)[2]
    foreign = camera(other, w, h, K, 3).create(*planes_of(pyramids[0], 0)[:2])
    shallow = camera(ctx, w, h, K, 1).create(*planes_of(pyramids[0], 0)[:2])
    T = np.ascontiguousarray(transforms[:2], np.float64)
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tp = T.ctypes.data_as(dp)
    out = np.full(2, 7, d.COVIS_DTYPE)
    handles = lambda *p: (C.c_void_p * len(p))(*[x if x is None else x.ptr for x in p])      # noqa: E731
    fr = handles(*pyramids)
    ints = lambda *v: np.array(v, np.int32)                                                   # noqa: E731
    pa, pb = ints(0, 1), ints(1, 2)
    good = d.covis_params_struct()

    def params(**kw):
        p = d.covis_params_struct()
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return C.byref(p)

    def T_with(value, at):
        bad = T.copy()
        bad.reshape(-1)[at] = value
        return bad

    def call(ctx_=ctx.ptr, nf=3, f=fr, n=2, a=pa, b=pb, t=tp, level=0, p=C.byref(good), o=C.c_void_p(out.ctypes.data), dev=0):
        return L.dvo_hip_frames_covisibility(ctx_, nf, f, n, a if a is None else a.ctypes.data_as(i32p), b if b is None else b.ctypes.data_as(i32p),
                                             t, level, p, o, dev)

    bad_params = [dict(depth_tolerance=-0.01), dict(depth_tolerance=float("nan")), dict(depth_tolerance_rel=-0.5), dict(depth_tolerance_rel=float("nan")),
                  dict(min_depth=2.0, max_depth=1.0), dict(min_depth=float("nan")), dict(max_depth=float("nan")), dict(reserved=0), dict(reserved=3)]
    bad_T = [T_with(np.nan, 3), T_with(np.inf, 16 + 5), T_with(-np.inf, 11), T_with(np.nan, 31)]
    # too many pixels: 700 000 entries of 12 blocks each exceed 2^31 / 256 blocks; too many pairs: 2^22 + 1, refused before any is read
    crowd = (C.c_void_p * 700000)(*([pyramids[0].ptr] * 700000))
    legion = np.zeros((1 << 22) + 1, np.int32)
    c1 = ctx.counter("covisibility_pairs")
    calls = [lambda: call(ctx_=other.ptr), lambda: call(nf=0), lambda: call(nf=-1), lambda: call(n=0), lambda: call(n=-3), lambda: call(f=None),
             lambda: call(a=None), lambda: call(b=None), lambda: call(t=None), lambda: call(o=None),
             lambda: call(f=handles(pyramids[0], None, pyramids[2])), lambda: call(f=handles(pyramids[0], pyramids[1], foreign)),
             lambda: call(level=3), lambda: call(level=-1), lambda: call(level=1, f=handles(pyramids[0], shallow, pyramids[2])),
             lambda: call(a=ints(0, 3)), lambda: call(a=ints(-1, 1)), lambda: call(b=ints(3, 0)), lambda: call(b=ints(0, -2)),
             lambda: call(nf=2),                                                              # pair_b names frame 2 of two
             lambda: call(o=C.c_void_p(1 << 20 | 4), dev=1), lambda: call(o=C.c_void_p(1 << 20 | 2), dev=1),
             lambda: call(nf=700000, f=crowd), lambda: call(n=(1 << 22) + 1, a=legion, b=legion)]
    calls += [lambda b=b: call(p=params(**b)) for b in bad_params]
    calls += [lambda b=b: call(t=b.ctypes.data_as(dp)) for b in bad_T]
    for k, refused in enumerate(calls):
        assert refused() == _lib.ERR_INVALID, k
    assert all(np.all(out[k] == 7) for k in FIELDS) and ctx.counter("covisibility_pairs") == c1
    # the same call with nothing wrong
    want = want_records(Planes(), pyramids, [(0, 1), (1, 2)], T, 0)
    assert call() == 0 and ctx.counter("covisibility_pairs") == c1 + 2
    assert [as_dict(r) for r in out] == [as_dict(r) for r in want]
    out[...] = np.full(2, 7, d.COVIS_DTYPE)
    assert call(p=None, n=1) == 0 and ctx.counter("covisibility_pairs") == c1 + 3
    assert as_dict(out[0]) == as_dict(want[0]) and all(out[1][k] == 7 for k in FIELDS)      # one pair: the second record is not touched
    d.covisibility_batch(pyramids, PAIRS7 % 3, small_motions(7), level=2)
    assert ctx.counter("covisibility_pairs") == c1 + 10
    with pytest.raises(ValueError):
        d.covisibility_batch([foreign, pyramids[0]], [(0, 1)], T[:1])
    p = L.dvo_hip_covis_params_default()
    assert (p.depth_tolerance_rel, p.min_depth, p.max_depth, list(p.reserved)) == (0.0, 0.0, INF, [0] * 4) and p.depth_tolerance == np.float32(0.05)
    del foreign
    other.close()


# ---- 7. the matrix and the candidates ---------------------------------------------------------------------------------------------------

def test_matrix_and_candidates_equal_the_same_functions_over_the_host_build():
    ctx, pyramids, _ = frames_of(64, 48)
    T = small_motions(5, 2.0)
    T[3, 0, 3] += 30.0                                                 # keyframe 3 stands thirty metres aside: nothing of it in view
    batch = host_batch_of(Planes())
    for level in (1, 2):
        M = d.covisibility_matrix(pyramids, T, level=level)
        want = d.covisibility_matrix(pyramids, T, level=level, batch=batch)
        assert M.shape == (5, 5) and np.array_equal(M, want)
        assert all(M[k, k]["valid"] == M[k, k]["consistent"] > 0 for k in range(5))
    S = d.overlap(M, M.T)
    assert np.all(np.diag(S) == 1.0) and np.all(S[3, [0, 1, 2, 4]] == 0.0) and M[0, 1]["in_view"] > 0 and M[1, 0]["in_view"] > 0
    for query in (0, 3):
        for kw in (dict(max_distance=1.0), dict(max_distance=1.0, min_overlap=0.05), dict(max_distance=5.0, min_overlap=0.01, **OTHER)):
            got = d.loop_closure_candidates(pyramids, T, query, level=2, **kw)
            assert got.tolist() == d.loop_closure_candidates(pyramids, T, query, level=2, batch=batch, **kw).tolist(), (query, kw)
            assert "min_depth" in kw or got[0] == query               # (the query overlaps itself entirely)
    assert d.loop_closure_candidates(pyramids, T, 3, 1.0, level=2).tolist() == [3]
    assert set(d.loop_closure_candidates(pyramids, T, 0, 1.0, level=2).tolist()) == {0, 1, 2, 4}


# ---- 8. the C++ facade ------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_search_equals_the_python_wrappers():
    d.build()
    exe = tcv.build_covisibility_facade_check()
    w, h, level = 64, 48, 1
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "records.bin")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, d.COVIS_DTYPE)
    lines = dict(line.split(":") for line in out.stdout.strip().splitlines()[:-1])
    ctx = d.default_context()
    cam = camera(ctx, w, h, np.array([60.0, 60.0, 31.5, 23.5], np.float32), 3)
    pyramids = [cam.create(*facade_frame(k)) for k in range(5)]
    poses = np.stack([np.eye(4)] * 5)
    poses[:, :3, 3] = [(0.0, 0.0, 0.0), (0.0625, 0.0, 0.0), (0.125, 0.03125, 0.0), (4.0, 0.0, 0.0), (0.0, -0.0625, -0.25)]
    pairs = np.array([(0, 1), (1, 0), (0, 0), (2, 4), (4, 2), (3, 0)])
    a, b = pairs[:, 0], pairs[:, 1]
    want = d.covisibility_batch(pyramids, pairs, np.linalg.inv(poses[b]) @ poses[a], level=level)
    assert [as_dict(r) for r in got] == [as_dict(r) for r in want]
    assert [int(x) for x in lines["radius"].split()] == d.radius_set(poses, 0, 1.0).tolist() == [0, 1, 2, 4]
    assert [int(x) for x in lines["ranked"].split()] == d.loop_closure_candidates(pyramids, poses, 0, 1.0, min_overlap=np.float32(0.05), level=level).tolist()
