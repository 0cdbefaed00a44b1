"""GPU tier: colour in the keyframe map on the device (include/dvo_hip.h, dvo_hip_frames_set_colour, dvo_hip_frame_download_colour,
dvo_hip_map_create_ex, dvo_hip_map_extract_colour, dvo_hip_map_render_colour; k_colour_pack, k_colour_level and the COLOUR instantiations
of k_map_insert, k_map_render and k_render_resolve).  The yardstick is the host build of dvo_slam_amd/csrc/cloud_colour.h with cloud_map.h
and map_render.h (tests/test_map_colour.py: pack_plane, level_colour, ColourHostMap), fed the planes dvo_hip_frame_download_plane
returns: the device results equal it BIT FOR BIT, there are no tolerances -- every accumulation is an integer atomic.
  1. k_colour_pack and k_colour_level: frames of 67 x 5 and 128 x 96 in one call, and 321 x 240; the four formats, tight and padded
     pitch, host and device sources; the colour planes of levels 0, 1 and 2 (of the 67 x 5 frame: 0 and 1, all that a height of 5
     admits -- dvo_hip_frame_create refuses a level below two pixels a side -- and level 2 refused);
  2. insert: slots and side table through the sorted colour extraction, levels 0 and 1; the grey extraction of a coloured map is the
     grey map's;
  3. the packed run sums at their worst: whole wavefronts of (255, 255, 255) folding into one voxel, a checkerboard of holes,
     (255, 0, 255) for a carry between the halves;
  4. remove, move, rehash -- also a rehash that fails;
  5. colour views: rgba against the yardstick, Z against dvo_hip_map_render, holes;
  6. refusals change nothing;
  7. the C++ facade's coloured PointCloudAggregator against KeyframeMap(colour=True)."""
import ctypes as C
import functools
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
from dvo_slam_amd import _lib
from test_gpu_cloud_map import frames_of, planes_of
from test_gpu_f32_ingest import camera
from test_gpu_lens_ingest import lens_of
from test_map_colour import ColourHostMap, assert_colour_maps_identical, level_colour, pack_plane

pytestmark = pytest.mark.gpu
INF = float("inf")
HOLE = 0x7FC00000


def image_with_pitch(w, h, channels, seed, pitch):
    """an [h, w, channels] uint8 view of random bytes whose rows lie `pitch` bytes apart, and the [h, pitch] array that holds them"""
    assert pitch >= w * channels
    store = np.random.default_rng(seed).integers(0, 256, (h, pitch), dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(store, (h, w, channels), (pitch, channels, 1)), store


def colour_of(pyramids, seed=70):
    """random BGR colour attached to the pyramids in one call; returns their level-0 planes of packed pixels"""
    imgs = [tmc.random_image(p.camera.width, p.camera.height, 3, seed + k) for k, p in enumerate(pyramids)]
    d.set_colour_batch(pyramids, imgs, "bgr8")
    return [pack_plane(np.ascontiguousarray(img), "bgr8") for img in imgs]


def yardstick(pyramids, poses, planes, level, leaf, capacity, min_depth=0.0, max_depth=INF):
    m = ColourHostMap(leaf, capacity)
    for p, T, plane in zip(pyramids, poses, planes):
        I, Z, K = planes_of(p, level)
        m.insert(I, Z, K, T, plane, level=level, min_depth=min_depth, max_depth=max_depth)
    return m


def roomy(pyramids, poses, planes, level, leaf):
    """the yardstick in a table at least four times its voxels: the device cannot drop, its probe sequences are the yardstick's"""
    want = yardstick(pyramids, poses, planes, level, leaf, 1 << 22)
    capacity = 64
    while capacity < 4 * want.stats()["occupied"]:
        capacity *= 2
    want = yardstick(pyramids, poses, planes, level, leaf, capacity)
    assert want.stats()["dropped"] == 0 and want.grey_table().longest_run() < tcm.MAX_PROBES
    return want, capacity


def check_against(m, want, what):
    got = m.extract(sort=True, colour=True)
    assert_colour_maps_identical(got, want.extract(), what)
    s, ws = m.stats(), want.stats()
    for k in ("occupied", "points", "dropped", "out_of_range", "unusable", "capacity", "removed", "unmatched"):
        assert s[k] == ws[k], (what, k, s, ws)
    assert s["over_limit"] == 0
    return got


# ---- 1. k_colour_pack and k_colour_level ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pack_pyramids():
    """pyramids of 67 x 5, 128 x 96 and 321 x 240 with every level up to 2 that their size admits (a frame's coarsest level is at least
    two pixels a side: 67 x 5 has levels 0 and 1 only); their content does not matter to the colour"""
    ctx = d.default_context()
    out = []
    for w, h, levels in ((67, 5, 2), (128, 96, 3), (321, 240, 3)):
        K = np.array([0.8 * w, 0.8 * w, w / 2 - 0.5, h / 2 - 0.5], np.float32)
        out.append(camera(ctx, w, h, K, levels).create(np.zeros((h, w), np.float32), np.ones((h, w), np.float32)))
    return out


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("pixel_format", tmc.FORMATS)
def test_pack_and_level_colour_equal_the_yardstick(pixel_format, padded, source):
    small, mid, large = pack_pyramids()
    ch = _lib.PIXEL_CHANNELS[pixel_format]
    seed = 100 + 8 * tmc.FORMATS.index(pixel_format) + 2 * int(padded) + int(source == "device")
    for k, group in enumerate(([small, mid], [large])):
        # one pitch per call: with padding, the widest frame's row and 13 bytes more (an odd pitch: rows aligned to nothing)
        pitch = max(p.camera.width for p in group) * ch + 13 if padded else 0
        made = [image_with_pitch(p.camera.width, p.camera.height, ch, seed + 50 * k + j, pitch or p.camera.width * ch) for j, p in enumerate(group)]
        planes = [pack_plane(img.copy(), pixel_format) for img, _ in made]
        if source == "host":
            d.set_colour_batch(group, [img for img, _ in made], pixel_format)
        else:
            keep = [torch.from_numpy(store).cuda() for _, store in made]
            d.set_colour_batch(group, [t.data_ptr() for t in keep], pixel_format, pitch)
            for t in keep:
                t.zero_()                                           # (the call has returned: the caller's memory is the caller's again)
            torch.cuda.synchronize()
            del keep
        for p, plane0 in zip(group, planes):
            for level in range(p.levels):
                got = p.colour(level)
                assert got.shape == (p.camera.height >> level, p.camera.width >> level)
                assert np.array_equal(got, level_colour(plane0, level)), (pixel_format, padded, source, p.camera.width, level)
            assert np.all(p.colour(0) >> 24 == 0)
    # 67 x 5 has no level 2 (5 >> 2 < 2 pixels): asked for, it is refused (the host yardstick covers that block shape, test_map_colour.py)
    out = np.full((1, 16), 7, np.uint32)
    ctx = small.ctx
    assert small.levels == 2 and mid.levels == 3 and large.levels == 3
    assert ctx._lib.dvo_hip_frame_download_colour(ctx.ptr, small.ptr, 2, out.ctypes.data_as(C.POINTER(C.c_uint32))) == _lib.ERR_INVALID
    assert np.all(out == 7)


def test_colour_stays_across_a_reingest_and_leaves_with_clear():
    ctx, pyramids, poses = frames_of(128, 96, 2)
    planes = colour_of(pyramids)
    before = pyramids[0].colour(1)
    I, Z, _ = tcm.float_views(128, 96)[1][1]
    d.update_f32_host_batch(pyramids[:1], [I], [Z])
    d.upload_wait(ctx)
    assert np.array_equal(planes_of(pyramids[0], 0)[0].view(np.uint32), I.view(np.uint32))   # (the frame holds the other content now)
    assert np.array_equal(pyramids[0].colour(1), before) and np.array_equal(before, level_colour(planes[0], 1))
    pyramids[0].clear_colour()
    with pytest.raises(ValueError):
        pyramids[0].colour(0)
    out = np.empty((96, 128), np.uint32)
    rc = ctx._lib.dvo_hip_frame_download_colour(ctx.ptr, pyramids[0].ptr, 0, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == _lib.ERR_INVALID
    rc = ctx._lib.dvo_hip_frame_download_colour(ctx.ptr, pyramids[1].ptr, 3, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == _lib.ERR_INVALID                                   # a level the frame lacks


# ---- 2. insert -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("w,h,n", [(128, 96, 2), (321, 240, 3)])
def test_coloured_map_equals_the_yardstick(w, h, n, level):
    ctx, pyramids, poses = frames_of(w, h, n)
    planes = colour_of(pyramids)
    want, capacity = roomy(pyramids, poses, planes, level, 0.02)
    m = d.KeyframeMap(ctx, 0.02, capacity, colour=True)
    m.insert(pyramids, poses, level=level)
    got = check_against(m, want, (w, h, n, level))
    assert (got[1] > 1).sum() > 50 and len(np.unique(got[3])) > 100
    # dvo_hip_map_extract of the coloured map: what a grey map fed the same frames returns
    grey = d.KeyframeMap(ctx, 0.02, capacity)
    grey.insert(pyramids, poses, level=level)
    tcm.assert_maps_identical(m.extract(sort=True), grey.extract(sort=True), "grey extraction")
    tcm.assert_maps_identical(got, grey.extract(sort=True), "colour extraction's grey part")
    # the device output, unsorted: the same records in some order
    xyzi, counts, keys, rgba = m.extract(device=True, colour=True)
    torch.cuda.synchronize()
    order = np.argsort(keys.cpu().numpy().view(np.uint64), kind="stable")
    assert_colour_maps_identical((xyzi.cpu().numpy()[order], counts.cpu().numpy().view(np.uint32)[order], keys.cpu().numpy().view(np.uint64)[order],
                                  rgba.cpu().numpy().view(np.uint32)[order]), got, "device")
    # frame by frame: the same map
    each = d.KeyframeMap(ctx, 0.02, capacity, colour=True)
    for p, T in zip(pyramids, poses):
        each.insert([p], T[None], level=level)
    assert_colour_maps_identical(each.extract(sort=True, colour=True), got, "frame by frame")
    for x in (m, grey, each):
        x.close()


def test_coloured_frames_of_different_sizes_share_a_call():
    ctx, a, pa = frames_of(128, 96, 2)
    _, b, pb = frames_of(102, 78, 1)
    pyramids, poses = [a[0], b[0], a[1]], np.stack([pa[0], pb[0], pa[1]])
    planes = colour_of(pyramids)
    want, capacity = roomy(pyramids, poses, planes, 0, 0.05)
    m = d.KeyframeMap(ctx, 0.05, capacity, colour=True)
    m.insert(pyramids, poses)
    check_against(m, want, "mixed sizes")
    m.close()


# ---- 3. the packed run sums at their worst ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("holes", ["none", "checkerboard"])
@pytest.mark.parametrize("rgb", [(255, 255, 255), (255, 0, 255)])
def test_whole_wavefronts_of_one_colour_fold_into_one_voxel(rgb, holes):
    """a fronto-parallel plane at 128 x 96 and leaf 4: every run of 64 lanes folds into one voxel, 64 * 255 = 16320 per 16-bit field;
    (255, 0, 255) would show a carry out of r into g; a checkerboard of holes makes every run one lane long"""
    w, h = 128, 96
    ctx, p = tgcm.plane_frame(w, h, holes)
    img = np.empty((h, w, 3), np.uint8)
    img[...] = rgb
    p.set_colour(img, "rgb8")
    plane = pack_plane(img, "rgb8")
    assert np.all(plane == (rgb[0] << 16 | rgb[1] << 8 | rgb[2]))
    T = np.eye(4)
    T[:3, 3] = [2.0, -0.2, 0.3]
    want, capacity = roomy([p], [T], [plane], 0, 4.0)
    assert want.stats()["occupied"] <= 2
    m = d.KeyframeMap(ctx, 4.0, capacity, colour=True)
    m.insert([p], T[None])
    got = check_against(m, want, (rgb, holes))
    usable = int(np.isfinite(planes_of(p, 0)[1]).sum())
    assert int(got[1].sum()) == usable and got[1].max() > 2000
    assert np.all(got[3] == (0xFF000000 | rgb[0] << 16 | rgb[1] << 8 | rgb[2]))
    s = m.stats()
    if holes == "none":
        assert s["updates"] <= usable // 32                         # runs were folded: far fewer updates than points
    else:
        assert s["updates"] == usable                               # every run has length 1
    m.remove([p], T[None])
    assert m.stats()["points"] == 0 and len(m.extract(colour=True)[2]) == 0
    m.close()


# ---- 4. remove, move, rehash --------------------------------------------------------------------------------------------------------------

VIEW_K = np.array([70.0, 70.0, 39.5, 29.5], np.float32)


def same_views(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_remove_move_and_rehash_carry_the_colour():
    ctx, pyramids, poses = frames_of(128, 96, 3)
    planes = colour_of(pyramids)
    want_all, capacity = roomy(pyramids, poses, planes, 0, 0.02)
    m = d.KeyframeMap(ctx, 0.02, capacity, colour=True)
    m.insert(pyramids, poses)
    everything = check_against(m, want_all, "three frames")
    # remove: the map that never held the frame
    m.remove(pyramids[1:2], poses[1:2])
    never = d.KeyframeMap(ctx, 0.02, capacity, colour=True)
    never.insert([pyramids[0], pyramids[2]], poses[[0, 2]])
    two = never.extract(sort=True, colour=True)
    assert_colour_maps_identical(m.extract(sort=True, colour=True), two, "after remove")
    assert_colour_maps_identical(two, yardstick([pyramids[0], pyramids[2]], poses[[0, 2]], [planes[0], planes[2]], 0, 0.02, capacity).extract(), "yardstick")
    views = poses[:2]
    assert same_views(m.render_colour(VIEW_K, 80, 60, views), never.render_colour(VIEW_K, 80, 60, views))
    s = m.stats()
    assert s["unmatched"] == 0 and s["vacant"] > 0 and len(two[2]) < len(everything[2])
    # move = remove + insert
    new = poses[2] @ tcm.scenes.se3_exp([0.02, 0.01, -0.015, 0.01, 0.0, -0.01])
    m.move(pyramids[2:], poses[2:], new[None])
    never.remove(pyramids[2:], poses[2:])
    never.insert(pyramids[2:], new[None])
    moved = m.extract(sort=True, colour=True)
    assert_colour_maps_identical(moved, never.extract(sort=True, colour=True), "move")
    assert_colour_maps_identical(moved, yardstick([pyramids[0], pyramids[2]], [poses[0], new], [planes[0], planes[2]], 0, 0.02, capacity).extract(), "move, yardstick")
    # rehash to a larger and to a smaller table keeps every record; the vacant slots go
    views_before = m.render_colour(VIEW_K, 80, 60, views)
    for cap in (capacity * 2, capacity // 2):
        m.rehash(cap)
        s = m.stats()
        assert s["capacity"] == cap and s["vacant"] == 0 and s["occupied"] == len(moved[2])
        assert_colour_maps_identical(m.extract(sort=True, colour=True), moved, "rehash to %d" % cap)
        assert same_views(m.render_colour(VIEW_K, 80, 60, views), views_before)
    # ... and goes on working: the third frame back to where it was
    m.move(pyramids[2:], new[None], poses[2:])
    assert_colour_maps_identical(m.extract(sort=True, colour=True), two, "after the rehashes")
    # a rehash that cannot fit leaves the map and its colours as they are
    stats = m.stats()
    with pytest.raises(d.DvoHipError) as err:
        m.rehash(64)
    assert err.value.code == _lib.ERR_CAPACITY and m.stats() == stats
    assert_colour_maps_identical(m.extract(sort=True, colour=True), two, "after the failed rehash")
    m.clear()
    assert m.stats()["occupied"] == 0
    m.insert(pyramids[:1], poses[:1])
    assert_colour_maps_identical(m.extract(sort=True, colour=True), yardstick(pyramids[:1], poses[:1], planes[:1], 0, 0.02, capacity // 2).extract(), "after clear")
    for x in (m, never):
        x.close()


# ---- 5. colour views ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", [{}, dict(max_splat=1)])
def test_colour_views_equal_the_yardstick(params):
    ctx, pyramids, poses = frames_of(128, 96, 2)
    planes = colour_of(pyramids)
    want, capacity = roomy(pyramids, poses, planes, 0, 0.02)
    m = d.KeyframeMap(ctx, 0.02, capacity, colour=True)
    m.insert(pyramids, poses)
    views = np.stack([poses[0], poses[1] @ tcm.scenes.se3_exp([0.05, 0.0, -0.1, 0.0, 0.03, 0.0])])
    rgba, Z = m.render_colour(VIEW_K, 80, 60, views, **params)
    want_rgba, want_Z = want.render(VIEW_K, 80, 60, views, **params)
    assert rgba.dtype == np.uint32 and rgba.shape == (2, 60, 80)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(Z.view(np.uint32), want_Z.view(np.uint32))
    I_grey, Z_grey = m.render(VIEW_K, 80, 60, views, **params)
    assert np.array_equal(Z.view(np.uint32), Z_grey.view(np.uint32))           # bit for bit the grey view's depth
    hole = Z.view(np.uint32) == HOLE
    assert hole.any() and (~hole).sum() > 1500
    assert np.all(rgba[hole] == 0) and np.all(rgba[~hole] >> 24 == 0xFF) and len(np.unique(rgba[~hole])) > 100
    dev_rgba, dev_Z = m.render_colour(VIEW_K, 80, 60, views, device=True, **params)
    torch.cuda.synchronize()
    assert np.array_equal(dev_rgba.cpu().numpy().view(np.uint32), rgba) and np.array_equal(dev_Z.cpu().numpy().view(np.uint32), Z.view(np.uint32))
    m.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing():
    ctx, pyramids, poses = frames_of(128, 96, 3)
    planes = colour_of(pyramids[:2])
    L = ctx._lib
    coloured, grey = d.KeyframeMap(ctx, 0.05, 1 << 16, colour=True), d.KeyframeMap(ctx, 0.05, 1 << 16)
    coloured.insert(pyramids[:2], poses[:2])
    grey.insert(pyramids, poses)                                    # (a grey map ignores attached colour, and takes frames without)
    before_c, before_g = coloured.stats(), grey.stats()
    records = coloured.extract(sort=True, colour=True)
    T = np.ascontiguousarray(poses, np.float64)
    tp = T.ctypes.data_as(C.POINTER(C.c_double))
    handles = (C.c_void_p * 3)(*[p.ptr for p in pyramids])          # the third carries no colour
    xyzi, rgba, got = np.full((8, 4), -7.0, np.float32), np.full(8, 7, np.uint32), C.c_size_t(99)
    plane_c, plane_z = np.full((60, 80), 7, np.uint32), np.full((60, 80), -7.0, np.float32)
    K = np.ascontiguousarray(VIEW_K)
    kp = K.ctypes.data_as(C.POINTER(C.c_float))
    outs_c, outs_z = (C.c_void_p * 1)(plane_c.ctypes.data), (C.c_void_p * 1)(plane_z.ctypes.data)
    calls = [
        lambda: L.dvo_hip_map_insert(ctx.ptr, coloured.ptr, 3, handles, tp, 0, 0.0, INF),
        lambda: L.dvo_hip_map_remove(ctx.ptr, coloured.ptr, 3, handles, tp, 0, 0.0, INF),
        lambda: L.dvo_hip_map_move(ctx.ptr, coloured.ptr, 3, handles, tp, tp, 0, 0.0, INF),
        lambda: L.dvo_hip_map_extract_colour(ctx.ptr, grey.ptr, 8, xyzi.ctypes.data, rgba.ctypes.data, None, None, 0, C.byref(got)),
        lambda: L.dvo_hip_map_render_colour(ctx.ptr, grey.ptr, 1, 80, 60, kp, tp, None, outs_c, outs_z, 0),
        lambda: L.dvo_hip_map_render_colour(ctx.ptr, coloured.ptr, 1, 80, 60, kp, tp, None, None, outs_z, 0),
        lambda: L.dvo_hip_map_extract_colour(ctx.ptr, coloured.ptr, 8, xyzi.ctypes.data, None, None, None, 0, C.byref(got)),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
    ptr = C.c_void_p()
    assert L.dvo_hip_map_create_ex(ctx.ptr, 0.05, 1024, 2, C.byref(ptr)) == _lib.ERR_INVALID and not ptr.value   # an unknown flag
    assert coloured.stats() == before_c and grey.stats() == before_g
    assert np.all(xyzi == -7.0) and np.all(rgba == 7) and np.all(plane_c == 7) and np.all(plane_z == -7.0)
    assert_colour_maps_identical(coloured.extract(sort=True, colour=True), records, "after the refusals")
    with pytest.raises(ValueError):
        coloured.insert(pyramids, poses)                            # the Python wrapper refuses it first
    with pytest.raises(ValueError):
        grey.extract(colour=True)
    # set_colour: a frame with a lens, a bad format, a short pitch, a null plane -- the frame keeps the colour it had
    lensed = pyramids[0]
    img = tmc.random_image(128, 96, 3, 9)
    addr = (C.c_void_p * 1)(img.ctypes.data)
    one = (C.c_void_p * 1)(lensed.ptr)
    assert L.dvo_hip_frames_set_colour(ctx.ptr, 1, one, addr, 7, 0, 0) == _lib.ERR_INVALID
    assert L.dvo_hip_frames_set_colour(ctx.ptr, 1, one, addr, 0, 0, 0) == _lib.ERR_INVALID          # grey8 is no colour
    assert L.dvo_hip_frames_set_colour(ctx.ptr, 1, one, addr, _lib.PIXEL_FORMATS["bgr8"], 128 * 3 - 1, 0) == _lib.ERR_INVALID
    assert L.dvo_hip_frames_set_colour(ctx.ptr, 1, one, (C.c_void_p * 1)(None), _lib.PIXEL_FORMATS["bgr8"], 0, 0) == _lib.ERR_INVALID
    assert L.dvo_hip_frames_set_colour(ctx.ptr, 1, one, None, _lib.PIXEL_FORMATS["bgr8"], 0, 0) == _lib.ERR_INVALID
    d.set_lens_batch([lensed], *lens_of(lensed.camera.K, "plumb_bob"))
    assert L.dvo_hip_frames_set_colour(ctx.ptr, 1, one, addr, _lib.PIXEL_FORMATS["bgr8"], 0, 0) == _lib.ERR_INVALID
    assert b"lens" in L.dvo_hip_last_error(ctx.ptr)
    with pytest.raises(ValueError):
        lensed.set_colour(np.ascontiguousarray(img))
    assert np.array_equal(lensed.colour(0), planes[0])
    d.clear_lens_batch([lensed])
    other = d.Context(0)
    foreign = camera(other, 128, 96, pyramids[0].camera.K, 3).create(*tcm.float_views(128, 96)[1][0][:2])
    assert L.dvo_hip_frames_set_colour(ctx.ptr, 1, (C.c_void_p * 1)(foreign.ptr), addr, _lib.PIXEL_FORMATS["bgr8"], 0, 0) == _lib.ERR_INVALID
    assert coloured.stats() == before_c
    for x in (coloured, grey):
        x.close()
    del foreign
    other.close()


# ---- 7. the C++ facade ----------------------------------------------------------------------------------------------------------------------

def facade_colour(k, w=64, h=48):
    """the colour of keyframe k of tests/cpp/map_colour_facade_check.cpp as bytes B, G, R: the floats truncated and saturated"""
    y, x = np.mgrid[0:h, 0:w]
    b = ((x * 5 + y * 3 + k * 7) % 300 - 20).astype(np.float32) + np.float32(0.5)
    g = ((x * 11 + y * 2 + k) % 256).astype(np.float32) + np.float32(0.75)
    r = ((x + y * 9 + k * 3) % 256).astype(np.float32)
    return np.stack([np.clip(np.trunc(c), 0, 255).astype(np.uint8) for c in (b, g, r)], axis=-1)


def test_cpp_facade_coloured_aggregator_equals_keyframe_map():
    d.build()
    exe = tmc.build_map_colour_facade_check()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.bin")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, np.uint32).reshape(-1, 5)
    ctx = d.default_context()
    cam = camera(ctx, 64, 48, np.array([60.0, 60.0, 31.5, 23.5], np.float32), 1)
    pyramids, poses, imgs = [], [], []
    for k in range(3):
        I, Z, T = tgcm.facade_frame(k)
        pyramids.append(cam.create(I, Z))
        poses.append(T)
        imgs.append(facade_colour(k))
    assert min(int(img[..., 0].min()) for img in imgs) == 0 and max(int(img[..., 0].max()) for img in imgs) == 255   # saturated both ways
    d.set_colour_batch(pyramids, imgs, "bgr8")
    m = d.KeyframeMap(ctx, 0.01, 1 << 20, colour=True)
    m.insert(pyramids, np.stack(poses))
    xyzi, counts, keys, rgba = m.extract(sort=True, colour=True)
    assert len(xyzi) > 1000 and m.stats()["dropped"] == 0
    assert got.shape[0] == len(xyzi) and np.array_equal(got[:, :4], xyzi.view(np.uint32)) and np.array_equal(got[:, 4], rgba)
    m.close()
