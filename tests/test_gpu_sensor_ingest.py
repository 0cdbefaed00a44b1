"""GPU tier (-m gpu): raw sensor planes at the ingest (DVO_HIP_PIXEL_BAYER_*, DVO_HIP_PIXEL_YUYV8 / _UYVY8; k_sensor_convert) against the
numpy statement of the formats (tests/sensor_formats.py).

A sensor plane is defined by its BGR8 image, and the frame is then a BGR8 frame: every frame here is compared bit for bit -- all six
planes of every level, selection counts and masks -- with the oracle pyramid of po.bgr_to_grey(converted), or with a twin fed the converted
image's grey plane through the grey entry points; set_colour with the packed converted image.  The sensor planes are the tinted scenes of
test_gpu_colour_ingest mosaicked / subsampled, uniform noise (smooth scenes hide rounding and phase errors), a constant and one-hot images.
The path each ingest took is asserted through the counters "sensor_ingests", "strip_ingests" and "colour_ingests"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import common as cm
import dvo_slam_amd as d
import scenes
import sensor_formats as sf
import test_depth_rig as tdr
import test_lens as tl
from dvo_slam_amd import _lib
from oracle import pyoracle as po
from test_gpu_colour_ingest import assert_records_identical, device_plane, match_records, tinted
from test_gpu_f32_ingest import assert_frames_equal, blank_frames, camera, config, host_view
from test_gpu_lens_ingest import SCALE, raw_scene
from test_gpu_scene_edges import assert_frame_equals_oracle

pytestmark = pytest.mark.gpu
ROLES = (None, "current", "reference")


def plane3(raw):
    return raw if raw.ndim == 3 else raw[..., None]


@functools.lru_cache(maxsize=None)
def sensor_scene(fmt, w, h):
    """(scene, per view: (sensor plane, its BGR image, u16 depth)): view 0 the tinted scene in the sensor's format, view 1 uniform noise"""
    p = cm.synth(5, w, h) if h < 16 else scenes.edge_scene(3, w, h)
    first = sf.to_sensor(tinted(p["grey_ref"], 1), fmt)
    second = sf.noise((h, w) if fmt in sf.BAYER else (h, w, 2), w + h)
    return p, [(first, sf.to_bgr(first, fmt), p["depth_ref"]), (second, sf.to_bgr(second, fmt), p["depth_cur"])]


def oracle_pyramid(bgr, depth, K, levels):
    return po.Pyramid(po.bgr_to_grey(bgr), po.convert_raw_depth(depth), K, levels)


def counters(ctx):
    return tuple(ctx.counter(k) for k in ("sensor_ingests", "strip_ingests", "colour_ingests"))


def depth_tensor(z):
    return torch.from_numpy(np.ascontiguousarray(z).astype(np.int16)).cuda()


def run_device(frames, raws, depths, fmt, role=None, levels=4, offset=0, pad=0, flags=0):
    keep, cptrs, dptrs, pitch = [], [], [], 0
    for raw, z in zip(raws, depths):
        r = plane3(raw)
        t, ptr, pitch = device_plane(r, offset, r.shape[1] * r.shape[2] + pad)
        tz = depth_tensor(z)
        keep += [t, tz]
        cptrs.append(ptr)
        dptrs.append(tz.data_ptr())
    d.update_colour_device_batch(frames, cptrs, dptrs, fmt, pitch, role=role, config=config(levels) if role else None, flags=flags)
    return keep


def run_host(frames, raws, depths, fmt, role=None, levels=4, pad=0, pinned=False, flags=0):
    hosts = []
    for raw in raws:
        if pinned:
            buf = torch.empty(raw.size, dtype=torch.uint8).pin_memory().numpy().reshape(raw.shape)
            buf[...] = raw
            hosts.append(buf)
        else:
            hosts.append(host_view(raw, pad))
    zs = [np.ascontiguousarray(z) for z in depths]
    d.update_colour_host_batch(frames, hosts, zs, fmt, role=role, config=config(levels) if role else None, flags=flags)
    d.upload_wait(frames[0].ctx)
    return hosts + zs


# ---- 1. planes and selection, every format, every path of the kernel ----------------------------------------------------------------

# (w, h, levels, byte offset of the sensor plane, row padding in bytes, strip ingest behind the pass); YUV takes the next even width
SHAPES = [(17, 5, 1, 0, 0, False), (18, 6, 2, 0, 0, False), (322, 242, 4, 1, 3, False), (640, 480, 4, 0, 64, True)]


def planes_cases():
    out = []
    for i, fmt in enumerate(sf.FORMATS):
        for j, s in enumerate(SHAPES):
            role = ROLES[(i + j) % 3]
            out.append(pytest.param(fmt, s, role, id="%s-%dx%d-%s" % (fmt, s[0], s[1], role)))
    return out


@pytest.mark.parametrize("fmt,shape,role", planes_cases())
def test_planes_and_selection(fmt, shape, role):
    w, h, levels, offset, pad, strip = shape
    w += w % 2 if fmt in sf.YUV else 0
    p, views = sensor_scene(fmt, w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], levels)
    frames = blank_frames(cam, 2)
    c0 = counters(ctx)
    keep = run_device(frames, [v[0] for v in views], [v[2] for v in views], fmt, role, levels, offset, pad)
    torch.cuda.synchronize()
    assert counters(ctx) == (c0[0] + 2, c0[1] + (2 if strip else 0), c0[2]), (fmt, shape)
    for f, v in zip(frames, views):
        assert_frame_equals_oracle(f, oracle_pyramid(v[1], v[2], p["K"], levels), levels, (fmt, shape, role))
    del keep


@pytest.mark.parametrize("fmt", sf.BAYER)
def test_constant_and_one_hot_mosaics(fmt):
    """level 0 of an 18 x 6 frame created from a constant mosaic and from a single 255 at each phase and corner"""
    w, h = 18, 6
    ctx = d.default_context()
    cam = camera(ctx, w, h, np.array([20.0, 20.0, 8.5, 2.5], np.float32), 1)
    z = np.full((h, w), 5000, np.uint16)
    for n, raw in enumerate([np.full((h, w), 201, np.uint8)] + sf.one_hots(h, w)):
        want = po.bgr_to_grey(sf.demosaic(raw, fmt))
        f = cam.create_colour(raw, z, fmt)                        # (host planes: the upload buffers carry 1 B per pixel)
        assert np.array_equal(np.asarray(f.level(0).intensity), want), (fmt, n)
        t, ptr, pitch = device_plane(plane3(raw), 2, w + 5)
        tz = depth_tensor(z)
        g = cam.create_colour_device(ptr, fmt, pitch, tz.data_ptr())
        assert np.array_equal(np.asarray(g.level(0).intensity), want), (fmt, n, "device")


# ---- 2. every (Y, U, V) once at both positions of a pair ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def every_yuv_grey():
    return po.bgr_to_grey(sf.every_yuv_bgr())


@pytest.mark.parametrize("fmt", sf.YUV)
def test_exhaustive_yuv_conversion(fmt):
    h, w = sf.EVERY_YUV_SHAPE
    ctx = d.default_context()
    t = torch.from_numpy(sf.every_yuv(fmt)).cuda()
    depth = torch.full((h, w), 5000, dtype=torch.int16, device="cuda")
    cam = camera(ctx, w, h, np.array([6000.0, 6000.0, 4095.5, 2047.5], np.float32), 1)
    c0 = counters(ctx)
    frame = cam.create_colour_device(t.data_ptr(), fmt, 0, depth.data_ptr())
    got = np.asarray(frame.level(0).intensity)
    assert np.array_equal(got, every_yuv_grey()), fmt
    assert counters(ctx) == (c0[0] + 1, c0[1] + 1, c0[2])


# ---- 3. colour ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", sf.FORMATS)
def test_set_colour_stores_the_packed_converted_image(fmt):
    ctx = d.default_context()
    small_w = 18 if fmt in sf.YUV else 17
    sizes = [(small_w, 5, 1), (322, 242, 4)]
    pyrs, views = [], []
    for w, h, levels in sizes:
        p, v = sensor_scene(fmt, w, h)
        f = blank_frames(camera(ctx, w, h, p["K"], levels), 2)
        pyrs += f
        views += v
    # host arrays, frames of two sizes in one call
    d.set_colour_batch(pyrs, [v[0] for v in views], fmt)
    for f, v in zip(pyrs, views):
        assert np.array_equal(f.colour(), sf.packed(v[1])), (fmt, "host")
    d.clear_colour_batch(pyrs)
    # device planes at byte offset 1 with 3 bytes of row padding (one pitch per call: the two sizes apart), views swapped
    for k in (0, 2):
        placed = [device_plane(plane3(views[k + 1 - i][0]), 1, plane3(views[k][0]).shape[1] * sf.channels(fmt) + 3) for i in range(2)]
        d.set_colour_batch(pyrs[k:k + 2], [x[1] for x in placed], fmt, placed[0][2])
        for i in range(2):
            assert np.array_equal(pyrs[k + i].colour(), sf.packed(views[k + 1 - i][1])), (fmt, "device", k, i)
    # a later re-ingest keeps it, and the pyramid levels' colour is the block mean of the packed plane
    keep = run_device(pyrs[2:], [v[0] for v in views[2:]], [v[2] for v in views[2:]], fmt, "reference", 4)
    assert np.array_equal(pyrs[2].colour(), sf.packed(views[3][1])) and np.array_equal(pyrs[3].colour(), sf.packed(views[2][1]))
    bgr = views[3][1].astype(np.uint32).reshape(121, 2, 161, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(pyrs[2].colour(1), sf.packed((bgr + 2) >> 2))
    del keep


# ---- 4. the ways in agree -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def three_frames(fmt):
    w, h = 320, 240
    p, views = sensor_scene(fmt, w, h)
    third = sf.to_sensor(tinted(p["grey_cur"], 2), fmt)
    return p, views + [(third, sf.to_bgr(third, fmt), p["depth_cur"])]


_baselines = {}


def baseline(fmt):
    """case 1: device planes, a plain update -- held to the oracle once, then the yardstick of every other way in"""
    if fmt not in _baselines:
        p, views = three_frames(fmt)
        ctx = d.default_context()
        cam = camera(ctx, 320, 240, p["K"], 4)
        frames = blank_frames(cam, 3)
        keep = run_device(frames, [v[0] for v in views], [v[2] for v in views], fmt)
        torch.cuda.synchronize()
        assert_frame_equals_oracle(frames[2], oracle_pyramid(views[2][1], views[2][2], p["K"], 4), 4, (fmt, "baseline"))
        _baselines[fmt] = (cam, frames, keep)
    return _baselines[fmt]


WAYS = ("pageable", "pinned", "current", "reference", "host_reference", "deferred", "keep_raw_copy_1", "keep_raw_copy_0", "current_then_reference")


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("fmt", ("bayer_grbg8", "yuyv8"))
def test_paths_agree(fmt, way):
    p, views = three_frames(fmt)
    cam, want, _ = baseline(fmt)
    ctx = d.default_context()
    frames = blank_frames(cam, 3)
    raws, zs = [v[0] for v in views], [v[2] for v in views]
    c0 = counters(ctx)
    refused = False
    if way in ("pageable", "pinned"):
        keep = run_host(frames, raws, zs, fmt, pinned=way == "pinned", pad=0 if way == "pinned" else 6)
    elif way == "host_reference":
        keep = run_host(frames, raws, zs, fmt, role="reference")
    elif way in ("current", "reference"):
        keep = run_device(frames, raws, zs, fmt, role=way)
    elif way == "deferred":
        d0 = ctx.counter("deferred_ingests")
        keep = run_device(frames, raws, zs, fmt, role="current", flags=_lib.INGEST_DEFER)
        assert counters(ctx) == c0                                  # recorded: nothing converted yet
        ctx.check(ctx._lib.dvo_hip_flush_deferred(ctx.ptr))
        assert ctx.counter("deferred_ingests") == d0 + 1
    elif way == "keep_raw_copy_1":
        keep = run_device(frames, raws, zs, fmt, role="reference")
        d.prepare_roles_batch(frames, "current", config(4))          # the other role, from the raw copy
    elif way == "keep_raw_copy_0":
        # without a copy the other role is refused, as after a grey ingest; the selection and the upper levels stand, and the frames
        # take the next ingest as any frame does
        keep = run_device(frames, raws, zs, fmt, role="reference", flags=_lib.INGEST_NO_RAW_COPY)
        with pytest.raises(d.DvoHipError) as e:
            d.prepare_roles_batch(frames, "current", config(4))
        assert e.value.code == _lib.ERR_INVALID
        for f, g in zip(frames, want):
            assert d.PointSelection(f, 6.0, 0.03).select(0) == d.PointSelection(g, 6.0, 0.03).select(0)
            for l in range(1, 4):
                assert np.array_equal(np.asarray(f.level(l).intensity), np.asarray(g.level(l).intensity)), (fmt, way, l)
        refused = True
        keep += run_device(frames, raws, zs, fmt)
    else:
        # a current frame keeps no copy either way; the reference role is derived from its sampling planes
        keep = run_device(frames, raws, zs, fmt, role="current", flags=_lib.INGEST_NO_RAW_COPY)
        d.prepare_roles_batch(frames, "reference", config(4))
    torch.cuda.synchronize()
    assert counters(ctx) == (c0[0] + (6 if refused else 3), c0[1] + (6 if refused else 3), c0[2]), (fmt, way)
    for f, g in zip(frames, want):
        assert_frames_equal(f, g, 4, (fmt, way))
    del keep


# ---- 5. with a lens, with a depth rig, with both --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ("bayer_rggb8", "uyvy8"))
@pytest.mark.parametrize("size", [(64, 48, 3), (320, 240, 4)], ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("rig,lens", [(False, True), (True, False), (True, True)], ids=("lens", "rig", "rig+lens"))
def test_with_lens_and_rig_equals_the_grey_fed_twin(fmt, size, rig, lens):
    w, h, levels = size
    K, scene_views = raw_scene(w, h)
    raws = [sf.to_sensor(v["bgr"], fmt) for v in scene_views]
    greys = [po.bgr_to_grey(sf.to_bgr(r, fmt)).astype(np.uint8) for r in raws]
    zs = [v["depth"] for v in scene_views]
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    for group in (frames, twins):
        if rig:
            d.set_depth_rig_batch(group, *tdr.kinect_rig(K))
        if lens:
            d.set_lens_batch(group, tl.raw_K(K), tl.FR1_D, rectify_depth=not rig)
    role = "reference" if rig else "current"
    c0 = counters(ctx)
    l0, r0 = ctx.counter("lens_ingests"), ctx.counter("depth_registrations")
    keep = run_device(frames, raws, zs, fmt, role, levels, offset=1 if lens else 0, pad=1 if lens else 0)
    assert counters(ctx)[0] == c0[0] + 2 and counters(ctx)[2] == c0[2]
    assert (ctx.counter("lens_ingests"), ctx.counter("depth_registrations")) == (l0 + (2 if lens else 0), r0 + (2 if rig else 0))
    tg, tz = [torch.from_numpy(g).cuda() for g in greys], [depth_tensor(z) for z in zs]
    d.update_raw_device_batch(twins, [t.data_ptr() for t in tg], [t.data_ptr() for t in tz], SCALE, role=role, config=config(levels))
    torch.cuda.synchronize()
    assert counters(ctx)[0] == c0[0] + 2                             # (the twins were fed grey)
    for f, t in zip(frames, twins):
        assert_frames_equal(f, t, levels, (fmt, size, rig, lens))
    del keep


# ---- 6. a match -------------------------------------------------------------------------------------------------------------------------

def test_match_equals_the_match_on_the_converted_bgr_image():
    w, h, fmt = 320, 240, "bayer_grbg8"
    p = cm.synth(103, w, h)
    raws = [sf.mosaic(tinted(p["grey_ref"], 11), fmt), sf.mosaic(tinted(p["grey_cur"], 21), fmt)]
    bgrs = [sf.demosaic(r, fmt) for r in raws]
    zs = [p["depth_ref"], p["depth_cur"]]
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], 4)
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    a, b = blank_frames(cam, 2), blank_frames(cam, 2)
    keep = run_device(a[:1], raws[:1], zs[:1], fmt, "reference") + run_device(a[1:], raws[1:], zs[1:], fmt, "current")
    keep += run_device(b[:1], bgrs[:1], zs[:1], "bgr8", "reference") + run_device(b[1:], bgrs[1:], zs[1:], "bgr8", "current")
    got, want = match_records(ctx, cfg, a[:1], a[1:]), match_records(ctx, cfg, b[:1], b[1:])
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1])
    assert_records_identical(got, want)
    assert not np.array_equal(got[0][0], np.eye(4))                  # (the pair does move)
    del keep


# ---- 7. refusals through the C-ABI ------------------------------------------------------------------------------------------------------

def level0(frame):
    torch.cuda.synchronize()
    return [np.asarray(getattr(frame.level(0), name)).copy() for name in ("intensity", "depth")]


def test_bad_arguments_are_refused_and_change_nothing():
    fmt = "bayer_grbg8"
    p, views = three_frames(fmt)
    ctx = d.default_context()
    cam = camera(ctx, 320, 240, p["K"], 4)
    frames = blank_frames(cam, 2)
    keep = run_device(frames, [v[0] for v in views[:2]], [v[2] for v in views[:2]], fmt, "reference")
    d.set_colour_batch(frames, [v[0] for v in views[:2]], fmt)
    before = [level0(f) for f in frames]
    colour_before = [f.colour() for f in frames]
    odd_cam = camera(ctx, 321, 240, p["K"], 4)
    odd = blank_frames(odd_cam, 2)
    odd_before = [level0(f) for f in odd]
    t = torch.zeros(320 * 240 * 2 + 64, dtype=torch.uint8, device="cuda")
    tz = depth_tensor(views[0][2])
    L, vp = ctx._lib, C.c_void_p
    fr, ofr = (vp * 2)(frames[0].ptr, frames[1].ptr), (vp * 2)(odd[0].ptr, odd[1].ptr)
    good, good_z = (vp * 2)(t.data_ptr(), t.data_ptr()), (vp * 2)(tz.data_ptr(), tz.data_ptr())
    holed = (vp * 2)(t.data_ptr(), None)
    cfg = config(4).to_c()
    update, f32depth, set_colour = L.dvo_hip_frames_update_colour_device_as_ex, L.dvo_hip_frames_update_colour_f32depth_device_as_ex, L.dvo_hip_frames_set_colour
    calls = [lambda v=v: update(ctx.ptr, 2, fr, good, v, 0, good_z, 2e-4, 1, C.byref(cfg), 0) for v in (6, 15, 22)]
    calls += [lambda v=v: set_colour(ctx.ptr, 2, fr, good, v, 0, 1) for v in (6, 15, 22)]
    calls += [lambda v=v: f32depth(ctx.ptr, 2, fr, good, v, 0, good_z, 0, 1.0, -1, None, 0) for v in (6, 15, 22)]
    calls += [
        lambda: update(ctx.ptr, 2, ofr, good, 20, 0, good_z, 2e-4, -1, None, 0),               # an odd YUV width
        lambda: update(ctx.ptr, 2, ofr, good, 21, 0, good_z, 2e-4, 0, C.byref(cfg), 0),
        lambda: set_colour(ctx.ptr, 2, ofr, good, 20, 0, 1),
        lambda: update(ctx.ptr, 2, fr, good, 19, 320 - 1, good_z, 2e-4, 1, C.byref(cfg), 0),   # pitch = w * bytes - 1
        lambda: update(ctx.ptr, 2, fr, good, 20, 640 - 1, good_z, 2e-4, -1, None, 1),
        lambda: set_colour(ctx.ptr, 2, fr, good, 21, 640 - 1, 1),
        lambda: L.dvo_hip_frames_update_colour_as_ex(ctx.ptr, 2, fr, good, 16, 320 - 1, good_z, 2e-4, -1, None, 0),
        lambda: update(ctx.ptr, 2, fr, holed, 17, 0, good_z, 2e-4, 1, C.byref(cfg), 0),        # a null plane in the table
        lambda: update(ctx.ptr, 2, fr, good, 18, 0, (vp * 2)(None, tz.data_ptr()), 2e-4, -1, None, 0),
        lambda: set_colour(ctx.ptr, 2, fr, holed, 19, 0, 1),
    ]
    c0 = counters(ctx)
    d0 = ctx.counter("deferred_ingests")
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
    out = vp()
    K = np.ascontiguousarray(p["K"], np.float32)
    fp = K.ctypes.data_as(C.POINTER(C.c_float))
    create = L.dvo_hip_frame_create_colour_device
    assert create(ctx.ptr, 1, 240, fp, t.data_ptr(), 16, 0, tz.data_ptr(), 2e-4, 1, C.byref(out)) == _lib.ERR_INVALID     # a 1-wide mosaic
    assert create(ctx.ptr, 320, 1, fp, t.data_ptr(), 19, 0, tz.data_ptr(), 2e-4, 1, C.byref(out)) == _lib.ERR_INVALID
    assert create(ctx.ptr, 321, 240, fp, t.data_ptr(), 20, 0, tz.data_ptr(), 2e-4, 4, C.byref(out)) == _lib.ERR_INVALID
    assert create(ctx.ptr, 320, 240, fp, t.data_ptr(), 22, 0, tz.data_ptr(), 2e-4, 4, C.byref(out)) == _lib.ERR_INVALID
    assert L.dvo_hip_frame_create_colour(ctx.ptr, 320, 240, fp, None, 19, 0, None, 2e-4, 4, C.byref(out)) == _lib.ERR_INVALID
    assert not out.value
    ctx.check(L.dvo_hip_flush_deferred(ctx.ptr))                     # (the refused deferred call recorded nothing)
    assert counters(ctx) == c0 and ctx.counter("deferred_ingests") == d0
    for f, b in zip(frames + odd, before + odd_before):
        for x, y in zip(level0(f), b):
            assert np.array_equal(x, y, equal_nan=True)
    for f, c in zip(frames, colour_before):
        assert np.array_equal(f.colour(), c)
    for f, v in zip(frames, views):
        assert_frame_equals_oracle(f, oracle_pyramid(v[1], v[2], p["K"], 4), 4, "after refused calls")
    del keep


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_takes_sensor_planes():
    """tests/cpp/sensor_facade_check.cpp: createFromColour from a Bayer mosaic, setColour from a YUYV plane"""
    import subprocess
    from test_sensor_formats import build_sensor_facade_check
    d.build()
    out = subprocess.run([build_sensor_facade_check()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split() == ["ok", str(64 * 48)], (out.returncode, out.stdout, out.stderr)
