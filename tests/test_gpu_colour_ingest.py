"""GPU tier (-m gpu): the colour ingest (dvo_hip_frame_create_colour*, dvo_hip_frames_update_colour*) against CPU restatements.

The colour images are the edge scene's and the synthetic pair's grey planes with a smooth tint of their own per channel, so a channel-
order error moves the grey value by tens of levels.  Every frame is compared with the oracle pyramid of po.bgr_to_grey(colour), bit for
bit: all six planes of every level, selection counts and masks; the path each ingest took (strip kernel or tile kernel) is asserted
through the counters "strip_ingests" / "colour_ingests"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import common as cm
import dvo_slam_amd as d
import scenes
from dvo_slam_amd import _lib, tum
from oracle import pyoracle as po
from test_gpu_scene_edges import assert_frame_equals_oracle

pytestmark = pytest.mark.gpu
FORMATS = ("bgr8", "rgb8", "bgra8", "rgba8")
CHANNELS = {"bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}
THR = (6.0, 0.03)


def tinted(grey, seed):
    """a BGR u8 image whose grey is close to `grey` and whose three channels differ by up to ~70 levels, smoothly"""
    h, w = grey.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = np.random.default_rng(seed).uniform(0, 6.28, 3)
    g = grey.astype(np.float64)
    b = g + 45 * np.sin(x / 37.0 + ph[0])
    gg = g + 25 * np.cos(y / 23.0 + ph[1])
    r = g - 40 * np.sin((x + y) / 51.0 + ph[2])
    return np.clip(np.rint(np.stack([b, gg, r], -1)), 0, 255).astype(np.uint8)


def in_format(bgr, fmt):
    """the same colours laid out as `fmt` (alpha: noise, which the conversion must ignore)"""
    c = bgr if fmt.startswith("bgr") else bgr[..., ::-1]
    if fmt.endswith("a8"):
        alpha = np.random.default_rng(7).integers(0, 256, bgr.shape[:2] + (1,), dtype=np.uint8)
        c = np.concatenate([c, alpha], -1)
    return np.ascontiguousarray(c)


@functools.lru_cache(maxsize=None)
def scene(kind, w, h):
    p = scenes.edge_scene(3, w, h) if kind == "edge" else cm.synth(5, w, h)
    return p, tinted(p["grey_ref"], 1), tinted(p["grey_cur"], 2)


def oracle_pyramid(bgr, depth, K, levels):
    return po.Pyramid(po.bgr_to_grey(bgr), po.convert_raw_depth(depth), K, levels)


def camera(ctx, w, h, K, levels):
    cam = d.RgbdCameraPyramid(w, h, K, ctx)
    cam.build(levels)
    return cam


def blank_frames(cam, n):
    w, h = cam.width, cam.height
    return [cam.create_raw(np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint16)) for _ in range(n)]


def device_plane(arr, offset=0, pitch=0):
    """(tensor, address, pitch) of `arr` [h, w, c] in device memory: `offset` bytes into the allocation, rows `pitch` bytes apart"""
    h, w, c = arr.shape
    pitch = pitch or w * c
    host = np.zeros(offset + pitch * h + 16, np.uint8)
    rows = host[offset:offset + pitch * h].reshape(h, pitch)
    rows[:, :w * c] = arr.reshape(h, w * c)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + offset, pitch


def config(levels):
    return d.Config(FirstLevel=levels - 1, LastLevel=0, IntensityDerivativeThreshold=THR[0], DepthDerivativeThreshold=THR[1])


def counters(ctx):
    return ctx.counter("strip_ingests"), ctx.counter("colour_ingests")


# ---- 1. every colour once, each format --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_exhaustive_conversion(fmt):
    ctx = d.default_context()
    i = np.arange(1 << 24, dtype=np.uint32)
    bgr = np.stack([(i >> 16).astype(np.uint8), (i >> 8 & 255).astype(np.uint8), (i & 255).astype(np.uint8)], -1).reshape(4096, 4096, 3)
    want = tum.bgr_to_grey(bgr).astype(np.float32)
    t, ptr, pitch = device_plane(in_format(bgr, fmt))
    depth = torch.full((4096, 4096), 5000, dtype=torch.int16, device="cuda")
    cam = camera(ctx, 4096, 4096, np.array([3000.0, 3000.0, 2047.5, 2047.5], np.float32), 1)
    s0, c0 = counters(ctx)
    frame = cam.create_colour_device(ptr, fmt, 0, depth.data_ptr())
    got = np.asarray(frame.level(0).intensity)
    assert np.array_equal(got, want), fmt
    assert counters(ctx) == (s0 + 1, c0 + 1)


# ---- 2. planes and selection on every path ----------------------------------------------------------------------------------------

# (kind, w, h, byte offset of the colour plane, row padding in bytes, strip path)
SHAPES = [("edge", 640, 480, 0, 0, True), ("edge", 640, 480, 0, 64, True), ("edge", 321, 240, 0, 0, False), ("synth", 17, 5, 0, 0, False),
          ("edge", 640, 480, 1, 0, False), ("edge", 640, 480, 0, 3, False)]
ROLES = (None, "current", "reference")


def run_update(frames, colours, depths, fmt, entry, role, levels, offset=0, pad=0, flags=0):
    keep = []
    if entry == "device":
        cptrs, dptrs = [], []
        for c, z in zip(colours, depths):
            t, ptr, pitch = device_plane(c, offset, c.shape[1] * c.shape[2] + pad)
            tz = torch.from_numpy(z.astype(np.int16)).cuda()
            keep += [t, tz]
            cptrs.append(ptr)
            dptrs.append(tz.data_ptr())
        d.update_colour_device_batch(frames, cptrs, dptrs, fmt, pitch, role=role, config=config(levels) if role else None, flags=flags)
    else:
        hosts = []
        for c in colours:
            h, w, ch = c.shape
            buf = np.zeros((h, w * ch + pad), np.uint8)
            view = buf[:, :w * ch].reshape(h, w, ch)
            view[...] = c
            hosts.append(view)
        keep += hosts
        d.update_colour_host_batch(frames, hosts, list(depths), fmt, role=role, config=config(levels) if role else None, flags=flags)
        d.upload_wait(frames[0].ctx)
    torch.cuda.synchronize()
    return keep


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s%dx%d_off%d_pad%d" % s[:5])
@pytest.mark.parametrize("role", ROLES, ids=str)
@pytest.mark.parametrize("fmt", FORMATS)
def test_planes_and_selection_device(shape, role, fmt):
    check_update(shape, role, fmt, "device")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] == 0], ids=lambda s: "%s%dx%d_pad%d" % (s[0], s[1], s[2], s[4]))
@pytest.mark.parametrize("role", ROLES, ids=str)
def test_planes_and_selection_host(shape, role):
    fmt = FORMATS[(shape[1] + shape[4] + len(str(role))) % 4]
    check_update(shape, role, fmt, "host")


def check_update(shape, role, fmt, entry):
    kind, w, h, offset, pad, strip = shape
    p, bgr_ref, bgr_cur = scene(kind, w, h)
    levels = 2 if h < 16 else 4
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], levels)
    frames = blank_frames(cam, 2)
    s0, c0 = counters(ctx)
    run_update(frames, [in_format(bgr_ref, fmt), in_format(bgr_cur, fmt)], [p["depth_ref"], p["depth_cur"]], fmt, entry, role, levels, offset, pad)
    if entry == "host":
        strip = w % 4 == 0                    # (host planes arrive in the upload buffer with tight rows, whatever the caller's pitch)
    assert counters(ctx) == (s0 + (2 if strip else 0), c0 + 2), (shape, fmt)
    for f, bgr, z in ((frames[0], bgr_ref, p["depth_ref"]), (frames[1], bgr_cur, p["depth_cur"])):
        assert_frame_equals_oracle(f, oracle_pyramid(bgr, z, p["K"], levels), levels, (shape, role, fmt, entry))


@pytest.mark.parametrize("fmt", FORMATS)
def test_create_colour_host(fmt):
    p, bgr_ref, _ = scene("edge", 640, 480)
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    s0, c0 = counters(ctx)
    f = cam.create_colour(in_format(bgr_ref, fmt), p["depth_ref"], fmt)
    assert counters(ctx) == (s0 + 1, c0 + 1)
    assert_frame_equals_oracle(f, oracle_pyramid(bgr_ref, p["depth_ref"], p["K"], 4), 4, fmt)
    # a padded host pitch (a view into a wider image) and an odd width
    p2, bgr2, _ = scene("edge", 321, 240)
    wide = np.zeros((240, 330, CHANNELS[fmt]), np.uint8)
    wide[:, :321] = in_format(bgr2, fmt)
    cam2 = camera(ctx, 321, 240, p2["K"], 4)
    f2 = cam2.create_colour(wide[:, :321], p2["depth_ref"], fmt)
    assert_frame_equals_oracle(f2, oracle_pyramid(bgr2, p2["depth_ref"], p2["K"], 4), 4, (fmt, "padded"))


# ---- 3. the raw copy stays grey ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ("device", "host"))
def test_raw_copy_serves_the_other_role(entry):
    p, bgr_ref, bgr_cur = scene("edge", 640, 480)
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    frames = blank_frames(cam, 2)
    run_update(frames, [in_format(bgr_ref, "bgra8"), in_format(bgr_cur, "bgra8")], [p["depth_ref"], p["depth_cur"]], "bgra8", entry, "reference", 4)
    d.prepare_roles_batch(frames, "current", d.Config(FirstLevel=3, LastLevel=0))
    for f, bgr, z in ((frames[0], bgr_ref, p["depth_ref"]), (frames[1], bgr_cur, p["depth_cur"])):
        assert_frame_equals_oracle(f, oracle_pyramid(bgr, z, p["K"], 4), 4, entry)   # (also reselects at other thresholds)


def test_no_raw_copy_refuses_the_other_role_and_keeps_the_frame():
    p, bgr_ref, _ = scene("edge", 640, 480)
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    frames = blank_frames(cam, 1)
    run_update(frames, [in_format(bgr_ref, "rgb8")], [p["depth_ref"]], "rgb8", "device", "reference", 4, flags=_lib.INGEST_NO_RAW_COPY)
    o = oracle_pyramid(bgr_ref, p["depth_ref"], p["K"], 4)
    with pytest.raises(d.DvoHipError) as e:
        d.prepare_roles_batch(frames, "current", d.Config(FirstLevel=3, LastLevel=0))
    assert e.value.code == _lib.ERR_INVALID
    assert d.PointSelection(frames[0], *THR).select(0) == o.select(0, *THR)[0]   # (the mask needs the current role: not here)
    for l in range(1, 4):
        for k, name in enumerate(("intensity", "depth")):
            assert np.array_equal(np.asarray(getattr(frames[0].level(l), name)), o.plane(l, k)[0], equal_nan=True), (l, name)
    with pytest.raises(d.DvoHipError):
        d.PointSelection(frames[0], 0.0, 0.0).select(0)


# ---- 4. deferred ingest, 5. whole matches -----------------------------------------------------------------------------------------

def pairs_of(n, w, h):
    out = []
    for k in range(n):
        p = cm.synth(100 + k % 8, w, h)
        out.append((p, tinted(p["grey_ref"], 10 + k % 8), tinted(p["grey_cur"], 20 + k % 8)))
    return out


def records(results):
    return [(r.Transformation.copy(), r.Information.copy(), r.LogLikelihood) for r in results]


def assert_records_identical(a, b):
    for (Ta, Ia, la), (Tb, Ib, lb) in zip(a, b):
        assert np.array_equal(Ta, Tb) and np.array_equal(Ia, Ib) and la == lb


def match_records(ctx, cfg, refs, curs):
    """the records of one batch under option "deterministic": by default the schedule follows the batch and the host's timing, and
    records agree to the stopping rule's precision, not to the bit (include/dvo_hip.h)"""
    res = [d.Result() for _ in refs]
    ctx.set_option("deterministic", 1)
    try:
        d.DenseTracker(cfg, ctx).match_batch(refs, curs, res)
    finally:
        ctx.set_option("deterministic", 0)
    return records(res)


def test_deferred_colour_ingest_equals_the_immediate_one():
    w, h, n = 320, 240, 8
    ps = pairs_of(n, w, h)
    ctx = d.default_context()
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    out = []
    for flags in (0, _lib.INGEST_DEFER):
        cam = camera(ctx, w, h, ps[0][0]["K"], 4)
        refs, curs = blank_frames(cam, n), blank_frames(cam, n)
        d0 = ctx.counter("deferred_ingests")
        keep = run_update(refs, [in_format(x[1], "bgr8") for x in ps], [x[0]["depth_ref"] for x in ps], "bgr8", "device", "reference", 4, flags=flags)
        keep += run_update(curs, [in_format(x[2], "rgba8") for x in ps], [x[0]["depth_cur"] for x in ps], "rgba8", "device", "current", 4,
                           flags=flags)
        out.append(match_records(ctx, cfg, refs, curs))
        assert ctx.counter("deferred_ingests") - d0 == (2 if flags else 0)
        del keep
    assert_records_identical(out[0], out[1])


def test_whole_matches_against_oracle_and_grey_ingest():
    w, h, n = 320, 240, 32
    ps = pairs_of(n, w, h)
    ctx = d.default_context()
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    cam = camera(ctx, w, h, ps[0][0]["K"], 4)
    refs, curs = blank_frames(cam, n), blank_frames(cam, n)
    keep = run_update(refs, [in_format(x[1], "rgb8") for x in ps], [x[0]["depth_ref"] for x in ps], "rgb8", "device", "reference", 4)
    keep += run_update(curs, [in_format(x[2], "bgr8") for x in ps], [x[0]["depth_cur"] for x in ps], "bgr8", "host", "current", 4)
    colour = match_records(ctx, cfg, refs, curs)
    # the same engine fed the CPU conversion through the grey entry points of the same kind, in the same roles
    grefs, gcurs = blank_frames(cam, n), blank_frames(cam, n)
    gr = [torch.from_numpy(po.bgr_to_grey(x[1]).astype(np.uint8)).cuda() for x in ps]
    zr = [torch.from_numpy(x[0]["depth_ref"].astype(np.int16)).cuda() for x in ps]
    d.update_raw_device_batch(grefs, [t.data_ptr() for t in gr], [t.data_ptr() for t in zr], role="reference", config=config(4))
    gc = [np.ascontiguousarray(po.bgr_to_grey(x[2]).astype(np.uint8)) for x in ps]
    zc = [np.ascontiguousarray(x[0]["depth_cur"]) for x in ps]
    d.update_raw_host_batch(gcurs, gc, zc, role="current", config=config(4))
    d.upload_wait(ctx)
    assert_records_identical(colour, match_records(ctx, cfg, grefs, gcurs))
    ocfg = po.make_config(first_level=3, last_level=0, mode=po.MATH)
    for k in range(8):
        p = ps[k][0]
        o = po.match(oracle_pyramid(ps[k][1], p["depth_ref"], p["K"], 4), oracle_pyramid(ps[k][2], p["depth_cur"], p["K"], 4), ocfg)
        assert cm.twist_matrix_error(colour[k][0], o["T"]) <= 5e-5, k
    # a single match on colour-ingested frames: the grey-fed engine's record
    one, gone = d.Result(), d.Result()
    ctx.set_option("deterministic", 1)
    try:
        d.DenseTracker(cfg, ctx).match(refs[3], curs[3], one)
        d.DenseTracker(cfg, ctx).match(grefs[3], gcurs[3], gone)
    finally:
        ctx.set_option("deterministic", 0)
    assert_records_identical(records([one]), records([gone]))
    assert cm.twist_matrix_error(one.Transformation, colour[3][0]) <= 1e-6
    del keep


# ---- 6. TUM layout ----------------------------------------------------------------------------------------------------------------

def test_tum_rgb_png_through_create_colour(tmp_path):
    p, bgr, _ = scene("edge", 640, 480)
    rgb = np.ascontiguousarray(bgr[..., ::-1])
    tum.write_png(str(tmp_path / "rgb.png"), rgb)
    tum.write_png(str(tmp_path / "depth.png"), p["depth_ref"])
    back = tum.read_png(str(tmp_path / "rgb.png"))
    assert np.array_equal(back, rgb)
    grey, depth = tum.load_frame(str(tmp_path / "rgb.png"), str(tmp_path / "depth.png"))
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    a = cam.create_colour(back, depth, "rgb8")
    b = cam.create_raw(grey, depth)
    for l in range(4):
        for name in ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy"):
            assert np.array_equal(np.asarray(getattr(a.level(l), name)), np.asarray(getattr(b.level(l), name)), equal_nan=True), (l, name)


# ---- 7. errors leave the frames as they were --------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_change_nothing():
    p, bgr_ref, bgr_cur = scene("edge", 640, 480)
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    frames = blank_frames(cam, 2)
    run_update(frames, [in_format(bgr_ref, "bgr8"), in_format(bgr_cur, "bgr8")], [p["depth_ref"], p["depth_cur"]], "bgr8", "device", "reference", 4)
    t, ptr, _ = device_plane(in_format(bgr_cur, "bgr8"))
    tz = torch.from_numpy(p["depth_cur"].astype(np.int16)).cuda()
    L, vp = ctx._lib, C.c_void_p
    fr = (vp * 2)(frames[0].ptr, frames[1].ptr)
    good_c, good_z = (vp * 2)(ptr, ptr), (vp * 2)(tz.data_ptr(), tz.data_ptr())
    cfg = config(4).to_c()
    calls = [
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, fr, good_c, 0, 0, good_z, 2e-4, 1, C.byref(cfg), 0),
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, fr, good_c, 5, 0, good_z, 2e-4, -1, None, 0),
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, fr, (vp * 2)(ptr, None), 1, 0, good_z, 2e-4, 1, C.byref(cfg), 0),
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, fr, good_c, 1, 0, (vp * 2)(None, tz.data_ptr()), 2e-4, -1, None, 0),
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, fr, good_c, 1, 640 * 3 - 1, good_z, 2e-4, 0, C.byref(cfg), 0),
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, fr, good_c, 3, 640 * 3, good_z, 2e-4, -1, None, 1),
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, (vp * 2)(frames[0].ptr, None), good_c, 1, 0, good_z, 2e-4, -1, None, 0),
        lambda: L.dvo_hip_frames_update_colour_as_ex(ctx.ptr, 2, fr, good_c, 9, 0, good_z, 2e-4, -1, None, 0),
        lambda: L.dvo_hip_frames_update_colour_as_ex(ctx.ptr, 2, fr, (vp * 2)(None, None), 2, 0, good_z, 2e-4, -1, None, 0),
        lambda: L.dvo_hip_frames_update_colour_as_ex(ctx.ptr, 2, fr, good_c, 4, 100, good_z, 2e-4, 1, C.byref(cfg), 0),
    ]
    c0 = ctx.counter("colour_ingests")
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
    out = vp()
    K = np.ascontiguousarray(p["K"], np.float32)
    fp = K.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dvo_hip_frame_create_colour_device(ctx.ptr, 640, 480, fp, ptr, 7, 0, tz.data_ptr(), 2e-4, 4, C.byref(out)) == _lib.ERR_INVALID
    assert L.dvo_hip_frame_create_colour_device(ctx.ptr, 640, 480, fp, ptr, 1, 1000, tz.data_ptr(), 2e-4, 4, C.byref(out)) == _lib.ERR_INVALID
    assert L.dvo_hip_frame_create_colour(ctx.ptr, 640, 480, fp, None, 1, 0, None, 2e-4, 4, C.byref(out)) == _lib.ERR_INVALID
    assert not out.value
    assert ctx.counter("colour_ingests") == c0
    # A grey ingest of frames with differing level counts is refused like a colour one, before any frame is touched and before any
    # transfer is enqueued (frames of any level count share a camera).  The refused calls carry another depth scale and other thresholds
    # than frames[0] was ingested with: a frame whose marks the call had reset would derive its level 0 anew with those.
    short = blank_frames(camera(ctx, 640, 480, p["K"], 3), 1)[0]
    mixed = (vp * 2)(frames[0].ptr, short.ptr)
    tg = torch.full((480, 640), 77, dtype=torch.uint8, device="cuda")
    hg, hz = np.full((480, 640), 77, np.uint8), np.ascontiguousarray(p["depth_cur"], np.uint16)
    other = d.Config(FirstLevel=2, LastLevel=0, IntensityDerivativeThreshold=1.0, DepthDerivativeThreshold=0.5).to_c()
    s0 = ctx.counter("strip_ingests")
    assert L.dvo_hip_frames_update_raw_device(ctx.ptr, 2, mixed, (vp * 2)(tg.data_ptr(), tg.data_ptr()), good_z, 1e-3) == _lib.ERR_INVALID
    assert L.dvo_hip_frames_update_raw_as_ex(ctx.ptr, 2, mixed, (vp * 2)(hg.ctypes.data, hg.ctypes.data), (vp * 2)(hz.ctypes.data, hz.ctypes.data),
                                             1e-3, 1, C.byref(other), 0) == _lib.ERR_INVALID
    d.upload_wait(ctx)
    assert ctx.counter("strip_ingests") == s0
    # ... and frames[0] still serves as a reference: the record of a pair ingested the same way that no refused call has named
    control = blank_frames(cam, 2)
    run_update(control, [in_format(bgr_ref, "bgr8"), in_format(bgr_cur, "bgr8")], [p["depth_ref"], p["depth_cur"]], "bgr8", "device", "reference", 4)
    assert_records_identical(match_records(ctx, config(4), [frames[0]], [frames[1]]), match_records(ctx, config(4), [control[0]], [control[1]]))
    for f, bgr, z in ((frames[0], bgr_ref, p["depth_ref"]), (frames[1], bgr_cur, p["depth_cur"])):
        assert_frame_equals_oracle(f, oracle_pyramid(bgr, z, p["K"], 4), 4, "after refused calls")


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------

def test_cpp_facade_colour_pyramid_fills_level_0_host_mirrors():
    """tests/cpp/colour_facade_check.cpp: RgbdCameraPyramid::createFromColour's level 0 holds the converted grey on the device and, with
    host mirrors on, in its host matrices, point cloud and acceleration structure"""
    import subprocess
    from test_colour_ingest import build_colour_facade_check
    d.build()
    out = subprocess.run([build_colour_facade_check()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split() == ["ok", str(64 * 48)], (out.returncode, out.stdout, out.stderr)
