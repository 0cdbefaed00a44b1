"""GPU tier (-m gpu): the float-plane ingest (dvo_hip_frame_create_f32_device, dvo_hip_frames_update_f32*,
dvo_hip_frames_update_colour_f32depth*) against the oracle's image model, bit for bit: all six planes of every level, selection counts
and masks at two threshold pairs.  The yardstick is po.Pyramid(intensity_f32, depth_f32, K, levels) -- for an 8-bit image with float depth
po.Pyramid(po.bgr_to_grey(colour), depth_f32, K, levels).

The inputs cannot pass through the 8 / 16-bit path: the intensity is a scene's grey plus a smooth sub-level ripple, the depth the scene's
depth * 2e-4 plus a smooth offset below 1e-4 m (no multiple of any u16 quantum), with the scenes' NaN holes at odd coordinates and on
strip borders.  The path each ingest took (strip or tile kernel) is asserted through the counters "strip_ingests" / "f32_ingests"."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest
import torch

import common as cm
import dvo_slam_amd as d
import scenes
from dvo_slam_amd import _lib
from oracle import pyoracle as po
from test_gpu_colour_ingest import assert_records_identical, in_format, match_records, tinted
from test_gpu_scene_edges import assert_frame_equals_oracle
from test_gpu_selection import masks_of

pytestmark = pytest.mark.gpu
THR = (6.0, 0.03)
ROLES = (None, "current", "reference")
MIXED = ("grey8", "bgr8", "rgb8", "bgra8", "rgba8")


def float_planes(grey_u8, depth_u16, seed):
    """(intensity f32 with fractional values, depth f32 in metres off every u16 quantum, NaN where the raw depth is 0)"""
    h, w = grey_u8.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = np.random.default_rng(seed).uniform(0, 6.28, 2)
    i = np.clip(grey_u8.astype(np.float64) + 0.45 * np.sin(x / 9.0 + ph[0]) * np.cos(y / 7.0), 0.0, 255.0).astype(np.float32)
    z = depth_u16.astype(np.float64) * 2e-4 + 0.9e-4 * np.sin(x / 13.0 + y / 17.0 + ph[1])
    z = np.where(depth_u16 == 0, np.nan, z).astype(np.float32)
    assert np.any(i != np.rint(i)) and np.isnan(z).any()
    return np.ascontiguousarray(i), np.ascontiguousarray(z)


@functools.lru_cache(maxsize=None)
def scene(kind, w, h):
    p = scenes.edge_scene(3, w, h) if kind == "edge" else cm.synth(5, w, h)
    ir, zr = float_planes(p["grey_ref"], p["depth_ref"], 1)
    ic, zc = float_planes(p["grey_cur"], p["depth_cur"], 2)
    return p, (ir, zr), (ic, zc)


def camera(ctx, w, h, K, levels):
    cam = d.RgbdCameraPyramid(w, h, K, ctx)
    cam.build(levels)
    return cam


def blank_frames(cam, n):
    w, h = cam.width, cam.height
    return [cam.create_raw(np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint16)) for _ in range(n)]


def device_bytes(arr, offset=0, pad=0):
    """(tensor, address, pitch) of the rows of `arr` (any dtype, [h, w] or [h, w, c]) in device memory: `offset` bytes into a 256-byte
    aligned allocation, rows padded by `pad` bytes"""
    h = arr.shape[0]
    row = np.ascontiguousarray(arr).view(np.uint8).reshape(h, -1)
    pitch = row.shape[1] + pad
    host = np.zeros(offset + pitch * h + 16, np.uint8)
    host[offset:offset + pitch * h].reshape(h, pitch)[:, :row.shape[1]] = row
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 8 == 0
    return t, t.data_ptr() + offset, pitch


def host_view(arr, pad=0):
    """`arr` as a view into a buffer whose rows are `pad` bytes longer"""
    h = arr.shape[0]
    row = np.ascontiguousarray(arr).view(np.uint8).reshape(h, -1)
    buf = np.zeros((h, row.shape[1] + pad), np.uint8)
    buf[:, :row.shape[1]] = row
    return buf[:, :row.shape[1]].view(arr.dtype).reshape(arr.shape)


def config(levels):
    return d.Config(FirstLevel=levels - 1, LastLevel=0, IntensityDerivativeThreshold=THR[0], DepthDerivativeThreshold=THR[1])


def counters(ctx):
    return ctx.counter("strip_ingests"), ctx.counter("f32_ingests")


def run_f32(frames, ints, deps, entry, role, levels, ioff=0, ipad=0, zoff=0, zpad=0, flags=0, depth_scale=1.0):
    keep = []
    cfg = config(levels) if role else None
    if entry == "device":
        iptrs, zptrs = [], []
        for i, z in zip(ints, deps):
            ti, pi, ipitch = device_bytes(i, ioff, ipad)
            tz, pz, zpitch = device_bytes(z, zoff, zpad)
            keep += [ti, tz]
            iptrs.append(pi)
            zptrs.append(pz)
        d.update_f32_device_batch(frames, iptrs, zptrs, ipitch, zpitch, depth_scale, role=role, config=cfg, flags=flags)
    else:
        hi, hz = [host_view(i, ipad) for i in ints], [host_view(z, zpad) for z in deps]
        keep += hi + hz
        d.update_f32_host_batch(frames, hi, hz, depth_scale, role=role, config=cfg, flags=flags)
        d.upload_wait(frames[0].ctx)
    torch.cuda.synchronize()
    return keep


def run_mixed(frames, colours, deps, fmt, entry, role, levels, cpad=0, zpad=0, flags=0):
    keep = []
    cfg = config(levels) if role else None
    if entry == "device":
        cptrs, zptrs = [], []
        for c, z in zip(colours, deps):
            tc, pc, cpitch = device_bytes(c, 0, cpad)
            tz, pz, zpitch = device_bytes(z, 0, zpad)
            keep += [tc, tz]
            cptrs.append(pc)
            zptrs.append(pz)
        d.update_colour_device_batch(frames, cptrs, zptrs, fmt, cpitch, 1.0, role=role, config=cfg, flags=flags, depth_format="f32", depth_pitch=zpitch)
    else:
        hc, hz = [host_view(c, cpad) for c in colours], [host_view(z, zpad) for z in deps]
        keep += hc + hz
        d.update_colour_host_batch(frames, hc, hz, fmt, 1.0, role=role, config=cfg, flags=flags, depth_format="f32")
        d.upload_wait(frames[0].ctx)
    torch.cuda.synchronize()
    return keep


# ---- 1. planes and selection on every path ----------------------------------------------------------------------------------------

# (kind, w, h, image offset, image padding, depth offset, depth padding, strip path) -- offsets and paddings in bytes
SHAPES = [("edge", 640, 480, 0, 0, 0, 0, True), ("edge", 640, 480, 0, 64, 0, 24, True), ("edge", 321, 240, 0, 0, 0, 0, False),
          ("synth", 17, 5, 0, 0, 0, 0, False), ("edge", 640, 480, 4, 0, 0, 0, False), ("edge", 640, 480, 0, 0, 4, 0, False)]
SHAPE_ID = lambda s: "%s%dx%d_i%d+%d_z%d+%d" % s[:7]   # noqa: E731


def check_f32(shape, role, entry):
    kind, w, h, ioff, ipad, zoff, zpad, strip = shape
    p, ref, cur = scene(kind, w, h)
    levels = 2 if h < 16 else 4
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], levels)
    frames = blank_frames(cam, 2)
    s0, f0 = counters(ctx)
    keep = run_f32(frames, [ref[0], cur[0]], [ref[1], cur[1]], entry, role, levels, ioff, ipad, zoff, zpad)
    if entry == "host":
        strip = w % 2 == 0                    # (host planes arrive in the upload buffer with tight rows, whatever the caller's pitch)
    assert counters(ctx) == (s0 + (2 if strip else 0), f0 + 2), (shape, role, entry)
    for f, (i, z) in ((frames[0], ref), (frames[1], cur)):
        assert_frame_equals_oracle(f, po.Pyramid(i, z, p["K"], levels), levels, (shape, role, entry))
    del keep


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("role", ROLES, ids=str)
def test_planes_and_selection_device(shape, role):
    check_f32(shape, role, "device")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] == 0 and s[5] == 0], ids=SHAPE_ID)
@pytest.mark.parametrize("role", ROLES, ids=str)
def test_planes_and_selection_host(shape, role):
    check_f32(shape, role, "host")


# ---- 2. an 8-bit image with float depth ---------------------------------------------------------------------------------------------

# (kind, w, h, image padding, depth padding, strip path when the planes are tight-rowed and aligned)
MIXED_SHAPES = [("edge", 640, 480, 0, 0), ("edge", 640, 480, 64, 24), ("edge", 321, 240, 0, 0), ("synth", 17, 5, 0, 0)]


def mixed_image(grey_u8, fmt, seed):
    """(the plane handed over, the oracle's intensity)"""
    if fmt == "grey8":
        return np.ascontiguousarray(grey_u8[..., None]), grey_u8.astype(np.float32)
    bgr = tinted(grey_u8, seed)
    return in_format(bgr, fmt), po.bgr_to_grey(bgr)


@pytest.mark.parametrize("shape", MIXED_SHAPES, ids=lambda s: "%s%dx%d_c+%d_z+%d" % s)
@pytest.mark.parametrize("role", ROLES, ids=str)
@pytest.mark.parametrize("fmt", MIXED)
@pytest.mark.parametrize("entry", ("device", "host"))
def test_mixed_planes_and_selection(shape, role, fmt, entry):
    kind, w, h, cpad, zpad = shape
    p, ref, cur = scene(kind, w, h)
    levels = 2 if h < 16 else 4
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], levels)
    frames = blank_frames(cam, 2)
    cr, gr = mixed_image(p["grey_ref"], fmt, 1)
    cc, gc = mixed_image(p["grey_cur"], fmt, 2)
    s0, f0 = counters(ctx)
    c0 = ctx.counter("colour_ingests")
    keep = run_mixed(frames, [cr, cc], [ref[1], cur[1]], fmt, entry, role, levels, cpad, zpad)
    strip = w % 4 == 0                        # (8-bit rows: 4 pixels; the paddings keep every row aligned)
    assert counters(ctx) == (s0 + (2 if strip else 0), f0 + 2), (shape, role, fmt, entry)
    assert ctx.counter("colour_ingests") == c0 + (0 if fmt == "grey8" else 2)
    for f, g, z in ((frames[0], gr, ref[1]), (frames[1], gc, cur[1])):
        assert_frame_equals_oracle(f, po.Pyramid(g, z, p["K"], levels), levels, (shape, role, fmt, entry))
    del keep


# ---- 3. create from device planes = create from host planes -------------------------------------------------------------------------

NAMES = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")


def assert_frames_equal(a, b, levels, what):
    for l in range(levels):
        for name in NAMES:
            x, y = np.asarray(getattr(a.level(l), name)), np.asarray(getattr(b.level(l), name))
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, l, name)
        for thr in ((0.0, 0.0), THR):
            na, ma = d.PointSelection(a, *thr).select(l, want_mask=True)
            nb, mb = d.PointSelection(b, *thr).select(l, want_mask=True)
            assert na == nb and np.array_equal(ma, mb), (what, l, thr)


@pytest.mark.parametrize("kind,w,h", [("edge", 640, 480), ("edge", 321, 240), ("synth", 17, 5)])
def test_create_f32_device_equals_create_f32(kind, w, h):
    p, ref, _ = scene(kind, w, h)
    levels = 2 if h < 16 else 4
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], levels)
    ti, tz = torch.from_numpy(ref[0]).cuda(), torch.from_numpy(ref[1]).cuda()
    s0, f0 = counters(ctx)
    a = cam.create_f32_device(ti.data_ptr(), tz.data_ptr())
    a.level(0)
    assert counters(ctx) == (s0 + (1 if w % 2 == 0 else 0), f0 + 1)
    b = cam.create(ref[0], ref[1])
    assert_frames_equal(a, b, levels, (kind, w, h))
    assert_frame_equals_oracle(a, po.Pyramid(ref[0], ref[1], p["K"], levels), levels, (kind, w, h))


# ---- 4. special float depths ----------------------------------------------------------------------------------------------------------

def sprinkled(z, seed):
    z = z.copy()
    rng = np.random.default_rng(seed)
    h, w = z.shape
    for k, v in enumerate((0.0, -1.25, np.inf, -np.inf, -0.0)):
        n = max(6, w * h // 900)
        z[rng.integers(0, h, n), rng.integers(0, w, n)] = v
        z[(7 + k) % h, (126 + k) % w] = v                     # next to a strip border
    return z


@pytest.mark.parametrize("entry", ("device", "host"))
@pytest.mark.parametrize("role", ROLES, ids=str)
@pytest.mark.parametrize("kind,w,h", [("edge", 640, 480), ("edge", 321, 240)])
def test_zero_negative_and_infinite_depths_are_taken_as_create_f32_takes_them(entry, role, kind, w, h):
    p, ref, _ = scene(kind, w, h)
    z = sprinkled(ref[1], 9)
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], 4)
    frames = blank_frames(cam, 1)
    keep = run_f32(frames, [ref[0]], [z], entry, role, 4)
    with np.errstate(invalid="ignore"):
        assert_frames_equal(frames[0], cam.create(ref[0], z), 4, (entry, role, w))
    got = np.asarray(frames[0].level(0).depth)
    assert np.array_equal(got.view(np.uint32)[~np.isnan(z)], z.view(np.uint32)[~np.isnan(z)])      # 0, -0, negative, +-inf: as they are
    assert np.array_equal(np.isnan(got), np.isnan(z))
    del keep


@pytest.mark.parametrize("entry", ("device", "host"))
@pytest.mark.parametrize("role", ROLES, ids=str)
def test_depth_scale_of_a_millimetre_plane(entry, role):
    p, ref, _ = scene("edge", 640, 480)
    mm = (ref[1].astype(np.float64) * 1000.0).astype(np.float32)
    want = np.float32(mm) * np.float32(1e-3)
    assert np.any(want != ref[1])
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    frames = blank_frames(cam, 1)
    keep = run_f32(frames, [ref[0]], [mm], entry, role, 4, depth_scale=1e-3)
    assert_frame_equals_oracle(frames[0], po.Pyramid(ref[0], want, p["K"], 4), 4, (entry, role))
    del keep


# ---- 5. the raw copy ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ("device", "host"))
@pytest.mark.parametrize("source", ("f32", "bgr8"))
def test_raw_copy_serves_the_other_role(entry, source):
    p, ref, cur = scene("edge", 640, 480)
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    frames = blank_frames(cam, 2)
    if source == "f32":
        keep = run_f32(frames, [ref[0], cur[0]], [ref[1], cur[1]], entry, "reference", 4)
        ints = [ref[0], cur[0]]
    else:
        (cr, gr), (cc, gc) = mixed_image(p["grey_ref"], source, 1), mixed_image(p["grey_cur"], source, 2)
        keep = run_mixed(frames, [cr, cc], [ref[1], cur[1]], source, entry, "reference", 4)
        ints = [gr, gc]
    d.prepare_roles_batch(frames, "current", d.Config(FirstLevel=3, LastLevel=0))
    for f, i, z in ((frames[0], ints[0], ref[1]), (frames[1], ints[1], cur[1])):
        assert_frame_equals_oracle(f, po.Pyramid(i, z, p["K"], 4), 4, (entry, source))   # (also reselects at other thresholds)
    del keep


def test_no_raw_copy_refuses_the_other_role_and_keeps_the_frame():
    p, ref, _ = scene("edge", 640, 480)
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    frames = blank_frames(cam, 1)
    keep = run_f32(frames, [ref[0]], [ref[1]], "device", "reference", 4, flags=_lib.INGEST_NO_RAW_COPY)
    o = po.Pyramid(ref[0], ref[1], p["K"], 4)
    with pytest.raises(d.DvoHipError) as e:
        d.prepare_roles_batch(frames, "current", d.Config(FirstLevel=3, LastLevel=0))
    assert e.value.code == _lib.ERR_INVALID
    assert d.PointSelection(frames[0], *THR).select(0) == o.select(0, *THR)[0]   # (the mask needs the current role: not here)
    for l in range(1, 4):
        for k, name in enumerate(("intensity", "depth")):
            assert np.array_equal(np.asarray(getattr(frames[0].level(l), name)), o.plane(l, k)[0], equal_nan=True), (l, name)
    with pytest.raises(d.DvoHipError):
        d.PointSelection(frames[0], 0.0, 0.0).select(0)
    del keep


@pytest.mark.parametrize("role", ("reference", "current"))
def test_a_frame_alternates_between_u16_and_float_ingests(role):
    p, ref, cur = scene("edge", 640, 480)
    ctx = d.default_context()
    cam = camera(ctx, 640, 480, p["K"], 4)
    frames = blank_frames(cam, 1)
    other = "current" if role == "reference" else "reference"
    tg = torch.from_numpy(p["grey_cur"]).cuda()
    tz = torch.from_numpy(p["depth_cur"].astype(np.int16)).cuda()
    o_raw = po.Pyramid(p["grey_cur"].astype(np.float32), po.convert_raw_depth(p["depth_cur"]), p["K"], 4)
    o_f32 = po.Pyramid(ref[0], ref[1], p["K"], 4)
    keep = []
    for step in ("u16", "f32", "u16", "f32 host", "u16"):
        if step == "u16":
            d.update_raw_device_batch(frames, [tg.data_ptr()], [tz.data_ptr()], 2e-4, role=role, config=config(4))
            want = o_raw
        else:
            keep += run_f32(frames, [ref[0]], [ref[1]], "host" if "host" in step else "device", role, 4)
            want = o_f32
        torch.cuda.synchronize()
        d.prepare_roles_batch(frames, other, config(4))
        assert_frame_equals_oracle(frames[0], want, 4, (role, step))
    del keep


# ---- 6. the caller selection survives ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ("device", "host"))
@pytest.mark.parametrize("role", ROLES, ids=str)
def test_caller_selection_survives_a_float_reingest(entry, role):
    w, h = 640, 480
    p, ref, cur = scene("edge", w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], 4)
    frames = blank_frames(cam, 1)
    mask0 = masks_of("blocks", 1, w, h)
    zmin, zmax = 0.8, 2.6
    frames[0].set_selection(mask0, zmin, zmax)
    keep = run_f32(frames, [cur[0]], [cur[1]], entry, role, 4)
    keep += run_f32(frames, [ref[0]], [ref[1]], entry, role, 4)
    o = po.Pyramid(ref[0], ref[1], p["K"], 4)
    for thr in (THR, (0.0, 0.0)):
        sel = d.PointSelection(frames[0], *thr)
        for l in range(4):
            _, m_o = o.select(l, *thr)
            z, _ = o.plane(l, 1)
            hl, wl = m_o.shape
            with np.errstate(invalid="ignore"):
                want = (m_o != 0) & (mask0[::2 ** l, ::2 ** l][:hl, :wl] != 0) & (z >= zmin) & (z <= zmax)
            n, m = sel.select(l, want_mask=True)
            assert np.array_equal(m != 0, want) and n == int(want.sum()), (entry, role, thr, l)
            assert sel.select(l) == n
    frames[0].clear_selection()
    assert d.PointSelection(frames[0], *THR).select(0) == o.select(0, *THR)[0]
    del keep


# ---- 7. deferred = immediate, 8. whole matches ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pairs_of(n, w, h):
    out = []
    for k in range(n):
        p = cm.synth(100 + k % 8, w, h)
        out.append((p, float_planes(p["grey_ref"], p["depth_ref"], 10 + k), float_planes(p["grey_cur"], p["depth_cur"], 50 + k)))
    return out


def test_deferred_float_ingest_equals_the_immediate_one():
    w, h, n = 320, 240, 8
    ps = pairs_of(n, w, h)
    ctx = d.default_context()
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    out = []
    for flags in (0, _lib.INGEST_DEFER):
        cam = camera(ctx, w, h, ps[0][0]["K"], 4)
        refs, curs = blank_frames(cam, n), blank_frames(cam, n)
        d0 = ctx.counter("deferred_ingests")
        keep = run_f32(refs, [x[1][0] for x in ps], [x[1][1] for x in ps], "device", "reference", 4, ipad=32, zpad=8, flags=flags)
        bgr = [tinted(x[0]["grey_cur"], 20 + k) for k, x in enumerate(ps)]
        keep += run_mixed(curs, [in_format(b, "rgba8") for b in bgr], [x[2][1] for x in ps], "rgba8", "device", "current", 4, cpad=16, zpad=40,
                          flags=flags)
        out.append(match_records(ctx, cfg, refs, curs))
        assert ctx.counter("deferred_ingests") - d0 == (2 if flags else 0)
        del keep
    assert_records_identical(out[0], out[1])


def test_whole_matches_against_create_f32_and_the_oracle():
    w, h, n = 320, 240, 32
    ps = pairs_of(n, w, h)
    ctx = d.default_context()
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    cam = camera(ctx, w, h, ps[0][0]["K"], 4)
    refs, curs = blank_frames(cam, n), blank_frames(cam, n)
    keep = run_f32(refs, [x[1][0] for x in ps], [x[1][1] for x in ps], "device", "reference", 4)
    keep += run_f32(curs, [x[2][0] for x in ps], [x[2][1] for x in ps], "host", "current", 4)
    got = match_records(ctx, cfg, refs, curs)
    # the same engine fed the same float planes the only way it took them before: one frame construction each
    crefs = [cam.create(x[1][0], x[1][1]) for x in ps]
    ccurs = [cam.create(x[2][0], x[2][1]) for x in ps]
    assert_records_identical(got, match_records(ctx, cfg, crefs, ccurs))
    ocfg = po.make_config(first_level=3, last_level=0, mode=po.MATH)
    for k in range(8):
        K = ps[k][0]["K"]
        o = po.match(po.Pyramid(ps[k][1][0], ps[k][1][1], K, 4), po.Pyramid(ps[k][2][0], ps[k][2][1], K, 4), ocfg)
        assert cm.twist_matrix_error(got[k][0], o["T"]) <= 5e-5, k
    del keep


# ---- 9. errors change nothing -----------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_change_nothing():
    w, h = 640, 480
    p, ref, cur = scene("edge", w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, p["K"], 4)
    frames = blank_frames(cam, 2)
    keep = run_f32(frames, [ref[0], cur[0]], [ref[1], cur[1]], "device", "reference", 4)
    ti, tz = torch.from_numpy(cur[0]).cuda(), torch.from_numpy(cur[1]).cuda()
    tu = torch.from_numpy(p["depth_cur"].astype(np.int16)).cuda()
    tc = torch.from_numpy(in_format(tinted(p["grey_cur"], 2), "bgr8")).cuda()
    L, vp = ctx._lib, C.c_void_p
    fr = (vp * 2)(frames[0].ptr, frames[1].ptr)
    gi, gz, gc = (vp * 2)(ti.data_ptr(), ti.data_ptr()), (vp * 2)(tz.data_ptr(), tz.data_ptr()), (vp * 2)(tc.data_ptr(), tc.data_ptr())
    hi, hz = (vp * 2)(cur[0].ctypes.data, cur[0].ctypes.data), (vp * 2)(cur[1].ctypes.data, cur[1].ctypes.data)
    zu = np.ascontiguousarray(p["depth_cur"], np.uint16)
    gu, hu = (vp * 2)(tu.data_ptr(), tu.data_ptr()), (vp * 2)(zu.ctypes.data, zu.ctypes.data)
    short = blank_frames(camera(ctx, w, h, p["K"], 3), 1)[0]
    mixed_levels = (vp * 2)(frames[0].ptr, short.ptr)
    other = d.Config(FirstLevel=2, LastLevel=0, IntensityDerivativeThreshold=1.0, DepthDerivativeThreshold=0.5).to_c()
    big = 2 ** 31
    f32d, f32h = L.dvo_hip_frames_update_f32_device_as_ex, L.dvo_hip_frames_update_f32_as_ex
    mixd, mixh = L.dvo_hip_frames_update_colour_f32depth_device_as_ex, L.dvo_hip_frames_update_colour_f32depth_as_ex
    calls = [
        lambda: mixd(ctx.ptr, 2, fr, gc, 9, 0, gz, 0, 0.5, 1, C.byref(other), 0),                       # an unknown format
        lambda: mixd(ctx.ptr, 2, fr, gc, 5, 0, gz, 0, 0.5, -1, None, 0),                                # (a float image is not an 8-bit one)
        lambda: mixh(ctx.ptr, 2, fr, gc, -1, 0, hz, 0, 0.5, -1, None, 0),
        lambda: L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, 2, fr, gi, 5, 0, gu, 0.5, -1, None, 0),   # F32 image + U16 depth
        lambda: L.dvo_hip_frames_update_colour_as_ex(ctx.ptr, 2, fr, hi, 5, 0, hu, 0.5, 1, C.byref(other), 0),
        lambda: f32d(ctx.ptr, 2, fr, None, 0, gz, 0, 0.5, 1, C.byref(other), 0),                        # a null array
        lambda: f32d(ctx.ptr, 2, fr, gi, 0, None, 0, 0.5, -1, None, 0),
        lambda: f32d(ctx.ptr, 2, fr, (vp * 2)(ti.data_ptr(), None), 0, gz, 0, 0.5, 1, C.byref(other), 0),   # a null entry
        lambda: f32h(ctx.ptr, 2, fr, hi, 0, (vp * 2)(None, cur[1].ctypes.data), 0, 0.5, -1, None, 0),
        lambda: f32d(ctx.ptr, 2, (vp * 2)(frames[0].ptr, None), gi, 0, gz, 0, 0.5, -1, None, 0),
        lambda: f32d(ctx.ptr, 2, fr, gi, w * 4 - 4, gz, 0, 0.5, 0, C.byref(other), 0),                  # a pitch below width * 4
        lambda: f32d(ctx.ptr, 2, fr, gi, 0, gz, w * 4 - 4, 0.5, -1, None, 0),
        lambda: f32h(ctx.ptr, 2, fr, hi, 0, hz, w * 4 - 8, 0.5, 1, C.byref(other), 0),
        lambda: mixd(ctx.ptr, 2, fr, gc, 1, w * 3 - 1, gz, 0, 0.5, -1, None, 0),
        lambda: mixd(ctx.ptr, 2, fr, gc, 1, 0, gz, w * 4 - 4, 0.5, -1, None, 0),
        lambda: f32d(ctx.ptr, 2, fr, gi, big, gz, 0, 0.5, -1, None, 0),                                 # a pitch above 2^31 - 1
        lambda: f32d(ctx.ptr, 2, fr, gi, 0, gz, big, 0.5, 1, C.byref(other), 0),
        lambda: mixh(ctx.ptr, 2, fr, gc, 1, 0, hz, big + 4, 0.5, -1, None, 0),
        lambda: f32d(ctx.ptr, 2, mixed_levels, gi, 0, gz, 0, 0.5, 1, C.byref(other), 0),                # frames of differing level counts
        lambda: f32h(ctx.ptr, 2, mixed_levels, hi, 0, hz, 0, 0.5, -1, None, 0),
        lambda: mixd(ctx.ptr, 2, mixed_levels, gc, 1, 0, gz, 0, 0.5, 1, C.byref(other), 0),
        lambda: f32h(ctx.ptr, 2, fr, hi, 0, hz, 0, 0.5, 1, C.byref(other), _lib.INGEST_DEFER),          # DEFER on a host entry point
        lambda: mixh(ctx.ptr, 2, fr, gc, 1, 0, hz, 0, 0.5, -1, None, _lib.INGEST_DEFER),
        lambda: f32d(ctx.ptr, 2, fr, gi, 0, gz, 0, 0.5, 2, C.byref(other), 0),                          # no such role
        lambda: f32d(ctx.ptr, 2, fr, gi, 0, gz, 0, 0.5, 1, None, 0),                                    # a role without a config
    ]
    names = ("strip_ingests", "f32_ingests", "colour_ingests", "deferred_ingests")
    before = [ctx.counter(k) for k in names]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, k
        assert [ctx.counter(c) for c in names] == before, k
    # the creation from device planes refuses what the checker refuses
    out = vp()
    K = np.ascontiguousarray(p["K"], np.float32)
    fp = K.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dvo_hip_frame_create_f32_device(ctx.ptr, w, h, fp, None, tz.data_ptr(), 4, C.byref(out)) == _lib.ERR_INVALID
    assert L.dvo_hip_frame_create_f32_device(ctx.ptr, w, h, fp, ti.data_ptr(), tz.data_ptr() + 2, 4, C.byref(out)) == _lib.ERR_INVALID
    assert not out.value
    d.upload_wait(ctx)
    assert [ctx.counter(c) for c in names] == before
    # the pair ingested before the refused calls still produces the record of a control pair no refused call has named
    control = blank_frames(cam, 2)
    keep += run_f32(control, [ref[0], cur[0]], [ref[1], cur[1]], "device", "reference", 4)
    assert_records_identical(match_records(ctx, config(4), [frames[0]], [frames[1]]), match_records(ctx, config(4), [control[0]], [control[1]]))
    for f, (i, z) in ((frames[0], ref), (frames[1], cur)):
        assert_frame_equals_oracle(f, po.Pyramid(i, z, p["K"], 4), 4, "after refused calls")
    del keep, tu


# ---- 10. the C++ facade -----------------------------------------------------------------------------------------------------------------

def test_cpp_facade_update_and_device_planes():
    """tests/cpp/f32_facade_check.cpp: RgbdImagePyramid::update keeps the frame handle and the selection and matches like a fresh pair;
    RgbdCameraPyramid::createFromFloatDevice fills level 0's host mirrors"""
    from test_f32_ingest import build_f32_facade_check
    d.build()
    out = subprocess.run([build_f32_facade_check()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split() == ["ok"], (out.returncode, out.stdout, out.stderr)
