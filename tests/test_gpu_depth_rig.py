"""GPU tier: frames that carry a depth rig have their depth plane registered into the colour camera on the device at ingest
(include/dvo_hip.h, dvo_hip_frames_set_depth_rig; k_depth_fill + k_depth_register).  The yardstick is reg(P), the host build of
dvo_slam_amd/csrc/depth_rig.h (tests/test_depth_rig.py, reg): a rigged frame ingested from the image plane and the depth sensor's plane P
equals, bit for bit, its rig-less TWIN fed the same image plane and reg(P) through the float-depth entry point of that image format.
  1. every level, plane, selection and match record on every entry-point family, host and device, every role, strip, odd and ragged sizes;
  2. many sources into one target: level 0 against the yardstick on a scene with a depth step (the atomic minimum's order does not matter);
  3. the identity rig is the plain ingest;
  4. rig plus lens;
  5. flags and lifetime: deferred, pending, no raw copy, replaced, cleared, grown;
  6. refusals change nothing;
  7. counters, the table, a mixed batch in match_batch;
  8. the C++ facade."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import test_depth_rig as tdr
import test_lens as tl
from dvo_slam_amd import _lib
from test_gpu_colour_ingest import assert_records_identical, in_format, match_records
from test_gpu_f32_ingest import assert_frames_equal, blank_frames, camera, config, device_bytes
from test_gpu_lens_ingest import SCALE, ingest, raw_scene, source

pytestmark = pytest.mark.gpu
ROLES = (None, "current", "reference")


def twin_family(family):
    """the float-depth entry point of an image format: a float image stays with update_f32_*, every 8-bit one goes to update_colour_f32depth_*"""
    return "f32" if family == "f32" else "mixed"


def feed_twin(twins, images, planes, family, fmt, entry, role, levels, ipad=0, flags=0):
    images = [np.ascontiguousarray(i[..., None]) if i.ndim == 2 and i.dtype == np.uint8 else i for i in images]   # (grey8 as a colour format: [h, w, 1])
    return ingest(twins, images, planes, twin_family(family), fmt, 1.0, entry, role, levels, ipad, 0, flags)


def counters(ctx):
    return tuple(ctx.counter(k) for k in ("depth_registrations", "f32_ingests", "colour_ingests", "lens_ingests"))


# ---- 1. a rigged frame equals its twin ------------------------------------------------------------------------------------------------

FAMILIES = [("raw", "grey8"), ("colour", "bgr8"), ("mixed", "rgb8"), ("f32", "f32")]
SHAPES = [(128, 96), (321, 240), (102, 78)]            # strip path; odd width (fill tail, tile kernel); a width no multiple of 64 or 4


def cases():
    """every family x entry x role, with shape and padding cycling so that each shape meets each role, each entry and each family"""
    out, i = [], 0
    for family, fmt in FAMILIES:
        for entry in ("device", "host"):
            for role in ROLES:
                shape = SHAPES[(i + i // 3) % 3]
                pad = 0 if family == "raw" else (0, 8)[(i + i // 3) % 2]
                out.append(pytest.param(family, fmt, entry, role, shape, pad, id="%s-%s-%s-%s-%dx%d-pad%d" % ((family, fmt, entry, role) + shape + (pad,))))
                i += 1
    return out


@pytest.mark.parametrize("family,fmt,entry,role,shape,pad", cases())
def test_rigged_frame_equals_its_twin(family, fmt, entry, role, shape, pad):
    w, h = shape
    K, views = raw_scene(w, h)
    levels = 4 if h >= 240 else 3
    K_depth, T = tdr.kinect_rig(K)
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    d.set_depth_rig_batch(frames, K_depth, T)
    src = [source(v, family, fmt) for v in views]
    scale = src[0][3]
    zpad = pad // 2 * 4 if src[0][2].dtype == np.float32 else 0   # (a padded pitch for the float sources)
    c0 = counters(ctx)
    keep = ingest(frames, [s[0] for s in src], [s[2] for s in src], family, fmt, scale, entry, role, levels, pad, zpad)
    colour = 2 if family in ("colour", "mixed") else 0
    assert counters(ctx) == (c0[0] + 2, c0[1] + 2, c0[2] + colour, c0[3])
    planes = [tdr.reg(s[2], K, K_depth, T, scale) for s in src]
    assert all(np.isnan(Z).any() and np.isfinite(Z).any() for Z in planes)
    keep += feed_twin(twins, [s[0] for s in src], planes, family, fmt, entry, role, levels, pad)
    assert counters(ctx) == (c0[0] + 2, c0[1] + 4, c0[2] + 2 * colour, c0[3])      # (the twins carry no rig)
    what = (family, fmt, entry, role, shape, pad)
    for f, t in zip(frames, twins):
        assert_frames_equal(f, t, levels, what)
    cfg = config(levels)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), match_records(ctx, cfg, twins[:1], twins[1:]))
    del keep


# ---- 2. many into one -------------------------------------------------------------------------------------------------------------------

def plane_of(frame, level=0):
    torch.cuda.synchronize()
    return np.array(frame.level(level).intensity, copy=True), np.array(frame.level(level).depth, copy=True)


def step_depth(w, h):
    """a wall at 2.5-3.5 m behind a slab at 0.8 m and a thin post at 0.5 m, with holes: several sources per target, occlusion, hole bands"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 2.5 + x / w + 0.2 * np.sin(y / 9.0)
    z[h // 5:4 * h // 5, w // 3:w // 2] = 0.8 + 0.05 * y[h // 5:4 * h // 5, w // 3:w // 2] / h
    z[:, 3 * w // 4:3 * w // 4 + 5] = 0.5
    depth = np.rint(z * 5000).astype(np.uint16)
    depth[np.random.default_rng(5).random((h, w)) < 0.03] = 0
    return depth


@pytest.mark.parametrize("w,h,fmt", [(321, 240, "u16"), (102, 78, "f32"), (640, 480, "u16")])
def test_level_0_equals_the_yardstick_on_a_depth_step(w, h, fmt):
    K = tdr.scaled_K(w)
    K_depth, T = tdr.kinect_rig(K)
    depth = step_depth(w, h)
    grey = (depth >> 6).astype(np.uint8)
    ctx = d.default_context()
    frames = blank_frames(camera(ctx, w, h, K, 3), 1)
    d.set_depth_rig_batch(frames, K_depth, T)
    if fmt == "f32":
        depth = (depth.astype(np.float32) * np.float32(2e-4)).astype(np.float32)
        depth[depth == 0] = np.nan
        keep = ingest(frames, [grey[..., None]], [depth], "mixed", "grey8", 0.5, "device", None, 3, 0, 12)
        want = tdr.reg(depth, K, K_depth, T, 0.5)
    else:
        keep = ingest(frames, [grey], [depth], "raw", "grey8", SCALE, "device", None, 3)
        want = tdr.reg(depth, K, K_depth, T, SCALE)
    at, _ = tdr.project(depth, K, K_depth, T, 0.5 if fmt == "f32" else SCALE)
    landed = np.bincount(at[at >= 0], minlength=w * h)
    assert (landed > 1).mean() > 0.1 and landed.max() >= 3                      # many into one, and more than two
    I, Z = plane_of(frames[0])
    assert np.array_equal(Z.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(I, grey.astype(np.float32))
    del keep


# ---- 3. the identity rig ----------------------------------------------------------------------------------------------------------------

def test_identity_rig_on_u16_depth_equals_the_plain_ingest():
    w, h, levels = 321, 240, 3
    K, views = raw_scene(w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    frames, plain = blank_frames(cam, 1), blank_frames(cam, 1)
    d.set_depth_rig_batch(frames, K, tdr.IDENTITY_T)
    keep = ingest(frames, [views[0]["grey"]], [views[0]["depth"]], "raw", "grey8", SCALE, "device", None, levels)
    keep += ingest(plain, [views[0]["grey"]], [views[0]["depth"]], "raw", "grey8", SCALE, "device", None, levels)
    (Ia, Za), (Ib, Zb) = plane_of(frames[0]), plane_of(plain[0])
    assert np.array_equal(Ia, Ib) and np.array_equal(Za, Zb, equal_nan=True) and np.isfinite(Za).any()
    del keep


# ---- 4. rig plus lens -------------------------------------------------------------------------------------------------------------------

def small_setup(w=320, h=240, levels=3):
    K, views = raw_scene(w, h)
    ctx = d.default_context()
    return ctx, camera(ctx, w, h, K, levels), K, views, levels


@pytest.mark.parametrize("order", ["rig_first", "lens_first"])
def test_rig_plus_lens_that_leaves_depth_alone_equals_the_lensed_twin(order):
    ctx, cam, K, views, levels = small_setup()
    K_depth, T = tdr.kinect_rig(K)
    K_raw, D = tl.raw_K(K), tl.FR1_D
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    if order == "rig_first":
        d.set_depth_rig_batch(frames, K_depth, T)
    d.set_lens_batch(frames, K_raw, D, rectify_depth=False)
    if order == "lens_first":
        d.set_depth_rig_batch(frames, K_depth, T)
    d.set_lens_batch(twins, K_raw, D, rectify_depth=False)
    images = [in_format(v["bgr"], "bgr8") for v in views]
    c0 = counters(ctx)
    keep = ingest(frames, images, [v["depth"] for v in views], "colour", "bgr8", SCALE, "device", "reference", levels)
    assert counters(ctx) == (c0[0] + 2, c0[1] + 2, c0[2], c0[3] + 2)
    planes = [tdr.reg(v["depth"], K, K_depth, T, SCALE) for v in views]
    keep += feed_twin(twins, images, planes, "colour", "bgr8", "device", "reference", levels)
    for f, t in zip(frames, twins):
        assert_frames_equal(f, t, levels, ("rig + lens", order))
    # pixels the lens leaves invalid end with Z = NaN whatever landed there
    I, Z = plane_of(frames[0])
    rect = tl.rectify(images[0], planes[0], K, K_raw, D, False, "bgr8", 1.0)
    assert np.array_equal(Z, rect[1], equal_nan=True) and np.array_equal(I, rect[0]) and np.isnan(Z[I == 0]).all()
    del keep


def test_rig_and_a_lens_that_rectifies_depth_exclude_each_other():
    ctx, cam, K, views, levels = small_setup()
    K_depth, T = tdr.kinect_rig(K)
    K_raw, D = tl.raw_K(K), tl.FR1_D
    a, b = blank_frames(cam, 1), blank_frames(cam, 1)
    keep = ingest(a + b, [views[0]["grey"]] * 2, [views[0]["depth"]] * 2, "raw", "grey8", SCALE, "device", None, levels)
    before = [plane_of(f[0]) for f in (a, b)]
    d.set_depth_rig_batch(a, K_depth, T)
    with pytest.raises(d.DvoHipError):
        d.set_lens_batch(a, K_raw, D, rectify_depth=True)         # a lens that rectifies depth on a rigged frame
    d.set_lens_batch(b, K_raw, D, rectify_depth=True)
    with pytest.raises(d.DvoHipError):
        d.set_depth_rig_batch(b, K_depth, T)                      # a rig on a frame whose lens rectifies depth
    with pytest.raises(d.DvoHipError):
        d.set_depth_rig_batch(a + b, K_depth, T)                  # ... also as one of a list: nobody's rig changes
    for f, (i0, z0) in zip((a, b), before):
        i1, z1 = plane_of(f[0])
        assert np.array_equal(i0, i1) and np.array_equal(z0, z1, equal_nan=True)
    # the frames kept what they had: a its rig and no lens, b its lens and no rig
    c0 = counters(ctx)
    keep += ingest(a, [views[1]["grey"]], [views[1]["depth"]], "raw", "grey8", SCALE, "device", None, levels)
    keep += ingest(b, [views[1]["grey"]], [views[1]["depth"]], "raw", "grey8", SCALE, "device", None, levels)
    assert counters(ctx) == (c0[0] + 1, c0[1] + 2, c0[2], c0[3] + 1)
    assert np.array_equal(plane_of(a[0])[1], tdr.reg(views[1]["depth"], K, K_depth, T, SCALE), equal_nan=True)
    assert np.array_equal(plane_of(b[0])[1], tl.rectify(views[1]["grey"], views[1]["depth"], K, K_raw, D, True, "grey8", SCALE)[1], equal_nan=True)
    del keep


# ---- 5. flags and lifetime --------------------------------------------------------------------------------------------------------------

def ingest_pair(ctx, cam, K, views, levels, flags=0, how="match"):
    """reference <- views[0] (bgr8, reference role), current <- views[1] (rgba8, current role), rigged, from device planes with `flags`;
    and their twins.  Returns ((records of the rigged pair, records of the twins), frames, twins)."""
    K_depth, T = tdr.kinect_rig(K)
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    d.set_depth_rig_batch(frames, K_depth, T)
    keep, fed = [], []
    sources = (("bgr8", "reference"), ("rgba8", "current"))
    for k, (fmt, role) in enumerate(sources):
        image = in_format(views[k]["bgr"], fmt)
        keep += ingest(frames[k:k + 1], [image], [views[k]["depth"]], "colour", fmt, SCALE, "device", role, levels, flags=flags)
        fed.append((image, tdr.reg(views[k]["depth"], K, K_depth, T, SCALE)))
    if how == "flush":
        ctx.check(ctx._lib.dvo_hip_flush_deferred(ctx.ptr))
    cfg = config(levels)
    rigged = match_records(ctx, cfg, frames[:1], frames[1:])      # (a deferred ingest is carried out here at the latest)
    for k, (fmt, role) in enumerate(sources):
        keep += feed_twin(twins[k:k + 1], [fed[k][0]], [fed[k][1]], "colour", fmt, "device", role, levels, flags=flags & ~_lib.INGEST_DEFER)
    out = rigged, match_records(ctx, cfg, twins[:1], twins[1:])
    del keep
    return out, frames, twins


@pytest.mark.parametrize("how", ["match", "flush"])
def test_deferred_rig_ingest_equals_the_twin(how):
    ctx, cam, K, views, levels = small_setup()
    d0, n0 = ctx.counter("deferred_ingests"), ctx.counter("depth_registrations")
    (a, b), frames, twins = ingest_pair(ctx, cam, K, views, levels, flags=_lib.INGEST_DEFER, how=how)
    assert ctx.counter("deferred_ingests") - d0 == 2 and ctx.counter("depth_registrations") - n0 == 2
    assert_records_identical(a, b)
    for f, t in zip(frames, twins):
        assert_frames_equal(f, t, levels, ("deferred", how))


def test_setting_a_rig_carries_out_a_pending_ingest_first():
    ctx, cam, K, views, levels = small_setup()
    K_depth, T = tdr.kinect_rig(K)
    frames, twins = blank_frames(cam, 1), blank_frames(cam, 1)
    image, depth = in_format(views[0]["bgr"], "bgr8"), views[0]["depth"]
    d0 = ctx.counter("deferred_ingests")
    keep = ingest(frames, [image], [depth], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    assert ctx.counter("deferred_ingests") == d0
    d.set_depth_rig_batch(frames, K_depth, T)                     # the recorded ingest ran without a rig ...
    assert ctx.counter("deferred_ingests") == d0 + 1
    keep += ingest(twins, [image], [depth], "colour", "bgr8", SCALE, "device", None, levels)
    assert_frames_equal(frames[0], twins[0], levels, "pending ingest before set_depth_rig")
    keep += ingest(frames, [image], [depth], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    d.clear_depth_rig_batch(frames)                               # ... and this one with it
    keep += feed_twin(twins, [image], [tdr.reg(depth, K, K_depth, T, SCALE)], "colour", "bgr8", "device", None, levels)
    assert_frames_equal(frames[0], twins[0], levels, "pending ingest before clear_depth_rig")
    del keep


def test_no_raw_copy_behaves_as_on_the_twin():
    ctx, cam, K, views, levels = small_setup()
    (a, b), frames, twins = ingest_pair(ctx, cam, K, views, levels, flags=_lib.INGEST_NO_RAW_COPY)
    assert_records_identical(a, b)
    cfg = config(levels)
    for f in (frames[0], twins[0]):                               # a reference without a raw copy serves no other role: refused alike
        with pytest.raises(d.DvoHipError):
            d.prepare_roles_batch([f], "current", cfg)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), a)


def test_rig_replaced_then_cleared():
    ctx, cam, K, views, levels = small_setup()
    frames, twins, fresh = blank_frames(cam, 1), blank_frames(cam, 1), blank_frames(cam, 1)
    image, depth = views[0]["grey"], views[0]["depth"]
    K_depth, T = tdr.kinect_rig(K)
    other_T = T.copy()
    other_T[:, 3] = [0.05, -0.002, 0.0]
    keep = []
    for name, (kd, t) in (("kinect", (K_depth, T)), ("other", (K, other_T))):      # replaced between ingests: the newest rig holds
        frames[0].set_depth_rig(kd, t)
        keep += ingest(frames, [image], [depth], "raw", "grey8", SCALE, "host", None, levels)
        keep += feed_twin(twins, [image[..., None]], [tdr.reg(depth, K, kd, t, SCALE)], "raw", "grey8", "host", None, levels)
        assert_frames_equal(frames[0], twins[0], levels, ("replaced", name))
    n0 = ctx.counter("depth_registrations")
    frames[0].clear_depth_rig()                                   # cleared: a frame that never carried one
    keep += ingest(frames, [image], [depth], "raw", "grey8", SCALE, "device", "reference", levels)
    keep += ingest(fresh, [image], [depth], "raw", "grey8", SCALE, "device", "reference", levels)
    assert ctx.counter("depth_registrations") == n0
    assert_frames_equal(frames[0], fresh[0], levels, "cleared")
    del keep


def test_a_pyramid_that_grows_levels_keeps_its_rig():
    ctx, cam, K, views, levels = small_setup()
    K_depth, T = tdr.kinect_rig(K)
    f = d.RgbdCameraPyramid(320, 240, K, ctx).create_raw(views[0]["grey"], views[0]["depth"])   # (one level so far)
    f.set_depth_rig(K_depth, T)
    f.build(levels)                                               # (a new device frame: the wrapper hands the rig over again)
    twins = blank_frames(cam, 1)
    keep = ingest([f], [views[0]["grey"]], [views[0]["depth"]], "raw", "grey8", SCALE, "host", None, levels)
    keep += feed_twin(twins, [views[0]["grey"][..., None]], [tdr.reg(views[0]["depth"], K, K_depth, T, SCALE)], "raw", "grey8", "host", None, levels)
    assert_frames_equal(f, twins[0], levels, "grown")
    del keep


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def rig_struct(K_depth, T, reserved=(0, 0)):
    rig = _lib.DepthRig()
    rig.K_depth[:] = [float(v) for v in K_depth]
    rig.T[:] = [float(v) for v in np.asarray(T, np.float64).reshape(-1)]
    rig.reserved[:] = list(reserved)
    return rig


def test_mixed_and_invalid_rigs_and_an_aliased_source_change_nothing():
    ctx, cam, K, views, levels = small_setup()
    K_depth, T = tdr.kinect_rig(K)
    frames = blank_frames(cam, 3)
    grey, depth = views[0]["grey"], views[0]["depth"]
    keep = ingest(frames, [grey] * 3, [depth] * 3, "raw", "grey8", SCALE, "device", None, levels)
    before = [plane_of(f) for f in frames]
    c0 = counters(ctx)
    other = [views[1]["grey"]] * 3, [views[1]["depth"]] * 3

    def unchanged():
        assert counters(ctx) == c0
        for f, (i0, z0) in zip(frames, before):
            i1, z1 = plane_of(f)
            assert np.array_equal(i0, i1) and np.array_equal(z0, z1, equal_nan=True)

    # one rigged frame among rig-less ones; two different rigs
    d.set_depth_rig_batch(frames[:1], K_depth, T)
    with pytest.raises(d.DvoHipError):
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", "current", levels)
    T2 = T.copy()
    T2[0, 3] += 1e-3
    d.set_depth_rig_batch(frames[1:], K_depth, T2)
    with pytest.raises(d.DvoHipError):
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "host", None, levels)
    with pytest.raises(d.DvoHipError):
        ingest(frames, [in_format(views[1]["bgr"], "bgr8")] * 3, other[1], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    unchanged()
    # invalid rigs, straight at the C-ABI (the Python wrapper would refuse them first): the frames keep the rig they have
    handles = (C.c_void_p * 3)(*[f.ptr for f in frames])
    nan_T, inf_T = T.copy(), T.copy()
    nan_T[2, 1], inf_T[0, 3] = np.nan, np.inf
    for rig in (rig_struct([np.nan, 500, 160, 120], T), rig_struct([500, np.inf, 160, 120], T), rig_struct([0.0, 500, 160, 120], T),
                rig_struct([500, -2.0, 160, 120], T), rig_struct(K_depth, nan_T), rig_struct(K_depth, inf_T), rig_struct(K_depth, T, (0, 1)),
                rig_struct(K_depth, T, (7, 0))):
        assert ctx._lib.dvo_hip_frames_set_depth_rig(ctx.ptr, 3, handles, C.byref(rig)) == _lib.ERR_INVALID
    good = d.depth_rig_struct(K_depth, T)
    assert ctx._lib.dvo_hip_frames_set_depth_rig(ctx.ptr, 3, handles, None) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_set_depth_rig(ctx.ptr, 0, handles, C.byref(good)) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_clear_depth_rig(ctx.ptr, 3, None) == _lib.ERR_INVALID
    with pytest.raises(d.DvoHipError):                            # (still the mixed rigs of above)
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", None, levels)
    unchanged()
    # one rig for all, but a float depth source that IS a frame's own level-0 plane Z (or overlaps its end)
    d.set_depth_rig_batch(frames, K_depth, T)
    own = C.c_void_p()
    ctx.check(ctx._lib.dvo_hip_frame_device_planes(frames[1].ptr, 0, None, C.byref(own)))
    tz, pz, _ = device_bytes(before[0][1])
    ti, pi, _ = device_bytes(np.ascontiguousarray(grey[..., None]))
    for alias in (own.value, own.value + 320 * 239 * 4):
        with pytest.raises(d.DvoHipError):
            d.update_colour_device_batch(frames, [pi] * 3, [pz, alias, pz], "grey8", 320, 1.0, role=None, config=None, depth_format="f32",
                                         depth_pitch=320 * 4)
    with pytest.raises(d.DvoHipError):                            # ... and an image source there: the fill would overwrite it too
        d.update_colour_device_batch(frames, [pi, own.value + 320 * 240 * 4 - 1, pi], [pz] * 3, "grey8", 320, 1.0, role=None, config=None,
                                     depth_format="f32", depth_pitch=320 * 4)
    unchanged()
    # ... accepted from anywhere else, counted once per frame
    keep += ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", None, levels)
    assert counters(ctx) == (c0[0] + 3, c0[1] + 3, c0[2], c0[3])
    want = tdr.reg(views[1]["depth"], K, K_depth, T, SCALE)
    for f in frames:
        assert np.array_equal(plane_of(f)[1], want, equal_nan=True)
    del keep, tz, ti


# ---- 7. counters, the table, a mixed batch ----------------------------------------------------------------------------------------------

def test_rig_less_frames_launch_and_allocate_nothing():
    K, views = raw_scene(320, 240)
    ctx = d.Context()                                             # (a context of its own: nothing has been registered in it)
    cam = camera(ctx, 320, 240, K, 3)
    frames = blank_frames(cam, 3)
    keep = ingest(frames, [views[0]["grey"]] * 3, [views[0]["depth"]] * 3, "raw", "grey8", SCALE, "device", "current", 3)
    keep += ingest(frames, [in_format(views[1]["bgr"], "bgr8")] * 3, [views[1]["fdepth"]] * 3, "mixed", "bgr8", 0.5, "host", None, 3)
    assert ctx.counter("depth_registrations") == 0 and ctx.counter("depth_rig_table_bytes") == 0
    d.set_depth_rig_batch(frames, *tdr.kinect_rig(K))
    assert ctx.counter("depth_rig_table_bytes") == 0              # (a rig alone allocates nothing either)
    keep += ingest(frames, [views[0]["grey"]] * 3, [views[0]["depth"]] * 3, "raw", "grey8", SCALE, "device", "current", 3)
    assert ctx.counter("depth_registrations") == 3 and ctx.counter("depth_rig_table_bytes") >= 3 * 16
    keep += ingest(frames[:2], [views[0]["grey"]] * 2, [views[0]["depth"]] * 2, "raw", "grey8", SCALE, "host", "reference", 3)
    assert ctx.counter("depth_registrations") == 5
    del keep


def test_match_batch_mixes_rigged_and_rig_less_frames():
    ctx, cam, K, views, levels = small_setup()
    (a, b), frames, twins = ingest_pair(ctx, cam, K, views, levels)
    assert_records_identical(a, b)
    cfg = config(levels)
    mixed = match_records(ctx, cfg, [frames[0], twins[0], frames[0]], [twins[1], frames[1], frames[1]])
    plain = match_records(ctx, cfg, [twins[0], twins[0], twins[0]], [twins[1], twins[1], twins[1]])
    assert_records_identical(mixed, plain)


# ---- 8. the facade ----------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_depth_rig():
    d.build()
    out = subprocess.run([tdr.build_depth_rig_facade_check()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
