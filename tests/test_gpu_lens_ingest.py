"""GPU tier: frames that carry a lens are rectified on the device at ingest (include/dvo_hip.h, dvo_hip_frames_set_lens; k_rectify).
The yardstick is rect(P), the host build of dvo_slam_amd/csrc/lens.h (tests/test_lens.py, rectify): a lensed frame ingested from raw
planes P equals, bit for bit, the oracle's pyramid of rect(P) and a lens-less frame fed rect(P) through update_f32_*.
  1. planes, selection and match records on every entry-point family, host and device, padded and tight, every role, strip and odd sizes,
     both lens families, rectify_depth 0 / 1;
  2. flags and lifetime: deferred, no raw copy, lens replaced, lens cleared, a caller selection, a mixed batch in match_batch;
  3. counters and refusals;
  4. end to end on the distorted pair of tests/test_lens.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import scenes
import test_lens as tl
from dvo_slam_amd import _lib
from oracle import pyoracle as po
from test_gpu_colour_ingest import assert_records_identical, in_format, match_records, tinted
from test_gpu_f32_ingest import assert_frames_equal, blank_frames, camera, config, device_bytes, float_planes, host_view
from test_gpu_scene_edges import assert_frame_equals_oracle
from test_gpu_selection import masks_of

pytestmark = pytest.mark.gpu
ROLES = (None, "current", "reference")
LENSES = {"plumb_bob": tl.FR1_D, "rational": tl.RATIONAL_D}
SCALE = 1.0 / 5000.0


def lens_of(K, name):
    return tl.raw_K(K), LENSES[name]


_scenes = {}


def raw_scene(w, h):
    """a pair of raw frames in every source form: (K, per view: dict(grey u8, bgr u8 [h, w, 3], depth u16, fimg f32, fdepth f32))"""
    if (w, h) not in _scenes:
        p = scenes.edge_scene(3, w, h)
        views = []
        for k, v in enumerate(("ref", "cur")):
            fi, fz = float_planes(p["grey_" + v], p["depth_" + v], k + 1)
            views.append(dict(grey=p["grey_" + v], bgr=tinted(p["grey_" + v], k + 1), depth=p["depth_" + v], fimg=fi, fdepth=fz))
        _scenes[(w, h)] = (p["K"], views)
    return _scenes[(w, h)]


def source(view, family, fmt):
    """(image plane, image format name for rectify(), depth plane, depth scale) of one view in an entry-point family"""
    if family == "raw":
        return view["grey"], "grey8", view["depth"], SCALE
    if family == "colour":
        return in_format(view["bgr"], fmt), fmt, view["depth"], SCALE
    if family == "f32":
        return view["fimg"], "f32", view["fdepth"], 0.5
    # "mixed": an 8-bit image with float depth
    image = np.ascontiguousarray(view["grey"][..., None]) if fmt == "grey8" else in_format(view["bgr"], fmt)
    return image, fmt, view["fdepth"], 0.5


def ingest(frames, images, depths, family, fmt, scale, entry, role, levels, ipad=0, zpad=0, flags=0):
    """the planes through the family's update_* entry point; returns what must stay alive"""
    cfg = config(levels) if role else None
    keep = []
    if entry == "device":
        iptr, zptr = [], []
        for i, z in zip(images, depths):
            ti, pi, ipitch = device_bytes(i, 0, ipad)
            tz, pz, zpitch = device_bytes(z, 0, zpad)
            keep += [ti, tz]
            iptr.append(pi)
            zptr.append(pz)
        if family == "raw":
            assert flags == 0
            d.update_raw_device_batch(frames, iptr, zptr, scale, role=role, config=cfg)
        elif family == "colour":
            d.update_colour_device_batch(frames, iptr, zptr, fmt, ipitch, scale, role=role, config=cfg, flags=flags)
        elif family == "f32":
            d.update_f32_device_batch(frames, iptr, zptr, ipitch, zpitch, scale, role=role, config=cfg, flags=flags)
        else:
            d.update_colour_device_batch(frames, iptr, zptr, fmt, ipitch, scale, role=role, config=cfg, flags=flags, depth_format="f32",
                                         depth_pitch=zpitch)
    else:
        hi, hz = [host_view(i, ipad) for i in images], [host_view(z, zpad) for z in depths]
        keep += hi + hz
        if family == "raw":
            d.update_raw_host_batch(frames, hi, hz, scale, role=role, config=cfg)
        elif family == "colour":
            d.update_colour_host_batch(frames, hi, hz, fmt, scale, role=role, config=cfg, flags=flags)
        elif family == "f32":
            d.update_f32_host_batch(frames, hi, hz, scale, role=role, config=cfg, flags=flags)
        else:
            d.update_colour_host_batch(frames, hi, hz, fmt, scale, role=role, config=cfg, flags=flags, depth_format="f32")
        d.upload_wait(frames[0].ctx)
    torch.cuda.synchronize()
    return keep


def feed_rectified(frames, pairs, role, levels, flags=0):
    """the lens-less twin: rect(P) through update_f32_device_batch, depth_scale 1"""
    keep, iptr, zptr = [], [], []
    for I, Z in pairs:
        ti, pi, _ = device_bytes(I)
        tz, pz, _ = device_bytes(Z)
        keep += [ti, tz]
        iptr.append(pi)
        zptr.append(pz)
    d.update_f32_device_batch(frames, iptr, zptr, 0, 0, 1.0, role=role, config=config(levels) if role else None, flags=flags)
    torch.cuda.synchronize()
    return keep


# ---- 1. planes, bit for bit -----------------------------------------------------------------------------------------------------------

FAMILIES = [("raw", "grey8"), ("colour", "bgr8"), ("colour", "rgba8"), ("f32", "f32"), ("mixed", "rgb8"), ("mixed", "grey8"), ("mixed", "bgra8")]
SHAPES = [(640, 480), (321, 240), (102, 78)]          # strip-eligible; odd; an odd half width


def cases():
    """every family x entry x role, with shape, lens family, rectify_depth and padding cycling so that each shape meets each role (the
    shape advances with the role and shifts by one per entry and family), and every (lens family, rectify_depth) pair each role, each shape and each entry"""
    out, i = [], 0
    for family, fmt in FAMILIES:
        for entry in ("device", "host"):
            for role in ROLES:
                shape = SHAPES[(i + i // 3) % 3]
                lens = ("plumb_bob", "rational")[(i + i // 2) % 2]
                rd = (i + i // 4) % 2
                pad = 0 if family == "raw" else (0, 8)[(i + i // 3) % 2]
                out.append(pytest.param(family, fmt, entry, role, shape, lens, rd, pad,
                                        id="%s-%s-%s-%s-%dx%d-%s-rd%d-pad%d" % ((family, fmt, entry, role) + shape + (lens, rd, pad))))
                i += 1
    return out


@pytest.mark.parametrize("family,fmt,entry,role,shape,lens,rectify_depth,pad", cases())
def test_lensed_frame_equals_the_oracle_of_the_rectified_planes(family, fmt, entry, role, shape, lens, rectify_depth, pad):
    w, h = shape
    K, views = raw_scene(w, h)
    levels = 4 if h >= 240 else 3
    K_raw, D = lens_of(K, lens)
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    d.set_lens_batch(frames, K_raw, D, bool(rectify_depth))
    src = [source(v, family, fmt) for v in views]
    scale = src[0][3]
    zpad = pad // 2 * 4 if src[0][2].dtype == np.float32 else 0
    n0, f0, c0 = ctx.counter("lens_ingests"), ctx.counter("f32_ingests"), ctx.counter("colour_ingests")
    keep = ingest(frames, [s[0] for s in src], [s[2] for s in src], family, fmt, scale, entry, role, levels, pad, zpad)
    assert (ctx.counter("lens_ingests"), ctx.counter("f32_ingests"), ctx.counter("colour_ingests")) == (n0 + 2, f0 + 2, c0)
    rect = [tl.rectify(s[0], s[2], K, K_raw, D, bool(rectify_depth), s[1], scale) for s in src]
    assert all(np.isnan(Z).any() and (I == 0).any() for I, Z in rect)             # (the lens leaves an invalid border)
    what = (family, fmt, entry, role, shape, lens, rectify_depth, pad)
    for f, (I, Z) in zip(frames, rect):
        assert_frame_equals_oracle(f, po.Pyramid(I, Z, K, levels), levels, what)
    keep += feed_rectified(twins, rect, role, levels)
    assert ctx.counter("lens_ingests") == n0 + 2                                  # (the twins carry no lens)
    cfg = config(levels)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), match_records(ctx, cfg, twins[:1], twins[1:]))
    del keep


# ---- 2. flags and lifetime ------------------------------------------------------------------------------------------------------------

def small_setup(n=2, w=320, h=240, levels=3):
    K, views = raw_scene(w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    return ctx, cam, K, views, levels


def ingest_pair(ctx, cam, K, views, levels, lens, flags=0, how="match", rectify_depth=True):
    """reference <- views[0] (bgr8, reference role), current <- views[1] (rgba8, current role), lensed, from device planes with `flags`;
    and their lens-less twins fed rect(P).  Returns (records of the lensed pair, records of the twins)."""
    K_raw, D = lens_of(K, lens)
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    d.set_lens_batch(frames, K_raw, D, rectify_depth)
    keep, rect = [], []
    sources = (("bgr8", "reference"), ("rgba8", "current"))
    for k, (fmt, role) in enumerate(sources):
        image = in_format(views[k]["bgr"], fmt)
        keep += ingest(frames[k:k + 1], [image], [views[k]["depth"]], "colour", fmt, SCALE, "device", role, levels, flags=flags)
        rect.append(tl.rectify(image, views[k]["depth"], K, K_raw, D, rectify_depth, fmt, SCALE))
    if how == "flush":
        ctx.check(ctx._lib.dvo_hip_flush_deferred(ctx.ptr))
    cfg = config(levels)
    lensed = match_records(ctx, cfg, frames[:1], frames[1:])      # (a deferred ingest is carried out here at the latest)
    for k, (fmt, role) in enumerate(sources):
        keep += feed_rectified(twins[k:k + 1], rect[k:k + 1], role, levels, flags=flags & ~_lib.INGEST_DEFER)
    out = lensed, match_records(ctx, cfg, twins[:1], twins[1:])
    del keep
    return out, frames, twins, rect


@pytest.mark.parametrize("how", ["match", "flush"])
def test_deferred_lens_ingest_equals_the_twin(how):
    ctx, cam, K, views, levels = small_setup()
    d0, n0 = ctx.counter("deferred_ingests"), ctx.counter("lens_ingests")
    (a, b), frames, twins, _ = ingest_pair(ctx, cam, K, views, levels, "plumb_bob", flags=_lib.INGEST_DEFER, how=how)
    assert ctx.counter("deferred_ingests") - d0 == 2 and ctx.counter("lens_ingests") - n0 == 2
    assert_records_identical(a, b)
    for f, t in zip(frames, twins):
        assert_frames_equal(f, t, levels, ("deferred", how))


def test_setting_a_lens_carries_out_a_pending_ingest_first():
    ctx, cam, K, views, levels = small_setup()
    K_raw, D = lens_of(K, "plumb_bob")
    frames, twins = blank_frames(cam, 1), blank_frames(cam, 1)
    image = in_format(views[0]["bgr"], "bgr8")
    d0 = ctx.counter("deferred_ingests")
    keep = ingest(frames, [image], [views[0]["depth"]], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    assert ctx.counter("deferred_ingests") == d0
    d.set_lens_batch(frames, K_raw, D)                            # the recorded ingest ran without a lens ...
    assert ctx.counter("deferred_ingests") == d0 + 1
    keep += ingest(twins, [image], [views[0]["depth"]], "colour", "bgr8", SCALE, "device", None, levels)
    assert_frames_equal(frames[0], twins[0], levels, "pending ingest before set_lens")
    keep += ingest(frames, [image], [views[0]["depth"]], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    d.clear_lens_batch(frames)                                    # ... and this one with it
    keep += feed_rectified(twins, [tl.rectify(image, views[0]["depth"], K, K_raw, D, True, "bgr8", SCALE)], None, levels)
    assert_frames_equal(frames[0], twins[0], levels, "pending ingest before clear_lens")
    del keep


def test_no_raw_copy_behaves_as_on_the_twin():
    ctx, cam, K, views, levels = small_setup()
    (a, b), frames, twins, _ = ingest_pair(ctx, cam, K, views, levels, "rational", flags=_lib.INGEST_NO_RAW_COPY)
    assert_records_identical(a, b)
    cfg = config(levels)
    for f in (frames[0], twins[0]):                               # a reference without a raw copy serves no other role: refused alike
        with pytest.raises(d.DvoHipError):
            d.prepare_roles_batch([f], "current", cfg)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), a)


def test_lens_replaced_then_cleared():
    ctx, cam, K, views, levels = small_setup()
    frames, twins, fresh = blank_frames(cam, 1), blank_frames(cam, 1), blank_frames(cam, 1)
    image, depth = views[0]["grey"], views[0]["depth"]
    keep = []
    for name, rd in (("plumb_bob", True), ("rational", False)):   # replaced between ingests: the newest lens holds
        K_raw, D = lens_of(K, name)
        d.set_lens_batch(frames, K_raw, D, rd)
        keep += ingest(frames, [image], [depth], "raw", "grey8", SCALE, "host", None, levels)
        keep += feed_rectified(twins, [tl.rectify(image, depth, K, K_raw, D, rd, "grey8", SCALE)], None, levels)
        assert_frames_equal(frames[0], twins[0], levels, ("replaced", name))
    n0 = ctx.counter("lens_ingests")
    frames[0].clear_lens()                                        # cleared: a frame that never carried one
    keep += ingest(frames, [image], [depth], "raw", "grey8", SCALE, "device", "reference", levels)
    keep += ingest(fresh, [image], [depth], "raw", "grey8", SCALE, "device", "reference", levels)
    assert ctx.counter("lens_ingests") == n0
    assert_frames_equal(frames[0], fresh[0], levels, "cleared")
    assert_frame_equals_oracle(frames[0], po.Pyramid(image.astype(np.float32), po.convert_raw_depth(depth), K, levels), levels, "cleared")
    del keep


def test_caller_selection_on_a_lensed_frame():
    ctx, cam, K, views, levels = small_setup()
    mask = masks_of("blocks", 5, 320, 240)
    (a, b), frames, twins, rect = ingest_pair(ctx, cam, K, views, levels, "plumb_bob")
    frames[0].set_selection(mask, 0.0, 3.0)                       # the mask is in rectified coordinates: the twin takes the same one
    twins[0].set_selection(mask, 0.0, 3.0)
    cfg = config(levels)
    sel_a, sel_b = match_records(ctx, cfg, frames[:1], frames[1:]), match_records(ctx, cfg, twins[:1], twins[1:])
    assert_records_identical(sel_a, sel_b)
    assert not np.array_equal(sel_a[0][0], a[0][0])
    for l in range(levels):
        assert d.PointSelection(frames[0], 6.0, 0.03).select(l) == d.PointSelection(twins[0], 6.0, 0.03).select(l)
    # ... and it survives a lens re-ingest
    image = in_format(views[0]["bgr"], "bgr8")
    keep = ingest(frames[:1], [image], [views[0]["depth"]], "colour", "bgr8", SCALE, "host", "reference", levels)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), sel_b)
    del keep


def test_match_batch_mixes_lensed_and_lens_less_frames():
    ctx, cam, K, views, levels = small_setup()
    (a, b), frames, twins, rect = ingest_pair(ctx, cam, K, views, levels, "rational")
    cfg = config(levels)
    mixed = match_records(ctx, cfg, [frames[0], twins[0], frames[0]], [twins[1], frames[1], frames[1]])
    plain = match_records(ctx, cfg, [twins[0], twins[0], twins[0]], [twins[1], twins[1], twins[1]])
    assert_records_identical(mixed, plain)


# ---- 3. counters and refusals -----------------------------------------------------------------------------------------------------------

def plane_of(frame, level=0):
    torch.cuda.synchronize()
    return np.array(frame.level(level).intensity, copy=True), np.array(frame.level(level).depth, copy=True)


def test_mixed_and_invalid_lenses_are_refused_and_change_nothing():
    ctx, cam, K, views, levels = small_setup()
    K_raw, D = lens_of(K, "plumb_bob")
    frames = blank_frames(cam, 3)
    grey, depth = views[0]["grey"], views[0]["depth"]
    keep = ingest(frames, [grey] * 3, [depth] * 3, "raw", "grey8", SCALE, "device", None, levels)
    before = [plane_of(f) for f in frames]
    n0 = ctx.counter("lens_ingests")
    other = [views[1]["grey"]] * 3, [views[1]["depth"]] * 3
    # one lensed frame among lens-less ones; two different lenses; lenses that differ in rectify_depth only
    d.set_lens_batch(frames[:1], K_raw, D)
    with pytest.raises(d.DvoHipError):
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", "current", levels)
    d.set_lens_batch(frames[1:], *lens_of(K, "rational"))
    with pytest.raises(d.DvoHipError):
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "host", None, levels)
    d.set_lens_batch(frames[1:], K_raw, D, rectify_depth=False)
    with pytest.raises(d.DvoHipError):
        ingest(frames, [in_format(views[1]["bgr"], "bgr8")] * 3, other[1], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    assert ctx.counter("lens_ingests") == n0
    for f, (i0, z0) in zip(frames, before):
        i1, z1 = plane_of(f)
        assert np.array_equal(i0, i1) and np.array_equal(z0, z1, equal_nan=True)
    # invalid lenses, straight at the C-ABI (the Python wrapper would refuse them first): the frames keep the lens they have
    handles = (C.c_void_p * 3)(*[f.ptr for f in frames])
    for k_raw, dd in (([np.nan, 500, 160, 120], D), ([500, np.inf, 160, 120], D), ([0.0, 500, 160, 120], D), ([500, -2.0, 160, 120], D),
                      (list(K_raw), [0.1, np.nan, 0, 0, 0, 0, 0, 0]), (list(K_raw), [0.1, 0, 0, 0, 0, 0, 0, np.inf])):
        lens = _lib.Lens()
        lens.K_raw[:] = [float(v) for v in k_raw]
        lens.D[:] = [float(v) for v in list(dd) + [0.0] * (8 - len(dd))]
        lens.rectify_depth = 1
        assert ctx._lib.dvo_hip_frames_set_lens(ctx.ptr, 3, handles, C.byref(lens)) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_set_lens(ctx.ptr, 3, handles, None) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_set_lens(ctx.ptr, 0, handles, C.byref(d.lens_struct(K_raw, D))) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_clear_lens(ctx.ptr, 3, None) == _lib.ERR_INVALID
    with pytest.raises(d.DvoHipError):                            # (still the mixed lenses of above)
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", None, levels)
    for f, (i0, z0) in zip(frames, before):
        i1, z1 = plane_of(f)
        assert np.array_equal(i0, i1) and np.array_equal(z0, z1, equal_nan=True)
    # one lens for all: accepted, counted once per frame; lens-less ingests count nothing
    d.set_lens_batch(frames, K_raw, D)
    keep += ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", None, levels)
    assert ctx.counter("lens_ingests") == n0 + 3
    I, Z = tl.rectify(views[1]["grey"], views[1]["depth"], K, K_raw, D, True, "grey8", SCALE)
    for f in frames:
        i1, z1 = plane_of(f)
        assert np.array_equal(i1, I) and np.array_equal(z1, Z, equal_nan=True)
    d.clear_lens_batch(frames)
    keep += ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "host", "reference", levels)
    assert ctx.counter("lens_ingests") == n0 + 3
    del keep


def test_a_pyramid_that_grows_levels_keeps_its_lens():
    ctx, cam, K, views, levels = small_setup()
    K_raw, D = lens_of(K, "plumb_bob")
    f = d.RgbdCameraPyramid(320, 240, K, ctx).create_raw(views[0]["grey"], views[0]["depth"])   # (one level so far)
    f.set_lens(K_raw, D)
    f.build(levels)                                               # (a new device frame: the wrapper hands the lens over again)
    keep = ingest([f], [views[0]["grey"]], [views[0]["depth"]], "raw", "grey8", SCALE, "host", None, levels)
    I, Z = tl.rectify(views[0]["grey"], views[0]["depth"], K, K_raw, D, True, "grey8", SCALE)
    assert_frame_equals_oracle(f, po.Pyramid(I, Z, K, levels), levels, "grown")
    del keep


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------

def test_engine_on_the_distorted_pair_matches_the_oracle_on_the_rectified_pair():
    """the engine's twist on the lens-ingested distorted pair against the oracle's match on rect(P): the project's default-mode parity
    bound, 3e-5 in twist (README)"""
    pair, raw, K_raw = tl.matters_pair()
    levels, D = tl.MATTERS["levels"], tl.MATTERS["D"]
    w, h = tl.MATTERS["w"], tl.MATTERS["h"]
    ctx = d.default_context()
    cam = camera(ctx, w, h, pair["K"], levels)
    frames = blank_frames(cam, 2)
    d.set_lens_batch(frames, K_raw, D)
    cfg = d.Config(FirstLevel=levels - 1, LastLevel=0)
    keep = ingest(frames[:1], [raw["grey_ref"]], [raw["depth_ref"]], "raw", "grey8", SCALE, "device", "reference", levels)
    keep += ingest(frames[1:], [raw["grey_cur"]], [raw["depth_cur"]], "raw", "grey8", SCALE, "device", "current", levels)
    res = d.Result()
    d.DenseTracker(cfg, ctx).match(frames[0], frames[1], res)
    o = po.match(*tl.rectified_pyramids(raw, pair["K"], K_raw, D, levels), po.make_config(first_level=levels - 1, last_level=0, mode=po.MATH))
    err = float(np.abs(po.se3_log(np.linalg.inv(res.Transformation) @ o["T"])).max())
    e_gpu = tl.pose_error(np.asarray(res.Transformation), pair["xi_true"])
    print("engine against the oracle on rect(P): |twist|_inf = %.3e; engine's pose error against the scene's true warp = %.3e" % (err, e_gpu))
    assert err < 3e-5
    del keep


def test_cpp_facade_lens():
    d.build()
    out = subprocess.run([tl.build_lens_facade_check()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
