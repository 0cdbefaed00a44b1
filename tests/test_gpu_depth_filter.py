"""GPU tier: frames that carry a depth filter have their depth plane conditioned on the device at ingest (include/dvo_hip.h,
dvo_hip_frames_set_depth_filter; k_depth_filter).  The yardstick is filt(P), the host build of dvo_slam_amd/csrc/depth_filter.h
(tests/test_depth_filter.py, filt): a filtered frame ingested from the image plane and the depth plane P equals, bit for bit, its
filter-less TWIN fed the same image plane and filt(P) through the float-depth entry point of that image format.
  1. every level, plane, selection and match record on every entry-point family, host and device, every role, strip, odd and ragged sizes;
  2. level 0 against the yardstick for every radius x edge_radius x hole_radius, at sizes around the kernel's tile;
  3. composition with a lens and a rig: the source is the frame's own plane Z;
  4. flags and lifetime: deferred, pending, no raw copy, replaced, cleared, re-ingested;
  5. refusals change nothing;
  6. counters, a mixed batch in match_batch;
  7. repeatability;
  8. the C++ facade."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import test_depth_filter as tdf
import test_depth_rig as tdr
import test_lens as tl
from dvo_slam_amd import _lib
from test_gpu_colour_ingest import assert_records_identical, in_format, match_records
from test_gpu_depth_rig import FAMILIES, ROLES, SHAPES, feed_twin, plane_of
from test_gpu_f32_ingest import assert_frames_equal, blank_frames, camera, config, device_bytes
from test_gpu_lens_ingest import SCALE, ingest, raw_scene, source

pytestmark = pytest.mark.gpu
TILE_W, TILE_H = 64, 16                                          # k_depth_filter's tile (depth_filter.hip)
STRONG = dict(radius=3, sigma_space=2.0, edge_radius=2, hole_radius=1)
INGEST_COUNTERS = ("depth_filter_ingests", "f32_ingests", "colour_ingests", "lens_ingests", "depth_registrations", "strip_ingests",
                   "sensor_ingests", "deferred_ingests")


def counters(ctx, keys=INGEST_COUNTERS[:5]):
    return tuple(ctx.counter(k) for k in keys)


# ---- 1. a filtered frame equals its twin ----------------------------------------------------------------------------------------------

def cases():
    """every family x entry x role, with shape, padding and parameters cycling so that each shape meets each role, each entry and each family"""
    out, i = [], 0
    for family, fmt in FAMILIES:
        for entry in ("device", "host"):
            for role in ROLES:
                shape = SHAPES[(i + i // 3) % 3]
                pad = 0 if family == "raw" else (0, 8)[(i + i // 3) % 2]
                params = ({}, STRONG)[i % 2]
                out.append(pytest.param(family, fmt, entry, role, shape, pad, params,
                                        id="%s-%s-%s-%s-%dx%d-pad%d-r%d" % ((family, fmt, entry, role) + shape + (pad, params.get("radius", 2)))))
                i += 1
    return out


@pytest.mark.parametrize("family,fmt,entry,role,shape,pad,params", cases())
def test_filtered_frame_equals_its_twin(family, fmt, entry, role, shape, pad, params):
    w, h = shape
    K, views = raw_scene(w, h)
    levels = 4 if h >= 240 else 3
    ctx = d.default_context()
    cam = camera(ctx, w, h, K, levels)
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    d.set_depth_filter_batch(frames, **params)
    src = [source(v, family, fmt) for v in views]
    scale = src[0][3]
    zpad = pad // 2 * 4 if src[0][2].dtype == np.float32 else 0   # (a padded pitch for the float sources)
    c0 = counters(ctx)
    keep = ingest(frames, [s[0] for s in src], [s[2] for s in src], family, fmt, scale, entry, role, levels, pad, zpad)
    colour = 2 if family in ("colour", "mixed") else 0
    assert counters(ctx) == (c0[0] + 2, c0[1] + 2, c0[2] + colour, c0[3], c0[4])
    planes = [tdf.filt(s[2], params, scale) for s in src]
    assert all(tdf.is_hole(Z).any() and np.isfinite(Z).any() for Z in planes)
    keep += feed_twin(twins, [s[0] for s in src], planes, family, fmt, entry, role, levels, pad)
    assert counters(ctx) == (c0[0] + 2, c0[1] + 4, c0[2] + 2 * colour, c0[3], c0[4])      # (the twins carry no filter)
    what = (family, fmt, entry, role, shape, pad)
    for f, t in zip(frames, twins):
        assert_frames_equal(f, t, levels, what)
    cfg = config(levels)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), match_records(ctx, cfg, twins[:1], twins[1:]))
    del keep


# ---- 2. level 0 against the yardstick -----------------------------------------------------------------------------------------------------

def check_level_0(ctx, w, h, raw, fmt, params, levels=2):
    """one ingest of the plane under `params`; returns (device plane, yardstick plane, converted input)"""
    K = tdr.scaled_K(max(w, 64))
    frames = blank_frames(camera(ctx, w, h, K, levels), 1)
    d.set_depth_filter_batch(frames, **params)
    grey = (raw >> 6).astype(np.uint8)
    if fmt == "f32":
        depth = np.where(raw == 0, np.nan, raw.astype(np.float32) * np.float32(4e-4)).astype(np.float32)
        keep = ingest(frames, [grey[..., None]], [depth], "mixed", "grey8", 0.5, "device", None, levels, 0, 12)
        want, z = tdf.filt(depth, params, 0.5), depth * np.float32(0.5)
    else:
        keep = ingest(frames, [grey], [raw], "raw", "grey8", SCALE, "device", None, levels)
        want, z = tdf.filt(raw, params, SCALE), tdf.converted(raw)
    I, Z = plane_of(frames[0])
    assert np.array_equal(I, grey.astype(np.float32))
    del keep
    return Z, want, z


@pytest.mark.parametrize("w,h,fmt", [(102, 78, "u16"), (321, 240, "f32")])
def test_level_0_equals_the_yardstick_for_every_radius(w, h, fmt):
    ctx = d.default_context()
    raw = tdf.busy_plane(w, h)
    for radius, edge_radius, hole_radius in itertools.product(range(4), range(3), range(3)):
        params = dict(radius=radius, sigma_space=0.6 + 0.5 * radius, edge_radius=edge_radius, hole_radius=hole_radius)
        Z, want, z = check_level_0(ctx, w, h, raw, fmt, params)
        what = (w, h, fmt, params)
        assert tdf.same_bits(Z, want), what
        # not vacuous: holes of the input, pixels the rules rejected, pixels the smoothing moved
        hole, valid_in = tdf.is_hole(Z), np.isfinite(z) & (z > 0)
        assert (hole & ~valid_in).any() and (~hole).any(), what
        assert (hole & valid_in).any() == (edge_radius > 0 or hole_radius > 0), what
        assert (tdf.bits(Z)[~hole] != tdf.bits(z)[~hole]).any() == (radius > 0), what


def tile_plane(w, h):
    """u16 depth for the small shapes, where tdf.busy_plane leaves little standing: a gently slanted wall with a millimetre of noise,
    one step near the right border, a few single holes, one in a corner; the last row and the last column carry depth"""
    rng = np.random.default_rng([7, w, h])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 2.0 + 0.2 * x / w + 0.05 * y / h + rng.normal(0, 0.001, (h, w))
    z[:, 3 * w // 4:] -= 1.0
    raw = np.rint(z * 5000).astype(np.uint16)
    raw[rng.random((h, w)) < 0.01] = 0
    raw[0, 0] = raw[h // 2, w // 3] = 0
    raw[h - 1, w - 1] = raw[h - 1, 0] = raw[0, w - 1] = 9000
    return raw


@pytest.mark.parametrize("w,h", [(TILE_W + 1, TILE_H + 1), (2 * TILE_W + 1, 3 * TILE_H + 1), (33, 9)],
                         ids=["one-more-than-a-tile", "one-more-than-tiles", "smaller-than-a-tile"])
@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_level_0_equals_the_yardstick_around_the_tile(w, h, fmt):
    ctx = d.default_context()
    raw = tile_plane(w, h)
    for params in ({}, STRONG, dict(radius=0, edge_radius=0, hole_radius=2)):
        Z, want, z = check_level_0(ctx, w, h, raw, fmt, params)
        assert tdf.same_bits(Z, want), (w, h, fmt, params)
        hole, valid_in = tdf.is_hole(Z), np.isfinite(z) & (z > 0)
        assert (hole & ~valid_in).any() and (hole & valid_in).any() and (~hole).mean() > 0.3
        assert (tdf.bits(Z)[~hole] != tdf.bits(z)[~hole]).any() == (params.get("radius", 2) > 0)


# ---- 3. composition with a lens and a rig -------------------------------------------------------------------------------------------------

def small_setup(w=320, h=240, levels=3):
    K, views = raw_scene(w, h)
    ctx = d.default_context()
    return ctx, camera(ctx, w, h, K, levels), K, views, levels


@pytest.mark.parametrize("kind", ["lens-rectify-depth", "lens-depth-alone", "rig", "rig-lens"])
@pytest.mark.parametrize("role", [None, "reference"])
def test_filter_behind_a_lens_and_a_rig(kind, role):
    """the twin carries the same lens and rig and no filter; its downloaded level-0 pair goes through filt into a plain frame"""
    ctx, cam, K, views, levels = small_setup()
    frames, twins, plain = blank_frames(cam, 2), blank_frames(cam, 2), blank_frames(cam, 2)
    K_depth, T = tdr.kinect_rig(K)
    for group in (frames, twins):
        if "rig" in kind:
            d.set_depth_rig_batch(group, K_depth, T)
        if "lens" in kind:
            d.set_lens_batch(group, tl.raw_K(K), tl.FR1_D, rectify_depth=kind == "lens-rectify-depth")
    d.set_depth_filter_batch(frames, **STRONG)
    images = [in_format(v["bgr"], "bgr8") for v in views]
    depths = [v["depth"] for v in views]
    c0 = counters(ctx)
    keep = ingest(frames, images, depths, "colour", "bgr8", SCALE, "device", role, levels)
    lens, rig = (2 if "lens" in kind else 0), (2 if "rig" in kind else 0)
    assert counters(ctx) == (c0[0] + 2, c0[1] + 2, c0[2] + (0 if lens else 2), c0[3] + lens, c0[4] + rig)
    keep += ingest(twins, images, depths, "colour", "bgr8", SCALE, "device", None, levels)
    pairs = [plane_of(t) for t in twins]
    filtered = [tdf.filt(Z, STRONG, 1.0) for _, Z in pairs]
    assert all((tdf.is_hole(F) & np.isfinite(Z)).any() and (~tdf.is_hole(F)).any() for F, (_, Z) in zip(filtered, pairs))
    if "lens" in kind:                                           # a lensed frame is a plain frame fed the rectified FLOAT pair
        keep += ingest(plain, [I for I, _ in pairs], filtered, "f32", "f32", 1.0, "device", role, levels)
    else:                                                        # a rigged frame is a plain frame fed the image and the registered plane
        keep += feed_twin(plain, images, filtered, "colour", "bgr8", "device", role, levels)
    for f, p in zip(frames, plain):
        assert_frames_equal(f, p, levels, (kind, role))
    cfg = config(levels)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), match_records(ctx, cfg, plain[:1], plain[1:]))
    del keep


# ---- 4. flags and lifetime --------------------------------------------------------------------------------------------------------------

def ingest_pair(ctx, cam, views, levels, flags=0, how="match", params=STRONG):
    """reference <- views[0] (bgr8, reference role), current <- views[1] (rgba8, current role), filtered, from device planes with `flags`;
    and their twins.  Returns ((records of the filtered pair, records of the twins), frames, twins)."""
    frames, twins = blank_frames(cam, 2), blank_frames(cam, 2)
    d.set_depth_filter_batch(frames, **params)
    keep, fed = [], []
    sources = (("bgr8", "reference"), ("rgba8", "current"))
    for k, (fmt, role) in enumerate(sources):
        image = in_format(views[k]["bgr"], fmt)
        keep += ingest(frames[k:k + 1], [image], [views[k]["depth"]], "colour", fmt, SCALE, "device", role, levels, flags=flags)
        fed.append((image, tdf.filt(views[k]["depth"], params, SCALE)))
    if how == "flush":
        ctx.check(ctx._lib.dvo_hip_flush_deferred(ctx.ptr))
    cfg = config(levels)
    filtered = match_records(ctx, cfg, frames[:1], frames[1:])    # (a deferred ingest is carried out here at the latest)
    for k, (fmt, role) in enumerate(sources):
        keep += feed_twin(twins[k:k + 1], [fed[k][0]], [fed[k][1]], "colour", fmt, "device", role, levels, flags=flags & ~_lib.INGEST_DEFER)
    out = filtered, match_records(ctx, cfg, twins[:1], twins[1:])
    del keep
    return out, frames, twins


@pytest.mark.parametrize("how", ["match", "flush"])
def test_deferred_filter_ingest_equals_the_twin(how):
    ctx, cam, K, views, levels = small_setup()
    d0, n0 = ctx.counter("deferred_ingests"), ctx.counter("depth_filter_ingests")
    (a, b), frames, twins = ingest_pair(ctx, cam, views, levels, flags=_lib.INGEST_DEFER, how=how)
    assert ctx.counter("deferred_ingests") - d0 == 2 and ctx.counter("depth_filter_ingests") - n0 == 2
    assert_records_identical(a, b)
    for f, t in zip(frames, twins):
        assert_frames_equal(f, t, levels, ("deferred", how))


def test_setting_a_filter_carries_out_a_pending_ingest_first():
    ctx, cam, K, views, levels = small_setup()
    frames, twins = blank_frames(cam, 1), blank_frames(cam, 1)
    image, depth = in_format(views[0]["bgr"], "bgr8"), views[0]["depth"]
    d0 = ctx.counter("deferred_ingests")
    keep = ingest(frames, [image], [depth], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    assert ctx.counter("deferred_ingests") == d0
    d.set_depth_filter_batch(frames)                              # the recorded ingest ran without a filter ...
    assert ctx.counter("deferred_ingests") == d0 + 1
    keep += ingest(twins, [image], [depth], "colour", "bgr8", SCALE, "device", None, levels)
    assert_frames_equal(frames[0], twins[0], levels, "pending ingest before set_depth_filter")
    keep += ingest(frames, [image], [depth], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    d.clear_depth_filter_batch(frames)                            # ... and this one with it
    keep += feed_twin(twins, [image], [tdf.filt(depth, {}, SCALE)], "colour", "bgr8", "device", None, levels)
    assert_frames_equal(frames[0], twins[0], levels, "pending ingest before clear_depth_filter")
    del keep


def test_no_raw_copy_behaves_as_on_the_twin():
    ctx, cam, K, views, levels = small_setup()
    (a, b), frames, twins = ingest_pair(ctx, cam, views, levels, flags=_lib.INGEST_NO_RAW_COPY)
    assert_records_identical(a, b)
    cfg = config(levels)
    for f in (frames[0], twins[0]):                               # a reference without a raw copy serves no other role: refused alike
        with pytest.raises(d.DvoHipError):
            d.prepare_roles_batch([f], "current", cfg)
    assert_records_identical(match_records(ctx, cfg, frames[:1], frames[1:]), a)


def test_filter_replaced_reingested_then_cleared():
    ctx, cam, K, views, levels = small_setup()
    frames, twins, fresh = blank_frames(cam, 1), blank_frames(cam, 1), blank_frames(cam, 1)
    image = views[0]["grey"]
    keep = []
    # replaced between ingests: the newest filter holds; re-ingested with another plane under the same filter: the new plane's filter
    for name, params, depth in (("default", {}, views[0]["depth"]), ("strong", STRONG, views[0]["depth"]), ("strong, new plane", None, views[1]["depth"])):
        if params is not None:
            frames[0].set_depth_filter(**params)
        keep += ingest(frames, [image], [depth], "raw", "grey8", SCALE, "host", None, levels)
        keep += feed_twin(twins, [image[..., None]], [tdf.filt(depth, STRONG if params is None else params, SCALE)], "raw", "grey8", "host", None, levels)
        assert_frames_equal(frames[0], twins[0], levels, ("replaced", name))
    n0 = ctx.counter("depth_filter_ingests")
    frames[0].clear_depth_filter()                                # cleared: a frame that never carried one
    keep += ingest(frames, [image], [views[0]["depth"]], "raw", "grey8", SCALE, "device", "reference", levels)
    keep += ingest(fresh, [image], [views[0]["depth"]], "raw", "grey8", SCALE, "device", "reference", levels)
    assert ctx.counter("depth_filter_ingests") == n0
    assert_frames_equal(frames[0], fresh[0], levels, "cleared")
    del keep


def test_a_pyramid_that_grows_levels_keeps_its_filter():
    ctx, cam, K, views, levels = small_setup()
    f = d.RgbdCameraPyramid(320, 240, K, ctx).create_raw(views[0]["grey"], views[0]["depth"])   # (one level so far)
    f.set_depth_filter(**STRONG)
    f.build(levels)                                               # (a new device frame: the wrapper hands the filter over again)
    twins = blank_frames(cam, 1)
    keep = ingest([f], [views[0]["grey"]], [views[0]["depth"]], "raw", "grey8", SCALE, "host", None, levels)
    keep += feed_twin(twins, [views[0]["grey"][..., None]], [tdf.filt(views[0]["depth"], STRONG, SCALE)], "raw", "grey8", "host", None, levels)
    assert_frames_equal(f, twins[0], levels, "grown")
    del keep


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------

def test_mixed_and_invalid_filters_and_an_aliased_source_change_nothing():
    ctx, cam, K, views, levels = small_setup()
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

    # one filtered frame among plain ones; two different filters
    d.set_depth_filter_batch(frames[:1])
    with pytest.raises(d.DvoHipError):
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", "current", levels)
    d.set_depth_filter_batch(frames[1:], gate=3.5)
    with pytest.raises(d.DvoHipError):
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "host", None, levels)
    with pytest.raises(d.DvoHipError):
        ingest(frames, [in_format(views[1]["bgr"], "bgr8")] * 3, other[1], "colour", "bgr8", SCALE, "device", None, levels, flags=_lib.INGEST_DEFER)
    unchanged()
    # invalid filters, straight at the C-ABI (the Python wrapper would refuse them first): the frames keep the filter they have
    handles = (C.c_void_p * 3)(*[f.ptr for f in frames])
    good = d.depth_filter_struct()
    for exc, params in tdf.BAD_PARAMS:
        if exc is TypeError:
            continue
        s = _lib.DepthFilter.from_buffer_copy(good)
        for k, v in params.items():
            setattr(s, k, float("inf") if k == "noise_b" and v > 1 else v)
        assert ctx._lib.dvo_hip_frames_set_depth_filter(ctx.ptr, 3, handles, C.byref(s)) == _lib.ERR_INVALID, params
    for reserved in ((0, 1), (7, 0)):
        s = _lib.DepthFilter.from_buffer_copy(good)
        s.reserved[:] = list(reserved)
        assert ctx._lib.dvo_hip_frames_set_depth_filter(ctx.ptr, 3, handles, C.byref(s)) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_set_depth_filter(ctx.ptr, 3, handles, None) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_set_depth_filter(ctx.ptr, 0, handles, C.byref(good)) == _lib.ERR_INVALID
    assert ctx._lib.dvo_hip_frames_clear_depth_filter(ctx.ptr, 3, None) == _lib.ERR_INVALID
    with pytest.raises(d.DvoHipError):                            # (still the mixed filters of above)
        ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", None, levels)
    unchanged()
    # one filter for all, but a float source that IS a frame's own level-0 plane (or overlaps its end)
    d.set_depth_filter_batch(frames)
    own_i, own_z = C.c_void_p(), C.c_void_p()
    ctx.check(ctx._lib.dvo_hip_frame_device_planes(frames[1].ptr, 0, C.byref(own_i), C.byref(own_z)))
    tz, pz, _ = device_bytes(before[0][1])
    ti, pi, _ = device_bytes(np.ascontiguousarray(grey[..., None]))
    for alias in (own_z.value, own_z.value + 320 * 239 * 4, own_i.value):
        with pytest.raises(d.DvoHipError):
            d.update_colour_device_batch(frames, [pi] * 3, [pz, alias, pz], "grey8", 320, 1.0, role=None, config=None, depth_format="f32",
                                         depth_pitch=320 * 4)
    for alias in (own_z.value + 320 * 240 * 4 - 1, own_i.value):  # ... and an image source there
        with pytest.raises(d.DvoHipError):
            d.update_colour_device_batch(frames, [pi, alias, pi], [pz] * 3, "grey8", 320, 1.0, role=None, config=None, depth_format="f32",
                                         depth_pitch=320 * 4)
    unchanged()
    # ... accepted from anywhere else, counted once per frame
    keep += ingest(frames, other[0], other[1], "raw", "grey8", SCALE, "device", None, levels)
    assert counters(ctx) == (c0[0] + 3, c0[1] + 3, c0[2], c0[3], c0[4])
    want = tdf.filt(views[1]["depth"], {}, SCALE)
    for f in frames:
        assert tdf.same_bits(plane_of(f)[1], want)
    del keep, tz, ti


# ---- 6. counters, a mixed batch ---------------------------------------------------------------------------------------------------------

def test_frames_without_a_filter_count_as_they_did():
    K, views = raw_scene(320, 240)
    ctx = d.Context()                                             # (a context of its own: nothing has been filtered in it)
    cam = camera(ctx, 320, 240, K, 3)
    frames = blank_frames(cam, 3)
    keep = ingest(frames, [views[0]["grey"]] * 3, [views[0]["depth"]] * 3, "raw", "grey8", SCALE, "device", "current", 3)
    keep += ingest(frames, [in_format(views[1]["bgr"], "bgr8")] * 3, [views[1]["fdepth"]] * 3, "mixed", "bgr8", 0.5, "host", None, 3)
    keep += ingest(frames, [in_format(views[1]["bgr"], "bgr8")] * 3, [views[1]["depth"]] * 3, "colour", "bgr8", SCALE, "device", None, 3,
                   flags=_lib.INGEST_DEFER)
    ctx.check(ctx._lib.dvo_hip_flush_deferred(ctx.ptr))
    plain = counters(ctx, INGEST_COUNTERS)
    # what these three ingests count on a build without the filter: 3 raw strip ingests, 3 colour + float-depth ones, 3 deferred colour ones
    assert plain[0] == 0 and plain[1:5] == (3, 6, 0, 0) and plain[6:] == (0, 1) and plain[5] >= 3
    d.set_depth_filter_batch(frames)
    assert counters(ctx, INGEST_COUNTERS) == plain               # (a filter alone counts nothing)
    keep += ingest(frames, [views[0]["grey"]] * 3, [views[0]["depth"]] * 3, "raw", "grey8", SCALE, "device", "current", 3)
    after = counters(ctx, INGEST_COUNTERS)
    assert after[0] == 3 and after[1] == plain[1] + 3 and after[2:5] == plain[2:5] and after[6:] == plain[6:]
    keep += ingest(frames[:2], [views[0]["grey"]] * 2, [views[0]["depth"]] * 2, "raw", "grey8", SCALE, "host", "reference", 3)
    assert ctx.counter("depth_filter_ingests") == 5
    del keep


def test_match_batch_mixes_filtered_and_plain_frames():
    ctx, cam, K, views, levels = small_setup()
    (a, b), frames, twins = ingest_pair(ctx, cam, views, levels)
    assert_records_identical(a, b)
    cfg = config(levels)
    mixed = match_records(ctx, cfg, [frames[0], twins[0], frames[0]], [twins[1], frames[1], frames[1]])
    plain = match_records(ctx, cfg, [twins[0], twins[0], twins[0]], [twins[1], twins[1], twins[1]])
    assert_records_identical(mixed, plain)


# ---- 7. repeatability -------------------------------------------------------------------------------------------------------------------

def test_the_same_ingest_twice_gives_identical_planes():
    ctx, cam, K, views, levels = small_setup()
    frames = blank_frames(cam, 2)
    d.set_depth_filter_batch(frames, **STRONG)
    images, depths = [v["grey"] for v in views], [v["depth"] for v in views]
    keep = ingest(frames, images, depths, "raw", "grey8", SCALE, "device", None, levels)
    first = [[plane_of(f, l) for l in range(levels)] for f in frames]
    keep += ingest(frames, images, depths, "raw", "grey8", SCALE, "device", None, levels)
    for f, planes in zip(frames, first):
        for l, (I, Z) in enumerate(planes):
            I2, Z2 = plane_of(f, l)
            assert tdf.same_bits(I, I2) and tdf.same_bits(Z, Z2), l
    assert not tdf.same_bits(first[0][0][1], first[1][0][1])
    del keep


# ---- 8. the facade ----------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_depth_filter():
    d.build()
    out = subprocess.run([tdf.build_depth_filter_facade_check()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
