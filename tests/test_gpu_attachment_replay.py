"""GPU tier: a pyramid that grows levels keeps EVERY attachment at once.  RgbdImagePyramid.build makes the device frame anew and hands
over again what the old one carried, from one table (dvo_slam_amd/attachments.py, ATTACHMENTS); the per-attachment tests grow a pyramid
that carries one thing.  Here a pyramid created with one level, given several attachments and grown to three equals, after the same
re-ingest, its TWIN that had three levels from the start: every plane of every level bit for bit, the selection counts, the colour.
No oracle, so no tolerance."""
import numpy as np
import pytest

import dvo_slam_amd as d
from test_gpu_lens_ingest import raw_scene

pytestmark = pytest.mark.gpu
W, H, LEVELS = 64, 48, 3                                          # level 2 is 16 x 12: the filter's radius-2 stencil and the rectifier still see an interior
PLANES = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")
THRESHOLDS = ((0.0, 0.0), (4.0, 0.02))
RANGE = (0.6, 3.5)                                                # the selections' depth range, metres


def attach_a(p, K, mask):
    """a depth rig, a lens that leaves the depth plane alone, a depth filter, a host mask with a depth range"""
    p.set_depth_rig(K * np.float32(0.97), [[1, 0, 0, 0.02], [0, 1, 0, -0.01], [0, 0, 1, 0.005]])
    p.set_lens(K * np.float32(1.03), [0.08, -0.03, 0.001, -0.002, 0.01], rectify_depth=False)
    p.set_depth_filter()
    p.set_selection(mask, *RANGE)


def attach_b(p, bgr):
    """colour (which a lens excludes), a depth filter, a depth range without a mask"""
    p.set_colour(bgr, "bgr8")
    p.set_depth_filter(radius=1, hole_radius=1)
    p.set_selection(None, *RANGE)


def planes_of(p):
    return [[np.asarray(getattr(p.level(l), name)).view(np.uint32) for name in PLANES] for l in range(LEVELS)]


def counts_of(p):
    return [[d.PointSelection(p, *thr).select(l) for thr in THRESHOLDS] for l in range(LEVELS)]


@pytest.mark.parametrize("which", ["rig-lens-filter-mask", "colour-filter-range"])
def test_a_pyramid_that_grows_levels_keeps_all_its_attachments(which):
    K, views = raw_scene(W, H)
    grey, depth, bgr = views[0]["grey"], views[0]["depth"], views[0]["bgr"]
    mask = (np.random.default_rng(7).random((H, W)) < 0.7).astype(np.uint8)
    ctx = d.default_context()
    attach = (lambda p: attach_a(p, K, mask)) if which.startswith("rig") else (lambda p: attach_b(p, bgr))

    grown = d.RgbdCameraPyramid(W, H, K, ctx).create_raw(grey, depth)          # (one level so far)
    attach(grown)
    grown.build(LEVELS)                                                        # (a new device frame: everything is handed over again)
    cam = d.RgbdCameraPyramid(W, H, K, ctx)
    cam.build(LEVELS)
    twin, plain = cam.create_raw(grey, depth), cam.create_raw(grey, depth)
    attach(twin)
    assert grown.levels == twin.levels == LEVELS
    for p in (grown, twin, plain):
        d.update_raw_host_batch([p], [grey], [depth])
    d.upload_wait(ctx)

    got, want = planes_of(grown), planes_of(twin)
    for l in range(LEVELS):
        for name, x, y in zip(PLANES, got[l], want[l]):
            assert np.array_equal(x, y), (which, l, name)
    assert counts_of(grown) == counts_of(twin)
    if which.startswith("colour"):
        for l in range(LEVELS):
            assert np.array_equal(grown.colour(l), twin.colour(l)), (which, l)
    # (the twin is no trivial yardstick: what it carries changed its depth plane and its selection)
    assert not np.array_equal(want[0][1], planes_of(plain)[0][1]) and counts_of(twin) != counts_of(plain)
