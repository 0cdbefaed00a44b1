"""CPU tier: the edge scene of tests/scenes.py keeps the content that tests/test_gpu_scene_edges.py relies on.

A later edit of the generator must not silently lose what makes it worth running: lane pairs (2l, 2l + 1) with one valid and one
invalid pixel at levels 0-2, validity changes between two rows of one 8-row strip, holes on the strip rows and columns and the border,
depth below 0.5 m and above 8 m, and -- at the true pose -- hundreds of selected pixels rejected by each of the bounds (Q4), NaN-tap
(Q9) and occlusion (Q5) tests.  The minimum counts are about a third of what seed 1 at 640 x 480 produces (comments)."""
import numpy as np
import pytest

import scenes
from oracle import pyoracle as po

W, H = 640, 480


@pytest.fixture(scope="module")
def pair():
    return scenes.edge_scene(1, W, H)


@pytest.fixture(scope="module")
def pyramids(pair):
    return po.pyramids_from_pair(pair, 4)


def true_warp(pair):
    """the float32 warp reference -> current of the true pose (what the kernels are handed), widened back to float64"""
    return np.linalg.inv(po.se3_exp(pair["xi_true"])).astype(np.float32).astype(np.float64)


def test_deterministic_and_shaped_like_synth_pair(pair):
    again = scenes.edge_scene(1, W, H)
    synth = po.synth_pair(1, 64, 48)
    assert set(pair) == set(synth)
    for k in pair:
        assert np.array_equal(pair[k], again[k]), k
        assert np.asarray(pair[k]).dtype == np.asarray(synth[k]).dtype, k
    assert pair["grey_ref"].shape == pair["depth_cur"].shape == (H, W)
    assert not np.array_equal(scenes.edge_scene(2, W, H)["depth_ref"], pair["depth_ref"])


def test_depth_range_and_holes(pair):
    for view in ("ref", "cur"):
        raw = pair["depth_" + view]
        z = raw[raw > 0] / 5000.0
        assert z.min() < 0.5 and z.max() > 8.0 and raw.max() <= scenes.SENSOR_RANGE_RAW        # measured: 0.32 m, 12.0 m
        assert (z < 0.5).sum() > 2000 and (z > 8.0).sum() > 20000
        hole = raw == 0
        assert 0.04 < hole.mean() < 0.15                                                        # measured: 0.084 / 0.088
        assert hole[:20].mean() > 0.3                     # the top rows: the plane beyond the sensor range (raw 0 there)
        rows = np.arange(H)
        assert hole[rows % 8 == 7].sum() > 100 and hole[(rows % 8 == 0) & (rows > 0)].sum() > 100
        assert hole[:, 127].sum() > 10 and hole[:, 128].sum() > 10 and hole[:, 255].sum() > 10 and hole[:, 256].sum() > 10
        assert hole[H - 1].sum() > 5 and hole[:, 0].sum() > 5 and hole[:, W - 1].sum() > 5
        for px in range(2):                               # isolated holes at every parity of x and y
            for py in range(2):
                inner = hole[1 + py:H - 1:2, 1 + px:W - 1:2]
                ys, xs = np.nonzero(inner)
                ys, xs = 2 * ys + 1 + py, 2 * xs + 1 + px
                alone = ~hole[ys - 1, xs] & ~hole[ys + 1, xs] & ~hole[ys, xs - 1] & ~hole[ys, xs + 1]
                assert alone.sum() >= 20, (view, px, py)


def test_validity_crosses_lane_pairs_and_strips(pyramids):
    ref, cur = pyramids
    want_mixed = {0: 2000, 1: 300, 2: 100}                # measured (reference frame): 6537, 1002, 383
    for pyr in (ref, cur):
        for level, least in want_mixed.items():
            valid = ~np.isnan(pyr.plane(level, 1)[0])
            assert (valid[:, 0::2] != valid[:, 1::2]).sum() >= least, level
        valid = ~np.isnan(pyr.plane(0, 1)[0])
        inside = np.arange(H - 1) % 8 != 7                # row y and y + 1 in the same 8-row strip
        assert (valid[:-1] != valid[1:])[inside].sum() >= 1000                                   # measured: 4361


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_classifier_restates_the_oracle_and_every_class_occurs(pair, pyramids, level):
    """The float64 classifier puts exactly the oracle's constraints (MATH mode) in VALID, apart from pixels it calls ambiguous; at the
    true pose every rejection class holds hundreds of selected pixels at level 0 (measured: 8914 out of bounds, 33107 NaN taps, 6141
    occluded)."""
    ref, cur = pyramids
    T = true_warp(pair)
    n_sel, mask = ref.select(level)
    cls, amb = scenes.classify(ref.plane(level, 1)[0], mask, [cur.plane(level, k)[0] for k in range(6)], ref.plane(level, 0)[1], T)
    o = po.level_iteration(ref, cur, level, T[:3], first=True, mode=po.MATH, want_residuals=True)
    valid = ~np.isnan(o["residuals"][:, :, 0])
    assert o["n_selected"] == n_sel == int((cls >= 0).sum())
    assert not ((cls == scenes.VALID) != valid)[~amb].any()
    assert amb.sum() <= max(1, int(1e-4 * o["n"]))
    counts = [int(((cls == c) & ~amb).sum()) for c in (scenes.OUT_OF_BOUNDS, scenes.NAN_TAP, scenes.OCCLUDED)]
    least = [3000, 10000, 2000] if level == 0 else [50, 300, 20]
    assert all(c >= m for c, m in zip(counts, least)), counts
