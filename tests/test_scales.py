"""CPU tier: the oracle's MATH mode under a change of the intensity's scale, and the scale-free metric of tests/common.py.

Multiplying both grey planes by 2^k changes every intensity-derived float32 by the same power of two exactly (products with a power
of two are exact, and nothing else in the arithmetic is an absolute constant of the intensity): the constraint set and the normal
equations do not move by a bit, the intensity residuals are x 2^k, the precision matrix is S P S with S = diag(2^-k, 1), and a whole
match ends at the same transform with the same information matrix.  It breaks only where the float32 range ends (k = -20: products of
two gradients underflow).  The device tier (tests/test_gpu_scales.py) relies on this: the oracle adds no error of its own with the
scale, so whatever grows with |k| there is the device's.
"""
import functools

import numpy as np
import pytest

import common as cm
from oracle import pyoracle as po

SEED = 23
SHAPES = [(160, 120), (131, 97)]
KI = [-4, -8, -12, -16]
# the scales of the device tier (intensity, depth), and its shapes
DEVICE_SCALES = [(0, 0), (-4, 0), (-8, 0), (-12, 0), (0, -2), (0, 2), (0, 4), (-8, 4), (-12, 4)]
DEVICE_SHAPES = [(160, 120), (258, 194), (131, 97), (80, 60)]


@functools.lru_cache(maxsize=None)
def passes(w, h, ki, kz, levels=1):
    """(first pass, weighted pass with the first one's P) of level 0 at the warp of the single-linearisation tests"""
    sp = cm.scaled_pair(cm.synth(SEED, w, h), ki, kz)
    oref, ocur = cm.scaled_oracle_pyramids(sp, levels)
    T34 = cm.scaled_warp(cm.SCALE_XI, kz)
    o1 = po.level_iteration(oref, ocur, 0, T34, first=True, mode=po.MATH, want_residuals=True)
    o2 = po.level_iteration(oref, ocur, 0, T34, P_prev=o1["P"], first=False, mode=po.MATH, want_residuals=True)
    return o1, o2


@functools.lru_cache(maxsize=None)
def whole_match(w, h, ki):
    sp = cm.scaled_pair(cm.synth(SEED, w, h), ki, 0)
    oref, ocur = cm.scaled_oracle_pyramids(sp, 3)
    return po.match(oref, ocur, po.make_config(2, 0, 100, 5e-7, mode=po.MATH))


def test_scaled_pair_is_exact_and_leaves_the_holes():
    pair = cm.synth(SEED, 131, 97)
    sp = cm.scaled_pair(pair, -12, 4)
    assert sp["grey_ref"].dtype == np.float32 and sp["depth_cur"].dtype == np.float32
    assert np.array_equal(sp["grey_cur"] * np.float32(4096.0), pair["grey_cur"].astype(np.float32))
    z = po.convert_raw_depth(pair["depth_ref"])
    assert np.array_equal(sp["depth_ref"], z * np.float32(16.0), equal_nan=True) and np.isnan(z).any()
    assert np.array_equal(sp["xi_true"], pair["xi_true"] * np.array([16.0, 16.0, 16.0, 1.0, 1.0, 1.0]))
    T, T0 = cm.scaled_warp(cm.SCALE_XI, 4), cm.scaled_warp(cm.SCALE_XI, 0)
    assert np.array_equal(T[:, :3], T0[:, :3]) and np.array_equal(T[:, 3], 16.0 * T0[:, 3])
    assert np.array_equal(T.astype(np.float32)[:, 3], np.float32(16.0) * T0.astype(np.float32)[:, 3])


@pytest.mark.parametrize("ki", KI)
@pytest.mark.parametrize("w,h", SHAPES)
def test_linearisation_is_exactly_covariant_under_intensity_scaling(w, h, ki):
    s = 2.0 ** ki
    S = np.array([1.0 / s, 1.0])
    for o0, ok in zip(passes(w, h, 0, 0), passes(w, h, ki, 0)):
        assert ok["n"] == o0["n"] and ok["n_selected"] == o0["n_selected"] and o0["n"] > 2800
        assert np.array_equal(ok["A"], o0["A"]) and np.array_equal(ok["b"], o0["b"])
        assert np.array_equal(ok["residuals"][:, :, 0], o0["residuals"][:, :, 0] * np.float32(s), equal_nan=True)
        assert np.array_equal(ok["residuals"][:, :, 1], o0["residuals"][:, :, 1], equal_nan=True)
        assert np.array_equal(ok["P"], o0["P"] * np.outer(S, S))


@pytest.mark.parametrize("ki", KI)
@pytest.mark.parametrize("w,h", SHAPES)
def test_whole_match_does_not_move_under_intensity_scaling(w, h, ki):
    a, b = whole_match(w, h, 0), whole_match(w, h, ki)
    assert np.array_equal(a["T"], b["T"]) and np.array_equal(a["information"], b["information"])
    assert [len(L["iterations"]) for L in a["levels"]] == [len(L["iterations"]) for L in b["levels"]]
    assert np.isfinite(a["T"]).all() and cm.twist_matrix_error(a["T"], np.eye(4)) > 1e-3


@pytest.mark.parametrize("w,h", DEVICE_SHAPES)
def test_metric_and_its_bound_on_the_oracle_itself(w, h):
    """The oracle against itself at scale (0, 0) is inside the bound (trivially: zero); an error planted in the smallest diagonal entry
    of A, 1e-5 of the LARGEST entry in size, sits exactly on it; kappa0 is what the issue measured (6-7 for A, 10-15 for P at 160 x
    120); and every scale of the device tier keeps n >= 2800 at every shape."""
    for o in passes(w, h, 0, 0):
        kA, kP, kb = cm.kappa0(o["A"]), cm.kappa0(o["P"]), cm.kappa0_b(o["A"], o["b"])
        e = cm.scale_errors(o, o)
        assert e["errA"] == 0.0 and e["errb"] == 0.0 and e["errP"] == 0.0
        assert e["errA"] <= 1e-5 * kA and e["errb"] <= 1e-5 * kb and e["errP"] <= 1e-5 * kP
        assert 1.0 <= kA < 50.0 and 1.0 <= kP < 100.0 and 1.0 <= kb < 50.0, (kA, kP, kb)
        i = int(np.argmin(np.diag(o["A"])))
        g = dict(A=o["A"].copy(), b=o["b"].copy(), P=o["P"].copy())
        g["A"][i, i] += 1e-5 * np.abs(o["A"]).max()
        g["b"][i] += 1e-5 * np.abs(o["b"]).max()
        e = cm.scale_errors(g, o)
        assert e["errA"] == pytest.approx(1e-5 * kA, rel=1e-6) and e["errb"] == pytest.approx(1e-5 * kb, rel=1e-6) and e["errP"] == 0.0
    for ki, kz in DEVICE_SCALES:
        for o in passes(w, h, ki, kz):
            assert o["n"] >= 2800, (w, h, ki, kz, o["n"])


def test_metric_sees_a_small_block_that_the_largest_entry_hides():
    """Depth x 16: the translation block of A is three orders of magnitude below the rotation block.  Half a per cent of error in
    that block passes "1e-5 of the largest entry" and fails the metric by a factor of more than fifty."""
    o = passes(160, 120, 0, 4)[0]
    assert cm.kappa0(o["A"]) > 500.0
    g = dict(A=o["A"].copy(), b=o["b"], P=o["P"])
    g["A"][:3, :3] *= 1.005
    assert np.abs(g["A"] - o["A"]).max() <= 1e-5 * np.abs(o["A"]).max()
    assert cm.scale_errors(g, o)["errA"] > 50.0 * 1e-5 * cm.kappa0(passes(160, 120, 0, 0)[0]["A"])
