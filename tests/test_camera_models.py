"""CPU tier: the host build of the device headers (tests/emul/emul_device.cpp) against the oracle's MATH mode under every camera of
tests/cameras.py -- not only the fr1 intrinsics every other alignment test feeds it.

  * pixel math: both emulation forms, every level, the statement of test_pixel_math_bit_exact_against_oracle (counts and residuals
    bit-exact, A and b within 1e-6 of the largest entry, the weighted second pass too);
  * whole matches at Precision 1e-4 on 320 x 240: the same iteration structure, T within 2e-5; the speculative control flow of the
    resident kernel leaves the plain loop's bytes;
  * level intrinsics: the oracle's K of level l is K halved l times in float32 (Q17) -- the number tests/test_gpu_camera_models.py
    holds the device's K against.

No whole match at the stopping precision 5e-7 below 640 x 480: on 160 x 120, two implementations whose residuals are bit-identical
end up to 1.98e-6 apart in T (wide, seed 9) and 2.7e-5 apart in an increment (tele, seed 8) -- the runs end on the noise floor one
pass apart -- which is outside the suite's 1e-6 / 2e-5 for that precision without any arithmetic being wrong."""
import numpy as np
import pytest

import cameras
import common as cm
import dvo_slam_amd as d
from oracle import pyoracle as po

XI = np.array([0.004, -0.003, 0.002, 0.005, -0.004, 0.003])


@pytest.fixture
def schedule():
    L = cm.emul_lib()
    yield L.emul_set_schedule
    L.emul_set_schedule(0)


def test_camera_set():
    """what the set is there to separate (tests/cameras.py), so that an edit of the table cannot quietly make it forgiving again"""
    for w, h in ((160, 120), (131, 97), (320, 240)):
        cams = cameras.CAMERAS(w, h)
        assert tuple(cams) == cameras.NAMES
        assert all(K.dtype == np.float32 and K.shape == (4,) and np.isfinite(K).all() and K[0] > 0 and K[1] > 0 for K in cams.values())
        assert np.array_equal(cams["fr1"], cm.synth(0, w, h)["K"])                  # the generators' default
        fx, fy, ox, oy = cams["aniso"]
        assert fy > 2 * fx and abs(ox - w / 2) > 0.1 * w and abs(oy - h / 2) > 0.1 * h and abs(ox / w - oy / h) > 0.2
        assert 2 * np.degrees(np.arctan(0.5 * w / cams["wide"][0])) > 109
        assert cams["tele"][0] > 3 * cams["fr1"][0]
        assert cams["outside"][2] < 0 and cams["outside"][3] > h


@pytest.mark.parametrize("w,h,levels", [(160, 120, 3), (131, 97, 2)])
@pytest.mark.parametrize("name", cameras.NAMES)
def test_pixel_math_bit_exact_against_oracle_per_camera(name, w, h, levels, schedule):
    K = cameras.CAMERAS(w, h)[name]
    pair = cm.synth(23, w, h, K)
    assert np.array_equal(pair["K"], K)
    ref, cur = cm.oracle_pyramids(pair, levels)
    ep = cm.EmulPair(ref, cur, levels)
    T34 = po.se3_exp(XI)[:3]
    for level in reversed(range(levels)):
        o = po.level_iteration(ref, cur, level, T34, first=True, mode=po.MATH, want_residuals=True)
        o2 = po.level_iteration(ref, cur, level, T34, P_prev=o["P"], first=False, mode=po.MATH, want_residuals=True)
        assert o["n"] >= 0.2 * o["n_selected"] and o["n"] >= 100, (name, level, o["n"], o["n_selected"])   # (not a vacuous comparison)
        for form in (0, 1):
            schedule(form)
            e = ep.level_iteration(level, T34, first=True)
            what = (name, level, form)
            assert e["n"] == o["n"] and e["n_selected"] == o["n_selected"], what
            assert np.array_equal(np.isnan(e["residuals"]), np.isnan(o["residuals"])), what
            assert np.array_equal(np.nan_to_num(e["residuals"]), np.nan_to_num(o["residuals"])), what
            assert np.allclose(e["P"], o["P"], rtol=1e-5), what
            assert abs(e["neg_ll"] - o["neg_ll"]) <= 1e-7 * abs(o["neg_ll"]), what
            assert np.abs(e["A"] - o["A"]).max() <= 1e-6 * np.abs(o["A"]).max(), what
            assert np.abs(e["b"] - o["b"]).max() <= 1e-6 * np.abs(o["b"]).max(), what
            e2 = ep.level_iteration(level, T34, P_prev=o["P"], first=False)
            assert e2["n"] == o2["n"], what
            assert np.array_equal(np.nan_to_num(e2["residuals"]), np.nan_to_num(o2["residuals"])), what
            assert np.abs(e2["A"] - o2["A"]).max() <= 1e-6 * np.abs(o2["A"]).max(), what
            assert np.abs(e2["b"] - o2["b"]).max() <= 1e-6 * np.abs(o2["b"]).max(), what


# (name, seed, Mu, UseInitialEstimate)
MATCHES = [(name, 7 + i, 0.0, False) for i, name in enumerate(cameras.NAMES)] + [("aniso", 8, 0.05, True)]


@pytest.mark.parametrize("name,seed,mu,init", MATCHES)
def test_state_machine_against_oracle_driver_per_camera(name, seed, mu, init):
    w, h = 320, 240
    pair = cm.synth(seed, w, h, cameras.CAMERAS(w, h)[name])
    ref, cur = cm.oracle_pyramids(pair, 3)
    ep = cm.EmulPair(ref, cur, 3)
    cfg = d.Config(FirstLevel=2, LastLevel=0, Mu=mu, UseInitialEstimate=init, Precision=1e-4, MaxIterationsPerLevel=50 if init else 100)
    T0 = po.se3_exp(0.5 * pair["xi_true"]) if init else None
    e = ep.match(cfg, T0, raw=True)
    o = po.match(ref, cur, cm.oracle_config_from(cfg, po.MATH), T0)
    s = cm.compare_runs(e, o)
    print(name, s)
    assert s["structure_mismatch"] == 0 and s["n_mismatch"] == 0, s
    assert s["T_err"] < 2e-5 and s["max_x_err"] < 2e-5, s
    assert np.abs(po.se3_log(e["T"]) - pair["xi_true"]).max() < 1e-3            # ... and the match found the motion
    if name in ("aniso", "outside"):
        spec = ep.match(cfg, T0, speculative=True, raw=True)
        assert spec["raw"] == e["raw"]


@pytest.mark.parametrize("w,h,levels", [(160, 120, 3), (131, 97, 2), (320, 240, 3), (130, 34, 2)])
@pytest.mark.parametrize("name", cameras.NAMES)
def test_level_intrinsics_are_float32_halvings(name, w, h, levels):
    K = cameras.CAMERAS(w, h)[name]
    ref, _ = cm.oracle_pyramids(cm.synth(17, w, h, K), levels)
    for l in range(levels):
        assert np.array_equal(ref.plane(l, 0)[1], cameras.level_K(K, l)), (name, l)
