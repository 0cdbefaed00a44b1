"""GPU tier (-m gpu): the kernels against the CPU oracle on the edge scenes of tests/scenes.py.

datagen.synth_pair never puts a validity change inside a lane pair (2l, 2l + 1) or inside an 8-row strip, never leaves 1.0-2.3 m and
never occludes anything at the true pose.  The edge scene does all of that (tests/test_scenes.py checks that it keeps doing it): a
slanted plane from 3 m to beyond the sensor range, boxes at 0.3-0.8 m, holes of every parity and on the strip rows and columns.  Here:
  * planes and selection of every ingest path, bit-exact against the oracle, in both roles;
  * one linearisation on levels 0-3 at the true pose and off it: the exact schedules and ref_compat bit-exact, the default schedule
    within its stated bounds and per matrix entry, and every pixel's constraint decision against the float64 classifier;
  * whole matches on the resident kernel and on the launch path against the oracle (and the reference's own match() when built).
Every comparison is kernel against a CPU reference; nothing is compared only with another GPU path."""
import functools

import numpy as np
import pytest

import common as cm
import dvo_slam_amd as d
import scenes
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
NAMES = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")
SEED = 1
OFF = np.array([0.004, -0.003, 0.002, 0.005, -0.004, 0.003])        # the pose off the truth: T_true exp(OFF)
Q1 = po.QUIRKS | po.Q_RCP_PROJECTION | po.Q_RCP_WEIGHTS               # the oracle's mode that option ref_compat reproduces


@functools.lru_cache(maxsize=None)
def scene(seed, w, h):
    return scenes.edge_scene(seed, w, h)


@functools.lru_cache(maxsize=None)
def oracle_pyramids(seed, w, h, levels, scale=None):
    p = scene(seed, w, h)
    if scale is None:
        return cm.oracle_pyramids(p, levels)
    return tuple(po.Pyramid(p["grey_" + v].astype(np.float32), po.convert_raw_depth(p["depth_" + v], scale), p["K"], levels)
                 for v in ("ref", "cur"))


def true_warp(p):
    """the warp reference -> current of the true pose (match() returns its inverse)"""
    return np.linalg.inv(po.se3_exp(p["xi_true"]))


def warps(p):
    T = true_warp(p)
    return (("true", T[:3].astype(np.float32)), ("off", (T @ po.se3_exp(OFF))[:3].astype(np.float32)))


def camera(ctx, p, levels):
    h, w = p["grey_ref"].shape
    cam = d.RgbdCameraPyramid(w, h, p["K"], ctx)
    cam.build(levels)
    return cam


def assert_frame_equals_oracle(frame, opyr, levels, what):
    """all six planes of every level, the selection mask and count (default and non-zero thresholds): bit for bit"""
    for l in range(levels):
        img = frame.level(l)
        for k, name in enumerate(NAMES):
            o, K = opyr.plane(l, k)
            g = np.asarray(getattr(img, name))
            assert g.shape == o.shape and np.array_equal(g, o, equal_nan=True), (what, l, name)
        assert np.array_equal(img.K, K), (what, l)
        for thr in ((0.0, 0.0), (6.0, 0.03)):
            n, mask = d.PointSelection(frame, *thr).select(l, want_mask=True)
            on, omask = opyr.select(l, *thr)
            assert n == on and np.array_equal(mask, omask), (what, l, thr, n, on)


def assert_linearisation_bit_exact(trk, gref, gcur, oref, ocur, level, T34, mode, what):
    """residuals and valid counts of a first pass bit-identical to the oracle's `mode`"""
    o = po.level_iteration(oref, ocur, level, T34, first=True, mode=mode, want_residuals=True)
    g = trk.level_iteration(gref, gcur, level, T34, first=True, want_residuals=True)
    assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"], (what, g["n"], o["n"])
    assert np.array_equal(g["residuals"], o["residuals"], equal_nan=True), what


# ---- 1. planes and selection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", [(640, 480, 4), (1280, 960, 5), (388, 122, 4), (140, 62, 3), (132, 34, 4),
                                        (102, 78, 3)])      # an odd half width: k_build_from_raw, not the strips
def test_planes_and_selection_bit_exact(gpu_ctx, w, h, levels):
    """Every ingest path against the oracle's pyramids: create_raw; frames_update_raw_as in the reference and the current role and
    each frame then used in the OTHER role (selection from a current frame's raw copy, planes of a reference frame); the current
    role's plane-C-only flavour (more frames in one call than the device has compute units); create_f32; a raw ingest at another
    depth scale.  Both frames of the pair; a linearisation on the role-ingested frames in both roles, bit-exact."""
    p = scene(SEED, w, h)
    oref, ocur = oracle_pyramids(SEED, w, h, levels)
    cam = camera(gpu_ctx, p, levels)
    cfg = d.Config(FirstLevel=levels - 1, LastLevel=0)
    grey = {v: np.ascontiguousarray(p["grey_" + v]) for v in ("ref", "cur")}
    raw = {v: np.ascontiguousarray(p["depth_" + v]) for v in ("ref", "cur")}
    opyr = {"ref": oref, "cur": ocur}
    for v in ("ref", "cur"):
        assert_frame_equals_oracle(cam.create_raw(grey[v], raw[v]), opyr[v], levels, ("create_raw", v))
        assert_frame_equals_oracle(cam.create(grey[v].astype(np.float32), po.convert_raw_depth(raw[v])), opyr[v], levels, ("create_f32", v))
    s_ref, s_cur = oracle_pyramids(SEED, w, h, levels, 1.0 / 1000.0)
    assert_frame_equals_oracle(cam.create_raw(grey["ref"], raw["ref"], depth_scale=1.0 / 1000.0), s_ref, levels, "depth_scale 1/1000")
    # role-aware ingest, each view in each role
    dummy = np.zeros((h, w), np.uint8), np.full((h, w), 5000, np.uint16)
    trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), gpu_ctx)
    gpu_ctx.set_option("variant", 7)
    try:
        for role in ("reference", "current"):
            F = [cam.create_raw(*dummy) for _ in range(2)]
            d.update_raw_host_batch(F, [grey["ref"], grey["cur"]], [raw["ref"], raw["cur"]], role=role, config=cfg)
            for f, v in zip(F, ("ref", "cur")):
                assert_frame_equals_oracle(f, opyr[v], levels, (role, v))
            d.update_raw_host_batch(F, [grey["ref"], grey["cur"]], [raw["ref"], raw["cur"]], role=role, config=cfg)
            T34 = warps(p)[1][1]
            assert_linearisation_bit_exact(trk, F[0], F[1], oref, ocur, 0, T34, po.MATH, (role, "forward"))
            assert_linearisation_bit_exact(trk, F[1], F[0], ocur, oref, 0, T34, po.MATH, (role, "backward"))
        if w * h <= 640 * 480:
            # plane C only: 300 current frames in one call; A + B derived on download, the reference role from the raw copy
            n = 300
            F = [cam.create_raw(*dummy) for _ in range(n)]
            gs = [grey["ref"] if i % 2 == 0 else grey["cur"] for i in range(n)]
            zs = [raw["ref"] if i % 2 == 0 else raw["cur"] for i in range(n)]
            d.update_raw_host_batch(F, gs, zs, role="current", config=cfg)
            assert_linearisation_bit_exact(trk, F[0], F[1], oref, ocur, 0, warps(p)[0][1], po.MATH, "plane C, forward")
            d.update_raw_host_batch(F, gs, zs, role="current", config=cfg)
            assert_linearisation_bit_exact(trk, F[n - 1], F[n - 2], ocur, oref, 0, warps(p)[0][1], po.MATH, "plane C, backward")
            d.update_raw_host_batch(F, gs, zs, role="current", config=cfg)
            for i in (0, 1, n - 1):
                assert_frame_equals_oracle(F[i], opyr["ref" if i % 2 == 0 else "cur"], levels, ("plane C", i))
    finally:
        gpu_ctx.set_option("variant", 8)


# ---- 2. one linearisation --------------------------------------------------------------------------------------------------------
def per_entry_error(g, o):
    """max over entries of |g - o| / sqrt(|o_ii o_jj|) (a vector: / |o_i|)"""
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    if o.ndim == 1:
        return float((np.abs(g - o) / np.abs(o)).max())
    dg = np.sqrt(np.abs(np.diag(o)))
    return float((np.abs(g - o) / np.outer(dg, dg)).max())


# The default schedule (variant 8) on depth edges.  Its tap coordinates are within a few ulp of the exact ones, and across a depth edge
# the blend moves by metres per pixel: residuals of edge pixels differ from the oracle's by up to 7.9e-4 m (level 0, true pose), not
# the 4e-6 m test_default_schedule_single_linearisation_against_oracle states for the smooth synthetic surface.  Stated here per pixel
# instead: |dr| <= (the smooth-scene bound) + EPS_UV (w + h) * (the blend's slope at the pixel).  The normal equations move with them:
# measured worst over levels 0-3, both poses and both passes: A 4.5e-5 (level 0, true pose, second pass) and b 1.7e-4 (level 1, true
# pose, second pass) of the largest entry; per entry (tol sqrt(|X_ii X_jj|)) P 3.4e-5 (level 0, true pose, first pass) and A 4.5e-5.
EPS_UV = 2.5e-7
VARIANT8_REL = {"A": 1e-4, "b": 2e-4}
VARIANT8_PER_ENTRY = 1e-4


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_linearisation_at_depth_edges(level):
    """One linearisation of the 640 x 480 edge scene at the true pose and off it, first pass and weighted second pass:
      * variants 0, 5, 6, 7: valid counts and residuals bit-identical to the oracle's MATH mode; P, A, b within 1e-5 of the largest
        entry (test_single_linearisation_against_oracle);
      * option ref_compat (variant 7): bit-identical to MATH + Q1;
      * the default schedule (variant 8): the constraint set, P and -ll within the bounds of
        test_default_schedule_single_linearisation_against_oracle; residuals per pixel and A, b as stated at EPS_UV; per entry
        |X_gpu - X_oracle|_ij <= tol sqrt(|X_ii X_jj|) for P and A;
      * every pixel's constraint decision (residual NaN or not) of variants 7 and 8 equals the float64 classifier's except at pixels
        it calls ambiguous (<= 1e-4 of n); the occluded pixels are rejected by the GPU."""
    p = scene(SEED, 640, 480)
    levels = level + 1
    oref, ocur = oracle_pyramids(SEED, 640, 480, 4)
    ctx = d.Context(0)
    cam = camera(ctx, p, levels)
    gref, gcur = cam.create_raw(p["grey_ref"], p["depth_ref"]), cam.create_raw(p["grey_cur"], p["depth_cur"])
    trk = d.DenseTracker(d.Config(FirstLevel=level, LastLevel=level), ctx)
    n_sel, mask = oref.select(level)
    cur_planes = [ocur.plane(level, k)[0] for k in range(6)]
    worst = {}
    for name, T34 in warps(p):
        T = np.vstack([T34.astype(np.float64), [0, 0, 0, 1]])
        cls, amb, slope_I, slope_Z = scenes.classify(oref.plane(level, 1)[0], mask, cur_planes, oref.plane(level, 0)[1], T, slopes=True)
        eps = EPS_UV * (cls.shape[0] + cls.shape[1])
        P_prev = None
        for first in (True, False):
            o = po.level_iteration(oref, ocur, level, T34, P_prev=P_prev, first=first, mode=po.MATH, want_residuals=True)
            ro = o["residuals"]
            for variant in (0, 5, 6, 7, 8):
                ctx.set_option("variant", variant)
                g = trk.level_iteration(gref, gcur, level, T34, P_prev=P_prev, first=first, want_residuals=True)
                rg = g["residuals"]
                assert g["n_selected"] == o["n_selected"] == n_sel
                vg = ~np.isnan(rg[:, :, 0])
                if variant == 8:
                    vo = ~np.isnan(ro[:, :, 0])
                    flipped = int((vo != vg).sum())
                    both = vo & vg
                    d0 = float(np.abs(ro[both, 0] - rg[both, 0]).max())
                    d1 = float(np.abs(ro[both, 1] - rg[both, 1]).max())
                    rel = {k: np.abs(g[k] - o[k]).max() / np.abs(o[k]).max() for k in ("P", "A", "b")}
                    rell = abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"])
                    ent = {k: per_entry_error(g[k], o[k]) for k in ("P", "A", "b")}
                    print("level %d %s first=%d variant 8: n %d vs %d, %d flipped, |dr_I| %.2e |dr_Z| %.2e, P %.1e A %.1e b %.1e -ll %.1e, "
                          "per entry P %.1e A %.1e b %.1e" % (level, name, first, g["n"], o["n"], flipped, d0, d1, rel["P"], rel["A"],
                                                             rel["b"], rell, ent["P"], ent["A"], ent["b"]))
                    assert g["n"] == int(vg.sum()) and flipped <= max(1, int(1e-4 * o["n"]))
                    assert (np.abs(ro[both, 0] - rg[both, 0]) <= 2e-5 + eps * slope_I[both] / 255.0).all()
                    assert (np.abs(ro[both, 1] - rg[both, 1]) <= 4e-6 + eps * slope_Z[both]).all()
                    slack = 20.0 * flipped / o["n"]
                    assert rel["P"] <= 1e-5 + slack and rel["A"] <= VARIANT8_REL["A"] + slack and rel["b"] <= VARIANT8_REL["b"] + slack
                    assert rell <= 2e-5 + slack
                    for k, e in ent.items():
                        if k == "b":
                            continue                    # (b_i near the solution is a difference of large terms: bounded above by rel["b"])
                        worst[k] = max(worst.get(k, 0.0), e)
                        assert e <= VARIANT8_PER_ENTRY + slack, (name, first, k, e)
                else:
                    assert g["n"] == o["n"], (variant, name, first)
                    assert np.array_equal(rg, ro, equal_nan=True), (variant, name, first)
                    for k in ("P", "A", "b"):
                        assert np.abs(g[k] - o[k]).max() <= 1e-5 * np.abs(o[k]).max(), (variant, k)
                    assert abs(g["neg_ll"] - o["neg_ll"]) <= 1e-6 * abs(o["neg_ll"])
                assert np.array_equal(g["A"], g["A"].T)
                if first and variant in (7, 8):
                    off = (cls == scenes.VALID) != vg
                    assert not off[~amb].any(), (variant, name, int(off[~amb].sum()), np.argwhere(off & ~amb)[:5])
                    assert amb.sum() <= max(1, int(1e-4 * o["n"])), (name, int(amb.sum()))
                    occluded = (cls == scenes.OCCLUDED) & ~amb
                    if name == "true":
                        assert occluded.sum() >= (2000 >> (2 * level)), int(occluded.sum())
                    assert not vg[occluded].any()
            P_prev = o["P"]
    print("level %d: variant 8 worst per-entry error P %.2e A %.2e" % (level, worst["P"], worst["A"]))
    # option ref_compat: the reciprocal of the host CPU in projection and weights, the exact sweep against MATH + Q1
    ctx.set_option("ref_compat", 1)
    ctx.set_option("variant", 7)
    rcam = camera(ctx, p, levels)
    cref, ccur = rcam.create_raw(p["grey_ref"], p["depth_ref"]), rcam.create_raw(p["grey_cur"], p["depth_cur"])
    P = np.array([900.0, 3.0, 3.0, 400.0], np.float32)
    for name, T34 in warps(p):
        for first in (True, False):
            o = po.level_iteration(oref, ocur, level, T34, P_prev=None if first else P, first=first, mode=Q1, want_residuals=True)
            g = trk.level_iteration(cref, ccur, level, T34, P_prev=None if first else P, first=first, want_residuals=True)
            assert g["n"] == o["n"] and np.array_equal(g["residuals"], o["residuals"], equal_nan=True), ("ref_compat", name, first)
            assert np.abs(g["A"] - o["A"]).max() <= 2e-5 * np.abs(o["A"]).max()


# ---- 3. whole matches ------------------------------------------------------------------------------------------------------------
MATCH_CFG = dict(FirstLevel=3, LastLevel=0, Precision=1e-4, MaxIterationsPerLevel=100)
TRUTH_TOL = 1e-2       # the estimator's own accuracy on these scenes (a far plane observes translation weakly): the oracle's worst is 5.2e-3


def assert_match_equals_oracle(g, p, oref, ocur, cfg, what):
    o = po.match(oref, ocur, cm.oracle_config_from(cfg, po.MATH))
    s = cm.compare_runs(g, o)
    print(what, s)
    assert s["n_mismatch"] == 0 and s["max_x_err"] < 2e-5, (what, s)
    assert s["max_iter_count_diff"] <= 2, (what, s)
    assert s["T_err"] < 2e-5, (what, s)
    if s["structure_mismatch"] == 0:
        assert np.abs(g["information"] - o["information"]).max() <= 2e-3 * np.abs(o["information"]).max()
        assert abs(g["loglik"] - o["loglik"]) <= 1e-3 * abs(o["loglik"])
    k = cm.keyframe_statistics_from(g)
    assert g["entropy"] == pytest.approx(k["entropy"], rel=1e-12)
    assert g["constraint_ratio"] == k["constraint_ratio"] and g["constraint_ratio_accepted"] == k["constraint_ratio_accepted"]
    # the quirk-faithful REF_SSE mode: on these scenes the quirks move the result by up to 5e-3 (the oracle's own MATH-vs-REF_SSE
    # distance, not 5e-5 as on synth_pair); the GPU is no farther from it than the oracle's MATH mode is, up to their own distance
    q = po.match(oref, ocur, cm.oracle_config_from(cfg, po.REF_SSE))
    assert cm.twist_matrix_error(g["T"], q["T"]) <= cm.twist_matrix_error(o["T"], q["T"]) + 2e-5, what
    assert np.abs(po.se3_log(g["T"]) - p["xi_true"]).max() < TRUTH_TOL
    if po.ref_lib() is not None and p["grey_ref"].shape[1] % (4 << cfg.FirstLevel) == 0:
        r = po.ref_match(p["grey_ref"].astype(np.float32), po.convert_raw_depth(p["depth_ref"]), p["grey_cur"].astype(np.float32),
                         po.convert_raw_depth(p["depth_cur"]), p["K"], cm.oracle_config_from(cfg, po.REF_SSE))
        assert np.array_equal(r["T"], q["T"])
        assert cm.twist_matrix_error(g["T"], r["T"]) <= cm.twist_matrix_error(o["T"], r["T"]) + 2e-5, what


def test_whole_match_on_the_default_policy():
    """One 640 x 480 pair, levels 3 -> 0, the library's default policy (the resident kernel takes the pair): the assertions of
    test_full_match_against_oracle.  f16_range_repeats is recorded: if the depth edges leave the f16 Gram's range, the repeated
    record must equal variant 6's bit for bit."""
    p = scene(SEED, 640, 480)
    oref, ocur = oracle_pyramids(SEED, 640, 480, 4)
    cfg = d.Config(**MATCH_CFG)
    recs = {}
    for variant in (None, 6):
        ctx = d.Context(0)
        ctx.set_option("condition_number", 1)
        if variant is not None:
            ctx.set_option("variant", variant)
        cam = camera(ctx, p, 4)
        gref, gcur = cam.create_raw(p["grey_ref"], p["depth_ref"]), cam.create_raw(p["grey_cur"], p["depth_cur"])
        r = d.Result()
        assert d.DenseTracker(cfg, ctx).match(gref, gcur, r) is True
        recs[variant] = (cm.tracker_result_to_dict(r), ctx.counter("f16_range_repeats"), ctx.counter("resident_launches"))
    g, repeats, resident = recs[None]
    print("default policy: f16_range_repeats %d, resident_launches %d" % (repeats, resident))
    assert resident >= 1
    assert_match_equals_oracle(g, p, oref, ocur, cfg, "default policy")
    if repeats:
        for k in ("T", "information", "loglik"):
            assert np.array_equal(g[k], recs[6][0][k], equal_nan=True), k


def test_batch_of_edge_scenes_on_the_launch_path():
    """Eight distinct 320 x 240 edge scenes in one batch with resident 0 (the launch path), each against the oracle.  On the exact
    schedule (variant 7): with the default one the larger edge residuals (EPS_UV) tip a termination test of pair 100 another way and
    its later levels start from another estimate (final transforms 6e-6 apart), so iteration records cannot be compared one to one."""
    w, h, n = 320, 240, 8
    ctx = d.Context(0)
    ctx.set_option("resident", 0)
    ctx.set_option("variant", 7)
    ctx.set_option("condition_number", 1)
    cfg = d.Config(**MATCH_CFG)
    pairs = [scene(100 + i, w, h) for i in range(n)]
    cam = camera(ctx, pairs[0], 4)
    refs = [cam.create_raw(q["grey_ref"], q["depth_ref"]) for q in pairs]
    curs = [cam.create_raw(q["grey_cur"], q["depth_cur"]) for q in pairs]
    res = [d.Result() for _ in range(n)]
    d.DenseTracker(cfg, ctx).match_batch(refs, curs, res, with_stats=True)
    print("launch path: f16_range_repeats %d" % ctx.counter("f16_range_repeats"))
    for i, (q, r) in enumerate(zip(pairs, res)):
        oref, ocur = oracle_pyramids(100 + i, w, h, 4)
        assert_match_equals_oracle(cm.tracker_result_to_dict(r), q, oref, ocur, cfg, "pair %d" % i)
