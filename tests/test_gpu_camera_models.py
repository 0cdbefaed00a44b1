"""GPU tier (-m gpu): every sweep schedule against the CPU oracle's MATH mode under the cameras of tests/cameras.py.

Every other alignment test hands the kernels the fr1 intrinsics: fx = fy to 0.15 %, the principal point near the centre, a mid-range
field of view.  Camera-dependent code is all over the hot path (get_camera's halving and tx / ty tables, make_geom's wi_x / wi_y /
half_fx / half_fy, make_KT and the level hand-over, the depth-gradient rows fx Zx, fy Zy in three spellings, the f16 hi + lo Gram
operands, the data-driven window), and fx for fy or ox for oy in one of them shows only under another camera.  Here, for fr1 (control),
aniso, wide, tele and outside:
  (a) planes, selection masks and the level K of every level, bit-exact;
  (b) one linearisation on the exact schedules (variants 0, 5, 6, 7; rows_per_wave 0 and 4): counts and residuals bit-exact, sums to
      1e-5 / 1e-6 -- the bounds of test_single_linearisation_against_oracle; variants 5 and 6 the same bits in A, b and -ll;
  (c) one linearisation on the default schedule (variant 8) at the sizes that take the fast window sweep, its half-empty last tile
      column and the contracted gathering sweep -- the bounds of test_default_schedule_single_linearisation_against_oracle;
  (d) the window sweeps under motions that spread a tile's taps beyond the staged window (counter window_fallbacks);
  (e) whole matches at Precision 1e-4 on the launch path (a batch of four) and on the resident path, against po.match(MATH).  Not
      stated, for the reasons given there: the default schedule's launch path from the identity, and any bound to REF_SSE;
  (f) two cameras of one size alive on one context (get_camera's cache), and the refusal of a K that is no camera.
Every comparison is kernel against the CPU oracle; the GPU-to-GPU statements ((b) 5 = 6, (e) launch = resident, (f)) come on top.

The default schedule's residual bound under these cameras.  |dr_I| <= 2e-5 is 3 ulp of the tap coordinate's operands times the
intensity step between neighbouring pixels / 255, stated for 640-wide levels under fr1.  It carries over:
  * the sizes here are at most 256 wide: an ulp of the pixel coordinate is a quarter of the ulp at 640;
  * the tap coordinate is u = fx X / Z + ox: its operands are at most |ox| + max |u - ox| <= 2.1 x the pixel coordinate's range
    (outside, in y: oy = 1.05 h; 1.2 in x; 1.0 for a centred principal point);
  * the steepest intensity step per pixel is about 2.3 x fr1's (wide: the same metric texture under less than half the focal length);
  so the worst case is 2.1 x 2.3 / 4 = 1.2 of the bound's own case, with the measured values (below) under it.  A constraint may flip
  only where scenes.classify calls the pixel ambiguous at its own eps_uv, 2.5e-7 (w + h), at most max(1, 1e-4 n) of them.

No whole match at Precision 5e-7 below 640 x 480: tests/test_camera_models.py says why.  The one at 640 x 480 (aniso) is a case of
tests/test_gpu_parity.py::test_full_match_against_oracle.

Measured on an MI355X (worst over sizes and both passes, per camera):
  default schedule, one linearisation (c), against MATH      fr1      aniso    wide     tele     outside   bound
    flipped constraints                                       0        0        0        0        0         max(1, 1e-4 n)
    |dr_I|                                                    6.9e-6   1.7e-5   1.1e-5   4.0e-6   8.2e-6    2e-5
    |dr_Z| [m]                                                1.7e-6   1.9e-6   1.4e-6   1.7e-6   1.7e-6    4e-6
    P / A / b, of the largest entry                           4.0e-6   3.8e-6   1.5e-6   1.4e-6   1.4e-6    1e-5
    -ll, relative                                             7.9e-7   5.3e-7   3.4e-7   3.2e-7   3.1e-7    2e-5
  (the largest |dr_I| is aniso at 192 x 80, fy = 250: the bound holds with a factor 1.2 to spare, not more.)
  exact schedules (b): counts and residuals bit-exact under every camera, size and schedule; variants 5 and 6 the same bits.
  window under parallax (d): window_fallbacks on variants 5 / 6 / 7 / 8: wide 0 / 672 / 672 / 526, tele 0 / 666 / 666 / 1202; variant 8
    against 7: no flipped constraint, |dr_I| 7.5e-6 / 3.0e-6, |dr_Z| 8.3e-7 / 1.1e-6, b 1.7e-6.
  whole matches (e), twist distance to po.match(MATH), worst over the pairs: resident path 9.3e-8 (increments 2.6e-7; the same under
    variants 7 and 8); launch path on variant 7 1.5e-7 (increments 5.7e-7), on variant 8 with an initial estimate 7.9e-8 (2.5e-7);
    launch against resident path under one schedule 1.2e-7;
    to REF_SSE (printed, no bound stated) 1.1e-5 ... 6.4e-5, equal to the oracle's own MATH-to-REF_SSE distance to two digits.
"""
import functools

import numpy as np
import pytest

import cameras
import common as cm
import dvo_slam_amd as d
import scenes
from dvo_slam_amd import datagen
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
NAMES = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")
XI = np.array([0.004, -0.003, 0.002, 0.005, -0.004, 0.003])
SEED = 23
EXACT_SCHEDULES = ((0, 0), (4, 0), (0, 5), (4, 5), (0, 6), (0, 7))      # (rows_per_wave, variant)


def camera_K(name, w, h):
    return cameras.CAMERAS(w, h)[name]


@functools.lru_cache(maxsize=None)
def oracle_case(name, w, h, levels, seed=SEED):
    pair = cm.synth(seed, w, h, camera_K(name, w, h))
    return (pair,) + tuple(cm.oracle_pyramids(pair, levels))


@functools.lru_cache(maxsize=None)
def oracle_passes(name, w, h, level, xi=tuple(XI), seed=SEED):
    """(first pass, second pass with the first one's P) of the oracle's MATH mode, with residuals; shared by the schedules"""
    _, oref, ocur = oracle_case(name, w, h, level + 1, seed)
    T34 = po.se3_exp(np.array(xi, np.float64))[:3]
    o = po.level_iteration(oref, ocur, level, T34, first=True, mode=po.MATH, want_residuals=True)
    o2 = po.level_iteration(oref, ocur, level, T34, P_prev=o["P"], first=False, mode=po.MATH, want_residuals=True)
    return T34, o, o2


def gpu_frames(ctx, pair, levels):
    h, w = pair["grey_ref"].shape
    cam = d.RgbdCameraPyramid(w, h, pair["K"], ctx)
    cam.build(levels)
    return cam.create_raw(pair["grey_ref"], pair["depth_ref"]), cam.create_raw(pair["grey_cur"], pair["depth_cur"])


def context(**options):
    ctx = d.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def gpu_passes(ctx, pair, level, T34, P):
    gref, gcur = gpu_frames(ctx, pair, level + 1)
    trk = d.DenseTracker(d.Config(FirstLevel=level, LastLevel=level), ctx)
    return (trk.level_iteration(gref, gcur, level, T34, first=True, want_residuals=True),
            trk.level_iteration(gref, gcur, level, T34, P_prev=P, first=False, want_residuals=True))


def rel(g, o, k):
    return float(np.abs(g[k] - o[k]).max() / np.abs(o[k]).max())


def assert_exact(g, o, what):
    """the statement of test_single_linearisation_against_oracle for one pass"""
    assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"], (what, g["n"], o["n"])
    assert np.array_equal(g["residuals"], o["residuals"], equal_nan=True), what
    for k in ("P", "A", "b"):
        assert rel(g, o, k) <= 1e-5, (what, k, rel(g, o, k))
    assert abs(g["neg_ll"] - o["neg_ll"]) <= 1e-6 * abs(o["neg_ll"]), what
    assert np.array_equal(g["A"], g["A"].T), what


def assert_same_bits(a, b, what):
    assert np.array_equal(a["A"], b["A"]) and np.array_equal(a["b"], b["b"]) and a["neg_ll"] == b["neg_ll"], what


def assert_contracted(g, o, classify, what):
    """the statement of test_default_schedule_single_linearisation_against_oracle for one pass of the contracted schedule `g` against
    `o` (the oracle, or a schedule whose residuals are the oracle's bits); classify() -> the ambiguity mask of scenes.classify.
    Returns the measured figures."""
    ro, rg = o["residuals"].reshape(-1, 2), g["residuals"].reshape(-1, 2)
    vo, vg = ~np.isnan(ro[:, 0]), ~np.isnan(rg[:, 0])
    flipped = vo != vg
    nf = int(flipped.sum())
    both = vo & vg
    m = dict(n=o["n"], flipped=nf, dI=float(np.abs(ro[both, 0] - rg[both, 0]).max()), dZ=float(np.abs(ro[both, 1] - rg[both, 1]).max()),
             P=rel(g, o, "P"), A=rel(g, o, "A"), b=rel(g, o, "b"), ll=abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"]))
    print("%s: n %d vs %d, %d flipped, |dr_I| %.2e |dr_Z| %.2e, P %.1e A %.1e b %.1e -ll %.1e"
          % (what, g["n"], o["n"], nf, m["dI"], m["dZ"], m["P"], m["A"], m["b"], m["ll"]))
    assert g["n_selected"] == o["n_selected"] and g["n"] == int(vg.sum()), what
    assert nf <= max(1, int(1e-4 * o["n"])), (what, nf)
    if nf:
        amb = classify().reshape(-1)
        assert amb[flipped].all(), (what, "a flipped constraint that sits on no bound", np.flatnonzero(flipped & ~amb)[:5])
    assert m["dI"] <= 2e-5 and m["dZ"] <= 4e-6, (what, m)
    slack = 20.0 * nf / o["n"]
    assert m["P"] <= 1e-5 + slack and m["A"] <= 1e-5 + slack and m["b"] <= 1e-5 + slack and m["ll"] <= 2e-5 + slack, (what, m)
    assert np.array_equal(g["A"], g["A"].T), what
    return m


def classifier(name, w, h, level, T34, seed=SEED):
    """-> a function giving scenes.classify's ambiguity mask for this linearisation (computed only when a constraint flipped)"""
    def run():
        _, oref, ocur = oracle_case(name, w, h, level + 1, seed)
        _, mask = oref.select(level)
        Zr, K = oref.plane(level, 1)
        cur = [ocur.plane(level, k)[0] for k in range(6)]
        T = np.vstack([np.asarray(T34, np.float32).astype(np.float64), [0, 0, 0, 1]])
        return scenes.classify(Zr, mask, cur, K, T)[1]
    return run


WORST = {}


def record_worst(name, m):
    w = WORST.setdefault(name, dict(flipped=0, dI=0.0, dZ=0.0, P=0.0, A=0.0, b=0.0, ll=0.0))
    for k in w:
        w[k] = max(w[k], m[k])
    print("worst so far, %s: %d flipped, |dr_I| %.2e |dr_Z| %.2e, P %.1e A %.1e b %.1e -ll %.1e"
          % (name, w["flipped"], w["dI"], w["dZ"], w["P"], w["A"], w["b"], w["ll"]))


# ---- (a) planes, selection, level K ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", [(130, 34, 2), (160, 120, 3)])
@pytest.mark.parametrize("name", cameras.NAMES)
def test_planes_selection_and_level_K_bit_exact(gpu_ctx, name, w, h, levels):
    """test_pyramid_planes_bit_exact's body under another K; on the shared context, which by now has seen other cameras of this size.
    img.K against the oracle's pins get_camera's float32 halving (tests/test_camera_models.py: the oracle's is K halved l times)."""
    pair, oref, ocur = oracle_case(name, w, h, levels, 17)
    for view, opyr in (("ref", oref), ("cur", ocur)):
        cam = d.RgbdCameraPyramid(w, h, pair["K"], gpu_ctx)
        cam.build(levels)
        frame = cam.create_raw(pair["grey_" + view], pair["depth_" + view])
        for l in range(levels):
            img = frame.level(l)
            for k, plane in enumerate(NAMES):
                o, K = opyr.plane(l, k)
                g = np.asarray(getattr(img, plane))
                assert g.shape == o.shape and np.array_equal(g, o, equal_nan=True), (view, l, plane)
            assert np.array_equal(img.K, K) and np.array_equal(img.K, cameras.level_K(pair["K"], l)), (view, l, img.K, K)
            for thr in ((0.0, 0.0), (5.0, 0.02)):
                n, mask = d.PointSelection(frame, *thr).select(l, want_mask=True)
                on, omask = opyr.select(l, *thr)
                assert n == on and np.array_equal(mask, omask), (view, l, thr, n, on)


# ---- (b) the exact schedules -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,level", [(128, 96, 0), (131, 97, 0), (258, 194, 1), (80, 60, 0)])
@pytest.mark.parametrize("name", cameras.NAMES)
def test_exact_schedules_single_linearisation_against_oracle(name, w, h, level):
    pair, _, _ = oracle_case(name, w, h, level + 1)
    T34, o, o2 = oracle_passes(name, w, h, level)
    assert o["n"] >= 500 and o["n"] >= 0.2 * o["n_selected"]
    out = {}
    for rows, variant in EXACT_SCHEDULES:
        ctx = context(variant=variant, rows_per_wave=rows)
        g, g2 = out[rows, variant] = gpu_passes(ctx, pair, level, T34, o["P"])
        assert_exact(g, o, (name, rows, variant, "first"))
        assert_exact(g2, o2, (name, rows, variant, "second"))
    # variant 6 = the gathering sweep bit for bit (test_window_sweep_against_the_gathering_sweep): a level the window sweep takes runs
    # at its tile height, four rows per wavefront; any other level runs the gathering sweep itself
    lw = w >> level
    same = (4, 5) if lw % 64 == 0 else (0, 5)
    for k in (0, 1):
        assert_same_bits(out[same][k], out[0, 6][k], (name, "5 = 6", k))


# ---- (c) the default schedule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(128, 96), (192, 80), (160, 120), (80, 60), (131, 97)])
@pytest.mark.parametrize("name", cameras.NAMES)
def test_default_schedule_single_linearisation_against_oracle_per_camera(name, w, h):
    """Variant 8 against MATH directly.  128 x 96 and 192 x 80: the fast window sweep; 160 x 120: the same with a half-empty last
    tile column; 80 x 60 and 131 x 97: the contracted gathering sweep."""
    pair, _, _ = oracle_case(name, w, h, 1)
    T34, o, o2 = oracle_passes(name, w, h, 0)
    assert o["n"] >= 500 and o["n"] >= 0.2 * o["n_selected"]
    ctx = context(variant=8, rows_per_wave=0)
    g, g2 = gpu_passes(ctx, pair, 0, T34, o["P"])
    cls = classifier(name, w, h, 0, T34)
    for gp, op, what in ((g, o, "first"), (g2, o2, "second")):
        record_worst(name, assert_contracted(gp, op, cls, "%s %dx%d %s" % (name, w, h, what)))
    assert ctx.counter("f16_range_repeats") == 0


# ---- (d) the window under parallax ---------------------------------------------------------------------------------------------------
# The motions are the warp reference -> current the linearisation takes, a base twist times a scale.  The window follows the bounding
# box of a tile's taps, so a motion leaves it only where it spreads the 64 x 16 tile's projection beyond 80 x 30 cells:
#   wide  [0.02, 0.01, 0.25, 0, 0, 0] x -2: half a metre BACKWARDS, a tile's projection grows by up to a third (forwards it shrinks,
#         whatever the distance, and every point lands behind the surface the current frame sees: the occlusion test then leaves 3.7 %
#         of the selected pixels); 29 % of the selected pixels are constraints;
#   tele  [0, 0, 0, 0.02, -0.03, 0.15] x 2: 0.3 rad about the optical axis turns a tile's 16 rows into more than 30 (0.15 rad: 25, inside
#         the window); 20.3 % are constraints.
# Both were found with the oracle and a float64 model of the window on the CPU; the test asserts the 20 % and window_fallbacks > 0.
PARALLAX = [("wide", 192, 80, -2.0, [0.02, 0.01, 0.25, 0, 0, 0]), ("tele", 192, 80, 2.0, [0, 0, 0, 0.02, -0.03, 0.15])]


@pytest.mark.parametrize("name,w,h,scale,xi", PARALLAX)
def test_window_sweeps_under_parallax(name, w, h, scale, xi):
    xi = tuple(scale * x for x in xi)
    pair, _, _ = oracle_case(name, w, h, 1, 31)
    T34, o, o2 = oracle_passes(name, w, h, 0, xi, 31)
    print("%s %dx%d xi %s: %d constraints of %d selected" % (name, w, h, xi, o["n"], o["n_selected"]))
    assert o["n"] >= 0.2 * o["n_selected"] and o["n"] >= 500
    out, fallbacks = {}, {}
    for v in (5, 6, 7, 8):
        ctx = context(variant=v, rows_per_wave=4)
        out[v] = gpu_passes(ctx, pair, 0, T34, o["P"])
        fallbacks[v] = ctx.counter("window_fallbacks")
    print("%s: window_fallbacks %s" % (name, fallbacks))
    cls = classifier(name, w, h, 0, T34, 31)
    for k, op in ((0, o), (1, o2)):
        assert_exact(out[5][k], op, (name, 5, k))                 # the anchor is the oracle's
        for v in (6, 7):
            assert_exact(out[v][k], out[5][k], (name, v, k))
        assert_same_bits(out[5][k], out[6][k], (name, "5 = 6", k))
        assert_contracted(out[8][k], out[7][k], cls, "%s parallax, 8 against 7, pass %d" % (name, k))
    assert fallbacks[5] == 0 and fallbacks[6] > 0 and fallbacks[7] == fallbacks[6]


# ---- (e) whole matches -------------------------------------------------------------------------------------------------------------
# What is NOT stated here, and why (measured on an MI355X, all five cameras, fr1 included):
#   * the DEFAULT schedule on the LAUNCH path for a match that starts at the identity.  Its first linearisation is
#     test_contracted_sweep_at_the_identity's case: every reference pixel projects onto a pixel centre, the contracted tap coordinate
#     lands on either side of floor()'s step, and next to holes the constraint set differs from MATH's by a per cent (first pass of
#     level 2: n 1326 against 1346 under fr1, 1374 against 1355 under tele; increments up to 7.9e-4 / 2.7e-3 apart where n_mismatch == 0
#     and 2e-5 are asked).  The later passes pull the estimate back -- final transforms 4.5e-8 ... 1.1e-5 from MATH's on 17 of the 18
#     pairs measured -- but at Precision 1e-4 a level may also stop a pass apart: outside, seed 105, ends 9.97e-5 from MATH.  None of the
#     bounds asked of a whole match holds there without being widened, under fr1 no more than under the others, so NO test here runs a
#     whole match on the default schedule's launch path from the identity.  Record by record the launch path is held to the oracle on
#     the exact schedule (variant 7: the same launches, level hand-over and solver steps, the sweep's arithmetic apart) under every
#     camera, and on the default schedule only where the match starts from an initial estimate (aniso, Mu 0.05).  The resident path,
#     which the default policy gives a single pair, meets the whole statement from the identity.  The default schedule's sweeps
#     themselves are held to MATH under every camera in (c) and (d).
#   * any bound to REF_SSE.  REF_SSE reproduces the reference's rcpps, whose table is the host CPU's, and at Precision 1e-4 it stops a
#     pass apart from MATH on some pairs: the oracle's own MATH-to-REF_SSE distance under these cameras is 5.6e-5 ... 6.4e-5 for all four
#     wide pairs on one host and 2e-5 on another, where seeds 83 and 101 under outside give 9.5e-5 and 9.7e-5.  No engine can be within
#     2e-5 of the one and 5e-5 of the other there, and where the two modes are close the 2e-5 to MATH already implies the 5e-5.  Both
#     distances are printed; the bound to REF_SSE at the stopping precision is test_full_match_against_oracle's.
MATCH_W, MATCH_H, MATCH_PAIRS = 320, 240, 4
# (name, first seed, Mu, UseInitialEstimate)
MATCHES = [("fr1", 40, 0.0, False), ("aniso", 50, 0.0, False), ("wide", 60, 0.0, False), ("tele", 70, 0.0, False),
           ("outside", 80, 0.0, False), ("aniso", 90, 0.05, True)]


def match_config(mu, init):
    return d.Config(FirstLevel=2, LastLevel=0, Mu=mu, UseInitialEstimate=init, Precision=1e-4, MaxIterationsPerLevel=50 if init else 100)


@functools.lru_cache(maxsize=None)
def oracle_matches(name, seed0, mu, init):
    b = datagen.synth_batch(seed0, MATCH_PAIRS, MATCH_W, MATCH_H, camera_K(name, MATCH_W, MATCH_H))
    cfg = match_config(mu, init)
    runs = []
    for i in range(MATCH_PAIRS):
        pair = dict(grey_ref=b["grey_ref"][i], depth_ref=b["depth_ref"][i], grey_cur=b["grey_cur"][i], depth_cur=b["depth_cur"][i], K=b["K"])
        oref, ocur = cm.oracle_pyramids(pair, 3)
        T0 = po.se3_exp(0.5 * b["xi_true"][i]) if init else None
        runs.append((pair, T0, po.match(oref, ocur, cm.oracle_config_from(cfg, po.MATH), T0),
                     po.match(oref, ocur, cm.oracle_config_from(cfg, po.REF_SSE), T0)["T"]))
    return runs


def assert_match(g, o, T_sse, what):
    s = cm.compare_runs(g, o)
    print(what, s, "to REF_SSE %.2e (the oracle's MATH mode: %.2e)" % (cm.twist_matrix_error(g["T"], T_sse), cm.twist_matrix_error(o["T"], T_sse)))
    assert s["n_mismatch"] == 0 and s["max_x_err"] < 2e-5, (what, s)
    assert s["max_iter_count_diff"] <= 1, (what, s)
    assert s["T_err"] < 2e-5, (what, s)


def run_launch_path(runs, cfg, variant):
    ctx = context(resident=0, variant=variant)
    frames = [gpu_frames(ctx, pair, 3) for pair, _, _, _ in runs]
    res = [d.Result() for _ in runs]
    for r, (_, T0, _, _) in zip(res, runs):
        if cfg.UseInitialEstimate:
            r.Transformation = np.array(T0)
    d.DenseTracker(cfg, ctx).match_batch([f[0] for f in frames], [f[1] for f in frames], res, with_stats=True)
    assert ctx.counter("resident_launches") == 0 and ctx.counter("f16_range_repeats") == 0
    return res


def run_resident_path(run, cfg, variant):
    pair, T0, _, _ = run
    ctx = context(variant=variant)
    gref, gcur = gpu_frames(ctx, pair, 3)
    r = d.Result()
    if cfg.UseInitialEstimate:
        r.Transformation = np.array(T0)
    d.DenseTracker(cfg, ctx).match(gref, gcur, r)
    assert ctx.counter("resident_launches") >= 1 and ctx.counter("f16_range_repeats") == 0
    return r


@pytest.mark.parametrize("name,seed0,mu,init", MATCHES)
def test_whole_matches_on_both_paths(name, seed0, mu, init):
    """320 x 240, levels 2 -> 0, Precision 1e-4: the first pair alone on the resident path (the default policy) and a batch of four
    pairs of one camera on the launch path (resident 0), each against po.match(MATH); the two paths against each other under the same
    schedule.  The default schedule (variant 8) on the resident path always, on the launch path where the match does not start at the
    identity; the exact schedule (variant 7) on both (see above)."""
    runs = oracle_matches(name, seed0, mu, init)
    cfg = match_config(mu, init)
    _, _, o0, T_sse0 = runs[0]
    for variant in (8, 7):
        resident = run_resident_path(runs[0], cfg, variant)
        assert_match(cm.tracker_result_to_dict(resident), o0, T_sse0, "%s resident path, variant %d" % (name, variant))
        if variant == 8 and not init:
            continue
        res = run_launch_path(runs, cfg, variant)
        for i, (r, (_, _, o, T_sse)) in enumerate(zip(res, runs)):
            assert_match(cm.tracker_result_to_dict(r), o, T_sse, "%s launch path, variant %d, pair %d" % (name, variant, i))
        both = cm.twist_matrix_error(resident.Transformation, res[0].Transformation)
        print("%s: launch path against resident path, variant %d: %.2e" % (name, variant, both))
        assert both < 1e-6


# ---- (f) two cameras of one size on one context; K that is no camera ---------------------------------------------------------------
def record_bytes(r):
    """everything a match returns, as bytes"""
    parts = [np.asarray(r.Transformation, np.float64).tobytes(), np.asarray(r.Information, np.float64).tobytes(),
             np.float64(r.LogLikelihood).tobytes()]
    for L in r.Statistics.Levels:
        parts.append(np.array([L.Id, L.MaxValidPixels, L.ValidPixels, L.TerminationCriterion, len(L.Iterations)], np.int64).tobytes())
        for s in L.Iterations:
            parts += [np.int64(s.ValidConstraints).tobytes(), np.float64(s.TDistributionLogLikelihood).tobytes(),
                      np.asarray(s.TDistributionPrecision, np.float64).tobytes(), np.asarray(s.EstimateIncrement, np.float64).tobytes(),
                      np.asarray(s.EstimateInformation, np.float64).tobytes()]
    return b"".join(parts)


@pytest.mark.parametrize("resident", [0, -1])
def test_two_cameras_of_one_size_on_one_context(resident):
    """get_camera keeps one geometry per (size, K bytes) and context: fr1 and aniso frames of 160 x 120 alive together, matched in turn
    (A, B, A, B) through one DenseTracker, give the records -- every byte -- that each pair gives on a context that has only ever seen
    its own camera; a batch mixing the cameras is refused and leaves the context as it was."""
    w, h = 160, 120
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    pairs = {name: [cm.synth(60 + i, w, h, camera_K(name, w, h)) for i in range(2)] for name in ("fr1", "aniso")}

    def run(ctx, trk, frames):
        r = d.Result()
        trk.match(frames[0], frames[1], r)
        return record_bytes(r)

    alone = {}
    for name in pairs:
        ctx = context(table_cache=1, resident=resident)
        trk = d.DenseTracker(cfg, ctx)
        frames = [gpu_frames(ctx, p, 3) for p in pairs[name]]
        alone[name] = [run(ctx, trk, f) for f in frames]
    assert alone["fr1"][0] != alone["aniso"][0]
    ctx = context(table_cache=1, resident=resident)
    trk = d.DenseTracker(cfg, ctx)
    # frames of both cameras are created before the first match, and alternately
    frames = {(name, i): gpu_frames(ctx, pairs[name][i], 3) for i in range(2) for name in ("fr1", "aniso")}
    for i in range(2):
        for name in ("fr1", "aniso"):
            assert run(ctx, trk, frames[name, i]) == alone[name][i], (name, i)
    a, b = frames["fr1", 0], frames["aniso", 0]
    with pytest.raises(d.DvoHipError):
        trk.match_batch([a[0], b[0]], [a[1], b[1]], [d.Result(), d.Result()])
    with pytest.raises(d.DvoHipError):
        trk.match(a[0], b[1], d.Result())
    for name in ("aniso", "fr1"):                               # refused calls leave the context as it was
        assert run(ctx, trk, frames[name, 1]) == alone[name][1], (name, "after the refusals")


@pytest.mark.parametrize("bad", [(np.nan, 100.0, 80.0, 60.0), (100.0, np.nan, 80.0, 60.0), (100.0, 100.0, np.inf, 60.0),
                                 (100.0, 100.0, 80.0, -np.inf), (100.0, 100.0, 80.0, np.nan), (0.0, 100.0, 80.0, 60.0),
                                 (100.0, 0.0, 80.0, 60.0), (-100.0, 100.0, 80.0, 60.0), (100.0, -0.0, 80.0, 60.0), (np.inf, 100.0, 80.0, 60.0)])
def test_a_K_that_is_no_camera_is_refused(bad):
    """dvo_hip_frame_create_*: a K that is not finite, or fx <= 0 or fy <= 0, is DVO_HIP_ERR_INVALID -- it would go into the tx / ty
    tables and into the camera cache's key.  The refused call leaves the context usable: a camera of the same size then gives the
    oracle's planes and linearisation."""
    w, h = 160, 120
    pair, oref, ocur = oracle_case("aniso", w, h, 1)
    ctx = context(variant=7)
    cam = d.RgbdCameraPyramid(w, h, np.array(bad, np.float32), ctx)
    with pytest.raises(d.DvoHipError):
        cam.create_raw(pair["grey_ref"], pair["depth_ref"])
    with pytest.raises(d.DvoHipError):
        cam.create(pair["grey_ref"].astype(np.float32), po.convert_raw_depth(pair["depth_ref"]))
    T34, o, o2 = oracle_passes("aniso", w, h, 0)
    g, g2 = gpu_passes(ctx, pair, 0, T34, o["P"])
    assert_exact(g, o, "after a refusal, first")
    assert_exact(g2, o2, "after a refusal, second")
