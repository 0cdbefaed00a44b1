"""GPU tier (-m gpu): the HIP path, called through the C-ABI of libdvo_hip.so, against the CPU oracle's MATH mode
on identical seeded inputs, against the committed golden fixtures, and -- at the BASELINE sizes -- through
size-independent properties.

Tolerances (float32 pixel arithmetic, float64 pose arithmetic), all relative to the oracle's MATH mode:
  image planes, selection masks                                   bit-exact
  valid-pixel counts, residuals                                   bit-exact on schedules 0, 5, 6, 7 (option "variant"); the default
                                                                  schedule 8 (contracted arithmetic): residuals within 2e-5 (3 ulp of
                                                                  the tap coordinate times the image gradient), counts equal except
                                                                  at pixels on a bound -- test_contracted_sweep_against_the_exact_one
  precision P, -ll, A, b of one linearisation                    1e-5 relative (tree reduction vs float64 sums)
  increments x along a full match                                2e-5 absolute
  final transform (twist of T_gpu^-1 T_oracle)                   1e-6 at Precision 5e-7, 2e-5 at Precision 1e-4
  vs the quirk-faithful REF_SSE mode                             5e-5 (the oracle's own MATH-vs-REF_SSE delta)
"""
import numpy as np
import pytest

import cameras
import common as cm
import dvo_slam_amd as d
from dvo_slam_amd import datagen
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
DEFAULT_VARIANT = 8     # the library's default sweep schedule (dvo_hip.h, option "variant"): window sweep, contracted arithmetic
EXACT_VARIANT = 7       # the window sweep whose residuals and constraint counts equal the oracle's MATH mode bit for bit: the anchor


def gpu_pyramids(ctx, pair, levels):
    h, w = pair["grey_ref"].shape
    cam = d.RgbdCameraPyramid(w, h, pair["K"], ctx)
    cam.build(levels)
    return cam.create_raw(pair["grey_ref"], pair["depth_ref"]), cam.create_raw(pair["grey_cur"], pair["depth_cur"])


def test_library_loaded_and_device_present(gpu_ctx):
    assert d.lib().dvo_hip_device_count() >= 1
    assert gpu_ctx.ptr


@pytest.mark.parametrize("w,h,levels", [(640, 480, 4), (160, 120, 3), (100, 76, 2),
                                        # the strip ingest (even rows of 4-pixel groups): ragged last strip, heights that are no multiple of
                                        # the 8-row strip or of the 32-row group, odd coarser levels; a one-strip image
                                        (140, 62, 3), (388, 122, 4), (128, 8, 2), (132, 34, 4),
                                        # the tile kernels: level 1 of 65 x 17 (odd width: k_derive_levels over one level, two tile columns and
                                        # rows, the second of each one pixel); the tile ingest and the float-plane derive at an odd level 0
                                        (130, 34, 2), (65, 17, 1)])
def test_pyramid_planes_bit_exact(gpu_ctx, w, h, levels):
    pair = cm.synth(17, w, h)
    oref, _ = cm.oracle_pyramids(pair, levels)
    gref, _ = gpu_pyramids(gpu_ctx, pair, levels)
    names = ["intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy"]
    for l in range(levels):
        img = gref.level(l)
        for k, name in enumerate(names):
            o, K = oref.plane(l, k)
            g = getattr(img, name)
            assert g.shape == o.shape
            assert np.array_equal(np.isnan(g), np.isnan(o)), (l, name)
            assert np.array_equal(np.nan_to_num(g), np.nan_to_num(o)), (l, name)
        assert np.array_equal(img.K, K)
        sel = d.PointSelection(gref)
        n, mask = sel.select(l, want_mask=True)
        on, omask = oref.select(l)
        assert n == on and np.array_equal(mask, omask)
    # f32 ingest path gives the same planes as the raw path
    cam = d.RgbdCameraPyramid(w, h, pair["K"], gpu_ctx)
    cam.build(levels)
    g2 = cam.create(pair["grey_ref"].astype(np.float32), po.convert_raw_depth(pair["depth_ref"]))
    a, b = g2.level(levels - 1).depth_dx, gref.level(levels - 1).depth_dx
    assert np.array_equal(np.nan_to_num(a), np.nan_to_num(b))
    # thresholds
    sel = d.PointSelection(gref, 5.0, 0.02)
    assert sel.select(0) == oref.select(0, 5.0, 0.02)[0]


@pytest.mark.parametrize("w,h,level", [(640, 480, 0), (640, 480, 1), (640, 480, 3), (160, 120, 0), (100, 76, 1),
                                       # odd and tiny sizes, widths around the 64-pixel tile, a tall image: ragged tiles / segments
                                       (131, 97, 0), (131, 97, 2), (65, 49, 0), (63, 130, 0), (258, 194, 1), (36, 20, 0), (1281, 13, 0)])
def test_single_linearisation_against_oracle(gpu_ctx, w, h, level):
    pair = cm.synth(23, w, h)
    levels = level + 1
    oref, ocur = cm.oracle_pyramids(pair, levels)
    gref, gcur = gpu_pyramids(gpu_ctx, pair, levels)
    trk = d.DenseTracker(d.Config(FirstLevel=level, LastLevel=level), gpu_ctx)
    T34 = po.se3_exp(np.array([0.004, -0.003, 0.002, 0.005, -0.004, 0.003]))[:3]
    # every tile height / schedule: same answer
    for rows, variant in ((0, 0), (1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (0, 5), (1, 5), (2, 5), (4, 5), (8, 5), (16, 5), (0, 6), (0, 7)):
        gpu_ctx.set_option("rows_per_wave", rows)
        gpu_ctx.set_option("variant", variant)
        o = po.level_iteration(oref, ocur, level, T34, first=True, mode=po.MATH, want_residuals=True)
        g = trk.level_iteration(gref, gcur, level, T34, first=True, want_residuals=True)
        assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"]
        assert np.array_equal(np.isnan(g["residuals"]), np.isnan(o["residuals"]))
        assert np.array_equal(np.nan_to_num(g["residuals"]), np.nan_to_num(o["residuals"]))
        # sums accumulated in another order: relative to the matrix, not to a small off-diagonal element that is a cancellation
        assert np.abs(g["P"] - o["P"]).max() <= 1e-5 * np.abs(o["P"]).max()
        assert abs(g["neg_ll"] - o["neg_ll"]) <= 1e-6 * abs(o["neg_ll"])
        assert np.abs(g["A"] - o["A"]).max() <= 1e-5 * np.abs(o["A"]).max()
        assert np.abs(g["b"] - o["b"]).max() <= 1e-5 * np.abs(o["b"]).max()
        assert np.array_equal(g["A"], g["A"].T)
        o2 = po.level_iteration(oref, ocur, level, T34, P_prev=o["P"], first=False, mode=po.MATH)
        g2 = trk.level_iteration(gref, gcur, level, T34, P_prev=o["P"], first=False)
        assert g2["n"] == o2["n"]
        assert np.abs(g2["P"] - o2["P"]).max() <= 1e-5 * np.abs(o2["P"]).max()
        assert abs(g2["neg_ll"] - o2["neg_ll"]) <= 1e-6 * abs(o2["neg_ll"])
        assert np.abs(g2["A"] - o2["A"]).max() <= 1e-5 * np.abs(o2["A"]).max()
        assert np.abs(g2["b"] - o2["b"]).max() <= 1e-5 * np.abs(o2["b"]).max()
    gpu_ctx.set_option("rows_per_wave", 0)
    gpu_ctx.set_option("variant", DEFAULT_VARIANT)


@pytest.mark.parametrize("w,h,level", [(640, 480, 0), (640, 480, 1), (640, 480, 2), (640, 480, 3), (160, 120, 0), (1280, 960, 0),
                                       # ragged: a tile column of two lanes and a tile row of two rows; an odd width (gathering sweep
                                       # with the contracted arithmetic); a level narrower than the window sweep takes
                                       (258, 194, 0), (131, 97, 0), (200, 64, 0), (80, 60, 0)])
def test_default_schedule_single_linearisation_against_oracle(gpu_ctx, w, h, level):
    """The schedule that SHIPS (variant 8: contracted arithmetic, v_rcp_f32 projection, f16 hi + lo Gram, packed residual pairs) against
    the oracle's MATH mode DIRECTLY -- not through the exact schedule (test_contracted_sweep_against_the_exact_one) -- for one
    linearisation (dense_tracking.cpp:271-343: residual pass, weights, scale, log-likelihood, normal equations), first pass (unit
    weights) and a second pass (t-distribution weights of the first pass' precision).  Stated and asserted:
      * constraints: the same set except at pixels whose tap coordinate sits on a bound (<= 1e-4 of them, at least 1 allowed);
      * residuals of common constraints: |dr_I| <= 2e-5, |dr_Z| <= 4e-6 m;
      * P, A, b: 1e-5 relative to the largest entry (+ what the flipped constraints can carry: each at most 20 / n of the sums) on EVERY
        level (round 6: the default keeps every operand's f16 low part; the high-part-only Jacobians of round 5 are option gram_lo_parts 0,
        whose b bound of 3e-5 is asserted in test_contracted_sweep_against_the_exact_one);
      * -ll: 2e-5 relative."""
    pair = cm.synth(23, w, h)
    levels = level + 1
    oref, ocur = cm.oracle_pyramids(pair, levels)
    gref, gcur = gpu_pyramids(gpu_ctx, pair, levels)
    trk = d.DenseTracker(d.Config(FirstLevel=level, LastLevel=level), gpu_ctx)
    gpu_ctx.set_option("rows_per_wave", 0)
    gpu_ctx.set_option("variant", DEFAULT_VARIANT)
    T34 = po.se3_exp(np.array([0.004, -0.003, 0.002, 0.005, -0.004, 0.003]))[:3]
    P_prev = None
    for first in (True, False):
        o = po.level_iteration(oref, ocur, level, T34, P_prev=P_prev, first=first, mode=po.MATH, want_residuals=True)
        g = trk.level_iteration(gref, gcur, level, T34, P_prev=P_prev, first=first, want_residuals=True)
        ro, rg = o["residuals"].reshape(-1, 2), g["residuals"].reshape(-1, 2)
        vo, vg = ~np.isnan(ro[:, 0]), ~np.isnan(rg[:, 0])
        flipped = int((vo != vg).sum())
        both = vo & vg
        d0 = float(np.abs(ro[both, 0] - rg[both, 0]).max())
        d1 = float(np.abs(ro[both, 1] - rg[both, 1]).max())
        relP = np.abs(g["P"] - o["P"]).max() / np.abs(o["P"]).max()
        relA = np.abs(g["A"] - o["A"]).max() / np.abs(o["A"]).max()
        relb = np.abs(g["b"] - o["b"]).max() / np.abs(o["b"]).max()
        rell = abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"])
        print("%dx%d level %d first=%d: n %d vs oracle %d, %d flipped, |dr_I| %.2e |dr_Z| %.2e, P %.1e A %.1e b %.1e -ll %.1e"
              % (w, h, level, first, g["n"], o["n"], flipped, d0, d1, relP, relA, relb, rell))
        assert g["n_selected"] == o["n_selected"] and g["n"] == int(vg.sum()) and o["n"] >= 500
        assert flipped <= max(1, int(1e-4 * o["n"]))
        assert d0 <= 2e-5 and d1 <= 4e-6
        slack = 20.0 * flipped / o["n"]
        assert relP <= 1e-5 + slack and relA <= 1e-5 + slack and relb <= 1e-5 + slack and rell <= 2e-5 + slack
        assert np.array_equal(g["A"], g["A"].T)
        P_prev = o["P"]


def test_default_schedule_finest_level_records_against_the_reference(gpu_ctx):
    """BASELINE config 2 (one 640 x 480 pair, levels 3 -> 0) on the default schedule: EVERY iteration record of the finest level
    against the records of the reference's own DenseTracker::match() (oracle/_ref: dvo_core's translation units compiled in place)
    on the same frames.  The two run different arithmetic by design (the reference: _mm_rcp_ps, round-toward-zero, odd-N drop, LL
    tail), and the level starts from coarser-level results that already differ by that distance, so the bounds
    are the quirk distance, stated per quantity: constraints within 0.1 % (measured 6e-5), increments within 5e-5 over the common
    passes (measured 7e-6), at most 2 passes more or fewer, final transforms within 5e-5 (measured 3.0e-5).  The precision matrix is
    printed, not bounded: the reference's comes out of computeScaleSse's lane pairing (dense_tracking_impl.cpp:608-615),
    which mixes the two residual channels -- it differs from the covariance's inverse by a factor (4.4 x the largest entry here), a
    quirk the engine does not reproduce."""
    if po.ref_lib() is None:
        pytest.skip("oracle/_ref is not built (no /root/reference here and no prebuilt library)")
    pair = cm.synth(1234, 640, 480)
    gref, gcur = gpu_pyramids(gpu_ctx, pair, 4)
    cfg = d.Config(FirstLevel=3, LastLevel=0, MaxIterationsPerLevel=100, Precision=5e-7)
    gpu_ctx.set_option("variant", DEFAULT_VARIANT)
    g = run_gpu_match(gpu_ctx, gref, gcur, cfg)
    r = po.ref_match(pair["grey_ref"].astype(np.float32), po.convert_raw_depth(pair["depth_ref"]),
                     pair["grey_cur"].astype(np.float32), po.convert_raw_depth(pair["depth_cur"]), pair["K"],
                     cm.oracle_config_from(cfg, po.REF_SSE))
    Lg, Lr = g["levels"][-1], r["levels"][-1]
    assert Lg["id"] == 0 and Lr["id"] == 0 and Lg["valid_pixels"] == Lr["valid_pixels"]
    ig, ir = Lg["iterations"], Lr["iterations"]
    print("finest level: %d passes on the engine, %d in the reference; terminations %d / %d" % (len(ig), len(ir), Lg["termination"], Lr["termination"]))
    assert abs(len(ig) - len(ir)) <= 2
    worst = dict(n=0.0, P=0.0, x=0.0)
    for a, b in zip(ig, ir):
        worst["n"] = max(worst["n"], abs(a["n"] - b["n"]) / b["n"])
        worst["P"] = max(worst["P"], np.abs(a["precision"] - b["precision"]).max() / np.abs(b["precision"]).max())
        if np.all(np.isfinite(a["x"])) and np.all(np.isfinite(b["x"])):
            worst["x"] = max(worst["x"], float(np.abs(a["x"] - b["x"]).max()))
    sum_g = sum(i["x"] for i in ig if np.all(np.isfinite(i["x"])))
    sum_r = sum(i["x"] for i in ir if np.all(np.isfinite(i["x"])))
    print("worst over the common passes: n %.2e, P %.2e, x %.2e; summed increments differ by %.2e; final twist distance %.2e"
          % (worst["n"], worst["P"], worst["x"], np.abs(sum_g - sum_r).max(), cm.twist_matrix_error(g["T"], r["T"])))
    assert worst["n"] <= 1e-3 and worst["x"] <= 5e-5
    assert cm.twist_matrix_error(g["T"], r["T"]) < 5e-5


@pytest.mark.parametrize("w,h,xi", [(640, 480, [0.004, -0.003, 0.002, 0.006, -0.004, 0.003]), (320, 240, [0.02, 0.01, -0.015, -0.02, 0.025, 0.03]),
                                    (640, 480, [0.05, -0.04, 0.03, 0.05, 0.04, -0.06]), (128, 96, [0, 0, 0, 0, 0, 0]), (64, 48, [0.01, 0, 0, 0, 0.01, 0]),
                                    (640, 480, [0.3, -0.2, 0.1, 0.2, 0.3, -0.4]), (192, 80, [-0.05, 0.08, 0.02, 0.1, -0.1, 0.2])])
def test_window_sweep_against_the_gathering_sweep(w, h, xi):
    """The sweep that stages the current frame's {I, Z} window in LDS and derives the gradient channels itself (align_window.hip,
    variants 6 / 7; the default on levels whose width is a multiple of 64) against the gathering sweep (variant 5) at the same tile
    height.  Variant 6 (f32 Gram) is the gathering sweep BIT FOR BIT: residuals, valid count, every entry of A and b -- which pins
    the staged window, the derived gradients (= the stored planes), the short division (= the IEEE division) and, for the large
    motions, the lanes whose taps fall outside the window and are fetched from memory (counter window_fallbacks).  Variant 7
    accumulates the Gram matrix on the f16 matrix pipe with an exact hi / lo split: residuals and counts identical, sums to 1e-6."""
    pair = cm.synth(31, w, h)
    T34 = po.se3_exp(np.array(xi, np.float64))[:3]
    out = {}
    for v in (5, 6, 7):
        ctx = d.Context(0)
        ctx.set_option("variant", v)
        ctx.set_option("rows_per_wave", 4)
        gref, gcur = gpu_pyramids(ctx, pair, 1)
        trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
        out[v] = [trk.level_iteration(gref, gcur, 0, T34, P_prev=[900.0, 3.0, 3.0, 400.0], first=f, want_residuals=True) for f in (True, False)]
        out[v].append(ctx.counter("window_fallbacks"))
    assert out[5][2] == 0
    if max(abs(x) for x in xi) > 0.15:
        assert out[6][2] > 0 and out[7][2] == out[6][2]              # the motion is large enough to leave the 80 x 30 window
    for k in (0, 1):
        a = out[5][k]
        for v in (6, 7):
            b = out[v][k]
            assert a["n"] == b["n"] and a["n_selected"] == b["n_selected"]
            assert np.array_equal(a["residuals"], b["residuals"], equal_nan=True)
        assert np.array_equal(a["A"], out[6][k]["A"]) and np.array_equal(a["b"], out[6][k]["b"]) and a["neg_ll"] == out[6][k]["neg_ll"]
        assert np.abs(a["A"] - out[7][k]["A"]).max() <= 1e-6 * np.abs(a["A"]).max()
        assert np.abs(a["b"] - out[7][k]["b"]).max() <= 1e-6 * np.abs(a["b"]).max() + 1e-9 * np.abs(a["A"]).max()
        assert abs(a["neg_ll"] - out[7][k]["neg_ll"]) <= 1e-5 * abs(a["neg_ll"])      # (through the inverse of the 2 x 2 scale matrix)


@pytest.mark.parametrize("w,h,xi", [(640, 480, [0.004, -0.003, 0.002, 0.006, -0.004, 0.003]), (320, 240, [0.02, 0.01, -0.015, -0.02, 0.025, 0.03]),
                                    (640, 480, [0.05, -0.04, 0.03, 0.05, 0.04, -0.06]), (128, 96, [0.003, 0.001, -0.002, 0.004, 0.002, -0.003]),
                                    (640, 480, [0.3, -0.2, 0.1, 0.2, 0.3, -0.4]), (192, 80, [-0.05, 0.08, 0.02, 0.1, -0.1, 0.2]),
                                    (1280, 960, [0.01, -0.01, 0.005, 0.01, 0.01, -0.01]), (640, 250, [0.01, 0.02, -0.01, -0.01, 0.02, 0.01])])
def test_contracted_sweep_against_the_exact_one(w, h, xi):
    """The default schedule (variant 8, align_fast.hip; 9 = the same with the matrix operands stored through lane swaps) against the window sweep
    whose residuals are the oracle's bit for bit (variant 7).  Same function, other rounding: the tap coordinate u = qx rcp(qz) carries
    up to ~3 ulp(u) where the exact schedule's quotient is correctly rounded (of inputs that themselves carry 2 ulp), the blends are
    contracted.  Stated and checked here, per pixel:
      * a pixel is a constraint in both or in neither, except where the tap coordinate sits on a bound: within 4 ulp of 0, w - 2 or
        h - 2 (Q4), of a pixel boundary with a hole behind it (another twelve-cell neighbourhood, Q9), or on the occlusion threshold
        (Q5) -- at most 1e-4 of the constraints, none at all in six of the eight cases;
      * residuals of common constraints: |dr_I| <= 3 ulp(640) x the intensity step between neighbouring pixels / 255 <= 2e-5 here
        (measured 1.5e-5), |dr_Z| <= 4e-6 m (measured 1.7e-6);
      * normal equations and log-likelihood: 1e-5 / 2e-5 relative (5e-6 / 3e-6 measured).
    Large motions leave the 84 x 28 window: the lanes concerned fetch their cells from memory (counter window_fallbacks)."""
    pair = cm.synth(31, w, h)
    T34 = po.se3_exp(np.array(xi, np.float64))[:3]
    out = {}
    # (8 here: with option gram_lo_parts 0, round 5's default -- on levels of 150 000 pixels and more the Jacobian components enter the matrix
    # pipe as f16 high parts; "8 lo" keeps every low part like variant 9 does: what ships since round 6)
    for v in (EXACT_VARIANT, 8, 9, "8 lo"):
        ctx = d.Context(0)
        ctx.set_option("variant", 8 if v == "8 lo" else v)
        ctx.set_option("gram_lo_parts", 1 if v == "8 lo" else 0)
        ctx.set_option("rows_per_wave", 4)
        gref, gcur = gpu_pyramids(ctx, pair, 1)
        trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
        out[v] = [trk.level_iteration(gref, gcur, 0, T34, P_prev=[900.0, 3.0, 3.0, 400.0], first=f, want_residuals=True) for f in (True, False)]
        out[v].append(ctx.counter("window_fallbacks"))
    if max(abs(x) for x in xi) > 0.15:
        assert out[8][2] > 0 and out[9][2] == out[8][2]
    else:
        assert out[8][2] == 0
    for k in (0, 1):
        a = out[EXACT_VARIANT][k]
        for v in (8, 9):
            b = out[v][k]
            ra, rb = a["residuals"].reshape(-1, 2), b["residuals"].reshape(-1, 2)
            assert np.array_equal(np.isnan(rb[:, 0]), np.isnan(rb[:, 1]))                  # NaN pairs on the boundary
            va, vb = ~np.isnan(ra[:, 0]), ~np.isnan(rb[:, 0])
            flipped = int((va != vb).sum())
            both = va & vb
            d0 = float(np.abs(ra[both, 0] - rb[both, 0]).max()) if both.any() else 0.0
            d1 = float(np.abs(ra[both, 1] - rb[both, 1]).max()) if both.any() else 0.0
            print("%dx%d variant %d first=%d: n %d vs %d, %d pixels flipped, max |dr_I| %.2e |dr_Z| %.2e, A rel %.1e, b rel %.1e"
                  % (w, h, v, 1 - k, a["n"], b["n"], flipped, d0, d1, np.abs(a["A"] - b["A"]).max() / np.abs(a["A"]).max(),
                     np.abs(a["b"] - b["b"]).max() / np.abs(a["b"]).max()))
            assert a["n_selected"] == b["n_selected"] and b["n"] == int(vb.sum())
            assert flipped <= max(1, int(1e-4 * a["n"]))
            assert d0 <= 2e-5 and d1 <= 4e-6
            if flipped == 0:
                # (b is a sum of cancelling terms: where the Jacobian enters the matrix pipe as f16 high parts -- variant 8 on a level of
                # 150 000 pixels and more -- its bound is 3e-5 of its largest entry: measured 1.1e-5 with 27 000 constraints, 4e-6 with 190 000)
                hi_j = v == 8 and w * h >= 150000
                assert np.abs(a["A"] - b["A"]).max() <= 1e-5 * np.abs(a["A"]).max()
                assert np.abs(a["b"] - b["b"]).max() <= (3e-5 if hi_j else 1e-5) * np.abs(a["b"]).max() + 1e-9 * np.abs(a["A"]).max()
                assert abs(a["neg_ll"] - b["neg_ll"]) <= 2e-5 * abs(a["neg_ll"])
        # the two operand-store schemes of the contracted sweep feed the same numbers to the matrix pipe
        assert np.array_equal(out[8][k]["residuals"], out[9][k]["residuals"], equal_nan=True) and out[8][k]["n"] == out[9][k]["n"]
        assert np.abs(out["8 lo"][k]["A"] - out[9][k]["A"]).max() <= 1e-6 * np.abs(out[9][k]["A"]).max()
        # ... and the Jacobian's high parts alone, where the level is large enough for it, stay inside the schedule's bound
        assert np.array_equal(out[8][k]["residuals"], out["8 lo"][k]["residuals"], equal_nan=True)
        assert np.abs(out[8][k]["A"] - out["8 lo"][k]["A"]).max() <= (6e-6 if w * h >= 150000 else 0.0) * np.abs(out[9][k]["A"]).max()
        assert np.abs(out[8][k]["b"] - out["8 lo"][k]["b"]).max() <= (3e-5 if w * h >= 150000 else 0.0) * np.abs(out[9][k]["b"]).max() + 1e-9 * np.abs(out[9][k]["A"]).max()


@pytest.mark.parametrize("w,h,rpw,xi", [(160, 120, 2, [0.01, -0.008, 0.006, 0.012, -0.01, 0.008]), (80, 60, 2, [0.02, 0.01, -0.015, -0.02, 0.025, 0.03]),
                                        (160, 120, 4, [0.05, -0.04, 0.03, 0.05, 0.04, -0.06]), (100, 76, 1, [0.01, 0.02, -0.01, -0.01, 0.02, 0.01]),
                                        (40, 30, 2, [0.003, 0.001, -0.002, 0.004, 0.002, -0.003]), (200, 64, 16, [-0.05, 0.08, 0.02, 0.1, -0.1, 0.2])])
def test_contracted_gathering_sweep_against_the_exact_one(w, h, rpw, xi):
    """The levels the window sweep does not take (narrower than 84 pixels or not a multiple of 64 wide: levels 2 and 3 of a 640 x 480
    pyramid) run the gathering sweep; under the default schedule with the contracted per-pixel arithmetic too (align_mfma.hip, MODE 2).
    Same statement as test_contracted_sweep_against_the_exact_one, against the same anchor (variant 7: residuals the oracle's bit for
    bit)."""
    pair = cm.synth(37, w, h)
    T34 = po.se3_exp(np.array(xi, np.float64))[:3]
    out = {}
    for v in (EXACT_VARIANT, 8):
        ctx = d.Context(0)
        ctx.set_option("variant", v)
        ctx.set_option("rows_per_wave", rpw)
        gref, gcur = gpu_pyramids(ctx, pair, 1)
        trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
        out[v] = [trk.level_iteration(gref, gcur, 0, T34, P_prev=[900.0, 3.0, 3.0, 400.0], first=f, want_residuals=True) for f in (True, False)]
    for k in (0, 1):
        a, b = out[EXACT_VARIANT][k], out[8][k]
        ra, rb = a["residuals"].reshape(-1, 2), b["residuals"].reshape(-1, 2)
        va, vb = ~np.isnan(ra[:, 0]), ~np.isnan(rb[:, 0])
        flipped = int((va != vb).sum())
        both = va & vb
        d0 = float(np.abs(ra[both, 0] - rb[both, 0]).max())
        d1 = float(np.abs(ra[both, 1] - rb[both, 1]).max())
        print("%dx%d rows per wave %d first=%d: n %d vs %d, %d pixels flipped, max |dr_I| %.2e |dr_Z| %.2e, A rel %.1e, b rel %.1e"
              % (w, h, rpw, 1 - k, a["n"], b["n"], flipped, d0, d1, np.abs(a["A"] - b["A"]).max() / np.abs(a["A"]).max(),
                 np.abs(a["b"] - b["b"]).max() / np.abs(a["b"]).max()))
        assert a["n_selected"] == b["n_selected"] and b["n"] == int(vb.sum()) and a["n"] > 0.2 * w * h
        assert flipped <= max(1, int(1e-4 * a["n"]))
        assert d0 <= 2e-5 and d1 <= 4e-6
        if flipped == 0:
            assert np.abs(a["A"] - b["A"]).max() <= 1e-5 * np.abs(a["A"]).max()
            assert np.abs(a["b"] - b["b"]).max() <= 1e-5 * np.abs(a["b"]).max() + 1e-9 * np.abs(a["A"]).max()
            assert abs(a["neg_ll"] - b["neg_ll"]) <= 2e-5 * abs(a["neg_ll"])


@pytest.mark.parametrize("w,h", [(640, 480), (160, 120), (320, 250), (200, 64)])
def test_packed_residuals_give_the_same_sums(w, h):
    """The contracted window sweep stores the residual pairs of constraints only, packed per wavefront slot (LevelGeom::compact), for
    the log-likelihood pass to read half the bytes.  Against the same sweep storing one pair per pixel (option compact_residuals 0):
    the normal equations are the same bits (their path does not change), the log-likelihood the same sum in another order (float64
    products: 1e-7 relative on the float it is returned as)."""
    pair = cm.synth(53, w, h)
    T34 = po.se3_exp(np.array([0.01, -0.008, 0.006, 0.012, -0.01, 0.008], np.float64))[:3]
    out = {}
    for packed in (1, 0):
        ctx = d.Context(0)
        ctx.set_option("compact_residuals", packed)
        gref, gcur = gpu_pyramids(ctx, pair, 1)
        trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
        out[packed] = [trk.level_iteration(gref, gcur, 0, T34, P_prev=[900.0, 3.0, 3.0, 400.0], first=f) for f in (True, False)]
    for k in (0, 1):
        a, b = out[1][k], out[0][k]
        assert a["n"] == b["n"] and a["n"] > 0.2 * w * h
        assert np.array_equal(a["A"], b["A"]) and np.array_equal(a["b"], b["b"]) and np.array_equal(a["P"], b["P"])
        assert abs(a["neg_ll"] - b["neg_ll"]) <= 1e-7 * abs(b["neg_ll"]), (a["neg_ll"], b["neg_ll"])


def test_packed_residuals_whole_matches():
    """... and whole matches of a batch on the launch path (every pair its own stride in the residual buffer; levels 0-2 packed, level 3
    by pixel): the same iteration counts, transforms within 1e-9."""
    n = 24
    b = datagen.synth_batch(3, n, 640, 480)
    rec = {}
    for packed in (1, 0):
        ctx = d.Context(0)
        ctx.set_option("compact_residuals", packed)
        ctx.set_option("resident", 0)
        cam = d.RgbdCameraPyramid(640, 480, b["K"], ctx)
        cam.build(4)
        refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
        curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
        rec[packed] = d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx).match_batch_arrays(refs, curs)
    assert np.array_equal(rec[1]["n_iterations"], rec[0]["n_iterations"])
    assert np.abs(rec[1]["T"] - rec[0]["T"]).max() <= 1e-9
    assert np.allclose(rec[1]["loglik"], rec[0]["loglik"], rtol=1e-7)


def test_solver_step_in_two_wavefront_workgroups_gives_the_same_records():
    """A large batch runs the solver step of its small levels in two-wavefront workgroups (four per compute unit instead of two); each
    wavefront plays two of the four (the same additions and products in the same order): every record the same bits, with the packed
    and with the by-pixel residual layout, statistics included."""
    n = 12
    b = datagen.synth_batch(5, n, 640, 480)
    for packed in (1, 0):
        rec = {}
        for waves in (4, 2):
            ctx = d.Context(0)
            ctx.set_option("solver_waves", waves)
            ctx.set_option("compact_residuals", packed)
            ctx.set_option("resident", 0)
            cam = d.RgbdCameraPyramid(640, 480, b["K"], ctx)
            cam.build(4)
            refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
            curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
            res = [d.Result() for _ in range(n)]
            d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx).match_batch(refs, curs, res, with_stats=True)
            rec[waves] = res
        for ra, rb in zip(rec[4], rec[2]):
            assert np.array_equal(ra.Transformation, rb.Transformation) and np.array_equal(ra.Information, rb.Information)
            assert ra.LogLikelihood == rb.LogLikelihood
            for La, Lb in zip(ra.Statistics.Levels, rb.Statistics.Levels):
                assert len(La.Iterations) == len(Lb.Iterations)
                for Ia, Ib in zip(La.Iterations, Lb.Iterations):
                    assert Ia.ValidConstraints == Ib.ValidConstraints and Ia.TDistributionLogLikelihood == Ib.TDistributionLogLikelihood
                    assert np.array_equal(Ia.EstimateIncrement, Ib.EstimateIncrement, equal_nan=True)


def test_contracted_sweep_random_sizes():
    """Twenty random level sizes for the default schedule as the match runs it -- packed residual pairs, tile grids that hang over the
    right and the lower edge by any amount (widths 84 ... 330 incl. 64 k + 2: a tile column of two lanes; heights 30 ... 250) -- against
    the exact schedule: the constraint count (a pixel on a bound may flip: at most 1e-4 of them), and where the counts agree the
    normal equations to 1e-5 and the log-likelihood to 2e-5."""
    rng = np.random.default_rng(77)
    sizes = [(130, 33), (194, 47), (86, 30), (320, 17)] + [(int(rng.integers(42, 166)) * 2, int(rng.integers(30, 251))) for _ in range(16)]
    worst = [0.0, 0.0, 0]
    for k, (w, h) in enumerate(sizes):
        pair = cm.synth(100 + k, w, h)
        T34 = po.se3_exp(rng.normal(0.0, 0.01, 6))[:3]
        out = {}
        for v in (EXACT_VARIANT, DEFAULT_VARIANT):
            ctx = d.Context(0)
            ctx.set_option("variant", v)
            gref, gcur = gpu_pyramids(ctx, pair, 1)
            trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
            out[v] = [trk.level_iteration(gref, gcur, 0, T34, P_prev=[900.0, 3.0, 3.0, 400.0], first=f) for f in (True, False)]
        for a, b in zip(out[EXACT_VARIANT], out[DEFAULT_VARIANT]):
            assert a["n_selected"] == b["n_selected"], (w, h)
            assert abs(a["n"] - b["n"]) <= max(1, int(1e-4 * a["n"])), (w, h, a["n"], b["n"])
            worst[2] = max(worst[2], abs(a["n"] - b["n"]))
            if a["n"] == b["n"] and a["n"] >= 6:
                ea = np.abs(a["A"] - b["A"]).max() / np.abs(a["A"]).max()
                el = abs(a["neg_ll"] - b["neg_ll"]) / abs(a["neg_ll"])
                worst[0], worst[1] = max(worst[0], ea), max(worst[1], el)
                assert ea <= 1e-5 and el <= 2e-5, (w, h, ea, el)
    print("20 random sizes: largest |dA| / |A| %.1e, |d ll| / |ll| %.1e, count difference %d" % tuple(worst))


def test_contracted_sweep_at_the_identity():
    """Identical frames, identity transform: every reference pixel projects EXACTLY onto a pixel centre of the current frame -- the
    discontinuity of floor().  Whichever side of it a rounding lands on, the blend is continuous (weight 0 or 1 on the same pixel),
    but the twelve-cell neighbourhood the validity test looks at (Q9) shifts by one pixel: next to holes the two schedules disagree
    about a per cent of the constraints, like the reference's own rcpps path disagrees with exact arithmetic there.  Residuals of the
    common constraints still agree, and both are zero to rounding."""
    w, h = 128, 96
    pair = cm.synth(14, w, h)
    out = {}
    for v in (EXACT_VARIANT, 8):
        ctx = d.Context(0)
        ctx.set_option("variant", v)
        ctx.set_option("rows_per_wave", 4)
        gref, _ = gpu_pyramids(ctx, pair, 1)
        trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
        out[v] = trk.level_iteration(gref, gref, 0, np.eye(4)[:3], first=True, want_residuals=True)
    ra, rb = out[EXACT_VARIANT]["residuals"].reshape(-1, 2), out[8]["residuals"].reshape(-1, 2)
    va, vb = ~np.isnan(ra[:, 0]), ~np.isnan(rb[:, 0])
    print("identity: n %d vs %d, %d flipped" % (out[EXACT_VARIANT]["n"], out[8]["n"], int((va != vb).sum())))
    assert (va != vb).sum() <= 0.05 * va.sum()
    both = va & vb
    assert np.abs(rb[both]).max() <= 1e-5 and np.abs(ra[both]).max() <= 1e-5


def test_f16_gram_does_not_lengthen_the_levels():
    """The f16 high / low Gram (default schedule) carries a little more rounding noise than the f32 one; a noise floor of the normal
    equations close to the stopping precision would show as levels that miss "increment too small" and run on until the log-likelihood
    stops improving.  Over 96 pairs at BASELINE precision (5e-7), every level on the launch path: the same mean iteration counts per
    level as the f32 schedule (within 0.25), no level more than three passes longer."""
    n = 96
    b = datagen.synth_batch(0, n, 640, 480)
    its = {}
    for v in (5, 7, 8):
        ctx = d.Context(0)
        ctx.set_option("variant", v)
        ctx.set_option("resident", 0)
        cam = d.RgbdCameraPyramid(640, 480, b["K"], ctx)
        cam.build(4)
        refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
        curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
        results = [d.Result() for _ in range(n)]
        d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx).match_batch(refs, curs, results, with_stats=True)
        its[v] = np.array([[len(L.Iterations) for L in r.Statistics.Levels] for r in results])
        del refs, curs, cam, ctx
    print("mean iterations per level (3..0): f32 Gram %s, f16 Gram %s; longest levels %s / %s" % (its[5].mean(0), its[7].mean(0), its[5].max(0), its[7].max(0)))
    assert np.abs(its[7].mean(0) - its[5].mean(0)).max() <= 0.25
    assert (its[7].max(0) <= its[5].max(0) + 3).all()
    print("contracted arithmetic (the default schedule): %s, longest levels %s" % (its[8].mean(0), its[8].max(0)))
    assert np.abs(its[8].mean(0) - its[5].mean(0)).max() <= 0.25
    assert (its[8].max(0) <= its[5].max(0) + 3).all()


@pytest.mark.parametrize("w,h", [(128, 96), (160, 120)])
def test_f16_gram_range_guard_repeats_with_the_f32_gram(w, h):
    """The default schedule forms its Gram operands as f16 high + low parts: a Jacobian component beyond +-65504 (a depth step of
    ten metres one centimetre in front of the camera: fx * 5 m/px / 0.01 m) is not representable.  The sweep notices (the diagonal of
    H H^T reaches 65504^2), the batch runs again with the f32 Gram: same record as the f32 schedule, the counter shows the repeat.
    An ordinary scene on the same context does not repeat.  (160 x 120: the contracted window sweep takes the level, the f32 schedule
    of the repeat is the gathering sweep -- another flavour of the current frame's planes, derived for the repeat.)"""
    pair = cm.synth(4, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 0.002, 10.0).astype(np.float32)
    grey = pair["grey_ref"].astype(np.float32)
    recs = {}
    for v in (6, 7, 8):
        ctx = d.Context(0)
        ctx.set_option("variant", v)
        ctx.set_option("resident", 0)
        cam = d.RgbdCameraPyramid(w, h, pair["K"], ctx)
        cam.build(1)
        trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0, MaxIterationsPerLevel=3), ctx)
        ref, cur = cam.create(grey, depth), cam.create(grey, depth)
        out = trk.match_batch_arrays([ref], [cur])
        recs[v] = (out, ctx.counter("f16_range_repeats"))
        if v >= 7:
            # the batches right after a repeat take the f32 Gram from the start (a sequence that keeps meeting such a depth step does
            # not pay twice per frame): the same scene again does not count another repeat, nor does an ordinary one
            again = trk.match_batch_arrays([ref], [cur])
            assert ctx.counter("f16_range_repeats") == recs[v][1]
            for k in ("T", "information", "loglik", "n_iterations"):
                assert np.array_equal(again[k], out[k], equal_nan=True), k
            gref, gcur = gpu_pyramids(ctx, pair, 1)
            trk.match_batch_arrays([gref], [gcur])
            assert ctx.counter("f16_range_repeats") == recs[v][1]
    assert recs[6][1] == 0 and recs[7][1] == 1 and recs[8][1] == 1
    for v in (7, 8):                                            # the repeat runs variant 6: its record, bit for bit
        for k in ("T", "information", "loglik", "n_iterations"):
            assert np.array_equal(recs[6][0][k], recs[v][0][k], equal_nan=True), (v, k)
    # many moderately large components do not trip the guard: only a component that really left the f16 range does
    ctx = d.Context(0)
    ctx.set_option("resident", 0)
    cam = d.RgbdCameraPyramid(w, h, pair["K"], ctx)
    cam.build(1)
    depth2 = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 0.35, 0.40).astype(np.float32)      # steps of 5 cm at 0.4 m: components of ~1e3 everywhere
    a, b = cam.create(grey, depth2), cam.create(grey, depth2)
    d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0, MaxIterationsPerLevel=3), ctx).match_batch_arrays([a], [b])
    assert ctx.counter("f16_range_repeats") == 0


def test_f16_gram_range_guard_repeats_only_the_pairs_concerned():
    """Round 5: the guard is per PAIR.  A batch of eight pairs, one of which carries a depth step that leaves the f16 range: only that
    pair runs again (f32 Gram, a batch of its own) -- the counter moves by one, its record is the f32 schedule's record of that pair bit
    for bit, the seven others keep the records they have in a batch without it, and the batch that follows starts on the f16 schedule
    again (no hold: most of the batch was in range).  Statistics travel with the replaced record."""
    w, h, n, bad = 128, 96, 8, 5
    b = datagen.synth_batch(11, n, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    step = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 0.002, 10.0).astype(np.float32)
    cfg = d.Config(FirstLevel=0, LastLevel=0, MaxIterationsPerLevel=3)

    def frames(ctx, with_bad):
        cam = d.RgbdCameraPyramid(w, h, b["K"], ctx)
        cam.build(1)
        refs, curs = [], []
        for i in range(n):
            g_r, g_c = b["grey_ref"][i].astype(np.float32), b["grey_cur"][i].astype(np.float32)
            z_r, z_c = po.convert_raw_depth(b["depth_ref"][i]), po.convert_raw_depth(b["depth_cur"][i])
            if with_bad and i == bad:
                g_c, z_r, z_c = g_r, step, step
            refs.append(cam.create(g_r, z_r))
            curs.append(cam.create(g_c, z_c))
        return refs, curs

    ctx = d.Context(0)
    ctx.set_option("resident", 0)
    refs, curs = frames(ctx, True)
    res = [d.Result() for _ in range(n)]
    trk = d.DenseTracker(cfg, ctx)
    trk.match_batch(refs, curs, res, with_stats=True)
    assert ctx.counter("f16_range_repeats") == 1
    trk.match_batch(refs[:bad], curs[:bad], [d.Result() for _ in range(bad)])          # an ordinary batch next: f16 again, no repeat
    assert ctx.counter("f16_range_repeats") == 1
    # the pair concerned, alone, on the f32 schedule
    c6 = d.Context(0)
    c6.set_option("resident", 0)
    c6.set_option("variant", 6)
    r6, k6 = frames(c6, True)
    one = d.Result()
    d.DenseTracker(cfg, c6).match(r6[bad], k6[bad], one)
    assert np.array_equal(res[bad].Transformation, one.Transformation) and np.array_equal(res[bad].Information, one.Information, equal_nan=True)
    assert [len(L.Iterations) for L in res[bad].Statistics.Levels] == [len(L.Iterations) for L in one.Statistics.Levels]
    for Ia, Ib in zip(res[bad].Statistics.Levels[0].Iterations, one.Statistics.Levels[0].Iterations):
        assert Ia.ValidConstraints == Ib.ValidConstraints and np.array_equal(Ia.EstimateIncrement, Ib.EstimateIncrement, equal_nan=True)
    # the others: what they are in a batch without the pair
    c8 = d.Context(0)
    c8.set_option("resident", 0)
    r8, k8 = frames(c8, False)
    clean = [d.Result() for _ in range(n)]
    d.DenseTracker(cfg, c8).match_batch(r8, k8, clean, with_stats=True)
    assert c8.counter("f16_range_repeats") == 0
    for i in range(n):
        if i != bad:
            assert np.array_equal(res[i].Transformation, clean[i].Transformation) and np.array_equal(res[i].Information, clean[i].Information)
            assert res[i].LogLikelihood == clean[i].LogLikelihood


def test_window_sweep_whole_matches_and_plane_flavours():
    """Whole matches on the three schedules (5: gathered taps; 6: window, f32 Gram -- identical records; 7: f16 Gram on every level --
    the same iteration structure up to one step on a level, transforms within 2e-7), and the two flavours of the current role: frames ingested in a batch too large
    for the resident kernel carry only the 8-byte plane C at the window levels; the taps A + B (a plane download, a small batch that
    runs the level resident) and the reference role (point selection) are derived from it on demand, bit-identically."""
    w, h, levels = 640, 480, 4
    pair = cm.synth(1234, w, h)
    res = {}
    for v in (5, 6, 7):
        ctx = d.Context(0)
        ctx.set_option("variant", v)
        ctx.set_option("rows_per_wave", 4)
        ctx.set_option("resident", 0)
        gref, gcur = gpu_pyramids(ctx, pair, levels)
        r = d.Result()
        d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx).match(gref, gcur, r)
        res[v] = r
    assert np.array_equal(res[5].Transformation, res[6].Transformation) and np.array_equal(res[5].Information, res[6].Information)
    # (the f16 Gram differs from the f32 one in the 7th digit of the normal equations: a termination test on the edge may fall the
    # other way on some level, the transforms agree far below the tracker's precision)
    its5, its7 = ([len(L.Iterations) for L in res[v].Statistics.Levels] for v in (5, 7))
    print("iterations per level: variant 5 %s, variant 7 %s; twist distance %.2e" % (its5, its7, cm.twist_matrix_error(res[5].Transformation, res[7].Transformation)))
    assert all(abs(a - b) <= 1 for a, b in zip(its5, its7))
    assert cm.twist_matrix_error(res[5].Transformation, res[7].Transformation) < 2e-7
    # flavours: 300 frames ingested as current frames in ONE call (> compute units: plane C only at levels 0 and 1)
    ctx = d.Context(0)
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    K = pair["K"]
    cam = d.RgbdCameraPyramid(w, h, K, ctx)
    cam.build(levels)
    n = 300
    b = datagen.synth_batch(5, 3, w, h)
    dummy = np.zeros((h, w), np.uint8), np.full((h, w), 5000, np.uint16)
    frames = [cam.create_raw(*dummy) for _ in range(n)]
    grey = [np.ascontiguousarray(b["grey_cur"][i % 3]) for i in range(n)]
    depth = [np.ascontiguousarray(b["depth_cur"][i % 3]) for i in range(n)]
    d.update_raw_host_batch(frames, grey, depth, role="current", config=cfg)
    long_way = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(3)]
    names = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")
    for i in (0, 1, 2, 299):
        for l in range(levels):
            for k in names:                                             # (the download derives A + B from C at levels 0 and 1)
                assert np.array_equal(getattr(frames[i].level(l), k), getattr(long_way[i % 3].level(l), k), equal_nan=True), (i, l, k)
    d.update_raw_host_batch(frames, grey, depth, role="current", config=cfg)            # C only again
    for l in range(levels):                                             # the reference role from a C-only current frame
        assert d.PointSelection(frames[1]).select(l) == d.PointSelection(long_way[1]).select(l)
        assert d.PointSelection(frames[2], 6.0, 0.03).select(l) == d.PointSelection(long_way[2], 6.0, 0.03).select(l)
    # ... and alignments: the same records whichever way the planes came about, in both roles, on both paths
    d.update_raw_host_batch(frames, grey, depth, role="current", config=cfg)
    refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(3)]
    trk = d.DenseTracker(cfg, ctx)

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations"))
    for resident in (0, -1):
        ctx.set_option("resident", resident)
        want = raw(trk.match_batch_arrays(refs, long_way))
        d.update_raw_host_batch(frames, grey, depth, role="current", config=cfg)
        assert raw(trk.match_batch_arrays(refs, frames[:3])) == want                    # current role: C (launch path) / A + B from C (resident)
        want_back = raw(trk.match_batch_arrays(long_way, refs))
        d.update_raw_host_batch(frames, grey, depth, role="current", config=cfg)
        assert raw(trk.match_batch_arrays(frames[:3], refs)) == want_back               # reference role from C


def test_golden_linearisation(gpu_ctx):
    g = cm.load_golden("s160_seed7.npz")
    pair = dict(grey_ref=g["grey_ref"], depth_ref=g["depth_ref"], grey_cur=g["grey_cur"], depth_cur=g["depth_cur"], K=g["K"])
    gref, gcur = gpu_pyramids(gpu_ctx, pair, 3)
    trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), gpu_ctx)
    # the exact schedule, and the default one (contracted arithmetic: a 160-pixel level is the window sweep's since round 4, its last
    # tile column half empty) at the log-likelihood tolerance test_contracted_sweep_against_the_exact_one states
    try:
        for variant, ll_tol in ((EXACT_VARIANT, 1e-6), (DEFAULT_VARIANT, 2e-5)):
            gpu_ctx.set_option("variant", variant)
            a = trk.level_iteration(gref, gcur, 0, g["lin_T34"], first=True)
            exp = g["lin_math_first"]
            assert a["n"] == int(exp[0])
            assert abs(a["neg_ll"] - exp[1]) <= ll_tol * abs(exp[1])
            if variant == EXACT_VARIANT:
                assert np.allclose(a["P"].ravel(), exp[5:9], rtol=1e-5)
            else:                                                        # (the small off-diagonal term is a difference of large ones)
                assert np.abs(a["P"].ravel() - exp[5:9]).max() <= 1e-5 * np.abs(exp[5:9]).max()
            assert np.abs(a["A"].ravel() - exp[9:45]).max() <= 1e-5 * np.abs(exp[9:45]).max()
            assert np.abs(a["b"] - exp[45:51]).max() <= 1e-5 * np.abs(exp[45:51]).max()
            b = trk.level_iteration(gref, gcur, 0, g["lin_T34"], P_prev=exp[5:9], first=False)
            exp2 = g["lin_math_weighted"]
            assert b["n"] == int(exp2[0])
            assert np.abs(b["A"].ravel() - exp2[9:45]).max() <= 1e-5 * np.abs(exp2[9:45]).max()
    finally:
        gpu_ctx.set_option("variant", DEFAULT_VARIANT)


def run_gpu_match(ctx, gref, gcur, cfg, T_init=None):
    ctx.set_option("condition_number", 1)
    trk = d.DenseTracker(cfg, ctx)
    r = d.Result()
    if T_init is not None:
        r.Transformation = np.array(T_init, dtype=np.float64)
    assert trk.match(gref, gcur, r) is True
    return cm.tracker_result_to_dict(r)


FULL_MATCHES = [
    (1234, 640, 480, 3, 0, 0.0, False, 5e-7, None),     # BASELINE config 2: single 640x480 pair, 4 levels, finest level 0
    (1234, 640, 480, 3, 0, 0.0, False, 1e-4, None),
    (5, 640, 480, 3, 1, 0.05, True, 1e-4, None),        # dvo_benchmark/launch/benchmark.yaml
    (6, 640, 480, 3, 1, 0.0, False, 5e-7, None),        # reference defaults
    (7, 160, 120, 2, 0, 0.0, False, 5e-7, None),
    (4321, 1280, 960, 4, 0, 0.0, False, 1e-4, None),    # BASELINE config 5: 1280x960, 5 levels
    (9, 131, 97, 2, 0, 0.0, False, 5e-7, None),         # odd sizes: every level has ragged tiles
    (10, 258, 194, 3, 0, 0.05, True, 1e-4, None),
    # a camera that is not fr1 (tests/cameras.py) at the stopping precision; 640 x 480 because below that size two implementations
    # with bit-identical residuals end a pass apart on the noise floor (tests/test_camera_models.py)
    (1234, 640, 480, 3, 0, 0.0, False, 5e-7, "aniso"),
]


@pytest.mark.parametrize("seed,w,h,first,last,mu,init,precision,camera", FULL_MATCHES,
                         ids=["-".join(str(v) for v in c[:8] + ((c[8],) if c[8] else ())) for c in FULL_MATCHES])
def test_full_match_against_oracle(gpu_ctx, seed, w, h, first, last, mu, init, precision, camera):
    pair = cm.synth(seed, w, h, cameras.CAMERAS(w, h)[camera] if camera else None)
    oref, ocur = cm.oracle_pyramids(pair, first + 1)
    gref, gcur = gpu_pyramids(gpu_ctx, pair, first + 1)
    cfg = d.Config(FirstLevel=first, LastLevel=last, Mu=mu, UseInitialEstimate=init, Precision=precision,
                   MaxIterationsPerLevel=50 if init else 100)
    T0 = po.se3_exp(0.5 * pair["xi_true"]) if init else None
    g = run_gpu_match(gpu_ctx, gref, gcur, cfg, T0)
    o = po.match(oref, ocur, cm.oracle_config_from(cfg, po.MATH), T0)
    s = cm.compare_runs(g, o)
    assert s["n_mismatch"] == 0 and s["max_x_err"] < 2e-5, s
    assert s["max_iter_count_diff"] <= 2, s
    assert s["T_err"] < (2e-5 if precision > 1e-6 else 1e-6), s
    if s["structure_mismatch"] == 0:
        assert np.abs(g["information"] - o["information"]).max() <= 2e-3 * np.abs(o["information"]).max()
        assert abs(g["loglik"] - o["loglik"]) <= 1e-3 * abs(o["loglik"])
    # keyframe-selection statistics computed on the device = the reference's host-side derivations from the same result
    k = cm.keyframe_statistics_from(g)
    assert g["entropy"] == pytest.approx(k["entropy"], rel=1e-12) and g["condition_number"] == pytest.approx(k["condition_number"], rel=1e-9)
    assert g["constraint_ratio"] == k["constraint_ratio"] and g["constraint_ratio_accepted"] == k["constraint_ratio_accepted"]
    if s["structure_mismatch"] == 0:
        ko = cm.keyframe_statistics_from(o)
        assert g["entropy"] == pytest.approx(ko["entropy"], abs=2e-2) and g["constraint_ratio"] == pytest.approx(ko["constraint_ratio"], abs=1e-3)
    # and against the quirk-faithful restatement of the SSE path, and the ground truth of the synthetic pair
    q = po.match(oref, ocur, cm.oracle_config_from(cfg, po.REF_SSE), T0)
    assert cm.twist_matrix_error(g["T"], q["T"]) < 5e-5
    assert np.abs(po.se3_log(g["T"]) - pair["xi_true"]).max() < (1e-4 if w >= 160 else 5e-4)   # the estimator's accuracy, by image size
    # ... and against the REFERENCE ITSELF: its own DenseTracker::match(), compiled from /root/reference into oracle/_ref (the built
    # library travels to the GPU box), on the same frames.  REF_SSE reproduces it bit for bit; the GPU within the quirk distance.
    if po.ref_lib() is not None and w % (4 << first) == 0:   # the reference's SSE derivative needs widths that are multiples of 4
        r = po.ref_match(pair["grey_ref"].astype(np.float32), po.convert_raw_depth(pair["depth_ref"]),
                         pair["grey_cur"].astype(np.float32), po.convert_raw_depth(pair["depth_cur"]), pair["K"],
                         cm.oracle_config_from(cfg, po.REF_SSE), T0)
        assert np.array_equal(r["T"], q["T"]) and [len(L["iterations"]) for L in r["levels"]] == [len(L["iterations"]) for L in q["levels"]]
        assert cm.twist_matrix_error(g["T"], r["T"]) < 5e-5


def test_golden_full_match(gpu_ctx):
    g = cm.load_golden("s160_seed7.npz")
    pair = dict(grey_ref=g["grey_ref"], depth_ref=g["depth_ref"], grey_cur=g["grey_cur"], depth_cur=g["depth_cur"], K=g["K"])
    gref, gcur = gpu_pyramids(gpu_ctx, pair, 3)
    run = run_gpu_match(gpu_ctx, gref, gcur, d.Config(FirstLevel=2, LastLevel=0, MaxIterationsPerLevel=100, Precision=5e-7))
    assert cm.twist_matrix_error(run["T"], g["math_T"]) < 1e-6
    assert cm.twist_matrix_error(run["T"], g["ref_sse_T"]) < 5e-5
    rows = g["math_iters"]
    first_level_rows = rows[rows[:, 0] == 2]
    for it, row in zip(run["levels"][0]["iterations"][:3], first_level_rows[:3]):   # the first passes are far from the noise floor
        assert it["n"] == int(row[2])
        assert abs(it["neg_ll"] - row[3]) <= 1e-5 * abs(row[3])
        assert np.abs(it["x"] - row[8:14]).max() < 1e-6


def test_batch_equals_singles_and_is_deterministic(gpu_ctx):
    pairs = [cm.synth(100 + i, 320, 240) for i in range(6)]
    pyr = [gpu_pyramids(gpu_ctx, p, 3) for p in pairs]
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    singles = []
    for r, c in pyr:
        res = d.Result()
        trk.match(r, c, res)
        singles.append(res)
    for rep in range(2):
        batch = [d.Result() for _ in pyr]
        trk.match_batch([p[0] for p in pyr], [p[1] for p in pyr], batch, with_stats=True)
        for s, b in zip(singles, batch):
            # fixed-order reductions: a pair's result must not depend on what else is in the launch.
            # (tile height differs between batch sizes, so allow float rounding, not more)
            assert cm.twist_matrix_error(s.Transformation, b.Transformation) < 1e-6
        if rep == 0:
            first = batch
        else:
            for a, b in zip(first, batch):   # same launch geometry twice: bit-identical
                assert np.array_equal(a.Transformation, b.Transformation)
                assert np.array_equal(a.Information, b.Information)
    # shared frames in one batch (the LocalTracker pattern: two references against one current frame)
    res = [d.Result(), d.Result()]
    trk.match_batch([pyr[0][0], pyr[1][0]], [pyr[0][1], pyr[0][1]], res)
    assert cm.twist_matrix_error(res[0].Transformation, singles[0].Transformation) < 1e-6


def test_properties_at_full_size(gpu_ctx):
    pair = cm.synth(77)
    gref, gcur = gpu_pyramids(gpu_ctx, pair, 4)
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    # identical frames: the alignment is the identity and the first increment is (numerically) zero
    r = d.Result()
    trk.match(gref, gref, r)
    assert np.abs(po.se3_log(r.Transformation)).max() < 1e-6
    # swapping the roles inverts the transform (up to the asymmetric hole patterns / occlusion test)
    a, b = d.Result(), d.Result()
    trk.match(gref, gcur, a)
    trk.match(gcur, gref, b)
    assert cm.twist_matrix_error(a.Transformation, np.linalg.inv(b.Transformation)) < 2e-4
    # information matrix is symmetric positive definite, statistics are appended not cleared (Q15)
    assert np.allclose(a.Information, a.Information.T) and np.linalg.eigvalsh(a.Information).min() > 0
    n_levels = len(a.Statistics.Levels)
    trk.match(gref, gcur, a)
    assert len(a.Statistics.Levels) == 2 * n_levels
    # Affine-matrix overload (dense_tracking.cpp:99-109): in/out 4x4
    T = np.eye(4)
    assert trk.match(gref, gcur, T) is True
    assert cm.twist_matrix_error(T, b.Transformation if False else a.Transformation) < 1e-9


def test_edge_cases(gpu_ctx):
    # no depth at all -> n = 0 on every level, identity out, NaN information, criterion IncrementTooSmall (Q22)
    h, w = 120, 160
    I = np.random.default_rng(0).uniform(0, 255, (h, w)).astype(np.float32)
    Z = np.full((h, w), np.nan, np.float32)
    cam = d.RgbdCameraPyramid(w, h, po.FR1_K / 4, gpu_ctx)
    cam.build(3)
    a, b = cam.create(I, Z), cam.create(I, Z)
    r = d.Result()
    d.DenseTracker(d.Config(FirstLevel=2, LastLevel=0), gpu_ctx).match(a, b, r)
    assert r.isNaN() and np.allclose(r.Transformation, np.eye(4))
    assert np.isnan(r.Entropy) and np.isnan(r.ConditionNumber) and np.isnan(r.ConstraintRatioAccepted)    # 0 constraints / 0 pixels
    assert [L.TerminationCriterion for L in r.Statistics.Levels] == [1, 1, 1]
    assert all(len(L.Iterations) == 1 and L.Iterations[0].ValidConstraints == 0 for L in r.Statistics.Levels)
    # misuse is rejected with an error code, not a crash
    with pytest.raises(d.DvoHipError):
        gpu_ctx.set_option("rows_per_wave", 3)
    trk = d.DenseTracker(d.Config(FirstLevel=2, LastLevel=0), gpu_ctx)
    small = d.RgbdCameraPyramid(w // 2, h // 2, po.FR1_K / 8, gpu_ctx)
    small.build(3)
    c = small.create(I[::2, ::2].copy(), Z[::2, ::2].copy())
    with pytest.raises(d.DvoHipError):
        trk.match(a, c, d.Result())          # frames of different cameras in one match
    # iteration cap and a ragged (non multiple-of-64) image
    pair = cm.synth(3, 100, 76)
    gref, gcur = gpu_pyramids(gpu_ctx, pair, 2)
    oref, ocur = cm.oracle_pyramids(pair, 2)
    cfg = d.Config(FirstLevel=1, LastLevel=0, MaxIterationsPerLevel=3, Precision=0.0)
    g = run_gpu_match(gpu_ctx, gref, gcur, cfg)
    o = po.match(oref, ocur, cm.oracle_config_from(cfg, po.MATH))
    s = cm.compare_runs(g, o)
    assert s["structure_mismatch"] == 0 and s["n_mismatch"] == 0 and s["T_err"] < 1e-6
    assert all(len(L["iterations"]) <= 3 for L in g["levels"])


def test_cpp_facade_matches_python_path(gpu_ctx, tmp_path):
    """The header-only C++ facade (include/dvo/), driven like dvo_benchmark drives dvo_core, gives the same transform."""
    import subprocess
    from test_capi import build_facade_example
    exe = build_facade_example()
    pair = cm.synth(55, 320, 240)
    frames = np.stack([pair["grey_ref"].astype(np.float32), po.convert_raw_depth(pair["depth_ref"]),
                       pair["grey_cur"].astype(np.float32), po.convert_raw_depth(pair["depth_cur"])])
    raw = tmp_path / "frames.raw"
    frames.tofile(raw)
    out = subprocess.check_output([exe, str(raw), "320", "240", "2", "0"], text=True)
    lines = out.strip().splitlines()
    assert lines[0].startswith("ok 1 nan 0 levels 3")
    T = np.array([[float(v) for v in ln.split()] for ln in lines[1:5]])
    gref, gcur = gpu_pyramids(gpu_ctx, pair, 3)
    g = run_gpu_match(gpu_ctx, gref, gcur, d.Config(FirstLevel=2, LastLevel=0))
    assert cm.twist_matrix_error(T, g["T"]) < 1e-9
    assert np.abs(po.se3_log(T) - pair["xi_true"]).max() < 1e-4


def test_device_ingest_prepare_and_background_build(gpu_ctx):
    """Frames ingested from device-resident raw planes, role planes prepared ahead of time, and a build of OTHER frames in
    flight on the build stream while a batch is aligned: none of it may change a single bit of the results."""
    import ctypes as C
    # plain device buffers for the raw planes, from the HIP runtime this process already has loaded (the library's own, or
    # torch's bundled copy when another test module imported torch first)
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert loaded, "libdvo_hip.so should have pulled in the HIP runtime"
    hip = C.CDLL(loaded[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def to_device(arr):
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), arr.nbytes) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0
        return p.value
    n, w, h = 6, 320, 240
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    cam = d.RgbdCameraPyramid(w, h, po.FR1_K * 0.5, gpu_ctx)
    cam.build(3)
    batches = [datagen.synth_batch(seed, n, w, h) for seed in (100, 200)]

    def host_frames(b):
        return ([cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)],
                [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)])

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations", "entropy"))
    base = []
    for b in batches:
        refs, curs = host_frames(b)
        base.append(raw(trk.match_batch_arrays(refs, curs)))
    assert base[0] != base[1]

    dev = []
    for b in batches:
        g = to_device(np.concatenate([b["grey_ref"], b["grey_cur"]]))
        z = to_device(np.concatenate([b["depth_ref"], b["depth_cur"]]))
        dev.append((g, z, [g + i * w * h for i in range(2 * n)], [z + 2 * i * w * h for i in range(2 * n)]))
    sets = [[cam.create_raw_device(dev[k][2][i], dev[k][3][i]) for i in range(2 * n)] for k in range(2)]
    for k in range(2):   # device ingest == host ingest
        assert raw(trk.match_batch_arrays(sets[k][:n], sets[k][n:])) == base[k]
    # re-ingest + eager role planes, then match
    d.update_raw_device_batch(sets[0], dev[0][2], dev[0][3])
    d.prepare_roles_batch(sets[0][:n], "reference", cfg)
    d.prepare_roles_batch(sets[0][n:], "current", cfg)
    assert raw(trk.match_batch_arrays(sets[0][:n], sets[0][n:])) == base[0]
    # a frame that is prepared for both roles can be used in either (the inverse pairing just has to run)
    d.prepare_roles_batch(sets[0][:n], "current", cfg)
    assert np.isfinite(trk.match_batch_arrays(sets[0][n:], sets[0][:n])["T"]).all()
    # set 1 is rebuilt (with set 0's data!) while set 0 is aligned: set 0's result is untouched, set 1 now gives set 0's result
    for _ in range(3):
        d.update_raw_device_batch(sets[1], dev[0][2], dev[0][3])
        d.prepare_roles_batch(sets[1][:n], "reference", cfg)
        d.prepare_roles_batch(sets[1][n:], "current", cfg)
        assert raw(trk.match_batch_arrays(sets[0][:n], sets[0][n:])) == base[0]
        assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[0]
        d.update_raw_device_batch(sets[1], dev[1][2], dev[1][3])         # back to its own data, roles built lazily by the match
        assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[1]
    # a narrow background build (grid-stride kernels) writes the same planes
    gpu_ctx.set_option("build_workgroups", 64)
    d.update_raw_device_batch(sets[1], dev[0][2], dev[0][3])
    d.prepare_roles_batch(sets[1][:n], "reference", cfg)
    d.prepare_roles_batch(sets[1][n:], "current", cfg)
    gpu_ctx.set_option("build_workgroups", 0)
    assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[0]
    # option "defer_ingest" (round 5): a role-aware re-ingest is only recorded and carried out by the NEXT match behind its first launches
    # -- of set 1 (with set 0's data) while set 0 is aligned; a match of the recorded frames themselves, or any other entry point,
    # carries it out first; switching the option off carries out what is left.  Not a bit of any result changes.
    k0 = gpu_ctx.counter("deferred_ingests")
    gpu_ctx.set_option("defer_ingest", 1)
    d.update_raw_device_batch(sets[1][:n], dev[0][2][:n], dev[0][3][:n], role="reference", config=cfg)
    d.update_raw_device_batch(sets[1][n:], dev[0][2][n:], dev[0][3][n:], role="current", config=cfg)
    assert gpu_ctx.counter("deferred_ingests") == k0                                   # recorded, nothing built yet
    assert raw(trk.match_batch_arrays(sets[0][:n], sets[0][n:])) == base[0]            # ... carried out behind this match's first launches
    assert gpu_ctx.counter("deferred_ingests") == k0 + 2
    assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[0]
    d.update_raw_device_batch(sets[1][:n], dev[1][2][:n], dev[1][3][:n], role="reference", config=cfg)
    d.update_raw_device_batch(sets[1][n:], dev[1][2][n:], dev[1][3][n:], role="current", config=cfg)
    assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[1]            # the recorded frames themselves: ingested first
    d.update_raw_device_batch(sets[1][:n], dev[0][2][:n], dev[0][3][:n], role="reference", config=cfg)
    assert d.PointSelection(sets[1][0]).select(0) == d.PointSelection(sets[0][0]).select(0)   # another entry point: ingested first
    d.update_raw_device_batch(sets[1][n:], dev[0][2][n:], dev[0][3][n:], role="current", config=cfg)
    gpu_ctx.set_option("defer_ingest", 0)                                              # carries out the recorded one
    assert gpu_ctx.counter("deferred_ingests") == k0 + 6
    assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[0]
    # option "keep_raw_copy" = 0 (round 5; the streaming loop's reference frames): the frame serves in the role and with the thresholds
    # it was ingested for -- the same bits -- and says so when asked for anything else, until it is ingested again
    gpu_ctx.set_option("keep_raw_copy", 0)
    d.update_raw_device_batch(sets[1][:n], dev[1][2][:n], dev[1][3][:n], role="reference", config=cfg)
    gpu_ctx.set_option("keep_raw_copy", 1)
    d.update_raw_device_batch(sets[1][n:], dev[1][2][n:], dev[1][3][n:], role="current", config=cfg)
    assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[1]
    with pytest.raises(d.DvoHipError):
        d.prepare_roles_batch(sets[1][:n], "current", cfg)
    with pytest.raises(d.DvoHipError):
        d.prepare_roles_batch(sets[1][:n], "reference", d.Config(FirstLevel=2, LastLevel=0, IntensityDerivativeThreshold=3.0))
    assert raw(trk.match_batch_arrays(sets[1][:n], sets[1][n:])) == base[1]            # (the failed requests left the frames alone)
    d.update_raw_device_batch(sets[1][:n], dev[1][2][:n], dev[1][3][:n], role="reference", config=cfg)   # with the copy again
    d.prepare_roles_batch(sets[1][:n], "current", cfg)
    assert np.isfinite(trk.match_batch_arrays(sets[1][n:], sets[1][:n])["T"]).all()
    with pytest.raises(d.DvoHipError):
        d.prepare_roles_batch(sets[0][:n], "reference", d.Config(FirstLevel=5, LastLevel=0))   # more levels than the frames have
    del sets
    for g, z, _, _ in dev:
        hip.hipFree(C.c_void_p(g))
        hip.hipFree(C.c_void_p(z))


@pytest.mark.gpu
def test_table_cache_never_serves_a_stale_table():
    """Round 5: the small tables of a batch (plane pointers of its frames and pairs, initial guesses) are not sent to the device again
    when the very bytes are already there (option table_cache, counter table_uploads_skipped).  The cache compares CONTENTS: a frame
    that is destroyed and replaced -- its device block is pooled, so the new frame has the old one's addresses -- by a frame with other
    pixels gives the other pixels' result, and every result equals the one of a context without the cache, bit for bit."""
    n, w, h = 6, 320, 240
    b = datagen.synth_batch(300, n + 1, w, h)
    cfg = d.Config(FirstLevel=2, LastLevel=0)

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations"))

    runs = {}
    for cache in (1, 0):
        ctx = d.Context(0)
        ctx.set_option("table_cache", cache)
        ctx.set_option("resident", 0)
        cam = d.RgbdCameraPyramid(w, h, b["K"], ctx)
        cam.build(3)
        refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
        curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
        trk = d.DenseTracker(cfg, ctx)
        first = raw(trk.match_batch_arrays(refs, curs))
        k0 = ctx.counter("table_uploads_skipped")
        again = raw(trk.match_batch_arrays(refs, curs))                       # the same tables: nothing is sent
        assert again == first
        assert (ctx.counter("table_uploads_skipped") > k0) == bool(cache)
        # pair 2 gets another current frame: the old one is destroyed first, the new one takes over its pooled device block
        curs[2] = None
        curs[2] = cam.create_raw(b["grey_cur"][n], b["depth_cur"][n])
        swapped = trk.match_batch_arrays(refs, curs)
        assert not np.array_equal(swapped["T"][2], np.frombuffer(first[:n * 128], np.float64).reshape(n, 4, 4)[2])
        runs[cache] = (first, raw(swapped), raw(trk.match_batch_arrays(refs, curs)))
        assert runs[cache][1] == runs[cache][2]
    assert runs[1] == runs[0]


@pytest.mark.gpu
def test_table_cache_with_alternating_batch_sizes():
    """Round-5 advisor finding: the role tables of a match (ensure_roles) are slices of one buffer at offsets that depend on the batch
    size, so the slices of batches of 3, 2, 3 pairs overlap without sharing a start address.  With a re-ingest between the matches (the
    role planes have to be derived again, through those tables) the third batch must find ITS table on the device, not the second's:
    every record equals the one of a context without the cache, bit for bit."""
    w, h = 320, 240
    b = datagen.synth_batch(310, 3, w, h)
    b2 = datagen.synth_batch(320, 3, w, h)
    cfg = d.Config(FirstLevel=2, LastLevel=0)

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations"))

    runs = {}
    for cache in (1, 0):
        ctx = d.Context(0)
        ctx.set_option("table_cache", cache)
        ctx.set_option("resident", 0)
        cam = d.RgbdCameraPyramid(w, h, b["K"], ctx)
        cam.build(3)
        refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(3)]
        curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(3)]
        trk = d.DenseTracker(cfg, ctx)
        out = []
        for step, (n, src) in enumerate([(3, b), (2, b2), (3, b), (2, b), (3, b2)]):
            # new pixels in every frame (plain re-ingest: no role planes, the match derives them through the role tables)
            d.update_raw_host_batch(refs, [np.ascontiguousarray(src["grey_ref"][i]) for i in range(3)], [np.ascontiguousarray(src["depth_ref"][i]) for i in range(3)])
            d.update_raw_host_batch(curs, [np.ascontiguousarray(src["grey_cur"][i]) for i in range(3)], [np.ascontiguousarray(src["depth_cur"][i]) for i in range(3)])
            d.upload_wait(ctx)
            out.append(raw(trk.match_batch_arrays(refs[:n], curs[:n])))
        assert out[0] == out[2], "the same pixels, the same batch: the same records"
        runs[cache] = out
    assert runs[1] == runs[0]


@pytest.mark.gpu
def test_reference_without_raw_copy_fails_cleanly_in_the_other_role():
    """Round-5 advisor finding: a frame ingested straight into the reference role with DVO_HIP_INGEST_NO_RAW_COPY has nothing its
    current role could be derived from.  Asking for it fails with DVO_HIP_ERR_INVALID BEFORE the state of any frame of the list is
    touched: the same list without the offending frame then aligns to the same bits as on a fresh context."""
    import ctypes as C
    from dvo_slam_amd import _lib
    w, h = 320, 240
    b = datagen.synth_batch(330, 3, w, h)
    cfg = d.Config(FirstLevel=2, LastLevel=0)

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations"))

    def frames(ctx):
        cam = d.RgbdCameraPyramid(w, h, b["K"], ctx)
        cam.build(3)
        refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(3)]
        curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(3)]
        return cam, refs, curs

    ctx0 = d.Context(0)
    ctx0.set_option("resident", 0)
    _, refs0, curs0 = frames(ctx0)
    want = raw(d.DenseTracker(cfg, ctx0).match_batch_arrays(refs0[:2], curs0[:2]))

    ctx = d.Context(0)
    ctx.set_option("resident", 0)
    cam, refs, curs = frames(ctx)
    # frame 2 of the CURRENT list becomes a reference without a raw copy (device planes: staged through a torch tensor)
    import torch
    g = torch.from_numpy(np.ascontiguousarray(b["grey_cur"][2])).cuda()
    z = torch.from_numpy(np.ascontiguousarray(b["depth_cur"][2]).view(np.int16)).cuda()
    vp = C.c_void_p
    fr = d.tracker._handles([curs[2]])
    ccfg = cfg.to_c()
    rc = ctx._lib.dvo_hip_frames_update_raw_device_as_ex(ctx.ptr, 1, fr, (vp * 1)(vp(g.data_ptr())), (vp * 1)(vp(z.data_ptr())), 1.0 / 5000.0,
                                                         _lib.ROLE_REFERENCE, C.byref(ccfg), _lib.INGEST_NO_RAW_COPY)
    assert rc == 0
    trk = d.DenseTracker(cfg, ctx)
    with pytest.raises(d.DvoHipError):
        trk.match_batch_arrays(refs, curs)                       # curs[2] cannot play the current role
    assert raw(trk.match_batch_arrays(refs[:2], curs[:2])) == want


@pytest.mark.gpu
def test_streaming_upload_from_host_memory(gpu_ctx):
    """dvo_hip_frames_update_raw: raw planes handed over in host memory (pinned block in the frame layout, pinned but separate
    planes, plain pageable numpy arrays) and DMA-ed on the upload stream while OTHER frames are aligned -- bit-identical results
    to frames created synchronously from the same planes, batch after batch on the same frame objects."""
    n, w, h = 5, 320, 240
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    cam = d.RgbdCameraPyramid(w, h, po.FR1_K * 0.5, gpu_ctx)
    cam.build(3)
    batches = [datagen.synth_batch(seed, n, w, h) for seed in (300, 400, 500)]

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations", "entropy"))
    base = []
    for b in batches:
        refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
        curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
        base.append(raw(trk.match_batch_arrays(refs, curs)))
    assert len(set(base)) == 3

    pinned = [d.PinnedRawPlanes(gpu_ctx, 2 * n, w, h) for _ in batches]
    for P, b in zip(pinned, batches):
        for i in range(n):
            P.grey[i][:], P.depth[i][:] = b["grey_ref"][i], b["depth_ref"][i]
            P.grey[n + i][:], P.depth[n + i][:] = b["grey_cur"][i], b["depth_cur"][i]
    sets = [[cam.create_raw(batches[0]["grey_ref"][0], batches[0]["depth_ref"][0]) for _ in range(2 * n)] for _ in range(2)]
    # pipeline: upload + build batch k+1 into one frame set while batch k is aligned on the other
    d.update_raw_host_batch(sets[0], pinned[0].grey, pinned[0].depth)
    for rounds in range(2):
        for k in range(3):
            nxt = (k + 1) % 3
            j = (rounds * 3 + k) % 2
            d.update_raw_host_batch(sets[1 - j], pinned[nxt].grey, pinned[nxt].depth)
            d.prepare_roles_batch(sets[1 - j][:n], "reference", cfg)
            d.prepare_roles_batch(sets[1 - j][n:], "current", cfg)
            assert raw(trk.match_batch_arrays(sets[j][:n], sets[j][n:])) == base[k]
    d.upload_wait(gpu_ctx)
    # separate (non-adjacent) planes take the two-transfer path; pageable memory is staged by the runtime
    b = batches[1]
    grey = [np.ascontiguousarray(a) for a in list(b["grey_ref"]) + list(b["grey_cur"])]
    depth = [np.ascontiguousarray(a) for a in list(b["depth_ref"]) + list(b["depth_cur"])]
    d.update_raw_host_batch(sets[0], grey, depth)
    d.upload_wait(gpu_ctx)
    assert raw(trk.match_batch_arrays(sets[0][:n], sets[0][n:])) == base[1]
    d.update_raw_host_batch(sets[0], pinned[2].grey[::-1][:2 * n][::-1], pinned[2].depth)     # same planes, list rebuilt
    assert raw(trk.match_batch_arrays(sets[0][:n], sets[0][n:])) == base[2]
    with pytest.raises(AssertionError):
        d.update_raw_host_batch(sets[0], [g.astype(np.float32) for g in grey], depth)
    del sets
    for P in pinned:
        P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,levels", [(320, 240, 3), (102, 78, 3), (640, 480, 4), (140, 62, 3), (388, 122, 4),
                                        (65, 33, 2)])    # the tile ingest in both roles, the other role from the raw copy and from plane C
def test_role_aware_ingest_is_bit_identical(gpu_ctx, w, h, levels):
    """dvo_hip_frames_update_raw_as: level 0 written straight from the raw planes into the role's planes (no float planes at
    level 0, 4-pixel-wide loads when the rows allow it).  Same planes, same selection, same alignment results as frames built
    the long way -- also when a frame is later used in the OTHER role (reference from its sampling planes, current from the
    raw copy it kept)."""
    n = 4
    cfg = d.Config(FirstLevel=levels - 1, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    K = po.FR1_K * (w / 640.0)
    cam = d.RgbdCameraPyramid(w, h, K, gpu_ctx)
    cam.build(levels)
    b = datagen.synth_batch(77, n, w, h)

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations", "entropy"))
    refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
    curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
    forward, backward = raw(trk.match_batch_arrays(refs, curs)), raw(trk.match_batch_arrays(curs, refs))
    assert forward != backward
    names = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")

    def all_planes(f):
        return [np.array(getattr(f.level(l), k)) for l in range(levels) for k in names]

    def count(f, level, ithr=0.0, dthr=0.0):
        return d.PointSelection(f, ithr, dthr).select(level)
    planes = [all_planes(f) for f in (refs[0], curs[0])]
    counts = [count(refs[0], l) for l in range(levels)]

    dummy = np.zeros((h, w), np.uint8), np.full((h, w), 5000, np.uint16)
    R = [cam.create_raw(*dummy) for _ in range(n)]
    Cu = [cam.create_raw(*dummy) for _ in range(n)]
    gr = [np.ascontiguousarray(a) for a in b["grey_ref"]]
    zr = [np.ascontiguousarray(a) for a in b["depth_ref"]]
    gc = [np.ascontiguousarray(a) for a in b["grey_cur"]]
    zc = [np.ascontiguousarray(a) for a in b["depth_cur"]]
    for rounds in range(2):
        d.update_raw_host_batch(R, gr, zr, role="reference", config=cfg)
        d.update_raw_host_batch(Cu, gc, zc, role="current", config=cfg)
        assert raw(trk.match_batch_arrays(R, Cu)) == forward
        assert raw(trk.match_batch_arrays(Cu, R)) == backward          # each frame in the role it was NOT built for
        assert raw(trk.match_batch_arrays(R, Cu)) == forward
    for want_f, got_f in zip(planes, [all_planes(f) for f in (R[0], Cu[0])]):
        for a, c in zip(want_f, got_f):
            assert np.array_equal(a, c, equal_nan=True)
    assert [count(R[0], l) for l in range(levels)] == counts
    # other thresholds on a role-ingested frame, then back
    n_tight = count(R[1], 0, 8.0, 0.02)
    assert 0 < n_tight < count(refs[1], 0) and n_tight == count(refs[1], 0, 8.0, 0.02)
    assert raw(trk.match_batch_arrays(R, Cu)) == forward
    # argument errors of the C-ABI entry point: unknown role, more levels than the frames have, a null plane
    import ctypes as C
    vp = C.c_void_p
    L, fr = gpu_ctx._lib, (vp * n)(*[f.ptr for f in R])
    g = (vp * n)(*[vp(a.ctypes.data) for a in gr])
    z = (vp * n)(*[vp(a.ctypes.data) for a in zr])
    ok_cfg, deep = cfg.to_c(), d.Config(FirstLevel=levels + 1, LastLevel=0).to_c()
    assert L.dvo_hip_frames_update_raw_as(gpu_ctx.ptr, n, fr, g, z, 0.0002, 7, C.byref(ok_cfg)) == d._lib.ERR_INVALID
    assert L.dvo_hip_frames_update_raw_as(gpu_ctx.ptr, n, fr, g, z, 0.0002, 1, C.byref(deep)) == d._lib.ERR_INVALID
    assert L.dvo_hip_frames_update_raw_as(gpu_ctx.ptr, n, fr, g, z, 0.0002, 1, None) == d._lib.ERR_INVALID
    g_bad = (vp * n)(*([vp(a.ctypes.data) for a in gr[:-1]] + [vp(None)]))
    assert L.dvo_hip_frames_update_raw_as(gpu_ctx.ptr, n, fr, g_bad, z, 0.0002, 1, C.byref(ok_cfg)) == d._lib.ERR_INVALID
    assert L.dvo_hip_frames_update_raw_device_as(gpu_ctx.ptr, n, fr, g_bad, z, 0.0002, 0, C.byref(ok_cfg)) == d._lib.ERR_INVALID
    assert raw(trk.match_batch_arrays(R, Cu)) == forward               # a rejected call leaves the frames untouched
    # a configuration that does not use level 0: nothing of level 0 is built at ingest, the match of the full pyramid still agrees
    coarse = d.Config(FirstLevel=levels - 1, LastLevel=1)
    d.update_raw_host_batch(R, gr, zr, role="reference", config=coarse)
    d.update_raw_host_batch(Cu, gc, zc, role="current", config=coarse)
    assert raw(trk.match_batch_arrays(R, Cu)) == forward


@pytest.mark.gpu
def test_strip_ingest_of_a_batch_that_only_needs_the_window_plane(gpu_ctx):
    """More current frames than the device has compute units: the role-aware ingest writes only the {I, Z} plane of the levels the
    window sweep reads (level 0 without neighbours, level 1 out of the same pass) -- ingest_strips.hip ROLE 0 / TAPS false and
    c_levels.  Same matches and same planes as frames built one by one the long way; the counter shows that the strips ran."""
    n, w, h, levels = 260, 128, 48, 2
    cfg = d.Config(FirstLevel=levels - 1, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    cam = d.RgbdCameraPyramid(w, h, po.FR1_K * (w / 640.0), gpu_ctx)
    cam.build(levels)
    b = datagen.synth_batch(303, 4, w, h)
    pick = lambda arrs, i: np.ascontiguousarray(arrs[i % 4] if i < 4 else np.roll(arrs[i % 4], i, axis=1))   # 260 distinct frames from 4 scenes
    gr, zr = [pick(b["grey_ref"], i) for i in range(n)], [pick(b["depth_ref"], i) for i in range(n)]
    gc, zc = [pick(b["grey_cur"], i) for i in range(n)], [pick(b["depth_cur"], i) for i in range(n)]
    refs = [cam.create_raw(gr[i], zr[i]) for i in range(n)]
    curs = [cam.create_raw(gc[i], zc[i]) for i in range(n)]
    want = trk.match_batch_arrays(refs, curs)
    dummy = np.zeros((h, w), np.uint8), np.full((h, w), 5000, np.uint16)
    R = [cam.create_raw(*dummy) for _ in range(n)]
    Cu = [cam.create_raw(*dummy) for _ in range(n)]
    before = gpu_ctx.counter("strip_ingests")
    d.update_raw_host_batch(R, gr, zr, role="reference", config=cfg)
    d.update_raw_host_batch(Cu, gc, zc, role="current", config=cfg)
    assert gpu_ctx.counter("strip_ingests") == before + 2 * n
    got = trk.match_batch_arrays(R, Cu)
    for k in ("T", "information", "loglik", "n_iterations", "entropy"):
        assert np.array_equal(want[k], got[k], equal_nan=True), k
    names = ("intensity", "depth", "intensity_dx", "intensity_dy", "depth_dx", "depth_dy")
    for i in (0, 5, n - 1):
        for a, c in ((refs[i], R[i]), (curs[i], Cu[i])):
            for l in range(levels):
                for k in names:
                    assert np.array_equal(np.array(getattr(a.level(l), k)), np.array(getattr(c.level(l), k)), equal_nan=True), (i, l, k)


@pytest.mark.gpu
def test_large_ragged_batch_equals_its_pairs(gpu_ctx):
    """603 pairs in one batch (frames shared between pairs, a batch size that divides nothing).  With the tile height of the launch
    path and the group size of the resident kernel pinned (options rows_per_wave, resident_group) a pair's record is bit-identical
    whatever else is in the launch: a batch of 603, of 77 in another
    order, of one.  With the default heuristic the tile height of a level follows the batch size, the per-tile partial sums group
    differently, and the records agree to rounding."""
    n_distinct, n = 9, 603
    w, h = 320, 240
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    cam = d.RgbdCameraPyramid(w, h, po.FR1_K * 0.5, gpu_ctx)
    cam.build(3)
    b = datagen.synth_batch(900, n_distinct, w, h)
    refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n_distinct)]
    curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n_distinct)]
    keys = ("T", "information", "loglik", "n_iterations", "entropy", "constraint_ratio")
    # pair j of the big batch = (refs[j % 9], curs[(j * 4) % 9]): also pairs that do not belong together (they just have to agree)
    pick_r = [j % n_distinct for j in range(n)]
    pick_c = [(j * 4) % n_distinct for j in range(n)]
    m = 77
    order = [(5 * j + 3) % n for j in range(m)]

    def run_all():
        big = trk.match_batch_arrays([refs[i] for i in pick_r], [curs[i] for i in pick_c])
        other = trk.match_batch_arrays([refs[pick_r[j]] for j in order], [curs[pick_c[j]] for j in order])
        singles = [trk.match_batch_arrays([refs[pick_r[j]]], [curs[pick_c[j]]]) for j in order[:6]]
        return big, other, singles
    try:
        gpu_ctx.set_option("rows_per_wave", 4)
        gpu_ctx.set_option("resident_group", 1)
        big, other, singles = run_all()
    finally:
        gpu_ctx.set_option("rows_per_wave", 0)
        gpu_ctx.set_option("resident_group", 0)
    def same(a, b, k, what):
        # the log-likelihood sweep groups its partial sums by batch-size class (inside the solver workgroup for full batches,
        # more loads in flight for small ones): that one number may differ in its last bits
        if k == "loglik":
            assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b)), what
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), what
    for slot, j in enumerate(order):
        for k in keys:
            same(big[k][j], other[k][slot], k, (j, k))
    for slot, j in enumerate(order[:6]):
        for k in keys:
            same(big[k][j], singles[slot][k][0], k, (j, k))
    first_seen = {}
    for j in range(n):          # equal pairs inside the batch got equal records
        key = (pick_r[j], pick_c[j])
        if key in first_seen:
            for k in keys:
                assert np.array_equal(np.asarray(big[k][j]), np.asarray(big[k][first_seen[key]]), equal_nan=True)
        else:
            first_seen[key] = j
    # default heuristic: the same answers to the precision of the stopping rule (a rounding difference may cost or save an iteration)
    big2, other2, singles2 = run_all()
    for slot, j in enumerate(order):
        assert np.abs(po.se3_log(np.linalg.inv(big2["T"][j]) @ other2["T"][slot])).max() < 5e-6
        assert abs(int(big2["n_iterations"][j]) - int(other2["n_iterations"][slot])) <= 2
    for slot, j in enumerate(order[:6]):
        assert np.abs(po.se3_log(np.linalg.inv(big2["T"][j]) @ singles2[slot]["T"][0])).max() < 5e-6
        assert np.abs(po.se3_log(np.linalg.inv(big2["T"][j]) @ big["T"][j])).max() < 5e-6


@pytest.mark.gpu
def test_one_context_per_host_thread(gpu_ctx):
    """The threading model of the boundary (one context per host thread, like one DenseTracker per TBB worker in
    dvo_slam/src/keyframe_graph.cpp:576-593): four threads align their own batches at the same time on one GPU, each through
    its own context, and get exactly what a single context gets alone."""
    import threading
    w, h, n = 320, 240, 12
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    K = po.FR1_K * 0.5
    batches = [datagen.synth_batch(1000 + t, n, w, h) for t in range(4)]

    def run(ctx, b, reps):
        cam = d.RgbdCameraPyramid(w, h, K, ctx)
        cam.build(3)
        trk = d.DenseTracker(cfg, ctx)
        out = None
        for _ in range(reps):
            refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
            curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
            out = trk.match_batch_arrays(refs, curs)
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations"))
    alone = [run(gpu_ctx, b, 1) for b in batches]
    assert len(set(alone)) == 4
    got, errors = [None] * 4, []

    def worker(t):
        try:
            got[t] = run(d.Context(0), batches[t], 5)
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == alone


@pytest.mark.gpu
def test_random_sizes_and_transforms_bit_exact(gpu_ctx):
    """twenty random image sizes (odd ones, tiny ones, wide and tall ones), levels and small transforms, first and later passes:
    valid count and residuals of the device sweep equal the oracle's MATH mode bit for bit."""
    rng = np.random.default_rng(2024)
    gpu_ctx.set_option("variant", EXACT_VARIANT)
    for case in range(20):
        w, h = int(rng.integers(24, 420)), int(rng.integers(20, 320))
        level = int(rng.integers(0, 2))
        if (w >> level) < 8 or (h >> level) < 8:
            level = 0
        pair = cm.synth(int(rng.integers(0, 10_000)), w, h)
        oref, ocur = cm.oracle_pyramids(pair, level + 1)
        gref, gcur = gpu_pyramids(gpu_ctx, pair, level + 1)
        trk = d.DenseTracker(d.Config(FirstLevel=level, LastLevel=level), gpu_ctx)
        T34 = po.se3_exp(rng.uniform(-0.05, 0.05, 6))[:3]
        o = po.level_iteration(oref, ocur, level, T34, first=True, mode=po.MATH, want_residuals=True)
        g = trk.level_iteration(gref, gcur, level, T34, first=True, want_residuals=True)
        assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"], (case, w, h, level)
        assert np.array_equal(np.isnan(g["residuals"]), np.isnan(o["residuals"])), (case, w, h, level)
        assert np.array_equal(np.nan_to_num(g["residuals"]), np.nan_to_num(o["residuals"])), (case, w, h, level)
        if o["n"] >= 6:
            assert np.abs(g["A"] - o["A"]).max() <= 1e-5 * np.abs(o["A"]).max()
            o2 = po.level_iteration(oref, ocur, level, T34, P_prev=o["P"], first=False, mode=po.MATH)
            g2 = trk.level_iteration(gref, gcur, level, T34, P_prev=o["P"], first=False)
            assert g2["n"] == o2["n"]
            assert abs(g2["neg_ll"] - o2["neg_ll"]) <= 1e-6 * abs(o2["neg_ll"])
            assert np.abs(g2["A"] - o2["A"]).max() <= 1e-5 * np.abs(o2["A"]).max()
    gpu_ctx.set_option("variant", DEFAULT_VARIANT)


@pytest.mark.gpu
def test_random_whole_matches_against_oracle(gpu_ctx):
    """twelve random sizes / level ranges / iteration caps / precisions / priors / initial guesses: every iteration record of
    the common prefix and the final transform agree with the oracle's MATH mode (see common.compare_runs for what may differ:
    a stopping decision at the float noise floor)."""
    rng = np.random.default_rng(777)
    for case in range(12):
        first = int(rng.integers(1, 4))
        last = int(rng.integers(0, first + 1))
        w = int(rng.integers(16, 60)) * (1 << first) + int(rng.integers(0, 1 << first))
        h = int(rng.integers(12, 44)) * (1 << first) + int(rng.integers(0, 1 << first))
        init = bool(rng.integers(0, 2))
        mu = float(rng.choice([0.0, 0.05, 0.5]))
        precision = float(rng.choice([5e-7, 1e-5, 1e-4]))
        max_iter = int(rng.integers(3, 60))
        pair = cm.synth(int(rng.integers(0, 10_000)), w, h)
        oref, ocur = cm.oracle_pyramids(pair, first + 1)
        gref, gcur = gpu_pyramids(gpu_ctx, pair, first + 1)
        cfg = d.Config(FirstLevel=first, LastLevel=last, Mu=mu, UseInitialEstimate=init, Precision=precision, MaxIterationsPerLevel=max_iter)
        T0 = po.se3_exp(float(rng.uniform(0.2, 1.5)) * pair["xi_true"]) if init else None
        g = run_gpu_match(gpu_ctx, gref, gcur, cfg, T0)
        o = po.match(oref, ocur, cm.oracle_config_from(cfg, po.MATH), T0)
        s = cm.compare_runs(g, o)
        what = (case, w, h, first, last, init, mu, precision, max_iter, s)
        assert s["n_mismatch"] == 0 and s["max_x_err"] < 5e-5, what
        assert s["max_iter_count_diff"] <= 2, what
        assert s["T_err"] < max(2e-5, 30 * precision), what
        if s["structure_mismatch"] == 0:
            # (a single pixel whose validity flips at an estimate 1e-7 apart weighs 1/n of the normal equations: the smallest case
            #  here, 61x68 at level 1, has 424 constraints)
            n_last = min(it["n"] for it in o["levels"][-1]["iterations"])
            assert np.abs(g["information"] - o["information"]).max() <= (2e-3 + 8.0 / max(n_last, 1)) * np.abs(o["information"]).max(), what


@pytest.mark.gpu
def test_config4_batch_of_1024_distinct_pairs(gpu_ctx):
    """BASELINE config 4 at size: 1024 DISTINCT 640x480 pairs (seeds 0..1023, 2048 frames, 41 GB of device planes) aligned as ONE
    batch, levels 3..0.  Every pair against the true motion of its synthetic scene; a sample of 32 against the oracle (MATH) and
    against the reference's own match() (oracle/_ref); and the batch equals eight 128-pair batches of the same pairs."""
    n, w, h = 1024, 640, 480
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    trk = d.DenseTracker(cfg, gpu_ctx)
    cam = d.RgbdCameraPyramid(w, h, po.FR1_K, gpu_ctx)
    cam.build(4)
    refs, curs, xi = [], [], []
    for s in range(0, n, 128):                                  # generated and ingested 128 pairs at a time (host memory)
        b = datagen.synth_batch(s, 128, w, h)
        refs += [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(128)]
        curs += [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(128)]
        xi.append(b["xi_true"])
    xi = np.concatenate(xi)
    try:
        gpu_ctx.set_option("rows_per_wave", 8)                  # pinned tile height and group size: records do not depend on the batch size
        gpu_ctx.set_option("resident_group", 1)
        out = trk.match_batch_arrays(refs, curs)
        parts = [trk.match_batch_arrays(refs[s:s + 128], curs[s:s + 128]) for s in range(0, n, 128)]
    finally:
        gpu_ctx.set_option("rows_per_wave", 0)
        gpu_ctx.set_option("resident_group", 0)
    assert np.isfinite(out["T"]).all() and np.isfinite(out["information"]).all()
    err = np.array([np.abs(po.se3_log(out["T"][i]) - xi[i]).max() for i in range(n)])
    print("1024 pairs: max / median distance to the true motion %.2e / %.2e, iterations per pair %.1f" % (err.max(), np.median(err), out["n_iterations"].mean()))
    assert err.max() < 3e-4 and np.median(err) < 5e-5          # 12 % holes, +-1.5 grey levels of noise, 0.2 mm depth quantisation
    for k in ("T", "information", "n_iterations", "entropy"):
        assert np.array_equal(out[k], np.concatenate([p[k] for p in parts]), equal_nan=True), k
    sample = list(range(0, n, 32))
    ocfg = po.make_config(3, 0, 100, 5e-7, mode=po.MATH)
    rcfg = po.make_config(3, 0, 100, 5e-7)
    worst_m = worst_r = 0.0
    have_ref = po.ref_lib() is not None
    for i in sample:
        pair = po.synth_pair(i, w, h)
        oref, ocur = po.pyramids_from_pair(pair, 4)
        o = po.match(oref, ocur, ocfg)
        worst_m = max(worst_m, cm.twist_matrix_error(out["T"][i], o["T"]))
        if have_ref:
            r = po.ref_match(pair["grey_ref"].astype(np.float32), po.convert_raw_depth(pair["depth_ref"]), pair["grey_cur"].astype(np.float32),
                             po.convert_raw_depth(pair["depth_cur"]), pair["K"], rcfg)
            worst_r = max(worst_r, cm.twist_matrix_error(out["T"][i], r["T"]))
    print("sample of %d: largest twist distance to the oracle (MATH) %.2e, to the reference's own match() %.2e" % (len(sample), worst_m, worst_r))
    assert worst_m < 2e-6
    assert worst_r < 5e-5


def test_deterministic_mode_records_do_not_depend_on_the_batch():
    """Option "deterministic": the record of a pair -- transform, information, log-likelihood, every iteration record -- is the same to
    the last bit whether the pair is aligned alone, among 6 others or among 299 others (three classes of tile height, resident plan and
    log-likelihood schedule in the default mode, whose records agree to the stopping rule's precision only)."""
    w, h = 320, 240
    ctx = d.Context(0)
    ctx.set_option("deterministic", 1)
    b = datagen.synth_batch(41, 12, w, h)
    cam = d.RgbdCameraPyramid(w, h, b["K"], ctx)
    cam.build(4)
    refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(12)]
    curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(12)]
    trk = d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx)

    def record(out, k):
        return b"".join(np.ascontiguousarray(out[key][k]).tobytes() for key in ("T", "information", "loglik", "n_iterations", "entropy"))
    alone = [record(trk.match_batch_arrays([refs[i]], [curs[i]]), 0) for i in range(12)]
    seven = trk.match_batch_arrays(refs[:7], curs[:7])
    assert [record(seven, i) for i in range(7)] == alone[:7]
    order = [(5 * i + 3) % 12 for i in range(300)]
    many = trk.match_batch_arrays([refs[i] for i in order], [curs[i] for i in order])
    assert all(record(many, k) == alone[i] for k, i in enumerate(order))
    # statistics as well (one pair, with and without company)
    r1 = d.Result()
    trk.match(refs[4], curs[4], r1)
    res = [d.Result() for _ in range(9)]
    trk.match_batch(refs[:9], curs[:9], res, with_stats=True)
    r2 = res[4]
    assert [len(L.Iterations) for L in r1.Statistics.Levels] == [len(L.Iterations) for L in r2.Statistics.Levels]
    for La, Lb in zip(r1.Statistics.Levels, r2.Statistics.Levels):
        for Ia, Ib in zip(La.Iterations, Lb.Iterations):
            assert Ia.ValidConstraints == Ib.ValidConstraints and Ia.TDistributionLogLikelihood == Ib.TDistributionLogLikelihood
            assert np.array_equal(Ia.EstimateIncrement, Ib.EstimateIncrement, equal_nan=True) and np.array_equal(Ia.EstimateInformation, Ib.EstimateInformation, equal_nan=True)
