"""GPU tier of option "ref_order" at its edges (ref_order.hip): ragged shapes, rank classes, the Q3 plane edit and the paths the option
enters.  tests/test_gpu_ref_order.py holds the kernels to the oracle on 640x480 and 320x240 pairs, where n is in the thousands; this file
forces the code of each kernel to its edges:

  k_ref_order_rows      lanes with no pixels (w < 64, w = 65), a ragged 8-load unroll (w = 1281), the 64-lane join;
  k_ref_order_combine   a ragged last thread (h = 257), R = 4 rows per thread (h = 960), the rank classes of the tail walk;
  k_ref_order_drop_last the scan back over many chunks, the first (partial) chunk, frames shared between pairs, rebuilt planes;
  run_batch / level_iteration under the option: the f16-range repeat, a mixed batch, one context over levels of different heights.

Every comparison goes through the C-ABI.  References: the oracle's target mode (QUIRKS | Q3 | Q7 | X_PAIRING_F64, + Q1 under
"ref_compat") for variant 7, whose residuals are bit-identical to the oracle's; common.rank_formula on the engine's own residual plane for
variant 8 (the default schedule).  Bounds are per entry: an entry (i, j) of cov or P is held to tol * sqrt(|X_ii X_jj|), not to the
largest entry, so an error in a small off-diagonal entry shows.
"""
import numpy as np
import pytest

import common as cm
import dvo_slam_amd as d
from oracle import pyoracle as po
from test_gpu_ref_order import check_against_oracle_and_reference, oracle_and_reference, rel_max

pytestmark = pytest.mark.gpu
TARGET = po.QUIRKS | po.Q_DROP_ODD | po.Q_LOGLIK_TAIL | po.X_PAIRING_F64
TARGET_COMPAT = TARGET | po.Q_RCP_PROJECTION | po.Q_RCP_WEIGHTS
RECORD_KEYS = ("T", "information", "loglik", "n_iterations")


def context(variant=8, ref_compat=0, ref_order=1, **options):
    ctx = d.Context(0)
    ctx.set_option("variant", variant)
    ctx.set_option("ref_compat", ref_compat)
    ctx.set_option("ref_order", ref_order)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def frames(ctx, pair, levels):
    h, w = pair["grey_ref"].shape
    cam = d.RgbdCameraPyramid(w, h, pair["K"], ctx)
    cam.build(levels)
    return cam.create_raw(pair["grey_ref"], pair["depth_ref"]), cam.create_raw(pair["grey_cur"], pair["depth_cur"])


def ty_pose(ty):
    return po.se3_exp(np.array([0.0, ty, 0.0, 0.0, 0.0, 0.0]))[:3]


def entry_err_cov(g, o):
    """max over the entries (00, 01, 11) of |g - o| / sqrt(|o_ii o_jj|)"""
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    scale = np.sqrt(np.abs([o[0] * o[0], o[0] * o[2], o[2] * o[2]]))
    return float((np.abs(g - o) / scale).max())


def entry_err_P(g, o):
    g, o = np.asarray(g, np.float64).reshape(2, 2), np.asarray(o, np.float64).reshape(2, 2)
    dg = np.abs(np.diag(o))
    return float((np.abs(g - o) / np.sqrt(np.outer(dg, dg))).max())


def records_equal(a, b, i=0, j=0):
    return all(np.array_equal(np.asarray(a[k][i]), np.asarray(b[k][j]), equal_nan=True) for k in RECORD_KEYS)


# ---- 2. shape matrix: one linearisation, first and weighted pass ----------------------------------------------------------------
# (w, h): the code path each one is chosen for
SHAPES = [
    (36, 20),       # w < 64: lanes 36 .. 63 of k_ref_order_rows own no pixel
    (63, 130),      # w < 64 on more rows than a block has wavefronts
    (65, 49),       # K = 2: lane 32 owns the last pixel, lanes 33 .. 63 none
    (1281, 13),     # K = 21: the 8-load unroll ends in a tail of 5
    (300, 257),     # h = 257: combine threads own 2 rows, thread 128 one, the rest none
    (640, 480),
    (1280, 960),    # R = 4 rows per combine thread (level 0 of BASELINE config 5's shape)
]


def _worst(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), value)


@pytest.mark.parametrize("w,h", SHAPES)
def test_shape_matrix_one_linearisation(w, h):
    """Level 0 of a (w, h) pair at ty = -0.01, first pass and a weighted pass.
    Variant 7 with and without "ref_compat" against the oracle's target mode: n exact, cov and P per entry within 1e-6, -ll within
    1e-6 relative, A and b within 1e-5 of their largest entry (the bounds of test_gpu_ref_order.py).  Variant 8 against the rank formula
    on its own residual plane: n exact, cov and P per entry 5e-7 on both passes, -ll 1e-6 relative.
    Measured worst cases over the seven shapes: variant 7 cov 1.9e-7, P 2.2e-7 (65x49), -ll 9.5e-8, A 3.1e-7, b 3.6e-7; variant 8 cov
    3.5e-8 (first pass) and 4.7e-8 (weighted pass), P 0, -ll 4.9e-8.  The variant-8 bounds were tightened from 1e-6 / 1e-5 (first /
    weighted) to 5e-7, about ten times the measured worst; the weighted pass needs no allowance for the formula's float32 weights."""
    pair = cm.synth(3, w, h)
    oref, ocur = cm.oracle_pyramids(pair, 1)
    T34 = ty_pose(-0.01)
    worst = {}
    for variant, compat in ((7, 0), (7, 1)):
        mode = TARGET_COMPAT if compat else TARGET
        ctx = context(variant, compat)
        gref, gcur = frames(ctx, pair, 1)
        trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
        o1 = po.level_iteration(oref, ocur, 0, T34, first=True, mode=mode)
        o2 = po.level_iteration(oref, ocur, 0, T34, P_prev=o1["P"], first=False, mode=mode)
        for o, P_prev, first in ((o1, None, True), (o2, o1["P"], False)):
            g = trk.level_iteration(gref, gcur, 0, T34, P_prev=P_prev, first=first)
            label = (w, h, variant, compat, first)
            assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"], label
            e = dict(cov=entry_err_cov(g["cov"], o["cov"]), P=entry_err_P(g["P"], o["P"]), ll=abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"]),
                     A=rel_max(g["A"], o["A"]), b=rel_max(g["b"], o["b"]))
            for k, v in e.items():
                _worst(worst, "v7 " + k, v)
            assert e["cov"] <= 1e-6 and e["P"] <= 1e-6 and e["ll"] <= 1e-6 and e["A"] <= 1e-5 and e["b"] <= 1e-5, (label, e)
    ctx = context(8, 0)
    gref, gcur = frames(ctx, pair, 1)
    trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
    g1 = trk.level_iteration(gref, gcur, 0, T34, first=True, want_residuals=True)
    g2 = trk.level_iteration(gref, gcur, 0, T34, P_prev=g1["P"], first=False, want_residuals=True)
    for g, P_prev, first, tol in ((g1, None, True, 5e-7), (g2, g1["P"], False, 5e-7)):
        f = cm.rank_formula(g["residuals"], P_prev, first)
        tag = "v8 first" if first else "v8 weighted"
        assert g["n"] == f["n"], (w, h, tag)
        e = dict(cov=entry_err_cov(g["cov"], f["cov"]), P=entry_err_P(g["P"], f["P"]), ll=abs(g["neg_ll"] - f["neg_ll"]) / abs(f["neg_ll"]))
        for k, v in e.items():
            _worst(worst, tag + " " + k, v)
        assert e["cov"] <= tol and e["P"] <= tol and e["ll"] <= 1e-6, (w, h, tag, e)
    print("%dx%d (n = %d): worst per-entry errors %s; bounds v7 1e-6 (A, b 1e-5), v8 5e-7, -ll 1e-6"
          % (w, h, g1["n"], {k: "%.1e" % v for k, v in sorted(worst.items())}))


# ---- 3. rank classes: the committed table (common.RANK_CLASS_TABLE), row by row against the oracle ------------------------------
@pytest.mark.parametrize("row", cm.RANK_CLASS_TABLE, ids=lambda r: "s%d_%dx%d_ty%g_i%g_d%g" % r[:6])
def test_rank_class_rows_against_the_oracle(row):
    """Every row of the table (tests/test_ref_order_classes.py checks each is in its classes): variant 7 against the oracle's target mode
    (first and weighted pass), variant 8 against the rank formula on its own residuals.  Where Q3 leaves n = 5 the level is abandoned: the
    whole match's records (levels, terminations, iteration counts, n, transform) equal the oracle's target match."""
    seed, w, h, ty, ithr, dthr, n_want, _ = row
    pair = cm.synth(seed, w, h)
    oref, ocur = cm.oracle_pyramids(pair, 1)
    T34 = ty_pose(ty)
    cfg = d.Config(FirstLevel=0, LastLevel=0, IntensityDerivativeThreshold=ithr, DepthDerivativeThreshold=dthr)
    ran = []
    ctx = context(7, 0)
    gref, gcur = frames(ctx, pair, 1)
    trk = d.DenseTracker(cfg, ctx)
    o1 = po.level_iteration(oref, ocur, 0, T34, first=True, mode=TARGET, ithr=ithr, dthr=dthr)
    assert o1["n"] == n_want
    passes = [(o1, None, True)]
    if o1["n"] >= 6:
        passes.append((po.level_iteration(oref, ocur, 0, T34, P_prev=o1["P"], first=False, mode=TARGET, ithr=ithr, dthr=dthr), o1["P"], False))
    for o, P_prev, first in passes:
        g = trk.level_iteration(gref, gcur, 0, T34, P_prev=P_prev, first=first)
        ran.append(g["n"])
        assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"], (row, first)
        if o["n"] >= 6:
            e = (entry_err_cov(g["cov"], o["cov"]), entry_err_P(g["P"], o["P"]), abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"]))
            assert max(e) <= 1e-6, (row, first, e)
    ctx8 = context(8, 0)
    gref8, gcur8 = frames(ctx8, pair, 1)
    trk8 = d.DenseTracker(cfg, ctx8)
    g = trk8.level_iteration(gref8, gcur8, 0, T34, first=True, want_residuals=True)
    f = cm.rank_formula(g["residuals"], None, True)
    ran.append(g["n"])
    assert g["n"] == f["n"]
    if f["n"] >= 6:
        e = (entry_err_cov(g["cov"], f["cov"]), entry_err_P(g["P"], f["P"]), abs(g["neg_ll"] - f["neg_ll"]) / abs(f["neg_ll"]))
        assert max(e) <= 1e-6, (row, e)
    if n_want < 6:
        mcfg = d.Config(FirstLevel=0, LastLevel=0, MaxIterationsPerLevel=20, IntensityDerivativeThreshold=ithr, DepthDerivativeThreshold=dthr)
        o = po.match(oref, ocur, cm.oracle_config_from(mcfg, TARGET))
        res = d.Result()
        d.DenseTracker(mcfg, ctx).match(gref, gcur, res)
        gm = cm.tracker_result_to_dict(res)
        assert len(gm["levels"]) == len(o["levels"]) == 1
        for Lg, Lo in zip(gm["levels"], o["levels"]):
            assert Lg["termination"] == Lo["termination"], (Lg["termination"], Lo["termination"])
            assert [it["n"] for it in Lg["iterations"]] == [it["n"] for it in Lo["iterations"]] == [5]
            assert Lg["valid_pixels"] == Lo["valid_pixels"]
        assert np.array_equal(gm["T"], o["T"]) and np.array_equal(gm["T"], np.eye(4))
    print("row %s: n ran %s" % (row[:6], ran))


# ---- 4. the Q3 plane edit --------------------------------------------------------------------------------------------------------
def _masked_pair(seed, w, h, zero_from_row):
    p = dict(cm.synth(seed, w, h))
    z = p["depth_ref"].copy()
    z[zero_from_row:] = 0
    p["depth_ref"] = z
    return p


@pytest.mark.parametrize("case", [
    # raw depth zero from row 320 of 480: the last selected pixel of level 0 lies 103055 pixels (100 chunks) before the plane's end
    dict(seed=2, zero_from=320, level=0, levels=1, ty=0.0, ithr=10.0, dthr=1e9),
    # zero from row 56: level 3 (80 x 60, chunks from the end: the first one holds pixels 0 .. 703) selects only pixels < 480
    dict(seed=1, zero_from=56, level=3, levels=4, ty=-0.01, ithr=0.0, dthr=0.0),
], ids=["far_before_the_end", "first_partial_chunk"])
def test_q3_edit_far_from_the_end_of_the_plane(case):
    """An odd selection whose last selected pixel is far from the end of the plane (k_ref_order_drop_last scans back chunk by chunk);
    the oracle confirms that Q3 takes a constraint away there.  Variant 7 against the oracle's target mode: n exact, first and
    weighted pass; the same on frames created afresh, bit for bit under "deterministic"."""
    pair = _masked_pair(case["seed"], 640, 480, case["zero_from"])
    level, ithr, dthr = case["level"], case["ithr"], case["dthr"]
    oref, ocur = cm.oracle_pyramids(pair, case["levels"])
    T34 = ty_pose(case["ty"])
    n_sel, mask = oref.select(level, ithr, dthr)
    last = int(np.flatnonzero(mask.reshape(-1))[-1])
    o1 = po.level_iteration(oref, ocur, level, T34, first=True, mode=TARGET, ithr=ithr, dthr=dthr)
    no_q3 = po.level_iteration(oref, ocur, level, T34, first=True, mode=TARGET & ~po.Q_DROP_ODD, ithr=ithr, dthr=dthr)
    assert n_sel % 2 == 1 and no_q3["n"] == o1["n"] + 1 and o1["n"] >= 6
    if level == 0:
        assert mask.size - 1 - last > 1024
    else:
        assert last < mask.size % 1024
    o2 = po.level_iteration(oref, ocur, level, T34, P_prev=o1["P"], first=False, mode=TARGET, ithr=ithr, dthr=dthr)
    cfg = d.Config(FirstLevel=level, LastLevel=level, IntensityDerivativeThreshold=ithr, DepthDerivativeThreshold=dthr)
    outs = []
    for _ in range(2):
        ctx = context(7, 0, deterministic=1)
        gref, gcur = frames(ctx, pair, case["levels"])
        trk = d.DenseTracker(cfg, ctx)
        got = []
        for o, P_prev, first in ((o1, None, True), (o2, o1["P"], False)):
            g = trk.level_iteration(gref, gcur, level, T34, P_prev=P_prev, first=first)
            assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"], (case, first)
            e = (entry_err_cov(g["cov"], o["cov"]), entry_err_P(g["P"], o["P"]), abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"]))
            assert max(e) <= 1e-6, (case, first, e)
            got.append(g)
        outs.append(got)
    for a, b in zip(*outs):
        for k in ("n", "cov", "P", "neg_ll", "A", "b"):
            assert np.array_equal(a[k], b[k]), k
    print("%s: n_selected %d, last selected pixel %d of %d, n %d" % (case, n_sel, last, mask.size, o1["n"]))


def _match(ctx, refs, curs, cfg):
    return d.DenseTracker(cfg, ctx).match_batch_arrays(refs, curs)


def _fresh_alone(pair_frames, cfg, **options):
    """every (reference, current) of `pair_frames` -- (pair, which-of-ref, pair, which-of-cur) -- on frames created afresh, alone"""
    out = []
    for (pr, sr), (pc, sc) in pair_frames:
        ctx = context(8, 1, 1, deterministic=1, **options)
        fr, fc = frames(ctx, pr, cfg.FirstLevel + 1), frames(ctx, pc, cfg.FirstLevel + 1)
        out.append(_match(ctx, [fr[sr]], [fc[sc]], cfg))
    return out


def _oracle_match(pr, sr, pc, sc, cfg):
    def pyr(p, s):
        g, z = (p["grey_ref"], p["depth_ref"]) if s == 0 else (p["grey_cur"], p["depth_cur"])
        return po.Pyramid(g.astype(np.float32), po.convert_raw_depth(z), p["K"], cfg.FirstLevel + 1)
    return po.match(pyr(pr, sr), pyr(pc, sc), cm.oracle_config_from(cfg, TARGET_COMPAT))


def _assert_near_oracle(g, i, o, label):
    e = (rel_max(g["information"][i], o["information"]), abs(g["loglik"][i] - o["loglik"]) / abs(o["loglik"]), cm.twist_matrix_error(g["T"][i], o["T"]))
    print("%s: engine-oracle I %.2e LL %.2e twist %.2e" % ((label,) + e))
    assert e[0] <= 2e-3 and e[1] <= 5e-5 and e[2] <= 5e-7, (label, e)


CFG3 = d.Config(FirstLevel=2, LastLevel=0, MaxIterationsPerLevel=100, Precision=5e-7)


def _odd_levels(pair, which):
    o = cm.oracle_pyramids(pair, 3)[which]
    return [o.select(l)[0] % 2 for l in range(3)]


def test_q3_reference_frame_shared_by_two_pairs():
    """One reference frame (odd selections on levels 0 and 1) aligned against two currents in one batch: Q3 edits its planes once,
    each record equals the pair alone on fresh frames bit for bit ("deterministic") and the oracle's target match."""
    a, b = cm.synth(107, 320, 240), cm.synth(101, 320, 240)
    assert _odd_levels(a, 0)[:2] == [1, 1]
    ctx = context(8, 1, 1, deterministic=1)
    ra, ca = frames(ctx, a, 3)
    _, cb = frames(ctx, b, 3)
    got = _match(ctx, [ra, ra], [ca, cb], CFG3)
    alone = _fresh_alone([((a, 0), (a, 1)), ((a, 0), (b, 1))], CFG3)
    for i in range(2):
        assert records_equal(got, alone[i], i, 0), i
    again = _match(ctx, [ra, ra], [ca, cb], CFG3)                 # the edited planes are not edited again
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in RECORD_KEYS)
    _assert_near_oracle(got, 0, _oracle_match(a, 0, a, 1, CFG3), "shared reference, pair 0")


def test_q3_frame_is_reference_and_current():
    """The current frame of pair 0 is the reference of pair 1 (and the reverse): the edit of its reference planes does not reach the
    planes it is read from as a current frame.  Records equal each pair alone on fresh frames bit for bit and the oracle's target match."""
    p = cm.synth(101, 320, 240)
    assert _odd_levels(p, 1) == [1, 1, 1] and _odd_levels(p, 0)[:2] == [1, 1]
    ctx = context(8, 1, 1, deterministic=1)
    r, c = frames(ctx, p, 3)
    got = _match(ctx, [r, c], [c, r], CFG3)
    alone = _fresh_alone([((p, 0), (p, 1)), ((p, 1), (p, 0))], CFG3)
    for i in range(2):
        assert records_equal(got, alone[i], i, 0), i
    _assert_near_oracle(got, 0, _oracle_match(p, 0, p, 1, CFG3), "forward")
    _assert_near_oracle(got, 1, _oracle_match(p, 1, p, 0, CFG3), "backward")


def test_q3_threshold_change_rebuilds_and_edits_once():
    """Two "ref_order" matches of the same frames with different selection thresholds, then the first thresholds again: every plane is
    rebuilt and edited once (no pixel of the old plane is put back onto the new one) -- each record equals fresh frames' bit for bit."""
    p = cm.synth(107, 320, 240)
    ctx = context(8, 1, 1, deterministic=1)
    r, c = frames(ctx, p, 3)
    cfg_b = d.Config(FirstLevel=2, LastLevel=0, IntensityDerivativeThreshold=20.0, DepthDerivativeThreshold=1e9)
    oref, _ = cm.oracle_pyramids(p, 3)
    assert any(oref.select(l, 20.0, 1e9)[0] % 2 for l in range(3)) and any(oref.select(l)[0] % 2 for l in range(3))
    seq = [CFG3, cfg_b, CFG3]
    for cfg in seq:
        got = _match(ctx, [r], [c], cfg)
        fresh = _fresh_alone([((p, 0), (p, 1))], cfg)[0]
        assert records_equal(got, fresh), (cfg.IntensityDerivativeThreshold,)
    _assert_near_oracle(got, 0, _oracle_match(p, 0, p, 1, CFG3), "thresholds 0 -> 20 -> 0")


# ---- 5. paths entered under the option -------------------------------------------------------------------------------------------
def _checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // 8) + (yy // 8)) % 2 == 0, 0.002, 10.0).astype(np.float32)


@pytest.mark.parametrize("variant", [7, 8])
def test_f16_range_repeat_single_linearisation(variant):
    """The checkerboard scene of test_f16_gram_range_guard_repeats_with_the_f32_gram: one linearisation repeats with the f32 Gram, and
    the repeat carries the ref_order passes -- n exact, cov and P per entry 1e-6 against the oracle's target mode.  -ll: 1e-6 relative
    plus what the precision of det P explains.  On this scene -ll (296) is what is left of n/2 log det P (~1.3e4) less the weighted sum,
    so the reference's float det P (the oracle's Q7 path) and the engine's float64 one lie 1.2e-6 of -ll apart (measured 1.24e-6 on
    variants 7 and 8, with cov and P bit-identical to the oracle's)."""
    w, h = 128, 96
    pair = cm.synth(4, w, h)
    grey, depth = pair["grey_ref"].astype(np.float32), _checker(w, h)
    oref, ocur = po.Pyramid(grey, depth, pair["K"], 1), po.Pyramid(grey, depth, pair["K"], 1)
    ctx = context(variant, 0)
    cam = d.RgbdCameraPyramid(w, h, pair["K"], ctx)
    cam.build(1)
    gref, gcur = cam.create(grey, depth), cam.create(grey, depth)
    trk = d.DenseTracker(d.Config(FirstLevel=0, LastLevel=0), ctx)
    T34 = ty_pose(-0.001)
    before = ctx.counter("f16_range_repeats")
    g = trk.level_iteration(gref, gcur, 0, T34, first=True)
    assert ctx.counter("f16_range_repeats") == before + 1
    o = po.level_iteration(oref, ocur, 0, T34, first=True, mode=TARGET)
    assert g["n"] == o["n"] and o["n"] >= 6
    e = (entry_err_cov(g["cov"], o["cov"]), entry_err_P(g["P"], o["P"]), abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"]))
    P = np.asarray(o["P"], np.float32)
    det32 = float(P[0, 0] * P[1, 1] - P[0, 1] * P[1, 0])
    det64 = float(P[0, 0]) * float(P[1, 1]) - float(P[0, 1]) * float(P[1, 0])
    ll_tol = 1e-6 + 0.5 * o["n"] * abs(np.log(det32) - np.log(det64)) / abs(o["neg_ll"])
    print("variant %d, f16-range repeat of one linearisation: n %d, errors cov %.1e P %.1e -ll %.2e (bound %.2e)" % ((variant, g["n"]) + e + (ll_tol,)))
    assert e[0] <= 1e-6 and e[1] <= 1e-6 and e[2] <= ll_tol, e


@pytest.mark.parametrize("n_pairs", [8, 2], ids=["fewer_than_half_flagged", "half_flagged"])
def test_f16_range_repeat_batch(n_pairs):
    """A batch whose pair `bad` carries the checkerboard: with 8 pairs only that pair runs again (a batch of its own), with 2 the whole
    batch does.  The counter shows the repeat; the repeated pair's first iteration has the oracle's n, precision (per entry 1e-6) and
    -ll (1e-6 relative), and its Information and LogLikelihood are within test_gpu_ref_order.py's bounds of the oracle's target match."""
    w, h, bad = 128, 96, 1
    from dvo_slam_amd import datagen
    b = datagen.synth_batch(11, n_pairs, w, h)
    step = _checker(w, h)
    cfg = d.Config(FirstLevel=0, LastLevel=0, MaxIterationsPerLevel=3)
    ctx = context(8, 0)
    cam = d.RgbdCameraPyramid(w, h, b["K"], ctx)
    cam.build(1)
    planes, refs, curs = [], [], []
    for i in range(n_pairs):
        g_r, g_c = b["grey_ref"][i].astype(np.float32), b["grey_cur"][i].astype(np.float32)
        z_r, z_c = po.convert_raw_depth(b["depth_ref"][i]), po.convert_raw_depth(b["depth_cur"][i])
        if i == bad:
            g_c, z_r, z_c = g_r, step, step
        planes.append((g_r, z_r, g_c, z_c))
        refs.append(cam.create(g_r, z_r))
        curs.append(cam.create(g_c, z_c))
    res = [d.Result() for _ in range(n_pairs)]
    before = ctx.counter("f16_range_repeats")
    d.DenseTracker(cfg, ctx).match_batch(refs, curs, res, with_stats=True)
    assert ctx.counter("f16_range_repeats") == before + 1
    g_r, z_r, g_c, z_c = planes[bad]
    o = po.match(po.Pyramid(g_r, z_r, b["K"], 1), po.Pyramid(g_c, z_c, b["K"], 1), cm.oracle_config_from(cfg, TARGET))
    gi, oi = res[bad].Statistics.Levels[0].Iterations[0], o["levels"][0]["iterations"][0]
    assert gi.ValidConstraints == oi["n"] and oi["n"] >= 6
    e = (entry_err_P(gi.TDistributionPrecision, oi["precision"]), abs(gi.TDistributionLogLikelihood - oi["neg_ll"]) / abs(oi["neg_ll"]))
    assert max(e) <= 1e-6, e
    I, LL = rel_max(res[bad].Information, o["information"]), abs(res[bad].LogLikelihood - o["loglik"]) / abs(o["loglik"])
    print("%d pairs, pair %d repeated: first iteration n %d, P %.1e, -ll %.1e; Information %.1e LogLikelihood %.1e" % ((n_pairs, bad, oi["n"]) + e + (I, LL)))
    assert I <= 2e-3 and LL <= 5e-5, (I, LL)


def test_mixed_batch_abandoned_and_early_pairs_equal_alone():
    """One 65x49 batch under "deterministic" with the selection of test_rank_class_rows' n = 5 row: a pair whose level is abandoned (Q3
    leaves 5 constraints), one whose current equals its reference (converges on its first step), and ordinary ones.  Every pair's record
    equals the same pair run alone."""
    w, h, ithr, dthr = 65, 49, 70.0, 1e9
    cfg = d.Config(FirstLevel=0, LastLevel=0, MaxIterationsPerLevel=20, IntensityDerivativeThreshold=ithr, DepthDerivativeThreshold=dthr)
    seeds = [0, 6, 1, 0, 5]
    ctx = context(8, 0, 1, deterministic=1)
    fr = [frames(ctx, cm.synth(s, w, h), 1) for s in seeds]
    refs = [f[0] for f in fr]
    curs = [f[1] for f in fr]
    curs[3] = refs[3]                                          # the early pair: its current is its reference
    res = [d.Result() for _ in seeds]
    d.DenseTracker(cfg, ctx).match_batch(refs, curs, res, with_stats=True)
    terms = [r.Statistics.Levels[0].TerminationCriterion for r in res]
    iters = [len(r.Statistics.Levels[0].Iterations) for r in res]
    print("mixed batch: terminations %s, iterations %s" % (terms, iters))
    assert res[1].Statistics.Levels[0].Iterations[-1].ValidConstraints == 5
    assert iters[3] == 1 and res[3].Statistics.Levels[0].Iterations[0].ValidConstraints >= 6 and iters[0] > 1
    batch = dict(T=[r.Transformation for r in res], information=[r.Information for r in res], loglik=[r.LogLikelihood for r in res],
                 n_iterations=iters)
    for i in range(len(seeds)):
        one = d.Result()
        d.DenseTracker(cfg, ctx).match_batch([refs[i]], [curs[i]], [one], with_stats=True)
        alone = dict(T=[one.Transformation], information=[one.Information], loglik=[one.LogLikelihood],
                     n_iterations=[len(one.Statistics.Levels[0].Iterations)])
        assert records_equal(batch, alone, i, 0), i


def test_one_context_small_large_small():
    """One context aligns a 65x49 pair, a 1280x960 pair (levels 4 .. 0: the rows' records of 960 rows) and the 65x49 pair again; every
    record equals a fresh context's bit for bit ("deterministic")."""
    small, large = cm.synth(3, 65, 49), cm.synth(5, 1280, 960)
    cfg_s = d.Config(FirstLevel=0, LastLevel=0)
    cfg_l = d.Config(FirstLevel=4, LastLevel=0)
    ctx = context(8, 1, 1, deterministic=1)
    seq = []
    for p, cfg, levels in ((small, cfg_s, 1), (large, cfg_l, 5), (small, cfg_s, 1)):
        r, c = frames(ctx, p, levels)
        got = _match(ctx, [r], [c], cfg)
        fctx = context(8, 1, 1, deterministic=1)
        fr, fc = frames(fctx, p, levels)
        assert records_equal(got, _match(fctx, [fr], [fc], cfg))
        seq.append(got)
    assert records_equal(seq[0], seq[2])


# ---- 6. a whole match at 1280x960 ------------------------------------------------------------------------------------------------
def test_whole_match_1280x960_levels_4_to_0():
    """BASELINE config 5's shape, "ref_compat" + "ref_order" on the default schedule, levels 4 .. 0, against the oracle's target match
    and the reference's own match() with the bounds of check_against_oracle_and_reference."""
    if po.ref_lib() is None:
        pytest.skip("oracle/_ref is not built")
    pair = cm.synth(1234, 1280, 960)
    cfg = d.Config(FirstLevel=4, LastLevel=0, MaxIterationsPerLevel=100, Precision=5e-7)
    o, r = oracle_and_reference(pair, cfg)
    ctx = context(8, 1, 1)
    gref, gcur = frames(ctx, pair, 5)
    g = d.DenseTracker(cfg, ctx).match_batch_arrays([gref], [gcur])
    check_against_oracle_and_reference((g["information"][0], g["loglik"][0], g["T"][0]), o, r, "1280x960 levels 4..0")
