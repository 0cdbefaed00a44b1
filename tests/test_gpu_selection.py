"""GPU tier of the caller selection of reference points (include/dvo_hip.h, dvo_hip_frames_set_selection /
dvo_hip_frame_set_level_selection; the apply pass k_apply_selection, pyramid_kernels.hip).

  no-op selections (an all-ones mask, the range [0, inf)) and explicit selections equal to the thresholds' own give records bit-identical
      to the frames without one: a single match (resident path), 64- and 256-pair batches (launch chain), variants 7 and 8, ref_order
  counts and masks of dvo_hip_frame_select against oracle_pyramid_select & mask0[::2^l, ::2^l] & range(oracle depth), every level
  one linearisation under variant 7: the oracle's unmasked residuals at the selected pixels, NaN elsewhere; n, the scale, the precision
      and -ll against a numpy restatement over those residuals
  what it is for: a box that moves on its own, masked in the reference, no longer pulls the estimate away from the camera's motion
  every path sees the same selection: single match, batches, the fused reference-role ingest (keep_raw_copy 0 and 1), deterministic
  invalidation: mask A then B equals a fresh frame with B, clear equals none, a re-ingest keeps it, a speculative prepare honours it
"""
import ctypes as C

import numpy as np
import pytest

import common as cm
import dvo_slam_amd as d
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
W, H, LEVELS = 640, 480, 4


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch's runtime is set up before the module's first context (the tests hand torch tensors' device addresses over)"""
    import torch
    torch.cuda.init()


def context(variant=8, **options):
    ctx = d.Context(0)
    ctx.set_option("variant", variant)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def pyramids(ctx, seeds, w=W, h=H):
    """reference and current pyramids of synthetic pairs, one pair per seed"""
    cam = d.RgbdCameraPyramid(w, h, cm.synth(seeds[0], w, h)["K"], ctx)
    cam.build(LEVELS)
    refs, curs = [], []
    for s in seeds:
        p = cm.synth(s, w, h)
        refs.append(cam.create_raw(p["grey_ref"], p["depth_ref"]))
        curs.append(cam.create_raw(p["grey_cur"], p["depth_cur"]))
    return cam, refs, curs


def records(ctx, refs, curs, cfg=None):
    """every field of every pair's record, for exact comparison"""
    tr = d.DenseTracker(cfg or d.Config(), ctx)
    res = [d.Result() for _ in refs]
    tr.match_batch(refs, curs, res, with_stats=True)
    return [cm.tracker_result_to_dict(r) for r in res]


def flatten(rec):
    out = [rec["T"], rec["information"], rec["loglik"]]
    for L in rec["levels"]:
        out += [L["id"], L["max_valid_pixels"], L["valid_pixels"], L["termination"]]
        for it in L["iterations"]:
            out += [it["n"], it["neg_ll"], it["precision"], it["prior_ll"], it["x"], it["A"]]
    return out


def assert_identical(a, b, what):
    assert len(a) == len(b)
    for i, (ra, rb) in enumerate(zip(a, b)):
        fa, fb = flatten(ra), flatten(rb)
        assert len(fa) == len(fb), (what, i, "structure")
        for k, (x, y) in enumerate(zip(fa, fb)):
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (what, i, k, x, y)


def masks_of(kind, seed=0, w=W, h=H):
    rng = np.random.default_rng(seed)
    if kind == "ones":
        return np.ones((h, w), np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "noise":
        return (rng.random((h, w)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    if kind == "stripes":
        m = np.zeros((h, w), np.uint8)
        m[:, (np.arange(w) // 7) % 2 == 0] = 1
        return m
    if kind == "blocks":
        m = np.ones((h, w), np.uint8)
        for _ in range(6):
            x0, y0 = rng.integers(0, w - 40), rng.integers(0, h - 40)
            m[y0:y0 + rng.integers(10, h // 2), x0:x0 + rng.integers(10, w // 2)] = 0
        return m
    raise ValueError(kind)


# ---- 1 / 2: selections that select what the thresholds select are exact ----------------------------------------------------------

@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("n_pairs", [1, 64, 256])
def test_noop_selection_is_exact(variant, n_pairs):
    ctx = context(variant)
    seeds = [11 + (i % 8) for i in range(n_pairs)]
    _, refs, curs = pyramids(ctx, seeds)
    plain = records(ctx, refs, curs)
    d.set_selection_batch(refs, [masks_of("ones")] * n_pairs, 0.0, float("inf"))
    assert_identical(records(ctx, refs, curs), plain, "all-ones mask")
    d.set_selection_batch(refs, None, 0.0, float("inf"))
    assert_identical(records(ctx, refs, curs), plain, "range [0, inf)")
    _, refs2, curs2 = pyramids(ctx, seeds)                          # a fresh set whose selection is set before its first match
    d.set_selection_batch(refs2, [masks_of("ones")] * n_pairs, 0.0, float("inf"))
    assert_identical(records(ctx, refs2, curs2), plain, "all-ones mask on fresh frames")


@pytest.mark.parametrize("n_pairs", [1, 32])
def test_noop_selection_is_exact_under_ref_order(n_pairs):
    ctx = context(7, ref_order=1)
    seeds = [21 + i for i in range(n_pairs)]
    _, refs, curs = pyramids(ctx, seeds)
    plain = records(ctx, refs, curs)
    d.set_selection_batch(refs, [masks_of("ones")] * n_pairs, 0.0, float("inf"))
    assert_identical(records(ctx, refs, curs), plain, "all-ones mask, ref_order")


@pytest.mark.parametrize("variant", [7, 8])
def test_explicit_selection_equal_to_the_thresholds_is_exact(variant):
    ctx = context(variant)
    seeds = [31, 32, 33]
    cfg = d.Config(IntensityDerivativeThreshold=2.0, DepthDerivativeThreshold=0.01)
    _, refs, curs = pyramids(ctx, seeds)
    plain = records(ctx, refs, curs, cfg)
    for r in refs:
        sel = d.PointSelection(r, cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold)
        for l in range(cfg.LastLevel, cfg.FirstLevel + 1):
            n, m = sel.select(l, want_mask=True)
            assert n == int(m.sum())
            d.set_level_selection(r, l, m)
    assert_identical(records(ctx, refs, curs, cfg), plain, "explicit = thresholds")
    # an explicit set holds whatever thresholds a match asks for
    a = records(ctx, refs, curs, d.Config())
    assert_identical(a, plain, "explicit set under other thresholds")


# ---- 3: counts and masks against numpy ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(640, 480), (322, 242)])
def test_counts_and_masks_against_the_oracle(shape):
    w, h = shape
    ctx = context(8)
    pair = cm.synth(41, w, h)
    oref, _ = cm.oracle_pyramids(pair, LEVELS)
    _, refs, _ = pyramids(ctx, [41], w, h)
    ref = refs[0]
    for ithr, dthr in ((0.0, 0.0), (4.0, 0.02)):
        sel = d.PointSelection(ref, ithr, dthr)
        for kind, seed in (("blocks", 1), ("stripes", 2), ("noise", 3), ("zeros", 4), ("ones", 5), (None, 6)):
            for zmin, zmax in ((0.0, float("inf")), (1.0, 2.5), (0.0, 1.8), (2.0, float("inf"))):
                mask0 = masks_of(kind, seed, w, h) if kind else None
                ref.set_selection(mask0, zmin, zmax)
                for l in range(LEVELS):
                    n_o, m_o = oref.select(l, ithr, dthr)
                    z, _ = oref.plane(l, 1)
                    hl, wl = m_o.shape
                    want = m_o != 0
                    if mask0 is not None:
                        want &= mask0[::2 ** l, ::2 ** l][:hl, :wl] != 0
                    if zmin > 0 or np.isfinite(zmax):
                        with np.errstate(invalid="ignore"):
                            want &= (z >= zmin) & (z <= zmax)
                    n, m = sel.select(l, want_mask=True)
                    assert np.array_equal(m != 0, want), (kind, zmin, zmax, l, ithr, int((m != 0).sum()), int(want.sum()))
                    assert n == int(want.sum()), (kind, zmin, zmax, l, ithr)
                    n_only = sel.select(l)                           # the count alone (the cached plane, no mask recomputation)
                    assert n_only == n
    ref.clear_selection()
    n_o, _ = oref.select(0)
    assert d.PointSelection(ref).select(0) == n_o


# ---- 4: one linearisation against the oracle ---------------------------------------------------------------------------------------

def test_linearisation_with_a_mask_against_the_oracle():
    ctx = context(7)
    pair = cm.synth(51, W, H)
    oref, ocur = cm.oracle_pyramids(pair, LEVELS)
    _, refs, curs = pyramids(ctx, [51])
    mask0 = masks_of("blocks", 9)
    refs[0].set_selection(mask0, 0.5, 3.0)
    tr = d.DenseTracker(d.Config(), ctx)
    T34 = np.eye(4, dtype=np.float32)[:3]
    T34[1, 3] = -0.01
    for l in range(LEVELS):
        g = tr.level_iteration(refs[0], curs[0], l, T34, want_residuals=True)
        o = po.level_iteration(oref, ocur, l, T34, mode=po.MATH, want_residuals=True)
        n_sel, m = d.PointSelection(refs[0]).select(l, want_mask=True)
        assert g["n_selected"] == n_sel
        sel = m != 0
        ro, rg = o["residuals"], g["residuals"]
        assert np.array_equal(rg[sel], ro[sel], equal_nan=True), l
        assert np.isnan(rg[~sel]).all(), l
        valid = sel & np.isfinite(ro).all(axis=2)
        assert g["n"] == int(valid.sum()), (l, g["n"], int(valid.sum()))
        # the scale, its inverse and -ll from the selected residuals, at the parity tolerances of tests/test_gpu_parity.py; then the
        # weighted pass at that precision
        n, cov, P, ll = restate_scale(rg, None, True)
        assert n == g["n"]
        assert np.abs(g["cov"] - cov).max() <= 1e-5 * np.abs(cov).max(), l
        assert np.abs(g["P"] - P).max() <= 1e-5 * np.abs(P).max(), l
        assert abs(g["neg_ll"] - ll) <= 1e-6 * abs(ll), l
        g2 = tr.level_iteration(refs[0], curs[0], l, T34, P_prev=g["P"], first=False, want_residuals=True)
        n2, cov2, P2, ll2 = restate_scale(g2["residuals"], g["P"], False)
        assert n2 == g2["n"] == n
        assert np.abs(g2["cov"] - cov2).max() <= 1e-5 * np.abs(cov2).max(), l
        assert np.abs(g2["P"] - P2).max() <= 1e-5 * np.abs(P2).max(), l
        assert abs(g2["neg_ll"] - ll2) <= 1e-6 * abs(ll2), l


def restate_scale(res, P_prev, first):
    """n, scale_cov (00, 01, 11), precision and -ll of one pass from its residual plane (NaN: no constraint), in float64: weights 1 on
    a first pass, else float32 7 / (5 + r^T P_prev r); cov = sum w r r^T / (n - 3); P the float32 inverse of its float32 rounding;
    -ll = -(n/2 log det P - 7/2 sum log(1 + r^T P r / 5)).  (Equals the oracle's MATH mode to 5e-8 on the unmasked planes.)"""
    r32 = np.asarray(res, np.float32).reshape(-1, 2)
    r32 = r32[~np.isnan(r32).any(axis=1)]
    r = r32.astype(np.float64)
    n = len(r)
    w = np.ones(n) if first else (np.float32(7.0) / (np.float32(5.0) + cm.mahalanobis_f32(r32, P_prev))).astype(np.float64)
    cov = np.array([(w * r[:, 0] * r[:, 0]).sum(), (w * r[:, 0] * r[:, 1]).sum(), (w * r[:, 1] * r[:, 1]).sum()]) / (n - 3)
    C32 = cov.astype(np.float32)
    inv = np.float32(1.0) / (C32[0] * C32[2] - C32[1] * C32[1])
    P = np.array([[C32[2] * inv, -C32[1] * inv], [-C32[1] * inv, C32[0] * inv]], np.float32)
    q = cm.mahalanobis_f32(r32, P).astype(np.float64)
    detP = float(P[0, 0] * P[1, 1] - P[0, 1] * P[1, 0])
    return n, cov, P, -(0.5 * n * np.log(detP) - 3.5 * np.log1p(0.2 * q).sum())


# ---- 5: every path sees the same selection -----------------------------------------------------------------------------------------

def _masked_set(ctx, seeds):
    _, refs, curs = pyramids(ctx, seeds)
    d.set_selection_batch(refs, [masks_of("blocks", s) for s in seeds], 0.3, 4.0)
    return refs, curs


def test_every_path_sees_the_same_selection_deterministic():
    ctx = context(8, deterministic=1)
    seeds = [61 + i for i in range(16)]
    refs, curs = _masked_set(ctx, seeds)
    batch = records(ctx, refs, curs)
    small = records(ctx, refs[:4], curs[:4])
    single = [records(ctx, [r], [c])[0] for r, c in zip(refs[:3], curs[:3])]
    assert_identical(small, batch[:4], "4-pair batch vs 16")
    assert_identical(single, batch[:3], "single vs batch")
    unmasked = records(ctx, *pyramids(ctx, seeds)[1:])
    fewer = 0
    for r, a, b in zip(refs, batch, unmasked):
        for La, Lb in zip(a["levels"], b["levels"]):
            assert La["valid_pixels"] == d.PointSelection(r).select(La["id"]), La["id"]   # what dvo_hip_frame_select reports
            assert La["valid_pixels"] <= Lb["valid_pixels"]
            fewer += La["valid_pixels"] < Lb["valid_pixels"]
    assert fewer > len(seeds), fewer


@pytest.mark.parametrize("keep_raw_copy", [1, 0])
def test_fused_reference_ingest_sees_the_selection(keep_raw_copy):
    import torch
    ctx = context(8, deterministic=1)
    seeds = [71 + i for i in range(8)]
    refs, curs = _masked_set(ctx, seeds)
    want = records(ctx, refs, curs)
    cam, refs2, curs2 = pyramids(ctx, seeds)
    d.set_selection_batch(refs2, [masks_of("blocks", s) for s in seeds], 0.3, 4.0)   # set before the update
    ps = [cm.synth(s, W, H) for s in seeds]
    grey = [torch.from_numpy(p["grey_ref"]).cuda() for p in ps]
    depth = [torch.from_numpy(p["depth_ref"].astype(np.int16)).cuda() for p in ps]
    torch.cuda.synchronize()
    ctx.set_option("keep_raw_copy", keep_raw_copy)
    d.update_raw_device_batch(refs2, [g.data_ptr() for g in grey], [z.data_ptr() for z in depth], role="reference", config=d.Config())
    got = records(ctx, refs2, curs2)
    ctx.set_option("keep_raw_copy", 1)
    assert_identical(got, want, "fused reference ingest, keep_raw_copy %d" % keep_raw_copy)


def test_batches_agree_with_single_matches_to_the_stopping_rule():
    ctx = context(8)
    seeds = [81 + (i % 8) for i in range(64)]
    refs, curs = _masked_set(ctx, seeds)
    batch = records(ctx, refs, curs)
    for i in (0, 5):
        one = records(ctx, [refs[i]], [curs[i]])[0]
        s = cm.compare_runs(one, batch[i])
        assert s["T_err"] < 1e-6 and s["structure_mismatch"] <= 1, s


# ---- 6: invalidation -------------------------------------------------------------------------------------------------------------

def test_invalidation_replace_clear_reingest_and_speculative_prepare():
    import torch
    ctx = context(8, deterministic=1)
    seeds = [91, 92]
    A, B = masks_of("blocks", 1), masks_of("stripes", 2)
    _, refs, curs = pyramids(ctx, seeds)
    plain = records(ctx, refs, curs)
    _, fresh_b, fcurs = pyramids(ctx, seeds)
    d.set_selection_batch(fresh_b, [B, B], 0.0, 3.0)
    want_b = records(ctx, fresh_b, fcurs)

    d.set_selection_batch(refs, [A, A], 0.5, float("inf"))
    with_a = records(ctx, refs, curs)
    assert with_a[0]["levels"][-1]["valid_pixels"] != want_b[0]["levels"][-1]["valid_pixels"]
    d.set_selection_batch(refs, [B, B], 0.0, 3.0)
    assert_identical(records(ctx, refs, curs), want_b, "A then B")
    d.clear_selection_batch(refs)
    assert_identical(records(ctx, refs, curs), plain, "cleared")

    # the selection persists across a re-ingest of the frame's pixels
    d.set_selection_batch(refs, [B, B], 0.0, 3.0)
    ps = [cm.synth(s, W, H) for s in seeds]
    grey = [torch.from_numpy(p["grey_ref"]).cuda() for p in ps]
    depth = [torch.from_numpy(p["depth_ref"].astype(np.int16)).cuda() for p in ps]
    torch.cuda.synchronize()
    d.update_raw_device_batch(refs, [g.data_ptr() for g in grey], [z.data_ptr() for z in depth])
    assert_identical(records(ctx, refs, curs), want_b, "after a re-ingest")

    # a speculative prepare (negative thresholds) made under mask B leaves no stale selection once A replaces it
    cfg = d.Config()
    spec = d.Config(IntensityDerivativeThreshold=-1.0, DepthDerivativeThreshold=-1.0)
    d.update_raw_device_batch(refs, [g.data_ptr() for g in grey], [z.data_ptr() for z in depth])
    d.prepare_roles_batch(refs, "reference", spec)
    d.set_selection_batch(refs, [A, A], 0.5, float("inf"))
    d.prepare_roles_batch(refs, "reference", spec)
    assert_identical(records(ctx, refs, curs, cfg), with_a, "speculative prepare, then A")
    d.set_selection_batch(refs, [B, B], 0.0, 3.0)
    assert_identical(records(ctx, refs, curs, cfg), want_b, "speculative prepare under A, then B")


def test_device_masks_and_pitch():
    import torch
    ctx = context(8, deterministic=1)
    seeds = [101, 102]
    A = masks_of("noise", 3)
    _, refs, curs = pyramids(ctx, seeds)
    d.set_selection_batch(refs, [A, None], 0.2, 5.0)
    want = records(ctx, refs, curs)
    _, refs2, curs2 = pyramids(ctx, seeds)
    pitch = W + 64
    padded = torch.zeros((H, pitch), dtype=torch.uint8, device="cuda")
    padded[:, :W] = torch.from_numpy(A).cuda()
    torch.cuda.synchronize()
    d.set_selection_batch(refs2, [padded.data_ptr(), None], 0.2, 5.0, pitch=pitch)
    assert_identical(records(ctx, refs2, curs2), want, "device mask with a pitch")


def test_refused_arguments():
    ctx = context(8)
    _, refs, _ = pyramids(ctx, [111])
    L = ctx._lib
    fr = (C.c_void_p * 1)(refs[0].ptr)
    assert L.dvo_hip_frames_set_selection(ctx.ptr, 1, fr, None, 0, 0, 3.0, 1.0) == -2
    assert L.dvo_hip_frames_set_selection(ctx.ptr, 1, fr, None, 0, 0, float("nan"), 1.0) == -2
    m = (C.c_void_p * 1)(masks_of("ones").ctypes.data)
    assert L.dvo_hip_frames_set_selection(ctx.ptr, 1, fr, m, W - 1, 0, 0.0, 1.0) == -2
    assert L.dvo_hip_frames_set_selection(ctx.ptr, 0, fr, None, 0, 0, 0.0, 1.0) == -2
    assert L.dvo_hip_frame_set_level_selection(ctx.ptr, refs[0].ptr, LEVELS, masks_of("ones").ctypes.data_as(C.POINTER(C.c_uint8))) == -2


# ---- 8: the C++ facade's caller-defined predicates -----------------------------------------------------------------------------------

def test_cpp_facade_custom_predicates():
    """tests/cpp/selection_check.cpp: z <= 2.5 on the host = the device range [0, 2.5]; x < 40 on the host = explicit sets; the stock
    predicate unchanged; getDebugIndex holds the selection"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(root, "tests", "cpp", "selection_check")
    libdir = os.path.join(root, "dvo_slam_amd", "lib")
    d.build()
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "selection_check.cpp"), "-o", out, "-L" + libdir, "-ldvo_hip",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok"], (r.returncode, r.stdout, r.stderr)


def test_python_pyramid_regrowth_keeps_a_host_mask_and_refuses_a_device_address():
    import torch
    ctx = context(8)
    p = cm.synth(121, W, H)
    cam = d.RgbdCameraPyramid(W, H, p["K"], ctx)
    cam.build(2)
    a = cam.create_raw(p["grey_ref"], p["depth_ref"])
    b = cam.create_raw(p["grey_ref"], p["depth_ref"])
    mask = masks_of("blocks", 4)
    a.set_selection(mask, 0.5, 3.0)
    dev = torch.from_numpy(mask).cuda()
    torch.cuda.synchronize()
    b.set_selection(dev.data_ptr(), 0.5, 3.0)
    cam.build(LEVELS)
    a.build(LEVELS)                                                 # a new frame: the host copy of the mask goes with it
    _, fresh, _ = pyramids(ctx, [121])
    fresh[0].set_selection(mask, 0.5, 3.0)
    for l in range(LEVELS):
        assert d.PointSelection(a).select(l) == d.PointSelection(fresh[0]).select(l), l
    with pytest.raises(ValueError):
        b.build(LEVELS)
    b.clear_selection()
    b.build(LEVELS)


# ---- 7: what it is for -----------------------------------------------------------------------------------------------------------

def moving_box_pair(seed, w=W, h=H):
    """A textured background plane at 2.8-3.6 m (tests/scenes.py's surfaces) and one textured box at about 1.2 m that covers about a fifth of the image;
    between the two frames the camera moves by xi_true (|v| <= 3 cm, |omega| <= 0.03 rad) and the box ALSO moves on its own, by 6-8 cm
    across the line of sight -- a person or a vehicle in view.  Returns datagen.synth_pair's dict plus `box_ref`, the reference pixels
    the box covers."""
    from scenes import FR1_K, _Scene, _quantise_depth, se3_exp
    rng = np.random.default_rng([seed, 77])
    K = np.ascontiguousarray(FR1_K * (w / 640.0), dtype=np.float32)
    fx, fy, ox, oy = (float(k) for k in K)
    scene = _Scene(rng)
    scene.plane = np.array([rng.uniform(-0.03, 0.03), rng.uniform(0.05, 0.08), rng.uniform(0.30, 0.34)])   # background at 2.8-3.6 m
    z0 = rng.uniform(1.1, 1.3)
    half = np.array([140.0 / fx * z0, 110.0 / fy * z0, 0.2])                 # 280 x 220 pixels of 640 x 480: a fifth
    centre = np.array([rng.uniform(-0.1, 0.1) * z0, rng.uniform(-0.08, 0.08) * z0, z0 + half[2]])
    scene.boxes = [(centre - half, centre + half)]
    xi = rng.uniform(-1, 1, 6)
    xi[:3] *= 0.03 / np.linalg.norm(xi[:3])
    xi[3:] *= 0.015 / np.linalg.norm(xi[3:])
    ang = rng.uniform(0, 2 * np.pi)
    own = np.array([np.cos(ang), np.sin(ang), 0.0]) * rng.uniform(0.06, 0.08)   # the box's own motion, reference coordinates
    M = se3_exp(xi)                                                          # current -> reference
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rays = np.stack([(xx - ox) / fx, (yy - oy) / fy, np.ones_like(xx)], -1)
    out = dict(K=K, xi_true=xi)
    for view, (o, dvec), shift in (("ref", (np.zeros(3), rays), np.zeros(3)), ("cur", (M[:3, 3], rays @ M[:3, :3].T), own)):
        scene.boxes = [(centre - half + shift, centre + half + shift)]
        s, sid, p = scene.cast(o, dvec)
        p = np.where((sid == 1)[..., None], p - shift, p)                    # the texture moves with the box
        out["grey_" + view] = scene.grey(p, sid, rng.uniform(-1.5, 1.5, (h, w)))
        out["depth_" + view] = _quantise_depth(s)
        if view == "ref":
            out["box_ref"] = sid == 1
    return out


def test_masking_an_independently_moving_box_recovers_the_camera_motion():
    """Calibrated on an MI355X over seeds 0-7 (default configuration, levels 3 .. 1): the twist error against the camera's true motion is
    4.8e-2 .. 1.06e-1 without a selection and 1.3e-5 .. 7.0e-5 with the box masked (a 48-pixel margin) in the reference; the same
    scene with a box that stays put tracks to 6e-4 and 1.3e-3 unmasked (seeds 0 and 4, CPU oracle, levels 3 .. 1).  The bounds: masked below 5e-4,
    unmasked above 2e-2."""
    ctx = context(8)
    errs = []
    for seed in range(8):
        p = moving_box_pair(seed)
        assert 0.17 < p["box_ref"].mean() < 0.23
        cam = d.RgbdCameraPyramid(W, H, p["K"], ctx)
        cam.build(LEVELS)
        ref = cam.create_raw(p["grey_ref"], p["depth_ref"])
        cur = cam.create_raw(p["grey_cur"], p["depth_cur"])
        tr = d.DenseTracker(d.Config(), ctx)
        plain = d.Result()
        tr.match(ref, cur, plain)
        # the box with a margin of 48 pixels -- six pixels of level 3, whose intensities average 8 x 8 blocks of level 0 -- as a
        # segmentation mask would be dilated (with 4 or 32 the coarse levels still see the box's texture: half the seeds stay at 1-9e-2)
        box = p["box_ref"].copy()
        for axis in (0, 1):
            grown = box.copy()
            for k in range(1, 49):
                grown |= np.roll(box, k, axis) | np.roll(box, -k, axis)
            box = grown
        ref.set_selection((~box).astype(np.uint8))
        masked = d.Result()
        tr.match(ref, cur, masked)
        e_plain = np.abs(po.se3_log(plain.Transformation) - p["xi_true"]).max()
        e_masked = np.abs(po.se3_log(masked.Transformation) - p["xi_true"]).max()
        errs.append((e_plain, e_masked))
    assert all(e_masked < 5e-4 for _, e_masked in errs), errs
    assert all(e_plain > 2e-2 for e_plain, _ in errs), errs
