"""Shared helpers of the test-suite: synthetic pairs, golden fixtures, the host emulation of the device code."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
DROPIN_BUILD = os.path.join(ROOT, "oracle", "_ref", "dropin")      # oracle/dropin.mk: the reference's callers built on the facade

from oracle import pyoracle as po   # noqa: E402
from dvo_slam_amd import _lib as hl  # noqa: E402

_pairs = {}


def synth(seed, w=640, h=480, K=None):
    """K: the intrinsics [fx, fy, ox, oy] the pair is rendered with (tests/cameras.py); None = fr1 scaled to the width"""
    key = (seed, w, h, None if K is None else np.asarray(K, np.float32).tobytes())
    if key not in _pairs:
        _pairs[key] = po.synth_pair(seed, w, h, K)
    return _pairs[key]


def oracle_pyramids(pair, levels):
    return po.pyramids_from_pair(pair, levels)


def twist_matrix_error(Ta, Tb):
    """max-abs twist of Ta^-1 Tb"""
    return np.abs(po.se3_log(np.linalg.inv(Ta) @ Tb)).max()


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


# ---- option "ref_order": the reference's rank quirks Q6 and Q7 restated in float64 ------------------------------------------------
def mahalanobis_f32(r, P):
    """r^T P r per row of r (float32, the order of pixel_math.h::mahalanobis, P row-major 2x2)"""
    r = np.asarray(r, np.float32)
    P = np.asarray(P, np.float32).reshape(2, 2)
    return (r[:, 0] * P[0, 0] + r[:, 1] * P[1, 0]) * r[:, 0] + (r[:, 0] * P[0, 1] + r[:, 1] * P[1, 1]) * r[:, 1]


def rank_formula(res, P_prev, first, weights=None):
    """One pass of option "ref_order" from a residual plane [h, w, 2] in raster order (NaN: no constraint), written out over the
    ranks k = 0 .. n-1 of the valid constraints, in float64:
      n, S = sum_{k even} w_k r_k r_k^T + sum_{k odd} w_k r_{k-1} r_{k-1}^T  (Q6; entries 00, 01, 11),
      cov = S / (n - 3) (float64; `P` is the float32 inverse of its float32 rounding, as the kernels form it),
      kept = 50 floor(n / 50): the ranks [kept, n) leave the log-likelihood sum (Q7),
      neg_ll = -(n/2 log det P - 7/2 sum_{k < kept} log(1 + 0.2 r_k^T P r_k))  (None where n < 6: no log-likelihood is formed).
    The weights: 1 on a first pass, else float32 7 / (5 + r^T P_prev r) as the sweep forms them; `weights` (float32 per valid
    constraint, in rank order) overrides both -- e.g. the host-reciprocal weights of option "ref_compat", which this formula does not
    restate (its reference is the oracle's target mode)."""
    r32 = np.asarray(res, np.float32).reshape(-1, 2)
    r32 = r32[~np.isnan(r32[:, 0])]
    r = r32.astype(np.float64)
    n = len(r)
    if weights is not None:
        w = np.asarray(weights, np.float32).astype(np.float64)
    elif first:
        w = np.ones(n)
    else:
        w = (np.float32(7.0) / (np.float32(5.0) + mahalanobis_f32(r32, P_prev))).astype(np.float64)
    rr = np.stack([r[:, 0] * r[:, 0], r[:, 0] * r[:, 1], r[:, 1] * r[:, 1]], 1)
    lead = np.arange(n) & ~1                                   # the rank whose residual a constraint's term uses
    S = (w[:, None] * rr[lead]).sum(0) if n else np.zeros(3)
    kept = n // 50 * 50
    out = dict(n=n, S=S, kept=kept, cov=None, P=None, neg_ll=None)
    if n >= 4:
        cov = S / (n - 3)
        C32 = cov.astype(np.float32)
        det = C32[0] * C32[2] - C32[1] * C32[1]
        inv = np.float32(1.0) / det
        P = np.array([[C32[2] * inv, -C32[1] * inv], [-C32[1] * inv, C32[0] * inv]], np.float32)
        out.update(cov=cov, P=P)
        if n >= 6:
            q = mahalanobis_f32(r32, P).astype(np.float64)
            detP = float(P[0, 0] * P[1, 1] - P[0, 1] * P[1, 0])
            out["neg_ll"] = -(0.5 * n * np.log(detP) - 3.5 * np.log1p(0.2 * q[:kept]).sum())
    return out


def rank_classes(res, res_without_q3, n_selected):
    """The rank classes a linearisation falls into (its residual plane under Q3 and the same state without Q3)"""
    valid = ~np.isnan(res[:, :, 0])
    counts = valid.sum(1)
    n = int(counts.sum())
    n_no_q3 = int((~np.isnan(res_without_q3[:, :, 0])).sum())
    kept = n // 50 * 50
    out = set()
    if 6 <= n < 50:
        out.add("n<50")
    if n >= 50 and n % 50 == 0:
        out.add("n%50==0")
    if n % 50 == 49:
        out.add("n%50==49")
    if n >= 6:
        out.add("odd" if n % 2 else "even")
    if n_no_q3 == n + 1:
        out.add("q3_removes")
    if n_selected % 2 and n_no_q3 == n:
        out.add("q3_last_gave_none")
    if n_no_q3 == 6 and n == 5:
        out.add("q3_6_to_5")
    if 6 <= n and kept < n:
        first = np.cumsum(counts) - counts                   # rank of each row's first constraint
        row_kept = int(np.searchsorted(np.cumsum(counts), kept, side="right"))
        row_last = int(np.searchsorted(np.cumsum(counts), n - 1, side="right"))
        if first[row_kept] == kept:
            out.add("tail_at_row_start")
        if (counts[row_kept:row_last + 1] == 0).any():
            out.add("tail_spans_empty_row")
    return out


# Inputs of one linearisation (level 0 of a synth(seed, w, h) pair, one pyramid level, T = exp(ty e_y), selection thresholds) that
# together hit every rank class of option "ref_order" (rank_classes), found with the oracle's target mode on the CPU: (seed, w, h, ty,
# intensity threshold, depth threshold, n, classes).  tests/test_ref_order_classes.py checks that the oracle still puts each row in its
# classes; tests/test_gpu_ref_order_edges.py runs every row on the GPU.
RANK_CLASSES = ("n<50", "n%50==0", "n%50==49", "odd", "even", "tail_at_row_start", "tail_spans_empty_row", "q3_removes",
                "q3_last_gave_none", "q3_6_to_5")
RANK_CLASS_TABLE = [
    (3, 36, 20, 0.0, 50.0, 1e9, 49, ("n%50==49", "n<50", "odd", "q3_last_gave_none", "tail_at_row_start", "tail_spans_empty_row")),
    (1, 36, 20, 0.0, 60.0, 1e9, 16, ("even", "n<50", "q3_removes", "tail_at_row_start", "tail_spans_empty_row")),
    (3, 36, 20, 0.0, 10.0, 1e9, 350, ("even", "n%50==0")),
    (5, 36, 20, 0.0, 70.0, 1e9, 5, ("q3_6_to_5", "q3_removes")),
    (0, 36, 20, 0.0, 40.0, 1e9, 97, ("odd", "q3_last_gave_none", "tail_at_row_start")),
    (0, 65, 49, 0.02, 50.0, 1e9, 83, ("odd", "tail_at_row_start", "tail_spans_empty_row")),
    (2, 65, 49, 0.0, 30.0, 0.02, 1750, ("even", "n%50==0")),
    (3, 65, 49, -0.02, 20.0, 1e9, 899, ("n%50==49", "odd", "q3_last_gave_none")),
    (6, 65, 49, 0.0, 70.0, 1e9, 5, ("q3_6_to_5", "q3_removes")),
    (1, 65, 49, 0.0, 70.0, 1e9, 6, ("even", "n<50", "q3_removes", "tail_at_row_start", "tail_spans_empty_row")),
]


def rank_class_row_oracle(row, want_residuals=True):
    """the oracle's target mode on a row of RANK_CLASS_TABLE: (first-pass output, the same without Q3)"""
    seed, w, h, ty, ithr, dthr = row[:6]
    ref, cur = oracle_pyramids(synth(seed, w, h), 1)
    T34 = po.se3_exp(np.array([0.0, ty, 0.0, 0.0, 0.0, 0.0]))[:3]
    target = po.QUIRKS | po.Q_DROP_ODD | po.Q_LOGLIK_TAIL | po.X_PAIRING_F64
    o = po.level_iteration(ref, cur, 0, T34, first=True, mode=target, ithr=ithr, dthr=dthr, want_residuals=want_residuals)
    o_no_q3 = po.level_iteration(ref, cur, 0, T34, first=True, mode=target & ~po.Q_DROP_ODD, ithr=ithr, dthr=dthr, want_residuals=want_residuals)
    return o, o_no_q3


# ---- host emulation of the device headers (tests/emul/emul_device.cpp) ---------------------------------
class EmulLevel(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("ox", C.c_float), ("oy", C.c_float),
                ("R", C.POINTER(C.c_float)), ("A", C.POINTER(C.c_float)), ("B", C.POINTER(C.c_float)), ("n_selected", C.c_int)]


_emul = None


def emul_lib():
    global _emul
    if _emul is None:
        src = os.path.join(HERE, "emul", "emul_device.cpp")
        out = os.path.join(HERE, "emul", "libemul_device.so")
        deps = [src] + [os.path.join(ROOT, "dvo_slam_amd", "csrc", f) for f in
                        ("pixel_math.h", "solver_logic.h", "se3_device.h", "device_types.h", "hd_compat.h", "linear_walk.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O2", "-march=native", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unknown-pragmas", "-pthread",
                                   "-shared", "-o", out, src])
        L = C.CDLL(out)
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        L.emul_level_iteration.argtypes = [C.POINTER(EmulLevel), fp, fp, C.c_int, C.POINTER(hl.IterationOut), fp]
        L.emul_match.argtypes = [C.POINTER(EmulLevel), C.POINTER(hl.Config), C.POINTER(hl.Result), C.POINTER(hl.LevelStats), C.c_int,
                                 C.POINTER(hl.IterationStats), C.c_int]
        L.emul_match_speculative.argtypes = L.emul_match.argtypes
        L.emul_exchange_stress.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint]
        L.emul_locate_check.argtypes = [C.c_int, C.c_int]
        L.emul_set_schedule.argtypes = [C.c_int]
        L.emul_set_schedule.restype = None
        L.emul_se3_exp.argtypes = [dp, dp]
        L.emul_se3_log.argtypes = [dp, dp]
        L.emul_solve6.argtypes = [dp, dp, dp]
        _emul = L
    return _emul


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class EmulPair:
    """Device-layout planes (R / A / B) built from the oracle's pyramids, as the pyramid kernels would."""

    def __init__(self, ref_pyr, cur_pyr, levels, ithr=0.0, dthr=0.0):
        self.keep = []
        self.arr = (EmulLevel * levels)()
        for l in range(levels):
            rp = [ref_pyr.plane(l, k)[0] for k in range(6)]
            cp = [cur_pyr.plane(l, k)[0] for k in range(6)]
            K = ref_pyr.plane(l, 0)[1]
            n_sel, mask = ref_pyr.select(l, ithr, dthr)
            Zsel = np.where(mask.astype(bool), rp[1], np.float32(np.nan)).astype(np.float32)
            R = np.ascontiguousarray(np.stack([Zsel, rp[0], rp[2], rp[3]], axis=-1), dtype=np.float32)
            A = np.ascontiguousarray(np.stack([cp[0], cp[1], cp[2], cp[3]], axis=-1), dtype=np.float32)
            B = np.ascontiguousarray(np.stack([cp[4], cp[5]], axis=-1), dtype=np.float32)
            self.keep += [R, A, B]
            h, w = rp[0].shape
            self.arr[l] = EmulLevel(w, h, K[0], K[1], K[2], K[3], _fp(R), _fp(A), _fp(B), n_sel)
        self.levels = levels

    def level_iteration(self, level, T34, P_prev=None, first=True):
        T34 = np.ascontiguousarray(np.asarray(T34, dtype=np.float32).reshape(-1)[:12])
        Pp = np.zeros(4, np.float32) if P_prev is None else np.ascontiguousarray(np.asarray(P_prev, np.float32).reshape(-1))
        out = hl.IterationOut()
        L = self.arr[level]
        res = np.empty((L.h, L.w, 2), np.float32)
        rc = emul_lib().emul_level_iteration(C.byref(self.arr[level]), _fp(T34), _fp(Pp), int(first),
                                             C.byref(out), _fp(res))
        return dict(rc=rc, n=out.n, n_selected=out.n_selected, cov=np.array(out.scale_cov), P=np.array(out.precision).reshape(2, 2),
                    neg_ll=out.neg_loglik, A=np.array(out.A).reshape(6, 6), b=np.array(out.b), residuals=res)

    def match(self, cfg, T_init=None, speculative=False, raw=False):
        """cfg: dvo_slam_amd.Config. Returns the same dict layout as pyoracle.match.  speculative: the control flow of the resident
        kernel (emul_match_speculative).  raw: also the raw bytes of result + level + iteration records (for bit comparisons)."""
        ccfg = cfg.to_c()
        res = hl.Result()
        T0 = np.eye(4) if T_init is None else np.asarray(T_init, dtype=np.float64)
        for i, v in enumerate(T0.reshape(-1)):
            res.transformation[i] = v
        nl = cfg.FirstLevel - cfg.LastLevel + 1
        cap = nl * cfg.MaxIterationsPerLevel
        levels = (hl.LevelStats * nl)()
        iters = (hl.IterationStats * cap)()
        fn = emul_lib().emul_match_speculative if speculative else emul_lib().emul_match
        rc = fn(self.arr, C.byref(ccfg), C.byref(res), levels, nl, iters, cap)
        assert rc == 0
        out = result_to_dict(res, levels, iters)
        if raw:
            used = sum(levels[i].n_iterations for i in range(res.n_levels))
            out["raw"] = (bytes(res), bytes(levels)[: res.n_levels * C.sizeof(hl.LevelStats)], bytes(iters)[: used * C.sizeof(hl.IterationStats)])
        return out


def result_to_dict(res, levels, iters):
    out_levels = []
    for li in range(res.n_levels):
        L = levels[li]
        its = []
        for k in range(L.n_iterations):
            s = iters[L.first_iteration_index + k]
            its.append(dict(id=s.id, n=s.valid_constraints, neg_ll=s.tdist_loglik, precision=np.array(s.tdist_precision).reshape(2, 2),
                            prior_ll=s.prior_loglik, x=np.array(s.increment), A=np.array(s.information).reshape(6, 6)))
        out_levels.append(dict(id=L.id, max_valid_pixels=L.max_valid_pixels, valid_pixels=L.valid_pixels, termination=L.termination,
                               iterations=its))
    return dict(T=np.array(res.transformation).reshape(4, 4), information=np.array(res.information).reshape(6, 6),
                loglik=res.loglik, levels=out_levels, entropy=res.entropy, condition_number=res.condition_number,
                constraint_ratio=res.constraint_ratio, constraint_ratio_accepted=res.constraint_ratio_accepted)


def keyframe_statistics_from(result):
    """The reference's host-side derivations from a Result dict (T, information, levels): keyframe_tracker.cpp:165-196,
    tracking_result_evaluation.cpp:52-55, constraint_proposal_voter.cpp:136-140, dense_tracking_config.cpp:138-150."""
    info = result["information"]
    ev = np.sort(np.linalg.eigvalsh(info)) if np.isfinite(info).all() else np.full(6, np.nan)
    level = result["levels"][-1]
    its, term = level["iterations"], level["termination"]
    need = 2 if term in (2, 3) else 1
    accepted = 0.0
    if len(its) >= need:
        accepted = float((its[-2] if term == 2 else its[-1])["n"]) / level["valid_pixels"]
    with np.errstate(all="ignore"):
        return dict(entropy=float(np.log(np.linalg.det(info))), condition_number=float(abs(ev[5] / ev[0])),
                    constraint_ratio=float(its[-1]["n"]) / level["valid_pixels"], constraint_ratio_accepted=accepted)


def tracker_result_to_dict(r):
    """dvo_slam_amd.Result -> the dict layout of pyoracle.match"""
    out_levels = []
    for L in r.Statistics.Levels:
        its = [dict(id=s.Id, n=s.ValidConstraints, neg_ll=s.TDistributionLogLikelihood, precision=s.TDistributionPrecision,
                    prior_ll=s.PriorLogLikelihood, x=s.EstimateIncrement, A=s.EstimateInformation) for s in L.Iterations]
        out_levels.append(dict(id=L.Id, max_valid_pixels=L.MaxValidPixels, valid_pixels=L.ValidPixels, termination=L.TerminationCriterion,
                               iterations=its))
    return dict(T=r.Transformation, information=r.Information, loglik=r.LogLikelihood, levels=out_levels, entropy=r.Entropy,
                condition_number=r.ConditionNumber, constraint_ratio=r.ConstraintRatio, constraint_ratio_accepted=r.ConstraintRatioAccepted)


def oracle_config_from(cfg, mode):
    return po.make_config(cfg.FirstLevel, cfg.LastLevel, cfg.MaxIterationsPerLevel, cfg.Precision, cfg.Mu, cfg.UseInitialEstimate,
                          cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold, mode)


def compare_runs(a, b):
    """Compare two match() result dicts over the common iteration prefix of every level.

    The iteration COUNT of a level is decided by comparisons at the float noise floor (|x|_inf against
    Precision = 5e-7, -ll against the previous -ll near convergence), so two correct implementations can
    legitimately stop one pass apart; `structure_mismatch` counts such levels and the callers bound it, while
    everything in the common prefix and the final transform must agree."""
    summary = dict(max_x_err=0.0, max_ll_rel=0.0, max_A_rel=0.0, n_mismatch=0, iters=0, structure_mismatch=0, max_iter_count_diff=0)
    assert len(a["levels"]) == len(b["levels"])
    for La, Lb in zip(a["levels"], b["levels"]):
        assert La["id"] == Lb["id"]
        assert La["valid_pixels"] == Lb["valid_pixels"], ("selection size", La["id"], La["valid_pixels"], Lb["valid_pixels"])
        assert La["max_valid_pixels"] == Lb["max_valid_pixels"]
        if len(La["iterations"]) != len(Lb["iterations"]) or La["termination"] != Lb["termination"]:
            summary["structure_mismatch"] += 1
            summary["max_iter_count_diff"] = max(summary["max_iter_count_diff"], abs(len(La["iterations"]) - len(Lb["iterations"])))
        for ia, ib in zip(La["iterations"], Lb["iterations"]):
            summary["iters"] += 1
            summary["n_mismatch"] += int(abs(ia["n"] - ib["n"]) > max(2, 2e-4 * ib["n"]))
            if np.isfinite(ia["neg_ll"]) and np.isfinite(ib["neg_ll"]):
                summary["max_ll_rel"] = max(summary["max_ll_rel"], abs(ia["neg_ll"] - ib["neg_ll"]) / max(1.0, abs(ib["neg_ll"])))
            if np.all(np.isfinite(ia["x"])) and np.all(np.isfinite(ib["x"])):
                summary["max_x_err"] = max(summary["max_x_err"], np.abs(ia["x"] - ib["x"]).max())
                summary["max_A_rel"] = max(summary["max_A_rel"], np.abs(ia["A"] - ib["A"]).max() / np.abs(ib["A"]).max())
    summary["T_err"] = twist_matrix_error(a["T"], b["T"])
    return summary


# ---- scenes at another scale of intensity and depth (tests/test_scales.py, tests/test_gpu_scales.py) ---------------------------------
# The warp of the single-linearisation tests (test_default_schedule_single_linearisation_against_oracle), as a twist (v, omega)
SCALE_XI = (0.004, -0.003, 0.002, 0.005, -0.004, 0.003)


def scaled_pair(pair, ki, kz):
    """The float32 planes of `pair` (synth / scenes.edge_scene) with the grey levels x 2^ki and the converted depth (metres) x 2^kz: a
    dimmer or lower-contrast frame, a nearer or farther scene.  Both products are exact (powers of two, no under- or overflow for the
    exponents the tests use: asserted), NaN = no depth stays NaN.  xi_true's translation is x 2^kz, as the true motion of the scaled
    scene is.  -> dict(grey_ref, depth_ref, grey_cur, depth_cur: float32; K; xi_true; ki; kz)"""
    si, sz = np.ldexp(np.float32(1.0), ki), np.ldexp(np.float32(1.0), kz)
    out = dict(K=pair["K"], ki=ki, kz=kz)
    for v in ("ref", "cur"):
        g = pair["grey_" + v].astype(np.float32)
        z = po.convert_raw_depth(pair["depth_" + v])
        gs, zs = g * si, z * sz
        assert np.array_equal(gs / si, g) and np.array_equal(zs / sz, z, equal_nan=True) and np.isfinite(gs).all()
        out["grey_" + v], out["depth_" + v] = gs, zs
    xi = np.array(pair["xi_true"], np.float64)
    xi[:3] *= 2.0 ** kz
    out["xi_true"] = xi
    return out


def scaled_warp(xi, kz):
    """exp(xi) as the 3 x 4 a linearisation takes, its translation x 2^kz (exact, in float32 too): the same warp of the scaled scene"""
    T34 = np.array(po.se3_exp(np.asarray(xi, np.float64))[:3])
    T34[:, 3] *= 2.0 ** kz
    return T34


def scaled_oracle_pyramids(sp, levels):
    return tuple(po.Pyramid(sp["grey_" + v], sp["depth_" + v], sp["K"], levels) for v in ("ref", "cur"))


def scaled_gpu_frames(ctx, sp, levels):
    """the frames of a scaled_pair through the float ingest (RgbdCameraPyramid.create: intensity "taken as is", depth in metres)"""
    import dvo_slam_amd as d
    h, w = sp["grey_ref"].shape
    cam = d.RgbdCameraPyramid(w, h, sp["K"], ctx)
    cam.build(levels)
    return cam.create(sp["grey_ref"], sp["depth_ref"]), cam.create(sp["grey_cur"], sp["depth_cur"])


def kappa0(M):
    """max|M| / min_i M_ii of a symmetric positive matrix: "1e-5 of the largest entry" is 1e-5 kappa0 in the metric of scale_errors"""
    M = np.asarray(M, np.float64)
    return float(np.abs(M).max() / np.diag(M).min())


def kappa0_b(A, b):
    """the same for the right-hand side: (max|b| / min_i D_i) / max|D^-1 b| with D = sqrt(diag A) -- an error of 1e-5 max|b| in the entry
    with the smallest D_i, in the metric of scale_errors"""
    D = np.sqrt(np.diag(np.asarray(A, np.float64)))
    b = np.asarray(b, np.float64)
    return float(np.abs(b).max() / D.min() / np.abs(b / D).max())


def scale_errors(g, o):
    """One linearisation `g` against the reference `o` (dicts with A, b, P) in a metric that survives a change of units of the twist's
    translation, of the intensity or of the depth: with D = sqrt(diag(A_o)),
      errA = max |D^-1 (A_g - A_o) D^-1|          (every entry relative to the geometric mean of its two diagonal entries),
      errb = max |D^-1 (b_g - b_o)| / max |D^-1 b_o|,
      errP = max |E^-1 (P_g - P_o) E^-1|  with E = sqrt(diag(P_o)).
    A block of A (or an entry of P) that is a thousand times smaller than the largest one is held as tightly as that one."""
    Ao, Po = np.asarray(o["A"], np.float64), np.asarray(o["P"], np.float64)
    D, E = np.sqrt(np.diag(Ao)), np.sqrt(np.diag(Po))
    dA = (np.asarray(g["A"], np.float64) - Ao) / np.outer(D, D)
    db = (np.asarray(g["b"], np.float64) - np.asarray(o["b"], np.float64)) / D
    dP = (np.asarray(g["P"], np.float64) - Po) / np.outer(E, E)
    return dict(errA=float(np.abs(dA).max()), errb=float(np.abs(db).max() / np.abs(np.asarray(o["b"], np.float64) / D).max()),
                errP=float(np.abs(dP).max()))


def unscaled_run(run, kz):
    """A match() result dict of a scene whose depth is x 2^kz, in the units of the unscaled scene: the translation of T and of every
    increment divided by 2^kz, the information matrices multiplied blockwise (exact: powers of two).  compare_runs then holds a far
    scene's translation as tightly as the near one's."""
    s = 2.0 ** kz
    S = np.array([s, s, s, 1.0, 1.0, 1.0])
    out = dict(run)
    T = np.array(run["T"], np.float64)
    T[:3, 3] /= s
    out["T"] = T
    out["information"] = np.asarray(run["information"]) * np.outer(S, S)
    out["levels"] = []
    for L in run["levels"]:
        its = [dict(it, x=np.asarray(it["x"]) / S, A=np.asarray(it["A"]) * np.outer(S, S)) for it in L["iterations"]]
        out["levels"].append(dict(L, iterations=its))
    return out


# ---- the reference's own callers on the engine (tests/dropin) -------------------------------------------------------
_dropin = None


def dropin_api():
    """(library, "dropin_") for the api= argument of pyoracle's ref_* wrappers: oracle/_ref/dropin/libdvo_dropin.so = the
    reference's unmodified dvo_slam sources + the shared caller code, compiled against include/dvo/ and linked with libdvo_hip.so.
    Built here when the reference tree is present (the built library travels to the GPU box); None when neither is there."""
    global _dropin
    if _dropin is None:
        import dvo_slam_amd
        dvo_slam_amd.build()
        po.build()
        if os.path.isdir("/root/reference/dvo_slam/src"):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-f", "dropin.mk", "-s"])
        path = os.path.join(DROPIN_BUILD, "libdvo_dropin.so")
        if not os.path.exists(path):
            return None
        L = C.CDLL(path)
        po.bind_public_api(L, "dropin_")
        L.dropin_engine.restype = C.c_char_p
        L.dropin_level_fields.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                          C.POINTER(C.c_float)]
        _dropin = (L, "dropin_")
    return _dropin
