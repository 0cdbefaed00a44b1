"""CPU tier of option "ref_order" (dvo_slam_amd/csrc/ref_order.h): the reference's rank-dependent quirks Q3 (odd selection: the last
selected pixel is skipped), Q6 (the scale sums pair the constraints by rank and use the first residual of a pair twice) and Q7 (the
log-likelihood sum drops its last n mod 50 terms).  The header's algebra, compiled for the host by tests/emul/ref_order_emul.cpp and
joined in the order of the kernels, against a plain rank formula on synthetic masks and against the oracle's quirk modes on the
oracle's own residual planes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common as cm
from oracle import pyoracle as po

TARGET = po.QUIRKS | po.Q_DROP_ODD | po.Q_LOGLIK_TAIL | po.X_PAIRING_F64
TARGET_COMPAT = TARGET | po.Q_RCP_PROJECTION | po.Q_RCP_WEIGHTS      # with option "ref_compat"
_lib = None


def emul():
    global _lib
    if _lib is None:
        src = os.path.join(cm.HERE, "emul", "ref_order_emul.cpp")
        out = os.path.join(cm.HERE, "emul", "libref_order_emul.so")
        deps = [src] + [os.path.join(cm.ROOT, "dvo_slam_amd", "csrc", f) for f in ("ref_order.h", "pixel_math.h", "device_types.h", "hd_compat.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-o", out, src])
        L = C.CDLL(out)
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        L.ref_order_emul.argtypes = [fp, C.c_int, C.c_int, fp, C.c_int, C.c_int, dp, fp, fp]
        L.ref_order_emul.restype = None
        _lib = L
    return _lib


def run_emul(res, P_prev, first, host_rcp=False):
    res = np.ascontiguousarray(res, np.float32)
    h, w = res.shape[:2]
    Pp = np.ascontiguousarray(np.asarray(P_prev, np.float32).reshape(-1))
    out, Cv, P = np.zeros(7), np.zeros(3, np.float32), np.zeros(4, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    emul().ref_order_emul(fp(res), w, h, fp(Pp), int(first), int(host_rcp), out.ctypes.data_as(C.POINTER(C.c_double)), fp(Cv), fp(P))
    return dict(n=int(out[0]), S=out[1:4], ll_all=out[4], ll_tail=out[5], neg_ll=out[6], cov=Cv, P=P.reshape(2, 2))


def synthetic_plane(rng, h, w, n_wanted, empty_rows=(), dense_rows=()):
    res = np.full((h, w, 2), np.nan, np.float32)
    free = [(v, u) for v in range(h) if v not in empty_rows for u in range(w)]
    pick = rng.choice(len(free), size=n_wanted, replace=False)
    for i in pick:
        v, u = free[i]
        res[v, u] = rng.normal(size=2) * [0.05, 0.02]
    for v in dense_rows:
        res[v, :] = rng.normal(size=(w, 2)) * [0.05, 0.02]
    return res


@pytest.mark.parametrize("case", [
    dict(h=7, w=5, n=6),                                      # n = 6: the smallest n the log-likelihood is formed for
    dict(h=12, w=70, n=49),                                   # n < 50: the whole log-likelihood sum is dropped
    dict(h=16, w=64, n=150, empty=(0, 3, 4, 15)),             # a multiple of 50: nothing dropped
    dict(h=40, w=130, n=1001, empty=tuple(range(10, 20))),    # odd n, runs of empty rows
    dict(h=30, w=200, n=1234, dense=(5, 29)),                 # even n, full rows
    dict(h=300, w=33, n=2717, empty=(299,)),                  # more rows than the combine has threads; width < 64
    dict(h=5, w=2500, n=3001),                                # wide rows: runs of 40 pixels per lane
])
@pytest.mark.parametrize("first", [True, False])
def test_join_equals_the_rank_formula_on_synthetic_masks(case, first):
    rng = np.random.default_rng(case["n"] + case["h"])
    res = synthetic_plane(rng, case["h"], case["w"], case["n"], case.get("empty", ()), case.get("dense", ()))
    P_prev = [900.0, 3.0, 3.0, 2500.0]
    e = run_emul(res, P_prev, first)
    f = cm.rank_formula(res, P_prev, first)
    n, S = f["n"], f["S"]
    assert e["n"] == n
    assert np.allclose(e["S"], S, rtol=1e-12, atol=0)
    # rows that begin on odd ranks exist (the pairing crosses row boundaries)
    counts = (~np.isnan(res[:, :, 0])).sum(1)
    assert ((np.cumsum(counts) - counts) % 2 == 1).any()
    # Q7: the last n mod 50 terms are the dropped ones
    kept = n // 50 * 50
    r = res.reshape(-1, 2)
    r = r[~np.isnan(r[:, 0])]
    P = e["P"]
    terms = np.log1p(0.2 * np.array([(a * P[0, 0] + b * P[1, 0]) * a + (a * P[0, 1] + b * P[1, 1]) * b for a, b in r.astype(np.float32)], np.float64))
    assert np.isclose(e["ll_tail"], terms[kept:].sum(), rtol=1e-9, atol=1e-12)
    if n % 50 == 0:
        assert e["ll_tail"] == 0.0


def test_a_plane_without_constraints():
    res = np.full((8, 16, 2), np.nan, np.float32)
    e = run_emul(res, [1, 0, 0, 1], True)
    assert e["n"] == 0 and not e["S"].any()


CASES = [(1234, 640, 480, 0.0), (1234, 640, 480, -0.03), (7, 640, 480, -0.03)]


@pytest.fixture(scope="module")
def oracle_pairs():
    out = {}
    for seed, w, h, _ in CASES:
        out[(seed, w, h)] = cm.oracle_pyramids(cm.synth(seed, w, h), 4)
    return out


@pytest.mark.parametrize("seed,w,h,ty", CASES)
@pytest.mark.parametrize("level", [3, 2, 1, 0])
@pytest.mark.parametrize("compat", [False, True])
def test_join_reproduces_the_oracle_target_mode(oracle_pairs, seed, w, h, ty, level, compat):
    """the oracle's residual plane in mode QUIRKS | Q3 | Q7 | X_PAIRING_F64 (+ Q1 under option "ref_compat"), first pass and a weighted
    one: n equal, scale_cov and P within 1e-6 of their largest entry, -ll within 1e-6 relative"""
    ref, cur = oracle_pairs[(seed, w, h)]
    T34 = po.se3_exp(np.array([0.0, ty, 0.0, 0.0, 0.0, 0.0]))[:3]
    mode = TARGET_COMPAT if compat else TARGET
    o1 = po.level_iteration(ref, cur, level, T34, first=True, mode=mode, want_residuals=True)
    o2 = po.level_iteration(ref, cur, level, T34, P_prev=o1["P"], first=False, mode=mode, want_residuals=True)
    for o, P_prev, first in ((o1, np.zeros(4), True), (o2, o1["P"], False)):
        e = run_emul(o["residuals"], P_prev, first, host_rcp=compat)
        assert e["n"] == o["n"]
        assert np.abs(e["cov"] - o["cov"]).max() <= 1e-6 * np.abs(o["cov"]).max(), (e["cov"], o["cov"])
        assert np.abs(e["P"] - o["P"]).max() <= 1e-6 * np.abs(o["P"]).max()
        assert abs(e["neg_ll"] - o["neg_ll"]) <= 1e-6 * abs(o["neg_ll"]), (e["neg_ll"], o["neg_ll"])


def test_rank_formula_recipe_on_the_oracle_plane(oracle_pairs):
    """the recipe itself: a numpy rank formula on the oracle's own residual plane reproduces its scale_cov on all four levels"""
    ref, cur = oracle_pairs[(1234, 640, 480)]
    T34 = po.se3_exp(np.array([0.0, -0.03, 0.0, 0.0, 0.0, 0.0]))[:3]
    for level in range(4):
        o = po.level_iteration(ref, cur, level, T34, first=True, mode=TARGET, want_residuals=True)
        f = cm.rank_formula(o["residuals"], None, True)
        n, S = f["n"], f["S"]
        assert n == o["n"]
        cov = S / (n - 3)                                     # (the oracle's is rounded to float32: half an ulp, 6e-8)
        assert np.abs(cov - o["cov"]).max() <= 1e-7 * np.abs(cov).max()
