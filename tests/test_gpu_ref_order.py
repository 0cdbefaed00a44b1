"""GPU tier of option "ref_order" (ref_order.hip): the reference's rank-dependent quirks Q3, Q6 and Q7 on the launch path.

  one linearisation (dvo_hip_level_iteration) against the oracle's modes QUIRKS | Q3 | Q7 | X_PAIRING_F64 (+ Q1 under "ref_compat"):
      n equal, scale_cov and P within 1e-5 of their largest entry, -ll within 1e-6 relative, A and b within 1e-5 of their largest entry
  the default schedule: its own residual plane through the rank formula gives its scale_cov and -ll
  whole matches with "ref_compat" + "ref_order" (variants 8 and 7; one pair alone and a 32-pair batch) against the oracle's target match
      (Information within 2e-3 of its largest entry, LogLikelihood 5e-5) and the reference's own match() (oracle/_ref: the issue's 5e-3 /
      1e-4, or the oracle's own distance plus those margins where it is larger)
  the reference's keyframe graph on the engine: loop-closure chi2 closest to the reference's with both options
  plumbing: values, variants, the counter, the environment variable, planes left behind, a pair alone and in a batch
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import common as cm
import dvo_slam_amd as d
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
TARGET = po.QUIRKS | po.Q_DROP_ODD | po.Q_LOGLIK_TAIL | po.X_PAIRING_F64
TARGET_COMPAT = TARGET | po.Q_RCP_PROJECTION | po.Q_RCP_WEIGHTS


def gpu_pyramids(ctx, pair, levels):
    h, w = pair["grey_ref"].shape
    cam = d.RgbdCameraPyramid(w, h, pair["K"], ctx)
    cam.build(levels)
    return cam.create_raw(pair["grey_ref"], pair["depth_ref"]), cam.create_raw(pair["grey_cur"], pair["depth_cur"])


def context(variant=7, ref_compat=0, ref_order=1, **options):
    ctx = d.Context(0)
    ctx.set_option("variant", variant)
    ctx.set_option("ref_compat", ref_compat)
    ctx.set_option("ref_order", ref_order)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def rel_max(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("compat", [1, 0])
def test_one_linearisation_against_the_oracle(compat):
    """variant 7 (residuals and counts bit-identical to the oracle's), levels 3 .. 0, first and weighted passes, at the identity and
    at ty = -0.03; seeds 1234 and 7 at ty = -0.03 are states where Q3 takes a valid constraint away (levels 1 and 0)"""
    mode = TARGET_COMPAT if compat else TARGET
    ctx = context(7, compat, 1)
    q3_seen = 0
    worst = dict(cov=0.0, P=0.0, ll=0.0, A=0.0, b=0.0)
    for seed, ty in ((1234, 0.0), (1234, -0.03), (7, -0.03)):
        pair = cm.synth(seed, 640, 480)
        oref, ocur = cm.oracle_pyramids(pair, 4)
        gref, gcur = gpu_pyramids(ctx, pair, 4)
        trk = d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx)
        T34 = po.se3_exp(np.array([0.0, ty, 0.0, 0.0, 0.0, 0.0]))[:3]
        for level in (3, 2, 1, 0):
            o1 = po.level_iteration(oref, ocur, level, T34, first=True, mode=mode)
            o2 = po.level_iteration(oref, ocur, level, T34, P_prev=o1["P"], first=False, mode=mode)
            without_q3 = po.level_iteration(oref, ocur, level, T34, first=True, mode=mode & ~po.Q_DROP_ODD)
            q3_seen += without_q3["n"] == o1["n"] + 1
            for o, P_prev, first in ((o1, None, True), (o2, o1["P"], False)):
                g = trk.level_iteration(gref, gcur, level, T34, P_prev=P_prev, first=first)
                assert g["n"] == o["n"] and g["n_selected"] == o["n_selected"], (seed, ty, level, first)
                e = dict(cov=rel_max(g["cov"], o["cov"]), P=rel_max(g["P"], o["P"]), ll=abs(g["neg_ll"] - o["neg_ll"]) / abs(o["neg_ll"]),
                         A=rel_max(g["A"], o["A"]), b=rel_max(g["b"], o["b"]))
                for k in worst:
                    worst[k] = max(worst[k], e[k])
                assert e["cov"] <= 1e-5 and e["P"] <= 1e-5 and e["ll"] <= 1e-6 and e["A"] <= 1e-5 and e["b"] <= 1e-5, (seed, ty, level, first, e)
    print("ref_compat %d: worst %s; states where Q3 dropped a constraint: %d" % (compat, worst, q3_seen))
    assert q3_seen >= 1


def test_default_schedule_is_self_consistent():
    """variant 8 (contracted arithmetic, its own residuals): on a first pass the rank formula and the Q7 tail applied to the GPU's own
    residual plane give the GPU's scale_cov (1e-5) and -ll (1e-6)"""
    ctx = context(8, 0, 1)
    pair = cm.synth(1234, 640, 480)
    gref, gcur = gpu_pyramids(ctx, pair, 4)
    trk = d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx)
    T34 = po.se3_exp(np.array([0.0, -0.03, 0.0, 0.0, 0.0, 0.0]))[:3]
    for level in (3, 2, 1, 0):
        g = trk.level_iteration(gref, gcur, level, T34, first=True, want_residuals=True)
        r = g["residuals"].reshape(-1, 2)
        r = r[~np.isnan(r[:, 0])].astype(np.float64)
        n = len(r)
        assert n == g["n"]
        lead = r[0:n:2]                                        # the first residual of every pair, used twice (Q6); an odd n: once
        weight = np.full(len(lead), 2.0)
        if n % 2:
            weight[-1] = 1.0
        S = np.array([(weight * lead[:, 0] ** 2).sum(), (weight * lead[:, 0] * lead[:, 1]).sum(), (weight * lead[:, 1] ** 2).sum()])
        cov = S / (n - 3)
        assert rel_max(g["cov"], cov) <= 1e-5
        P = np.asarray(g["P"], np.float64)
        q = np.einsum("ki,ij,kj->k", r, P, r)
        kept = n // 50 * 50
        ll = 0.5 * n * np.log(np.linalg.det(P)) - 3.5 * np.log1p(0.2 * q[:kept]).sum()
        assert abs(g["neg_ll"] + ll) <= 1e-6 * abs(ll), (level, g["neg_ll"], -ll)


# the table of the issue: pairs and levels (first, last)
REF_PAIRS = [(1234, 640, 480, 3, 0), (5, 640, 480, 3, 1), (7, 640, 480, 3, 1), (55, 320, 240, 2, 0)]


def oracle_and_reference(pair, cfg):
    """the oracle's match in the target mode (+ Q1) and the reference's own match(), both on this host's CPU"""
    I0, Z0 = pair["grey_ref"].astype(np.float32), po.convert_raw_depth(pair["depth_ref"])
    I1, Z1 = pair["grey_cur"].astype(np.float32), po.convert_raw_depth(pair["depth_cur"])
    r = po.ref_match(I0, Z0, I1, Z1, pair["K"], cm.oracle_config_from(cfg, po.REF_SSE))
    oref, ocur = cm.oracle_pyramids(pair, cfg.FirstLevel + 1)
    o = po.match(oref, ocur, cm.oracle_config_from(cfg, TARGET_COMPAT))
    return o, r


def distances(I, LL, T, other):
    return rel_max(I, other["information"]), abs(LL - other["loglik"]) / abs(other["loglik"]), cm.twist_matrix_error(T, other["T"])


def check_against_oracle_and_reference(g, o, r, label, margin=(2e-3, 5e-5, 5e-7)):
    """The engine follows the oracle's target match (I within 2e-3 of its largest entry, LL 5e-5, twist 5e-7); against the reference's
    own match it is held to the issue's bounds (I 5e-3, LL 1e-4, twist 1e-6) or, where the oracle's target match is itself further
    from the reference than that (its Q1 is the host CPU's _mm_rcp_ps table, Q2 round-toward-zero is not reproduced), to the oracle's
    own distance plus the engine-to-oracle bounds"""
    go, gr, orf = distances(*g, o), distances(*g, r), distances(o["information"], o["loglik"], o["T"], r)
    print("%s: engine-oracle I %.2e LL %.2e twist %.2e | engine-reference I %.2e LL %.2e twist %.2e | oracle-reference I %.2e LL %.2e twist %.2e"
          % ((label,) + go + gr + orf))
    assert go[0] <= margin[0] and go[1] <= margin[1] and go[2] <= margin[2], (label, go)
    assert gr[0] <= max(5e-3, orf[0] + margin[0]) and gr[1] <= max(1e-4, orf[1] + margin[1]) and gr[2] <= max(1e-6, orf[2] + margin[2]), (label, gr, orf)
    return gr, orf


@pytest.mark.parametrize("seed,w,h,first,last", REF_PAIRS)
def test_whole_match_against_the_oracle_and_the_reference(seed, w, h, first, last):
    """One pair: "ref_compat" + "ref_order" under variant 8 (the default, what DVO_HIP_REF_COMPAT=1 DVO_HIP_REF_ORDER=1 give an unmodified
    executable) and variant 7, against the oracle's target match and the reference's own match() (oracle/_ref); "ref_compat" alone is
    printed beside them and must be at least ten times further from the reference's Information"""
    if po.ref_lib() is None:
        pytest.skip("oracle/_ref is not built")
    pair = cm.synth(seed, w, h)
    cfg = d.Config(FirstLevel=first, LastLevel=last, MaxIterationsPerLevel=100, Precision=5e-7)
    o, r = oracle_and_reference(pair, cfg)
    alone = None
    for variant, order in ((8, 0), (8, 1), (7, 1)):
        ctx = context(variant, 1, order, resident=0)
        gref, gcur = gpu_pyramids(ctx, pair, first + 1)
        g = d.DenseTracker(cfg, ctx).match_batch_arrays([gref], [gcur])
        res = (g["information"][0], g["loglik"][0], g["T"][0])
        if order == 0:
            alone = distances(*res, r)
            print("seed %d, ref_compat alone: engine-reference I %.2e LL %.2e twist %.2e" % ((seed,) + alone))
            continue
        gr, _ = check_against_oracle_and_reference(res, o, r, "seed %d %dx%d variant %d" % (seed, w, h, variant))
        assert gr[0] < alone[0] / 10


def test_batch_sample_against_the_oracle_and_the_reference():
    """32 pairs of the benchmark's 1024-pair batch (seeds 0 .. 31), aligned in ONE batch on the default schedule with "ref_compat" +
    "ref_order", pair by pair against the oracle's target match and the reference's own match()"""
    if po.ref_lib() is None:
        pytest.skip("oracle/_ref is not built")
    from dvo_slam_amd import datagen
    n = 32
    b = datagen.synth_batch(0, n, 640, 480)
    cfg = d.Config(FirstLevel=3, LastLevel=0, MaxIterationsPerLevel=100, Precision=5e-7)
    ctx = context(8, 1, 1)
    cam = d.RgbdCameraPyramid(640, 480, b["K"], ctx)
    cam.build(4)
    refs = [cam.create_raw(b["grey_ref"][i], b["depth_ref"][i]) for i in range(n)]
    curs = [cam.create_raw(b["grey_cur"][i], b["depth_cur"][i]) for i in range(n)]
    g = d.DenseTracker(cfg, ctx).match_batch_arrays(refs, curs)
    # Pair by pair the three implementations -- engine, oracle target mode, reference -- lie up to ~1e-2 apart in every direction
    # (measured: pair 28 engine-reference 1.5e-4, oracle-reference 1.0e-2; pair 6 engine-oracle 5.4e-3, engine-reference 1.8e-3): a rank
    # shift by one constraint at the finest level re-pairs half the residuals of Q6, and each one's own rounding (the reference's Q2, the
    # oracle's float64 pairing, the engine's f16 Gram) decides where it happens.  So the engine is held, pair by pair, to ten times closer
    # than "ref_compat" alone (0.2), and over the sample to be as close to the reference as the oracle's target mode is.
    I_gr, I_or, LL_gr, LL_or = [], [], [], []
    for i in range(n):
        pair = dict(grey_ref=b["grey_ref"][i], depth_ref=b["depth_ref"][i], grey_cur=b["grey_cur"][i], depth_cur=b["depth_cur"][i], K=b["K"])
        o, r = oracle_and_reference(pair, cfg)
        gr, orf = distances(g["information"][i], g["loglik"][i], g["T"][i], r), distances(o["information"], o["loglik"], o["T"], r)
        print("batch pair %d: engine-reference I %.2e LL %.2e twist %.2e | oracle-reference I %.2e LL %.2e twist %.2e" % ((i,) + gr + orf))
        assert gr[0] <= 2e-2 and gr[1] <= 2.5e-4 and gr[2] <= 1e-6, (i, gr)
        I_gr.append(gr[0]); I_or.append(orf[0]); LL_gr.append(gr[1]); LL_or.append(orf[1])
    print("32-pair batch against the reference: Information engine median %.2e worst %.2e, oracle target median %.2e worst %.2e; "
          "LogLikelihood engine median %.2e, oracle %.2e" % (np.median(I_gr), np.max(I_gr), np.median(I_or), np.max(I_or), np.median(LL_gr), np.median(LL_or)))
    assert np.median(I_gr) <= 1.25 * np.median(I_or) and np.median(LL_gr) <= 1.25 * np.median(LL_or)


def test_dropin_graph_chi2_against_the_reference(tmp_path):
    """The reference's benchmark_slam_graph (keyframe_graph.cpp unmodified, one thread) on the engine: the chi2 of the loop closures it
    has in common with the reference's own run -- edges that carry the alignment's Information -- median ratio engine / reference, for the
    default mode, "ref_compat", and "ref_compat" + "ref_order" (environment variables: the executable sets no options).  The last is the
    closest to 1."""
    from test_dropin import _loop_closures, _loop_folder, _run_graph_target, _target, need_dropin
    need_dropin()
    exe, ref = _target("benchmark_slam_graph"), _target("benchmark_slam_graph_ref")
    root_ref, root_hip = str(tmp_path / "ref"), str(tmp_path / "hip")
    _loop_folder(root_ref)
    _loop_folder(root_hip)
    single = ["_use_multithreading:=false"]
    _, _, edge_r, _ = _run_graph_target(ref, root_ref, "ref", extra=single)
    ratios = {}
    for tag, env in (("default", {}), ("ref_compat", {"DVO_HIP_REF_COMPAT": "1"}),
                     ("ref_compat + ref_order", {"DVO_HIP_REF_COMPAT": "1", "DVO_HIP_REF_ORDER": "1"})):
        _, _, edge, _ = _run_graph_target(exe, root_hip, tag.replace(" ", "").replace("+", "_"), env=env, extra=single)
        common = sorted(i for i in _loop_closures(edge) & _loop_closures(edge_r) if edge_r[i][3] > 0)
        ratios[tag] = float(np.median([edge[i][3] / edge_r[i][3] for i in common]))
        print("%s: %d common loop closures, median chi2 ratio engine / reference %.4f" % (tag, len(common), ratios[tag]))
    best = min(ratios, key=lambda k: abs(np.log(ratios[k])))
    assert best == "ref_compat + ref_order", ratios


def test_options_and_counter():
    ctx = d.Context(0)
    for bad in (-1, 2):
        with pytest.raises(Exception):
            ctx.set_option("ref_order", bad)
    ctx.set_option("variant", 5)
    with pytest.raises(Exception):
        ctx.set_option("ref_order", 1)
    ctx.set_option("variant", 7)
    ctx.set_option("ref_order", 1)
    for other in (0, 5, 6, 9):
        with pytest.raises(Exception):
            ctx.set_option("variant", other)
    ctx.set_option("variant", 8)
    pair = cm.synth(1234, 320, 240)
    gref, gcur = gpu_pyramids(ctx, pair, 3)
    trk = d.DenseTracker(d.Config(FirstLevel=2, LastLevel=0), ctx)
    before = ctx.counter("ref_order_passes")
    res = trk.match_batch_arrays([gref], [gcur])
    after = ctx.counter("ref_order_passes")
    assert after - before >= res["n_iterations"][0] >= 3
    ctx.set_option("ref_order", 0)
    trk.match_batch_arrays([gref], [gcur])
    assert ctx.counter("ref_order_passes") == after


def test_environment_variable_in_a_child_process():
    code = ("import dvo_slam_amd as d\n"
            "ctx = d.Context(0)\n"
            "ctx.set_option('variant', 5)\n")
    env = dict(os.environ, DVO_HIP_REF_ORDER="1")
    # the option is on from the start: a variant it does not run under is refused
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=cm.ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "ref_order" in (p.stdout + p.stderr)
    env.pop("DVO_HIP_REF_ORDER")
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=cm.ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr


def _records(ctx, refs, curs, first=3, last=0):
    return d.DenseTracker(d.Config(FirstLevel=first, LastLevel=last), ctx).match_batch_arrays(refs, curs)


def test_no_edited_planes_left_behind():
    """on, match, off: the records equal a fresh context's bit for bit (Q3's edited reference planes are built again)"""
    pairs = [cm.synth(s, 320, 240) for s in (1234, 7, 55)]
    ctx = context(8, 0, 0)
    frames = [gpu_pyramids(ctx, p, 4) for p in pairs]
    refs, curs = [f[0] for f in frames], [f[1] for f in frames]
    before = _records(ctx, refs, curs)
    ctx.set_option("ref_order", 1)
    on = _records(ctx, refs, curs)
    ctx.set_option("ref_order", 0)
    off = _records(ctx, refs, curs)
    fresh = context(8, 0, 0)
    fframes = [gpu_pyramids(fresh, p, 4) for p in pairs]
    clean = _records(fresh, [f[0] for f in fframes], [f[1] for f in fframes])
    for k in ("T", "information", "loglik"):
        assert np.array_equal(off[k], clean[k]) and np.array_equal(before[k], clean[k]), k
    assert not np.array_equal(on["information"], clean["information"])


def test_deterministic_pair_alone_and_in_a_batch():
    ctx = context(8, 1, 1, deterministic=1)
    pairs = [cm.synth(100 + s, 320, 240) for s in range(32)]
    frames = [gpu_pyramids(ctx, p, 4) for p in pairs]
    refs, curs = [f[0] for f in frames], [f[1] for f in frames]
    batch = _records(ctx, refs, curs)
    for i in (0, 13, 31):
        alone = _records(ctx, [refs[i]], [curs[i]])
        for k in ("T", "information", "loglik"):
            assert np.array_equal(alone[k][0], batch[k][i]), (i, k)


def test_toggle_on_reference_frames_without_a_raw_copy():
    """Reference frames ingested straight into their role without a copy of their raw planes (option "keep_raw_copy" 0) cannot have a
    plane built again: switching "ref_order" on and off again puts back the pixels Q3 cleared, and the records equal the first run's"""
    import ctypes as C
    from dvo_slam_amd import datagen
    d.default_context()                                        # (the HIP runtime the library loaded: device buffers from it)
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    hip = C.CDLL(loaded[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    ptrs = []

    def to_device(arr):
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), arr.nbytes) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0
        ptrs.append(p)
        return p.value
    n, w, h = 6, 320, 240
    ctx = context(8, 0, 0)
    cfg = d.Config(FirstLevel=2, LastLevel=0)
    trk = d.DenseTracker(cfg, ctx)
    cam = d.RgbdCameraPyramid(w, h, po.FR1_K * 0.5, ctx)
    cam.build(3)
    b = datagen.synth_batch(300, n, w, h)
    g = to_device(np.concatenate([b["grey_ref"], b["grey_cur"]]))
    z = to_device(np.concatenate([b["depth_ref"], b["depth_cur"]]))
    gp, zp = [g + i * w * h for i in range(2 * n)], [z + 2 * i * w * h for i in range(2 * n)]
    frames = [cam.create_raw_device(gp[i], zp[i]) for i in range(2 * n)]
    ctx.set_option("keep_raw_copy", 0)
    d.update_raw_device_batch(frames[:n], gp[:n], zp[:n], role="reference", config=cfg)
    ctx.set_option("keep_raw_copy", 1)
    d.update_raw_device_batch(frames[n:], gp[n:], zp[n:], role="current", config=cfg)

    def raw(out):
        return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("T", "information", "loglik", "n_iterations"))
    before = raw(trk.match_batch_arrays(frames[:n], frames[n:]))
    ctx.set_option("ref_order", 1)
    on = raw(trk.match_batch_arrays(frames[:n], frames[n:]))
    ctx.set_option("ref_order", 0)
    after = raw(trk.match_batch_arrays(frames[:n], frames[n:]))
    ctx.set_option("ref_order", 1)
    again = raw(trk.match_batch_arrays(frames[:n], frames[n:]))
    assert after == before and again == on and on != before
    del frames, trk
    for p in ptrs:
        hip.hipFree(p)
