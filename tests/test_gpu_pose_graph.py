"""GPU tier: the pose-graph optimiser on the device (include/dvo_hip.h, dvo_hip_graph_*; dvo_slam_amd/csrc/pose_graph.hip) against the host
yardstick of tests/test_pose_graph.py -- the same header compiled by g++ with contraction off, the same incidence lists and trees.
  1. stage by stage, bit for bit: dvo_hip_graph_linearise and dvo_hip_graph_multiply at the smallest shapes where the indexing can go
     wrong: (n, m) = (2, 1); 65 vertices with 64 and 65 edges (across a wavefront); (257, 1000) (several workgroups and their partials);
     a hub of degree 300; a vertex of degree 0; edges in descending and in shuffled order;
  2. the whole optimisation on the three graphs of the CPU tier: poses, report and records bit for bit, and the same again on a second run;
  3. meeting the map: three keyframes inserted at drifted poses, a 3-vertex graph optimised, KeyframeMap.move(old, new): the extraction
     equals a map built at the optimised poses;
  4. argument errors return DVO_HIP_ERR_INVALID and change nothing;
  5. the C++ facade (tests/cpp/pose_graph_facade_check.cpp device)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import dvo_slam_amd as d
import test_pose_graph as tpg
from dvo_slam_amd import _lib
from test_cloud_map import assert_maps_identical
from test_gpu_cloud_map import frames_of, roomy

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same_bits(got, want, what):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        at = np.argwhere(g != w)[0]
        raise AssertionError("%s: first differing word at %s: %r (%#x) against %r (%#x); %d of %d differ" % (
            what, tuple(at), np.asarray(got)[tuple(at)], g[tuple(at)], np.asarray(want)[tuple(at)], w[tuple(at)], int((g != w).sum()), g.size))


def random_graph(n, pairs, seed, kernel_every=3):
    """n random poses, the given (from, to) pairs with measurements a few centimetres off, dense information matrices, a kernel on
    every third edge, every seventh vertex fixed"""
    rng = np.random.default_rng(seed)
    X = np.stack([tpg.random_pose(rng) for _ in range(n)])
    i, j = np.array([a for a, _ in pairs], np.int32), np.array([b for _, b in pairs], np.int32)
    Z = np.stack([np.linalg.inv(X[a]) @ X[b] @ tpg.random_pose(rng, 0.1, 0.05) for a, b in pairs])
    W = np.stack([tpg.spd(rng) for _ in pairs])
    delta = np.where(np.arange(len(pairs)) % kernel_every == 0, 2.0, 0.0)
    fixed = np.arange(n) % 7 == 3
    return X, fixed, i, j, Z, W, delta


def ring_pairs(n, m, rng):
    """m pairs: the ring first, then random chords (repeats allowed: duplicate edges are legal)"""
    pairs = [(a, (a + 1) % n) for a in range(min(n, m))]
    while len(pairs) < m:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            pairs.append((a, b))
    return pairs[:m]


def stage_cases():
    rng = np.random.default_rng(21)
    cases = {"2x1": (2, [(0, 1)]),
             "65x64": (65, ring_pairs(65, 64, rng)),
             "65x65": (65, ring_pairs(65, 65, rng)),
             "257x1000": (257, ring_pairs(257, 1000, rng)),
             "hub300": (320, [(5, v) if v % 2 else (v, 5) for v in range(6, 306)] + ring_pairs(320, 40, rng)),
             "degree0": (70, [(a, b) for a, b in ring_pairs(69, 150, rng)])}           # vertex 69 has no edge
    base = ring_pairs(90, 260, rng)
    cases["descending"] = (90, sorted(base, key=lambda p: (-p[0], -p[1])))
    cases["shuffled"] = (90, [base[k] for k in rng.permutation(len(base))])
    return cases


STAGE_CASES = stage_cases()


@pytest.mark.parametrize("name", sorted(STAGE_CASES))
def test_linearise_and_multiply_equal_the_yardstick_bit_for_bit(name):
    n, pairs = STAGE_CASES[name]
    X, fixed, i, j, Z, W, delta = random_graph(n, pairs, 100 + len(pairs))
    if name == "2x1":
        fixed[:] = [True, False]
    host, dev = tpg.HostGraph(), d.PoseGraph()
    for g in (host, dev):
        g.set_vertices(X, fixed)
        g.set_edges(i, j, Z, W, delta)
    if name == "hub300":
        assert np.bincount(np.concatenate([i, j]), minlength=n)[5] >= 300
    if name == "degree0":
        assert np.bincount(np.concatenate([i, j]), minlength=n)[69] == 0
    want, got = host.linearise(), dev.linearise()
    for key in ("error", "chi2", "weight", "blocks", "gradient"):
        assert_same_bits(got[key], want[key], (name, "linearise", key))
    assert_same_bits([got["cost"]], [want["cost"]], (name, "cost"))
    p = np.random.default_rng(5).normal(size=(n, 6))
    for damping in (0.0 if name != "2x1" else 0.5, 3.7):
        want, got = host.multiply(damping, p), dev.multiply(damping, p)
        for key in ("diagonal", "rhs", "inverse", "y"):
            assert_same_bits(got[key], want[key], (name, "multiply", damping, key))
        assert_same_bits([got["pty"]], [want["pty"]], (name, "pty", damping))
    assert np.any(want["y"] != 0) and not want["y"][fixed].any()
    s, w = dev.edge_stats()
    assert_same_bits(s, host.linearise()["chi2"], (name, "edge_stats"))
    assert np.all(w[delta == 0] == 1.0) and np.all(w[delta > 0] < 1.0)
    dev.close()


@pytest.mark.parametrize("name", ["noise_free", "noisy", "outliers"])
def test_whole_optimisation_equals_the_yardstick_bit_for_bit_and_repeats(name):
    g, want_report, want_poses, want_weights, _ = tpg.yardstick_run(name)
    runs = []
    for _ in range(2):
        dev = tpg.load(d.PoseGraph(), g)
        report = dev.optimize()
        runs.append((report, dev.poses(), dev.edge_stats()[1]))
        dev.close()
    report, poses, weights = runs[0]
    print(name, report["status"], report["iterations"], report["accepted"], report["cg_iterations"], report["final_cost"])
    assert {k: v for k, v in report.items() if k != "records"} == {k: v for k, v in want_report.items() if k != "records"}
    assert report["records"] == want_report["records"]
    assert_same_bits(poses, want_poses, (name, "poses"))
    assert_same_bits(weights, want_weights, (name, "weights"))
    assert runs[1][0] == report
    assert_same_bits(runs[1][1], poses, (name, "second run"))
    if name == "outliers":
        dev = tpg.load(d.PoseGraph(), g)
        dev.optimize()
        assert sorted(dev.remove_outliers(0.1)) == sorted(g["planted"]) and dev.m == len(g["edges"][0]) - 4
        assert dev.edge_stats()[1].min() > 0.1
        dev.close()


def test_nothing_to_do_and_untouched_vertices_on_the_device():
    g = tpg.noisy_graph()
    dev = tpg.load(d.PoseGraph(), dict(g, fixed=np.ones(60, bool)))
    report = dev.optimize()
    assert report["iterations"] == 0 and report["status"] == "nothing_to_do" and report["initial_cost"] == report["final_cost"] > 0
    dev.set_vertices(g["start"], g["fixed"])
    report = dev.optimize()
    assert report["iterations"] == 0 and report["status"] == "nothing_to_do" and np.array_equal(dev.poses(), g["start"])
    start = np.concatenate([g["start"], [tpg.pose([5, 5, 5], [0.1, 0.2, 0.3])]])
    fixed = np.concatenate([g["fixed"], [False]])
    fixed[30] = True
    dev.set_vertices(start, fixed)
    dev.set_edges(*g["edges"])
    assert dev.optimize(max_iterations=4)["accepted"] >= 1
    poses = dev.poses()
    for v in (0, 30, 60):
        assert np.array_equal(poses[v], start[v])
    assert not np.array_equal(poses[10], start[10])
    dev.close()


def test_the_optimised_poses_move_the_keyframe_map():
    ctx, pyramids, truth = frames_of(102, 78, 3)
    level, leaf = 1, 0.02
    drifted = truth.copy()
    drifted[1] = truth[1] @ tpg.pose([0.02, -0.01, 0.015], [0.004, -0.003, 0.002])
    drifted[2] = truth[2] @ tpg.pose([-0.03, 0.02, 0.01], [-0.002, 0.005, 0.003])
    graph = d.PoseGraph(ctx)
    graph.set_vertices(drifted, [True, False, False])
    pairs = [(0, 1), (1, 2), (0, 2)]
    graph.set_edges([a for a, _ in pairs], [b for _, b in pairs], [np.linalg.inv(truth[a]) @ truth[b] for a, b in pairs],
                    [np.diag([1e4] * 3 + [4e4] * 3)] * 3)
    report = graph.optimize()
    new = graph.poses()
    assert report["accepted"] >= 1 and np.abs(new - truth).max() < 1e-9 and np.array_equal(new[0], drifted[0])
    capacity = 4 * roomy(pyramids, new, level, leaf)[1]
    moved, built = d.KeyframeMap(ctx, leaf, capacity), d.KeyframeMap(ctx, leaf, capacity)
    moved.insert(pyramids, drifted, level=level)
    before = moved.extract(sort=True)
    moved.move(pyramids, drifted, new, level=level)
    built.insert(pyramids, new, level=level)
    assert_maps_identical(moved.extract(sort=True), built.extract(sort=True), "move after the optimisation")
    assert moved.stats()["points"] == built.stats()["points"] and moved.stats()["unmatched"] == 0
    assert len(before[2]) != len(built.extract(sort=True)[2]) or not np.array_equal(before[0], built.extract(sort=True)[0])
    for m in (moved, built):
        m.close()
    graph.close()


def test_argument_errors_are_refused_and_change_nothing():
    ctx = d.default_context()
    L = ctx._lib
    g = tpg.noisy_graph()
    dev = tpg.load(d.PoseGraph(ctx), g)
    chi2 = dev.edge_stats()[0]
    i, j, Z, W = (np.ascontiguousarray(a) for a in g["edges"])
    m, dp, ip = len(i), C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def set_edges(i, j, Z, W, delta=None):
        return L.dvo_hip_graph_set_edges(ctx.ptr, dev.ptr, len(i), i.ctypes.data_as(ip), j.ctypes.data_as(ip), Z.ctypes.data_as(dp), W.ctypes.data_as(dp),
                                         None if delta is None else delta.ctypes.data_as(dp))
    bad_index, self_edge, nan_Z, neg_delta = j.copy(), j.copy(), Z.copy(), np.zeros(m)
    bad_index[5], self_edge[7], nan_Z[3, 1, 2], neg_delta[2] = 60, i[7], np.nan, -1.0
    bad_W = W.copy()
    bad_W[9, 2, 2] = np.inf
    for rc in (set_edges(i, bad_index, Z, W), set_edges(i, self_edge, Z, W), set_edges(i, j, nan_Z, W), set_edges(i, j, Z, bad_W),
               set_edges(i, j, Z, W, neg_delta), set_edges(-i - 1, j, Z, W),
               L.dvo_hip_graph_set_vertices(ctx.ptr, dev.ptr, 0, g["start"].ctypes.data_as(dp), None),
               L.dvo_hip_graph_set_poses(ctx.ptr, dev.ptr, 59, g["start"].ctypes.data_as(dp)),
               L.dvo_hip_graph_set_poses(ctx.ptr, dev.ptr, 60, (g["start"] * np.nan).ctypes.data_as(dp)),
               L.dvo_hip_graph_get_poses(ctx.ptr, dev.ptr, 61, g["start"].copy().ctypes.data_as(dp)),
               L.dvo_hip_graph_edge_stats(ctx.ptr, dev.ptr, m - 1, chi2.copy().ctypes.data_as(dp), chi2.copy().ctypes.data_as(dp)),
               L.dvo_hip_graph_optimize(ctx.ptr, dev.ptr, None, None, None, 0)):
        assert rc == _lib.ERR_INVALID
    assert dev.m == m and np.array_equal(dev.edge_stats()[0], chi2) and np.array_equal(dev.poses(), g["start"])
    assert b"graph" in L.dvo_hip_last_error(ctx.ptr)
    dev.close()


def test_cpp_facade_optimises_a_local_map_on_the_device():
    d.build()
    exe = tpg.build_pose_graph_facade_check()
    out = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
