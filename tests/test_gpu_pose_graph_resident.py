"""GPU tier: the resident schedule of the pose-graph optimiser (dvo_hip_graph_optimize_batch, option "graph_resident"; k_pg_resident in
dvo_slam_amd/csrc/pose_graph.hip) -- a graph optimised from start to end by one workgroup of one launch, a batch by one workgroup each
-- against the host yardstick of tests/test_pose_graph.py, bit for bit throughout.
  1. every ending in one launch: every entry of EDGE_RUNS whose graph is resident-sized (ring_600, three vertex blocks and six edge
     blocks, under its five parameter sets; three_blocks; small, two, half_turns and the four chains), each in a graph of its own with
     its own parameters, plus full_block, the two graphs without edges and one with a fixed and an isolated vertex.  The batch mixes
     graphs the kernel solves out of LDS (two, half_turns, the one with the untouched vertices) with graphs it solves from memory
     (ring_600, three_blocks, small, full_block, the chains): both instances of the kernel's body run in the one launch;
  2. the three converging graphs of the CPU tier at the default parameters;
  3. the batch of (1) in reversed order: the same bits, whatever a graph's workgroup index and neighbours;
  4. 300 graphs of 12 vertices: more workgroups than compute units;
  5. the state a batch leaves: set_poses and the launch path on the same object, the other way round, a second batch from the estimate;
  6. option "graph_resident" and counter "graph_resident_solves";
  7. refusals, which change nothing."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import dvo_slam_amd as d
import test_pose_graph as tpg
from dvo_slam_amd import _lib
from test_gpu_pose_graph import assert_same_bits
from test_gpu_pose_graph_edges import assert_same_optimisation
from test_pose_graph_resident import build_batch_facade_check

pytestmark = pytest.mark.gpu


def resident_sized(g):
    return len(g["start"]) <= _lib.GRAPH_RESIDENT_MAX_VERTICES and len(g["edges"][0]) <= _lib.GRAPH_RESIDENT_MAX_EDGES


def untouched_graph():
    """the noisy graph with vertex 30 fixed as well and a vertex 60 without an edge"""
    g = tpg.noisy_graph()
    start = np.concatenate([g["start"], [tpg.pose([5, 5, 5], [0.1, 0.2, 0.3])]])
    fixed = np.concatenate([g["fixed"], [False]])
    fixed[30] = True
    return dict(g, start=start, fixed=fixed)


@functools.lru_cache(maxsize=None)
def host_run(name):
    """(graph, parameters, report, poses, weights) of the yardstick on one of the cases (1) adds to EDGE_RUNS: computed once, shared"""
    g, params = dict(full_block=(lambda: tpg.edge_graph("full_block"), dict(max_iterations=4)),
                     no_edges_1=(lambda: tpg.edge_graph("no_edges_1"), {}),
                     no_edges_300=(lambda: tpg.edge_graph("no_edges_300"), {}),
                     untouched=(untouched_graph, dict(max_iterations=6)))[name]
    g = g()
    h = tpg.load(tpg.HostGraph(), g)
    report = h.optimize(**params)
    out = g, params, report, h.poses(), h.edge_stats()[1]
    h.close()
    return out


@functools.lru_cache(maxsize=None)
def every_ending():
    """name -> (graph, parameters, (report, poses, weights) of the yardstick), in the order of the batch"""
    cases = {}
    for name, (graph, params, _, _) in tpg.EDGE_RUNS.items():
        if resident_sized(tpg.edge_graph(graph)):
            g, report, poses, weights = tpg.edge_run(name)
            cases[name] = (g, params, (report, poses, weights))
    for name in ("full_block", "no_edges_1", "no_edges_300", "untouched"):
        g, params, report, poses, weights = host_run(name)
        cases[name] = (g, params, (report, poses, weights))
    return cases


def run_batch(cases, order, ctx=None):
    """the cases, each in a PoseGraph of its own, through ONE optimize_batch in the given order: name -> (report, poses, weights)"""
    graphs = [tpg.load(d.PoseGraph(ctx), cases[name][0]) for name in order]
    reports = d.PoseGraph.optimize_batch(graphs, params=[cases[name][1] for name in order])
    out = {name: (report, g.poses(), g.edge_stats()[1]) for name, g, report in zip(order, graphs, reports)}
    for g in graphs:
        g.close()
    return out


@functools.lru_cache(maxsize=None)
def forward_batch():
    cases = every_ending()
    ctx = d.default_context()
    before = ctx.counter("graph_resident_solves")
    got = run_batch(cases, list(cases))
    assert ctx.counter("graph_resident_solves") == before + len(cases)
    return got


def test_every_ending_in_one_launch_equals_the_yardstick():
    cases = every_ending()
    assert sorted(set(tpg.EDGE_RUNS) - set(cases)) == ["long_tree"] and len(cases) == len(tpg.EDGE_RUNS) - 1 + 4
    assert sum(tpg.EDGE_RUNS[name][0] == "ring_600" for name in cases if name in tpg.EDGE_RUNS) == 5
    g = tpg.edge_graph("ring_600")
    assert (len(g["start"]), len(g["edges"][0])) == (600, 1500)       # three vertex blocks, six edge blocks
    got = forward_batch()
    seen_cg, seen_lm = set(), set()
    for name, (g, params, want) in cases.items():
        report = got[name][0]
        cg = [r["cg_status"] for r in report["records"]]
        print(name, report["status"], report["iterations"], report["accepted"], report["cg_iterations"], report["final_cost"],
              {s: cg.count(s) for s in sorted(set(cg))})
        assert_same_optimisation(got[name], want, (name,))
        if name in tpg.EDGE_RUNS:                                     # what the case is there for, as the CPU tier asserts it of the yardstick
            _, _, lm_status, cg_statuses = tpg.EDGE_RUNS[name]
            assert lm_status is None or report["status"] == lm_status, name
            assert all(s in cg for s in cg_statuses), name
        seen_cg.update(cg)
        seen_lm.add(report["status"])
    assert {"zero_rhs", "cholesky", "breakdown", "iteration_cap", "converged"} <= seen_cg
    assert {"damping_overflow", "iteration_cap", "nothing_to_do"} <= seen_lm
    assert got["full_block"][0]["iterations"] >= 1 and got["full_block"][0]["accepted"] >= 1
    for name in ("no_edges_1", "no_edges_300"):
        report, poses, weights = got[name]
        assert report["status"] == "nothing_to_do" and report["iterations"] == 0 and report["records"] == [] and report["final_cost"] == 0.0
        assert_same_bits(poses, cases[name][0]["start"], (name, "poses"))
        assert weights.shape == (0,)
    report, poses, _ = got["untouched"]
    start = cases["untouched"][0]["start"]
    assert report["accepted"] >= 1 and not np.array_equal(poses[10], start[10])
    for v in (0, 30, 60):
        assert np.array_equal(poses[v], start[v]), v


def test_the_converging_graphs_in_one_batch_equal_the_yardstick():
    names = ["noise_free", "noisy", "outliers"]
    runs = {name: tpg.yardstick_run(name) for name in names}
    graphs = [tpg.load(d.PoseGraph(), runs[name][0]) for name in names]
    reports = d.PoseGraph.optimize_batch(graphs)
    for name, g, report in zip(names, graphs, reports):
        _, want_report, want_poses, want_weights, _ = runs[name]
        assert_same_optimisation((report, g.poses(), g.edge_stats()[1]), (want_report, want_poses, want_weights), (name,))
        assert report["status"] == ("stalled" if name == "noise_free" else "converged") and report["accepted"] >= 1     # (ten rejected trials at the optimum)
    assert sorted(graphs[2].remove_outliers(0.1)) == sorted(runs["outliers"][0]["planted"])
    for g in graphs:
        g.close()


def test_a_graph_depends_neither_on_its_workgroup_nor_on_its_neighbours():
    cases = every_ending()
    forward = forward_batch()
    backward = run_batch(cases, list(cases)[::-1])
    for name in cases:
        assert_same_optimisation(backward[name], forward[name], (name, "reversed"))
    alone = run_batch(cases, ["many_workgroups"])
    assert_same_optimisation(alone["many_workgroups"], forward["many_workgroups"], ("many_workgroups", "alone"))


def test_more_graphs_than_compute_units():
    count = 300
    assert count > d.default_context().counter("compute_units") > 0
    inputs = [tpg.graph_of(12, *tpg.ring_with_chords(12, 20, np.random.default_rng(1000 + seed)), 2000 + seed) for seed in range(count)]
    graphs = [tpg.load(d.PoseGraph(), g) for g in inputs]
    reports = d.PoseGraph.optimize_batch(graphs)
    host = tpg.HostGraph()
    iterations = set()
    for k, (g, dev, report) in enumerate(zip(inputs, graphs, reports)):
        tpg.load(host, g)
        want = host.optimize()
        assert_same_optimisation((report, dev.poses(), dev.edge_stats()[1]), (want, host.poses(), host.edge_stats()[1]), ("graph", k))
        iterations.add(report["iterations"])
        dev.close()
    host.close()
    assert len(iterations) > 1 and min(iterations) >= 1               # (they do not all end at the same time)


def test_the_state_a_batch_leaves_is_the_launch_paths():
    g = tpg.edge_graph("ring_600")
    params = dict(max_iterations=3)
    host = tpg.load(tpg.HostGraph(), g)
    want = host.optimize(**params), host.poses(), host.edge_stats()[1]
    assert want[0]["accepted"] == 3                                   # (an odd number of swaps: the estimate is in the second pose buffer)
    # a batch, back to the start, the launch path; and the other way round
    for first in ("batch", "launch"):
        dev = tpg.load(d.PoseGraph(), g)
        for step in ((first,) + (("launch",) if first == "batch" else ("batch",))):
            report = d.PoseGraph.optimize_batch([dev], params)[0] if step == "batch" else dev.optimize(**params)
            assert_same_optimisation((report, dev.poses(), dev.edge_stats()[1]), want, (first, "then", step))
            dev.set_poses(g["start"])
            assert_same_bits(dev.poses(), g["start"], (first, step, "set_poses"))
        dev.close()
    # a second and a third batch continue from the estimate, as a second HostGraph.optimize does; then the launch path takes over
    dev = tpg.load(d.PoseGraph(), g)
    assert_same_optimisation((d.PoseGraph.optimize_batch([dev], params)[0], dev.poses(), dev.edge_stats()[1]), want, ("call", 0))
    for call in (1, 2, 3):
        want_report = host.optimize(**params)
        report = d.PoseGraph.optimize_batch([dev], params)[0] if call < 3 else dev.optimize(**params)
        assert_same_optimisation((report, dev.poses(), dev.edge_stats()[1]), (want_report, host.poses(), host.edge_stats()[1]), ("call", call))
    lin_dev, lin_host = dev.linearise(), host.linearise()
    for key in lin_host:
        assert_same_bits(np.atleast_1d(lin_dev[key]), np.atleast_1d(lin_host[key]), ("afterwards", key))
    dev.close()
    host.close()


def test_max_records_keeps_the_first_trials_of_each_graph():
    cases = every_ending()
    names = ["small", "cg_cap_2", "no_edges_1"]
    graphs = [tpg.load(d.PoseGraph(), cases[name][0]) for name in names]
    reports = d.PoseGraph.optimize_batch(graphs, params=[cases[name][1] for name in names], max_records=2)
    for name, g, report in zip(names, graphs, reports):
        want = cases[name][2][0]
        assert {k: v for k, v in report.items() if k != "records"} == {k: v for k, v in want.items() if k != "records"}, name
        assert report["records"] == want["records"][:2], name
        g.close()


def test_the_option_sends_a_resident_sized_graph_through_the_resident_kernel():
    ctx = d.Context(0)
    try:
        g, want_report, want_poses, want_weights = tpg.edge_run("small")
        large = tpg.graph_of(1025, *tpg.ring_with_chords(1025, 1500, np.random.default_rng(81)), 82)
        large_params = dict(max_iterations=2, cg_max_iterations=5)
        host = tpg.load(tpg.HostGraph(), large)
        want_large = host.optimize(**large_params), host.poses(), host.edge_stats()[1]
        host.close()
        assert ctx.counter("graph_resident_solves") == 0
        ctx.set_option("graph_resident", 1)
        dev = tpg.load(d.PoseGraph(ctx), g)
        got = dev.optimize(**tpg.EDGE_RUNS["small"][1]), dev.poses(), dev.edge_stats()[1]
        assert_same_optimisation(got, (want_report, want_poses, want_weights), ("small", "graph_resident"))
        assert ctx.counter("graph_resident_solves") == 1
        tpg.load(dev, large)
        got = dev.optimize(**large_params), dev.poses(), dev.edge_stats()[1]
        assert_same_optimisation(got, want_large, ("1025 vertices", "graph_resident"))
        assert got[0]["iterations"] == 2 and ctx.counter("graph_resident_solves") == 1
        ctx.set_option("graph_resident", 0)
        tpg.load(dev, g)
        got = dev.optimize(**tpg.EDGE_RUNS["small"][1]), dev.poses(), dev.edge_stats()[1]
        assert_same_optimisation(got, (want_report, want_poses, want_weights), ("small", "launch path"))
        assert ctx.counter("graph_resident_solves") == 1
        with pytest.raises(d.DvoHipError):
            ctx.set_option("graph_resident", 2)
        dev.close()
    finally:
        ctx.close()


def test_refusals_change_nothing():
    ctx, other = d.default_context(), d.Context(0)
    L = ctx._lib
    small, two = tpg.edge_graph("small"), tpg.edge_graph("two")
    good = [tpg.load(d.PoseGraph(ctx), small), tpg.load(d.PoseGraph(ctx), two), tpg.load(d.PoseGraph(ctx), tpg.edge_graph("half_turns")),
            tpg.load(d.PoseGraph(ctx), tpg.edge_graph("full_block"))]
    too_many_vertices = tpg.load(d.PoseGraph(ctx), tpg.graph_of(1025, *tpg.ring_with_chords(1025, 1100, np.random.default_rng(83)), 84))
    too_many_edges = tpg.load(d.PoseGraph(ctx), tpg.graph_of(50, *tpg.ring_with_chords(50, 4097, np.random.default_rng(85)), 86))
    foreign = tpg.load(d.PoseGraph(other), two)
    empty = d.PoseGraph(ctx)
    assert (too_many_vertices.n, too_many_edges.m) == (1025, 4097)
    everyone = good + [too_many_vertices, too_many_edges, foreign]
    before = [(g.poses(), g.edge_stats()) for g in everyone]
    solves = ctx.counter("graph_resident_solves")

    def call(graphs, params=None, reports=True, records=None, max_records=0, count=None):
        ptrs = (C.c_void_p * len(graphs))(*[None if g is None else g.ptr.value for g in graphs])
        prm = None if params is None else (_lib.GraphParams * len(params))(*params)
        reps = (_lib.GraphReport * len(graphs))() if reports else None
        return L.dvo_hip_graph_optimize_batch(ctx.ptr, len(graphs) if count is None else count, ptrs, prm, reps, records, max_records)

    bad_third = [d.graph_params_struct() for _ in range(4)]
    bad_third[2].cg_tolerance = 0.0
    recs = (_lib.GraphIteration * 8)()
    for what, rc in (("1025 vertices", call(good[:2] + [too_many_vertices] + good[2:])),
                     ("4097 edges", call(good + [too_many_edges])),
                     ("a duplicate", call(good + [good[1]])),
                     ("another context", call(good[:3] + [foreign])),
                     ("a bad parameter", call(good, bad_third)),
                     ("a null entry", call(good[:1] + [None] + good[1:])),
                     ("no vertices", call(good + [empty])),
                     ("no graph", call(good, count=0)),
                     ("no reports", call(good, reports=False)),
                     ("negative max_records", call(good, records=recs, max_records=-1)),
                     ("records missing", call(good, max_records=2))):
        assert rc == _lib.ERR_INVALID, what
        assert b"graph_optimize_batch" in L.dvo_hip_last_error(ctx.ptr), what
    assert ctx.counter("graph_resident_solves") == solves
    for g, (poses, (chi2, weights)) in zip(everyone, before):
        assert_same_bits(g.poses(), poses, ("poses",))
        now = g.edge_stats()
        assert_same_bits(now[0], chi2, ("chi2",))
        assert_same_bits(now[1], weights, ("weights",))
    # ... and the good ones still optimise: the same bits as the yardstick
    reports = d.PoseGraph.optimize_batch(good[:2], params=[tpg.EDGE_RUNS["small"][1], tpg.EDGE_RUNS["reuse_two"][1]])
    for g, report, name in zip(good, reports, ("small", "reuse_two")):
        assert_same_optimisation((report, g.poses(), g.edge_stats()[1]), tpg.edge_run(name)[1:], (name, "after the refusals"))
    for g in everyone + [empty]:
        g.close()
    other.close()


def test_cpp_facade_batch_equals_its_own_optimize_on_the_device():
    d.build()
    out = subprocess.run([build_batch_facade_check(), "device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
