"""GPU tier: the pose-graph optimiser where only pose_graph.hip and capi_graph.inc decide (the workgroups' protocol, the partials' trees,
the endings, the buffers), against the host yardstick of tests/test_pose_graph.py, bit for bit throughout.  The inputs are that module's
edge_graphs(); its CPU tier asserts that each does what it is here for.
  1. stage by stage (linearise, multiply, edge_stats):
       full_block    (256, 256)        one full workgroup, one partial
       three_blocks  (513, 1281)       3 and 6 partials, padded to 4 and 8; the last vertex workgroup holds one lane
       ring_65537    (65537, 65537)    257 partials, padded to 512: partials_tree's chunk is 2 and lane 128 takes a short one
       few_vertices  (90, 65537)       the long tree over the edges alone; incidence lists of about 1450
       ring_196613   (196613, 196613)  769 partials, padded to 1024: chunk 4, lane 192 takes one of its four
       half_turns    (70, 150)         errors that turn by 125 .. 200 degrees: the three other branches of pg_quat; s / delta^2 from
                                       1e-10 to 1e8 in pg_log1p
       no_edges      (1, 0), (300, 0)  and a graph that had 1000 edges set to none;
  2. whole optimisations: CG solves over three workgroups; the long tree inside a solve (the scale of the gain through k_pg_reduce's
     second operand); every ending -- the CG's iteration cap at 1, 2, 3 and 4 iterations (both rows of rz and both of kPgP0 / kPgP1 as
     the last), zero_rhs, a Cholesky failure in the second workgroup alone, breakdown, the damping's overflow, the optimisation's cap;
     steps beyond the unit quaternion;
  3. one object through (65537, 65537), (2, 1), (513, 1281) and (65537, 65537) again, against fresh objects; two graphs driven in turn on
     the default context, against their solo runs; a second and a third optimisation on one object, from the pose buffer the first left
     the estimate in."""
import numpy as np
import pytest

import dvo_slam_amd as d
import test_pose_graph as tpg
from test_gpu_pose_graph import assert_same_bits

pytestmark = pytest.mark.gpu

LONG = 65536                                                          # from here on one damping per case: each multiply linearises again


def assert_same_stages(got, want, what):
    """two results of linearise() or multiply(): every array and every scalar the same bits"""
    assert sorted(got) == sorted(want)
    for key in want:
        assert_same_bits(np.atleast_1d(got[key]), np.atleast_1d(want[key]), what + (key,))


def assert_same_optimisation(got, want, what):
    """(report, poses, weights) twice: report and records equal, poses and weights the same bits"""
    assert {k: v for k, v in got[0].items() if k != "records"} == {k: v for k, v in want[0].items() if k != "records"}, what
    assert got[0]["records"] == want[0]["records"], what
    assert_same_bits(got[1], want[1], what + ("poses",))
    assert_same_bits(got[2], want[2], what + ("weights",))


def direction(n):
    return np.random.default_rng(5).normal(size=(n, 6))


@pytest.mark.parametrize("name", ["full_block", "three_blocks", "ring_65537", "few_vertices", "ring_196613", "half_turns"])
def test_stages_equal_the_yardstick_bit_for_bit_at_the_edges_of_the_trees(name):
    g = tpg.edge_graph(name)
    n, m = len(g["start"]), len(g["edges"][0])
    host, dev = tpg.load(tpg.HostGraph(), g), tpg.load(d.PoseGraph(), g)
    assert (n, m) == dict(full_block=(256, 256), three_blocks=(513, 1281), ring_65537=(65537, 65537), few_vertices=(90, 65537),
                          ring_196613=(196613, 196613), half_turns=(70, 150))[name]
    want, got = host.linearise(), dev.linearise()
    assert_same_stages(got, want, (name, "linearise"))
    chi2 = want["chi2"]
    p = direction(n)
    for damping in ((0.0, 3.7) if max(n, m) < LONG else (3.7,)):
        want, got = host.multiply(damping, p), dev.multiply(damping, p)
        assert_same_stages(got, want, (name, "multiply", damping))
    assert np.any(want["y"] != 0) and not want["y"][g["fixed"]].any() and want["pty"] != 0
    s, w = dev.edge_stats()
    assert_same_bits(s, chi2, (name, "edge_stats"))
    assert np.all(w[g["delta"] == 0] == 1.0) and np.all(w[g["delta"] > 0] < 1.0)
    dev.close()
    host.close()


@pytest.mark.parametrize("name", ["no_edges_1", "no_edges_300", "emptied"])
def test_a_graph_without_edges_runs_no_kernel_over_edges_and_leaves_no_error(name):
    ctx = d.Context(0)                                                # (a context of its own: no earlier test has left an error in it)
    g = tpg.edge_graph("no_edges_300" if name == "emptied" else name)
    n = len(g["start"])
    host, dev = tpg.load(tpg.HostGraph(), g), d.PoseGraph(ctx)
    if name == "emptied":                                             # 1000 edges, a run on them, then none
        full = tpg.graph_of(n, *tpg.ring_with_chords(n, 1000, np.random.default_rng(77)), 50 + n)     # (seed 50 + n: the poses of no_edges(n))
        tpg.load(dev, full)
        assert dev.optimize(max_iterations=2)["iterations"] == 2
        dev.set_poses(g["start"])
        none = np.zeros(0, np.int32)
        assert ctx._lib.dvo_hip_graph_set_edges(ctx.ptr, dev.ptr, 0, None, None, None, None, None) == d._lib.OK       # m = 0 needs no array
        dev.set_edges(none, none, np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
        assert dev.m == 0
    else:
        tpg.load(dev, g)
    want, got = host.linearise(), dev.linearise()
    assert_same_stages(got, want, (name, "linearise"))
    assert got["cost"] == 0.0 and got["error"].shape == (0, 6)
    p = direction(n)
    for damping in (0.0, 3.7):
        want, got = host.multiply(damping, p), dev.multiply(damping, p)
        assert_same_stages(got, want, (name, "multiply", damping))
        assert not got["y"].any() and not got["inverse"].any() and got["pty"] == 0.0
    s, w = dev.edge_stats()
    assert s.shape == w.shape == (0,)
    want, got = host.optimize(), dev.optimize()
    assert got == want and got["status"] == "nothing_to_do" and got["iterations"] == 0 and got["records"] == []
    assert_same_bits(dev.poses(), g["start"], (name, "poses"))
    assert ctx._lib.dvo_hip_last_error(ctx.ptr) == b""
    dev.close()
    host.close()
    ctx.close()


def optimise_on_the_device(name):
    graph, params, _, _ = tpg.EDGE_RUNS[name]
    dev = tpg.load(d.PoseGraph(), tpg.edge_graph(graph))
    out = dev.optimize(**params), dev.poses(), dev.edge_stats()[1]
    dev.close()
    return out


@pytest.mark.parametrize("name", ["many_workgroups", "long_tree", "cg_cap_1", "cg_cap_2", "cg_cap_3", "cg_cap_4", "zero_rhs", "cholesky_in_workgroup_1",
                                  "breakdown", "damping_overflow", "lm_iteration_cap", "large_steps"])
def test_whole_optimisations_equal_the_yardstick_across_workgroups_and_to_every_ending(name):
    g, want_report, want_poses, want_weights = tpg.edge_run(name)
    _, params, lm_status, cg_statuses = tpg.EDGE_RUNS[name]
    got = optimise_on_the_device(name)
    report, poses, _ = got
    seen = [r["cg_status"] for r in report["records"]]
    print(name, report["status"], report["iterations"], report["accepted"], report["cg_iterations"], report["final_cost"],
          {s: seen.count(s) for s in sorted(set(seen))})
    assert_same_optimisation(got, (want_report, want_poses, want_weights), (name,))
    # what the case is here for, as the CPU tier asserts it of the yardstick
    assert lm_status is None or report["status"] == lm_status
    assert all(s in seen for s in cg_statuses)
    if name.startswith("cg_cap_"):
        assert [(r["cg_status"], r["cg_iterations"]) for r in report["records"]] == [("iteration_cap", params["cg_max_iterations"])] * 6
    if name == "zero_rhs":
        assert report["initial_cost"] == 0.0 and report["iterations"] == 1 and report["accepted"] == 0 and np.array_equal(poses, g["start"])
    if name == "long_tree":
        assert report["records"][0]["accepted"] and report["records"][1]["damping"] != report["records"][0]["damping"]
    if name == "large_steps":
        R = poses[:, :3, :3]
        assert np.all(np.isfinite(poses)) and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14     # (the CPU tier's bound for chained updates)
    if len(g["start"]) < LONG:                                        # the same bits from a second, fresh object
        assert_same_optimisation(optimise_on_the_device(name), got, (name, "second run"))


def test_a_second_optimisation_continues_from_the_stepped_pose_buffer():
    """three accepted trials leave the estimate in the second pose buffer; the next call starts there, and set_poses writes there"""
    g = tpg.edge_graph("ring_600")
    host, dev = tpg.load(tpg.HostGraph(), g), tpg.load(d.PoseGraph(), g)
    for call in range(3):
        want, got = host.optimize(max_iterations=3), dev.optimize(max_iterations=3)
        assert got == want and got["accepted"] >= 1, call
        assert_same_bits(dev.poses(), host.poses(), ("call", call, "poses"))
        if call == 0:
            assert got["accepted"] == 3                               # (an odd number of swaps)
        if call == 1:
            for graph in (host, dev):
                graph.set_poses(g["start"])
            assert_same_bits(dev.poses(), g["start"], ("set_poses",))
    assert_same_stages(dev.linearise(), host.linearise(), ("after three calls", "linearise"))
    dev.close()
    host.close()


def drive(dev, graph, run, steps=None):
    """linearise, multiply and the optimisation of EDGE_RUNS[run] on `dev`, loaded with the graph; with `steps`, only those"""
    g = tpg.edge_graph(graph)

    def load():
        tpg.load(dev, g)
    calls = dict(load=load, linearise=dev.linearise, multiply=lambda: dev.multiply(3.7, direction(len(g["start"]))),
                 optimize=lambda: (dev.optimize(**tpg.EDGE_RUNS[run][1]), dev.poses(), dev.edge_stats()[1]))
    return {step: calls[step]() for step in (steps or ("load", "linearise", "multiply", "optimize"))}


def assert_same_drive(got, want, what):
    for step in got:
        if step in ("linearise", "multiply"):
            assert_same_stages(got[step], want[step], what + (step,))
        if step == "optimize":
            assert_same_optimisation(got[step], want[step], what)


def test_one_object_through_large_small_and_large_graphs_equals_fresh_objects():
    stops = [("ring_65537", "long_tree"), ("two", "reuse_two"), ("three_blocks", "reuse_three_blocks"), ("ring_65537", "long_tree")]
    fresh = {}
    for graph, run in stops[:3]:
        dev = d.PoseGraph()
        fresh[graph] = drive(dev, graph, run)
        dev.close()
        assert_same_optimisation(fresh[graph]["optimize"], tpg.edge_run(run)[1:], (graph, "fresh"))
        assert fresh[graph]["optimize"][0]["iterations"] == 2
    reused = d.PoseGraph()
    for stop, (graph, run) in enumerate(stops):
        got = drive(reused, graph, run)
        assert reused.n == len(tpg.edge_graph(graph)["start"]) and reused.m == len(tpg.edge_graph(graph)["edges"][0])
        assert_same_drive(got, fresh[graph], ("stop %d" % stop, graph))
    reused.close()


def test_two_graphs_driven_in_turn_on_one_context_equal_their_solo_runs():
    cases = [("ring_600", "many_workgroups"), ("small", "small")]
    solo = []
    for graph, run in cases:
        dev = d.PoseGraph()
        solo.append(drive(dev, graph, run))
        solo[-1]["again"] = drive(dev, graph, run, ("linearise",))["linearise"]       # (at the optimised poses)
        dev.close()
        assert_same_optimisation(solo[-1]["optimize"], tpg.edge_run(run)[1:], (graph, "solo"))
    ctx = d.default_context()
    pair = [d.PoseGraph(ctx), d.PoseGraph(ctx)]
    turns = [{}, {}]
    for step in ("load", "linearise", "multiply", "optimize"):
        for k, (graph, run) in enumerate(cases):
            turns[k].update(drive(pair[k], graph, run, (step,)))
    for k, (graph, run) in reversed(list(enumerate(cases))):
        turns[k]["again"] = drive(pair[k], graph, run, ("linearise",))["linearise"]
    for k, (graph, _) in enumerate(cases):
        assert_same_drive(turns[k], solo[k], (graph, "in turn"))
        assert_same_stages(turns[k]["again"], solo[k]["again"], (graph, "in turn", "again"))
        assert not np.array_equal(turns[k]["again"]["error"], turns[k]["linearise"]["error"])
        pair[k].close()
