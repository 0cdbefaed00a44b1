"""Cost of a pose-graph optimisation on the device (profiles/pose_graph.md).  Prints one JSON line per graph size.

Synthetic ring-with-loops graphs: n poses on a closed helix, edges i -> i + 1 (the ring, closed) and a loop closure i -> i + n / 8 from
every fourth vertex, measured with 1 cm / 0.005 noise, Cauchy kernel delta = 5 on every edge, vertex 0 fixed, started from the integrated
odometry.  Per size (default 64, 512, 4096, 32768):
  optimize_ms        wall time of PoseGraph.optimize() with the default schedule (the call is synchronous), and what it did;
  per_lm_ms          that over its Levenberg-Marquardt trials;
  cg_iteration_us    the time of one REAL CG iteration (both launches): two runs of `--trials` trials whose solves cannot stop early
                     (cg_tolerance 1e-300) at cg_max_iterations = 32 and 96, their difference over 64 x trials;
  idle_pair_us       the time of a pair of launches that return at once (the solve has ended): the same difference with the default tolerance
                     where the solves end before 32 iterations, else null;
  launches_per_cg_iteration   2 (k_pg_multiply, k_pg_cg_update), by construction;
  multiply_bytes     the algorithmic bytes of one k_pg_multiply: per vertex D (36), z, p_old, p_new, y (6 each) and the incidence words, per
                     incidence entry the block B (36) and the neighbour's z and p_old (12), 8 B each; multiply_gbps_floor = those bytes
                     over cg_iteration_us, a lower bound on the kernel's rate (the vector kernel's time is in the denominator too);
  host_optimize_ms   the host yardstick of tests/test_pose_graph.py on the same graph, one thread, same box -- the same arithmetic, so the
                     same trials and the same bits.
The kernels' own times come from
    rocprofv3 --kernel-trace --stats -- python scripts/pose_graph_rate.py --sizes 4096

--resident: the resident schedule instead (one workgroup per graph, one launch per call: dvo_hip_graph_optimize_batch).  Per size
(default 8, 64, 512 vertices: 10, 80, 640 edges), default schedule, wall clock around the synchronous call, one JSON line:
  launch_ms          one graph (seed 1) by the launch path;
  resident_ms        the same graph by PoseGraph.optimize() under option "graph_resident";
  batch_ms           batches of 16, 256 and 1024 DISTINCT graphs (seeds 1 .. 1024) in one optimize_batch each (no records asked for), and
                     batch_us_per_graph, that over the batch size;
  host_ms            the host yardstick on the graph of seed 1, one thread;
  host_equals_device every graph of every leg against its own yardstick run: poses and report, and the records of a run that asks for
                     them (the yardstick runs spread over --host-threads threads; that time is not reported).

    python scripts/pose_graph_rate.py [--sizes 64,512,4096,32768] [--trials 3] [--no-host] [--host-max-n 4096]
    python scripts/pose_graph_rate.py --resident [--sizes 8,64,512] [--batches 16,256,1024] [--host-threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dvo_slam_amd as d  # noqa: E402


def quat_pose(t, v):
    x, y, z = v
    w = np.sqrt(1.0 - x * x - y * y - z * z)
    X = np.eye(4)
    X[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    X[:3, 3] = t
    return X


def ring_with_loops(n, seed=1):
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / n
    r = n / 20.0                                                     # neighbours about 0.3 m apart
    truth = np.stack([quat_pose([r * np.cos(t), r * np.sin(t), 0.2 * np.sin(3 * t)], [0.0, 0.0, np.sin(t / 4)]) for t in a])
    hop = max(2, n // 8)
    pairs = [(k, (k + 1) % n) for k in range(n)] + [(k, (k + hop) % n) for k in range(0, n, 4)]
    i, j = np.array([p for p, _ in pairs], np.int32), np.array([q for _, q in pairs], np.int32)
    inv = np.linalg.inv(truth)
    noise = np.stack([quat_pose(rng.normal(0, 0.01, 3), rng.normal(0, 0.005, 3)) for _ in pairs])
    Z = inv[i] @ truth[j] @ noise
    W = np.tile(np.diag([1e4] * 3 + [4e4] * 3), (len(pairs), 1, 1))
    start = truth.copy()
    for k in range(1, n):
        start[k] = start[k - 1] @ Z[k - 1]
    fixed = np.zeros(n, bool)
    fixed[0] = True
    return start, fixed, (i, j, Z, W), 5.0


def timed(graph, start, **params):
    graph.set_poses(start)
    t0 = time.perf_counter()
    report = graph.optimize(**params)
    return (time.perf_counter() - t0) * 1e3, report


def same_report(got, want):
    return {k: v for k, v in got.items() if k != "records"} == {k: v for k, v in want.items() if k != "records"}


def resident_leg(n, batches, host_threads):
    from concurrent.futures import ThreadPoolExecutor
    import test_pose_graph as tpg
    count = max(batches)
    inputs = [ring_with_loops(n, seed) for seed in range(1, count + 1)]
    m = len(inputs[0][2][0])
    print("n = %d: %d graphs built" % (n, count), file=sys.stderr, flush=True)

    def host_run(k):
        start, fixed, edges, delta = inputs[k]
        h = tpg.HostGraph()
        h.set_vertices(start, fixed)
        h.set_edges(*edges, delta)
        t0 = time.perf_counter()
        report = h.optimize()
        ms = (time.perf_counter() - t0) * 1e3
        out = report, h.poses(), ms
        h.close()
        return out
    tpg.host_lib()
    host_ms = host_run(0)[2]                                         # (alone: one thread, nothing beside it)
    with ThreadPoolExecutor(host_threads) as pool:
        host = list(pool.map(host_run, range(count)))
    print("n = %d: the yardstick has run" % n, file=sys.stderr, flush=True)
    ctx = d.default_context()
    graphs = []
    for start, fixed, edges, delta in inputs:
        g = d.PoseGraph(ctx)
        g.set_vertices(start, fixed)
        g.set_edges(*edges, delta)
        graphs.append(g)

    def rewind(k):
        for g, (start, _, _, _) in zip(graphs[:k], inputs):
            g.set_poses(start)

    def equal(k, reports, records):
        return all(same_report(r, host[i][0]) and (not records or r["records"] == host[i][0]["records"]) and np.array_equal(graphs[i].poses(), host[i][1])
                   for i, r in enumerate(reports[:k]))
    timed(graphs[0], inputs[0][0], max_iterations=2)                 # warm-up of both paths
    d.PoseGraph.optimize_batch(graphs[:2], dict(max_iterations=2))
    launch_ms, report = timed(graphs[0], inputs[0][0])
    same = equal(1, [report], True)
    ctx.set_option("graph_resident", 1)
    before = ctx.counter("graph_resident_solves")
    resident_ms, resident_report = timed(graphs[0], inputs[0][0])
    same = same and equal(1, [resident_report], True) and ctx.counter("graph_resident_solves") == before + 1
    ctx.set_option("graph_resident", 0)
    batch_ms = {}
    for k in batches:
        rewind(k)
        t0 = time.perf_counter()
        reports = d.PoseGraph.optimize_batch(graphs[:k], max_records=0)
        batch_ms[k] = (time.perf_counter() - t0) * 1e3
        same = same and equal(k, reports, False)
    rewind(count)
    same = same and equal(count, d.PoseGraph.optimize_batch(graphs), True)
    for g in graphs:
        g.close()
    return dict(n=n, m=m, status=report["status"], lm_trials=report["iterations"], cg_iterations=report["cg_iterations"], launch_ms=launch_ms,
                resident_ms=resident_ms, batch_ms={str(k): v for k, v in batch_ms.items()},
                batch_us_per_graph={str(k): v * 1e3 / k for k, v in batch_ms.items()}, host_ms=host_ms, host_equals_device=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--batches", default="16,256,1024")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-max-n", type=int, default=4096)          # (the yardstick's 50 trials of 200 iterations take minutes beyond)
    a = ap.parse_args()
    if a.resident:
        for n in (int(s) for s in (a.sizes or "8,64,512").split(",")):
            print(json.dumps(resident_leg(n, [int(s) for s in a.batches.split(",")], a.host_threads)), flush=True)
        return
    a.sizes = a.sizes or "64,512,4096,32768"
    for n in (int(s) for s in a.sizes.split(",")):
        start, fixed, edges, delta = ring_with_loops(n)
        m = len(edges[0])
        g = d.PoseGraph()
        g.set_vertices(start, fixed)
        g.set_edges(*edges, delta)
        timed(g, start, max_iterations=2)                            # warm-up
        ms, report = timed(g, start)
        full = {k: timed(g, start, max_iterations=a.trials, cg_max_iterations=k, cg_tolerance=1e-300, min_relative_decrease=0.0)[0] for k in (32, 96)}
        early = {k: timed(g, start, max_iterations=a.trials, cg_max_iterations=k, min_relative_decrease=0.0) for k in (32, 96)}
        ended = all(r["cg_iterations"] < 32 for r in early[32][1]["records"]) and early[32][1]["iterations"] == early[96][1]["iterations"] == a.trials
        cg_us = (full[96] - full[32]) * 1e3 / (64 * a.trials)
        multiply_bytes = 8 * (n * (36 + 4 * 6) + 2 * m * (36 + 12)) + 4 * (n + 1 + 2 * m + 2 * m)
        out = dict(n=n, m=m, optimize_ms=ms, status=report["status"], lm_trials=report["iterations"], accepted=report["accepted"],
                   cg_iterations=report["cg_iterations"], per_lm_ms=ms / max(report["iterations"], 1), cg_iteration_us=cg_us,
                   idle_pair_us=(early[96][0] - early[32][0]) * 1e3 / (64 * a.trials) if ended else None, launches_per_cg_iteration=2,
                   multiply_bytes=multiply_bytes, multiply_gbps_floor=multiply_bytes / (cg_us * 1e-6) / 1e9 if cg_us > 0 else None,
                   initial_cost=report["initial_cost"], final_cost=report["final_cost"])
        if not a.no_host and n <= a.host_max_n:
            import test_pose_graph as tpg
            h = tpg.HostGraph()
            h.set_vertices(start, fixed)
            h.set_edges(*edges, delta)
            t0 = time.perf_counter()
            host_report = h.optimize()
            out["host_optimize_ms"] = (time.perf_counter() - t0) * 1e3
            dev_report = timed(g, start)[1]
            out["host_equals_device"] = bool(np.array_equal(h.poses(), g.poses()) and host_report["records"] == dev_report["records"])
        g.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
