"""Cost of surface normals in the keyframe map (profiles/keyframe_map_normals.md).  Prints one JSON line.

N keyframes of 640 x 480 (the input of scripts/keyframe_map_colour_rate.py) go into a map without normals and into one with them
(KeyframeMap(normals=True)).  Per repetition and per map, ALTERNATING between the two so that both see the same drift of the machine,
each step timed with HIP events on the context's stream around the call (which includes the call's own small transfers and its read-back
of the map's counters):
  insert     KeyframeMap.clear (not timed), then insert of all N keyframes in one launch;
  extract    KeyframeMap.extract to device arrays (the map with normals: with the normal records);
  render     one 640 x 480 view from the middle keyframe's pose (KeyframeMap.render / render_normals to device planes);
  frames     (once per repetition) normals_batch of all N keyframes to device arrays: k_frame_normals, beside world_points_batch.
Medians over the repetitions.  `--plain-only` runs the half without normals alone: with DVO_HIP_LIBRARY naming the library of another
commit it measures that commit's map with this script (an A/B of two builds alternates invocations of the two).
    rocprofv3 --kernel-trace --stats -- python scripts/keyframe_map_normals_rate.py ...
gives the kernels' own times over the same loop.

    python scripts/keyframe_map_normals_rate.py [--frames 16] [--level 0] [--leaf 0.01] [--capacity 4194304] [--reps 15] [--warmup 3] [--plain-only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dvo_slam_amd as d  # noqa: E402
from dvo_slam_amd import _lib, datagen  # noqa: E402

W, H = 640, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    n = a.frames
    ctx = d.default_context()
    stream = torch.cuda.ExternalStream(ctx._lib.dvo_hip_context_stream(ctx.ptr))
    pair = datagen.synth_pair(3, W, H)
    I0 = pair["grey_ref"].astype(np.float32)
    Z0 = pair["depth_ref"].astype(np.float32) * np.float32(2e-4)
    Z0[pair["depth_ref"] == 0] = np.nan
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(a.level + 1)
    frames, poses = [], []
    for i in range(n):
        frames.append(cam.create(np.roll(I0, (i % 7, 3 * i), (0, 1)), Z0))
        T = np.eye(4)
        th = 0.001 * i
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
        T[:3, 3] = [0.004 * i, 0.001 * i, 0.002 * i]
        poses.append(T)
    poses = np.stack(poses)
    maps = {"plain": d.KeyframeMap(ctx, a.leaf, a.capacity)}
    if not a.plain_only:
        maps["normals"] = d.KeyframeMap(ctx, a.leaf, a.capacity, normals=True)
    view = poses[n // 2][None]
    K0 = np.asarray(pair["K"], np.float32)

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        call()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end)

    def steps_of(name, m):
        if name == "plain":
            return [("insert", lambda: m.insert(frames, poses, a.level)), ("extract", lambda: m.extract(device=True)),
                    ("render", lambda: m.render(K0, W, H, view, device=True))]
        return [("insert", lambda: m.insert(frames, poses, a.level)), ("extract", lambda: m.extract(device=True, normals=True)),
                ("render", lambda: m.render_normals(K0, W, H, view, device=True))]

    times = {name: {"insert": [], "extract": [], "render": []} for name in maps}
    organised = {"world_points": [], "normals": []}
    for rep in range(a.warmup + a.reps):
        for name, m in maps.items():                               # plain, normals, plain, normals, ...
            m.clear()
            for step, call in steps_of(name, m):
                ms = timed(call)
                if rep >= a.warmup:
                    times[name][step].append(ms)
        for name, call in (("world_points", d.world_points_batch), ("normals", None if a.plain_only else d.normals_batch)):
            if call is not None:
                ms = timed(lambda: call(frames, poses, a.level, device=True))
                if rep >= a.warmup:
                    organised[name].append(ms)

    def summary(v):
        return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}

    stats = {name: m.stats() for name, m in maps.items()}
    out = {"frames": n, "width": W >> a.level, "height": H >> a.level, "level": a.level, "leaf": a.leaf, "reps": a.reps,
           "library": _lib.LIB_PATH, "timing": "HIP events on the context's stream around each call; the two maps alternate",
           "stats": {name: {k: s[k] for k in ("occupied", "points", "dropped", "updates", "capacity")} for name, s in stats.items()},
           "ms": {name: {step: summary(v) for step, v in t.items()} for name, t in times.items()},
           "organised_ms": {name: summary(v) for name, v in organised.items() if v}}
    if "normals" in maps:
        plain, normals = maps["plain"].extract(sort=True), maps["normals"].extract(sort=True, normals=True)
        out["plain_part_equal"] = bool(np.array_equal(plain[2], normals[2]) and np.array_equal(plain[1], normals[1]) and
                                       np.array_equal(plain[0].view(np.uint32), normals[0].view(np.uint32)))
        out["voxels_with_a_normal"] = int((normals[3][:, 3] > 0).sum())
        out["normals_over_plain"] = {step: round(out["ms"]["normals"][step]["median"] / out["ms"]["plain"][step]["median"], 3)
                                     for step in ("insert", "extract", "render")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
