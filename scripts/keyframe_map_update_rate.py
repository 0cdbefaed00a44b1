"""Cost of keeping the keyframe map consistent with the pose graph (profiles/keyframe_map_update.md).  Prints one JSON line.

N keyframes of 640 x 480 (the input of scripts/keyframe_map_rate.py) lie in a map.  Per repetition, each timed with HIP events on the
context's stream around the call (which includes the call's own small transfers and its read-back of the map's counters):
  move       `--moved` keyframes re-posed by a small twist (KeyframeMap.move: one launch), then moved back (not timed);
  remove     the same keyframes removed (KeyframeMap.remove), then inserted again (timed as insert_back);
  rehash     KeyframeMap.rehash at the same capacity, behind a removal that left vacant slots;
  rebuild    KeyframeMap.clear + insert of all N keyframes: what a map that cannot follow the pose graph pays for any of the above.
The comparison that matters is `move` of one keyframe against `rebuild`.  The kernels' own times come from
    rocprofv3 --kernel-trace --stats -- python scripts/keyframe_map_update_rate.py ...
over the same loop (k_map_insert covers inserts, removals and moves; k_map_rehash; k_map_clear).

    python scripts/keyframe_map_update_rate.py [--frames 50] [--moved 1] [--level 0] [--leaf 0.01] [--capacity 4194304] [--reps 20] [--warmup 3]
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
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--moved", type=int, default=1)
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n, k = a.frames, max(1, min(a.moved, a.frames))
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
    which = [int(x) for x in np.linspace(0, n - 1, k).round()] if k > 1 else [n // 2]
    sel = [frames[i] for i in which]
    old = poses[which]
    twist = np.eye(4)
    twist[0, 1], twist[1, 0], twist[:3, 3] = -0.002, 0.002, [0.003, -0.002, 0.001]
    new = old @ twist
    m = d.KeyframeMap(ctx, a.leaf, a.capacity)
    m.insert(frames, poses, a.level)

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        call()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end)

    def rebuild():
        m.clear()
        m.insert(frames, poses, a.level)

    steps = [("move", lambda: m.move(sel, old, new, a.level)), (None, lambda: m.move(sel, new, old, a.level)),
             ("remove", lambda: m.remove(sel, old, a.level)), ("rehash", lambda: m.rehash()),
             ("insert_back", lambda: m.insert(sel, old, a.level)), ("rebuild", rebuild)]
    times = {name: [] for name, _ in steps if name}
    vacant_before_rehash = None
    for rep in range(a.warmup + a.reps):
        for name, call in steps:
            if name == "rehash":
                vacant_before_rehash = m.stats()["vacant"]
            ms = timed(call)
            if name and rep >= a.warmup:
                times[name].append(ms)
    # the moved map against the rebuilt one
    m.move(sel, old, new, a.level)
    moved = m.extract(sort=True)
    stats_moved = m.stats()
    after = poses.copy()
    after[which] = new
    m.clear()
    m.insert(frames, after, a.level)
    rebuilt = m.extract(sort=True)
    equal = bool(np.array_equal(moved[2], rebuilt[2]) and np.array_equal(moved[1], rebuilt[1]) and
                 np.array_equal(moved[0].view(np.uint32), rebuilt[0].view(np.uint32)))
    out = {"frames": n, "moved": k, "width": W >> a.level, "height": H >> a.level, "level": a.level, "leaf": a.leaf, "reps": a.reps,
           "library": _lib.LIB_PATH, "timing": "HIP events on the context's stream around each call", "stats_after_move": stats_moved,
           "vacant_before_rehash": vacant_before_rehash, "moved_equals_rebuilt": equal,
           "ms": {name: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}
                  for name, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
