"""Cost of colour in the keyframe map (profiles/keyframe_map_colour.md).  Prints one JSON line.

N keyframes of 640 x 480 (the input of scripts/keyframe_map_update_rate.py, with a colour image each) go into a grey map and into a
coloured one (KeyframeMap(colour=True)).  Per repetition and per map, ALTERNATING between the two so that both see the same drift of the
machine, each step timed with HIP events on the context's stream around the call (which includes the call's own small transfers and
its read-back of the map's counters):
  insert     KeyframeMap.clear (not timed), then insert of all N keyframes in one launch;
  extract    KeyframeMap.extract to device arrays (the coloured map: with the colour records);
  render     one 640 x 480 view from the middle keyframe's pose (KeyframeMap.render / render_colour to device planes).
Medians over the repetitions.  `--grey-only` runs the grey half alone: with DVO_HIP_LIBRARY naming the library of another commit it
measures that commit's grey map with this script (an A/B of two builds alternates invocations of the two).
    rocprofv3 --kernel-trace --stats -- python scripts/keyframe_map_colour_rate.py ...
gives the kernels' own times over the same loop.

    python scripts/keyframe_map_colour_rate.py [--frames 64] [--level 0] [--leaf 0.01] [--capacity 4194304] [--reps 15] [--warmup 3] [--grey-only]
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
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grey-only", action="store_true")
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
    rng = np.random.default_rng(5)
    frames, poses, images = [], [], []
    for i in range(n):
        I = np.roll(I0, (i % 7, 3 * i), (0, 1))
        frames.append(cam.create(I, Z0))
        # a colour image whose grey is roughly the frame's intensity: smooth, not noise
        images.append(np.stack([np.clip(I + s, 0, 255).astype(np.uint8) for s in rng.integers(-20, 21, 3)], axis=-1))
        T = np.eye(4)
        th = 0.001 * i
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
        T[:3, 3] = [0.004 * i, 0.001 * i, 0.002 * i]
        poses.append(T)
    poses = np.stack(poses)
    maps = {"grey": d.KeyframeMap(ctx, a.leaf, a.capacity)}
    if not a.grey_only:
        d.set_colour_batch(frames, images, "bgr8")
        maps["colour"] = d.KeyframeMap(ctx, a.leaf, a.capacity, colour=True)
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
        if name == "grey":
            return [("insert", lambda: m.insert(frames, poses, a.level)), ("extract", lambda: m.extract(device=True)),
                    ("render", lambda: m.render(K0, W, H, view, device=True))]
        return [("insert", lambda: m.insert(frames, poses, a.level)), ("extract", lambda: m.extract(device=True, colour=True)),
                ("render", lambda: m.render_colour(K0, W, H, view, device=True))]

    times = {name: {"insert": [], "extract": [], "render": []} for name in maps}
    for rep in range(a.warmup + a.reps):
        for name, m in maps.items():                               # grey, colour, grey, colour, ...
            m.clear()
            for step, call in steps_of(name, m):
                ms = timed(call)
                if rep >= a.warmup:
                    times[name][step].append(ms)
    stats = {name: m.stats() for name, m in maps.items()}
    out = {"frames": n, "width": W >> a.level, "height": H >> a.level, "level": a.level, "leaf": a.leaf, "reps": a.reps,
           "library": _lib.LIB_PATH, "timing": "HIP events on the context's stream around each call; grey and coloured runs alternate",
           "stats": {name: {k: s[k] for k in ("occupied", "points", "dropped", "updates", "capacity")} for name, s in stats.items()},
           "ms": {name: {step: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}
                         for step, v in t.items()} for name, t in times.items()}}
    if "colour" in maps:
        grey, colour = maps["grey"].extract(sort=True), maps["colour"].extract(sort=True, colour=True)
        out["grey_part_equal"] = bool(np.array_equal(grey[2], colour[2]) and np.array_equal(grey[1], colour[1]) and
                                      np.array_equal(grey[0].view(np.uint32), colour[0].view(np.uint32)))
        out["colour_over_grey"] = {step: round(out["ms"]["colour"][step]["median"] / out["ms"]["grey"][step]["median"], 3)
                                   for step in ("insert", "extract", "render")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
