"""Cost of the keyframe map (profiles/keyframe_map.md).  Prints one JSON line.

N keyframes of 640 x 480 (float planes created once, so nothing but the map's own kernels runs in the loop) under poses along a short
trajectory; per repetition: KeyframeMap.clear + insert of all frames in one call, world_points_batch to device memory, extract to device
memory and extract to the host.  Each call is timed with HIP events on the context's stream around the call -- which includes the
call's own small transfers and waits (an insert reads the map's counters back behind its launch) -- so the kernels' own times come from
    rocprofv3 --kernel-trace --stats -- python scripts/keyframe_map_rate.py ...
over the same loop (k_map_insert, k_world_points, k_map_extract, k_map_clear; the median of the trace's per-launch durations).
DVO_HIP_LIBRARY names another build for the A/B of the insert forms (make -C dvo_slam_amd/csrc FLAGS_cloud_map=-DDVO_MAP_COMBINE_RUNS=0 in
a copy of the tree).  --host also times the host build of cloud_map.h (tests/test_cloud_map.py, one thread) on the same input.

    python scripts/keyframe_map_rate.py [--frames 50] [--level 0] [--leaf 0.01] [--capacity 4194304] [--reps 20] [--warmup 3] [--host]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", action="store_true")
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
        frames.append(cam.create(np.roll(I0, (i % 7, 3 * i), (0, 1)), Z0))   # (one surface seen again and again: overlapping keyframes)
        T = np.eye(4)
        th = 0.001 * i
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
        T[:3, 3] = [0.004 * i, 0.001 * i, 0.002 * i]
        poses.append(T)
    frames, poses = d.FrameSet(frames), np.stack(poses)
    m = d.KeyframeMap(ctx, a.leaf, a.capacity)

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        failed = None
        try:
            call()
        except d.DvoHipError as e:                 # (a full table: the call still ran, DVO_HIP_ERR_CAPACITY is its answer)
            if e.code != _lib.ERR_CAPACITY:
                raise
            failed = e
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end), failed

    steps = {"clear": m.clear, "insert": lambda: m.insert(frames, poses, a.level),
             "world_points_device": lambda: d.world_points_batch(frames, poses, a.level, device=True),
             "extract_device": lambda: m.extract(device=True), "extract_host": lambda: m.extract()}
    times = {k: [] for k in steps}
    capacity_error = False
    for rep in range(a.warmup + a.reps):
        for name, call in steps.items():
            ms, failed = timed(call)
            capacity_error = capacity_error or failed is not None
            if rep >= a.warmup:
                times[name].append(ms)
    stats = m.stats()
    pixels = sum((W >> a.level) * (H >> a.level) for _ in range(n))
    out = {"frames": n, "width": W >> a.level, "height": H >> a.level, "level": a.level, "leaf": a.leaf, "reps": a.reps, "library": _lib.LIB_PATH,
           "timing": "HIP events on the context's stream around each call", "pixels": pixels, "stats": stats, "capacity_error": capacity_error,
           "ms": {k: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)} for k, v in times.items()}}
    if a.host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_cloud_map as tcm
        host = tcm.HostMap(a.leaf, a.capacity)
        planes = []
        for p in frames:
            img = p.level(a.level)
            planes.append((np.array(img.intensity), np.array(img.depth), np.array(img.K)))
        t0 = time.perf_counter()
        for (I, Z, K), T in zip(planes, poses):
            host.insert(I, Z, K, T)
        out["host_insert_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        t0 = time.perf_counter()
        want = host.extract()
        out["host_extract_and_sort_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        got = m.extract(sort=True)
        out["equals_host"] = bool(np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and
                                  np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
