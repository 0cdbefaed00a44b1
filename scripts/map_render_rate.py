"""Cost of rendering the keyframe map (profiles/map_render.md).  Prints one JSON line.

The input of scripts/keyframe_map_rate.py: N keyframes of 640 x 480 (one surface seen again and again) under poses along a short
trajectory, fused at leaf 0.01.  The map is rendered into 1 and into 16 views of 640 x 480 at poses along the same trajectory.  Per view
count: the HIP-event times of the three kernels (k_render_fill, k_map_render, k_render_resolve: dvo_hip_time_map_render records an event
around each launch on the context's stream and returns the medians over --reps renders), the whole call KeyframeMap.render to device and
to host memory with HIP events around the call, and -- what a caller would otherwise do to look at the map -- KeyframeMap.extract to the
host on the same run.  The number of covered-pixel updates (one 8-byte atomic each) is counted on the host yardstick
(tests/test_map_render.py, render_host) from the device map's own extraction, and the device planes are compared with it.
--host also prints the one-thread host time of that yardstick.  DVO_HIP_LIBRARY names another build for the A/B of the plain-load form
(make -C dvo_slam_amd/csrc FLAGS_map_render=-DDVO_RENDER_PRELOAD=1 in a copy of the tree).

    python scripts/map_render_rate.py [--frames 50] [--leaf 0.01] [--capacity 4194304] [--reps 20] [--warmup 3] [--host]
"""
import argparse
import ctypes as C
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


def pose_at(i):
    T = np.eye(4)
    th = 0.001 * i
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
    T[:3, 3] = [0.004 * i, 0.001 * i, 0.002 * i]
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
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
    K = np.ascontiguousarray(pair["K"], np.float32)
    cam = d.RgbdCameraPyramid(W, H, K, ctx)
    cam.build(1)
    frames = d.FrameSet([cam.create(np.roll(I0, (i % 7, 3 * i), (0, 1)), Z0) for i in range(n)])
    m = d.KeyframeMap(ctx, a.leaf, a.capacity)
    m.insert(frames, np.stack([pose_at(i) for i in range(n)]))
    stats = m.stats()

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        call()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end)

    def spread(v):
        return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}

    params = d.render_params_struct()
    out = {"frames": n, "width": W, "height": H, "leaf": a.leaf, "reps": a.reps, "library": _lib.LIB_PATH, "stats": stats,
           "timing": "kernels: HIP events around each launch (dvo_hip_time_map_render, medians); calls: HIP events on the context's stream around the call",
           "views": {}}
    xyzi, counts, keys = m.extract(sort=True)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_map_render as tmr
    for n_views in (1, 16):
        views = np.ascontiguousarray(np.stack([pose_at((n - 1) * k / max(n_views - 1, 1) + 0.5) for k in range(n_views)]))
        ms = (C.c_float * 3)()
        for reps in (a.warmup, a.reps):
            ctx.check(ctx._lib.dvo_hip_time_map_render(ctx.ptr, m.ptr, n_views, W, H, K.ctypes.data_as(C.POINTER(C.c_float)),
                                                       views.ctypes.data_as(C.POINTER(C.c_double)), C.byref(params), max(reps, 1), ms))
        calls = {"render_device": lambda: m.render(K, W, H, views, device=True), "render_host": lambda: m.render(K, W, H, views),
                 "extract_host": lambda: m.extract()}
        times = {k: [] for k in calls}
        for rep in range(a.warmup + a.reps):
            for name, call in calls.items():
                t = timed(call)
                if rep >= a.warmup:
                    times[name].append(t)
        t0 = time.perf_counter()
        want = tmr.render_host(xyzi, counts, a.leaf, K, W, H, views, want_updates=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = m.render(K, W, H, views)
        rec = {"kernel_ms": {"k_render_fill": round(ms[0], 4), "k_map_render": round(ms[1], 4), "k_render_resolve": round(ms[2], 4)},
               "call_ms": {k: spread(v) for k, v in times.items()}, "covered_pixel_updates": want[2],
               "filled_share": round(float((~tmr.holes(got[1])).mean()), 4), "equals_host": bool(tmr.same_bits(got, want[:2]))}
        if a.host:
            rec["host_render_ms"] = round(host_ms, 2)
        out["views"][str(n_views)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
