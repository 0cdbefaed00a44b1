"""Cost of warping frames under a pose (profiles/frame_warp.md).  Prints one JSON line.

--frames distinct frames of 640 x 480 (the scene of scripts/map_render_rate.py, rolled) are warped as 1 item and as --items items, every
item under a transform of its own along a short trajectory; the items cycle through the frames (128 frames hold 315 MB of {I, Z} pairs,
more than the Infinity Cache).  Per item count and per entry point -- the inverse warp without and with the difference plane, the forward
warp in both modes -- the whole C-ABI call into preallocated DEVICE planes is timed with HIP events on the context's stream around the
call, which ends in a wait for that stream: argument checks, the frame table's upload and every launch are inside.  The bytes a pixel
must move are counted from the shapes (inverse: 4 or 8 B read coalesced, 32 B of taps, 8 or 12 B stored; forward: 8 B read, 8 B filled,
16 B resolved, and one 8-byte atomic per covered pixel, counted on the host yardstick for item 0) and priced at the HBM peak of
8.0 TB/s: achieved_fraction is that count over the call time, a whole-call figure, not a kernel's.  Item 0's planes are compared with
the host build of frame_warp.h (tests/test_frame_warp.py).

    python scripts/frame_warp_rate.py [--items 1024] [--frames 128] [--level 0] [--reps 20] [--warmup 3]
"""
import argparse
import ctypes as C
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
HBM_PEAK = 8.0e12


def transform_at(i):
    T = np.eye(4)
    th = 0.002 + 0.00001 * i
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
    T[:3, 3] = [0.01 + 0.00002 * i, -0.005, -0.02 - 0.00001 * i]
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--level", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = d.default_context()
    L = ctx._lib
    stream = torch.cuda.ExternalStream(L.dvo_hip_context_stream(ctx.ptr))
    pair = datagen.synth_pair(3, W, H)
    I0 = pair["grey_ref"].astype(np.float32)
    Z0 = pair["depth_ref"].astype(np.float32) * np.float32(2e-4)
    Z0[pair["depth_ref"] == 0] = np.nan
    K = np.ascontiguousarray(pair["K"], np.float32)
    cam = d.RgbdCameraPyramid(W, H, K, ctx)
    cam.build(a.level + 1)
    frames = [cam.create(np.roll(I0, (i % 7, 3 * i), (0, 1)), np.roll(Z0, (i % 5, 2 * i), (0, 1))) for i in range(a.frames)]
    w, h = W >> a.level, H >> a.level
    pixels = w * h

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        rc = call()
        end.record(stream)
        end.synchronize()
        ctx.check(rc)
        return start.elapsed_time(end)

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_frame_warp as tfw
    img = frames[0].level(a.level)
    I_0, Z_0, K_l = np.array(img.intensity), np.array(img.depth), np.array(img.K)
    img1 = frames[1 % a.frames].level(a.level)
    out = {"width": w, "height": h, "level": a.level, "frames": a.frames, "reps": a.reps, "library": _lib.LIB_PATH, "hbm_peak_Bps": HBM_PEAK,
           "timing": "HIP events on the context's stream around the whole C-ABI call (device planes; the call waits for the stream)", "items": {}}
    for n in (1, a.items):
        T = np.ascontiguousarray(np.stack([transform_at(i) for i in range(n)]))
        tp = T.ctypes.data_as(C.POINTER(C.c_double))
        raster = d.tracker._handles([frames[i % a.frames] for i in range(n)])
        sampled = d.tracker._handles([frames[(i + 1) % a.frames] for i in range(n)])
        planes = [torch.empty((n, h, w), dtype=torch.float32, device="cuda:%d" % ctx.device) for _ in range(3)]
        ptrs = [d.device_pointer_array([p[i].data_ptr() for i in range(n)]) for p in planes]
        params = {mode: d.warp_params_struct(mode=mode) for mode in ("nearest", "splat")}
        calls = {
            "inverse": (lambda: L.dvo_hip_frames_warp_inverse(ctx.ptr, n, raster, sampled, tp, a.level, None, ptrs[0], ptrs[1], None, 1), 4 + 32 + 8),
            "inverse_difference": (lambda: L.dvo_hip_frames_warp_inverse(ctx.ptr, n, raster, sampled, tp, a.level, None, ptrs[0], ptrs[1], ptrs[2], 1),
                                   8 + 32 + 12),
            "forward_nearest": (lambda: L.dvo_hip_frames_warp_forward(ctx.ptr, n, raster, tp, a.level, C.byref(params["nearest"]), ptrs[0], ptrs[1], 1),
                                8 + 8 + 16),
            "forward_splat": (lambda: L.dvo_hip_frames_warp_forward(ctx.ptr, n, raster, tp, a.level, C.byref(params["splat"]), ptrs[0], ptrs[1], 1),
                              8 + 8 + 16),
        }
        rec = {}
        for name, (call, bytes_per_pixel) in calls.items():
            times = [timed(call) for _ in range(a.warmup + a.reps)][a.warmup:]
            got = [p[0].cpu().numpy() for p in planes]
            if name.startswith("inverse"):
                want = tfw.warp_inverse_host(I_0, Z_0, np.array(img1.intensity), np.array(img1.depth), K_l, K_l, T[0], difference=True)
                same = tfw.same_bits(got[:3 if name.endswith("difference") else 2], want[:3 if name.endswith("difference") else 2])
                extra = {}
            else:
                mode = tfw.SPLAT if name.endswith("splat") else tfw.NEAREST
                want = tfw.warp_forward_host(I_0, Z_0, K_l, T[0], mode, want_updates=True)
                same = tfw.same_bits(got[:2], want[:2])
                extra = {"covered_pixel_updates_item0": want[2], "filled_share_item0": round(float((~tfw.holes(want[1])).mean()), 4)}
            ms = float(np.median(times))
            moved = float(bytes_per_pixel) * pixels * n
            rec[name] = dict({"call_ms": {"median": round(ms, 4), "min": round(float(np.min(times)), 4), "max": round(float(np.max(times)), 4)},
                              "bytes_per_pixel": bytes_per_pixel, "bytes": moved, "achieved_Bps": round(moved / (ms * 1e-3), 1),
                              "achieved_fraction_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 4), "equals_host_item0": bool(same)}, **extra)
        out["items"][str(n)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
