"""Cost of the registering ingest (profiles/depth_registration.md).  Prints one JSON line.

An ingest loop of N frames of 640 x 480 per call, grey8 image + u16 depth from device planes of their own (nothing comes from the
caches), ingested straight into the CURRENT role (dvo_hip_frames_update_raw_device_as).  --kind picks the frames' state for the whole
process, so that one `rocprofv3 --kernel-trace --stats -- python scripts/depth_registration_rate.py --kind K` holds one loop's kernels:
    plain   no rig, no lens (also what an older build named by DVO_HIP_LIBRARY can run: the parent commit's, for the A/B)
    rig     the Kinect-like depth rig (25 mm baseline, 0.6 degrees, fx_d = 1.10 fx): k_depth_fill + k_depth_register ahead of the ingest
    lens    the fr1-like plumb-bob lens: k_rectify ahead of the ingest -- the yardstick, a pass over comparable bytes on the same frames
Each call is also timed with HIP events on the context's stream around the call and a download of one 80 x 60 plane of the batch's
first frame, which makes that stream wait for the build stream (scripts/lens_ingest_rate.py times the lens ingest the same way).

    python scripts/depth_registration_rate.py --kind rig [--frames 256] [--reps 10] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dvo_slam_amd as d  # noqa: E402
from dvo_slam_amd import _lib, datagen  # noqa: E402

W, H = 640, 480
FR1_D = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633, 0.0, 0.0, 0.0]


def ptrs(t):
    step = t[0].numel() * t.element_size()
    return d.device_pointer_array([t.data_ptr() + i * step for i in range(t.shape[0])])


def kinect_rig(K):
    K = np.asarray(K, np.float64)
    axis = np.array([0.3, 0.9, 0.316])
    axis /= np.linalg.norm(axis)
    th = np.deg2rad(0.6)
    O = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) + np.sin(th) * O + (1 - np.cos(th)) * (O @ O)
    T[:, 3] = [-0.025, 0.001, 0.003]
    return K * np.array([1.10, 1.10, 1.004, 0.993]), T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["plain", "rig", "lens"], default="plain")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = a.frames
    ctx = d.default_context()
    L = ctx._lib
    stream = torch.cuda.ExternalStream(L.dvo_hip_context_stream(ctx.ptr))
    pair = datagen.synth_pair(3, W, H)
    g = torch.from_numpy(pair["grey_ref"]).cuda()
    z = torch.from_numpy(pair["depth_ref"].astype(np.int16)).cuda()
    shift = lambda t, i: torch.roll(t, shifts=(i % 97, 3 * (i // 97)), dims=(0, 1))   # noqa: E731
    grey = torch.stack([shift(g, i) for i in range(n)]).contiguous()
    raw = torch.stack([shift(z, i) for i in range(n)]).contiguous()
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(4)
    frames = d.FrameSet([cam.create_raw(pair["grey_ref"], pair["depth_ref"]) for _ in range(n)])
    if a.kind == "rig":
        d.set_depth_rig_batch(frames.pyramids, *kinect_rig(pair["K"]))
    elif a.kind == "lens":
        K_raw = (np.asarray(pair["K"], np.float64) * np.array([1.013, 1.009, 0.994, 1.011])).astype(np.float32)
        d.set_lens_batch(frames.pyramids, K_raw, FR1_D)
    cfg = d.Config(FirstLevel=3, LastLevel=0).to_c()
    probe = np.empty((H >> 3, W >> 3), np.float32)
    pg, pr = ptrs(grey), ptrs(raw)

    def ingest():
        ctx.check(L.dvo_hip_frames_update_raw_device_as(ctx.ptr, n, frames.handles, pg, pr, 2e-4, 0, C.byref(cfg)))
        ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, frames.handles[0], 3, 0, probe.ctypes.data_as(C.POINTER(C.c_float))))

    for _ in range(a.warmup):
        ingest()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        ingest()
        end.record(stream)
        end.synchronize()
        times.append(start.elapsed_time(end))
    out = {"kind": a.kind, "frames": n, "width": W, "height": H, "calls": a.reps + a.warmup, "library": _lib.LIB_PATH,
           "timing": "HIP events on the context's stream",
           "ms": {"median": round(float(np.median(times)), 4), "min": round(min(times), 4), "max": round(max(times), 4)}}
    if a.kind == "rig":
        out["depth_registrations"] = ctx.counter("depth_registrations")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
