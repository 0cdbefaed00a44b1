"""Cost of the depth filter at ingest (profiles/depth_filter.md).  Prints one JSON line per configuration.

An ingest loop of N frames of 640 x 480 per call, grey8 image + u16 depth (--format u16) or + float depth (--format f32) from device
planes of their own (nothing comes from the caches), ingested straight into the CURRENT role.  --kind picks the frames' state:
    plain    no filter (also what an older build named by DVO_HIP_LIBRARY can run: the parent commit's, for the A/B)
    filter   a depth filter with --radius / --edge-radius / --hole-radius over the defaults: k_depth_filter ahead of the ingest
--radius takes several values: the loop runs once per value in one process (the frames are created once), and one
`rocprofv3 --kernel-trace --stats -- python scripts/depth_filter_rate.py --kind filter --radius 0 2 3` holds each radius' kernel under a
name of its own (k_depth_filter<R, E, ZF, NT>).  Each call is also timed with HIP events on the context's stream around the call and a
download of one 80 x 60 plane of the batch's first frame, which makes that stream wait for the build stream.

    python scripts/depth_filter_rate.py --kind filter [--format u16] [--frames 256] [--radius 2] [--reps 10] [--warmup 3]
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


def ptrs(t):
    step = t[0].numel() * t.element_size()
    return d.device_pointer_array([t.data_ptr() + i * step for i in range(t.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["plain", "filter"], default="plain")
    ap.add_argument("--format", choices=["u16", "f32"], default="u16")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--radius", type=int, nargs="+", default=[2])
    ap.add_argument("--edge-radius", type=int, default=1)
    ap.add_argument("--hole-radius", type=int, default=0)
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
    if a.format == "f32":
        metres = raw.to(torch.int32).bitwise_and(0xFFFF).to(torch.float32) * 2e-4
        raw = torch.where(metres > 0, metres, torch.full_like(metres, float("nan"))).contiguous()
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(4)
    frames = d.FrameSet([cam.create_raw(pair["grey_ref"], pair["depth_ref"]) for _ in range(n)])
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    probe = np.empty((H >> 3, W >> 3), np.float32)
    pg, pr = ptrs(grey), ptrs(raw)

    def ingest():
        if a.format == "u16":
            d.update_raw_device_batch(frames, pg, pr, 2e-4, role="current", config=cfg)
        else:
            d.update_colour_device_batch(frames, pg, pr, "grey8", W, 1.0, role="current", config=cfg, depth_format="f32", depth_pitch=W * 4)
        ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, frames.handles[0], 3, 0, probe.ctypes.data_as(C.POINTER(C.c_float))))

    for radius in (a.radius if a.kind == "filter" else [None]):
        if radius is not None:
            d.set_depth_filter_batch(frames.pyramids, radius=radius, edge_radius=a.edge_radius, hole_radius=a.hole_radius)
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
        out = {"kind": a.kind, "format": a.format, "frames": n, "width": W, "height": H, "calls": a.reps + a.warmup, "library": _lib.LIB_PATH,
               "timing": "HIP events on the context's stream",
               "ms": {"median": round(float(np.median(times)), 4), "min": round(min(times), 4), "max": round(max(times), 4)}}
        if radius is not None:
            out.update(radius=radius, edge_radius=a.edge_radius, hole_radius=a.hole_radius, depth_filter_ingests=ctx.counter("depth_filter_ingests"))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
