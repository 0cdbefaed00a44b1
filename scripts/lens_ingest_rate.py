"""Cost of the rectifying ingest (profiles/lens_ingest.md).  Prints one JSON line.

N frames of 640 x 480 per call, u16 depth + BGR8 image from device planes of their own (nothing comes from the caches), ingested
straight into a role (dvo_hip_frames_update_colour_device_as_ex: CURRENT, and REFERENCE with DVO_HIP_INGEST_NO_RAW_COPY), without a
lens and -- where the library has dvo_hip_frames_set_lens -- with the fr1-like plumb-bob lens, alternated in one process.  Timed with HIP
events on the context's stream around the call and a download of one 80 x 60 plane of the batch's first frame, which makes that stream
wait for the build stream (scripts/f32_ingest_rate.py times the float ingest the same way).  DVO_HIP_LIBRARY selects another build of
the library (the parent commit's, for the A/B of the lens-less path).
Bytes of the rectify pass per pixel: 5 read (3 colour + 2 depth; every source byte is wanted about once, the taps of neighbouring
pixels overlap) + 8 written.  The rate to hold them against is what dvo_hip_time_stream_mix reaches on the same box (16 B read + 8 B
written per pixel of a level-0 pair).

    python scripts/lens_ingest_rate.py [--frames 1024] [--reps 10] [--warmup 3]
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
ROLE = {"current": 0, "reference": 1}
FR1_D = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633, 0.0, 0.0, 0.0]
PASS_BYTES = 5 + 8


def ptrs(t):
    step = t[0].numel() * t.element_size()
    return d.device_pointer_array([t.data_ptr() + i * step for i in range(t.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = a.frames
    ctx = d.default_context()
    L = ctx._lib
    has_lens = hasattr(L, "dvo_hip_frames_set_lens")             # (an older build named by DVO_HIP_LIBRARY has none)
    stream = torch.cuda.ExternalStream(L.dvo_hip_context_stream(ctx.ptr))
    pair = datagen.synth_pair(3, W, H)
    g = torch.from_numpy(pair["grey_ref"]).cuda()
    z = torch.from_numpy(pair["depth_ref"].astype(np.int16)).cuda()
    shift = lambda t, i: torch.roll(t, shifts=(i % 97, 3 * (i // 97)), dims=(0, 1))   # noqa: E731
    grey = torch.stack([shift(g, i) for i in range(n)]).contiguous()
    raw = torch.stack([shift(z, i) for i in range(n)]).contiguous()
    bgr = torch.stack([grey, grey, grey], -1).contiguous()
    del grey
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(4)
    sets = {"plain": d.FrameSet([cam.create_raw(pair["grey_ref"], pair["depth_ref"]) for _ in range(n)])}
    if has_lens:
        sets["lens"] = d.FrameSet([cam.create_raw(pair["grey_ref"], pair["depth_ref"]) for _ in range(n)])
        K_raw = (np.asarray(pair["K"], np.float64) * np.array([1.013, 1.009, 0.994, 1.011])).astype(np.float32)
        d.set_lens_batch(sets["lens"].pyramids, K_raw, FR1_D)
    cfg = d.Config(FirstLevel=3, LastLevel=0).to_c()
    probe = np.empty((H >> 3, W >> 3), np.float32)
    pb, pr = ptrs(bgr), ptrs(raw)

    def ingest(kind, role):
        flags = _lib.INGEST_NO_RAW_COPY if role == "reference" else 0
        frames = sets[kind]
        ctx.check(L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, n, frames.handles, pb, _lib.PIXEL_FORMATS["bgr8"], 0, pr, 2e-4, ROLE[role],
                                                              C.byref(cfg), flags))
        ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, frames.handles[0], 3, 0, probe.ctypes.data_as(C.POINTER(C.c_float))))

    times = {(k, r): [] for k in sets for r in ROLE}
    for k, r in times:
        for _ in range(a.warmup):
            ingest(k, r)
    torch.cuda.synchronize()
    for rep in range(a.reps):                                    # alternated: every kind and role once per round
        for k, r in times:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            ingest(k, r)
            end.record(stream)
            end.synchronize()
            times[(k, r)].append(start.elapsed_time(end))
    out = {"frames": n, "width": W, "height": H, "library": os.path.basename(_lib.LIB_PATH), "timing": "HIP events on the context's stream",
           "ms": {"%s_%s" % (k, r): {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                  for (k, r), t in times.items()}}
    # the HBM rate of the box: the plain streaming kernel over level-0 planes of min(n, 256) pairs, 16 B read + 8 B written per pixel
    m = min(n, 256)
    frames = sets["plain"].pyramids
    ingest("plain", "current")                                   # (every frame holds its current role: the other is derived from it)
    trk = d.DenseTracker(d.Config(FirstLevel=3, LastLevel=0), ctx)
    half = m // 2
    if half >= 1:
        ms = trk.time_stream_mix(frames[:half], frames[half:2 * half], 0, reps=20, with_write=True)
        torch.cuda.synchronize()
        rate = half * W * H * 24 / ms / 1e6
        out["stream_mix"] = {"pairs": half, "ms": round(ms, 4), "GB/s": round(rate, 1)}
        if has_lens:
            out["lens_cost"] = {}
            for r in ROLE:
                extra = float(np.median(times[("lens", r)])) - float(np.median(times[("plain", r)]))
                at_rate = n * W * H * PASS_BYTES / rate / 1e6
                out["lens_cost"][r] = {"extra_ms": round(extra, 4), "us_per_frame": round(extra * 1e3 / n, 3),
                                       "pass_bytes_at_stream_rate_ms": round(at_rate, 4), "ratio": round(extra / at_rate, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
