"""Rate of the float-plane ingest against the grey + u16 one (profiles/f32_ingest.md).  Prints one JSON line.

Ingest alone: 1024 frames of 640 x 480 per call, device planes, every frame with planes of its own (nothing comes from the caches); role
CURRENT and role REFERENCE, the latter with DVO_HIP_INGEST_NO_RAW_COPY; grey + u16 (dvo_hip_frames_update_raw_device_as_ex, the baseline
of the same run), F32 + F32 (dvo_hip_frames_update_f32_device_as_ex) and BGR8 + F32 depth
(dvo_hip_frames_update_colour_f32depth_device_as_ex), alternated in one process.  Timed with HIP events on the context's stream around the
call and a download of one 80 x 60 plane of the batch's first frame, which makes that stream wait for the build stream -- the same few
microseconds in every run (scripts/colour_ingest_rate.py times the colour ingest the same way).
Bytes per level-0 pixel, from the code: the source read + level 0's role plane (R or C, 8 B) + levels 1-3 (I and Z, 8 B, and for a current
frame their plane C, 8 B more, on 21 / 64 of the pixels).
Host path: the same 1024 float frames from pinned host memory, on the host clock: dvo_hip_frame_create_f32 per frame +
dvo_hip_frames_prepare (the only way without the float ingest) against one dvo_hip_frames_update_f32_as_ex + dvo_hip_upload_wait.

    python scripts/f32_ingest_rate.py [--frames 1024] [--reps 10] [--warmup 3] [--host-reps 2]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dvo_slam_amd as d  # noqa: E402
from dvo_slam_amd import _lib, datagen  # noqa: E402

W, H = 640, 480
SOURCE = {"grey_u16": 3, "f32_f32": 8, "bgr8_f32": 7}
WRITTEN = {"current": 8 + 16 * 21 / 64, "reference": 8 + 8 * 21 / 64}
ROLE = {"current": 0, "reference": 1}


def ptrs(t):
    step = t[0].numel() * t.element_size()
    return d.device_pointer_array([t.data_ptr() + i * step for i in range(t.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()
    n = a.frames
    ctx = d.default_context()
    L, vp = ctx._lib, C.c_void_p
    stream = torch.cuda.ExternalStream(L.dvo_hip_context_stream(ctx.ptr))
    pair = datagen.synth_pair(3, W, H)
    g = torch.from_numpy(pair["grey_ref"]).cuda()
    z = torch.from_numpy(pair["depth_ref"].astype(np.int16)).cuda()
    shift = lambda t, i: torch.roll(t, shifts=(i % 97, 3 * (i // 97)), dims=(0, 1))   # noqa: E731
    grey = torch.stack([shift(g, i) for i in range(n)]).contiguous()
    raw = torch.stack([shift(z, i) for i in range(n)]).contiguous()
    y, x = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    inten = (grey.float() + 0.45 * torch.sin(x / 9.0) * torch.cos(y / 7.0)).clamp(0, 255).contiguous()
    depth = torch.where(raw == 0, torch.full((), float("nan"), device="cuda"), raw.float() * 2e-4 + 0.9e-4 * torch.sin(x / 13.0 + y / 17.0)).contiguous()
    bgr = torch.stack([grey, grey, grey], -1).contiguous()
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(4)
    frames = d.FrameSet([cam.create_raw(pair["grey_ref"], pair["depth_ref"]) for _ in range(n)])
    cfg = d.Config(FirstLevel=3, LastLevel=0).to_c()
    probe = np.empty((H >> 3, W >> 3), np.float32)
    pg, pr, pi, pz, pb = ptrs(grey), ptrs(raw), ptrs(inten), ptrs(depth), ptrs(bgr)

    def ingest(kind, role):
        flags = _lib.INGEST_NO_RAW_COPY if role == "reference" else 0
        if kind == "grey_u16":
            rc = L.dvo_hip_frames_update_raw_device_as_ex(ctx.ptr, n, frames.handles, pg, pr, 2e-4, ROLE[role], C.byref(cfg), flags)
        elif kind == "f32_f32":
            rc = L.dvo_hip_frames_update_f32_device_as_ex(ctx.ptr, n, frames.handles, pi, 0, pz, 0, 1.0, ROLE[role], C.byref(cfg), flags)
        else:
            rc = L.dvo_hip_frames_update_colour_f32depth_device_as_ex(ctx.ptr, n, frames.handles, pb, _lib.PIXEL_FORMATS["bgr8"], 0, pz, 0, 1.0,
                                                                      ROLE[role], C.byref(cfg), flags)
        ctx.check(rc)
        ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, frames.handles[0], 3, 0, probe.ctypes.data_as(C.POINTER(C.c_float))))

    out = {"frames": n, "width": W, "height": H, "timing": "HIP events on the context's stream", "ingest": {}}
    times = {(k, r): [] for k in SOURCE for r in ROLE}
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
    for (k, r), t in times.items():
        ms = float(np.median(t))
        b = SOURCE[k] + WRITTEN[r]
        base = float(np.median(times[("grey_u16", r)]))
        out["ingest"]["%s_%s" % (r, k)] = {"ms": round(ms, 4), "B_per_pixel": round(b, 2), "GB/s": round(n * W * H * b / ms / 1e6, 1),
                                           "time_ratio": round(ms / base, 3), "byte_ratio": round(b / (SOURCE["grey_u16"] + WRITTEN[r]), 3)}

    # host path, on the host clock
    plane = W * H * 4
    pinned = vp()
    ctx.check(L.dvo_hip_host_alloc(ctx.ptr, 2 * plane * n, C.byref(pinned)))
    host = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_float)), (n, 2, H, W))
    host[:, 0] = depth.cpu().numpy()                             # [depth][image] per frame: a run of frames in the slot layout
    host[:, 1] = inten.cpu().numpy()
    hz = (vp * n)(*[pinned.value + 2 * plane * i for i in range(n)])
    hi = (vp * n)(*[pinned.value + 2 * plane * i + plane for i in range(n)])
    K = np.ascontiguousarray(pair["K"], np.float32)
    fp = C.POINTER(C.c_float)
    host_ms = {"create_f32_each": [], "update_f32": []}
    for role in ("current", "reference"):
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            made = (vp * n)()
            for i in range(n):
                one = vp()
                ctx.check(L.dvo_hip_frame_create_f32(ctx.ptr, W, H, K.ctypes.data_as(fp), C.cast(hi[i], fp), C.cast(hz[i], fp), 4, C.byref(one)))
                made[i] = one.value
            ctx.check(L.dvo_hip_frames_prepare(ctx.ptr, n, made, ROLE[role], C.byref(cfg)))
            ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, made[0], 3, 0, probe.ctypes.data_as(fp)))
            host_ms["create_f32_each"].append((role, (time.perf_counter() - t0) * 1e3))
            for i in range(n):
                L.dvo_hip_frame_destroy(ctx.ptr, made[i])
            t0 = time.perf_counter()
            ctx.check(L.dvo_hip_frames_update_f32_as_ex(ctx.ptr, n, frames.handles, hi, 0, hz, 0, 1.0, ROLE[role], C.byref(cfg), 0))
            ctx.check(L.dvo_hip_upload_wait(ctx.ptr))
            ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, frames.handles[0], 3, 0, probe.ctypes.data_as(fp)))
            host_ms["update_f32"].append((role, (time.perf_counter() - t0) * 1e3))
    out["host"] = {"%s_%s" % (k, role): round(min(ms for r, ms in v if r == role), 2) for k, v in host_ms.items() for role in ROLE}
    out["host"]["timing"] = "host clock, best of %d, ms per %d frames from pinned memory" % (a.host_reps, n)
    L.dvo_hip_host_free(ctx.ptr, pinned)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
