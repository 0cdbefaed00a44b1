"""Rate of the colour ingest against the grey one (profiles/colour_ingest.md).  Prints one JSON line.

Every frame has input planes of its own (1024 distinct colour, grey and depth planes in HBM: nothing comes from the caches), and the
grey planes are the CV_BGR2GRAY grey of the colour ones, so both runs ingest the same images and build the same frames.
Ingest alone: 1024 frames of 640 x 480 into the CURRENT or REFERENCE role (dvo_hip_frames_update_raw_device_as_ex /
dvo_hip_frames_update_colour_device_as_ex) from grey, BGR8 and RGBA8 planes.  Timed with HIP events on the context's stream: the
ingest runs on the context's build stream, and a download of one 80 x 60 plane of the batch's first frame
(dvo_hip_frame_download_plane) makes the context's stream wait for it -- the same few microseconds in every run.
Bytes per pixel from the shapes: the grey ingest's 40 (CURRENT) / 33 (REFERENCE) plus 2 (BGR8) or 3 (RGBA8) input bytes.
Whole step: 1024 pairs, both sides ingested in their roles, then dvo_hip_match_batch; HIP events on the context's stream (the match
waits for the build).  Unlike bench.py's loop, the ingest of a step does not overlap the match of the step before."""
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
BYTES = {"current": 40, "reference": 33}
EXTRA = {"grey": 0, "bgr8": 2, "rgba8": 3}
ROLE = {"current": 0, "reference": 1}


def distinct_planes(grey, depth, n, seed):
    """n distinct BGR8 frames (the grey scene with a channel tint, shifted by frame), their RGBA8 copies, their CV_BGR2GRAY grey, and n
    distinct depth planes, all on the device"""
    g = torch.from_numpy(grey.astype(np.int32)).cuda()
    y, x = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    tint = [torch.sin(x / 37.0 + seed) * 45, torch.cos(y / 23.0 + seed) * 25, -torch.sin((x + y) / 51.0 + seed) * 40]
    base = torch.stack([(g + t).round().clamp(0, 255) for t in tint], -1).to(torch.uint8)           # [H, W, 3] B, G, R
    z = torch.from_numpy(depth.astype(np.int16)).cuda()
    bgr = torch.stack([torch.roll(base, shifts=(i % 97, 3 * (i // 97)), dims=(0, 1)) for i in range(n)])
    deps = torch.stack([torch.roll(z, shifts=(i % 97, 3 * (i // 97)), dims=(0, 1)) for i in range(n)])
    b, gg, r = (bgr[..., k].to(torch.int32) for k in range(3))
    grey_n = ((b * 1868 + gg * 9617 + r * 4899 + 8192) >> 14).to(torch.uint8).contiguous()
    rgba = torch.cat([bgr.flip(-1), torch.full_like(bgr[..., :1], 255)], -1).contiguous()
    return {"grey": grey_n, "bgr8": bgr.contiguous(), "rgba8": rgba}, deps.contiguous()


def ptrs(t):
    step = t[0].numel() * t.element_size()
    return d.device_pointer_array([t.data_ptr() + i * step for i in range(t.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    n = a.frames
    ctx = d.default_context()
    L = ctx._lib
    stream = torch.cuda.ExternalStream(L.dvo_hip_context_stream(ctx.ptr))
    pair = datagen.synth_pair(3, W, H)
    ref_planes, ref_depth = distinct_planes(pair["grey_ref"], pair["depth_ref"], n, 0.5)
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(4)
    frames = d.FrameSet([cam.create_raw(pair["grey_ref"], pair["depth_ref"]) for _ in range(n)])
    cfg = d.Config(FirstLevel=3, LastLevel=0).to_c()
    probe = np.empty((H >> 3, W >> 3), np.float32)

    def ingest(fs, planes, depth, kind, role):
        if kind == "grey":
            rc = L.dvo_hip_frames_update_raw_device_as_ex(ctx.ptr, n, fs.handles, planes, depth, 1 / 5000.0, ROLE[role], C.byref(cfg), 0)
        else:
            rc = L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, n, fs.handles, planes, _lib.PIXEL_FORMATS[kind], 0, depth, 1 / 5000.0,
                                                             ROLE[role], C.byref(cfg), 0)
        ctx.check(rc)

    def timed(body, reps, warmup):
        for _ in range(warmup):
            body()
        torch.cuda.synchronize()
        total = 0.0
        for _ in range(reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            body()
            end.record(stream)
            end.synchronize()
            total += start.elapsed_time(end)
        return total / reps

    def wait_build(fs):   # the context's stream waits for the build of the batch (and downloads 19 KB)
        ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, fs.handles[0], 3, 0, probe.ctypes.data_as(C.POINTER(C.c_float))))

    out = {"frames": n, "width": W, "height": H, "timing": "HIP events on the context's stream", "ingest": {}}
    zp = ptrs(ref_depth)
    for role in ("current", "reference"):
        for kind in ("grey", "bgr8", "rgba8"):
            pp = ptrs(ref_planes[kind])

            def body():
                ingest(frames, pp, zp, kind, role)
                wait_build(frames)
            ms = timed(body, a.reps, a.warmup)
            gb = n * W * H * (BYTES[role] + EXTRA[kind]) / 1e9
            out["ingest"]["%s_%s" % (role, kind)] = {"ms": round(ms, 4), "GB/s": round(gb / ms * 1e3, 1), "of_8TB/s": round(gb / ms * 1e3 / 8000, 3)}
        for kind in ("bgr8", "rgba8"):
            e = out["ingest"]["%s_%s" % (role, kind)]
            e["ratio_to_grey"] = round(e["ms"] / out["ingest"]["%s_grey" % role]["ms"], 3)

    # whole step: 1024 pairs; the current frames are a second set of distinct planes; grey = the CV_BGR2GRAY grey of the colour planes
    cur_planes, cur_depth = distinct_planes(pair["grey_cur"], pair["depth_cur"], n, 0.5)
    refs, curs = frames, d.FrameSet([cam.create_raw(pair["grey_cur"], pair["depth_cur"]) for _ in range(n)])
    res = (_lib.Result * n)()                                  # (no initial estimate: the transforms are outputs only)
    zc = ptrs(cur_depth)
    out["step"] = {}
    records = {}
    for kind in ("grey", "bgr8"):
        pr, pc = ptrs(ref_planes[kind]), ptrs(cur_planes[kind])

        def step():
            ingest(refs, pr, zp, kind, "reference")
            ingest(curs, pc, zc, kind, "current")
            ctx.check(L.dvo_hip_match_batch(ctx.ptr, n, refs.handles, curs.handles, C.byref(cfg), res, None, 0, None, 0))
        out["step"][kind] = {"ms": round(timed(step, a.reps, a.warmup), 4)}
        records[kind] = np.array([list(res[i].transformation) for i in range(n)])
    out["step"]["ratio"] = round(out["step"]["bgr8"]["ms"] / out["step"]["grey"]["ms"], 3)
    out["step"]["max_transform_difference"] = float(np.abs(records["bgr8"] - records["grey"]).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
