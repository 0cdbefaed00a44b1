"""Cost of the sensor-format ingest (profiles/sensor_ingest.md): Bayer GRBG and YUYV planes against the BGR8 ingest of the same scenes.

Three measurements on 640 x 480 frames, in batches (--batches, default 64 and 2048), every frame with input planes of its own:
  (a) device-resident planes: one dvo_hip_frames_update_colour_device_as_ex per batch straight into a role, per format, alternated in one
      process; HIP events on the context's stream around the call and a download of one 80 x 60 plane of the batch's first frame, which
      makes that stream wait for the build stream (scripts/lens_ingest_rate.py times the lens pass the same way);
  (b) host-fed planes from pinned memory (dvo_hip_host_alloc; slots of [u16 depth][image] that follow each other, so a batch moves in
      one transfer): dvo_hip_frames_update_colour_as_ex + dvo_hip_upload_wait, host clock, frames per second;
  (c) --kernel-pass: nothing but ingests from device planes, first uncapped and then under the build stream's workgroup cap (option
      "build_workgroups" = counter "background_build_workgroups"), to be run under `rocprofv3 --kernel-trace`; --report reads
      k_sensor_convert's dispatches out of the trace (the capped ones have the smaller grid).
DVO_HIP_LIBRARY selects another build of the library (scripts/build_base.sh: the parent commit's); a build without the sensor formats is
timed on BGR8 alone.  Each run writes one JSON file; --report turns the files of several runs -- this build's and the parent's, alternated
by the caller so that the run-to-run spread of the BGR8 figure is measured too -- into profiles/sensor_ingest.md.

    python scripts/sensor_ingest_rate.py --out new_1.json                       (and with DVO_HIP_LIBRARY=...: --out base_1.json)
    rocprofv3 --kernel-trace -d trace -o sensor -- python scripts/sensor_ingest_rate.py --kernel-pass
    python scripts/sensor_ingest_rate.py --report new_*.json base_*.json --trace trace/.../sensor_kernel_trace.csv --bench bench.txt
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 640, 480
ROLE = {"current": 0, "reference": 1}
FORMATS = {"bgr8": (1, 3), "bayer_grbg8": (19, 1), "yuyv8": (20, 2)}       # DVO_HIP_PIXEL_*, bytes per pixel
HBM_PEAK = 8.0e12                                                          # bytes / s (MI355X)
# bytes k_sensor_convert moves per pixel in grey mode: the sensor plane read once, the grey plane written once
PASS_BYTES = {"bayer_grbg8": 1 + 1, "yuyv8": 2 + 1}


def stats(t):
    t = np.asarray(t, np.float64)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4), "n": int(t.size)}


def device_planes(torch, pair, n):
    """n distinct scenes on the device as BGR8, Bayer GRBG and YUYV planes, and their u16 depth planes"""
    g = torch.from_numpy(pair["grey_ref"].astype(np.int32)).cuda()
    y, x = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    tint = [torch.sin(x / 37.0 + 0.5) * 45, torch.cos(y / 23.0 + 0.5) * 25, -torch.sin((x + y) / 51.0 + 0.5) * 40]
    base = torch.stack([(g + t).round().clamp(0, 255) for t in tint], -1).to(torch.uint8)           # [H, W, 3] B, G, R
    z = torch.from_numpy(pair["depth_ref"].astype(np.int16)).cuda()
    roll = lambda t, i: torch.roll(t, shifts=(i % 97, 3 * (i // 97)), dims=(0, 1))                  # noqa: E731
    bgr = torch.stack([roll(base, i) for i in range(n)]).contiguous()
    depth = torch.stack([roll(z, i) for i in range(n)]).contiguous()
    green = ((x + y) % 2 == 0)                                    # G R / B G
    red = (y % 2 == 0) & (x % 2 == 1)
    bayer = torch.where(green, bgr[..., 1], torch.where(red, bgr[..., 2], bgr[..., 0])).contiguous()
    b, gg, r = (bgr[..., k].to(torch.float32) for k in range(3))
    luma = (16.0 + 0.257 * r + 0.504 * gg + 0.098 * b).round().clamp(0, 255).to(torch.uint8)
    u = (128.0 - 0.148 * r - 0.291 * gg + 0.439 * b).round().clamp(0, 255).to(torch.uint8)
    v = (128.0 + 0.439 * r - 0.368 * gg - 0.071 * b).round().clamp(0, 255).to(torch.uint8)
    chroma = torch.where(x % 2 == 0, u, torch.roll(v, 1, dims=2))
    yuyv = torch.stack([luma, chroma], -1).contiguous()
    return {"bgr8": bgr, "bayer_grbg8": bayer, "yuyv8": yuyv}, depth


def setup(n):
    import torch
    import dvo_slam_amd as d
    from dvo_slam_amd import datagen
    ctx = d.default_context()
    pair = datagen.synth_pair(3, W, H)
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(4)
    frames = d.FrameSet([cam.create_raw(pair["grey_ref"], pair["depth_ref"]) for _ in range(n)])
    try:
        ctx.counter("sensor_ingests")
        kinds = list(FORMATS)
    except d.DvoHipError:                                        # (a build from before the sensor formats)
        kinds = ["bgr8"]
    return torch, d, ctx, pair, frames, kinds


def ptrs(d, t):
    step = t[0].numel() * t.element_size()
    return d.device_pointer_array([t.data_ptr() + i * step for i in range(t.shape[0])])


def measure(a):
    from dvo_slam_amd import _lib
    out = {"library": os.path.abspath(_lib.LIB_PATH), "width": W, "height": H, "reps": a.reps, "warmup": a.warmup, "device": {}, "host": {}}
    for n in a.batches:
        torch, d, ctx, pair, frames, kinds = setup(n)
        L = ctx._lib
        stream = torch.cuda.ExternalStream(L.dvo_hip_context_stream(ctx.ptr))
        cfg = d.Config(FirstLevel=3, LastLevel=0).to_c()
        probe = np.empty((H >> 3, W >> 3), np.float32)
        planes, depth = device_planes(torch, pair, n)
        zp = ptrs(d, depth)
        pp = {k: ptrs(d, planes[k]) for k in kinds}

        def wait_build():
            ctx.check(L.dvo_hip_frame_download_plane(ctx.ptr, frames.handles[0], 3, 0, probe.ctypes.data_as(C.POINTER(C.c_float))))

        def ingest(kind, role):
            ctx.check(L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, n, frames.handles, pp[kind], FORMATS[kind][0], 0, zp, 2e-4, ROLE[role],
                                                                  C.byref(cfg), 0))
            wait_build()

        # (a) device-resident planes, every kind and role once per round
        times = {(k, r): [] for k in kinds for r in ROLE}
        for key in times:
            for _ in range(a.warmup):
                ingest(*key)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for key in times:
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                ingest(*key)
                end.record(stream)
                end.synchronize()
                times[key].append(start.elapsed_time(end) * 1e3 / n)      # us per frame
        out["device"][str(n)] = {"%s_%s" % key: stats(t) for key, t in times.items()}
        out["device"][str(n)]["sensor_ingests"] = ctx.counter("sensor_ingests") if len(kinds) > 1 else None

        # (b) host-fed from pinned memory: slots of [depth][image], one after the other
        host = {}
        for kind in kinds:
            bytes_px = FORMATS[kind][1]
            slot = W * H * (2 + bytes_px)
            pinned = C.c_void_p()
            ctx.check(L.dvo_hip_host_alloc(ctx.ptr, slot * n, C.byref(pinned)))
            buf = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint8)), shape=(n, slot))
            buf[:, :W * H * 2] = depth.cpu().numpy().view(np.uint8).reshape(n, -1)
            buf[:, W * H * 2:] = planes[kind].cpu().numpy().reshape(n, -1)
            vp = C.c_void_p
            cp = (vp * n)(*[pinned.value + i * slot + W * H * 2 for i in range(n)])
            dp = (vp * n)(*[pinned.value + i * slot for i in range(n)])
            host[kind] = (pinned, cp, dp)
        rates = {k: [] for k in kinds}

        def feed(kind):
            _, cp, dp = host[kind]
            ctx.check(L.dvo_hip_frames_update_colour_as_ex(ctx.ptr, n, frames.handles, cp, FORMATS[kind][0], 0, dp, 2e-4, 0, C.byref(cfg), 0))
            ctx.check(L.dvo_hip_upload_wait(ctx.ptr))
            wait_build()

        for kind in kinds:
            for _ in range(a.warmup):
                feed(kind)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for kind in kinds:
                t0 = time.perf_counter()
                feed(kind)
                rates[kind].append(n / (time.perf_counter() - t0))        # frames per second
        out["host"][str(n)] = {k: stats(t) for k, t in rates.items()}
        for pinned, _, _ in host.values():
            L.dvo_hip_host_free(ctx.ptr, pinned)
        del planes, depth, frames
        torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump(out, f)
    print(json.dumps(out))


def kernel_pass(a):
    """ingests only, for a kernel trace: per batch size and format, `reps` uncapped and then `reps` under the build stream's cap"""
    for n in a.batches:
        torch, d, ctx, pair, frames, kinds = setup(n)
        L = ctx._lib
        cfg = d.Config(FirstLevel=3, LastLevel=0).to_c()
        planes, depth = device_planes(torch, pair, n)
        zp = ptrs(d, depth)
        cap = ctx.counter("background_build_workgroups")
        for kind in kinds[1:]:
            pp = ptrs(d, planes[kind])
            for workgroups in (0, cap):
                ctx.set_option("build_workgroups", workgroups)
                for _ in range(a.warmup + a.reps):
                    ctx.check(L.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, n, frames.handles, pp, FORMATS[kind][0], 0, zp, 2e-4, 0, C.byref(cfg), 0))
                torch.cuda.synchronize()
        ctx.set_option("build_workgroups", 0)
        print(json.dumps({"frames": n, "cap": cap, "warmup": a.warmup, "reps": a.reps}))
        del planes, depth, frames


def read_trace(path, batches, warmup, reps):
    """k_sensor_convert's dispatches of a --kernel-pass run, in order: per batch size, per format (Bayer, then YUV), uncapped then capped"""
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "k_sensor_convert" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), int(row["Grid_Size_X"]) if "Grid_Size_X" in row else int(row["Grid_Size"])))
    rows.sort()
    out, at = {}, 0
    for n in batches:
        for kind in ("bayer_grbg8", "yuyv8"):
            for cap in ("uncapped", "capped"):
                block = rows[at:at + warmup + reps][warmup:]
                at += warmup + reps
                if not block:
                    continue
                us = [(e - s) / 1e3 for s, e, _ in block]
                gb = n * W * H * PASS_BYTES[kind]
                med = float(np.median(us))
                out["%d_%s_%s" % (n, kind, cap)] = {"us": stats(us), "workgroups": block[0][2] // 256, "GB/s": round(gb / med / 1e3, 1),
                                                    "of_hbm_peak": round(gb / (med * 1e-6) / HBM_PEAK, 3)}
    return out


def report(a):
    runs = [json.load(open(p)) for p in a.report]
    new = [r for r in runs if any("bayer_grbg8_current" in v for v in r["device"].values())]
    base = [r for r in runs if r not in new]
    lines = ["# Sensor-format ingest: Bayer GRBG and YUYV against BGR8", "",
             "Written by `scripts/sensor_ingest_rate.py --report` from %d runs of this build and %d of the parent commit's library" % (len(new), len(base)),
             "(`scripts/build_base.sh`, `DVO_HIP_LIBRARY`), alternated on one MI355X.  640 x 480 frames; every figure is a median over the runs'",
             "medians, with the smallest and the largest single repetition of all runs in brackets.", ""]

    def pooled(rs, section, n, key):
        got = [r[section][str(n)][key] for r in rs if str(n) in r[section] and key in r[section][str(n)]]
        if not got:
            return None
        return float(np.median([g["median"] for g in got])), min(g["min"] for g in got), max(g["max"] for g in got), [g["median"] for g in got]

    batches = sorted({int(n) for r in runs for n in r["device"]})
    lines += ["## (a) Device-resident planes: us per frame of a role ingest", "",
              "By bytes a sensor ingest and the BGR8 ingest are level: 1 read + 1 written + 1 read B/pixel (Bayer; YUYV 2 + 1 + 1) against 3 read.",
              "The bar is the parent's BGR8 figure within the spread of its own runs' medians.", "",
              "| batch | role | BGR8 parent | BGR8 this build | bayer_grbg8 | yuyv8 | parent's run-to-run spread | bayer / parent | yuyv / parent |", "|---|---|---|---|---|---|---|---|---|"]
    for n in batches:
        for role in ROLE:
            p = pooled(base, "device", n, "bgr8_" + role)
            cells = [pooled(new, "device", n, k + "_" + role) for k in FORMATS]
            fmt = lambda c: "not measured" if c is None else "%.2f [%.2f, %.2f]" % c[:3]            # noqa: E731
            spread = "not measured" if p is None or len(p[3]) < 2 else "%.1f %%" % (100 * (max(p[3]) - min(p[3])) / p[0])
            ratio = lambda c: "-" if c is None or p is None else "%.3f" % (c[0] / p[0])              # noqa: E731
            lines.append("| %d | %s | %s | %s | %s | %s | %s | %s | %s |" % (n, role, fmt(p), fmt(cells[0]), fmt(cells[1]), fmt(cells[2]), spread,
                                                                          ratio(cells[1]), ratio(cells[2])))
    lines += ["", "## (b) Host-fed planes from pinned memory: frames per second", "",
              "The link carries 3 (Bayer) or 4 (YUYV) B/pixel instead of 5, depth included: by bytes 1.67 x and 1.25 x the BGR8 rate.", "",
              "| batch | BGR8 parent | BGR8 this build | bayer_grbg8 | yuyv8 | bayer / parent (bytes: 1.67) | yuyv / parent (bytes: 1.25) |", "|---|---|---|---|---|---|---|"]
    for n in batches:
        p = pooled(base, "host", n, "bgr8")
        cells = [pooled(new, "host", n, k) for k in FORMATS]
        fmt = lambda c: "not measured" if c is None else "%.0f [%.0f, %.0f]" % c[:3]                # noqa: E731
        ratio = lambda c: "-" if c is None or p is None else "%.3f" % (c[0] / p[0])                  # noqa: E731
        lines.append("| %d | %s | %s | %s | %s | %s | %s |" % (n, fmt(p), fmt(cells[0]), fmt(cells[1]), fmt(cells[2]), ratio(cells[1]), ratio(cells[2])))
    lines += ["", "## (c) `k_sensor_convert` alone", ""]
    if a.trace:
        k = read_trace(a.trace, a.batches, a.warmup, a.reps)
        lines += ["From a `rocprofv3 --kernel-trace` run of `--kernel-pass` (a run of its own).  Bytes: the sensor plane read once and the grey plane",
                  "written once, %d (Bayer) and %d (YUYV) B/pixel; HBM peak taken as %.0f TB/s.  Capped: option \"build_workgroups\" at the" %
                  (PASS_BYTES["bayer_grbg8"], PASS_BYTES["yuyv8"], HBM_PEAK / 1e12),
                  "build stream's background cap.", "", "| batch | format | grid | workgroups | us per launch | GB/s | of HBM peak |", "|---|---|---|---|---|---|---|"]
        for key, v in k.items():
            n, rest = key.split("_", 1)
            kind, cap = rest.rsplit("_", 1)
            lines.append("| %s | %s | %s | %d | %.1f [%.1f, %.1f] | %.0f | %.3f |" % (n, kind, cap, v["workgroups"], v["us"]["median"], v["us"]["min"],
                                                                                 v["us"]["max"], v["GB/s"], v["of_hbm_peak"]))
    else:
        lines.append("Not measured: no kernel trace was given.")
    lines += ["", "## bench.py", ""]
    if a.bench and os.path.exists(a.bench):
        lines += ["`bench.py` is untouched; its result lines with the parent's library and with this build's, same box, alternated:", "", "```"]
        lines += [ln.rstrip() for ln in open(a.bench) if ln.strip()]
        lines += ["```"]
    else:
        lines.append("Not measured here.")
    if a.notes and os.path.exists(a.notes):
        lines += [""] + [ln.rstrip() for ln in open(a.notes)]
    with open(a.md, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[64, 2048])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="sensor_ingest_rate.json")
    ap.add_argument("--kernel-pass", action="store_true")
    ap.add_argument("--report", nargs="+")
    ap.add_argument("--trace")
    ap.add_argument("--bench")
    ap.add_argument("--notes")
    ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sensor_ingest.md"))
    a = ap.parse_args()
    if a.report:
        a.report = [p for pat in a.report for p in sorted(glob.glob(pat))]
        report(a)
    elif a.kernel_pass:
        kernel_pass(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
