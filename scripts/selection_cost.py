"""Cost of the caller selection (include/dvo_hip.h, dvo_hip_frames_set_selection) on a streaming step: every step re-ingests its
reference frames into the reference role (the fused raw ingest, where the apply pass runs behind the build) and its current frames, then
aligns the batch.  The same step with every reference frame masked (a block mask and a depth range) and without, alternated in one
process, several rounds; prints one JSON line per batch size with the per-step medians.

    python scripts/selection_cost.py [--pairs 1024 128] [--rounds 6] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dvo_slam_amd as d  # noqa: E402
from dvo_slam_amd import datagen  # noqa: E402

W, H = 640, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1024, 128])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    ctx = d.Context(0)
    pairs = [datagen.synth_pair(100 + i, W, H) for i in range(8)]
    cam = d.RgbdCameraPyramid(W, H, pairs[0]["K"], ctx)
    cam.build(4)
    grey_r = [torch.from_numpy(p["grey_ref"]).cuda() for p in pairs]
    depth_r = [torch.from_numpy(p["depth_ref"].astype(np.int16)).cuda() for p in pairs]
    grey_c = [torch.from_numpy(p["grey_cur"]).cuda() for p in pairs]
    depth_c = [torch.from_numpy(p["depth_cur"].astype(np.int16)).cuda() for p in pairs]
    mask = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    mask[100:260, 200:400] = 0                                  # a fifth of the image
    torch.cuda.synchronize()
    cfg = d.Config()
    out = []
    for n in a.pairs:
        refs = [cam.create_raw(p["grey_ref"], p["depth_ref"]) for p in (pairs * (n // 8 + 1))[:n]]
        curs = [cam.create_raw(p["grey_cur"], p["depth_cur"]) for p in (pairs * (n // 8 + 1))[:n]]
        gr = d.device_pointer_array([grey_r[i % 8].data_ptr() for i in range(n)])
        zr = d.device_pointer_array([depth_r[i % 8].data_ptr() for i in range(n)])
        gc = d.device_pointer_array([grey_c[i % 8].data_ptr() for i in range(n)])
        zc = d.device_pointer_array([depth_c[i % 8].data_ptr() for i in range(n)])
        tr = d.DenseTracker(cfg, ctx)
        fr, fc = d.FrameSet(refs), d.FrameSet(curs)

        def step():
            d.update_raw_device_batch(fr, gr, zr, role="reference", config=cfg)
            d.update_raw_device_batch(fc, gc, zc, role="current", config=cfg)
            tr.match_batch_arrays(fr, fc)

        times = {"masked": [], "plain": []}
        for r in range(a.rounds):
            for kind in (("plain", "masked") if r % 2 == 0 else ("masked", "plain")):
                if kind == "masked":
                    d.set_selection_batch(refs, [mask.data_ptr()] * n, 0.0, 4.0)
                else:
                    d.clear_selection_batch(refs)
                step()                                          # warm-up of this configuration
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                times[kind].append((time.perf_counter() - t0) / a.steps * 1e3)
        row = dict(pairs=n, steps_per_sample=a.steps, rounds=a.rounds,
                   plain_ms_median=float(np.median(times["plain"])), masked_ms_median=float(np.median(times["masked"])),
                   plain_ms=[round(x, 3) for x in times["plain"]], masked_ms=[round(x, 3) for x in times["masked"]])
        row["masked_minus_plain_ms"] = row["masked_ms_median"] - row["plain_ms_median"]
        print(json.dumps(row), flush=True)
        out.append(row)
        d.clear_selection_batch(refs)
        del refs, curs, fr, fc


if __name__ == "__main__":
    main()
