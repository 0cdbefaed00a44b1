"""Cost of counting keyframe covisibility on the device (profiles/covisibility.md).  Prints one JSON line.

n keyframes of 640 x 480 (the scene of scripts/frame_warp_rate.py, rolled) stand along a short trajectory.  For n = 32 and 256, at
levels 2 and 3, a 1 x n pair list (keyframe 0 against all) and the n x n list (all ordered pairs) are counted three ways:

  covisibility   dvo_hip_frames_covisibility into preallocated DEVICE records: the new call;
  warp_inverse   what the parent offers for the same numbers: warp_inverse_batch to host planes, then counted on the host (finite Z_w: in
                 view; finite I_w: consistent; the sum of |I_w - I_a| over them);
  match_coarse   what the validator spends per candidate: match_batch restricted to the one level, from the pair's transform.

Each is timed with a host clock around the whole call, which ends in a wait for the context's stream: argument checks, table uploads,
launches, downloads and (warp_inverse) the host's counting are inside.  The two older ways are run on at most --cap pairs of a list
(the first ones) and reported per pair: 65 536 items of warp planes are 10 GB of downloads.  The new call's bytes are counted from the
shapes by the traffic model of covisibility.hip's head comment (8 B per pixel of a, 8 B per pixel in view -- counted from the records
-- and 32 B + 56 B per pair) and priced at the HBM peak of 8.0 TB/s: a whole-call figure over an upper bound of the traffic (b's planes
are shared and should hit in cache), not a kernel's share of peak.  The first 3 records of every list are compared with the host build
of covisibility.h (tests/test_covisibility.py).

    python scripts/covisibility_rate.py [--sizes 32 256] [--levels 2 3] [--reps 7] [--warmup 2] [--cap 2048]
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
HBM_PEAK = 8.0e12


def pose_at(i):
    """camera -> world along a gentle arc: 2 cm and 0.2 degrees per keyframe"""
    T = np.eye(4)
    th = 0.0035 * i
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
    T[:3, 3] = [0.02 * i, -0.002 * i, 0.005 * i]
    return T


def timed(call, warmup, reps):
    times = []
    out = None
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    t = times[warmup:]
    return out, {"median": round(float(np.median(t)), 4), "min": round(float(np.min(t)), 4), "max": round(float(np.max(t)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cap", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("covisibility_rate: no GPU; a rate is measured on the device or not at all")
    ctx = d.default_context()
    pair = datagen.synth_pair(3, W, H)
    I0 = pair["grey_ref"].astype(np.float32)
    Z0 = pair["depth_ref"].astype(np.float32) * np.float32(2e-4)
    Z0[pair["depth_ref"] == 0] = np.nan
    K = np.ascontiguousarray(pair["K"], np.float32)
    levels = max(a.levels) + 1
    cam = d.RgbdCameraPyramid(W, H, K, ctx)
    cam.build(levels)
    n_max = max(a.sizes)
    frames = [cam.create(np.roll(I0, (i % 7, 3 * i), (0, 1)), np.roll(Z0, (i % 5, 2 * i), (0, 1))) for i in range(n_max)]
    for f in frames:
        f.build(levels)
    poses = np.stack([pose_at(i) for i in range(n_max)])
    inv = np.linalg.inv(poses)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_covisibility as tcv
    out = {"width": W, "height": H, "reps": a.reps, "cap": a.cap, "library": _lib.LIB_PATH, "hbm_peak_Bps": HBM_PEAK,
           "timing": "host clock around the whole call, which ends in a wait for the context's stream", "lists": []}
    for level in a.levels:
        w, h = W >> level, H >> level
        tracker = d.DenseTracker(d.Config(FirstLevel=level, LastLevel=level, UseInitialEstimate=True), ctx)
        for n in a.sizes:
            for shape in ("1xn", "nxn"):
                if shape == "1xn":
                    pa, pb = np.zeros(n, np.int64), np.arange(n)
                else:
                    pa, pb = (x.reshape(-1) for x in np.mgrid[0:n, 0:n])
                pairs = np.stack([pa, pb], 1)
                T = np.ascontiguousarray(inv[pb] @ poses[pa])
                m = len(pairs)
                rec, ms = timed(lambda: d.covisibility_batch(frames[:n], pairs, T, level=level, device=True), a.warmup, a.reps)
                rec = rec.cpu().numpy().view(d.COVIS_DTYPE).reshape(-1)
                same = True
                for k in range(min(3, m)):
                    (ia, ib) = pairs[k]
                    A, B = frames[ia].level(level), frames[ib].level(level)
                    want = tcv.covisibility_host(np.array(A.intensity), np.array(A.depth), np.array(B.intensity), np.array(B.depth), np.array(A.K),
                                                 np.array(B.K), T[k])
                    same = same and tcv.as_dict(rec[k]) == tcv.as_dict(want)
                model = 8.0 * w * h * m + 8.0 * float(rec["in_view"].sum()) + (32 + 56) * m
                entry = {"level": level, "width": w, "height": h, "keyframes": n, "list": shape, "pairs": m, "equals_host_first3": bool(same),
                         "mean_in_view_share": round(float(rec["in_view"].sum()) / (w * h * m), 4),
                         "mean_consistent_share": round(float(rec["consistent"].sum()) / (w * h * m), 4),
                         "covisibility": {"call_ms": ms, "us_per_pair": round(ms["median"] * 1e3 / m, 4), "model_bytes": model,
                                          "achieved_Bps": round(model / (ms["median"] * 1e-3), 1),
                                          "achieved_fraction_of_hbm_peak": round(model / (ms["median"] * 1e-3) / HBM_PEAK, 5)}}
                c = min(m, a.cap)
                ra, rb = [frames[i] for i in pa[:c]], [frames[i] for i in pb[:c]]
                planes_a = [np.array(frames[i].level(level).intensity) for i in range(n)]

                def by_warp():
                    Iw, Zw = d.warp_inverse_batch(ra, rb, T[:c], level=level)
                    counts = np.zeros((c, 3))
                    for k in range(c):
                        ok = np.isfinite(Iw[k])
                        counts[k] = (np.isfinite(Zw[k]).sum(), ok.sum(), np.abs(Iw[k][ok] - planes_a[pa[k]][ok]).sum())
                    return counts

                _, ms_w = timed(by_warp, 1, max(3, a.reps // 2))
                entry["warp_inverse"] = {"pairs": c, "call_ms": ms_w, "us_per_pair": round(ms_w["median"] * 1e3 / c, 4)}
                # Result.transformation is current -> reference: the pair's a is the reference, b the current frame
                _, ms_m = timed(lambda: tracker.match_batch_arrays(ra, rb, np.linalg.inv(T[:c])), 1, max(3, a.reps // 2))
                entry["match_coarse"] = {"pairs": c, "call_ms": ms_m, "us_per_pair": round(ms_m["median"] * 1e3 / c, 4)}
                entry["cheapest"] = min(("covisibility", "warp_inverse", "match_coarse"), key=lambda k: entry[k]["us_per_pair"])
                out["lists"].append(entry)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
