"""Cost of keyframe retrieval by appearance on the device (profiles/keyframe_codes.md).  Prints one JSON line.

A book of N random codes of m = 512 ferns (N = 1 024, 65 536 and 1 048 576) is asked 1 and 16 queries, k = 8, two ways:

  device   KeyframeCodebook.query_codes with device outputs: dvo_hip_codebook_query_codes -- the upload of the queries, k_code_search,
           k_code_topk and the wait for the context's stream;
  numpy    the same search on the host, because no earlier path exists: the block-wise distance of every stored code by xor, shift-or,
           mask and a byte-wise popcount table, then argpartition + a sort of the k least (distance, id).

and 256 frames of 640 x 480 are encoded at level 4 (40 x 30) in one dvo_hip_frames_encode call, beside the same encoding in numpy over
downloaded planes.  Each is timed with a host clock around the whole call.  The device search's bytes are counted by the traffic model of
keyframe_codes.hip's head comment (N m / 2 bytes of codes per tile of 16 queries, 2 Q N bytes of distances written once and read three
times, 8 k bytes per query) and priced at the HBM peak of 8.0 TB/s: a whole-call figure over a model, not a kernel's share of peak.
Every search's rows are compared with the numpy search and the codes with the numpy encoding; the script still prints its line but
EXITS WITH STATUS 1 if any of them differs.

    python scripts/keyframe_codes_rate.py [--sizes 1024 65536 1048576] [--queries 1 16] [--reps 7] [--warmup 2]
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

M, K = 512, 8
HBM_PEAK = 8.0e12
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


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


def numpy_search(codes, queries, k):
    """rows [Q, k] of (id, distance): the stated search on the host"""
    rows = np.zeros((len(queries), k), d.CODE_MATCH_DTYPE)
    for q, code in enumerate(queries):
        x = codes ^ code
        x = (x | x >> 1 | x >> 2 | x >> 3) & np.uint32(0x11111111)
        dist = POP8[x.view(np.uint8)].reshape(len(codes), -1).sum(1, dtype=np.int64)
        key = dist << 24 | np.arange(len(codes))
        least = np.sort(key[np.argpartition(key, min(k, len(key) - 1))[:k]])
        rows[q]["id"], rows[q]["distance"] = least & 0xFFFFFF, least >> 24
    return rows


def numpy_encode(I, Z, ferns):
    """the code of planes I, Z under the ferns: the statement of keyframe_codes.h, a whole table at a time"""
    h, w = I.shape
    x, y = (ferns["u"].astype(np.int64) * w) >> 16, (ferns["v"].astype(np.int64) * h) >> 16
    x2, y2 = (ferns["u2"].astype(np.int64) * w) >> 16, (ferns["v2"].astype(np.int64) * h) >> 16
    a, b, z = I[y, x], I[y2, x2], Z[y, x]
    with np.errstate(invalid="ignore"):
        known = np.isfinite(z)
        nib = ((a > ferns["t_i"]) * 1 + (a > b) * 2 + (known & (z > ferns["t_z"])) * 4 + known * 8).astype(np.uint32)
    return np.bitwise_or.reduce(nib.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32)), axis=1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 65536, 1048576])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("keyframe_codes_rate: no GPU; a rate is measured on the device or not at all")
    ctx = d.default_context()
    rng = np.random.default_rng(1)
    out = {"m": M, "k": K, "reps": a.reps, "library": _lib.LIB_PATH, "hbm_peak_Bps": HBM_PEAK,
           "timing": "host clock around the whole call, which ends in a wait for the context's stream", "searches": []}
    for n in a.sizes:
        # codes scattered round one base code, as the codes of one environment are: distances of a few dozen to a few hundred ferns
        base = rng.integers(0, 1 << 32, M // 8, dtype=np.uint64).astype(np.uint32)
        noise = rng.integers(0, 1 << 32, (n, M // 8), dtype=np.uint64).astype(np.uint32)
        codes = base ^ (noise & rng.integers(0, 1 << 32, (n, M // 8), dtype=np.uint64).astype(np.uint32))
        book = d.KeyframeCodebook(ctx, m=M, capacity=n, seed=0)
        book.add_codes(torch.from_numpy(codes.view(np.int32)).cuda())
        for nq in a.queries:
            queries = codes[rng.integers(0, n, nq)] ^ (rng.integers(0, 1 << 32, (nq, M // 8), dtype=np.uint64).astype(np.uint32) & np.uint32(0x01010101))
            dev_q = torch.from_numpy(queries.view(np.int32)).cuda()
            rows, ms = timed(lambda: book.query_codes(dev_q, k=K, device=True), a.warmup, a.reps)
            rows = rows.cpu().numpy().view(np.uint32).view(d.CODE_MATCH_DTYPE).reshape(nq, K)
            want, ms_np = timed(lambda: numpy_search(codes, queries, K), 0, max(2, a.reps // 3))
            tiles = (nq + 15) // 16
            model = n * (M // 2) * tiles + 2.0 * nq * n * 4 + 8.0 * K * nq        # the matrix: written once, read three times
            out["searches"].append({"entries": n, "queries": nq, "equals_numpy": bool(np.array_equal(rows, want)),
                                    "device": {"call_ms": ms, "us_per_query": round(ms["median"] * 1e3 / nq, 3), "model_bytes": model,
                                               "achieved_fraction_of_hbm_peak": round(model / (ms["median"] * 1e-3) / HBM_PEAK, 5)},
                                    "numpy": {"call_ms": ms_np, "us_per_query": round(ms_np["median"] * 1e3 / nq, 3)},
                                    "numpy_over_device": round(ms_np["median"] / ms["median"], 2)})
        book.close()
    # the encoding of many frames at a coarse level
    W, H, level = 640, 480, 4
    pair = datagen.synth_pair(3, W, H)
    I0 = pair["grey_ref"].astype(np.float32)
    Z0 = pair["depth_ref"].astype(np.float32) * np.float32(2e-4)
    Z0[pair["depth_ref"] == 0] = np.nan
    cam = d.RgbdCameraPyramid(W, H, np.ascontiguousarray(pair["K"], np.float32), ctx)
    cam.build(level + 1)
    frames = [cam.create(np.roll(I0, (i % 7, 3 * i), (0, 1)), np.roll(Z0, (i % 5, 2 * i), (0, 1))) for i in range(a.frames)]
    for f in frames:
        f.build(level + 1)
    book = d.KeyframeCodebook(ctx, m=M, capacity=a.frames, seed=0)
    book.encode(frames, level)                                     # (the level's {I, Z} pairs are built where a frame lacks them: not timed)
    got, ms = timed(lambda: book.encode(frames, level, device=True), a.warmup, a.reps)
    planes = [(np.array(f.level(level).intensity), np.array(f.level(level).depth)) for f in frames]
    ferns = book.ferns()
    want, ms_host = timed(lambda: np.stack([numpy_encode(I, Z, ferns) for I, Z in planes]), 0, 3)
    out["encode"] = {"frames": a.frames, "width": W >> level, "height": H >> level, "level": level,
                     "equals_numpy": bool(np.array_equal(got.cpu().numpy().view(np.uint32), want)),
                     "device": {"call_ms": ms, "us_per_frame": round(ms["median"] * 1e3 / a.frames, 3)},
                     "numpy_over_downloaded_planes": {"call_ms": ms_host, "us_per_frame": round(ms_host["median"] * 1e3 / a.frames, 3)}}
    book.close()
    print(json.dumps(out))
    if not (out["encode"]["equals_numpy"] and all(s["equals_numpy"] for s in out["searches"])):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
