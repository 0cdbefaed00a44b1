"""Cost of keyframe sub-maps (profiles/keyframe_map_merge.md): merge, move and export of voxel tables against the frame-based calls
that existed before them.  Prints one JSON line.

k sub-maps of m keyframes of 640 x 480 each (the input of scripts/keyframe_map_rate.py), built in the coordinates of their first
keyframe.  Three steps, each in a child process of its own under a time limit (a step that hangs or faults ends the measurement: the
steps behind it are not started), each call timed with HIP events on the context's stream around the call (which includes the call's
own small transfers and its read-back of the map's counters):
  move     KeyframeMap.move_submaps of the k sub-maps (one launch over 2 k tables) against KeyframeMap.move of the same k m keyframes'
           frames (one launch over 2 k m frames) in a map built from the frames: the yardstick, it needs every frame resident;
  merge    a plain KeyframeMap.merge of the frame-built table into an empty table of the same capacity against KeyframeMap.rehash of
           that table: the same walk and the same claims;
  export   KeyframeMap.export(device=True) against KeyframeMap.extract(device=True).
GB/s: bytes of SOURCE TABLE walked (32 per slot) per second.  The kernels' own times come from
    rocprofv3 --kernel-trace --stats -- python scripts/keyframe_map_merge_rate.py --step move ...
(k_map_merge, k_map_export against k_map_insert, k_map_rehash, k_map_extract).

    python scripts/keyframe_map_merge_rate.py [--submaps 5] [--frames 10] [--leaf 0.01] [--capacity 4194304] [--submap-capacity 2097152]
                                              [--reps 10] [--warmup 2] [--limit 240]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("move", "merge", "export")
W, H = 640, 480


def run_step(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import dvo_slam_amd as d
    from dvo_slam_amd import datagen

    k, m = a.submaps, a.frames
    ctx = d.default_context()
    stream = torch.cuda.ExternalStream(ctx._lib.dvo_hip_context_stream(ctx.ptr))
    pair = datagen.synth_pair(3, W, H)
    I0 = pair["grey_ref"].astype(np.float32)
    Z0 = pair["depth_ref"].astype(np.float32) * np.float32(2e-4)
    Z0[pair["depth_ref"] == 0] = np.nan
    cam = d.RgbdCameraPyramid(W, H, pair["K"], ctx)
    cam.build(1)
    frames, poses = [], []
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(ctx.device)[0]
    for i in range(k * m):
        frames.append(cam.create(np.roll(I0, (i % 7, 3 * i), (0, 1)), Z0))
        T = np.eye(4)
        th = 0.001 * i
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
        T[:3, 3] = [0.004 * i, 0.001 * i, 0.002 * i]
        poses.append(T)
    poses = np.stack(poses)
    ctx.check(ctx._lib.dvo_hip_upload_wait(ctx.ptr))
    torch.cuda.synchronize()
    # what a keyframe keeps in device memory while its frame lives (the allocator's granularity included)
    frame_bytes = (free_before - torch.cuda.mem_get_info(ctx.device)[0]) // (k * m)
    anchors = poses[::m].copy()
    twist = np.eye(4)
    twist[0, 1], twist[1, 0], twist[:3, 3] = -0.002, 0.002, [0.003, -0.002, 0.001]
    anchors_new = anchors @ twist
    # a keyframe moves rigidly with its anchor: T_i' = T_anchor' T_anchor^-1 T_i
    poses_new = np.stack([anchors_new[i // m] @ np.linalg.inv(anchors[i // m]) @ poses[i] for i in range(k * m)])

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        call()
        end.record(stream)
        end.synchronize()
        return start.elapsed_time(end)

    def measure(steps):
        times = {name: [] for name, _ in steps if name}
        for rep in range(a.warmup + a.reps):
            for name, call in steps:
                ms = timed(call)
                if name and rep >= a.warmup:
                    times[name].append(ms)
        return {name: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}
                for name, v in times.items()}

    gbs = lambda slots, ms: round(slots * 32 / (ms * 1e-3) / 1e9, 2)
    out = {"step": a.step, "frame_resident_bytes": int(frame_bytes)}
    if a.step == "move":
        subs = []
        for g in range(k):
            s = d.KeyframeMap(ctx, a.leaf, a.submap_capacity)
            s.insert(frames[g * m:(g + 1) * m], np.stack([np.linalg.inv(anchors[g]) @ T for T in poses[g * m:(g + 1) * m]]))
            subs.append(s)
        out["submap_stats"] = subs[0].stats()
        out["submap_live_voxel_bytes_per_keyframe"] = int((out["submap_stats"]["occupied"] - out["submap_stats"]["vacant"]) * 32 // m)
        from_tables, from_frames = d.KeyframeMap(ctx, a.leaf, a.capacity), d.KeyframeMap(ctx, a.leaf, a.capacity)
        from_tables.merge(subs, poses=anchors)
        from_frames.insert(frames, poses)
        out["ms"] = measure([("move_submaps", lambda: from_tables.move_submaps(subs, anchors, anchors_new)),
                             (None, lambda: from_tables.move_submaps(subs, anchors_new, anchors)),
                             ("move_frames", lambda: from_frames.move(frames, poses, poses_new)),
                             (None, lambda: from_frames.move(frames, poses_new, poses))])
        out["map_of_tables"], out["map_of_frames"] = from_tables.stats(), from_frames.stats()
        out["source_table_gb_per_s"] = gbs(2 * k * subs[0].info()["capacity"], out["ms"]["move_submaps"]["median"])
        out["frame_gb_per_s"] = round(2 * k * m * W * H * 8 / (out["ms"]["move_frames"]["median"] * 1e-3) / 1e9, 2)
    else:
        src = d.KeyframeMap(ctx, a.leaf, a.capacity)
        src.insert(frames, poses)
        out["source_stats"] = src.stats()
        slots = src.info()["capacity"]
        if a.step == "merge":
            dst = d.KeyframeMap(ctx, a.leaf, a.capacity)
            out["ms"] = measure([(None, dst.clear), ("merge_into_empty", lambda: dst.merge([src])), ("rehash", src.rehash)])
            a_, b_ = dst.extract(sort=True), src.extract(sort=True)
            out["merged_equals_source"] = bool(np.array_equal(a_[2], b_[2]) and np.array_equal(a_[0].view(np.uint32), b_[0].view(np.uint32)))
            out["source_table_gb_per_s"] = {name: gbs(slots, v["median"]) for name, v in out["ms"].items()}
        else:
            out["ms"] = measure([("export_device", lambda: src.export(device=True)), ("extract_device", lambda: src.extract(device=True))])
            out["source_table_gb_per_s"] = {name: gbs(slots, v["median"]) for name, v in out["ms"].items()}
            out["records"] = int(src.export(device=True)[0].shape[0])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process (what the driver starts its children with)")
    ap.add_argument("--submaps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=10, help="keyframes per sub-map")
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--submap-capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    a = ap.parse_args()
    if a.step:
        return run_step(a)
    # the driver: never touches the GPU itself
    out = {"submaps": a.submaps, "frames_per_submap": a.frames, "width": W, "height": H, "leaf": a.leaf, "capacity": a.capacity,
           "submap_capacity": a.submap_capacity, "reps": a.reps, "timing": "HIP events on the context's stream around each call", "steps": {}}
    passed = [x for x in sys.argv[1:]]
    for step in STEPS:
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + passed, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            out["steps"][step] = {"error": "no answer within %d s" % a.limit}
            break
        if child.returncode != 0:
            out["steps"][step] = {"error": "exit status %d" % child.returncode, "stderr": child.stderr[-2000:]}
            break
        out["steps"][step] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out["steps"].values()) and len(out["steps"]) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
