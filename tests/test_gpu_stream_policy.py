"""GPU tier (-m gpu): the option "stream_policy" (include/dvo_hip.h) changes the cache policy of the build stream's strip kernels and
nothing else.  The streaming loop of bench.py (re-ingest of the next batch on the build stream beside the alignment of the current one)
runs in two contexts, the option on in one and off in the other; every step's results and records, the iteration records of a
batched match over the ingested frames, and the intensity and depth planes of levels 1-3 of those frames must be the same bit for bit.
(The pipeline ingests its frames straight into their roles without a copy of the raw planes: level 0 holds only the role planes, which
the records are computed from.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
from dvo_slam_amd import _lib, datagen
from dvo_slam_amd.stream import StreamPipeline

pytestmark = pytest.mark.gpu

W, H, B, LEVELS = 640, 480, 48, 4
NAMES = ("intensity", "depth")


@pytest.fixture(scope="module")
def planes():
    b = datagen.synth_batch(901, 8, W, H)
    order = [(5 * i + 3) % 8 for i in range(B)]
    dev = torch.device("cuda", 0)
    grey = torch.from_numpy(np.concatenate([b["grey_ref"][order], b["grey_cur"][order]])).to(dev)
    depth = torch.from_numpy(np.concatenate([b["depth_ref"][order], b["depth_cur"][order]]).view(np.int16)).to(dev)
    torch.cuda.synchronize()
    return dict(K=b["K"], grey=grey, depth=depth, gp=[grey[i].data_ptr() for i in range(2 * B)], zp=[depth[i].data_ptr() for i in range(2 * B)])


def run(planes, policy, steps=3):
    ctx = d.Context(0)
    ctx.set_option("stream_policy", policy)
    cam = d.RgbdCameraPyramid(W, H, planes["K"], ctx)
    cam.build(LEVELS)
    gp, zp = planes["gp"], planes["zp"]
    sets = [[cam.create_raw_device(gp[i], zp[i]) for i in range(2 * B)] for _ in range(2)]
    cfg = d.Config(FirstLevel=3, LastLevel=0)
    pipe = StreamPipeline(ctx, cfg, [d.FrameSet(fs[:B]) for fs in sets], [d.FrameSet(fs[B:]) for fs in sets], gp[:B], zp[:B], gp[B:], zp[B:])
    pipe.step(now=None, nxt=0)
    out = {"results": [], "records": []}
    for k in range(steps):
        out["results"].append(pipe.step(now=k % 2, nxt=(k + 1) % 2).tobytes())
        out["records"].append(pipe.records().copy())
    # the iteration records of a batched match over the frames the last step ingested
    fs = sets[steps % 2]
    n, nl = B, cfg.FirstLevel - cfg.LastLevel + 1
    cap_it = nl * cfg.MaxIterationsPerLevel
    vp = C.c_void_p
    refs, curs = (vp * n)(*[f.ptr for f in fs[:B]]), (vp * n)(*[f.ptr for f in fs[B:]])
    cres = (_lib.Result * n)()
    for r in cres:
        for k in (0, 5, 10, 15):
            r.transformation[k] = 1.0
    levels, iters = (_lib.LevelStats * (n * nl))(), (_lib.IterationStats * (n * cap_it))()
    ccfg = cfg.to_c()
    ctx.check(ctx._lib.dvo_hip_match_batch(ctx.ptr, n, refs, curs, C.byref(ccfg), cres, levels, nl, iters, cap_it))
    out["batch"] = (bytes(cres), bytes(levels), bytes(iters))
    # the float planes of levels 1-3 of both buffers' frames (the second buffer: ingested by the steps before)
    out["planes"] = [[np.asarray(getattr(f.level(l), name)).copy() for l in range(1, LEVELS) for name in NAMES] for s in sets for f in s]
    out["ingests"] = ctx.counter("strip_ingests")
    return out


def test_stream_policy_changes_no_bit(planes):
    on, off = run(planes, 1), run(planes, 0)
    assert on["ingests"] > 0 and on["ingests"] == off["ingests"]          # the strip kernels ran, as often in both
    for k, (a, b) in enumerate(zip(on["results"], off["results"])):
        assert a == b, ("results of step", k)
    for k, (a, b) in enumerate(zip(on["records"], off["records"])):
        assert np.array_equal(a, b, equal_nan=True), ("records of step", k)
        assert np.isfinite(a[:, :6]).all(), ("step", k)
    for what, a, b in zip(("results", "level records", "iteration records"), on["batch"], off["batch"]):
        assert a == b, what
    for i, (fa, fb) in enumerate(zip(on["planes"], off["planes"])):
        for j, (a, b) in enumerate(zip(fa, fb)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), ("frame", i, "level", 1 + j // len(NAMES), NAMES[j % len(NAMES)])
