"""GPU tier (-m gpu): the streaming loop (dvo_slam_amd/apps/stream_pipeline.cpp, dvo_stream_step / dvo_stream_step_host / dvo_stream_lanes_*)
on frames that CHANGE from step to step.  Three batches rotate through the two frame sets (3 is coprime to 2: each set receives each
batch), 14 aligned steps behind the priming one -- the build-ticket ring (16) and the upload ring (3) wrap -- and every step's output is
held to what that step's batch must give.  With the same planes at every step a stale plane is bit-equal to a fresh one: a missing wait
for the build, a recorded ingest that is dropped or lands in the other buffer, a role plane or flag left over from the previous step, a
build table served from the cache for other addresses, an upload buffer overwritten too early or a result slot handed out a step late
would all pass.  Here each of them puts another batch's record, or a mixture, where this batch's belongs.

Expected values, none of them the overlapped loop itself:
 1. the QUIET loop: the same entry point with nothing concurrent (ingest, device idle, match) in a context of its own -- the overlapped
    loop reproduces it bit for bit, every byte of the results (the NaNs of the pair without depth included) and the packed records;
 2. PLAIN frames (create_raw_device + match_batch at the same n): the quiet loop agrees to a twist error below 2e-6 per pair (the bound
    tests/test_gpu_stream_lanes.py holds another batch-size class of the schedule to; streamed frames take other plans, so no bit
    identity), and the float planes of levels 1 and up of the frames the loop ingested last are bit-equal to the plain frames'
    (whose pyramid tests/test_gpu_parity.py::test_pyramid_planes_bit_exact pins to the oracle);
 3. the ORACLE (MATH mode, CPU): every distinct pair of the small shapes, twist error below 2e-5
    (tests/test_gpu_parity.py::test_random_whole_matches_against_oracle at this precision).

Batch sizes come from the context's policy counters; the values in brackets are those at 256 compute units:
  direct     cus/32 [8]         whole match resident, results direct; ingest deferred; taps ingested
  no_taps    cus/8 + 8 [40]     level-0 taps skipped at ingest (ingest_skips_taps) and derived by the match, or -- 640 x 480 -- the first
                                level alone resident because the window level below it holds no taps (window_taps_missing); deferred
  hand_over  3 cus/4 + 8 [200]  launch path with the level hand-over; deferred with the long lead
  beside     cus + 44 [300]     not deferred: the ingest runs beside the whole match; finish launch, short gather tiles
Each case asserts by counters that it ran in the class it names."""
import ctypes as C

import numpy as np
import pytest
import torch

import common as cm
import dvo_slam_amd as d
from dvo_slam_amd import datagen
from dvo_slam_amd.stream import StreamLanes, StreamPipeline
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

K, STEPS, PAIRS = 3, 14, 6
SEEDS = (2100, 2200, 2300)
# position i of batch b holds pair (stride * i + offset) % 6 of the batch: neighbours differ, a position's index differs from batch to
# batch (only 1 and 5 are coprime to 6: the third batch takes the first's stride at another offset; its pairs are others anyway)
DEAL = ((1, 0), (5, 2), (1, 3))
HOLES_BATCH, HOLES_POS = 1, 1                 # this position of this batch: depth planes all 0 (no depth anywhere)
LAST = STEPS % K                              # the batch the last step ingests (into set STEPS % 2)
SIZES = ("direct", "no_taps", "hand_over", "beside")
NAMES = ("intensity", "depth")
WATCHED = ("resident_timeouts", "f16_range_repeats")          # both legitimately change last bits (include/dvo_hip.h)
COUNTERS = ("deferred_ingests", "resident_launches", "resident_levels", "strip_ingests") + WATCHED

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def device_idle():
    """the whole device, as bench.py's barrier waits for it; and through every HIP runtime the process holds, should the library have loaded
    another one than torch's (found as tests/test_gpu_parity.py::test_device_ingest_prepare_and_background_build finds it)"""
    torch.cuda.synchronize()
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    if len(loaded) > 1:
        for path in loaded:
            assert C.CDLL(path).hipDeviceSynchronize() == 0


def policy():
    def make():
        ctx = d.Context(0)
        cus, defer_max = ctx.counter("compute_units"), ctx.counter("defer_ingest_max_pairs")
        ctx.close()
        return dict(cus=cus, defer_max=defer_max, n=dict(direct=cus // 32, no_taps=cus // 8 + 8, hand_over=3 * cus // 4 + 8, beside=cus + 44))
    return cached("policy", make)


def config_of(levels):
    return d.Config(FirstLevel=levels - 1, LastLevel=0)


def dealt(b, idx):
    s, o = DEAL[b]
    return [(s * i + o) % PAIRS for i in idx]


def scene(w, h):
    return cached(("scene", w, h), lambda: [datagen.synth_batch(seed, PAIRS, w, h) for seed in SEEDS])


def host_planes(w, h, b, idx):
    """the raw planes of batch b at the positions idx: grey [2 n, h, w] u8 and depth [2 n, h, w] u16, references first"""
    bt, order = scene(w, h)[b], dealt(b, idx)
    grey = np.concatenate([bt["grey_ref"][order], bt["grey_cur"][order]])
    depth = np.concatenate([bt["depth_ref"][order], bt["depth_cur"][order]])
    if b == HOLES_BATCH and HOLES_POS in idx:
        j = list(idx).index(HOLES_POS)
        depth[j] = 0
        depth[len(idx) + j] = 0
    return grey, depth


class DevicePlanes:
    """one resident plane set: 2 n raw frames and their addresses"""

    def __init__(self, grey, depth):
        dev = torch.device("cuda", 0)
        self.grey, self.depth = torch.from_numpy(grey).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev)
        torch.cuda.synchronize()
        n2 = grey.shape[0]
        self.n = n2 // 2
        self.gp, self.zp = [self.grey[i].data_ptr() for i in range(n2)], [self.depth[i].data_ptr() for i in range(n2)]

    def roles(self):
        n = self.n
        return self.gp[:n], self.zp[:n], self.gp[n:], self.zp[n:]

    def overwrite(self, other):
        """... with another set's contents; returns when the copy is done"""
        self.grey.copy_(other.grey)
        self.depth.copy_(other.depth)
        torch.cuda.synchronize()


def device_sets(w, h, idx):
    return cached(("device", w, h, idx), lambda: [DevicePlanes(*host_planes(w, h, b, idx)) for b in range(K)])


def counters(ctx):
    return {k: ctx.counter(k) for k in COUNTERS}


def advance(ctx, before):
    return {k: ctx.counter(k) - before[k] for k in COUNTERS}


def new_pipeline(w, h, levels, idx, planes):
    """a context of its own, two frame sets of n pairs (created from `planes`, which every case ingests over) and the pipeline on them"""
    n = len(idx)
    ctx = d.Context(0)
    cam = d.RgbdCameraPyramid(w, h, scene(w, h)[0]["K"], ctx)
    cam.build(levels)
    sets = [[cam.create_raw_device(planes.gp[i], planes.zp[i]) for i in range(2 * n)] for _ in range(2)]
    pipe = StreamPipeline(ctx, config_of(levels), [d.FrameSet(fs[:n]) for fs in sets], [d.FrameSet(fs[n:]) for fs in sets], *planes.roles())
    device_idle()
    return ctx, sets, pipe


def quiet_loop(w, h, levels, idx):
    """Tier 1: per batch, ingest with nothing else going on, wait for the device, align with nothing else going on.  -> per batch the
    result array and the packed records; the counters' advance."""
    def make():
        planes = device_sets(w, h, idx)
        ctx, sets, pipe = new_pipeline(w, h, levels, idx, planes[0])
        before = counters(ctx)
        out = dict(results=[], records=[])
        for b in range(K):
            pipe.set_device_planes(*planes[b].roles())
            pipe.step(now=None, nxt=b % 2)
            device_idle()
            out["results"].append(pipe.step(now=b % 2, nxt=None).copy())
            out["records"].append(pipe.records().copy())
            device_idle()
        out["advance"] = advance(ctx, before)
        for k in WATCHED:
            assert out["advance"][k] == 0, "the quiet loop's %s advanced by %d: its last bits are another schedule's" % (k, out["advance"][k])
        # before anything else: at every position the three batches' records differ pairwise as bytes -- a swap of batches cannot pass
        for i in range(len(idx)):
            assert len({out["results"][b][i].tobytes() for b in range(K)}) == K, ("position", idx[i], "has the same record in two batches")
        if HOLES_POS in idx:
            r = out["results"][HOLES_BATCH][list(idx).index(HOLES_POS)]
            assert np.array_equal(r["transformation"].reshape(4, 4), np.eye(4)) and np.isnan(r["information"]).all()
        del pipe, sets
        ctx.close()
        return out
    return cached(("quiet", w, h, levels, idx), make)


def plain_frames(w, h, levels, idx):
    """Tier 2's reference: frames created from the same planes, aligned as one batch of the same n.  -> per batch the transforms; the
    float planes of levels 1 and up of batch LAST's frames."""
    def make():
        n = len(idx)
        ctx = d.Context(0)
        cam = d.RgbdCameraPyramid(w, h, scene(w, h)[0]["K"], ctx)
        cam.build(levels)
        trk = d.DenseTracker(config_of(levels), ctx)
        out = dict(T=[])
        for b, planes in enumerate(device_sets(w, h, idx)):
            frames = [cam.create_raw_device(planes.gp[i], planes.zp[i]) for i in range(2 * n)]
            out["T"].append(trk.match_batch_arrays(frames[:n], frames[n:])["T"])
            if b == LAST:
                out["planes"] = [[np.asarray(getattr(f.level(l), name)).tobytes() for l in range(1, levels) for name in NAMES] for f in frames]
            del frames
        ctx.close()
        return out
    return cached(("plain", w, h, levels, idx), make)


def oracle_matches(w, h, levels):
    """Tier 3's reference: the 18 pairs and the pair without depth, aligned once on the CPU"""
    def make():
        cfg = cm.oracle_config_from(config_of(levels), po.MATH)
        out = {}
        for b, bt in enumerate(scene(w, h)):
            for p in range(PAIRS):
                pair = {k: bt[k][p] for k in ("grey_ref", "depth_ref", "grey_cur", "depth_cur")}
                pair["K"] = bt["K"]
                out[b, p] = po.match(*po.pyramids_from_pair(pair, levels), cfg)
        grey, depth = host_planes(w, h, HOLES_BATCH, (HOLES_POS,))
        holes = dict(grey_ref=grey[0], depth_ref=depth[0], grey_cur=grey[1], depth_cur=depth[1], K=scene(w, h)[0]["K"])
        out["holes"] = po.match(*po.pyramids_from_pair(holes, levels), cfg)
        return out
    return cached(("oracle", w, h, levels), make)


def explain(got, want_all, b, idx):
    """which positions of a step's results differ from batch b's, and whose records they hold instead"""
    notes = []
    for i in range(len(idx)):
        if got[i].tobytes() == want_all[b][i].tobytes():
            continue
        other = [j for j in range(K) if j != b and got[i].tobytes() == want_all[j][i].tobytes()]
        Tg, Tw = got[i]["transformation"].reshape(4, 4), want_all[b][i]["transformation"].reshape(4, 4)
        err = cm.twist_matrix_error(Tg, Tw) if np.isfinite(Tg).all() and np.isfinite(Tw).all() else float("nan")
        notes.append((idx[i], "batch %d's record (stale)" % other[0] if other else "no batch's record", "twist error %.3g" % err))
    return "%d of %d positions differ from batch %d; the first: %s" % (len(notes), len(idx), b, notes[:6])


def check_step(pipe, quiet, b, idx, step):
    got = pipe.results
    assert got.tobytes() == quiet["results"][b].tobytes(), ("results of step", step, explain(got, quiet["results"], b, idx))
    assert np.array_equal(pipe.records(), quiet["records"][b], equal_nan=True), ("records of step", step)


# pyramid levels the resident kernel runs per match, by shape and size class (plan_resident, dvo_slam_amd/csrc/capi_schedule.inc, with the
# thresholds of batch_policy.h): up to cus/4 pairs the coarse-level plan takes every level whose rows fit, which at the small shapes is the
# whole match -- the level-0 taps the ingest left out from cus/8 frames on are derived by the match; at 640 x 480 the level below the first
# is a window level that holds no taps, and the first level alone runs resident (window_taps_missing); beyond 7 cus/16 pairs: none.
def resident_levels_per_match(w, levels, size):
    if size == "direct":
        return levels
    if size == "no_taps":
        return 1 if w == 640 else levels
    return 0


def check_class(w, levels, size, n, adv, quiet, matches, deferred_steps):
    for k in WATCHED:
        assert adv[k] == 0, "%s advanced by %d in the overlapped loop: its last bits are another schedule's, not a data race" % (k, adv[k])
    assert adv["deferred_ingests"] == 2 * deferred_steps, adv
    per_match = resident_levels_per_match(w, levels, size)
    assert adv["resident_launches"] == (matches if per_match else 0), adv
    assert adv["resident_levels"] == per_match * matches, adv
    # the quiet loop ran the same plan
    assert quiet["advance"]["resident_launches"] * matches == adv["resident_launches"] * K, (quiet["advance"], adv)
    assert quiet["advance"]["resident_levels"] * matches == adv["resident_levels"] * K, (quiet["advance"], adv)
    assert (adv["strip_ingests"] > 0) == (w % 4 == 0), adv               # the strip ingest, or the tile ingest


def check_planes(sets, plain, levels):
    """the frames of the set ingested last against the plain frames of that batch"""
    for i, f in enumerate(sets[STEPS % 2]):
        got = [np.asarray(getattr(f.level(l), name)).tobytes() for l in range(1, levels) for name in NAMES]
        for j, (a, b) in enumerate(zip(got, plain["planes"][i])):
            assert a == b, ("frame", i, "level", 1 + j // len(NAMES), NAMES[j % len(NAMES)])


SHAPES = {160: (160, 120, 3), 102: (102, 78, 3), 640: (640, 480, 4)}
CASES = [(160, "direct"), (160, "no_taps"), (160, "hand_over"), (160, "beside"), (102, "no_taps"), (102, "beside"), (640, "no_taps")]


@pytest.mark.parametrize("shape,size", CASES)
def test_quiet_loop_against_plain_frames_and_oracle(shape, size):
    """Tiers 2 and 3: what the overlapped loop is held to bit for bit is itself held to the library's plain path and to the oracle."""
    w, h, levels = SHAPES[shape]
    n = policy()["n"][size]
    idx = tuple(range(n))
    quiet, plain = quiet_loop(w, h, levels, idx), plain_frames(w, h, levels, idx)
    worst = 0.0
    for b in range(K):
        T = quiet["results"][b]["transformation"].reshape(n, 4, 4)
        assert np.isfinite(T).all()
        errs = [cm.twist_matrix_error(T[i], plain["T"][b][i]) for i in range(n)]
        worst = max(worst, max(errs))
        assert max(errs) < 2e-6, ("batch", b, "position", int(np.argmax(errs)), max(errs))
    print("%d x %d, %d pairs: quiet loop against plain frames, worst twist error %.3g" % (w, h, n, worst))
    if shape == 640:
        return
    oracle = oracle_matches(w, h, levels)
    worst = 0.0
    for b in range(K):
        order = dealt(b, idx)
        T = quiet["results"][b]["transformation"].reshape(n, 4, 4)
        for p in range(PAIRS):
            first = [i for i in range(n) if order[i] == p and not (b == HOLES_BATCH and i == HOLES_POS)][0]
            err = cm.twist_matrix_error(T[first], oracle[b, p]["T"])
            worst = max(worst, err)
            assert err < 2e-5, ("batch", b, "pair", p, "position", first, err)
    # the pair without depth, as tests/test_emul_device.py::test_state_machine_edge_cases pins it: identity, NaN information, the oracle's passes
    o, r = oracle["holes"], quiet["results"][HOLES_BATCH][HOLES_POS]
    assert np.array_equal(o["T"], np.eye(4)) and np.isnan(o["information"]).all()
    assert np.array_equal(r["transformation"].reshape(4, 4), np.eye(4)) and np.isnan(r["information"]).all()
    assert r["n_iterations_total"] == sum(len(L["iterations"]) for L in o["levels"])
    print("%d x %d, %d pairs: quiet loop against the oracle, worst twist error %.3g" % (w, h, n, worst))


@pytest.mark.parametrize("mode", ["rotating", "fixed"])
@pytest.mark.parametrize("shape,size", CASES)
def test_overlapped_loop_reproduces_the_quiet_loop(shape, size, mode):
    """dvo_stream_step from device planes.  rotating: three resident plane sets, the step's source addresses switched (a build table for
    other addresses every step); fixed: one staging set per frame set, overwritten with the next batch once the match of the frames it fed
    has returned (the contract of dvo_hip_frames_update_raw_device_as_ex) -- the same tables, new contents."""
    w, h, levels = SHAPES[shape]
    n = policy()["n"][size]
    idx = tuple(range(n))
    quiet, planes = quiet_loop(w, h, levels, idx), device_sets(w, h, idx)
    if mode == "fixed":
        staging = [DevicePlanes(*host_planes(w, h, 0, idx)) for _ in range(2)]
    ctx, sets, pipe = new_pipeline(w, h, levels, idx, planes[0])

    def feed(b, s):
        if mode == "rotating":
            pipe.set_device_planes(*planes[b].roles())
        else:
            staging[s].overwrite(planes[b])
            pipe.set_device_planes(*staging[s].roles())
    before = counters(ctx)
    feed(0, 0)
    pipe.step(now=None, nxt=0)
    for k in range(STEPS):                        # step k aligns batch k % 3 in set k % 2 and ingests batch (k + 1) % 3 into the other
        feed((k + 1) % K, (k + 1) % 2)
        pipe.step(now=k % 2, nxt=(k + 1) % 2)
        check_step(pipe, quiet, k % K, idx, k)
    adv = advance(ctx, before)
    print("%d x %d, %d pairs (%s), %s addresses: %s" % (w, h, n, size, mode, adv))
    assert (n <= policy()["defer_max"]) == (size != "beside")
    check_class(w, levels, size, n, adv, quiet, STEPS, STEPS if size != "beside" else 0)
    check_planes(sets, plain_frames(w, h, levels, idx), levels)
    device_idle()
    del pipe, sets
    ctx.close()


@pytest.mark.parametrize("size", ["no_taps", "beside"])
def test_overlapped_loop_from_host_memory(size):
    """dvo_stream_step_host: three pinned plane sets switched per step, two uploads per step through the upload ring of three"""
    w, h, levels = SHAPES[160]
    n = policy()["n"][size]
    idx = tuple(range(n))
    quiet, planes = quiet_loop(w, h, levels, idx), device_sets(w, h, idx)
    ctx, sets, pipe = new_pipeline(w, h, levels, idx, planes[0])
    pinned = [d.PinnedRawPlanes(ctx, 2 * n, w, h) for _ in range(K)]
    for b, P in enumerate(pinned):
        grey, depth = host_planes(w, h, b, idx)
        for i in range(2 * n):
            P.grey[i][:], P.depth[i][:] = grey[i], depth[i]

    def feed(b):
        P = pinned[b]
        pipe.set_host_planes(P.grey[:n], P.depth[:n], P.grey[n:], P.depth[n:])
    before = counters(ctx)
    feed(0)
    pipe.step_host(now=None, nxt=0)
    for k in range(STEPS):
        feed((k + 1) % K)
        pipe.step_host(now=k % 2, nxt=(k + 1) % 2)
        check_step(pipe, quiet, k % K, idx, k)
    adv = advance(ctx, before)
    print("%d x %d, %d pairs (%s), host planes: %s" % (w, h, n, size, adv))
    check_class(w, levels, size, n, adv, quiet, STEPS, 0)               # (the host entry points do not defer)
    check_planes(sets, plain_frames(w, h, levels, idx), levels)
    d.upload_wait(ctx)
    device_idle()
    del pipe, sets
    for P in pinned:
        P.close()
    ctx.close()


@pytest.mark.parametrize("n_lanes", [2, 3])
def test_lanes_on_planes_that_change(n_lanes):
    """StreamLanes, one step in flight, on fixed addresses whose contents change between a step's collection and the next submission.
    Step k aligns what step k - 1 ingested: per lane shard, the quiet loop's records of the shard's pairs at the shard's n."""
    w, h, levels = SHAPES[160]
    n = policy()["n"]["beside"]
    idx = tuple(range(n))
    shards = [tuple(range(l, n, n_lanes)) for l in range(n_lanes)]
    quiet, planes = [quiet_loop(w, h, levels, s) for s in shards], device_sets(w, h, idx)
    # a shard's expected value is tied to tiers 2 and 3 through the quiet loop of all n pairs: another batch-size class, 2e-6
    whole = quiet_loop(w, h, levels, idx)
    for l, s in enumerate(shards):
        for b in range(K):
            Ts, Tw = quiet[l]["results"][b]["transformation"].reshape(-1, 4, 4), whole["results"][b]["transformation"].reshape(n, 4, 4)[l::n_lanes]
            assert max(cm.twist_matrix_error(Ts[i], Tw[i]) for i in range(len(s))) < 2e-6, ("lane", l, "batch", b)
    staging = DevicePlanes(*host_planes(w, h, 0, idx))
    ctxs = [d.Context(0) for _ in range(n_lanes)]
    cams = {}
    for c in ctxs:
        cams[id(c)] = d.RgbdCameraPyramid(w, h, scene(w, h)[0]["K"], c)
        cams[id(c)].build(levels)
    gp, zp = staging.gp, staging.zp

    def make_frames(c, ids):
        return ([cams[id(c)].create_raw_device(gp[i], zp[i]) for i in ids], [cams[id(c)].create_raw_device(gp[n + i], zp[n + i]) for i in ids])
    lanes = StreamLanes(ctxs, config_of(levels), n, make_frames, *staging.roles(), depth=1)      # (set 0 of every lane: batch 0)
    before = [counters(c) for c in ctxs]
    device_idle()
    staging.overwrite(planes[1])
    for k in range(2 * K):                        # step k aligns batch k % 3 and ingests what the planes hold: batch (k + 1) % 3
        lanes.submit()
        got, rec = lanes.collect().copy(), lanes.records().copy()
        device_idle()                             # the ingest of the step just collected may still be reading
        staging.overwrite(planes[(k + 2) % K])
        for l, s in enumerate(shards):
            b = k % K
            assert got[l::n_lanes].tobytes() == quiet[l]["results"][b].tobytes(), \
                ("step", k, "lane", l, explain(got[l::n_lanes], quiet[l]["results"], b, s))
            assert np.array_equal(rec[l::n_lanes], quiet[l]["records"][b], equal_nan=True), ("records of step", k, "lane", l)
    for l, c in enumerate(ctxs):
        adv = advance(c, before[l])
        print("%d lanes, lane %d, %d pairs: %s" % (n_lanes, l, len(shards[l]), adv))
        for key in WATCHED:
            assert adv[key] == 0, "%s advanced by %d on lane %d: its last bits are another schedule's, not a data race" % (key, adv[key], l)
        assert adv["deferred_ingests"] == 2 * 2 * K and adv["strip_ingests"] > 0, adv     # a shard is below the deferral's limit
        assert quiet[l]["advance"]["resident_levels"] * 2 == adv["resident_levels"], (quiet[l]["advance"], adv)
    lanes.close()
    device_idle()
    del lanes
    for c in ctxs:
        c.close()
