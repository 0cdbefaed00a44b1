"""The calls that read frames at one pyramid level through the C-ABI (dvo_slam_amd/csrc/capi_frame_calls.inc), all from one table: what
each refuses -- the return code, the text of dvo_hip_last_error, counters and outputs left alone -- and that host outputs are the device
outputs bit for bit when one call mixes frame sizes.  The codes and texts were recorded from the driver as it stood before the calls
shared their checks and their staging."""
import ctypes as C

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
from dvo_slam_amd import _lib
from test_gpu_f32_ingest import camera

pytestmark = pytest.mark.gpu
INF = float("inf")
COUNTERS = ("frame_warps", "covisibility_pairs", "codebook_encoded", "codebook_queries", "map_renders")
SENTINEL = 0xA5
M = 128                                  # ferns of the book: 16 words a code
vp, dp, i32p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)


def planes(k, w, h):
    """frame k: integer-valued formulas (as tests/test_gpu_frame_warp.py, facade_frame)"""
    y, x = np.mgrid[0:h, 0:w]
    I = ((x * 7 + y * 13 + k * 5) % 256).astype(np.float32)
    Z = (1000 + (x * 3 + y * 5 + k * 11) % 512).astype(np.float32) * np.float32(0.001)
    Z[(x // 2 + 2 * (y // 2) + k) % 29 == 0] = np.nan
    return I, Z


def motion(k):
    T = np.eye(4)
    T[0, 2], T[2, 0] = k / 1024.0, -k / 1024.0
    T[:3, 3] = [0.01 * k, -0.005 * k, 0.002 * k]
    return T


def handles(*pyramids):
    return (vp * len(pyramids))(*[p if p is None else p.ptr for p in pyramids])


class Outputs:
    """the output arrays of one call, sentinel-filled: byte arrays in host memory or -- device -- on the GPU, `skew` bytes off 256"""
    def __init__(self, sizes, device=False, skew=0):
        self.device = device
        self.arrays = [torch.full((s + 256,), SENTINEL, dtype=torch.uint8, device="cuda")[skew:skew + s] if device
                       else np.full(s, SENTINEL, np.uint8) for s in sizes]

    def address(self, k):
        a = self.arrays[k]
        return a.data_ptr() if self.device else a.ctypes.data

    def table(self, ks, null=None):
        return (vp * len(ks))(*[None if k == null else self.address(k) for k in ks])

    def bytes(self):
        if self.device:
            torch.cuda.synchronize()
        return [a.cpu().numpy() if self.device else a for a in self.arrays]

    def untouched(self):
        return all(np.all(b == SENTINEL) for b in self.bytes())


@pytest.fixture(scope="module")
def world():
    """two contexts; in the first, cameras of 32 x 24, 16 x 12 and 18 x 14 (level 1: 9 x 7, planes of 252 bytes) with two levels, frames
    of each, a map that holds some of them and a book that holds their codes"""
    ctx, other = d.default_context(), d.Context(0)
    K = lambda w, h: np.array([w * 0.9, w * 0.9, w / 2 - 0.5, h / 2 - 0.5], np.float32)      # noqa: E731
    cams = {s: camera(ctx, s[0], s[1], K(*s), 2) for s in ((32, 24), (16, 12), (18, 14))}
    frames = {s: [cam.create(*planes(k, *s)) for k in range(3)] for s, cam in cams.items()}
    foreign = camera(other, 32, 24, K(32, 24), 2).create(*planes(0, 32, 24))
    mixed = [frames[(18, 14)][0], frames[(32, 24)][0], frames[(16, 12)][0]]                  # a plane of 252 bytes in front of the others
    partner = {id(f): fs[(k + 1) % 3] for fs in frames.values() for k, f in enumerate(fs)}  # a frame's second in a pair: the next of its camera
    targets = [cams[(32, 24)].create(*planes(5, 32, 24)) for _ in range(2)]                  # what a render into frames overwrites
    m = d.KeyframeMap(ctx, 0.05, 1 << 14)
    m.insert(frames[(32, 24)][:2], np.stack([motion(0), motion(1)]))
    book = d.KeyframeCodebook(ctx, m=M, capacity=16)
    book.add(mixed + frames[(32, 24)][1:], 1)
    yield dict(ctx=ctx, other=other, frames=frames, foreign=foreign, mixed=mixed, partner=partner, targets=targets, map=m, book=book)
    m.close()
    book.close()
    del foreign
    other.close()


def pixels(pyramids, level):
    return [(p.camera.width >> level) * (p.camera.height >> level) for p in pyramids]


class Call:
    """One entry point with the arguments of a good call over `pyramids`; run(**changes) makes the call with some of them changed and
    returns its code.  sizes(): the bytes of its outputs."""
    transforms = text_null = text_align = None       # the rules it refuses a NaN transform, a null and a misaligned output with, if it does
    skew = 4                                         # bytes that break the alignment of its device outputs (2: the codes' 4)

    def __init__(self, world, pyramids, level=1):
        self.w, self.ctx, self.L = world, world["ctx"], world["ctx"]._lib
        self.pyramids, self.level = list(pyramids), level
        self.T = np.ascontiguousarray(np.stack([motion(k + 1) for k in range(self.items())]))

    def items(self):
        return len(self.pyramids)

    def run(self, device=False, skew=0, frames="good", n=None, level=None, T=None, null_output=False):
        self.out = Outputs(self.sizes(), device, skew)
        f = self.pyramids if frames == "good" else frames
        return self.call(self.ctx.ptr, len(self.pyramids) if n is None else n, None if f is None else handles(*f),
                         self.level if level is None else level, (self.T if T is None else T).ctypes.data_as(dp), self.out, 1 if device else 0,
                         null_output)


class Organised(Call):
    name, text_null, text_align = "frames_world_points", "null output", "a device output must be 16-byte aligned"

    def sizes(self):
        return [16 * n for n in pixels(self.pyramids, self.level)]

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        table = out.table(range(len(out.arrays)), null=1 if null_output else None)
        return getattr(self.L, "dvo_hip_" + self.name)(ctx, n, f, T, level, 0.0, INF, table, dev)


class Normals(Organised):
    name = "frames_normals"


class Insert(Call):
    name = "map_insert"

    def sizes(self):
        return []

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        return self.L.dvo_hip_map_insert(ctx, self.w["map"].ptr, n, f, T, level, 0.0, INF)


class WarpInverse(Call):
    name, text_null, text_align, transforms = "frames_warp_inverse", "null output", "a device plane must be 16-byte aligned", "a transform is not finite"

    def sizes(self):
        return [4 * n for n in pixels(self.pyramids, self.level)] * 3

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        k = len(self.pyramids)
        tables = [out.table(range(j * k, j * k + k), null=k + 1 if null_output else None) for j in range(3)]
        sampled = handles(*[self.w["partner"][id(p)] for p in self.pyramids])
        return self.L.dvo_hip_frames_warp_inverse(ctx, n, f, sampled, T, level, None, tables[0], tables[1], tables[2], dev)


class WarpForward(WarpInverse):
    name = "frames_warp_forward"

    def sizes(self):
        return [4 * n for n in pixels(self.pyramids, self.level)] * 2

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        k = len(self.pyramids)
        tables = [out.table(range(j * k, j * k + k), null=k + 1 if null_output else None) for j in range(2)]
        return self.L.dvo_hip_frames_warp_forward(ctx, n, f, T, level, None, tables[0], tables[1], dev)


class Covisibility(Call):
    name, text_null, text_align, transforms = "frames_covisibility", "bad argument", "device records must be 8-byte aligned", "a transform is not finite"
    PAIRS = np.array([(0, 1), (1, 2), (2, 0), (0, 0)], np.int32)

    def items(self):
        return len(self.PAIRS)

    def sizes(self):
        return [32 * len(self.PAIRS)]

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        a, b = np.ascontiguousarray(self.PAIRS[:, 0]), np.ascontiguousarray(self.PAIRS[:, 1])
        return self.L.dvo_hip_frames_covisibility(ctx, n, f, len(self.PAIRS), a.ctypes.data_as(i32p), b.ctypes.data_as(i32p), T, level, None,
                                                  None if null_output else vp(out.address(0)), dev)


class Encode(Call):
    name, text_null, text_align, skew = "frames_encode", "null codes_out", "device codes must be 4-byte aligned", 2

    def sizes(self):
        return [M // 8 * 4 * len(self.pyramids)]

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        return self.L.dvo_hip_frames_encode(ctx, self.w["book"].ptr, n, f, level, None if null_output else vp(out.address(0)), dev)


class Query(Call):
    name, text_null, text_align, K = "codebook_query_frames", "bad argument", "device result rows must be 8-byte aligned", 3

    def sizes(self):
        return [8 * self.K * len(self.pyramids), 2 * 5 * len(self.pyramids)]       # result rows, and distances to the book's five entries

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        return self.L.dvo_hip_codebook_query_frames(ctx, self.w["book"].ptr, n, f, level, self.K, None, None,
                                                    None if null_output else vp(out.address(0)), vp(out.address(1)), dev)


class RenderFrames(Call):
    name = "map_render_frames"

    def sizes(self):
        return []

    def call(self, ctx, n, f, level, T, out, dev, null_output):
        return self.L.dvo_hip_map_render_frames(ctx, self.w["map"].ptr, n, f, T, None, -1, None, 0)


CALLS = [Organised, Normals, Insert, WarpInverse, WarpForward, Covisibility, Encode, Query, RenderFrames]


@pytest.mark.parametrize("kind", CALLS, ids=lambda k: k.name)
def test_refusals_and_one_good_call(world, kind):
    ctx = world["ctx"]
    same_size = world["frames"][(32, 24)]
    call = kind(world, same_size)
    error = lambda: ctx._lib.dvo_hip_last_error(ctx.ptr).decode()                             # noqa: E731
    before = [ctx.counter(c) for c in COUNTERS]
    inserts = ctx.counter("map_inserts")
    nan = call.T.copy()
    nan[-1, 2, 3] = np.nan
    has_level = kind is not RenderFrames
    refusals = [("n = 0", dict(n=0), "bad argument"),
                ("a null list", dict(frames=None), "bad argument"),
                ("a null frame", dict(frames=[same_size[0], None, same_size[2]]), "null frame"),
                ("a frame of the other context", dict(frames=[same_size[0], same_size[1], world["foreign"]]), "a frame of another context"),
                ("level -1", dict(level=-1), "a frame does not have that level" if has_level else None),
                ("level 2", dict(level=2), "a frame does not have that level" if has_level else None),
                ("a NaN transform", dict(T=nan), call.transforms),
                ("a null output", dict(null_output=True), call.text_null if call.sizes() else None),
                ("a device output off by %d bytes" % call.skew, dict(device=True, skew=call.skew), call.text_align if call.sizes() else None)]
    for what, changes, rule in refusals:
        if rule is None:                     # the call has no such argument, or takes it: not a refusal
            continue
        rc = call.run(**changes)
        print(kind.name, what, rc, error())
        assert (rc, error()) == (_lib.ERR_INVALID, "%s: %s" % (kind.name, rule)), what
        assert [ctx.counter(c) for c in COUNTERS] == before and ctx.counter("map_inserts") == inserts, what
        assert call.out.untouched(), what
    # one good call over frames of three sizes (a render takes frames of one camera): host outputs are the device outputs, bit for bit
    good = kind(world, world["targets"] if kind is RenderFrames else world["mixed"])
    assert good.run() == _lib.OK, error()
    host = good.out.bytes()
    assert good.run(device=True) == _lib.OK, error()
    device = good.out.bytes()
    assert len(host) == len(device) and all(np.array_equal(h, g) for h, g in zip(host, device))
    assert not any(np.all(h == SENTINEL) for h in host)
    moved = [ctx.counter(c) - b for c, b in zip(COUNTERS, before)]
    n = 2 * good.items()
    want = {WarpInverse: [n, 0, 0, 0, 0], WarpForward: [n, 0, 0, 0, 0], Covisibility: [0, n, 0, 0, 0], Encode: [0, 0, n, 0, 0],
            Query: [0, 0, n, n, 0], RenderFrames: [0, 0, 0, 0, n]}.get(kind, [0] * 5)
    assert moved == want and ctx.counter("map_inserts") - inserts == (n if kind is Insert else 0)
