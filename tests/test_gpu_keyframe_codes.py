"""Keyframes retrieved by appearance on the device (include/dvo_hip.h, dvo_hip_codebook_*; dvo_slam_amd/csrc/keyframe_codes.hip).

The yardstick is the host build of keyframe_codes.h (tests/test_keyframe_codes.py: encode_host, topk_host, HostCodebook) fed the planes
the device holds at the level (planes_of): codes, distances and result rows are integers and must be EQUAL, whatever order anything ran in.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import dvo_slam_amd as d
import test_keyframe_codes as tkc
from dvo_slam_amd import _lib
from oracle import pyoracle as po
from test_gpu_cloud_map import planes_of
from test_gpu_f32_ingest import blank_frames, camera
from test_gpu_frame_warp import frames_of
from test_keyframe_codes import MASKED, NONE, HostCodebook, crafted_book, encode_host, np_topk, random_codes, topk_host

pytestmark = pytest.mark.gpu
u32p = C.POINTER(C.c_uint32)


class DevicePlanes(HostCodebook):
    """the host build over the planes the device holds, downloaded once per (pyramid, level)"""
    seen = {}

    @staticmethod
    def planes(pyramid, level):
        key = (id(pyramid), level)
        if key not in DevicePlanes.seen:
            DevicePlanes.seen[key] = (pyramid, planes_of(pyramid, level))       # (the pyramid is kept: its id is not given again)
        return DevicePlanes.seen[key][1]


def host(a):
    """a device or host output as a numpy array of the same bits"""
    if not hasattr(a, "data_ptr"):
        return a
    torch.cuda.synchronize()
    return a.cpu().numpy()


def as_rows(a):
    a = host(a)
    return a if a.dtype == d.CODE_MATCH_DTYPE else np.ascontiguousarray(a).view(np.uint32).view(d.CODE_MATCH_DTYPE).reshape(a.shape[0], -1)


def as_u(a, dtype):
    return np.ascontiguousarray(host(a)).view(dtype)


# ---- 1. encoding ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [128, 384, 2048])
def test_codes_equal_the_host_build(m):
    """64 x 48 and 128 x 96 at levels 0, 2 and the coarsest (3): level 2 of 64 x 48 is 16 x 12, narrower than a wavefront, level 3 is 8 x 6;
    two cameras in one call; host and device outputs; encoding into a book equals dvo_hip_frames_encode"""
    ctx, large, _ = frames_of(128, 96, 3, levels=4)
    _, small, _ = frames_of(64, 48, 2, levels=4)
    pyramids = [large[0], small[0], large[1], small[1], large[2]]
    book = d.KeyframeCodebook(ctx, m=m, capacity=16, seed=m)
    want_book = DevicePlanes(m=m, capacity=16, seed=m)
    assert book.ferns().tobytes() == want_book.ferns().tobytes() == tkc.fern_table(m, m).tobytes()
    c0 = ctx.counter("codebook_encoded")
    for level in (0, 2, 3):
        want = want_book.encode(pyramids, level)
        for device in (False, True):
            got = as_u(book.encode(pyramids, level, device=device), np.uint32)
            assert got.shape == (5, m // 8) and np.array_equal(got, want), (m, level, device)
        assert len(set(x.tobytes() for x in want)) == 5                                    # not a comparison of equal codes
        nib = tkc.np_unpack(want)
        assert all(0 < ((nib & bit) != 0).sum() < nib.size for bit in (1, 2, 4, 8))         # every bit is set somewhere and clear somewhere
    assert ctx.counter("codebook_encoded") == c0 + 30 and book.size == 0                   # (encode leaves the book unchanged)
    assert book.add(pyramids[:3], 2).tolist() == [0, 1, 2] and book.add(pyramids[3:], 3).tolist() == [3, 4]
    want = np.concatenate([want_book.encode(pyramids[:3], 2), want_book.encode(pyramids[3:], 3)])
    assert np.array_equal(book.codes(), want) and np.array_equal(as_u(book.codes(1, 3, device=True), np.uint32), want[1:4])
    assert book.info() == dict(m=m, capacity=16, size=5, live=5) and ctx.counter("codebook_encoded") == c0 + 35
    book.close()


def test_codes_of_frames_that_hold_plane_c_and_of_frames_that_hold_the_taps():
    """a current-role ingest of 32 frames leaves plane C alone where level 0 has one (96 x 64: {I, Z} 8 bytes apart), frames created
    from float planes hold the taps A (16 bytes apart); both in one call, before anything downloads (and so derives) other planes"""
    w, h, levels = 96, 64, 3
    b = d.datagen.synth_batch(811, 3, w, h)
    ctx = d.default_context()
    cam = camera(ctx, w, h, b["K"], levels)
    cfg = d.Config(FirstLevel=levels - 1, LastLevel=0)
    crowd = blank_frames(cam, 32)
    dummy = np.zeros((h, w), np.uint8), np.full((h, w), 5000, np.uint16)
    d.update_raw_host_batch(crowd, [b["grey_ref"][0], b["grey_cur"][0]] + [dummy[0]] * 30, [b["depth_ref"][0], b["depth_cur"][0]] + [dummy[1]] * 30,
                            role="current", config=cfg)
    d.upload_wait(ctx)
    taps = [cam.create(b["grey_ref"][k].astype(np.float32), po.convert_raw_depth(b["depth_ref"][k])) for k in (1, 2)]
    pyramids = [crowd[0], taps[0], crowd[1], taps[1]]
    book = d.KeyframeCodebook(ctx, m=256, capacity=8, seed=9)
    got = {level: book.encode(pyramids, level) for level in (0, 1, 2)}
    want_book = DevicePlanes(m=256, capacity=8, seed=9)
    for level in (0, 1, 2):
        assert np.array_equal(got[level], want_book.encode(pyramids, level)), level
        assert np.array_equal(book.encode(pyramids, level), got[level])                    # ... and again, whatever the frames hold by now
    book.close()


# ---- 2. search against crafted codes -----------------------------------------------------------------------------------------------------------

def crafted(n, m, seed):
    rng = np.random.default_rng(seed)
    base, codes = crafted_book(rng, n, m)
    if n >= 63:
        codes[57] ^= np.uint32(0x0F0F0F0F)                                                 # half the ferns away from every other code
        codes[40] = codes[11] = codes[57]                                                  # one code three times: ids 11, 40, 57 in that order
    dead = np.array([i for i in rng.permutation(n) if i not in (11, 40, 57)][:n // 6], dtype=np.int64)   # (the three equal codes stay alive)
    live = np.ones(n, np.uint8)
    live[dead] = 0
    queries = np.concatenate([base[None], codes[[n // 2, 57 % n, n - 1]], crafted_book(rng, 13, m, base)[1]])   # 17: more than one LDS tile
    return codes, live, np.sort(dead), queries


@pytest.mark.parametrize("n,m", [(1, 512), (63, 128), (65, 512), (257, 384), (1030, 512), (300, 2048)])
def test_rows_and_distances_equal_the_host_build(n, m):
    """book sizes around a wavefront's entries (63, 65), a workgroup's (257) and many workgroups' (1030: 65 of them at m = 512, still one
    step of the grid -- the walk of k_code_search and ids past 4096 are test_books_past_the_search_grid_and_past_4096_ids's); 1, 3 and 17
    queries; k of 1, 5, 64 and beyond the live count; removed entries and skipped intervals; the same call twice"""
    ctx = d.default_context()
    codes, live, dead, queries = crafted(n, m, n + m)
    book = d.KeyframeCodebook(ctx, m=m, capacity=n + 3, seed=1)
    assert book.add_codes(codes).tolist() == list(range(n))
    c0 = ctx.counter("codebook_queries")
    asked = 0
    for removed in (False, True):
        if removed and len(dead):
            book.remove(dead)
        lv = live if removed else np.ones(n, np.uint8)
        for nq in (1, 3, 17):
            skip = np.stack([np.arange(nq) * 7 % (n + 1), np.arange(nq) * 7 % (n + 1) + np.arange(nq) % 5 * 3], 1)
            skip[nq - 1] = (0, n)                                                          # the last query: everything skipped
            for k in (1, 5, 64):
                for sk in (None, skip):
                    want_rows, want_D = topk_host(codes, lv, queries[:nq], k, sk)
                    for device in (False, True):
                        rows, D = book.query_codes(queries[:nq], k=k, skip=sk, distances=True, device=device)
                        rows, D = as_rows(rows), as_u(D, np.uint16)
                        assert np.array_equal(D, want_D), (n, m, nq, k, sk is not None, device)
                        assert np.array_equal(rows, want_rows), (n, m, nq, k, sk is not None, device, rows, want_rows)
                        asked += nq
                    again = book.query_codes(queries[:nq], k=k, skip=sk)
                    assert again.tobytes() == rows.tobytes()                                   # ... without the matrix, and twice the same bytes
                    asked += nq
    assert ctx.counter("codebook_queries") == c0 + asked
    # the yardstick itself against the numpy sort at this size, what the padding looks like, and who may never be named
    rows, D = topk_host(codes, live, queries, 64, None)
    want = np_topk(codes, live, queries, 64, None)
    assert np.array_equal(rows, want[0]) and np.array_equal(D, want[1])
    assert np.all(D[:, live == 0] == MASKED) and not np.isin(rows["id"], dead).any()
    if int(live.sum()) < 64:
        assert np.all(rows["id"][:, int(live.sum()):] == NONE) and np.all(rows["distance"][:, int(live.sum()):] == NONE)
    if n >= 63:
        full = book.query_codes(codes[57:58], k=64)[0]
        fresh = d.KeyframeCodebook(ctx, m=m, capacity=n, seed=1)
        fresh.add_codes(codes)
        trio = fresh.query_codes(codes[57:58], k=5)[0]
        assert trio["id"][:3].tolist() == [11, 40, 57] and trio["distance"][:3].tolist() == [0, 0, 0]
        assert full["id"][:3].tolist() == [11, 40, 57]
        fresh.close()
    book.close()


NEAR_IDS = (0, 4094, 4095, 4096, 4097, 8190, 8191, 8192, 8193, 65534, 65535, 65536, 65537, 262142, 262143, 262144, 262145)
SEARCH_GRID_ENTRIES = {128: 4096 * 64, 512: 4096 * 16}      # keyframe_codes.hip: kSearchMaxBlocks workgroups of 256 / LPE entries


def boundary_book(n, m, seed):
    """n random codes -- about 15 ferns of 16 away from anything -- of which those at NEAR_IDS (and the last two) lie 2 or 3 ferns from a
    base code: ties in distance on both sides of every 4096-id boundary, some of them dead"""
    rng = np.random.default_rng(seed)
    codes, base = random_codes(rng, n, m), random_codes(rng, 1, m)[0]
    near = sorted(set(i for i in NEAR_IDS + (n - 2, n - 1) if 0 <= i < n))
    for j, i in enumerate(near):
        nib = tkc.np_unpack(base).copy()
        at = rng.permutation(m)[:2 + (j % 3 == 2)]
        nib[at] ^= rng.integers(1, 16, len(at)).astype(np.uint32)
        codes[i] = tkc.np_pack(nib)
    live = (rng.uniform(size=n) > 0.125).astype(np.uint8)
    live[near] = 1
    live[[i for i in (4095, 8192, 65536, 262143) if i < n]] = 0
    return codes, base, near, live


@pytest.mark.parametrize("n,m", [(5000, 128), (70000, 512), (4096 * 64 + 70, 128)])
def test_books_past_the_search_grid_and_past_4096_ids(n, m):
    """70 000 entries at m = 512 and 262 214 at m = 128 are more than one step of k_code_search's grid (65 536 and 262 144 entries): the
    kernel walks.  Every book here has ids past 4096, so the k-th key of k_code_topk has a high id digit other than 0 and the last radix
    pass runs over a window of the row that does not start at 0; the nearest entries tie in distance across the 4096-id boundaries, with
    dead and skipped entries on both sides, and the queries that are far from everything tie among thousands of entries anywhere."""
    ctx = d.default_context()
    codes, base, near, live = boundary_book(n, m, n + m)
    assert (n > SEARCH_GRID_ENTRIES[m]) == (n >= 70000)
    book = d.KeyframeCodebook(ctx, m=m, capacity=n, seed=1)
    book.add_codes(codes)
    book.remove(np.nonzero(live == 0)[0])
    rng = np.random.default_rng(n)
    queries = np.stack([base, codes[near[3]], random_codes(rng, 1, m)[0], base, base, random_codes(rng, 1, m)[0]])
    skip = np.array([(0, 0), (0, 1), (0, 0), (4090, 4097), (4097, min(8192, n)), (4000, 4200)])
    high_digit = set()
    for k in (1, 3, 6, 64):
        for sk in (None, skip):
            want_rows, want_D = topk_host(codes, live, queries, k, sk)
            rows, D = book.query_codes(queries, k=k, skip=sk, distances=True)
            assert np.array_equal(D, want_D), (n, m, k, sk is not None)
            assert np.array_equal(rows, want_rows), (n, m, k, sk is not None, rows, want_rows)
            high_digit |= set((want_rows["id"][:, -1][want_rows["id"][:, -1] != NONE] >> 12).tolist())
    rows, D = book.query_codes(queries, k=64, skip=skip, distances=True, device=True)
    assert np.array_equal(as_rows(rows), want_rows) and np.array_equal(as_u(D, np.uint16), want_D)
    # what the cases are there for: k-th keys whose ids lie in several 4096-id windows of the row, the first one among them
    assert 0 in high_digit and len(high_digit) >= min(3, ((n - 1) >> 12) + 1), high_digit
    first = topk_host(codes, live, queries[:1], 6)[0][0]
    assert first["distance"].tolist() == sorted(first["distance"].tolist()) and first["distance"][0] == 2 and first["distance"][5] <= 3
    assert first["id"][0] == 0 and first["id"][2] >= 4096 and not np.isin(first["id"], [4095, 8192]).any()
    book.close()


def test_queries_answered_in_rounds_equal_one_round():
    """option "codebook_round_kb": with 64 KB of staging a row of 5000 entries (10 KB) leaves 6 queries to a round, with 256 KB 26, cut to
    the 16 of a whole tile; 40 queries then take 7 and 3 rounds, the last one short.  Rows, host distances and device rows are those of
    the yardstick: the queries, the skipped intervals, the rows and the matrix are all taken at the round's first query."""
    ctx = d.default_context()
    n, m, nq = 5000, 128, 40
    codes, base, near, live = boundary_book(n, m, 77)
    rng = np.random.default_rng(78)
    queries = np.concatenate([crafted_book(rng, nq // 2, m, base)[1], random_codes(rng, nq - nq // 2, m)])
    skip = np.stack([np.arange(nq) * 131 % n, np.arange(nq) * 131 % n + np.arange(nq) * 37], 1)
    book = d.KeyframeCodebook(ctx, m=m, capacity=n, seed=1)
    book.add_codes(codes)
    book.remove(np.nonzero(live == 0)[0])
    want_rows, want_D = topk_host(codes, live, queries, 5, skip)
    assert len(set(r.tobytes() for r in want_rows)) > nq // 2                                # (a row in the wrong place would show)
    try:
        for kb in (64, 256):
            ctx.set_option("codebook_round_kb", kb)
            rows, D = book.query_codes(queries, k=5, skip=skip, distances=True)
            assert np.array_equal(rows, want_rows) and np.array_equal(D, want_D), kb
            assert np.array_equal(as_rows(book.query_codes(queries, k=5, skip=skip, device=True)), want_rows), kb
            assert np.array_equal(book.query_ids(np.arange(nq) * 3, k=5, skip=skip), topk_host(codes, live, codes[np.arange(nq) * 3], 5, skip)[0]), kb
        ctx.set_option("codebook_round_kb", 1)                                               # less than a row: a query to a round
        assert np.array_equal(book.query_codes(queries[:3], k=5, skip=skip[:3]), want_rows[:3])
        with pytest.raises(d.DvoHipError):
            ctx.set_option("codebook_round_kb", 0)
    finally:
        ctx.set_option("codebook_round_kb", 256 * 1024)
    assert np.array_equal(book.query_codes(queries, k=5, skip=skip), want_rows)
    book.close()


def test_query_ids_equals_query_codes_of_the_codes_read_back():
    ctx = d.default_context()
    n, m = 130, 256
    codes, live, dead, _ = crafted(n, m, 5)
    book = d.KeyframeCodebook(ctx, m=m, capacity=n, seed=1)
    book.add_codes(torch.from_numpy(codes.view(np.int32)).cuda())                          # raw codes from device memory
    assert np.array_equal(book.codes(), codes)
    book.remove(dead)
    ids = np.array([0, 57, int(dead[0]), n - 1, 11, 11])                                    # a dead entry may ask; an id may ask twice
    skip = np.stack([ids, ids + 1], 1)
    for sk in (None, skip):
        rows, D = book.query_ids(ids, k=6, skip=sk, distances=True)
        want = book.query_codes(book.codes()[ids], k=6, skip=sk, distances=True)
        assert np.array_equal(rows, want[0]) and np.array_equal(D, want[1])
        assert np.array_equal(rows, topk_host(codes, live, codes[ids], 6, sk)[0])
    assert all(r["id"][0] != i for r, i in zip(rows, ids)) and rows[1]["id"][:2].tolist() == [11, 40]
    M = book.distance_matrix()
    assert M.shape == (n, n) and np.array_equal(M, topk_host(codes, live, codes, 1)[1])
    assert np.array_equal(as_u(book.distance_matrix(device=True), np.uint16), M)
    got = d.loop_closure_candidates_by_appearance(book, [57, 20], 2, k=4, max_distance=30)
    want_book = HostCodebook(m=m, capacity=n, seed=1)
    want_book.add_codes(codes)
    want_book.remove(dead)
    assert got == d.loop_closure_candidates_by_appearance(want_book, [57, 20], 2, k=4, max_distance=30) and got[0][:2] == [(11, 0), (40, 0)]
    # save and load, and growth: the same ids, the same answers, the dead stay dead
    with tempfile.TemporaryDirectory() as tmp:
        book.save(os.path.join(tmp, "book.npz"))
        back = d.KeyframeCodebook.load(os.path.join(tmp, "book.npz"), ctx)
    big = book.grown()
    for other in (back, big):
        assert other.info()["size"] == n and other.live == book.live and np.array_equal(other.codes(), codes)
        assert np.array_equal(other.query_ids(ids, k=6), book.query_ids(ids, k=6))
        other.close()
    book.clear()
    assert book.info() == dict(m=m, capacity=n, size=0, live=0) and np.all(book.query_codes(codes[:2], k=3)["id"] == NONE)
    assert book.add_codes(codes[:2]).tolist() == [0, 1]
    book.close()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_touch_nothing_and_a_full_book_is_a_capacity_error():
    ctx, pyramids, _ = frames_of(64, 48, 3)
    L = ctx._lib
    other = d.Context(0)
    foreign_frame = camera(other, 64, 48, planes_of(pyramids[0], 0)[2], 3).create(*planes_of(pyramids[0], 0)[:2])
    shallow = camera(ctx, 64, 48, planes_of(pyramids[0], 0)[2], 1).create(*planes_of(pyramids[0], 0)[:2])
    foreign_book = d.KeyframeCodebook(other, m=128, capacity=4)
    m, words = 128, 16
    book = d.KeyframeCodebook(ctx, m=m, capacity=4, seed=3)
    book.add(pyramids, 1)
    before = book.codes().copy()
    handles = lambda *p: (C.c_void_p * len(p))(*[x if x is None else x.ptr for x in p])      # noqa: E731
    fr = handles(*pyramids)
    rows = np.full((3, 2), 7, d.CODE_MATCH_DTYPE)
    dist = np.full((3, 3), 7, np.uint16)
    codes = np.full((3, words), 7, np.uint32)
    ids = np.arange(3, dtype=np.uint32)
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    vp = lambda a: C.c_void_p(a if isinstance(a, int) else a.ctypes.data)                     # noqa: E731
    idp = lambda a: a.ctypes.data_as(u32p)                                                    # noqa: E731
    out = C.c_void_p()

    def create(m_=128, capacity=4, ctx_=ctx.ptr, z=(0.5, 5.0), o=C.byref(out)):
        return L.dvo_hip_codebook_create(ctx_, m_, capacity, 0, None, z[0], z[1], o)

    def qf(ctx_=ctx.ptr, b=book.ptr, n=3, f=fr, level=1, k=2, lo=None, hi=None, r=vp(rows), dd=vp(dist), on=0):
        return L.dvo_hip_codebook_query_frames(ctx_, b, n, f, level, k, lo, hi, r, dd, on)

    def qc(b=book.ptr, n=3, c=vp(codes), c_on=0, k=2, r=vp(rows), dd=vp(dist), on=0):
        return L.dvo_hip_codebook_query_codes(ctx.ptr, b, n, c, c_on, k, None, None, r, dd, on)

    def qi(b=book.ptr, n=3, i=idp(ids), k=2):
        return L.dvo_hip_codebook_query_ids(ctx.ptr, b, n, i, k, None, None, vp(rows), vp(dist), 0)

    def enc(b=book.ptr, n=3, f=fr, level=1, o=vp(codes), on=0):
        return L.dvo_hip_frames_encode(ctx.ptr, b, n, f, level, o, on)

    beyond, lone = np.array([0, 3], np.uint32), np.array([5], np.uint32)
    base = dev.data_ptr()
    c1 = [ctx.counter("codebook_encoded"), ctx.counter("codebook_queries")]
    refused = [
        lambda: create(m_=200), lambda: create(m_=0), lambda: create(m_=2176), lambda: create(capacity=0), lambda: create(capacity=(1 << 24) + 1),
        lambda: create(ctx_=None), lambda: create(o=None), lambda: create(z=(2.0, 1.0)), lambda: create(z=(float("nan"), 1.0)),
        # a null or foreign handle
        lambda: qf(b=None), lambda: qf(b=foreign_book.ptr), lambda: qf(ctx_=other.ptr), lambda: qc(b=None), lambda: qi(b=foreign_book.ptr),
        lambda: enc(b=None), lambda: enc(b=foreign_book.ptr), lambda: L.dvo_hip_codebook_clear(ctx.ptr, foreign_book.ptr),
        lambda: L.dvo_hip_codebook_info(ctx.ptr, None, None, None, None, None), lambda: L.dvo_hip_codebook_ferns(ctx.ptr, book.ptr, None),
        lambda: L.dvo_hip_codebook_remove(ctx.ptr, foreign_book.ptr, 1, idp(ids)), lambda: L.dvo_hip_codebook_add_codes(ctx.ptr, None, 1, vp(codes), 0, None),
        lambda: L.dvo_hip_codebook_add_frames(ctx.ptr, foreign_book.ptr, 1, fr, 1, None),
        lambda: L.dvo_hip_codebook_read_codes(ctx.ptr, foreign_book.ptr, 0, 1, vp(codes), 0),
        # k, the queries, the frames and the level
        lambda: qf(k=0), lambda: qf(k=65), lambda: qc(k=0), lambda: qi(k=65), lambda: qf(n=0), lambda: qc(n=-1), lambda: qc(n=4097), lambda: qf(r=None),
        lambda: qf(f=None), lambda: qf(f=handles(pyramids[0], None, pyramids[2])), lambda: qf(f=handles(pyramids[0], foreign_frame, pyramids[2])),
        lambda: qf(level=3), lambda: qf(level=-1), lambda: qf(f=handles(pyramids[0], shallow, pyramids[2])), lambda: enc(level=3), lambda: enc(n=0),
        lambda: enc(f=handles(foreign_frame, pyramids[1], pyramids[2])), lambda: enc(o=None), lambda: qc(c=None),
        lambda: qf(lo=idp(ids)), lambda: qf(hi=idp(ids)),                                     # one bound of the skipped interval without the other
        lambda: L.dvo_hip_codebook_add_frames(ctx.ptr, book.ptr, 1, handles(shallow), 1, None),
        # an id beyond the size
        lambda: qi(n=2, i=idp(beyond)), lambda: qi(n=1, i=idp(lone)), lambda: L.dvo_hip_codebook_remove(ctx.ptr, book.ptr, 2, idp(beyond)),
        lambda: L.dvo_hip_codebook_remove(ctx.ptr, book.ptr, 0, idp(ids)), lambda: L.dvo_hip_codebook_read_codes(ctx.ptr, book.ptr, 2, 2, vp(codes), 0),
        lambda: L.dvo_hip_codebook_read_codes(ctx.ptr, book.ptr, -1, 1, vp(codes), 0), lambda: L.dvo_hip_codebook_read_codes(ctx.ptr, book.ptr, 0, 0, vp(codes), 0),
        # a misaligned device buffer
        lambda: qf(r=vp(base + 4), dd=None, on=1), lambda: qf(r=vp(base), dd=vp(base + 1025), on=1), lambda: qc(c=vp(base + 2), c_on=1),
        lambda: enc(o=vp(base + 2), on=1), lambda: L.dvo_hip_codebook_add_codes(ctx.ptr, book.ptr, 1, vp(base + 1), 1, None),
        lambda: L.dvo_hip_codebook_read_codes(ctx.ptr, book.ptr, 0, 1, vp(base + 3), 1),
    ]
    for i, call in enumerate(refused):
        assert call() == _lib.ERR_INVALID, i
    assert out.value is None
    # a full book: one entry fits, two do not
    two = handles(pyramids[0], pyramids[1])
    assert L.dvo_hip_codebook_add_frames(ctx.ptr, book.ptr, 2, two, 1, None) == _lib.ERR_CAPACITY
    assert L.dvo_hip_codebook_add_codes(ctx.ptr, book.ptr, 2, vp(codes), 0, None) == _lib.ERR_CAPACITY
    with pytest.raises(d.DvoHipError):
        book.add(pyramids[:2], 1)
    # nothing was touched
    assert [ctx.counter("codebook_encoded"), ctx.counter("codebook_queries")] == c1
    assert book.info() == dict(m=m, capacity=4, size=3, live=3) and np.array_equal(book.codes(), before)
    assert np.all(rows["id"] == 7) and np.all(rows["distance"] == 7) and np.all(dist == 7) and np.all(codes == 7) and not dev.cpu().numpy().any()
    # the same calls with nothing wrong
    want_book = DevicePlanes(m=m, capacity=4, seed=3)
    want_book.add(pyramids, 1)
    assert np.array_equal(before, want_book.codes())
    assert qf() == 0 and np.array_equal(rows, want_book.query(pyramids, 1, k=2)) and rows["id"][:, 0].tolist() == [0, 1, 2]
    assert np.array_equal(dist, want_book.query(pyramids, 1, k=2, distances=True)[1])
    assert enc() == 0 and np.array_equal(codes, before) and qc() == 0 and qi() == 0
    assert [ctx.counter("codebook_encoded"), ctx.counter("codebook_queries")] == [c1[0] + 6, c1[1] + 9]
    assert L.dvo_hip_codebook_add_frames(ctx.ptr, book.ptr, 1, two, 1, None) == 0 and book.info()["size"] == 4
    del foreign_frame
    foreign_book.close()
    other.close()
    book.close()


# ---- 4. retrieval -------------------------------------------------------------------------------------------------------------------------

def test_retrieval_condition_on_the_device():
    """the condition of tests/test_keyframe_codes.py on the device: frame 0 of 16 synthetic scenes in the book at level 2 (40 x 30), m = 256;
    frame 1 of every scene finds its own scene first with a margin of at least 8 ferns -- and the rows equal the host build's"""
    R = tkc.RETRIEVAL
    ctx = d.default_context()
    seqs = tkc.retrieval_sequences()
    cam = camera(ctx, R["w"], R["h"], seqs[0][2], R["level"] + 1)
    stored = [cam.create_raw(g[0], z[0]) for g, z, K in seqs]
    queries = [cam.create_raw(g[1], z[1]) for g, z, K in seqs]
    book = d.KeyframeCodebook(ctx, m=R["m"], capacity=17, seed=R["seed"])
    rows, own, other = tkc.retrieval_margins(book, stored, queries, R["level"])
    print("own scene at most %d, nearest other scene at least %d, worst margin %d" % (own.max(), other.min(), (other - own).min()))
    assert rows["id"][:, 0].tolist() == list(range(16)) and (other - own).min() >= R["margin"], (own.tolist(), other.tolist())
    want_book = DevicePlanes(m=R["m"], capacity=16, seed=R["seed"])
    want = tkc.retrieval_margins(want_book, stored, queries, R["level"])
    assert np.array_equal(rows, want[0]) and np.array_equal(own, want[1]) and np.array_equal(other, want[2])
    assert d.relocalisation_candidates(book, queries[3:5], R["level"], k=2) == d.relocalisation_candidates(want_book, queries[3:5], R["level"], k=2)
    far = planes_of(queries[0], R["level"])
    assert book.harvest(queries[0], R["level"], int(own[0])) == 16 and book.harvest(queries[0], R["level"], 1) is None and far[0].shape == (30, 40)
    book.close()


# ---- 5. the C++ facade ----------------------------------------------------------------------------------------------------------------------

def facade_frame(k, changed=False, w=64, h=48):
    """keyframe k of tests/cpp/appearance_facade_check.cpp: integer-valued formulas, exact in float32 on both sides"""
    y, x = np.mgrid[0:h, 0:w]
    I = ((x * (7 + 2 * k) + y * (13 + 4 * k) + k * 37) % 256).astype(np.float32)
    Z = (1000 + (x * (3 + k) + y * 5 + k * 111) % 4096).astype(np.float32) * np.float32(0.001)
    Z[(x // 2 + 2 * (y // 2) + k) % 29 == 0] = np.nan
    if changed:
        flip = (x // 4 + y // 4) % 5 == 0
        I[flip] = np.float32(255.0) - I[flip]
    return I, Z


def test_cpp_facade_search_equals_the_python_wrappers():
    exe = tkc.build_appearance_facade_check()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "matches.bin")
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
        got = np.fromfile(path, d.CODE_MATCH_DTYPE)
    ctx = d.default_context()
    cam = camera(ctx, 64, 48, np.array([60.0, 60.0, 31.5, 23.5], np.float32), 3)
    book = d.KeyframeCodebook(ctx, m=256, capacity=8, seed=5)
    book.add([cam.create(*facade_frame(k)) for k in range(6)], 1)
    want = book.query([cam.create(*facade_frame(2, True))], 1, k=3)[0]
    assert np.array_equal(got, want) and want["id"][0] == 2
    line = [x for x in out.stdout.splitlines() if x.startswith("query:")][0]
    assert line.split()[1:] == ["%d:%d" % (r["id"], r["distance"]) for r in want]
    book.close()
