"""Keyframes retrieved by appearance, CPU tier (dvo_slam_amd/csrc/keyframe_codes.h; include/dvo_hip.h, dvo_hip_codebook_*).

keyframe_codes.h is compiled for the host (g++, -ffp-contract=off, every warning an error) the way tests/test_covisibility.py compiles
covisibility.h, and exposed as fern_table(), encode_host(), distance_host() and topk_host(): the yardsticks the device results are
compared with in tests/test_gpu_keyframe_codes.py.  Here they are held to an independent numpy statement of the header, and the Python
logic above the device calls (CodebookLogic: harvest, growth, save and load; relocalisation_candidates,
loop_closure_candidates_by_appearance) runs with the host build in the device call's place (HostCodebook).
"""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
from dvo_slam_amd import _lib, datagen
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")
f32 = np.float32
NONE, MASKED = d.CODE_NONE, d.CODE_MASKED

HOST_SOURCE = r"""
#include "keyframe_codes.h"
using namespace dvo_hip;
extern "C" {
void codes_fern_table(unsigned long long seed, int m, float z_lo, float z_hi, dvo_hip_fern* out) { fern_table(seed, m, z_lo, z_hi, out); }
void codes_encode(const float* I, const float* Z, int w, int h, const dvo_hip_fern* ferns, int m, uint32_t* out) {
  encode_frame_host(I, Z, w, h, ferns, m, out);
}
unsigned codes_distance(const uint32_t* a, const uint32_t* b, int words) { return code_distance(a, b, words); }
void codes_topk(const uint32_t* codes, const unsigned char* live, int n, int m, const uint32_t* queries, int n_queries, const uint32_t* skip_from,
                const uint32_t* skip_to, int k, dvo_hip_code_match* rows, uint16_t* distances) {
  codes_topk_host(codes, live, n, m, queries, n_queries, skip_from, skip_to, k, rows, distances);
}
int codes_lanes_per_entry(int m) { return code_lanes_per_entry(m); }
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    """keyframe_codes.h compiled for the host: g++, every warning an error, no contraction"""
    tmp = tempfile.mkdtemp(prefix="keyframe_codes_host_")
    src, out = os.path.join(tmp, "keyframe_codes_host.cpp"), os.path.join(tmp, "keyframe_codes_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.codes_fern_table.argtypes = [C.c_uint64, C.c_int, C.c_float, C.c_float, vp]
    L.codes_fern_table.restype = None
    L.codes_encode.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.codes_encode.restype = None
    L.codes_distance.argtypes = [vp, vp, C.c_int]
    L.codes_distance.restype = C.c_uint
    L.codes_topk.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.codes_topk.restype = None
    return L


def fern_table(seed, m, z_lo=0.5, z_hi=5.0):
    out = np.zeros(m, d.FERN_DTYPE)
    host_lib().codes_fern_table(seed, m, z_lo, z_hi, out.ctypes.data)
    return out


def encode_host(I, Z, ferns):
    """the code of tight planes I, Z under the ferns: [m / 8] uint32"""
    I, Z = np.ascontiguousarray(I, f32), np.ascontiguousarray(Z, f32)
    assert I.shape == Z.shape and I.ndim == 2
    out = np.zeros(len(ferns) // 8, np.uint32)
    host_lib().codes_encode(I.ctypes.data, Z.ctypes.data, I.shape[1], I.shape[0], np.ascontiguousarray(ferns).ctypes.data, len(ferns), out.ctypes.data)
    return out


def distance_host(a, b):
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    return int(host_lib().codes_distance(a.ctypes.data, b.ctypes.data, a.size))


def topk_host(codes, live, queries, k, skip=None):
    """(rows [Q, k] CODE_MATCH_DTYPE, distances [Q, n] uint16) of codes_topk_host"""
    codes = np.ascontiguousarray(codes, np.uint32).reshape(len(live), -1) if len(live) else np.zeros((0, np.shape(queries)[1]), np.uint32)
    queries = np.ascontiguousarray(queries, np.uint32)
    live = np.ascontiguousarray(live, np.uint8)
    Q, words = queries.shape
    rows, D = np.zeros((Q, k), d.CODE_MATCH_DTYPE), np.zeros((Q, len(live)), np.uint16)
    lo = hi = None
    if skip is not None:
        lo, hi = np.ascontiguousarray(np.asarray(skip)[:, 0], np.uint32), np.ascontiguousarray(np.asarray(skip)[:, 1], np.uint32)
    host_lib().codes_topk(codes.ctypes.data, live.ctypes.data, len(live), words * 8, queries.ctypes.data, Q, None if lo is None else lo.ctypes.data,
                          None if hi is None else hi.ctypes.data, k, rows.ctypes.data, D.ctypes.data)
    return rows, D


# ---- the independent numpy statement -----------------------------------------------------------------------------------------------------

M64 = (1 << 64) - 1


def np_fern_table(seed, m, z_lo=0.5, z_hi=5.0):
    out = np.zeros(m, d.FERN_DTYPE)
    state = seed
    def draw():
        nonlocal state
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    for i in range(m):
        p, t = draw(), draw()
        out[i]["u"], out[i]["v"], out[i]["u2"], out[i]["v2"] = p & 0xFFFF, (p >> 16) & 0xFFFF, (p >> 32) & 0xFFFF, (p >> 48) & 0xFFFF
        out[i]["t_i"] = f32(32 + (t & 0xFFFFFFFF) % 192)
        out[i]["t_z"] = f32(z_lo) + f32(f32(f32(z_hi) - f32(z_lo)) * f32((t >> 32) & 0xFFFF)) / f32(65536)
    return out


def np_nibbles(I, Z, ferns):
    """the m nibbles of planes I, Z, whole table at a time"""
    h, w = I.shape
    x, y = (ferns["u"].astype(np.int64) * w) >> 16, (ferns["v"].astype(np.int64) * h) >> 16
    x2, y2 = (ferns["u2"].astype(np.int64) * w) >> 16, (ferns["v2"].astype(np.int64) * h) >> 16
    a, b, z = I[y, x], I[y2, x2], Z[y, x]
    with np.errstate(invalid="ignore"):
        known = np.isfinite(z)
        return ((a > ferns["t_i"]) * 1 + (a > b) * 2 + (known & (z > ferns["t_z"])) * 4 + known * 8).astype(np.uint32)


def np_pack(nibbles):
    n = nibbles.reshape(-1, 8).astype(np.uint32)
    return np.bitwise_or.reduce(n << (4 * np.arange(8, dtype=np.uint32)), axis=1).astype(np.uint32)


def np_unpack(code):
    return ((np.asarray(code, np.uint32)[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).reshape(*np.shape(code)[:-1], -1)


def np_distances(queries, codes):
    """[Q, n] ferns whose nibbles differ"""
    return (np_unpack(queries)[:, None, :] != np_unpack(codes)[None, :, :]).sum(-1)


def np_topk(codes, live, queries, k, skip=None):
    Dm = np_distances(queries, codes) if len(codes) else np.zeros((len(queries), 0), np.int64)
    rows, D = np.zeros((len(queries), k), d.CODE_MATCH_DTYPE), np.zeros(Dm.shape, np.uint16)
    for q in range(len(queries)):
        ids = np.arange(len(codes))
        out = ~np.asarray(live, bool)
        if skip is not None:
            out |= (ids >= skip[q][0]) & (ids < skip[q][1])
        D[q] = np.where(out, MASKED, Dm[q])
        ranked = sorted((int(Dm[q, i]), int(i)) for i in ids[~out])[:k]
        ranked += [(NONE, NONE)] * (k - len(ranked))
        rows[q]["distance"], rows[q]["id"] = [r[0] for r in ranked], [r[1] for r in ranked]
    return rows, D


def random_planes(rng, w, h, holes=0.2):
    I = rng.uniform(0, 255, (h, w)).astype(f32)
    Z = rng.uniform(0.3, 6.0, (h, w)).astype(f32)
    Z[rng.uniform(size=(h, w)) < holes] = np.nan
    Z[rng.uniform(size=(h, w)) < (0.02 if holes > 0 else 0.0)] = np.inf
    return I, Z


def random_codes(rng, n, m):
    return rng.integers(0, 1 << 32, (n, m // 8), dtype=np.uint64).astype(np.uint32)


# ---- 1. the fern table and the nibbles ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,m,z", [(0, 128, (0.5, 5.0)), (7, 384, (0.25, 3.5)), ((1 << 64) - 3, 2048, (1.0, 1.0))])
def test_fern_table_is_the_stated_generator(seed, m, z):
    got, want = fern_table(seed, m, *z), np_fern_table(seed, m, *z)
    assert got.tobytes() == want.tobytes()
    assert got["t_i"].min() >= 32 and got["t_i"].max() <= 223 and np.all(got["t_i"] == np.floor(got["t_i"]))
    assert got["t_z"].min() >= z[0] and got["t_z"].max() <= z[1]
    assert len(set(got["u"].tolist())) > m // 2 and (m < 2048 or got["u"].max() > 60000)


@pytest.mark.parametrize("shape", [(16, 12), (40, 30), (37, 23), (1, 1)])
def test_nibbles_equal_the_numpy_statement(shape):
    w, h = shape
    rng = np.random.default_rng(w * 100 + h)
    ferns = fern_table(3, 256)
    # ferns that land on the last row and column, on the first, and on one pixel twice (bit 1 compares a sample with itself: false)
    ferns[0]["u"], ferns[0]["v"], ferns[0]["u2"], ferns[0]["v2"] = 65535, 65535, 0, 0
    ferns[1]["u"], ferns[1]["v"], ferns[1]["u2"], ferns[1]["v2"] = 0, 65535, 65535, 0
    ferns[2]["u"], ferns[2]["v"], ferns[2]["u2"], ferns[2]["v2"] = 65535, 0, 65535, 0
    for holes in (0.0, 0.3, 1.0):
        I, Z = random_planes(rng, w, h, holes)
        want = np_nibbles(I, Z, ferns)
        got = encode_host(I, Z, ferns)
        assert np.array_equal(got, np_pack(want)) and np.array_equal(np_unpack(got), want)
        assert want[2] & 2 == 0
        if holes == 1.0:
            assert np.all(want & 12 == 0)
        if holes == 0.0 and w > 1:
            assert np.all(want & 8 == 8) and 0 < (want & 4 == 4).sum() < len(want) and 0 < (want & 1).sum() < len(want)
    # NaN intensity: every comparison with it is false
    I, Z = random_planes(rng, w, h)
    I[...] = np.nan
    assert np.all(np_unpack(encode_host(I, Z, ferns)) & 3 == 0)


def test_a_fern_reads_the_stated_pixel():
    """x = (u * w) >> 16: one bright pixel with depth switches exactly the ferns that land on it"""
    w, h = 40, 30
    ferns = fern_table(11, 128)
    x, y = (int(ferns[5]["u"]) * w) >> 16, (int(ferns[5]["v"]) * h) >> 16
    I, Z = np.zeros((h, w), f32), np.full((h, w), np.nan, f32)
    I[y, x], Z[y, x] = 255.0, 100.0
    got = np_unpack(encode_host(I, Z, ferns))
    on = ((ferns["u"].astype(np.int64) * w) >> 16 == x) & ((ferns["v"].astype(np.int64) * h) >> 16 == y)
    assert on[5] and np.array_equal(got & 13 == 13, on) and np.all(got[~on] & 13 == 0)


# ---- 2. the distance ---------------------------------------------------------------------------------------------------------------------

def test_distance_counts_ferns_not_bits():
    rng = np.random.default_rng(5)
    a = random_codes(rng, 1, 512)[0]
    assert distance_host(a, a) == 0
    b = a.copy()
    b[3] ^= np.uint32(0xF << 8)                       # all four bits of one nibble: 1, not 4
    assert distance_host(a, b) == 1
    for j in (1, 7, 64, 512):                          # one bit in each of j nibbles: j
        c = np_unpack(a).copy()
        at = rng.permutation(512)[:j]
        c[at] ^= (1 << rng.integers(0, 4, j)).astype(np.uint32)
        assert distance_host(a, np_pack(c)) == j
    assert distance_host(a, ~a) == 512
    for m in (128, 384, 2048):
        A, B = random_codes(rng, 4, m), random_codes(rng, 5, m)
        want = np_distances(A, B)
        assert [[distance_host(x, y) for y in B] for x in A] == want.tolist() and want.max() <= m


def test_lanes_per_entry_divide_the_code():
    for m in range(128, 2049, 128):
        lpe = host_lib().codes_lanes_per_entry(m)
        assert lpe in (4, 8, 16) and (m // 32) % lpe == 0
    assert host_lib().codes_lanes_per_entry(512) == 16 and host_lib().codes_lanes_per_entry(384) == 4


# ---- 3. the answer to a query --------------------------------------------------------------------------------------------------------------

def crafted_book(rng, n, m, base=None):
    """n codes at small known distances from `base`: many ties"""
    base = random_codes(rng, 1, m)[0] if base is None else base
    nib = np.tile(np_unpack(base), (n, 1))
    for i in range(n):
        at = rng.permutation(m)[:rng.integers(0, 12)]
        nib[i, at] ^= rng.integers(1, 16, len(at)).astype(np.uint32)
    return base, np.stack([np_pack(x) for x in nib]) if n else np.zeros((0, m // 8), np.uint32)


@pytest.mark.parametrize("n,m,k", [(1, 128, 1), (40, 128, 5), (40, 384, 64), (257, 256, 7), (0, 128, 3)])
def test_topk_equals_a_numpy_sort(n, m, k):
    rng = np.random.default_rng(n + m + k)
    base, codes = crafted_book(rng, n, m)
    if n >= 40:
        codes[7] = codes[3] = codes[21]                # the same code three times: ids 3, 7, 21 in that order
    live = np.ones(n, np.uint8)
    live[rng.permutation(n)[:n // 5]] = 0
    queries = np.concatenate([base[None], codes[:2], random_codes(rng, 1, m)]) if n else base[None]
    skip = np.array([(0, 0), (0, 1), (1, n), (5, 3)][:len(queries)])
    for lv, sk in ((np.ones(n, np.uint8), None), (live, None), (live, skip)):
        got, want = topk_host(codes, lv, queries, k, sk), np_topk(codes, lv, queries, k, sk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, m, k, sk is not None)
    rows, D = topk_host(codes, live, queries, k, skip)
    if n >= 40:
        assert np.all(D[:, live == 0] == MASKED) and D[1, 0] == MASKED and np.all(D[2, 1:] == MASKED)
        named = rows["id"][rows["id"] != NONE]
        assert np.all(live[named] == 1)
        assert (rows[2]["id"] != NONE).sum() == (1 if live[0] else 0)              # everything but entry 0 skipped: padding
        assert np.all(np.diff(rows["distance"].astype(np.int64), axis=1) >= 0)
        full = topk_host(codes, np.ones(n, np.uint8), codes[21:22], 64)[0][0]
        trio = [int(i) for i, dd in zip(full["id"], full["distance"]) if dd == 0]
        assert trio == [3, 7, 21]
    if n == 0:
        assert np.all(rows["id"] == NONE) and np.all(rows["distance"] == NONE) and D.shape == (1, 0)


# ---- 4. the Python logic with the host build in the device call's place ------------------------------------------------------------------------

class HostPyramid:
    """planes per level, as a pyramid the logic can ask for its levels"""
    def __init__(self, planes):
        self.planes, self.levels, self.ctx = planes, len(planes), None


class HostCodebook(d.CodebookLogic):
    """CodebookLogic over the host build of keyframe_codes.h; `planes`: how the planes of (pyramid, level) are obtained"""
    planes = staticmethod(lambda pyramid, level: pyramid.planes[level])

    def _open(self, m, capacity, seed, ferns):
        self._ferns = fern_table(seed, m, *self.z_range) if ferns is None else ferns.copy()
        self._codes, self._live = np.zeros((0, m // 8), np.uint32), np.zeros(0, np.uint8)

    def info(self):
        return dict(m=self.m, capacity=self.capacity, size=len(self._live), live=int(self._live.sum()))

    def ferns(self):
        return self._ferns.copy()

    def encode(self, pyramids, level, device=False):
        return np.stack([encode_host(*self.planes(p, level)[:2], self._ferns) for p in pyramids])

    def _add_codes(self, codes):
        first = len(self._live)
        self._codes = np.concatenate([self._codes, codes])
        self._live = np.concatenate([self._live, np.ones(len(codes), np.uint8)])
        return np.arange(first, len(self._live), dtype=np.uint32)

    def _add_frames(self, frames, level):
        return self._add_codes(self.encode(frames, level))

    def _remove(self, ids):
        self._live[ids] = 0

    def codes(self, first=0, n=None, device=False):
        return self._codes[first:None if n is None else first + n].copy()

    def _query(self, kind, what, level, k, skip_from, skip_to, distances, device):
        queries = self.encode(what, level) if kind == "frames" else what if kind == "codes" else self._codes[what]
        skip = None if skip_from is None else np.stack([skip_from, skip_to], 1)
        rows, D = topk_host(self._codes, self._live, queries, k, skip)
        return (rows, D) if distances else rows


def plane_pyramid(rng, w=40, h=30):
    return HostPyramid([random_planes(rng, w, h, 0.1)])


def nudged(rng, pyramid, share):
    """the pyramid with `share` of its pixels drawn anew"""
    I, Z = (x.copy() for x in pyramid.planes[0])
    J, Y = random_planes(rng, I.shape[1], I.shape[0], 0.1)
    pick = rng.uniform(size=I.shape) < share
    I[pick], Z[pick] = J[pick], Y[pick]
    return HostPyramid([(I, Z)])


def test_harvest_adds_only_what_is_far_enough():
    rng = np.random.default_rng(1)
    book = HostCodebook(m=256, capacity=8, seed=2)
    a, b = plane_pyramid(rng), plane_pyramid(rng)
    assert book.harvest(a, 0, 40) == 0                                              # an empty book takes anything
    near = nudged(rng, a, 0.02)
    d_near = distance_host(book.encode([near], 0)[0], book.codes()[0])
    d_far = distance_host(book.encode([b], 0)[0], book.codes()[0])
    assert 0 < d_near < 40 < d_far
    assert book.harvest(near, 0, 40) is None and book.size == 1
    assert book.harvest(near, 0, d_near) == 1 and book.harvest(near, 0, 1) is None  # at least min_distance away: taken; now stored: 0 away
    assert book.harvest(b, 0, 40) == 2
    book.remove([0, 1])
    assert book.harvest(a, 0, 40) == 3 and book.live == 2                           # the dead do not hold a newcomer off
    with pytest.raises(ValueError):
        book.harvest(a, 1, 40)
    with pytest.raises(TypeError):
        book.harvest(a, 0, 1.5)


def test_candidates_and_growth():
    rng = np.random.default_rng(2)
    scenes_ = [plane_pyramid(rng) for _ in range(6)]
    book = HostCodebook(m=256, capacity=6, seed=4)
    assert book.add(scenes_, 0).tolist() == list(range(6))
    with pytest.raises(d.DvoHipError) as full:
        book.add(scenes_[:1], 0)
    assert full.value.code == _lib.ERR_CAPACITY and book.size == 6
    queries = [nudged(rng, scenes_[4], 0.05), nudged(rng, scenes_[1], 0.05)]
    got = d.relocalisation_candidates(book, queries, 0, k=3)
    assert [g[0][0] for g in got] == [4, 1] and all(len(g) == 3 and g[0][1] < g[1][1] - 8 for g in got)
    near = d.relocalisation_candidates(book, queries, 0, k=3, max_distance=got[0][0][1])
    assert near[0] == got[0][:1] and all(dist <= got[0][0][1] for g in near for _, dist in g)
    # growth past the capacity: a new book with the same ids, and the dead stay dead
    book.remove([2])
    big = book.grown()
    assert big.capacity == 12 and big.size == 6 and big.live == 5 and np.array_equal(big.codes(), book.codes())
    assert big.ferns().tobytes() == book.ferns().tobytes() and big.dead().tolist() == [2]
    assert big.add(queries, 0).tolist() == [6, 7]
    # all against the own book: an entry finds itself unless its window is skipped
    ids = [4, 6, 1, 7]
    assert [g[0] for g in d.loop_closure_candidates_by_appearance(big, ids, 0, k=2)] == [(6, got[0][0][1]), (4, got[0][0][1]), (7, got[1][0][1]), (1, got[1][0][1])]
    wide = d.loop_closure_candidates_by_appearance(big, ids, 1, k=8)
    for i, g in zip(ids, wide):
        assert all(abs(j - i) > 1 and j != 2 for j, _ in g) and [x[1] for x in g] == sorted(x[1] for x in g)
    assert d.loop_closure_candidates_by_appearance(big, [4], 0, k=2, max_distance=0) == [[]]
    D = big.distance_matrix()
    assert D.shape == (8, 8) and np.all(D[:, 2] == MASKED) and np.all(np.diag(D)[[0, 1, 3]] == 0) and D[4, 6] == got[0][0][1]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "book.npz")
        big.save(path)
        back = HostCodebook.load(path)
    assert back.info() == big.info() and np.array_equal(back.codes(), big.codes()) and back.dead().tolist() == [2]
    assert np.array_equal(back.query(queries, 0, k=3), big.query(queries, 0, k=3))


def test_wrappers_reject_bad_arguments_before_the_library():
    rng = np.random.default_rng(3)
    book = HostCodebook(m=128, capacity=4)
    book.add([plane_pyramid(rng)], 0)
    code = book.codes()
    for bad in (dict(m=200), dict(m=64), dict(m=2176), dict(capacity=0), dict(capacity=(1 << 24) + 1), dict(z_lo=2.0, z_hi=1.0), dict(z_lo=float("nan")),
                dict(ferns=np.zeros(64, d.FERN_DTYPE)), dict(ferns=np.zeros(128, np.uint32))):
        with pytest.raises(ValueError):
            HostCodebook(**dict(dict(m=128, capacity=4), **bad))
    for call in (lambda: book.query_codes(code, k=0), lambda: book.query_codes(code, k=65), lambda: book.query_codes(code[:, :8]),
                 lambda: book.query_codes(code, skip=[(0, 1), (0, 1)]), lambda: book.query_ids([1]), lambda: book.query_ids([-1]), lambda: book.remove([1]),
                 lambda: book.query([], 0), lambda: book.add_codes(np.zeros((0, 16), np.uint32))):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: book.query_codes(code.astype(np.int64)), lambda: book.query_codes(code, k=1.0), lambda: book.query_ids([0.5]),
                 lambda: HostCodebook(m=128.0)):
        with pytest.raises(TypeError):
            call()
    assert C.sizeof(C.c_uint32) * 4 == d.FERN_DTYPE.itemsize == 16 and d.CODE_MATCH_DTYPE.itemsize == 8


# ---- 5. the retrieval condition ----------------------------------------------------------------------------------------------------------

RETRIEVAL = dict(scenes=16, w=160, h=120, level=2, m=256, seed=0, margin=8)


@functools.lru_cache(maxsize=None)
def retrieval_sequences():
    """frames 0 and 1 of the 16 scenes: (grey u8, depth u16, K) per scene"""
    out = []
    for s in range(RETRIEVAL["scenes"]):
        q = datagen.synth_sequence(100 + s, 3, w=RETRIEVAL["w"], h=RETRIEVAL["h"])
        out.append((q["grey"][:2].copy(), q["depth"][:2].copy(), q["K"]))
    return out


def retrieval_margins(book, stored, queries, level):
    """per scene (distance to the own scene, least distance to another scene) of its query, after the stored frames entered the book"""
    assert book.add(stored, level).tolist() == list(range(len(stored)))
    rows, D = book.query(queries, level, k=2, distances=True)
    D = np.asarray(D).astype(np.int64)
    own = np.diag(D)
    other = np.where(np.eye(len(stored), dtype=bool), 1 << 20, D).min(1)
    return rows, own, other


def test_retrieval_condition_on_the_host_build():
    """Not a quality claim: a condition that keeps the feature from being vacuous.  Frame 0 of each of 16 synthetic scenes is in the book
    at level 2 (40 x 30) with m = 256; the query with frame 1 of every scene returns its own scene first with a margin of at least 8
    ferns, over the project's own planes (the oracle's pyramid, which the device planes equal)."""
    level = RETRIEVAL["level"]
    def pyramid(grey, depth, K):
        o = po.Pyramid(grey.astype(f32), po.convert_raw_depth(depth), K, level + 1)
        return HostPyramid([(o.plane(l, 0)[0], o.plane(l, 1)[0]) for l in range(level + 1)])
    seqs = retrieval_sequences()
    stored = [pyramid(g[0], z[0], K) for g, z, K in seqs]
    queries = [pyramid(g[1], z[1], K) for g, z, K in seqs]
    assert stored[0].planes[level][0].shape == (30, 40)
    book = HostCodebook(m=RETRIEVAL["m"], capacity=16, seed=RETRIEVAL["seed"])
    rows, own, other = retrieval_margins(book, stored, queries, level)
    print("own scene at most %d, nearest other scene at least %d, worst margin %d" % (own.max(), other.min(), (other - own).min()))
    assert rows["id"][:, 0].tolist() == list(range(16))
    assert (other - own).min() >= RETRIEVAL["margin"], (own.tolist(), other.tolist())
    assert np.array_equal(rows["distance"][:, 0], own) and np.array_equal(rows["distance"][:, 1], other)


# ---- 6. the C++ facade ----------------------------------------------------------------------------------------------------------------------

def build_appearance_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "appearance_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "appearance_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_appearance_compiles():
    d.build()
    assert os.path.exists(build_appearance_facade_check())
