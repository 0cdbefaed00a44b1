"""CPU tier: keyframe sub-maps (dvo_slam_amd/csrc/cloud_map.h, Merge), without a GPU.
  * map_host_merge below is the host restatement of k_map_merge, written against the header's helpers (map_pose_record, map_word,
    map_negate, map_slot_live, colour_word) and compiled like tests/test_cloud_map.py's library (g++ -Wall -Werror -ffp-contract=off);
    MergeMap wraps a table of that file's HostMap (or of tests/test_map_colour.py's ColourHostMap) and is the yardstick of
    tests/test_gpu_map_merge.py;
  * the plain merge of two sub-maps equals the map built from all their keyframes at once -- sorted raw records and statistics, bit for
    bit -- in either order and from a shuffled record array, grey and coloured;
  * subtract after merge restores the records; a voxel only the subtracted map held is vacant and still on the probe path;
  * crafted records at the carry boundaries: absorbed twice and subtracted once the words equal a single absorb;
  * posed merge: subtraction under the same pose restores bit for bit; one voxel lands where its transformed centroid lies; over a scene
    the points are conserved and the point-weighted mean is kept to quantisation;
  * table edges: a lookup claims nothing, a full table drops and reports, a map that dropped refuses a subtraction;
  * the Python wrappers refuse bad arguments before the library; the facade compiles (tests/cpp/map_merge_facade_check.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import scenes
from dvo_slam_amd import _lib, tracker
from test_cloud_map import CSRC, ROOT, HostMap, _d, assert_maps_identical, host_lib
from test_map_update import UpdMap, colliding_points, four_views

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include "cloud_colour.h"
using namespace dvo_hip;
extern "C" {
// `count` records (and their colour records, or null) of leaf leaf_src into (sign > 0) or out of (sign < 0) the table, as k_map_merge
// does it: whole words.  T16 null: plain; else under that pose (map_pose_record).  counters: 0 usable points in range of what was
// added, 1 dropped, 2 out of range, 3 unusable, 4 slot updates, 5 occupied slots, 6 points to remove, 7 of them unmatched.
void map_host_merge(MapSlot* slots, MapColourSlot* tint, uint64_t capacity, uint64_t* counters, float leaf_dst, const MapSlot* rec,
                    const MapColourSlot* rec_tint, uint64_t count, float leaf_src, int sign, const double* T16) {
  const bool minus = sign < 0;
  MapPose pose;
  std::memset(&pose, 0, sizeof pose);
  if (T16) pose = map_pose_prepare(T16);
  for (uint64_t i = 0; i < count; ++i) {
    const MapSlot& r = rec[i];
    if (!map_slot_live(r.key, r.n)) continue;
    uint64_t key = r.key;
    uint32_t add[5] = {r.n, r.sx, r.sy, r.sz, r.si};
    if (T16) {
      const int how = map_pose_record(pose, r.key, r.n, r.sx, r.sy, r.sz, r.si, leaf_src, leaf_dst, &key, add);
      if (how == kMapPoseUnusable) { counters[3] += minus ? uint64_t(0) - r.n : uint64_t(r.n); continue; }
      if (how == kMapPoseOutOfRange) { counters[2] += minus ? uint64_t(0) - r.n : uint64_t(r.n); continue; }
    }
    counters[minus ? 6 : 0] += r.n;
    uint64_t at = map_hash(key, capacity);
    bool placed = false;
    for (int p = 0; p < kMapMaxProbes && !placed; ++p, at = (at + 1) & (capacity - 1)) {
      MapSlot& s = slots[at];
      if (s.key == kMapEmptyKey) {
        if (minus) break;                                          // a lookup never claims a slot
        s.key = key;
        counters[5] += 1;
      }
      if (s.key != key) continue;
      uint64_t w1 = map_word(s.n, s.sx), w2 = map_word(s.sy, s.sz);
      const uint64_t a1 = map_word(add[0], add[1]), a2 = map_word(add[2], add[3]);
      w1 += minus ? map_negate(a1) : a1;
      w2 += minus ? map_negate(a2) : a2;
      s.n = uint32_t(w1); s.sx = uint32_t(w1 >> 32); s.sy = uint32_t(w2); s.sz = uint32_t(w2 >> 32);
      s.si += minus ? 0u - add[4] : add[4];
      if (tint) {
        MapColourSlot& t = tint[at];
        uint64_t w3 = colour_word(t.sr, t.sg);
        const uint64_t a3 = colour_word(rec_tint[i].sr, rec_tint[i].sg);
        w3 += minus ? map_negate(a3) : a3;
        t.sr = uint32_t(w3); t.sg = uint32_t(w3 >> 32);
        t.sb += minus ? 0u - rec_tint[i].sb : rec_tint[i].sb;
      }
      counters[4] += 1;
      placed = true;
    }
    if (!placed) counters[minus ? 7 : 1] += r.n;
  }
}
void map_host_pose_point(const double* T16, const float* c, float* P) { map_pose_point(map_pose_prepare(T16), c, P); }
}
"""

RECORD, COLOUR_RECORD = np.dtype(_lib.MAP_RECORD), np.dtype(_lib.MAP_COLOUR_RECORD)
EMPTY = np.uint64(2 ** 64 - 1)
MAX_POINTS = 1 << 20                                               # kMapVoxelMaxPoints


@functools.lru_cache(maxsize=None)
def merge_lib():
    tmp = tempfile.mkdtemp(prefix="map_merge_host_")
    src, out = os.path.join(tmp, "map_merge_host.cpp"), os.path.join(tmp, "map_merge_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    vp, u64 = C.c_void_p, C.c_uint64
    L.map_host_merge.argtypes = [vp, vp, u64, vp, C.c_float, vp, vp, u64, C.c_float, C.c_int, vp]
    L.map_host_merge.restype = None
    L.map_host_pose_point.argtypes = [vp, vp, vp]
    L.map_host_pose_point.restype = None
    return L


STAT_KEYS = ("points", "dropped", "out_of_range", "unusable", "over_limit")


class MergeMap:
    """the yardstick of a map that merges: cloud_map.h's table (and, coloured, cloud_colour.h's side table) in host memory"""

    def __init__(self, leaf, capacity, colour=False):
        self.leaf = float(np.float32(leaf))
        self.capacity = 64
        while self.capacity < capacity:
            self.capacity *= 2
        self.slots = np.zeros(self.capacity, RECORD)
        self.slots["key"] = EMPTY
        self.tint = np.zeros(self.capacity, COLOUR_RECORD) if colour else None
        self.counters = np.zeros(8, np.uint64)

    @classmethod
    def of(cls, built):
        """the table a tests/test_cloud_map.py HostMap (or UpdMap) or a tests/test_map_colour.py ColourHostMap holds, adopted"""
        coloured = hasattr(built, "colour")
        m = cls(built.leaf, built.capacity, coloured)
        m.slots[:] = built.slots.view(RECORD)
        c = built.counters
        if coloured:
            m.tint[:] = built.colour.view(COLOUR_RECORD)
            m.counters[:] = [c[0], c[1], c[2], c[3], 0, c[5], c[6], c[7]]
        else:
            removed, unmatched = (int(x) for x in getattr(built, "ucounters", (0, 0)))
            m.counters[:] = [c[0], c[1], c[2], c[3], 0, c[5], removed + unmatched, unmatched]
        return m

    def copy(self):
        m = MergeMap(self.leaf, self.capacity, self.tint is not None)
        m.slots[:], m.counters[:] = self.slots, self.counters
        if self.tint is not None:
            m.tint[:] = self.tint
        return m

    def absorb(self, records, colour=None, leaf=None, sign=1, pose=None):
        """what dvo_hip_map_merge_records does, refusals included"""
        leaf = self.leaf if leaf is None else float(np.float32(leaf))
        assert (colour is not None) == (self.tint is not None) and sign in (1, -1)
        if pose is None and np.float32(leaf) != np.float32(self.leaf):
            raise ValueError("a plain merge needs the destination's leaf")
        if sign < 0 and int(self.counters[1]) != 0:
            raise ValueError("the map has dropped points")
        records = np.ascontiguousarray(records, RECORD)
        colour = None if colour is None else np.ascontiguousarray(colour, COLOUR_RECORD)
        T = None if pose is None else _d(pose)[0]
        merge_lib().map_host_merge(self.slots.ctypes.data, None if self.tint is None else self.tint.ctypes.data, self.capacity, self.counters.ctypes.data,
                                   self.leaf, records.ctypes.data, None if colour is None else colour.ctypes.data, len(records), leaf, sign,
                                   None if T is None else T.ctypes.data)
        return self

    def merge(self, src, sign=1, pose=None):
        """what dvo_hip_map_merge does with one source: the table as it lies, and -- plain -- the source's out-of-range and unusable counts"""
        self.absorb(src.slots, src.tint, src.leaf, sign, pose)
        if pose is None:
            for k in (2, 3):
                self.counters[k] = np.uint64((int(self.counters[k]) + sign * int(src.counters[k])) % 2 ** 64)
        return self

    def subtract(self, src, pose=None):
        return self.merge(src, -1, pose)

    def live(self):
        return (self.slots["key"] != EMPTY) & (self.slots["n"] > 0)

    def records(self):
        """(records, colour records or None) of the live voxels, sorted by key; pad 0"""
        live = self.live()
        order = np.argsort(self.slots["key"][live], kind="stable")
        rec = self.slots[live][order].copy()
        rec["pad"] = 0
        return rec, (None if self.tint is None else self.tint[live][order].copy())

    def stats(self):
        c = [int(x) for x in self.counters]
        live = self.live()
        return dict(points=c[0] - c[1] - (c[6] - c[7]), dropped=c[1], out_of_range=c[2], unusable=c[3], updates=c[4], occupied=c[5],
                    removed=c[6] - c[7], unmatched=c[7], capacity=self.capacity, over_limit=int((self.slots["n"][live] > MAX_POINTS).sum()),
                    vacant=int(((self.slots["key"] != EMPTY) & (self.slots["n"] == 0)).sum()))

    def grey_table(self):
        """the slot table as a tests/test_cloud_map.py HostMap: for its extract() and for tests/test_map_render.py's render_host"""
        m = HostMap(self.leaf, self.capacity)
        m.slots[:] = self.slots.view(np.uint8)
        m.counters[5] = int(self.live().sum())
        return m

    def extract(self):
        return self.grey_table().extract()


def assert_records_identical(a, b, what=""):
    """two (records, colour records) pairs, each sorted by key: the same bytes"""
    assert a[0].shape == b[0].shape and np.array_equal(a[0]["key"], b[0]["key"]), "%s: keys differ" % (what,)
    assert a[0].tobytes() == b[0].tobytes(), "%s: sums differ" % (what,)
    assert (a[1] is None) == (b[1] is None), what
    if a[1] is not None:
        assert a[1].tobytes() == b[1].tobytes(), "%s: colour sums differ" % (what,)


def centroids(records, leaf):
    """the centroids [n, 3] of records in float64: (i + (s / n + 0.5) / 1024) * leaf per axis, the extraction without its rounding"""
    key, n = records["key"].astype(np.uint64), records["n"].astype(np.float64)
    out = np.empty((len(records), 3))
    for axis, (shift, s) in enumerate(((42, "sx"), (21, "sy"), (0, "sz"))):
        cell = ((key >> np.uint64(shift)) & np.uint64(0x1fffff)).astype(np.int64) - (1 << 20)
        out[:, axis] = (cell + (records[s].astype(np.float64) / n + 0.5) / 1024.0) * float(leaf)
    return out


def built(views, K, leaf=0.02, capacity=1 << 16):
    m = HostMap(leaf, capacity)
    for I, Z, T in views:
        m.insert(I, Z, K, T)
    return MergeMap.of(m)


def built_colour(frames, K, leaf=0.02, capacity=1 << 16):
    import test_map_colour as tmc
    m = tmc.ColourHostMap(leaf, capacity)
    for I, Z, T, plane0 in frames:
        m.insert(I, Z, K, T, plane0)
    return MergeMap.of(m)


POSE = scenes.se3_exp([0.31, -0.12, 0.07, 0.04, -0.09, 0.12])


# ---- plain merge ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [False, True])
def test_merge_of_two_submaps_equals_the_single_build(colour):
    if colour:
        import test_map_colour as tmc
        K, frames = tmc.scene_frames(128, 96, 4)
        frames = [(I, Z, T if k < 2 else T @ scenes.se3_exp([0.03 * k, -0.02, 0.01 * k, 0.01, -0.02 * k, 0.015]), p) for k, (I, Z, T, p) in enumerate(frames)]
        make = lambda part: built_colour(part, K)
    else:
        K, frames = four_views(128, 96)
        make = lambda part: built(part, K)
    whole, a, b = make(frames), make(frames[:2]), make(frames[2:])
    want, ws = whole.records(), whole.stats()
    assert ws["points"] > 20000 and ws["unusable"] > 0 and ws["dropped"] == 0
    assert len(np.intersect1d(a.records()[0]["key"], b.records()[0]["key"])) > 100      # voxels both sub-maps hold
    ab, ba = a.copy().merge(b), b.copy().merge(a)
    rng = np.random.default_rng(5)
    order = rng.permutation(b.capacity)                               # the raw table, shuffled: empty slots in between
    shuffled = a.copy().absorb(b.slots[order], None if b.tint is None else b.tint[order])
    for name, m in (("a + b", ab), ("b + a", ba), ("a + shuffled records of b", shuffled)):
        assert_records_identical(m.records(), want, name)
        for key in STAT_KEYS:
            if name.endswith("of b") and key in ("out_of_range", "unusable"):
                continue                                              # (records carry no such counts)
            assert m.stats()[key] == ws[key], (name, key)
    assert shuffled.stats()["unusable"] == a.stats()["unusable"]
    assert_maps_identical(ab.extract(), whole.extract(), "extraction")
    # an exported record array (live records only, compacted) is the same source
    rec, tint = b.records()
    assert_records_identical(a.copy().absorb(rec, tint).records(), want, "a + exported b")


def test_subtract_restores_and_a_vacated_voxel_stays_on_the_probe_path():
    K, views = four_views(128, 96)
    a, b = built(views[:2], K), built(views[2:], K)
    before, s0 = a.records(), a.stats()
    m = a.copy().merge(b)
    only_b = m.stats()["occupied"] - s0["occupied"]
    assert only_b > 100
    m.subtract(b)
    s = m.stats()
    assert_records_identical(m.records(), before, "merge, subtract")
    for key in STAT_KEYS:
        assert s[key] == s0[key], key
    assert s["unmatched"] == 0 and s["removed"] == b.stats()["points"] and s["vacant"] == only_b and s["occupied"] == s0["occupied"] + only_b
    # three keys that start at one slot: b's voxel is taken out again, the key behind it is still found
    (xa, xb, xc), start = colliding_points(64)
    one = lambda x: MergeMap.of(HostMap(1.0, 64).insert(np.full((1, 1), 100.0, np.float32), np.ones((1, 1), np.float32),
                                                           np.array([1.0, 1.0, 0.0, 0.0], np.float32), np.array([[1, 0, 0, x], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])))
    first, second, third = one(xa), one(xb), one(xc)
    dst = MergeMap(1.0, 64).merge(first).merge(second)
    assert dst.slots["n"][start] == 1 and dst.slots["n"][(start + 1) & 63] == 1
    dst.subtract(first)
    assert dst.slots["n"][start] == 0 and dst.slots["key"][start] != EMPTY and dst.stats()["vacant"] == 1
    dst.merge(second)                                                 # walks over the vacant slot to its own, claims none
    assert dst.slots["n"][(start + 1) & 63] == 2 and dst.stats()["occupied"] == 2
    snapshot = dst.slots.copy()
    dst.subtract(third)                                               # never merged: an empty slot ends the lookup
    assert dst.stats()["unmatched"] == 1 and np.array_equal(dst.slots, snapshot) and dst.stats()["occupied"] == 2


def test_carries_between_the_half_words():
    rec = np.zeros(3, RECORD)
    rec["key"] = [int(host_lib().map_host_pack(i, -2, 7)) for i in range(3)]
    rec["n"], rec["sx"], rec["sy"], rec["sz"], rec["si"] = 1 << 20, 1023 << 20, 1023 << 20, 1023 << 20, 4095 << 20
    rec[2] = (rec["key"][2], 0xFFFFFFFF, 0x80000001, 0xFFFFFF00, 7, 0xFFFFFFF0, 0)       # n and sy just below a carry
    once = MergeMap(0.5, 64).absorb(rec)
    assert once.stats()["over_limit"] == 1 and once.stats()["points"] == 2 * (1 << 20) + 0xFFFFFFFF
    m = MergeMap(0.5, 64).absorb(rec).absorb(rec)
    at = {int(k): i for i, k in enumerate(m.slots["key"]) if k != EMPTY}
    s = m.slots[at[int(rec["key"][0])]]
    assert s["n"] == 1 << 21 and s["sx"] == (1023 << 21) % 2 ** 32 and s["si"] == (4095 << 21) % 2 ** 32      # sums beyond 2^32 wrap
    t = m.slots[at[int(rec["key"][2])]]
    assert t["n"] == 0xFFFFFFFE and t["sx"] == (2 * 0x80000001 + 1) % 2 ** 32 and t["sz"] == 15                  # carries out of n and sy
    assert m.stats()["over_limit"] == 3                                # n alone decides
    m.absorb(rec, sign=-1)
    assert_records_identical(m.records(), once.records(), "twice in, once out")
    assert m.stats()["over_limit"] == 1 and m.stats()["unmatched"] == 0


# ---- posed merge ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [False, True])
def test_posed_subtraction_restores_bit_for_bit(colour):
    if colour:
        import test_map_colour as tmc
        K, frames = tmc.scene_frames(128, 96, 4)
        a, b = built_colour(frames[:2], K), built_colour(frames[2:], K, leaf=0.03)
    else:
        K, views = four_views(128, 96)
        a, b = built(views[:2], K), built(views[2:], K, leaf=0.03)
    before, s0 = a.records(), a.stats()
    m = a.copy().merge(b, pose=POSE)
    assert m.stats()["points"] == s0["points"] + b.stats()["points"] and m.records()[0].tobytes() != before[0].tobytes()
    m.subtract(b, pose=POSE)
    assert_records_identical(m.records(), before, "posed merge, posed subtract")
    s = m.stats()
    for key in STAT_KEYS:
        assert s[key] == s0[key], key
    assert s["unmatched"] == 0 and s["vacant"] > 0
    # another pose does not match: counted, and what was matched is subtracted from voxels of other points
    m = a.copy().merge(b, pose=POSE).subtract(b, pose=POSE @ scenes.se3_exp([0.5, 0.0, 0.0, 0.0, 0.0, 0.0]))
    assert m.stats()["unmatched"] > 0


def test_a_posed_voxel_lands_at_its_transformed_centroid():
    """bound per axis: leaf_dst / 2048 (the truncated offset, corrected by its half step) + float32 rounding: of the centroid (1/2 ulp),
    of the three products and three sums of a row (1/2 ulp each of at most |R| |c| + |t|), of P / leaf (1/2 ulp) and of the extracted
    float (1/2 ulp) -- 8 * 2^-24 * (|R| |c| + |t|) covers them"""
    leaf_src, leaf_dst = 0.02, 0.05
    rec = np.zeros(1, RECORD)
    rec[0] = (int(host_lib().map_host_pack(37, -12, 81)), 5, 5 * 700 + 3, 5 * 12, 5 * 1000 + 4, 5 * 1600, 0)
    dst = MergeMap(leaf_dst, 64).absorb(rec, leaf=leaf_src, pose=POSE)
    got, counts, keys, over = dst.extract()
    assert len(keys) == 1 and counts[0] == 5 and dst.stats()["points"] == 5
    c = centroids(rec, np.float32(leaf_src))[0]
    T32 = POSE.astype(np.float32).astype(np.float64)
    want = T32[:3, :3] @ c + T32[:3, 3]
    bound = np.float32(leaf_dst) / 2048.0 + 8 * 2.0 ** -24 * (np.abs(T32[:3, :3]) @ np.abs(c) + np.abs(T32[:3, 3]))
    assert np.all(np.abs(got[0, :3].astype(np.float64) - want) <= bound), (got[0], want)
    assert got[0, 3] == np.float32(1600 / 16.0)                        # the intensity sum goes unchanged
    # ... and the helper alone: the float transform of the float centroid
    cf, P = np.ascontiguousarray(c, np.float32), np.empty(3, np.float32)
    merge_lib().map_host_pose_point(_d(POSE)[0].ctypes.data, cf.ctypes.data, P.ctypes.data)
    assert np.all(np.abs(P.astype(np.float64) - want) <= bound - np.float32(leaf_dst) / 2048.0)


def test_a_posed_scene_conserves_points_and_keeps_the_weighted_mean():
    """Total points are conserved exactly, less the counted out-of-range ones.  The point-weighted mean position of the destination
    equals the source's, transformed in double, per axis within (leaf_src + leaf_dst) / 2048 -- the two truncations, each corrected by
    its half step -- plus 16 float32 ulps of the largest coordinate: the float centroid, the float transform (three products, three
    sums) and the division by the leaf are each rounded to half an ulp of a value no larger than the sum of four coordinates."""
    K, views = four_views(128, 96)
    leaf_src, leaf_dst = 0.02, 0.035
    src = built(views, K, leaf=leaf_src)
    n_src = src.stats()["points"]
    dst = MergeMap(leaf_dst, 1 << 16).merge(src, pose=POSE)
    s = dst.stats()
    assert s["out_of_range"] == 0 and s["unusable"] == 0 and s["dropped"] == 0 and s["points"] == n_src
    assert s["occupied"] < src.stats()["occupied"]                     # a coarser grid: voxels fused
    a, b = src.records()[0], dst.records()[0]
    assert int(b["n"].astype(np.uint64).sum()) == n_src
    T32 = POSE.astype(np.float32).astype(np.float64)
    ca, cb = centroids(a, np.float32(leaf_src)), centroids(b, np.float32(leaf_dst))
    moved = ca @ T32[:3, :3].T + T32[:3, 3]
    mean_src = (moved * a["n"][:, None].astype(np.float64)).sum(0) / n_src
    mean_dst = (cb * b["n"][:, None].astype(np.float64)).sum(0) / n_src
    largest = max(np.abs(ca).max(), np.abs(moved).max())
    bound = (np.float32(leaf_src) + np.float32(leaf_dst)) / 2048.0 + 16 * float(np.spacing(np.float32(largest)))
    err = np.abs(mean_dst - mean_src)
    print("weighted mean: error", err, "bound", bound)
    assert np.all(err <= bound), (err, bound)
    # beyond +-2^20 voxels nothing is placed and every point is counted
    far = POSE.copy()
    far[0, 3] = 0.035 * (1 << 20) + 100.0
    gone = MergeMap(leaf_dst, 1 << 16).merge(src, pose=far)
    assert gone.stats()["out_of_range"] == n_src and gone.stats()["points"] == 0 and gone.stats()["occupied"] == 0
    nan = POSE.copy()
    nan[1, 3] = np.inf
    assert MergeMap(leaf_dst, 64).merge(src, pose=nan).stats()["unusable"] == n_src


# ---- table edges ------------------------------------------------------------------------------------------------------------------------

def test_table_edges():
    K, views = four_views(128, 96)
    src = built(views[:1], K)
    n = src.stats()["points"]
    # a lookup that meets an empty slot is unmatched and claims nothing
    empty = MergeMap(0.02, 1 << 10)
    snapshot = empty.slots.copy()
    empty.subtract(src)
    assert empty.stats()["unmatched"] == n and empty.stats()["removed"] == 0 and empty.stats()["occupied"] == 0 and np.array_equal(empty.slots, snapshot)
    # more distinct keys than a table of 64 slots has: it fills, drops and says so
    small = MergeMap(0.02, 64).merge(src)
    s = small.stats()
    assert src.stats()["occupied"] > 64 and s["occupied"] == 64 and s["dropped"] > 0 and s["points"] + s["dropped"] == n
    # ... and refuses a subtraction: what it holds of the sub-map is not known
    before = small.slots.copy()
    with pytest.raises(ValueError):
        small.subtract(src)
    assert np.array_equal(small.slots, before)
    with pytest.raises(ValueError):
        MergeMap(0.03, 64).merge(src)                                 # a plain merge of another leaf


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------------

def fake_map(ctx, leaf=0.01, coloured=False):
    m = d.KeyframeMap.__new__(d.KeyframeMap)
    m.ctx, m.ptr, m.leaf, m.coloured = ctx, C.c_void_p(1), leaf, coloured
    return m


def test_python_wrappers_refuse_bad_arguments_before_the_library():
    ctx = object()                                                   # (no library behind it: a call that got that far raises AttributeError)
    m, a, b = fake_map(ctx), fake_map(ctx), fake_map(ctx)
    closed = fake_map(ctx)
    closed.ptr = None
    eye2, eye = np.stack([np.eye(4), np.eye(4)]), np.eye(4)
    bad = eye.copy()
    bad[2, 3] = np.nan
    rec, tint = np.zeros(3, RECORD), np.zeros(3, COLOUR_RECORD)
    coloured = fake_map(ctx, coloured=True)
    for call in (lambda: m.merge([m]), lambda: m.merge([a, m]), lambda: m.merge([closed]), lambda: m.merge([fake_map(object())]),
                 lambda: m.merge([fake_map(ctx, coloured=True)]), lambda: coloured.merge([a]), lambda: m.merge([fake_map(ctx, leaf=0.02)]),
                 lambda: m.merge([a, b], signs=[1]), lambda: m.merge([a, b], signs=[1, 0]), lambda: m.merge([a, b], signs=[1, 2]),
                 lambda: m.merge([a, b], poses=eye2[:1]), lambda: m.merge([a, b], poses=np.zeros((2, 3, 4))), lambda: m.merge([a], poses=bad),
                 lambda: m.subtract([m]), lambda: m.subtract([a], poses=bad), lambda: m.subtract([fake_map(ctx, leaf=0.02)]),
                 lambda: m.move_submaps([a, b], eye2, eye2[:1]), lambda: m.move_submaps([a, b], eye2[:1], eye2), lambda: m.move_submaps([a], eye, bad),
                 lambda: m.move_submaps([a], bad, eye), lambda: m.move_submaps([m], eye, eye), lambda: m.move_submaps([a], None, eye),
                 lambda: m.move_submaps([fake_map(ctx, coloured=True)], eye, eye),
                 lambda: m.absorb(rec, tint), lambda: coloured.absorb(rec), lambda: coloured.absorb(rec, tint[:2]), lambda: m.absorb(rec, leaf=0.02),
                 lambda: m.absorb(rec, sign=0), lambda: m.absorb(rec, sign=2), lambda: m.absorb(rec, pose=bad), lambda: m.absorb(rec, leaf=-1.0, pose=eye),
                 lambda: m.absorb(rec, leaf=float("nan"), pose=eye), lambda: m.absorb(rec, pose=np.zeros((3, 4))), lambda: m.absorb(rec[::2])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: m.merge([object()]), lambda: m.merge([a], signs=[1.0]), lambda: m.merge([a], signs=[True]), lambda: m.merge([a], poses=[["a"] * 4] * 4),
                 lambda: m.absorb(np.zeros((3, 8), np.uint32)), lambda: m.absorb(np.zeros(3, COLOUR_RECORD)), lambda: m.absorb(rec, sign=1.0),
                 lambda: m.absorb([1, 2, 3]), lambda: coloured.absorb(rec, np.zeros((3, 4), np.uint32))):
        with pytest.raises(TypeError):
            call()
    # what is fine reaches the library (here: the attribute lookup on the stand-in context)
    for call in (lambda: m.merge([a, b], signs=[1, -1], poses=eye2), lambda: m.merge(a), lambda: m.subtract([a, a]), lambda: m.move_submaps([a, b], eye2, eye2),
                 lambda: m.absorb(rec), lambda: coloured.absorb(rec, tint, leaf=0.02, sign=-1, pose=eye), lambda: m.export(), lambda: m.info()):
        with pytest.raises(AttributeError):
            call()
    assert m.merge([]) is None and m.move_submaps([], np.zeros((0, 4, 4)), np.zeros((0, 4, 4))) is None and m.absorb(rec[:0]) is None
    assert RECORD.itemsize == 32 and COLOUR_RECORD.itemsize == 16 and RECORD.names == ("key", "n", "sx", "sy", "sz", "si", "pad")
    for name in ("dvo_hip_map_info", "dvo_hip_map_merge", "dvo_hip_map_move_submaps", "dvo_hip_map_export", "dvo_hip_map_merge_records"):
        assert name in d._lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    for name in ("dvo_hip_map_info(", "dvo_hip_map_merge(", "dvo_hip_map_move_submaps(", "dvo_hip_map_export(", "dvo_hip_map_merge_records("):
        assert "int " + name in header


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------------

def build_map_merge_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "map_merge_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "map_merge_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_compiles_with_submaps():
    d.build()
    assert os.path.exists(build_map_merge_facade_check())
