"""CPU tier: a keyframe map that follows the pose graph (dvo_slam_amd/csrc/cloud_map.h, Removal and Rehash), without a GPU.
  * map_host_update and map_host_rehash below are written against the header's helpers (map_word, map_negate, map_slot_live,
    map_slot_vacant) and compiled like tests/test_cloud_map.py's library (g++ -Wall -Werror -ffp-contract=off); UpdMap extends that
    file's HostMap by subclassing.  map_host_update adds and subtracts WHOLE WORDS, as the device does;
  * remove after insert equals never inserted -- sorted extractions and statistics, bit for bit -- in any order of the pixels and
    with the frame split over calls; a word-wise insert equals the yardstick's field-wise one;
  * removing an over-limit voxel's points restores the words, carries between the halves included;
  * a key behind a vacant slot is still found; a lookup that meets an empty slot is unmatched and claims nothing;
  * rehash drops vacant slots and preserves every record; into too small a table it reports and leaves the map as it was;
  * unmatched points are counted and subtract nothing;
  * the Python wrappers refuse bad arguments before the library; the facade compiles with setIncremental
    (tests/cpp/map_update_facade_check.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import scenes
from dvo_slam_amd import tracker
from test_cloud_map import CSRC, INF, MAX_PROBES, ROOT, FakePyramid, HostMap, _d, _f, assert_maps_identical, float_views, host_lib

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include "cloud_map.h"
using namespace dvo_hip;
extern "C" {
// The pixels first .. first + count - 1 of the frame (reverse != 0: last to first) into (sign > 0) or out of (sign < 0) the table, as
// k_map_insert does it: {n, sx} and {sy, sz} as one 64-bit add each, si as a 32-bit one.
// counters: those of tests/test_cloud_map.py (0 usable points in range, 1 dropped, 2 out of range, 3 unusable, 4 probes, 5 occupied);
// a removal takes its out-of-range and unusable pixels back.  ucounters: 0 points subtracted, 1 unmatched.
void map_host_update(MapSlot* slots, uint64_t capacity, uint64_t* counters, uint64_t* ucounters, float leaf, const float* K, const double* T16,
                     int w, int h, const float* I, const float* Z, float min_depth, float max_depth, int first, int count, int reverse, int sign) {
  const MapPose pose = map_pose_prepare(T16);
  const uint64_t one = sign > 0 ? 1 : map_negate(1);
  for (int k = 0; k < count; ++k) {
    const int i = reverse ? first + count - 1 - k : first + k;
    float P[3];
    uint64_t key;
    uint32_t q[4];
    if (!map_world_point(pose, K, i % w, i / w, Z[i], min_depth, max_depth, P)) { counters[3] += one; continue; }
    if (!map_key_of(P, I[i], leaf, &key, q)) { counters[2] += one; continue; }
    if (sign > 0) counters[0] += 1;
    uint64_t at = map_hash(key, capacity);
    bool placed = false;
    for (int p = 0; p < kMapMaxProbes && !placed; ++p, at = (at + 1) & (capacity - 1)) {
      counters[4] += 1;
      MapSlot& s = slots[at];
      if (s.key == kMapEmptyKey) {
        if (sign < 0) break;                                       // a lookup never claims a slot
        s.key = key;
        counters[5] += 1;
      }
      if (s.key != key) continue;
      uint64_t w1 = map_word(s.n, s.sx), w2 = map_word(s.sy, s.sz);
      const uint64_t a1 = map_word(1u, q[0]), a2 = map_word(q[1], q[2]);
      w1 += sign > 0 ? a1 : map_negate(a1);
      w2 += sign > 0 ? a2 : map_negate(a2);
      s.n = uint32_t(w1); s.sx = uint32_t(w1 >> 32); s.sy = uint32_t(w2); s.sz = uint32_t(w2 >> 32);
      s.si += sign > 0 ? q[3] : 0u - q[3];
      placed = true;
    }
    if (sign < 0) ucounters[placed ? 0 : 1] += 1;
    else if (!placed) counters[1] += 1;
  }
}
// every live slot of `from` into `to` (cleared here) with its sums unchanged; out[0] = slots claimed, out[1] = records without a slot
void map_host_rehash(const MapSlot* from, uint64_t from_capacity, MapSlot* to, uint64_t to_capacity, uint64_t* out) {
  for (uint64_t i = 0; i < to_capacity; ++i) { std::memset(&to[i], 0, sizeof(MapSlot)); to[i].key = kMapEmptyKey; }
  out[0] = out[1] = 0;
  for (uint64_t i = 0; i < from_capacity; ++i) {
    const MapSlot& s = from[i];
    if (!map_slot_live(s.key, s.n)) continue;
    uint64_t at = map_hash(s.key, to_capacity);
    bool placed = false;
    for (int p = 0; p < kMapMaxProbes && !placed; ++p, at = (at + 1) & (to_capacity - 1)) {
      if (to[at].key != kMapEmptyKey) continue;
      to[at] = s;
      to[at].pad = 0;
      placed = true;
    }
    out[placed ? 0 : 1] += 1;
  }
}
uint64_t map_host_vacant(const MapSlot* slots, uint64_t capacity) {
  uint64_t n = 0;
  for (uint64_t i = 0; i < capacity; ++i) n += map_slot_vacant(slots[i].key, slots[i].n) ? 1 : 0;
  return n;
}
}
"""


@functools.lru_cache(maxsize=None)
def update_lib():
    tmp = tempfile.mkdtemp(prefix="map_update_host_")
    src, out = os.path.join(tmp, "map_update_host.cpp"), os.path.join(tmp, "map_update_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    fp, dp, vp, u64 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p, C.c_uint64
    L.map_host_update.argtypes = [vp, u64, vp, vp, C.c_float, fp, dp, C.c_int, C.c_int, fp, fp, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
    L.map_host_update.restype = None
    L.map_host_rehash.argtypes = [vp, u64, vp, u64, vp]
    L.map_host_rehash.restype = None
    L.map_host_vacant.argtypes = [vp, u64]
    L.map_host_vacant.restype = u64
    return L


class UpdMap(HostMap):
    """the yardstick map with removal and rehash"""

    def __init__(self, leaf, capacity):
        self.ucounters = np.zeros(2, np.uint64)
        super().__init__(leaf, capacity)

    def clear(self):
        super().clear()
        self.ucounters[:] = 0

    def update(self, sign, I, Z, K, T, min_depth=0.0, max_depth=INF, first=0, count=None, reverse=False):
        h, w = Z.shape
        (ki, kp), (ti, tp), (ii, ip), (zi, zp) = _f(K), _d(T), _f(I), _f(Z)
        update_lib().map_host_update(self.slots.ctypes.data, self.capacity, self.counters.ctypes.data, self.ucounters.ctypes.data, self.leaf, kp, tp,
                                     w, h, ip, zp, min_depth, max_depth, first, w * h - first if count is None else count, 1 if reverse else 0, sign)
        return self

    def insert_words(self, *a, **k):
        return self.update(1, *a, **k)

    def remove(self, *a, **k):
        return self.update(-1, *a, **k)

    def vacant(self):
        return int(update_lib().map_host_vacant(self.slots.ctypes.data, self.capacity))

    def stats(self):
        s = super().stats()
        removed, unmatched = (int(x) for x in self.ucounters)
        s.update(points=s["points"] - removed, removed=removed, unmatched=unmatched, vacant=self.vacant())
        return s

    def extract(self):
        """(xyzi, counts, keys, voxels over the limit) of the live slots, sorted by key"""
        n = self.stats()["occupied"]
        xyzi, counts, keys = np.empty((max(n, 1), 4), np.float32), np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.uint64)
        over = C.c_uint64(0)
        got = host_lib().map_host_extract(self.slots.ctypes.data, self.capacity, self.leaf, xyzi.ctypes.data, counts.ctypes.data, keys.ctypes.data,
                                          C.byref(over))
        assert got == n - self.vacant()
        order = np.argsort(keys[:got], kind="stable")
        return xyzi[:got][order], counts[:got][order], keys[:got][order], int(over.value)

    def rehash(self, capacity=None):
        """True and the new table, or False and the map as it was"""
        capacity = self.capacity if capacity is None else capacity
        assert capacity >= 64 and capacity & (capacity - 1) == 0
        to, out = np.empty(capacity * 32, np.uint8), np.zeros(2, np.uint64)
        update_lib().map_host_rehash(self.slots.ctypes.data, self.capacity, to.ctypes.data, capacity, out.ctypes.data)
        if out[1] != 0:
            return False
        self.slots, self.capacity = to, capacity
        self.counters[0] -= self.counters[1]                       # points is unchanged
        self.counters[1] = 0
        self.counters[5] = out[0]
        return True


STAT_KEYS = ("points", "dropped", "out_of_range", "unusable")


def four_views(w, h):
    """(K, [(I, Z, T)] x 4): the two views of float_views and the same planes under poses a few centimetres off, as
    tests/test_gpu_cloud_map.py::frames_of poses its frames"""
    K, views = float_views(w, h)
    out = []
    for k in range(4):
        I, Z, T = views[k % 2]
        if k >= 2:
            T = T @ scenes.se3_exp([0.03 * k, -0.02, 0.01 * k, 0.01, -0.02 * k, 0.015])
        out.append((I, Z, T))
    return K, out


# ---- removal ----------------------------------------------------------------------------------------------------------------------------

def test_a_wordwise_insert_equals_the_fieldwise_yardstick():
    K, views = four_views(128, 96)
    a, b = HostMap(0.02, 1 << 16), UpdMap(0.02, 1 << 16)
    for I, Z, T in views:
        a.insert(I, Z, K, T)
        b.insert_words(I, Z, K, T)
    assert np.array_equal(a.slots, b.slots) and np.array_equal(a.counters, b.counters) and a.stats()["occupied"] > 10000


@pytest.mark.parametrize("w,h,leaf", [(128, 96, 0.02), (102, 78, 0.5)])
@pytest.mark.parametrize("gone", [0, 2])
def test_remove_after_insert_equals_never_inserted(w, h, leaf, gone):
    K, views = four_views(w, h)
    cap = 1 << 16
    never = HostMap(leaf, cap)
    for k, (I, Z, T) in enumerate(views):
        if k != gone:
            never.insert(I, Z, K, T)
    n = w * h
    I, Z, T = views[gone]
    for how in ("forward", "backward", "split"):
        m = UpdMap(leaf, cap)
        for Ik, Zk, Tk in views:
            m.insert(Ik, Zk, K, Tk)
        full, full_points = m.stats()["occupied"], m.stats()["points"]
        if how == "forward":
            m.remove(I, Z, K, T)
        elif how == "backward":
            m.remove(I, Z, K, T, reverse=True)
        else:
            m.remove(I, Z, K, T, first=n // 3)
            m.remove(I, Z, K, T, first=0, count=n // 3)
        s, want = m.stats(), never.stats()
        assert_maps_identical(m.extract(), never.extract(), how)
        for key in STAT_KEYS:
            assert s[key] == want[key], (how, key)
        assert s["unmatched"] == 0 and s["removed"] == full_points - want["points"] > 0
        assert s["occupied"] == full and s["vacant"] == full - want["occupied"] and s["vacant"] > 0     # the keys stay in their slots


def one_pixel(x, y=0.0, z=1.0, intensity=100.0):
    """(I, Z, K, T) of a 1 x 1 frame whose only point lies at (x, y, z)"""
    T = np.eye(4)
    T[0, 3], T[1, 3] = x, y
    return np.full((1, 1), intensity, np.float32), np.full((1, 1), z, np.float32), np.array([1.0, 1.0, 0.0, 0.0], np.float32), T


def slot_words(m, at):
    return m.slots[at * 32:at * 32 + 32].view(np.uint32).copy()    # key lo hi | n sx sy sz si pad


def test_removing_an_over_limit_voxels_points_restores_the_words():
    """a voxel far beyond 2^20 points whose low halves stand just below a carry: the insertion carries from n into sx and from sy
    into sz, the removal borrows it back"""
    m = UpdMap(1.0, 64)
    frame = one_pixel(0.75, 0.5, 1.25, 255.0)                       # q = 768, 512, 256; qi = 4080
    m.insert_words(*frame)
    at = int(np.nonzero(m.slots.view(np.uint64).reshape(-1, 4)[:, 0] != np.uint64(2 ** 64 - 1))[0][0])
    assert list(slot_words(m, at)[2:7]) == [1, 768, 512, 256, 4080]
    words = m.slots[at * 32:at * 32 + 32].view(np.uint32)
    words[2:7] = [0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFF00, 12345, 0xFFFFFFF0]   # n, sx, sy, sz, si
    before = slot_words(m, at)
    m.insert_words(*frame)
    after = slot_words(m, at)
    assert after[2] == 0 and after[3] == 0x7FFFFFFF + 768 + 1      # the carry out of n went into sx
    assert after[4] == (0xFFFFFF00 + 512) % 2 ** 32 and after[5] == 12345 + 256 + 1 and after[6] == (0xFFFFFFF0 + 4080) % 2 ** 32
    m.remove(*frame)
    assert np.array_equal(slot_words(m, at), before) and m.stats()["unmatched"] == 0
    # ... and an over-limit voxel as the extraction sees it: n > 2^20 before and after
    words[2:7] = [(1 << 20) + 5, 3, 4, 5, 6]
    before = slot_words(m, at)
    m.insert_words(*frame)
    assert m.extract()[3] == 1
    m.remove(*frame)
    assert np.array_equal(slot_words(m, at), before) and m.extract()[3] == 1


def colliding_points(capacity, leaf=1.0):
    """x of three points whose voxels hash to the same slot of a table of `capacity`"""
    L = host_lib()
    by_start = {}
    for i in range(4000):
        x = (i + 0.5) * leaf
        key = int(L.map_host_pack(i, 0, 1))
        by_start.setdefault(int(L.map_host_hash(key, capacity)), []).append(x)
        if len(by_start[int(L.map_host_hash(key, capacity))]) == 3:
            return by_start[int(L.map_host_hash(key, capacity))], int(L.map_host_hash(key, capacity))
    raise AssertionError("no three colliding keys")


def test_a_key_behind_a_vacant_slot_is_still_found():
    (xa, xb, xc), start = colliding_points(64)
    m = UpdMap(1.0, 64)
    m.insert_words(*one_pixel(xa)).insert_words(*one_pixel(xb))
    nxt = (start + 1) & 63
    assert slot_words(m, start)[2] == 1 and slot_words(m, nxt)[2] == 1 and m.stats()["occupied"] == 2
    m.remove(*one_pixel(xa))
    assert slot_words(m, start)[2] == 0 and m.stats()["vacant"] == 1 and m.stats()["occupied"] == 2
    m.insert_words(*one_pixel(xb))                                  # walks over the vacant slot to its own, claims none
    assert slot_words(m, nxt)[2] == 2 and m.stats()["occupied"] == 2
    m.remove(*one_pixel(xb)).remove(*one_pixel(xb))
    assert slot_words(m, nxt)[2] == 0 and m.stats()["unmatched"] == 0 and m.stats()["vacant"] == 2 and len(m.extract()[2]) == 0
    # a key that was never inserted: its lookup walks the two and meets an empty slot -- unmatched, nothing claimed or changed
    snapshot = m.slots.copy()
    m.remove(*one_pixel(xc))
    assert m.stats()["unmatched"] == 1 and m.stats()["occupied"] == 2 and np.array_equal(m.slots, snapshot)
    m.insert_words(*one_pixel(xa))                                  # a vacant slot takes its key's points again
    assert slot_words(m, start)[2] == 1 and m.stats()["occupied"] == 2 and m.stats()["vacant"] == 1


def test_unmatched_points_are_counted_and_subtract_nothing():
    K, views = four_views(128, 96)
    m = UpdMap(0.02, 1 << 16)
    for I, Z, T in views[:2]:
        m.insert_words(I, Z, K, T)
    before, points = m.extract(), m.stats()["points"]
    I, Z, T = views[0]
    usable = int((np.isfinite(Z) & (Z > 0)).sum())
    m.remove(I, Z, K, T @ scenes.se3_exp([0.2, 0.1, -0.1, 0.0, 0.05, 0.0]))       # not the pose of the insertion
    s = m.stats()
    assert s["unmatched"] > 0 and s["removed"] + s["unmatched"] == usable and s["points"] == points - s["removed"]
    assert int(m.extract()[1].sum()) == int(before[1].sum()) - s["removed"]       # what was not matched subtracted nothing
    empty = UpdMap(0.02, 1 << 10)
    snapshot = empty.slots.copy()
    empty.remove(I, Z, K, T)
    assert empty.stats()["unmatched"] == usable and empty.stats()["removed"] == 0 and np.array_equal(empty.slots, snapshot)
    assert empty.stats()["probes"] == usable                        # one probe each: the first slot is empty


# ---- rehash -----------------------------------------------------------------------------------------------------------------------------

def test_rehash_drops_vacant_slots_and_preserves_every_record():
    K, views = four_views(128, 96)
    leaf, cap = 0.02, 1 << 16
    for new_cap in (None, 1 << 17):
        m, never = UpdMap(leaf, cap), HostMap(leaf, new_cap or cap)
        for k, (I, Z, T) in enumerate(views):
            m.insert_words(I, Z, K, T)
            if k != 1:
                never.insert(I, Z, K, T)
        m.remove(*views[1][:2], K, views[1][2])
        before, s0 = m.extract(), m.stats()
        assert s0["vacant"] > 1000 and m.rehash(new_cap)
        s = m.stats()
        assert_maps_identical(m.extract(), before, "rehash")
        assert s["vacant"] == 0 and s["occupied"] == len(before[2]) == never.stats()["occupied"] and s["capacity"] == (new_cap or cap)
        for key in STAT_KEYS + ("removed", "unmatched"):
            assert s[key] == s0[key], key
        # the SET of slots in use does not depend on the order of arrival: it is that of a table that never held the frame
        in_use = lambda x: x.slots.view(np.uint64).reshape(-1, 4)[:, 0] != np.uint64(2 ** 64 - 1)
        assert np.array_equal(in_use(m), in_use(never))
        # the rebuilt table takes a later insert and a later remove like one that was built that way
        m.insert_words(*views[1][:2], K, views[1][2]).remove(*views[3][:2], K, views[3][2])
        never.insert(*views[1][:2], K, views[1][2])
        want = HostMap(leaf, cap)
        for k in (0, 1, 2):
            want.insert(*views[k][:2], K, views[k][2])
        assert_maps_identical(m.extract(), want.extract(), "after the rehash")
        assert m.stats()["unmatched"] == 0 and m.stats()["points"] == want.stats()["points"]


def test_rehash_into_too_small_a_table_reports_and_leaves_the_map_as_it_was():
    K, views = four_views(128, 96)
    m = UpdMap(0.02, 1 << 16)
    for I, Z, T in views:
        m.insert_words(I, Z, K, T)
    slots, counters = m.slots.copy(), m.counters.copy()
    assert m.stats()["occupied"] > 64 and not m.rehash(64)
    assert m.capacity == 1 << 16 and np.array_equal(m.slots, slots) and np.array_equal(m.counters, counters)
    # a map that overflowed grows: what it took is kept, the dropped points are forgotten
    small = UpdMap(0.02, 64)
    small.insert_words(*views[0][:2], K, views[0][2])
    s0 = small.stats()
    assert s0["dropped"] > 0 and small.rehash(1 << 10)
    s = small.stats()
    assert s["dropped"] == 0 and s["points"] == s0["points"] and s["occupied"] == 64 and small.longest_run() < MAX_PROBES


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------------

def test_python_wrappers_refuse_bad_arguments_before_the_library():
    ctx = object()                                                   # (no library behind it: a call that got that far raises AttributeError)
    m = d.KeyframeMap.__new__(d.KeyframeMap)
    m.ctx, m.ptr, m.leaf = ctx, None, 0.01
    two = [FakePyramid(ctx), FakePyramid(ctx)]
    eye2 = np.stack([np.eye(4), np.eye(4)])
    for call in (lambda: m.remove(two, eye2[:1]), lambda: m.remove(two, np.zeros((2, 3, 4))), lambda: m.remove([], eye2),
                 lambda: m.remove(two, eye2, level=3), lambda: m.remove(two, eye2, min_depth=2.0, max_depth=1.0),
                 lambda: m.remove([FakePyramid(object()), FakePyramid(object())][:1] + two[:1], eye2),
                 lambda: m.remove([FakePyramid(object())], np.eye(4)),
                 lambda: m.move(two, eye2, eye2[:1]), lambda: m.move(two, eye2[:1], eye2), lambda: m.move(two, eye2, np.zeros((2, 16))),
                 lambda: m.move(two, eye2, eye2, level=-1), lambda: m.move(two, eye2, eye2, min_depth=float("nan")),
                 lambda: m.move([FakePyramid(object())], np.eye(4), np.eye(4)),
                 lambda: m.rehash(0), lambda: m.rehash(63), lambda: m.rehash(1000), lambda: m.rehash(32), lambda: m.rehash(1 << 33)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: m.remove(two, eye2, level=1.0), lambda: m.move(two, eye2, [["a"] * 4] * 4), lambda: m.rehash(1024.0), lambda: m.rehash(True)):
        with pytest.raises(TypeError):
            call()
    assert tracker._rehash_capacity(None) == 0 and tracker._rehash_capacity(1 << 20) == 1 << 20 and tracker._rehash_capacity(np.int64(64)) == 64
    assert C.sizeof(d._lib.MapStats) == 16 * 8
    fields = [name for name, _ in d._lib.MapStats._fields_]
    assert fields[:8] == ["occupied", "points", "dropped", "out_of_range", "unusable", "over_limit", "capacity", "updates"]
    assert fields[8:11] == ["vacant", "removed", "unmatched"] and d._lib.MapStats.reserved.size == 5 * 8
    for name in ("dvo_hip_map_remove", "dvo_hip_map_move", "dvo_hip_map_rehash"):
        assert name in d._lib.EXPORTS


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------------

def build_map_update_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "map_update_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "map_update_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_compiles_with_set_incremental():
    d.build()
    assert os.path.exists(build_map_update_facade_check())
