"""CPU tier: colour in the keyframe map (dvo_slam_amd/csrc/cloud_colour.h), without a GPU.
  * cloud_colour.h with cloud_map.h and map_render.h compiled for the host with g++ -Werror and -ffp-contract=off; pack_plane(),
    level_colour() and ColourHostMap below are the yardstick of tests/test_gpu_map_colour.py: a table and its colour side table in host
    memory, filled, emptied, extracted and rendered with the headers' own functions;
  * colour_pack for the four pixel formats; the level mean against a numpy integer restatement at levels 0, 1, 2 and odd sizes, the
    blocks at the right and bottom edges included;
  * the extraction's rounding at n = 1, at n = 3 around the half, and at n = 2^20 with every channel 255;
  * insert followed by remove restores the side table's words; the result does not depend on the order of the pixels;
  * the colour view's depth plane equals the grey view's, holes are word 0;
  * the Python wrappers reject bad formats, pitches and shapes, and a grey map asked for colour, before the library is reached; the C++
    facade compiles (tests/cpp/map_colour_facade_check.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import test_cloud_map as tcm
import test_map_render as tmr
from dvo_slam_amd import _lib, tracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")
INF = float("inf")
HOLE = 0x7FC00000
FORMATS = ["bgr8", "rgb8", "bgra8", "rgba8"]

HOST_SOURCE = r"""
#include <cstddef>
#include <cstring>
#include <vector>
#include "cloud_colour.h"
#include "map_render.h"
using namespace dvo_hip;
extern "C" {
int colour_host_slot_bytes() { return int(sizeof(MapColourSlot)); }
uint32_t colour_host_pack(const uint8_t* px, int format) { return colour_pack(px, format); }
void colour_host_pack_plane(const uint8_t* src, size_t pitch, int w, int h, int format, uint32_t* dst) {
  const int channels = pixel_channels(format);
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) dst[size_t(v) * w + u] = colour_pack(src + size_t(v) * pitch + size_t(u) * channels, format);
}
// the colour plane of level `shift` (w x h) from the level-0 plane (rows of w0 dwords)
void colour_host_level(const uint32_t* plane, int w0, int shift, int w, int h, uint32_t* out) {
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) out[size_t(v) * w + u] = colour_level(plane, w0, u, v, shift);
}
uint32_t colour_host_mean(uint32_t s, uint32_t n) { return colour_mean(s, n); }
uint32_t colour_host_extract_one(uint32_t n, uint32_t sr, uint32_t sg, uint32_t sb) { return colour_extract(n, sr, sg, sb); }
void colour_host_clear(MapSlot* slots, MapColourSlot* colour, uint64_t capacity, uint64_t* counters) {
  for (uint64_t i = 0; i < capacity; ++i) {
    std::memset(&slots[i], 0, sizeof(MapSlot));
    std::memset(&colour[i], 0, sizeof(MapColourSlot));
    slots[i].key = kMapEmptyKey;
  }
  for (int i = 0; i < 8; ++i) counters[i] = 0;
}
// One frame into (sign +1) or out of (sign -1) the table, word by word as k_map_insert does it: {n, sx}, {sy, sz} and {sr, sg} as 64-bit
// two's-complement adds, si and sb as 32-bit ones.  counters: 0 usable points in range of the frames added, 1 dropped, 2 out of range,
// 3 unusable, 5 occupied slots, 6 points to remove, 7 of them unmatched.  The pixels in raster order, or (reverse != 0) last to first.
void colour_host_update(MapSlot* slots, MapColourSlot* colour, uint64_t capacity, uint64_t* counters, float leaf, const float* K, const double* T16,
                        int w, int h, const float* I, const float* Z, const uint32_t* plane0, int w0, int shift, float min_depth, float max_depth,
                        int sign, int reverse) {
  const MapPose pose = map_pose_prepare(T16);
  const bool minus = sign < 0;
  for (int k = 0; k < w * h; ++k) {
    const int i = reverse ? w * h - 1 - k : k;
    float P[3];
    uint64_t key;
    uint32_t q[4];
    if (!map_world_point(pose, K, i % w, i / w, Z[i], min_depth, max_depth, P)) { counters[3] += minus ? uint64_t(0) - 1 : 1; continue; }
    if (!map_key_of(P, I[i], leaf, &key, q)) { counters[2] += minus ? uint64_t(0) - 1 : 1; continue; }
    counters[minus ? 6 : 0] += 1;
    const uint32_t c = colour_level(plane0, w0, i % w, i / w, shift);
    uint64_t at = map_hash(key, capacity);
    bool placed = false;
    for (int p = 0; p < kMapMaxProbes && !placed; ++p, at = (at + 1) & (capacity - 1)) {
      MapSlot& s = slots[at];
      if (s.key == kMapEmptyKey) {
        if (minus) break;
        s.key = key;
        counters[5] += 1;
      }
      if (s.key != key) continue;
      uint64_t words[3];
      std::memcpy(words, &s.n, 16);
      std::memcpy(words + 2, &colour[at], 8);
      const uint64_t add[3] = {map_word(1u, q[0]), map_word(q[1], q[2]), colour_word(colour_r(c), colour_g(c))};
      for (int j = 0; j < 3; ++j) words[j] += minus ? map_negate(add[j]) : add[j];
      std::memcpy(&s.n, words, 16);
      std::memcpy(&colour[at], words + 2, 8);
      s.si += minus ? 0u - q[3] : q[3];
      colour[at].sb += minus ? 0u - colour_b(c) : colour_b(c);
      placed = true;
    }
    if (!placed) counters[minus ? 7 : 1] += 1;
  }
}
// live slots in table order; returns their number
uint64_t colour_host_extract(const MapSlot* slots, const MapColourSlot* colour, uint64_t capacity, float leaf, float* xyzi, uint32_t* rgba,
                             uint32_t* counts, uint64_t* keys) {
  uint64_t n = 0;
  for (uint64_t i = 0; i < capacity; ++i) {
    const MapSlot& s = slots[i];
    if (!map_slot_live(s.key, s.n)) continue;
    map_extract_voxel(s.key, s.n, s.sx, s.sy, s.sz, s.si, leaf, xyzi + 4 * n);
    rgba[n] = colour_extract(s.n, colour[i].sr, colour[i].sg, colour[i].sb);
    counts[n] = s.n;
    keys[n] = s.key;
    ++n;
  }
  return n;
}
// the colour views of the table: what k_map_render and k_render_resolve do in their COLOUR instantiations
void colour_host_render(const MapSlot* slots, const MapColourSlot* colour, uint64_t capacity, const RenderArgs* a, const float* K, int w, int h,
                        const double* poses, int n_views, uint32_t* rgba, uint32_t* Z) {
  for (int k = 0; k < n_views; ++k) {
    const MapView view = map_view_prepare(poses + 16 * k, K, w, h);
    std::vector<uint64_t> z(size_t(w) * h, kRenderEmpty);
    for (uint64_t j = 0; j < capacity; ++j) {
      const MapSlot& s = slots[j];
      RenderFootprint f;
      if (s.key == kMapEmptyKey || !map_render_voxel(view, *a, s.key, s.n, s.sx, s.sy, s.sz, s.si, &f)) continue;
      const uint64_t value = colour_render_value(f.value, colour_extract(s.n, colour[j].sr, colour[j].sg, colour[j].sb));
      for (int v = f.v0; v <= f.v1; ++v)
        for (int u = f.u0; u <= f.u1; ++u) {
          uint64_t& e = z[size_t(v) * w + u];
          if (value < e) e = value;
        }
    }
    for (size_t i = 0; i < z.size(); ++i) colour_render_resolve(z[i], rgba + size_t(k) * w * h + i, Z + size_t(k) * w * h + i);
  }
}
uint64_t colour_host_render_value(uint64_t grey, uint32_t rgba) { return colour_render_value(grey, rgba); }
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    """cloud_colour.h compiled for the host: g++, every warning an error, no contraction"""
    tmp = tempfile.mkdtemp(prefix="map_colour_host_")
    src, out = os.path.join(tmp, "map_colour_host.cpp"), os.path.join(tmp, "map_colour_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), src, "-o", out])
    L = C.CDLL(out)
    fp, dp, vp, u64, u32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p, C.c_uint64, C.c_uint32
    L.colour_host_pack.argtypes = [vp, C.c_int]
    L.colour_host_pack.restype = u32
    L.colour_host_pack_plane.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]
    L.colour_host_pack_plane.restype = None
    L.colour_host_level.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.colour_host_level.restype = None
    L.colour_host_mean.argtypes = [u32, u32]
    L.colour_host_mean.restype = u32
    L.colour_host_extract_one.argtypes = [u32, u32, u32, u32]
    L.colour_host_extract_one.restype = u32
    L.colour_host_clear.argtypes = [vp, vp, u64, vp]
    L.colour_host_clear.restype = None
    L.colour_host_update.argtypes = [vp, vp, u64, vp, C.c_float, fp, dp, C.c_int, C.c_int, fp, fp, vp, C.c_int, C.c_int, C.c_float, C.c_float,
                                     C.c_int, C.c_int]
    L.colour_host_update.restype = None
    L.colour_host_extract.argtypes = [vp, vp, u64, C.c_float, vp, vp, vp, vp]
    L.colour_host_extract.restype = u64
    L.colour_host_render.argtypes = [vp, vp, u64, C.POINTER(tmr.RenderArgs), fp, C.c_int, C.c_int, dp, C.c_int, vp, vp]
    L.colour_host_render.restype = None
    L.colour_host_render_value.argtypes = [u64, u32]
    L.colour_host_render_value.restype = u64
    assert L.colour_host_slot_bytes() == 16
    return L


def pack_plane(img, pixel_format):
    """the plane of packed pixels 0x00RRGGBB [h, w] uint32 of an [h, w, 3 | 4] uint8 image (rows may be padded), as cloud_colour.h packs it"""
    h, w, ch = img.shape
    assert img.dtype == np.uint8 and ch == _lib.PIXEL_CHANNELS[pixel_format] and img.strides[1:] == (ch, 1)
    out = np.empty((h, w), np.uint32)
    host_lib().colour_host_pack_plane(img.ctypes.data, img.strides[0], w, h, _lib.PIXEL_FORMATS[pixel_format], out.ctypes.data)
    return out


def level_colour(plane0, level):
    """the colour plane of a pyramid level [h0 >> level, w0 >> level] from the level-0 plane of packed pixels"""
    plane0 = np.ascontiguousarray(plane0, np.uint32)
    h0, w0 = plane0.shape
    out = np.empty((h0 >> level, w0 >> level), np.uint32)
    host_lib().colour_host_level(plane0.ctypes.data, w0, level, w0 >> level, h0 >> level, out.ctypes.data)
    return out


def level_colour_numpy(plane0, level):
    """the same in numpy integers: per channel (sum over the 2^L x 2^L block + 2^(2L - 1)) >> 2L"""
    h0, w0 = plane0.shape
    h, w, s = h0 >> level, w0 >> level, 1 << level
    out = np.zeros((h, w), np.uint32)
    for shift in (16, 8, 0):
        ch = ((plane0 >> shift) & 0xff).astype(np.int64)[:h * s, :w * s].reshape(h, s, w, s).sum(axis=(1, 3))
        mean = ch if level == 0 else (ch + (1 << (2 * level - 1))) >> (2 * level)
        out |= mean.astype(np.uint32) << shift
    return out


def random_image(w, h, channels, seed, pad=0):
    """an [h, w, channels] uint8 image with every byte random, rows padded by `pad` bytes"""
    rng = np.random.default_rng(seed)
    store = rng.integers(0, 256, (h, w * channels + pad), dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(store, (h, w, channels), (w * channels + pad, channels, 1))


class ColourHostMap:
    """the yardstick of a coloured map: cloud_map.h's table and cloud_colour.h's side table in host memory"""

    def __init__(self, leaf, capacity):
        self.leaf = float(np.float32(leaf))
        self.capacity = 64
        while self.capacity < capacity:
            self.capacity *= 2
        self.slots = np.empty(self.capacity * 32, np.uint8)
        self.colour = np.empty(self.capacity * 4, np.uint32)
        self.counters = np.zeros(8, np.uint64)
        host_lib().colour_host_clear(self.slots.ctypes.data, self.colour.ctypes.data, self.capacity, self.counters.ctypes.data)

    def update(self, I, Z, K, T, plane0, level=0, sign=1, min_depth=0.0, max_depth=INF, reverse=False):
        """the level's planes I, Z [h, w] with intrinsics K under pose T, coloured from the LEVEL-0 plane of packed pixels"""
        h, w = Z.shape
        plane0 = np.ascontiguousarray(plane0, np.uint32)
        assert plane0.shape[0] >> level == h and plane0.shape[1] >> level == w
        (ki, kp), (ti, tp), (ii, ip), (zi, zp) = tcm._f(K), tcm._d(T), tcm._f(I), tcm._f(Z)
        host_lib().colour_host_update(self.slots.ctypes.data, self.colour.ctypes.data, self.capacity, self.counters.ctypes.data, self.leaf, kp, tp, w, h,
                                      ip, zp, plane0.ctypes.data, plane0.shape[1], level, min_depth, max_depth, sign, 1 if reverse else 0)
        return self

    def insert(self, *args, **kw):
        return self.update(*args, sign=1, **kw)

    def remove(self, *args, **kw):
        return self.update(*args, sign=-1, **kw)

    def stats(self):
        c = [int(x) for x in self.counters]
        return dict(points=c[0] - c[1] - (c[6] - c[7]), dropped=c[1], out_of_range=c[2], unusable=c[3], occupied=c[5], removed=c[6] - c[7],
                    unmatched=c[7], capacity=self.capacity)

    def extract(self):
        """(xyzi, counts, keys, rgba) of the live voxels, sorted by key"""
        n = self.capacity
        xyzi, rgba, counts, keys = np.empty((n, 4), np.float32), np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint64)
        got = int(host_lib().colour_host_extract(self.slots.ctypes.data, self.colour.ctypes.data, self.capacity, self.leaf, xyzi.ctypes.data,
                                                 rgba.ctypes.data, counts.ctypes.data, keys.ctypes.data))
        order = np.argsort(keys[:got], kind="stable")
        return xyzi[:got][order], counts[:got][order], keys[:got][order], rgba[:got][order]

    def render(self, K, w, h, poses, **params):
        """(rgba [n, h, w] uint32, Z [n, h, w] float32) of the colour views"""
        K, T = tmr._views(K, poses)
        rgba, Z = np.empty((len(T), h, w), np.uint32), np.empty((len(T), h, w), np.float32)
        a = tmr._args(self.leaf, params)
        host_lib().colour_host_render(self.slots.ctypes.data, self.colour.ctypes.data, self.capacity, C.byref(a), K.ctypes.data_as(C.POINTER(C.c_float)),
                                      w, h, T.ctypes.data_as(C.POINTER(C.c_double)), len(T), rgba.ctypes.data, Z.ctypes.data)
        return rgba, Z

    def grey_table(self):
        """the slot table as a tests/test_cloud_map.py HostMap (what a grey map fed the same frames holds)"""
        m = tcm.HostMap(self.leaf, self.capacity)
        m.slots[:] = self.slots
        m.counters[:6] = [self.counters[0], self.counters[1], self.counters[2], self.counters[3], 0, self.counters[5]]
        return m


def assert_colour_maps_identical(a, b, what=""):
    """two sorted colour extractions (xyzi, counts, keys, rgba): identical bit for bit"""
    tcm.assert_maps_identical(a, b, what)
    assert np.array_equal(np.asarray(a[3]), np.asarray(b[3])), "%s: rgba differ" % (what,)


def scene_frames(w, h, n=2):
    """[(I, Z, T, plane0)] for n views of the (w, h) scene of tests/test_cloud_map.py with random colours, and K"""
    K, views = tcm.float_views(w, h)
    out = []
    for k in range(n):
        I, Z, T = views[k % 2]
        out.append((I, Z, T, pack_plane(random_image(w, h, 3, 40 + k), "bgr8")))
    return K, out


# ---- packing and the level mean -----------------------------------------------------------------------------------------------------------

def test_colour_pack_for_the_four_formats():
    L = host_lib()
    rng = np.random.default_rng(1)
    for _ in range(50):
        r, g, b, a = (int(x) for x in rng.integers(0, 256, 4))
        want = r << 16 | g << 8 | b
        for name, px in (("bgr8", [b, g, r]), ("rgb8", [r, g, b]), ("bgra8", [b, g, r, a]), ("rgba8", [r, g, b, a])):
            buf = np.array(px, np.uint8)
            assert L.colour_host_pack(buf.ctypes.data, _lib.PIXEL_FORMATS[name]) == want, (name, px)
    assert L.colour_host_pack(np.array([1, 2, 3, 255], np.uint8).ctypes.data, _lib.PIXEL_FORMATS["rgba8"]) == 0x00010203   # A = 0
    img = random_image(67, 5, 4, 2, pad=9)
    packed = pack_plane(img, "bgra8")
    assert np.array_equal(packed, img[..., 2].astype(np.uint32) << 16 | img[..., 1].astype(np.uint32) << 8 | img[..., 0])


@pytest.mark.parametrize("w,h", [(67, 5), (321, 240)])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_level_mean_equals_the_integer_restatement(w, h, level):
    plane0 = pack_plane(random_image(w, h, 3, 3), "rgb8")
    got, want = level_colour(plane0, level), level_colour_numpy(plane0, level)
    assert got.shape == (h >> level, w >> level) and np.array_equal(got, want)
    if level == 0:
        assert np.array_equal(got, plane0)
    # the top-right and bottom-right blocks, by hand: odd widths leave a column of level 0 unused, never read beyond
    s = 1 << level
    for v in (0, (h >> level) - 1):
        u = (w >> level) - 1
        block = plane0[v * s:(v + 1) * s, u * s:(u + 1) * s]
        assert block.shape == (s, s)
        chans = [int((((block >> sh) & 0xff).astype(np.int64).sum() + (s * s) // 2) // (s * s)) for sh in (16, 8, 0)]
        assert int(got[v, u]) == chans[0] << 16 | chans[1] << 8 | chans[2]


def test_level_mean_rounds_half_up_and_saturates_nowhere():
    plane = np.array([[0x000000, 0x010101], [0x000000, 0x010101]], np.uint32)          # sum 2 of 4: 0.5 -> 1
    assert level_colour(plane, 1)[0, 0] == 0x010101
    plane = np.array([[0x000000, 0x010101], [0x000000, 0x000000]], np.uint32)          # sum 1 of 4: 0.25 -> 0
    assert level_colour(plane, 1)[0, 0] == 0
    assert level_colour(np.full((4, 4), 0xffffff, np.uint32), 2)[0, 0] == 0xffffff      # 16 * 255: no carry between the channels
    assert level_colour(np.full((4, 4), 0xff00ff, np.uint32), 2)[0, 0] == 0xff00ff


# ---- extraction ---------------------------------------------------------------------------------------------------------------------------

def test_extraction_rounding():
    L = host_lib()
    for s in (0, 1, 17, 255):
        assert L.colour_host_mean(s, 1) == s                                             # n = 1: the pixel itself
    assert L.colour_host_mean(1, 3) == 0 and L.colour_host_mean(2, 3) == 1               # 1/3 -> 0, 2/3 -> 1
    assert L.colour_host_mean(1, 2) == 1 and L.colour_host_mean(3, 2) == 2               # halves go up
    n = 1 << 20
    assert L.colour_host_mean(255 * n, n) == 255 and L.colour_host_mean(255 * n - n // 2, n) == 255 and L.colour_host_mean(255 * n - n // 2 - 1, n) == 254
    assert L.colour_host_extract_one(n, 255 * n, 255 * n, 255 * n) == 0xFFFFFFFF
    assert L.colour_host_mean(0xFFFFFFFF, 1) == 255                                      # clamped (a wrapped sum never gives a channel above 255)
    assert L.colour_host_extract_one(3, 1, 2, 3 * 255) == 0xFF000000 | 0 << 16 | 1 << 8 | 255
    assert L.colour_host_render_value(0x3f80000012345678, 0xFFABCDEF) == 0x3f80000000ABCDEF


# ---- the map ------------------------------------------------------------------------------------------------------------------------------

def test_insert_then_remove_restores_the_side_table():
    K, frames = scene_frames(102, 78, 3)
    m = ColourHostMap(0.02, 1 << 16)
    for I, Z, T, plane in frames[:2]:
        m.insert(I, Z, K, T, plane)
    slots, colour = m.slots.copy(), m.colour.copy()
    before = m.extract()
    I, Z, T, plane = frames[2]
    T = T @ tcm.scenes.se3_exp([0.03, -0.02, 0.01, 0.01, -0.02, 0.015])
    m.insert(I, Z, K, T, plane)
    assert not np.array_equal(m.colour, colour) and len(m.extract()[2]) >= len(before[2])
    m.remove(I, Z, K, T, plane)
    s = m.stats()
    assert s["unmatched"] == 0 and s["removed"] > 1000
    assert np.array_equal(m.colour, colour)                                              # every word, vacant slots (zeros) included
    live = m.slots.view(np.uint32).reshape(-1, 8)[:, 2] > 0
    assert np.array_equal(m.slots.reshape(-1, 32)[live], slots.reshape(-1, 32)[live])
    assert_colour_maps_identical(m.extract(), before, "after the removal")
    # a removal with the wrong colour plane is NOT exact: the sums are what tell
    m.insert(I, Z, K, T, plane)
    m.remove(I, Z, K, T, plane ^ np.uint32(0x010101))
    assert not np.array_equal(m.colour, colour)


@pytest.mark.parametrize("level", [0, 1])
def test_the_result_does_not_depend_on_the_order(level):
    K, frames = scene_frames(102, 78, 2)
    Kl = np.array(K, np.float32) / np.float32(1 << level) if level else K
    fwd, rev = ColourHostMap(0.05, 1 << 14), ColourHostMap(0.05, 1 << 14)
    for I, Z, T, plane in frames:
        Il, Zl = I[::1 << level, ::1 << level][:78 >> level, :102 >> level], Z[::1 << level, ::1 << level][:78 >> level, :102 >> level]
        fwd.insert(np.ascontiguousarray(Il), np.ascontiguousarray(Zl), Kl, T, plane, level=level)
    for I, Z, T, plane in reversed(frames):
        Il, Zl = I[::1 << level, ::1 << level][:78 >> level, :102 >> level], Z[::1 << level, ::1 << level][:78 >> level, :102 >> level]
        rev.insert(np.ascontiguousarray(Il), np.ascontiguousarray(Zl), Kl, T, plane, level=level, reverse=True)
    a, b = fwd.extract(), rev.extract()
    assert len(a[2]) > 300 and (a[1] > 1).sum() > 50
    assert_colour_maps_identical(a, b, "forward against reversed")
    assert len(np.unique(a[3])) > 100 and np.all(a[3] >> 24 == 0xFF)
    # the grey sums are those of a grey map fed the same frames
    grey = tcm.HostMap(0.05, 1 << 14)
    for I, Z, T, plane in frames:
        Il, Zl = I[::1 << level, ::1 << level][:78 >> level, :102 >> level], Z[::1 << level, ::1 << level][:78 >> level, :102 >> level]
        grey.insert(np.ascontiguousarray(Il), np.ascontiguousarray(Zl), Kl, T)
    tcm.assert_maps_identical(a, grey.extract(), "the grey map")


def test_a_voxel_of_one_colour_has_that_colour_and_a_mixed_one_the_mean():
    w, h = 16, 8
    K = np.array([20.0, 20.0, 7.5, 3.5], np.float32)
    I, Z = np.full((h, w), 10.0, np.float32), np.full((h, w), 2.0, np.float32)
    m = ColourHostMap(8.0, 64)
    plane = np.full((h, w), 0x0a141e, np.uint32)
    plane[:, ::2] = 0x0b1520                                                              # half the pixels one step / two steps up
    T = np.eye(4)
    T[:3, 3] = [4.0, 4.0, 1.0]                                                            # all 128 points in one voxel
    m.insert(I, Z, K, T, plane)
    xyzi, counts, keys, rgba = m.extract()
    assert len(keys) == 1 and counts[0] == w * h
    assert rgba[0] == 0xFF000000 | 0x0b << 16 | 0x15 << 8 | 0x1f                          # 10.5 -> 11, 20.5 -> 21, 31


def test_colour_view_shares_the_depth_plane_and_marks_holes():
    K, frames = scene_frames(102, 78, 2)
    m = ColourHostMap(0.02, 1 << 16)
    for I, Z, T, plane in frames:
        m.insert(I, Z, K, T, plane)
    Kv = np.array([70.0, 70.0, 39.5, 29.5], np.float32)
    poses = np.stack([frames[0][2], frames[1][2]])
    for params in ({}, dict(max_splat=1)):
        rgba, Z = m.render(Kv, 80, 60, poses, **params)
        I_grey, Z_grey = tmr.render_host_map(m.grey_table(), Kv, 80, 60, poses, **params)
        assert np.array_equal(Z.view(np.uint32), Z_grey.view(np.uint32))
        hole = Z.view(np.uint32) == HOLE
        assert hole.any() and (~hole).sum() > 1000
        assert np.all(rgba[hole] == 0) and np.all(rgba[~hole] >> 24 == 0xFF)
        # a covered pixel shows the colour of some voxel of the map
        assert np.isin(rgba[~hole], m.extract()[3]).all()


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------------

CTX = "ctx"


class FakeCamera:
    def __init__(self, w, h):
        self.width, self.height = w, h


class FakePyr:
    """enough of a pyramid for the argument checks; a call that reached the library would fail on ctx"""

    def __init__(self, w=64, h=48, ctx=CTX):
        self.camera, self.ctx, self.ptr, self.levels = FakeCamera(w, h), ctx, None, 3


def test_set_colour_rejects_bad_arguments_before_the_library():
    p, img = FakePyr(), np.zeros((48, 64, 3), np.uint8)
    with pytest.raises(ValueError):
        d.set_colour_batch([p], [img], "yuv8")
    with pytest.raises(ValueError):
        d.set_colour_batch([p], [img], "grey8")
    with pytest.raises(ValueError):
        d.set_colour_batch([p], [np.zeros((48, 64, 4), np.uint8)], "bgr8")               # channels
    with pytest.raises(ValueError):
        d.set_colour_batch([p], [np.zeros((48, 63, 3), np.uint8)], "bgr8")               # shape
    with pytest.raises(TypeError):
        d.set_colour_batch([p], [np.zeros((48, 64, 3), np.float32)], "bgr8")
    with pytest.raises(ValueError):
        d.set_colour_batch([p], [0x7f0000000000], "bgr8", pitch=64 * 3 - 1)              # 0 < pitch < width * channels
    with pytest.raises(ValueError):
        d.set_colour_batch([p], [0x7f0000000000], "bgra8", pitch=64 * 3)
    with pytest.raises(TypeError):
        d.set_colour_batch([p], [0], "bgr8")                                             # a null address
    with pytest.raises(TypeError):
        d.set_colour_batch([p], [None], "bgr8")
    with pytest.raises(TypeError):
        d.set_colour_batch([p], [0x7f0000000000], "bgr8", pitch=1.5)
    with pytest.raises(ValueError):
        d.set_colour_batch([p], [img], "bgr8", pitch=256)                                # an array brings its own stride
    with pytest.raises(ValueError):
        d.set_colour_batch([p, p], [img, img], "bgr8")                                   # the same pyramid twice
    with pytest.raises(ValueError):
        d.set_colour_batch([p, FakePyr()], [img], "bgr8")                                # one plane per pyramid
    with pytest.raises(ValueError):
        d.set_colour_batch([], [], "bgr8")
    with pytest.raises(TypeError):
        d.set_colour_batch([p, FakePyr()], [img, 0x7f0000000000], "bgr8")                # arrays and addresses mixed
    with pytest.raises(ValueError):
        d.set_colour_batch([p, FakePyr(ctx="other")], [img, img], "bgr8")
    lensed = FakePyr()
    lensed._lens = ([1, 1, 0, 0], [0] * 8, True)
    with pytest.raises(ValueError):
        d.set_colour_batch([lensed], [img], "bgr8")
    # what passes: a padded view keeps its stride, mixed paddings go tight
    padded = random_image(64, 48, 3, 5, pad=16)
    fmt, row, on_device, addrs, keep, remember = tracker._colour_sources([p], [padded], "rgb8", 0)
    assert (fmt, row, on_device) == (_lib.PIXEL_FORMATS["rgb8"], 64 * 3 + 16, 0) and addrs == [padded.ctypes.data]
    assert remember[0].flags["C_CONTIGUOUS"] and np.array_equal(remember[0], padded)
    fmt, row, on_device, addrs, keep, remember = tracker._colour_sources([p, FakePyr()], [padded, img], "rgb8", 0)
    assert row == 0 and all(a.flags["C_CONTIGUOUS"] for a in keep)
    assert tracker._colour_sources([p], [0x7f0000000000], "bgra8", 512)[1:3] == (512, 1)


def test_pyramid_colour_rejects_bad_levels_and_missing_colour():
    p = FakePyr()
    for bad in (True, 1.0, "0"):
        with pytest.raises(TypeError):
            tracker.RgbdImagePyramid.colour(p, bad)
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            tracker.RgbdImagePyramid.colour(p, bad)
    with pytest.raises(ValueError):
        tracker.RgbdImagePyramid.colour(p, 0)                                            # no colour attached


def test_a_grey_map_asked_for_colour_refuses_before_the_library():
    m = object.__new__(d.KeyframeMap)
    m.coloured, m.ptr, m.ctx = False, None, None
    with pytest.raises(ValueError):
        m.extract(colour=True)
    with pytest.raises(ValueError):
        m.render_colour([60, 60, 31.5, 23.5], 64, 48, np.eye(4))
    with pytest.raises(TypeError):
        d.KeyframeMap(ctx="ctx", colour=1)
    coloured = object.__new__(d.KeyframeMap)
    coloured.coloured, coloured.ptr, coloured.ctx = True, None, CTX
    with pytest.raises(ValueError):
        coloured.insert([FakePyr()], np.eye(4)[None])                                    # a pyramid without colour
    with pytest.raises(ValueError):
        coloured.render_colour([60, 60, 31.5, 23.5], 64, 48, np.eye(4), max_splat=2)
    with pytest.raises(ValueError):
        coloured.render_colour([60, -60, 31.5, 23.5], 64, 48, np.eye(4))


def test_header_and_bindings_declare_the_colour_entry_points():
    text = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    for name in ("dvo_hip_frames_set_colour", "dvo_hip_frames_clear_colour", "dvo_hip_frame_download_colour", "dvo_hip_map_create_ex",
                 "dvo_hip_map_extract_colour", "dvo_hip_map_render_colour"):
        assert "int %s(dvo_hip_context* ctx" % name in text and name in _lib.EXPORTS
    assert "#define DVO_HIP_MAP_COLOUR 1u" in text and _lib.MAP_COLOUR == 1
    d.build()
    L = C.CDLL(d.LIB_PATH)
    for name in _lib.EXPORTS:
        assert hasattr(L, name), name


# ---- the C++ facade -----------------------------------------------------------------------------------------------------------------------

def build_map_colour_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "map_colour_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "map_colour_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_colour_classes_compile():
    d.build()
    assert os.path.exists(build_map_colour_facade_check())
