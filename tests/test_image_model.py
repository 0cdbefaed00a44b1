"""CPU tier of the image data model (dvo_slam_amd/csrc/image_model.h): the per-pixel arithmetic every frame-build kernel inlines -- the
clamped central differences, the selection predicate, the 2 x 2 mean and the depth subsample -- compiled for the host (g++ -Werror,
-ffp-contract=off: what the header's pragmas say to clang) and run over one pyramid level.  The derivative planes, the selection mask and
count and the next level's I / Z equal the oracle's bit for bit, NaN positions included: no tolerance."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common as cm
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")

HOST_SOURCE = r"""
#include <cstddef>
#include <cstdint>
#include "image_model.h"
using namespace dvo_hip;
// one level (w x h planes I, Z): its four derivative planes, the selection mask and count, and the next level's planes I1, Z1
extern "C" int image_model_level(const float* I, const float* Z, int w, int h, float ithr, float dthr, float* idx, float* idy, float* zdx,
                                 float* zdy, uint8_t* mask, float* I1, float* Z1) {
  auto at = [&](int x, int y) { return make_float2(I[size_t(y) * w + x], Z[size_t(y) * w + x]); };
  int count = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const Derivs d = derive_at(at, w, h, x, y);
      const size_t i = size_t(y) * w + x;
      idx[i] = d.idx; idy[i] = d.idy; zdx[i] = d.zdx; zdy[i] = d.zdy;
      mask[i] = selects(d.z0, d.idx, d.idy, d.zdx, d.zdy, ithr, dthr) ? 1 : 0;
      count += mask[i];
    }
  const int w1 = w / 2, h1 = h / 2;
  for (int y = 0; y < h1; ++y)
    for (int x = 0; x < w1; ++x) {
      const float2 a = at(2 * x, 2 * y), b = at(2 * x + 1, 2 * y), c = at(2 * x, 2 * y + 1), d = at(2 * x + 1, 2 * y + 1);
      I1[size_t(y) * w1 + x] = mean_2x2(a.x, b.x, c.x, d.x);
      Z1[size_t(y) * w1 + x] = depth_subsample(a.y);
    }
  return count;
}
"""


@functools.lru_cache(maxsize=None)
def host_lib():
    tmp = tempfile.mkdtemp(prefix="image_model_")
    src, out = os.path.join(tmp, "image_model_host.cpp"), os.path.join(tmp, "image_model_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, src, "-o", out])
    L = C.CDLL(out)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    L.image_model_level.argtypes = [fp, fp, C.c_int, C.c_int, C.c_float, C.c_float, fp, fp, fp, fp, bp, fp, fp]
    L.image_model_level.restype = C.c_int
    return L


@functools.lru_cache(maxsize=None)
def level0_and_oracle(w, h):
    """A synthetic frame with depth holes -- a corner, a border pixel, the opposite corner and one inside, beside the scene's own -- as the
    float planes of level 0, and the oracle's two-level pyramid over them."""
    pair = cm.synth(29, w, h)
    raw = pair["depth_ref"].copy()
    raw[0, 0] = 0
    raw[h // 2, 0] = 0
    raw[h - 1, w - 1] = 0
    raw[h // 2, w // 2] = 0
    I = np.ascontiguousarray(pair["grey_ref"], np.float32)
    Z = po.convert_raw_depth(raw)
    assert np.isnan(Z[0, 0]) and np.isnan(Z[h // 2, 0]) and np.isnan(Z[h - 1, w - 1]) and np.isfinite(Z).any()
    return I, Z, po.Pyramid(I, Z, pair["K"], 2)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


@pytest.mark.parametrize("ithr,dthr", [(0.0, 0.0), (5.0, 0.02)])
@pytest.mark.parametrize("w,h", [(5, 4), (7, 9), (65, 17), (130, 34)])
def test_header_equals_the_oracle_bit_for_bit(w, h, ithr, dthr):
    I, Z, oracle = level0_and_oracle(w, h)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    planes = [np.empty((h, w), np.float32) for _ in range(4)]
    mask = np.empty((h, w), np.uint8)
    I1, Z1 = np.empty((h // 2, w // 2), np.float32), np.empty((h // 2, w // 2), np.float32)
    count = host_lib().image_model_level(I.ctypes.data_as(fp), Z.ctypes.data_as(fp), w, h, ithr, dthr, *[p.ctypes.data_as(fp) for p in planes],
                                         mask.ctypes.data_as(bp), I1.ctypes.data_as(fp), Z1.ctypes.data_as(fp))
    for k, (name, got) in enumerate(zip(("intensity_dx", "intensity_dy", "depth_dx", "depth_dy"), planes)):
        assert same_bits(got, oracle.plane(0, 2 + k)[0]), name
    want_count, want_mask = oracle.select(0, ithr, dthr)
    assert count == want_count and np.array_equal(mask, want_mask)
    assert 0 < count < w * h                                         # the holes and their neighbours are out, the rest not all
    assert same_bits(I1, oracle.plane(1, 0)[0])
    assert same_bits(Z1, oracle.plane(1, 1)[0])
