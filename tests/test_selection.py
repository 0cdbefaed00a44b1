"""CPU tier of the caller selection of reference points (include/dvo_hip.h, dvo_hip_frames_set_selection).
  * dvo_slam_amd/csrc/selection.h (the per-pixel rule the apply pass inlines) compiled for the host and run over random selections,
    masks, pitches and depth ranges at every pyramid level: equal to the rule restated in numpy;
  * the Python wrappers reject bad masks before anything reaches the library;
  * the C++ facade compiles with a caller-defined PointSelectionPredicate (tests/cpp/selection_check.cpp, -fsyntax-only)."""
import os
import subprocess

import numpy as np
import pytest

import dvo_slam_amd as d
from dvo_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")

APPLY_ALL = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "selection.h"
using namespace dvo_hip;
// argv: in-file out-file w0 h0 pitch level wl hl min max.  in: pitch*h0 mask bytes, then wl*hl float depths (NaN = not selected)
int main(int argc, char** argv) {
  const int w0 = std::atoi(argv[3]), h0 = std::atoi(argv[4]), pitch = std::atoi(argv[5]), level = std::atoi(argv[6]);
  const int wl = std::atoi(argv[7]), hl = std::atoi(argv[8]);
  const float zmin = std::strtof(argv[9], nullptr), zmax = std::strtof(argv[10], nullptr);
  (void)w0;
  std::vector<unsigned char> mask(size_t(pitch) * h0), keep(size_t(wl) * hl);
  std::vector<float> z(size_t(wl) * hl);
  FILE* f = std::fopen(argv[1], "rb");
  if (std::fread(mask.data(), 1, mask.size(), f) != mask.size() || std::fread(z.data(), 4, z.size(), f) != z.size()) return 2;
  std::fclose(f);
  const bool use_mask = mask[0] != 2;                      // (first byte 2: run without a mask)
  const bool on = selection_range_on(zmin, zmax);
  for (int y = 0; y < hl; ++y)
    for (int x = 0; x < wl; ++x) {
      const float zz = z[size_t(y) * wl + x];
      keep[size_t(y) * wl + x] = zz == zz && selection_keeps(use_mask ? mask.data() : nullptr, size_t(pitch), level, x, y, zz, on, zmin, zmax);
    }
  f = std::fopen(argv[2], "wb");
  std::fwrite(keep.data(), 1, keep.size(), f);
  std::fclose(f);
  std::printf("%d %d %d\n", int(selection_range_on(0.0f, INFINITY)), int(selection_range_on(0.5f, INFINITY)), int(selection_range_on(0.0f, 4.0f)));
  return 0;
}
"""


@pytest.fixture(scope="module")
def apply_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("selection")
    src = tmp / "apply_all.cpp"
    src.write_text(APPLY_ALL)
    exe = tmp / "apply_all"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    return exe


def numpy_rule(mask0, z, level, zmin, zmax):
    hl, wl = z.shape
    keep = np.isfinite(z)
    if mask0 is not None:
        keep &= mask0[::2 ** level, ::2 ** level][:hl, :wl] != 0
    if zmin > 0 or np.isfinite(zmax):
        with np.errstate(invalid="ignore"):
            keep &= (z >= zmin) & (z <= zmax)
    return keep


@pytest.mark.parametrize("w0,h0", [(640, 480), (322, 242), (41, 29)])
def test_rule_header_equals_numpy(apply_exe, tmp_path, w0, h0):
    rng = np.random.default_rng(w0)
    for level in range(4):
        wl, hl = w0, h0
        for _ in range(level):
            wl, hl = wl // 2, hl // 2
        for trial, (zmin, zmax) in enumerate(((0.0, np.inf), (0.8, 2.5), (0.0, 1.5), (2.0, np.inf), (1.0, 1.0))):
            pitch = w0 + int(rng.integers(0, 40)) * (trial % 2)
            mask = (rng.random((h0, pitch)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (h0, pitch)).astype(np.uint8)
            use_mask = trial != 4
            if not use_mask:
                mask[0, 0] = 2
            else:
                mask[0, 0] = 1 if mask[0, 0] == 2 else mask[0, 0]
            z = rng.uniform(0.3, 4.0, (hl, wl)).astype(np.float32)
            z[rng.random((hl, wl)) < 0.3] = np.nan
            z[0, :min(wl, 3)] = np.float32(zmin) if zmin > 0 else z[0, :min(wl, 3)]      # the bounds themselves are inside
            inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
            with open(inp, "wb") as f:
                f.write(mask.tobytes())
                f.write(z.tobytes())
            got = subprocess.check_output([str(apply_exe), str(inp), str(out), str(w0), str(h0), str(pitch), str(level), str(wl), str(hl),
                                           repr(float(zmin)), repr(float(zmax))], text=True)
            assert got.split() == ["0", "1", "1"]
            keep = np.fromfile(str(out), np.uint8).reshape(hl, wl) != 0
            want = numpy_rule(mask[:, :w0] if use_mask else None, z, level, zmin, zmax)
            assert np.array_equal(keep, want), (w0, h0, level, zmin, zmax)


def test_python_wrappers_reject_bad_masks():
    class FakeCam:
        width, height = 64, 48

    class FakePyr:
        camera = FakeCam()
        ctx = None
    with pytest.raises(ValueError):
        d.set_selection_batch([FakePyr()], [np.ones((48, 64), np.uint8), np.ones((48, 64), np.uint8)])
    with pytest.raises(ValueError):
        d.set_selection_batch([FakePyr()], [np.ones((48, 63), np.uint8)])
    with pytest.raises(ValueError):
        d.set_selection_batch([FakePyr()], [np.ones((48, 64), np.float32)])
    with pytest.raises(ValueError):
        d.set_selection_batch([FakePyr(), FakePyr()], [np.ones((48, 64), np.uint8), 12345])


def test_selection_entry_points_are_exported():
    for name in ("dvo_hip_frames_set_selection", "dvo_hip_frames_clear_selection", "dvo_hip_frame_set_level_selection"):
        assert name in _lib.EXPORTS


def test_facade_compiles_with_a_custom_predicate():
    src = os.path.join(ROOT, "tests", "cpp", "selection_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src])
