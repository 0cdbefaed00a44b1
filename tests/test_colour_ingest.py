"""CPU tier: the colour ingest's pieces that need no GPU.
  * dvo_slam_amd/csrc/colour.h (the conversion the ingest kernels inline) compiled for the host over all 2^24 (B, G, R) triples, in
    both channel orders: equal to tum.bgr_to_grey, the oracle's bgr_to_grey and the facade's greyFromRgb8 (OpenCV's CV_BGR2GRAY);
  * the Python wrappers reject bad shapes, dtypes, format names and pitches before anything reaches the library;
  * the C++ facade's RgbdCameraPyramid::createFromColour compiles (tests/cpp/colour_facade_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import dvo_slam_amd as d
from dvo_slam_amd import _lib, tum
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")

CONVERT_ALL = r"""
#include <cstdio>
#include <vector>
#include "colour.h"
#include "dvo_benchmark/image_io.h"
using namespace dvo_hip;
int main(int argc, char** argv) {
  // index b << 16 | g << 8 | r: grey of the BGR-ordered pixel, of the RGB-ordered pixel with the same colour, greyFromRgb8
  std::vector<unsigned char> bgr(1u << 24), rgb(1u << 24), ref(1u << 24);
  const GreyWeights wb = grey_weights(pixel_red_first(DVO_HIP_PIXEL_BGR8)), wr = grey_weights(pixel_red_first(DVO_HIP_PIXEL_RGBA8));
  for (unsigned i = 0; i < (1u << 24); ++i) {
    const unsigned b = i >> 16, g = i >> 8 & 255u, r = i & 255u;
    bgr[i] = (unsigned char)grey_of(b, g, r, wb);
    const unsigned long long bits = (unsigned long long)(r | g << 8 | b << 16) << 8;   // an RGB pixel at byte 1 of a word
    rgb[i] = (unsigned char)grey_at_bits(bits, 8, wr);
    ref[i] = dvo_benchmark::greyFromRgb8(r, g, b);
  }
  FILE* f = std::fopen(argv[1], "wb");
  std::fwrite(bgr.data(), 1, bgr.size(), f);
  std::fwrite(rgb.data(), 1, rgb.size(), f);
  std::fwrite(ref.data(), 1, ref.size(), f);
  std::fclose(f);
  std::printf("%d %d %d %d\n", pixel_channels(DVO_HIP_PIXEL_BGR8), pixel_channels(DVO_HIP_PIXEL_RGB8), pixel_channels(DVO_HIP_PIXEL_BGRA8),
              pixel_channels(DVO_HIP_PIXEL_RGBA8) * 10 + pixel_channels(0) + pixel_channels(5));
  return 0;
}
"""


def test_conversion_header_over_every_colour_equals_the_cpu_formulas(tmp_path):
    src = tmp_path / "convert_all.cpp"
    src.write_text(CONVERT_ALL)
    exe = tmp_path / "convert_all"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-lz"])
    out = tmp_path / "grey.bin"
    assert subprocess.check_output([str(exe), str(out)], text=True).split() == ["3", "3", "4", "40"]
    got = np.fromfile(str(out), np.uint8).reshape(3, 1 << 24)
    i = np.arange(1 << 24, dtype=np.uint32)
    bgr = np.stack([(i >> 16).astype(np.uint8), (i >> 8 & 255).astype(np.uint8), (i & 255).astype(np.uint8)], axis=-1)
    want = tum.bgr_to_grey(bgr)
    assert np.array_equal(got[0], want)                   # BGR order
    assert np.array_equal(got[1], want)                   # RGB order, the same colours
    assert np.array_equal(got[2], want)                   # greyFromRgb8 (include/dvo_benchmark/image_io.h)
    assert np.array_equal(po.bgr_to_grey(bgr), want.astype(np.float32))


class _NoLibrary:
    """stands in for a context: any use of the library is a test failure"""
    ptr = None

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _camera(w=32, h=24):
    return d.RgbdCameraPyramid(w, h, np.array([30.0, 30.0, 15.5, 11.5], np.float32), ctx=_NoLibrary())


def test_create_colour_rejects_bad_arguments_before_the_library():
    cam = _camera()
    depth = np.zeros((24, 32), np.uint16)
    good = np.zeros((24, 32, 3), np.uint8)
    with pytest.raises(ValueError):
        cam.create_colour(good, depth, "yuv")
    with pytest.raises(ValueError):
        cam.create_colour(good, depth, "BGR8")
    with pytest.raises(ValueError):
        cam.create_colour(good, depth, "bgra8")                       # 3 channels for a 4-byte format
    with pytest.raises(ValueError):
        cam.create_colour(np.zeros((24, 32, 4), np.uint8), depth, "rgb8")
    with pytest.raises(ValueError):
        cam.create_colour(np.zeros((24, 31, 3), np.uint8), depth, "bgr8")
    with pytest.raises(ValueError):
        cam.create_colour(np.zeros((24, 32), np.uint8), depth, "bgr8")  # a grey plane
    with pytest.raises(TypeError):
        cam.create_colour(good.astype(np.uint16), depth, "bgr8")
    with pytest.raises(TypeError):
        cam.create_colour(good, depth.astype(np.float32), "bgr8")
    with pytest.raises(ValueError):
        cam.create_colour(good, np.zeros((24, 33), np.uint16), "bgr8")
    with pytest.raises(ValueError):
        cam.create_colour_device(0x1000, "argb", 0, 0x2000)
    with pytest.raises(ValueError):
        cam.create_colour_device(0x1000, "rgba8", 32 * 4 - 1, 0x2000)  # pitch below width * channels


class _Pyramid:
    def __init__(self, cam):
        self.camera, self.ctx, self.ptr = cam, cam.ctx, None


def test_batch_wrappers_reject_bad_arguments_before_the_library():
    cam = _camera()
    pyrs = [_Pyramid(cam), _Pyramid(cam)]
    depth = [np.zeros((24, 32), np.uint16)] * 2
    colour = [np.zeros((24, 32, 4), np.uint8)] * 2
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, colour, depth, "bgr")
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, colour, depth, "bgr8")        # 4 channels for a 3-byte format
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, colour[:1], depth, "rgba8")
    with pytest.raises(TypeError):
        d.update_colour_host_batch(pyrs, [c.astype(np.int8) for c in colour], depth, "rgba8")
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, colour, depth, "rgba8", role="previous", config=d.Config())
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "rgb", 0)
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "rgb8", 95)  # < 32 * 3
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1], [3, 4], "rgb8", 0)
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "rgb8", 0, role="current")   # a role needs a config
    assert _lib.PIXEL_FORMATS == {"bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4}


def test_header_declares_the_pixel_formats():
    text = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    for name, value in (("BGR8", 1), ("RGB8", 2), ("BGRA8", 3), ("RGBA8", 4)):
        assert "#define DVO_HIP_PIXEL_%s %d" % (name, value) in text


def build_colour_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "colour_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "colour_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_colour_method_compiles():
    d.build()
    assert os.path.exists(build_colour_facade_check())
