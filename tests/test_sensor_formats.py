"""CPU tier: the raw sensor formats' pieces that need no GPU.
  * dvo_slam_amd/csrc/sensor_formats.h (the conversion k_sensor_convert inlines) compiled for the host against its second statement in
    numpy (tests/sensor_formats.py): the four Bayer patterns at sizes down to 2 x 2 on noise and one-hot images, YUV 4:2:2 over all
    2^24 (Y, U, V) at both positions of a pixel pair in both byte orders; BGR, grey and packed colour, bit for bit;
  * the Python wrappers reject bad widths, channel counts, pitches, dtypes and names before anything reaches the library, and the three
    older format dicts are as they were;
  * include/dvo_hip.h declares the six formats and the C++ facade takes them (tests/cpp/sensor_facade_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dvo_slam_amd as d
import sensor_formats as sf
from dvo_slam_amd import _lib, tum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")

HOST_SOURCE = r"""
#include "sensor_formats.h"
using namespace dvo_hip;
extern "C" {
int sf_bytes(int format) { return sensor_bytes(format); }
// the w x h plane of `format` (rows of `pitch` bytes) -> BGR triples, grey bytes and packed pixels (each may be null)
void sf_convert(const uint8_t* plane, size_t pitch, int w, int h, int format, uint8_t* bgr, uint8_t* grey, uint32_t* packed) {
  const int rx = bayer_red_x(format), ry = bayer_red_y(format);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const SensorBgr c = sensor_is_bayer(format) ? bayer_pixel(plane, pitch, w, h, x, y, rx, ry) : yuv_at(plane, pitch, x, y, yuv_luma_first(format));
      const size_t at = size_t(y) * size_t(w) + size_t(x);
      if (bgr) {
        bgr[at * 3] = uint8_t(c.b);
        bgr[at * 3 + 1] = uint8_t(c.g);
        bgr[at * 3 + 2] = uint8_t(c.r);
      }
      if (grey) grey[at] = uint8_t(sensor_grey(c));
      if (packed) packed[at] = sensor_packed(c);
    }
}
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """sensor_formats.h behind two C functions, compiled by the host compiler"""
    tmp = tmp_path_factory.mktemp("sensor_formats")
    src = tmp / "sensor_host.cpp"
    src.write_text(HOST_SOURCE)
    lib = tmp / "libsensor_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(lib)])
    L = C.CDLL(str(lib))
    L.sf_bytes.argtypes, L.sf_bytes.restype = [C.c_int], C.c_int
    L.sf_convert.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sf_convert.restype = None
    return L


def convert(L, raw, fmt, pad=0, want=("bgr", "grey", "packed")):
    """the header's (bgr, grey, packed) of the sensor plane `raw`, read from rows `pad` bytes longer than tight"""
    h, w = raw.shape[:2]
    row = w * sf.channels(fmt)
    buf = np.full((h, row + pad), 0xA5, np.uint8)
    buf[:, :row] = raw.reshape(h, row)
    bgr = np.empty((h, w, 3), np.uint8) if "bgr" in want else None
    grey = np.empty((h, w), np.uint8) if "grey" in want else None
    packed = np.empty((h, w), np.uint32) if "packed" in want else None
    L.sf_convert(buf.ctypes.data, row + pad, w, h, _lib.SENSOR_PIXEL_FORMATS[fmt], *(a.ctypes.data if a is not None else None for a in (bgr, grey, packed)))
    return bgr, grey, packed


def assert_equals_numpy(L, raw, fmt, pad, what):
    bgr, grey, packed = convert(L, raw, fmt, pad)
    want = sf.to_bgr(raw, fmt)
    assert np.array_equal(bgr, want), what
    assert np.array_equal(grey, tum.bgr_to_grey(want)), what
    assert np.array_equal(packed, sf.packed(want)), what


BAYER_SIZES = [(2, 2), (3, 2), (2, 3), (5, 4), (17, 5), (64, 48)]      # (w, h)


@pytest.mark.parametrize("fmt", sf.BAYER)
def test_bayer_header_equals_the_numpy_statement(host, fmt):
    for k, (w, h) in enumerate(BAYER_SIZES):
        assert_equals_numpy(host, sf.noise((h, w), 10 + k), fmt, k % 3, (fmt, w, h, "noise"))
        assert_equals_numpy(host, np.full((h, w), 201, np.uint8), fmt, 0, (fmt, w, h, "constant"))
        for n, hot in enumerate(sf.one_hots(h, w)):
            assert_equals_numpy(host, hot, fmt, 0, (fmt, w, h, "one-hot", n))


def test_bayer_statement_by_hand():
    """the numpy statement itself on a case small enough to work out: RGGB, a single 255 at the red site (2, 2) of a 6 x 6 mosaic"""
    raw = np.zeros((6, 6), np.uint8)
    raw[2, 2] = 255
    bgr = sf.demosaic(raw, "bayer_rggb8")
    red = np.zeros((6, 6), np.uint8)
    red[2, 2] = 255
    red[2, 1] = red[2, 3] = red[1, 2] = red[3, 2] = 128          # green sites beside / above it: (255 + 0 + 1) >> 1
    red[1, 1] = red[1, 3] = red[3, 1] = red[3, 3] = 64           # blue sites diagonal to it: (255 + 2) >> 2
    assert np.array_equal(bgr[:, :, 2], red)
    assert not bgr[:, :, 0].any() and not bgr[:, :, 1].any()
    # a constant image stays constant in every channel, borders included; the four patterns are the same mosaic shifted by a site
    flat = sf.demosaic(np.full((5, 7), 93, np.uint8), "bayer_gbrg8")
    assert (flat == 93).all()
    noise = sf.noise((9, 11), 3)
    assert np.array_equal(sf.demosaic(noise, "bayer_rggb8")[1:-1, 2:-1], sf.demosaic(noise[:, 1:], "bayer_grbg8")[1:-1, 1:-1])
    assert np.array_equal(sf.demosaic(noise, "bayer_rggb8")[2:-1, 1:-1], sf.demosaic(noise[1:], "bayer_gbrg8")[1:-1, 1:-1])
    assert np.array_equal(sf.demosaic(noise, "bayer_rggb8")[..., ::-1], sf.demosaic(noise, "bayer_bggr8"))


def test_yuv_header_over_every_value_equals_the_numpy_statement(host):
    want = sf.every_yuv_bgr()
    # black, white, mid grey, and saturation at both ends, worked out from the definition
    for (y, u, v), bgr in (((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((126, 128, 128), (128, 128, 128)),
                           ((255, 255, 255), (255, 125, 255)), ((0, 0, 0), (0, 154, 0))):
        assert tuple(want[v * 16 + u // 16, (u % 16 * 256 + y) * 2]) == bgr, (y, u, v)
    grey_want = tum.bgr_to_grey(want)
    for fmt in sf.YUV:
        bgr, grey, _ = convert(host, sf.every_yuv(fmt), fmt, want=("bgr", "grey"))
        assert np.array_equal(bgr, want), fmt
        assert np.array_equal(grey, grey_want), fmt
    # the numpy statement's own byte orders agree on a plane it does not share with the exhaustive case, at an odd row pitch
    raw = sf.noise((6, 10, 2), 5)
    swapped = np.ascontiguousarray(raw[:, :, ::-1])
    assert np.array_equal(sf.yuv422_to_bgr(raw, "yuyv8"), sf.yuv422_to_bgr(swapped, "uyvy8"))
    for fmt, plane in (("yuyv8", raw), ("uyvy8", swapped)):
        assert_equals_numpy(host, plane, fmt, 3, fmt)


def test_header_knows_its_formats(host):
    assert [host.sf_bytes(v) for v in range(0, 24)] == [0] * 16 + [1, 1, 1, 1, 2, 2, 0, 0]
    text = open(os.path.join(ROOT, "include", "dvo_hip.h")).read()
    for name, value in (("BAYER_RGGB8", 16), ("BAYER_BGGR8", 17), ("BAYER_GBRG8", 18), ("BAYER_GRBG8", 19), ("YUYV8", 20), ("UYVY8", 21)):
        assert any(line.split()[:3] == ["#define", "DVO_HIP_PIXEL_" + name, str(value)] for line in text.splitlines()), name
    assert '"sensor_ingests"' in text


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------

class _NoLibrary:
    """stands in for a context: any use of the library is a test failure"""
    ptr = None

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _camera(w=32, h=24):
    return d.RgbdCameraPyramid(w, h, np.array([30.0, 30.0, 15.5, 11.5], np.float32), ctx=_NoLibrary())


class _Pyramid:
    def __init__(self, cam):
        self.camera, self.ctx, self.ptr = cam, cam.ctx, None


def test_format_tables():
    assert _lib.SENSOR_PIXEL_FORMATS == {"bayer_rggb8": 16, "bayer_bggr8": 17, "bayer_gbrg8": 18, "bayer_grbg8": 19, "yuyv8": 20, "uyvy8": 21}
    assert [_lib.SENSOR_PIXEL_CHANNELS[k] for k in sorted(_lib.SENSOR_PIXEL_FORMATS, key=_lib.SENSOR_PIXEL_FORMATS.get)] == [1, 1, 1, 1, 2, 2]
    assert _lib.PIXEL_FORMATS == {"bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4}
    assert _lib.PIXEL_CHANNELS == {"bgr8": 3, "rgb8": 3, "bgra8": 4, "rgba8": 4}
    assert _lib.MIXED_PIXEL_FORMATS == {"bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4, "grey8": 0}


def test_create_colour_rejects_bad_sensor_arguments_before_the_library():
    cam = _camera()
    depth = np.zeros((24, 32), np.uint16)
    bayer, yuv = np.zeros((24, 32), np.uint8), np.zeros((24, 32, 2), np.uint8)
    for name in ("yuv", "argb", "BGR8", "bayer", "bayer_rggb", "YUYV8", "yuv422", 16, None):
        with pytest.raises(ValueError):
            cam.create_colour(bayer, depth, name)
    with pytest.raises(ValueError):
        cam.create_colour(yuv, depth, "bayer_grbg8")                   # 2 channels for a mosaic
    with pytest.raises(ValueError):
        cam.create_colour(bayer, depth, "yuyv8")                       # a flat plane for YUV
    with pytest.raises(ValueError):
        cam.create_colour(np.zeros((24, 32, 3), np.uint8), depth, "uyvy8")
    with pytest.raises(ValueError):
        cam.create_colour(np.zeros((24, 31), np.uint8), depth, "bayer_rggb8")
    with pytest.raises(TypeError):
        cam.create_colour(bayer.astype(np.uint16), depth, "bayer_bggr8")
    with pytest.raises(TypeError):
        cam.create_colour(yuv.astype(np.int8), depth, "yuyv8")
    with pytest.raises(ValueError):
        cam.create_colour_device(0x1000, "bayer_gbrg8", 31, 0x2000)    # pitch below width * 1
    with pytest.raises(ValueError):
        cam.create_colour_device(0x1000, "uyvy8", 63, 0x2000)          # pitch below width * 2
    odd = _camera(31, 24)
    with pytest.raises(ValueError):
        odd.create_colour(np.zeros((24, 31, 2), np.uint8), np.zeros((24, 31), np.uint16), "yuyv8")     # an odd YUV width
    with pytest.raises(ValueError):
        odd.create_colour_device(0x1000, "uyvy8", 0, 0x2000)
    thin = _camera(1, 24)
    with pytest.raises(ValueError):
        thin.create_colour(np.zeros((24, 1), np.uint8), np.zeros((24, 1), np.uint16), "bayer_rggb8")   # a 1-wide mosaic
    with pytest.raises(ValueError):
        thin.create_colour_device(0x1000, "bayer_grbg8", 0, 0x2000)
    with pytest.raises(ValueError):
        _camera(32, 1).create_colour_device(0x1000, "bayer_grbg8", 0, 0x2000)


def test_batch_wrappers_reject_bad_sensor_arguments_before_the_library():
    cam = _camera()
    pyrs = [_Pyramid(cam), _Pyramid(cam)]
    depth = [np.zeros((24, 32), np.uint16)] * 2
    bayer, yuv = [np.zeros((24, 32), np.uint8)] * 2, [np.zeros((24, 32, 2), np.uint8)] * 2
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, bayer, depth, "bayer")
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, yuv, depth, "bayer_rggb8")    # 2 channels for a mosaic
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, bayer, depth, "uyvy8")
    with pytest.raises(TypeError):
        d.update_colour_host_batch(pyrs, [a.astype(np.int8) for a in yuv], depth, "yuyv8")
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "yuyv", 0)
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "yuyv8", 63)       # < 32 * 2
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "bayer_bggr8", 31)
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "bayer_bggr8", 31, depth_format="f32")
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [1, 2], [3, 4], "grey16", 0, depth_format="f32")
    odd = _camera(31, 24)
    opyrs = [_Pyramid(odd)]
    with pytest.raises(ValueError):
        d.update_colour_device_batch(opyrs, [1], [3], "yuyv8", 0)
    with pytest.raises(ValueError):
        d.update_colour_device_batch(opyrs, [1], [3], "uyvy8", 0, depth_format="f32")
    with pytest.raises(ValueError):
        d.update_colour_host_batch(opyrs, [np.zeros((24, 31, 2), np.uint8)], [np.zeros((24, 31), np.uint16)], "uyvy8")
    with pytest.raises(ValueError):
        d.update_colour_device_batch([_Pyramid(_camera(1, 24))], [1], [3], "bayer_rggb8", 0)
    # set_colour
    with pytest.raises(ValueError):
        d.set_colour_batch(pyrs, yuv, "bayer_grbg8")
    with pytest.raises(ValueError):
        d.set_colour_batch(pyrs, bayer, "yuyv8")
    with pytest.raises(TypeError):
        d.set_colour_batch(pyrs, [a.astype(np.uint16) for a in bayer], "bayer_grbg8")
    with pytest.raises(ValueError):
        d.set_colour_batch(pyrs, [0x1000, 0x2000], "uyvy8", 63)
    with pytest.raises(ValueError):
        d.set_colour_batch(opyrs, [0x1000], "yuyv8", 0)
    with pytest.raises(ValueError):
        d.set_colour_batch(pyrs, [0x1000, 0x2000], "yuv8", 0)


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------

def build_sensor_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "sensor_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "sensor_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_takes_the_sensor_formats():
    d.build()
    assert os.path.exists(build_sensor_facade_check())
