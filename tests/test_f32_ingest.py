"""CPU tier: the float-plane ingest's pieces that need no GPU.
  * the library exports every new entry point, the header declares them and the formats, and the ctypes prototypes carry as many
    arguments as the header's declarations;
  * the Python wrappers reject bad shapes, dtypes, strides, format names and role / config mismatches before anything reaches the library;
  * dvo_slam_amd/csrc/colour.h's float-depth rule (depth_of_f32: z * scale, one rounding, NaN kept, everything else as it is), compiled
    for the host, equals numpy on a plane with the special values;
  * the C++ facade's RgbdImagePyramid::update / RgbdCameraPyramid::createFromFloatDevice compile (tests/cpp/f32_facade_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dvo_slam_amd as d
from dvo_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")

NEW_SYMBOLS = ["dvo_hip_frame_create_f32_device", "dvo_hip_frames_update_f32_device_as_ex", "dvo_hip_frames_update_f32_as_ex",
               "dvo_hip_frames_update_colour_f32depth_device_as_ex", "dvo_hip_frames_update_colour_f32depth_as_ex"]


def _header():
    return open(os.path.join(ROOT, "include", "dvo_hip.h")).read()


def test_library_exports_the_float_entry_points():
    d.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), name


def test_ctypes_prototypes_match_the_header():
    d.build()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint %s\((.*?)\);" % name, text, flags=re.S)
        assert m, "%s is not declared in include/dvo_hip.h" % name
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")), name


def test_header_declares_the_formats_and_documents_the_counter():
    text = _header()
    for line in ("#define DVO_HIP_PIXEL_GREY8 0", "#define DVO_HIP_PIXEL_F32 5", "#define DVO_HIP_DEPTH_U16 0", "#define DVO_HIP_DEPTH_F32 1"):
        assert line in text
    assert '"f32_ingests"' in text
    assert _lib.PIXEL_F32 == 5 and _lib.DEPTH_FORMATS == {"u16": 0, "f32": 1}
    assert _lib.MIXED_PIXEL_FORMATS == {"grey8": 0, "bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4}
    assert _lib.PIXEL_FORMATS == {"bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4}      # the colour entry points still refuse grey8


class _NoLibrary:
    """stands in for a context: any use of the library is a test failure"""
    ptr = None

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


class _Pyramid:
    def __init__(self, cam):
        self.camera, self.ctx, self.ptr = cam, cam.ctx, None


def _camera(w=32, h=24):
    return d.RgbdCameraPyramid(w, h, np.array([30.0, 30.0, 15.5, 11.5], np.float32), ctx=_NoLibrary())


def test_create_f32_device_rejects_bad_addresses_before_the_library():
    cam = _camera()
    with pytest.raises(ValueError):
        cam.create_f32_device(0, 0x2000)
    with pytest.raises(ValueError):
        cam.create_f32_device(0x1000, None)
    with pytest.raises(ValueError):
        cam.create_f32_device(0x1002, 0x2000)                              # a float plane is 4-byte aligned
    with pytest.raises(ValueError):
        cam.create_f32_device(np.zeros((24, 32), np.float32), 0x2000)      # an array is no device address


def test_f32_batch_wrappers_reject_bad_arguments_before_the_library():
    cam = _camera()
    pyrs = [_Pyramid(cam), _Pyramid(cam)]
    good = [np.zeros((24, 32), np.float32), np.zeros((24, 32), np.float32)]
    padded = [np.zeros((24, 40), np.float32)[:, :32] for _ in range(2)]
    cfg = d.Config()
    # host planes
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, good[:1], good)
    with pytest.raises(TypeError):
        d.update_f32_host_batch(pyrs, [a.astype(np.float64) for a in good], good)
    with pytest.raises(TypeError):
        d.update_f32_host_batch(pyrs, good, [a.astype(np.uint16) for a in good])
    with pytest.raises(TypeError):
        d.update_f32_host_batch(pyrs, good, [a.tolist() for a in good])
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, [np.zeros((24, 31), np.float32)] * 2, good)
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, [np.zeros((24, 32, 1), np.float32)] * 2, good)
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, [np.zeros((24, 64), np.float32)[:, ::2]] * 2, good)     # pixels 8 bytes apart
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, good, [np.zeros((32, 24), np.float32).T] * 2)           # column-major
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, [good[0], padded[1]], good)                             # two row strides in one batch
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, good, [padded[0], good[1]])
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, good, good, role="previous", config=cfg)
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, good, good, role="reference")                           # a role needs a config
    with pytest.raises(ValueError):
        d.update_f32_host_batch(pyrs, good, good, flags=_lib.INGEST_DEFER)                    # host planes cannot be deferred
    # device planes
    with pytest.raises(ValueError):
        d.update_f32_device_batch(pyrs, [8, 16], [24])
    with pytest.raises(ValueError):
        d.update_f32_device_batch(pyrs, [8, 16], [24, 32], intensity_pitch=32 * 4 - 4)
    with pytest.raises(ValueError):
        d.update_f32_device_batch(pyrs, [8, 16], [24, 32], depth_pitch=32 * 4 - 4)
    with pytest.raises(ValueError):
        d.update_f32_device_batch(pyrs, [8, 16], [24, 32], depth_pitch=32 * 4 + 2)            # no multiple of 4
    with pytest.raises(ValueError):
        d.update_f32_device_batch(pyrs, [8, 16], [24, 32], role="current")
    with pytest.raises(ValueError):
        d.update_f32_device_batch(pyrs, [8, 16], [24, 32], role="both", config=cfg)


def test_mixed_batch_wrappers_reject_bad_arguments_before_the_library():
    cam = _camera()
    pyrs = [_Pyramid(cam), _Pyramid(cam)]
    zf = [np.zeros((24, 32), np.float32)] * 2
    zu = [np.zeros((24, 32), np.uint16)] * 2
    bgr = [np.zeros((24, 32, 3), np.uint8)] * 2
    grey = [np.zeros((24, 32, 1), np.uint8)] * 2
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, bgr, zf, "bgr8", depth_format="f16")
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, bgr, zf, "bgr8", depth_format=1)
    with pytest.raises(TypeError):
        d.update_colour_host_batch(pyrs, bgr, zu, "bgr8", depth_format="f32")                 # u16 planes named float
    with pytest.raises(TypeError):
        d.update_colour_host_batch(pyrs, bgr, zf, "bgr8")                                     # float planes named u16 (the default)
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, grey, zu, "grey8")                                   # grey8 comes with float depth only
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, bgr, zf, "grey8", depth_format="f32")                # 3 channels for a 1-byte format
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, bgr, zf, "f32", depth_format="f32")
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, grey, [np.zeros((24, 64), np.float32)[:, ::2]] * 2, "grey8", depth_format="f32")
    with pytest.raises(ValueError):
        d.update_colour_host_batch(pyrs, bgr, zf, "bgr8", depth_format="f32", flags=_lib.INGEST_DEFER)
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [8, 16], [24, 32], "grey8", 0)                     # grey8 + u16: the raw entry points
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [8, 16], [24, 32], "bgr8", 0, depth_pitch=128)     # a u16 plane has no pitch
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [8, 16], [24, 32], "bgr8", 0, depth_format="f32", depth_pitch=124)
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [8, 16], [24, 32], "grey8", 31, depth_format="f32")
    with pytest.raises(ValueError):
        d.update_colour_device_batch(pyrs, [8, 16], [24, 32], "rgba8", 0, depth_format="f32", role="current")


DEPTH_RULE = r"""
#include <cstdio>
#include <vector>
#include "colour.h"
int main(int argc, char** argv) {
  std::FILE* in = std::fopen(argv[1], "rb");
  float scale;
  unsigned n;
  if (!in || std::fread(&scale, 4, 1, in) != 1 || std::fread(&n, 4, 1, in) != 1) return 1;
  std::vector<float> z(n);
  if (std::fread(z.data(), 4, n, in) != n) return 1;
  std::fclose(in);
  for (unsigned i = 0; i < n; ++i) z[i] = dvo_hip::depth_of_f32(z[i], scale);
  std::FILE* out = std::fopen(argv[2], "wb");
  std::fwrite(z.data(), 4, n, out);
  std::fclose(out);
  return 0;
}
"""


def test_float_depth_rule_of_the_shared_header_equals_numpy(tmp_path):
    src = tmp_path / "depth_rule.cpp"
    src.write_text(DEPTH_RULE)
    exe = tmp_path / "depth_rule"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe)])
    rng = np.random.default_rng(5)
    z = (rng.random(4096, dtype=np.float32) * np.float32(8000.0)).astype(np.float32)
    z[::7] = np.nan
    z[1::97] = 0.0
    z[2::97] = -0.0
    z[3::97] = -z[3::97]
    z[4::97] = np.inf
    z[5::97] = -np.inf
    z[6::97] = np.float32(1e-42)                  # a subnormal
    for scale in (np.float32(1.0), np.float32(1e-3), np.float32(2e-4)):
        inp, out = tmp_path / "z.bin", tmp_path / "out.bin"
        with open(inp, "wb") as f:
            f.write(np.float32(scale).tobytes())
            f.write(np.uint32(z.size).tobytes())
            f.write(z.tobytes())
        subprocess.check_call([str(exe), str(inp), str(out)])
        got = np.fromfile(str(out), np.float32)
        with np.errstate(invalid="ignore"):
            want = z * scale
        assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
        assert np.array_equal(np.isnan(got), np.isnan(z))
        if scale == 1.0:
            assert np.array_equal(got.view(np.uint32), z.view(np.uint32))          # exact, NaN bits included


def build_f32_facade_check():
    out = os.path.join(ROOT, "tests", "cpp", "f32_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "f32_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-isystem", "/opt/rocm/include", src, "-o", out, "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lz"])
    return out


def test_cpp_facade_float_methods_compile():
    d.build()
    assert os.path.exists(build_f32_facade_check())
