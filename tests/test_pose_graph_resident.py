"""CPU tier of the resident pose-graph path (dvo_hip_graph_optimize_batch; k_pg_resident in dvo_slam_amd/csrc/pose_graph.hip): what
needs no device.  The library exports the entry point; the limits of a resident-sized graph are stated once in pose_graph.h and
repeated faithfully by _lib.py and the wrapper; PoseGraph.optimize_batch refuses bad arguments before the library is called; without a
device the entry point says so; the C++ facade's optimizeBatch compiles and refuses what it must (tests/cpp/pose_graph_batch_facade_check.cpp
host).  The device's arithmetic is held to the yardstick in tests/test_gpu_pose_graph_resident.py."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
import test_pose_graph as tpg
from dvo_slam_amd import _lib


def test_the_library_exports_the_batch_entry_point():
    d.build()
    assert "dvo_hip_graph_optimize_batch" in _lib.EXPORTS
    L = C.CDLL(d.LIB_PATH)
    assert hasattr(L, "dvo_hip_graph_optimize_batch")
    header = open(os.path.join(tpg.ROOT, "include", "dvo_hip.h")).read()
    assert "int dvo_hip_graph_optimize_batch(dvo_hip_context* ctx, int n_graphs, dvo_hip_graph* const* graphs" in header
    assert "1024 vertices" in header and "4096 edges" in header and '"graph_resident_solves"' in header


def test_the_limits_are_stated_once_and_repeated_faithfully():
    src = open(os.path.join(tpg.CSRC, "pose_graph.h")).read()
    limits = {name: int(value) for name, value in re.findall(r"constexpr int (kPgResidentMax(?:Vertices|Edges)) = (\d+);", src)}
    assert limits == dict(kPgResidentMaxVertices=1024, kPgResidentMaxEdges=4096)
    assert (_lib.GRAPH_RESIDENT_MAX_VERTICES, _lib.GRAPH_RESIDENT_MAX_EDGES) == (1024, 4096)
    # the wrapper refuses by the same numbers: a graph one past either limit, and takes one at both (as far as the library)
    for n, m, refused in ((1025, 10, True), (10, 4097, True), (1024, 4096, False)):
        g = bare_graph(n, m)
        if refused:
            with pytest.raises(ValueError, match="1024 / 4096"):
                d.PoseGraph.optimize_batch([g])
        else:
            with pytest.raises(AttributeError):                       # (it got as far as the library, of which this object has none)
                d.PoseGraph.optimize_batch([g])


def bare_graph(n=3, m=2, ctx=None):
    """a PoseGraph with no library behind it: a call that gets as far as the library raises AttributeError"""
    g = d.PoseGraph.__new__(d.PoseGraph)
    g.ctx, g.ptr, g.n, g.m, g.delta, g._edges = ctx if ctx is not None else BARE_CONTEXT, None, n, m, np.zeros(m), None
    return g


BARE_CONTEXT = object()


def test_the_wrapper_refuses_bad_arguments_before_the_library():
    a, b = bare_graph(), bare_graph()
    batch = d.PoseGraph.optimize_batch
    for call in (lambda: batch([]), lambda: batch([a, a]), lambda: batch([a, b, a]), lambda: batch([a, b], params=[{}]),
                 lambda: batch([a, b], params=[{}, {}, {}]), lambda: batch([a, bare_graph(n=0)]), lambda: batch([a, bare_graph(ctx=object())]),
                 lambda: batch([a, b], params=dict(cg_tolerance=0.0)), lambda: batch([a, b], params=[{}, dict(max_iterations=-1)]),
                 lambda: batch([a, b], max_records=-1)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: batch([a, object()]), lambda: batch([a, None]), lambda: batch([tpg.HostGraph()]), lambda: batch([a, b], params=[{}, 3]),
                 lambda: batch([a, b], params=dict(iterations=3)), lambda: batch([a, b], max_records=1.5), lambda: batch([a, b], max_records=True)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: batch([a, b]), lambda: batch((a, b), params=dict(max_iterations=3)), lambda: batch([a], params=[dict(cg_max_iterations=5)], max_records=0)):
        with pytest.raises(AttributeError):                           # good arguments reach the library
            call()


def test_without_a_device_the_entry_point_says_so():
    d.build()
    L = C.CDLL(d.LIB_PATH)
    rep = _lib.GraphReport()
    ptrs = (C.c_void_p * 1)(None)
    L.dvo_hip_graph_optimize_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(_lib.GraphReport), C.c_void_p, C.c_int]
    rc = L.dvo_hip_graph_optimize_batch(None, 1, ptrs, None, C.byref(rep), None, 0)
    if L.dvo_hip_device_count() == 0:
        assert rc == _lib.ERR_NO_DEVICE
        with pytest.raises(d.DvoHipError) as err:                     # ... and so does the way to a graph: there is no context to make one in
            d.PoseGraph(d.Context(0))
        assert err.value.code == _lib.ERR_NO_DEVICE
    else:
        assert rc == _lib.ERR_INVALID                                 # (a device, but no context)


def build_batch_facade_check():
    out = os.path.join(tempfile.mkdtemp(prefix="pose_graph_batch_facade_"), "pose_graph_batch_facade_check")
    src = os.path.join(tpg.ROOT, "tests", "cpp", "pose_graph_batch_facade_check.cpp")
    libdir = os.path.join(tpg.ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(tpg.ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_batch_compiles_and_refuses_bad_lists():
    d.build()
    out = subprocess.run([build_batch_facade_check(), "host"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
