"""The Python binding's surface (CPU tier): every public name of dvo_slam_amd and dvo_slam_amd.tracker with its signature and docstring,
as scripts/dump_python_api.py tabulates them, against the table recorded before tracker.py was split by subject
(tests/golden/python_api.json) -- what holds the names, arguments and documentation still for the calls no other test makes."""
import glob
import importlib.util
import json
import os

from common import ROOT

import dvo_slam_amd
from dvo_slam_amd import tracker


def _dump_module():
    spec = importlib.util.spec_from_file_location("dump_python_api", os.path.join(ROOT, "scripts", "dump_python_api.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_surface_is_the_recorded_one():
    dump = _dump_module()
    got = json.loads(json.dumps(dump.table()))                 # (through JSON, as the fixture went)
    want = json.load(open(dump.FIXTURE))
    assert sorted(got) == sorted(want)
    assert got["tracker_private"] == want["tracker_private"] == list(dump.PRIVATE)
    for module in dump.MODULES:
        assert sorted(got[module]) == sorted(want[module]), module
        for name in want[module]:
            assert got[module][name] == want[module][name], "%s.%s" % (module, name)


def test_the_package_exports_the_trackers_own_objects():
    exported = [n for n in vars(dvo_slam_amd) if not n.startswith("_") and hasattr(tracker, n)]
    assert len(exported) >= 60
    for n in exported:
        assert getattr(dvo_slam_amd, n) is getattr(tracker, n), n


def test_no_module_of_the_binding_is_longer_than_700_lines():
    files = sorted(glob.glob(os.path.join(ROOT, "dvo_slam_amd", "*.py")))
    assert len(files) >= 10
    for path in files:
        with open(path) as f:
            assert sum(1 for _ in f) <= 700, os.path.relpath(path, ROOT)
