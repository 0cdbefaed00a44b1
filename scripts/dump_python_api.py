#!/usr/bin/env python3
"""The Python binding's surface as one table: what tests/test_python_api.py holds against tests/golden/python_api.json.

For dvo_slam_amd and dvo_slam_amd.tracker, every public module-level name that the package defines (modules, and classes and
functions of other packages such as numpy, are the importing file's business and are left out) with its kind; for callables
str(inspect.signature(...)) and the SHA-1 of inspect.getdoc(...); for classes the same for every public method and for __init__;
for plain constants and dtypes their repr; and the private tracker._* names the tests and scripts reach.

  python scripts/dump_python_api.py             prints the table
  python scripts/dump_python_api.py --write     rewrites the fixture (only when the surface is meant to change)
"""
import hashlib
import importlib
import inspect
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "python_api.json")
MODULES = ("dvo_slam_amd", "dvo_slam_amd.tracker")
PRIVATE = ("_handles", "_colour_sources", "_covis_args", "_map_frames_args", "_warp_args", "_render_view_args", "_rehash_capacity",
           "_RESULT_DTYPE")


def _doc(obj):
    doc = inspect.getdoc(obj)
    return None if doc is None else hashlib.sha1(doc.encode()).hexdigest()


def _callable(obj):
    try:
        sig = str(inspect.signature(obj))
    except (TypeError, ValueError):
        sig = None
    return {"signature": sig, "doc": _doc(obj)}


def _member(cls, name):
    raw = inspect.getattr_static(cls, name)
    if isinstance(raw, (staticmethod, classmethod)):
        return dict(_callable(raw.__func__), kind=type(raw).__name__)
    if isinstance(raw, property):
        return {"kind": "property", "doc": _doc(raw)}
    if inspect.isfunction(raw):
        return dict(_callable(raw), kind="method")
    return {"kind": "attribute", "repr": repr(raw)}


def _ours(obj):
    return (getattr(obj, "__module__", None) or "").split(".")[0] == "dvo_slam_amd"


def describe(obj):
    """the table's entry of one module-level object, or None for what the table leaves out"""
    if isinstance(obj, types.ModuleType):
        return None
    if inspect.isclass(obj):
        if not _ours(obj):
            return None
        names = sorted(n for c in obj.__mro__ if _ours(c) for n in vars(c) if not n.startswith("_") or n == "__init__")
        return {"kind": "class", "doc": _doc(obj), "bases": [b.__name__ for b in obj.__bases__],
                "members": {n: _member(obj, n) for n in sorted(set(names))}}
    if inspect.isfunction(obj) or inspect.isbuiltin(obj):
        return dict(_callable(obj), kind="function") if _ours(obj) else None
    return {"kind": "constant", "repr": repr(obj).replace(ROOT, "<root>")}      # (LIB_PATH: the same table in every checkout)


def table():
    """{module: {name: entry}}; a name of the package that is the tracker's own object with the tracker's entry is only listed, under the key "=tracker" """
    out = {}
    for name in MODULES:
        mod = importlib.import_module(name)
        out[name] = {n: d for n, d in ((n, describe(getattr(mod, n))) for n in sorted(vars(mod)) if not n.startswith("_")) if d is not None}
    tracker = importlib.import_module("dvo_slam_amd.tracker")
    package, own = importlib.import_module("dvo_slam_amd"), out["dvo_slam_amd"]
    same = [n for n in sorted(own) if getattr(package, n) is getattr(tracker, n, None) and own[n] == out["dvo_slam_amd.tracker"].get(n)]
    out["dvo_slam_amd"] = dict({n: d for n, d in own.items() if n not in same}, **{"=tracker": same})
    out["tracker_private"] = [n for n in PRIVATE if hasattr(tracker, n)]
    return out


def text(t):
    """the table as JSON with one line per name"""
    def compact(v):
        return json.dumps(v, sort_keys=True, separators=(",", ":"))
    parts = []
    for key in sorted(t):
        if isinstance(t[key], dict):
            parts.append("%s: {\n%s\n}" % (json.dumps(key), ",\n".join("%s: %s" % (json.dumps(n), compact(t[key][n])) for n in sorted(t[key]))))
        else:
            parts.append("%s: %s" % (json.dumps(key), compact(t[key])))
    return "{\n%s\n}\n" % ",\n".join(parts)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w") as f:
            f.write(text(table()))
    else:
        sys.stdout.write(text(table()))
