"""Re-ingest of planes into existing pyramids, batched (capi_ingest.inc): seven public calls, each its own checks and then one _ingest()."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .planes import _addresses, _colour_plane, _depth_format, _depth_plane, _f32_pitch, _f32_plane, _handles, _one_pitch, _pitch, _pixel_format


_ROLES = {"current": 0, "reference": 1}
_Plane = namedtuple("_Plane", "kind planes extra", defaults=((),))    # kind; addresses or host arrays; the C arguments that follow them (format, pitch)

# [image kind, depth kind, on the device][with a role] -> the C entry, one per IngestSource of capi_ingest.inc (_ex: role -1 for none)
_INGEST_ENTRIES = {("grey", "u16", False): ("dvo_hip_frames_update_raw", "dvo_hip_frames_update_raw_as"),
                   ("grey", "u16", True): ("dvo_hip_frames_update_raw_device", "dvo_hip_frames_update_raw_device_as"),
                   ("colour", "u16", False): ("dvo_hip_frames_update_colour_as_ex",) * 2,
                   ("colour", "u16", True): ("dvo_hip_frames_update_colour_device_as_ex",) * 2,
                   ("colour", "f32", False): ("dvo_hip_frames_update_colour_f32depth_as_ex",) * 2,
                   ("colour", "f32", True): ("dvo_hip_frames_update_colour_f32depth_device_as_ex",) * 2,
                   ("f32", "f32", False): ("dvo_hip_frames_update_f32_as_ex",) * 2,
                   ("f32", "f32", True): ("dvo_hip_frames_update_f32_device_as_ex",) * 2}


def _role_args(role, config, checked=True):
    """(role, config) as the C-ABI takes them, (-1, None) for no role; checked: ValueError for a role that is none or a role without a config"""
    if role is None:
        return -1, None
    if checked and role not in _ROLES:
        raise ValueError("role must be 'current', 'reference' or None, not %r" % (role,))
    if checked and config is None:
        raise ValueError("a role needs a config")
    ccfg = config if isinstance(config, _lib.Config) else config.to_c()
    return _ROLES[role], C.byref(ccfg)


def _ingest(pyramids, image, depth, on_device, depth_scale, role_args, flags=None):
    """The one way into dvo_hip_frames_update_*: image and depth are _Plane descriptions, role_args what _role_args gave (its place among
    a caller's checks is the caller's), flags None for the grey entries, which take none."""
    n, ctx = len(pyramids), pyramids[0].ctx
    with_role = role_args[0] >= 0
    entry = getattr(ctx._lib, _INGEST_ENTRIES[image.kind, depth.kind, bool(on_device)][with_role])
    tail = (role_args if with_role else ()) if flags is None else role_args + (int(flags),)
    ctx.check(entry(ctx.ptr, n, _handles(pyramids), _addresses(image.planes, n, on_device), *image.extra,
                    _addresses(depth.planes, n, on_device), *depth.extra, depth_scale, *tail))


def _one_per_pyramid(pyramids, image_planes, depth_planes, what):
    if len(image_planes) != len(pyramids) or len(depth_planes) != len(pyramids):
        raise ValueError("one %s and one depth plane per pyramid" % what)


def update_raw_device_batch(pyramids, grey_dev_ptrs, depth_dev_ptrs, depth_scale=1.0 / 5000.0, role=None, config=None):
    """Re-ingest raw planes (device pointers) into n existing pyramids of one camera, batched.  With role ("current" /
    "reference") and config: ingest and prepare_roles_batch in one pass over the raw planes (dvo_hip_frames_update_raw_device_as)."""
    role_args = _role_args(role, config, checked=False)    # (the grey calls never checked: KeyError for an unknown role, AttributeError for no config)
    _ingest(pyramids, _Plane("grey", grey_dev_ptrs), _Plane("u16", depth_dev_ptrs), True, depth_scale, role_args)


def update_raw_host_batch(pyramids, grey_host, depth_host, depth_scale=1.0 / 5000.0, role=None, config=None):
    """Re-ingest raw planes from HOST arrays (uint8 / uint16, C-contiguous) into n existing pyramids: asynchronous DMA on the
    context's upload stream, then the batched build (dvo_hip_frames_update_raw).  The arrays must stay unchanged until
    upload_wait() or until a match on these pyramids has returned."""
    if not isinstance(grey_host, C.Array):      # (else addresses prepared once by the caller: device_pointer_array of host addresses)
        for a, b in zip(grey_host, depth_host):  # (AssertionError, not TypeError: the grey calls' way, and tests hold it)
            assert a.dtype == np.uint8 and b.dtype == np.uint16 and a.flags.c_contiguous and b.flags.c_contiguous
    role_args = _role_args(role, config, checked=False)    # (as update_raw_device_batch)
    _ingest(pyramids, _Plane("grey", grey_host), _Plane("u16", depth_host), False, depth_scale, role_args)


def update_f32_device_batch(pyramids, intensity_ptrs, depth_ptrs, intensity_pitch=0, depth_pitch=0, depth_scale=1.0, role=None, config=None,
                            flags=0):
    """Re-ingest float32 planes (device pointers: intensity 0..255, depth in metres * depth_scale with NaN = hole; one row pitch in bytes
    per kind for all, 0 = tight) into n existing pyramids of one camera (dvo_hip_frames_update_f32_device_as_ex).  role None: a plain
    update; "current" / "reference" with config: ingest and prepare in one pass.  flags: _lib.INGEST_DEFER | _lib.INGEST_NO_RAW_COPY."""
    width = pyramids[0].camera.width
    ipitch, zpitch = _f32_pitch(intensity_pitch, width, "intensity"), _f32_pitch(depth_pitch, width, "depth")
    _one_per_pyramid(pyramids, intensity_ptrs, depth_ptrs, "intensity")
    _ingest(pyramids, _Plane("f32", intensity_ptrs, (ipitch,)), _Plane("f32", depth_ptrs, (zpitch,)), True, depth_scale, _role_args(role, config), flags)


def update_f32_host_batch(pyramids, intensity_host, depth_host, depth_scale=1.0, role=None, config=None, flags=0):
    """Re-ingest float32 planes from HOST arrays ([h, w] float32 views with contiguous pixels; the row stride of each kind, the same for
    the whole batch, is taken from the views) into n existing pyramids: DMA on the context's upload stream, then the batched build
    (dvo_hip_frames_update_f32_as_ex).  The arrays must stay unchanged until upload_wait() or a match on these pyramids has returned.
    flags: _lib.INGEST_NO_RAW_COPY (a host ingest cannot be deferred)."""
    cam = pyramids[0].camera
    _one_per_pyramid(pyramids, intensity_host, depth_host, "intensity")
    if int(flags) & _lib.INGEST_DEFER:
        raise ValueError("INGEST_DEFER takes device planes")
    ints = [_f32_plane(a, cam.height, cam.width, "intensity") for a in intensity_host]
    deps = [_f32_plane(b, cam.height, cam.width, "depth") for b in depth_host]
    ipitch, zpitch = _one_pitch(ints, "intensity"), _one_pitch(deps, "depth")
    _ingest(pyramids, _Plane("f32", ints, (ipitch,)), _Plane("f32", deps, (zpitch,)), False, depth_scale, _role_args(role, config), flags)


def update_colour_device_batch(pyramids, colour_dev_ptrs, depth_dev_ptrs, pixel_format="bgr8", pitch=0, depth_scale=1.0 / 5000.0, role=None,
                               config=None, flags=0, depth_format="u16", depth_pitch=0):
    """Re-ingest 8-bit colour planes (device pointers, one format and row pitch in bytes for all, 0 = tight) + u16 depth planes into n
    existing pyramids of one camera (dvo_hip_frames_update_colour_device_as_ex).  role None: a plain update; "current" / "reference"
    with config: ingest and prepare in one pass.  flags: _lib.INGEST_DEFER | _lib.INGEST_NO_RAW_COPY.
    depth_format "f32": the depth planes are float32 metres with NaN = hole and a row pitch of their own (depth_pitch, bytes, 0 = tight;
    dvo_hip_frames_update_colour_f32depth_device_as_ex); pixel_format may then also be "grey8".  Mind depth_scale: 1.0 for metres."""
    zf = _depth_format(depth_format) == _lib.DEPTH_F32
    pyr0 = pyramids[0]
    fmt, ch = _pixel_format(pixel_format, pyr0.camera.width, pyr0.camera.height, mixed=zf)
    pitch = _pitch(pitch, pyr0.camera.width, ch)
    if zf:
        depth_pitch = _f32_pitch(depth_pitch, pyr0.camera.width, "depth")
    elif int(depth_pitch) != 0:
        raise ValueError("a u16 depth plane is tight: depth_pitch goes with depth_format 'f32'")
    _one_per_pyramid(pyramids, colour_dev_ptrs, depth_dev_ptrs, "colour")
    depth = _Plane("f32", depth_dev_ptrs, (depth_pitch,)) if zf else _Plane("u16", depth_dev_ptrs)
    _ingest(pyramids, _Plane("colour", colour_dev_ptrs, (fmt, pitch)), depth, True, depth_scale, _role_args(role, config), flags)


def update_colour_host_batch(pyramids, colour_host, depth_host, pixel_format="bgr8", depth_scale=1.0 / 5000.0, role=None, config=None, flags=0,
                             depth_format="u16"):
    """Re-ingest 8-bit colour planes from HOST arrays ([h, w, 3 | 4] uint8, one format; rows may be padded by the same stride) + u16 depth
    planes (C-contiguous) into n existing pyramids: DMA on the context's upload stream, then the batched build
    (dvo_hip_frames_update_colour_as_ex).  The arrays must stay unchanged until upload_wait() or a match on these pyramids has returned.
    depth_format "f32": the depth planes are [h, w] float32 views (metres, NaN = hole; rows may be padded by the same stride;
    dvo_hip_frames_update_colour_f32depth_as_ex); pixel_format may then also be "grey8" ([h, w, 1] uint8).  Mind depth_scale: 1.0 for metres."""
    zf = _depth_format(depth_format) == _lib.DEPTH_F32
    cam = pyramids[0].camera
    fmt, ch = _pixel_format(pixel_format, cam.width, cam.height, mixed=zf)
    _one_per_pyramid(pyramids, colour_host, depth_host, "colour")
    if zf and int(flags) & _lib.INGEST_DEFER:
        raise ValueError("INGEST_DEFER takes device planes")
    cols = [_colour_plane(a, cam.height, cam.width, ch, pixel_format in _lib.SENSOR_PIXEL_FORMATS) for a in colour_host]
    deps = [_f32_plane(b, cam.height, cam.width, "depth") if zf else _depth_plane(b, cam.height, cam.width) for b in depth_host]
    if any(a is not b for a, b in zip(cols, colour_host)) or any(a is not b for a, b in zip(deps, depth_host)):
        raise ValueError("host planes must be usable in place (pixels contiguous, depth C-contiguous): the transfer is asynchronous")
    pitch = _one_pitch(cols, "colour")
    role_args = _role_args(role, config)
    depth = _Plane("f32", deps, (_one_pitch(deps, "depth"),)) if zf else _Plane("u16", deps)
    _ingest(pyramids, _Plane("colour", cols, (fmt, pitch)), depth, False, depth_scale, role_args, flags)


def upload_wait(ctx):
    ctx.check(ctx._lib.dvo_hip_upload_wait(ctx.ptr))


def prepare_roles_batch(pyramids, role, config):
    """Build the role planes of n pyramids ahead of time and asynchronously (dvo_hip_frames_prepare): role "current" = sampling
    planes, "reference" = point selection for config's thresholds.  Together with update_raw_device_batch this runs on the
    context's build stream, concurrently with a match started afterwards on other frames."""
    ctx = pyramids[0].ctx
    cfg = _role_args(role, config, checked=False)[1]
    ctx.check(ctx._lib.dvo_hip_frames_prepare(ctx.ptr, len(pyramids), _handles(pyramids), _ROLES[role], cfg))   # (_ROLES[role]: KeyError for no role)
