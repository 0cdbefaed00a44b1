"""What a frame carries besides its planes (dvo_hip_frames_set_* / _clear_*): selection, lens, depth rig, depth filter, colour -- one table."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .planes import _colour_plane, _handles, _pitch, _pixel_format, device_pointer_array


def set_selection_batch(pyramids, masks=None, min_depth=0.0, max_depth=float("inf"), pitch=0):
    """RgbdImagePyramid.set_selection for n pyramids of one context in one call.  masks: None, or one entry per pyramid -- None (no
    mask), a (height, width) uint8 numpy array, or a device address; host arrays and device addresses are not mixed in one call."""
    n, ctx = len(pyramids), pyramids[0].ctx
    ptrs, on_device, keep = None, 0, []
    if masks is not None:
        if len(masks) != n:
            raise ValueError("set_selection_batch: one mask entry per pyramid")
        kinds = {isinstance(m, np.ndarray) for m in masks if m is not None}
        if len(kinds) > 1:
            raise ValueError("set_selection_batch: host arrays and device addresses in one call")
        on_device = 1 if kinds == {False} else 0
        entries = []
        for p, m in zip(pyramids, masks):
            if m is None:
                entries.append(None)
            elif isinstance(m, np.ndarray):
                c = p.camera
                if m.dtype != np.uint8 or m.shape != (c.height, c.width):
                    raise ValueError("set_selection_batch: a host mask is a (%d, %d) uint8 array" % (c.height, c.width))
                m = np.ascontiguousarray(m)
                keep.append(m)
                entries.append(m.ctypes.data)
            else:
                entries.append(int(m))
        ptrs = (C.c_void_p * n)(*entries)
    ctx.check(ctx._lib.dvo_hip_frames_set_selection(ctx.ptr, n, _handles(pyramids), ptrs, pitch if on_device else 0, on_device,
                                                    float(min_depth), float(max_depth)))
    for i, p in enumerate(pyramids):
        m = None if masks is None else masks[i]
        if isinstance(m, np.ndarray):
            m = np.array(m, np.uint8)                      # (kept for a frame that is built again with more levels)
        p._selection = ([m] if m is not None else None, min_depth, max_depth, pitch)


def clear_selection_batch(pyramids):
    ctx = pyramids[0].ctx
    for p in pyramids:
        p._selection = None
    ctx.check(ctx._lib.dvo_hip_frames_clear_selection(ctx.ptr, len(pyramids), _handles(pyramids)))


def _intrinsics_and(who, k_name, K, o_name, other):
    """K and the argument beside it as float64 arrays, K being (fx, fy, ox, oy), or TypeError / ValueError in the words of `who`"""
    for name, a in ((k_name, K), (o_name, other)):
        if a is None or (isinstance(a, np.ndarray) and a.dtype.kind not in "fiu"):
            raise TypeError("%s: %s must be real numbers" % (who, name))
    try:
        k, o = np.asarray(K, np.float64), np.asarray(other, np.float64)
    except (TypeError, ValueError):
        raise TypeError("%s: %s and %s must be sequences of real numbers" % (who, k_name, o_name))
    if k.shape != (4,):
        raise ValueError("%s: %s is (fx, fy, ox, oy)" % (who, k_name))
    return k, o


def _finite_float32(who, k_name, k, o_name, other, focal):
    """k and the array beside it as float32, or ValueError where one is not finite then or a focal length (named `focal`) not positive"""
    with np.errstate(over="ignore"):
        k32, o32 = k.astype(np.float32), other.astype(np.float32)
    if not (np.isfinite(k32).all() and np.isfinite(o32).all()):
        raise ValueError("%s: %s and %s must be finite" % (who, k_name, o_name))
    if not (k32[0] > 0 and k32[1] > 0):
        raise ValueError("%s: %s must be positive" % (who, focal))
    return k32, o32


def lens_struct(K_raw, D, rectify_depth=True):
    """dvo_hip_lens from K_raw (4 finite floats, fx and fy positive) and D (4, 5 or 8 finite floats, padded with zeros); raises before
    anything reaches the library."""
    k, d = _intrinsics_and("set_lens", "K_raw", K_raw, "D", D)
    if d.ndim != 1 or d.shape[0] not in (4, 5, 8):
        raise ValueError("set_lens: D has 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
    k32, d32 = _finite_float32("set_lens", "K_raw", k, "D", d, "fx_raw and fy_raw")
    if not isinstance(rectify_depth, (bool, int, np.bool_, np.integer)):
        raise TypeError("set_lens: rectify_depth is a bool")
    lens = _lib.Lens()
    lens.K_raw[:] = [float(v) for v in k32]
    lens.D[:] = [float(v) for v in d32] + [0.0] * (8 - d32.shape[0])
    lens.rectify_depth = 1 if rectify_depth else 0
    lens.reserved = 0
    return lens


def depth_rig_struct(K_depth, T):
    """dvo_hip_depth_rig from K_depth (4 finite floats, fx and fy positive) and T (3 x 4, 4 x 4 with a last row of 0 0 0 1, or 12 finite
    floats row-major: [R | t], depth sensor -> colour camera, metres); raises before anything reaches the library."""
    k, t = _intrinsics_and("set_depth_rig", "K_depth", K_depth, "T", T)
    if t.shape == (4, 4):
        if not np.array_equal(t[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("set_depth_rig: the last row of a 4 x 4 T is 0 0 0 1")
        t = t[:3]
    if t.shape == (12,):
        t = t.reshape(3, 4)
    if t.shape != (3, 4):
        raise ValueError("set_depth_rig: T is 3 x 4 (or 4 x 4, or 12 values row-major): [R | t]")
    k32, t32 = _finite_float32("set_depth_rig", "K_depth", k, "T", t, "fx_d and fy_d")
    rig = _lib.DepthRig()
    rig.K_depth[:] = [float(v) for v in k32]
    rig.T[:] = [float(v) for v in t32.reshape(-1)]
    rig.reserved[:] = [0, 0]
    return rig


def _colour_sources(pyramids, sources, pixel_format, pitch, who="set_colour"):
    """(format, pitch, on_device, addresses, what to keep alive during the call, what each pyramid remembers) of a set_colour call, or
    ValueError / TypeError: nothing reaches the library with a value it would refuse"""
    n = len(pyramids)
    if n < 1:
        raise ValueError("%s: no pyramids" % who)
    for p in pyramids:
        fmt, ch = _pixel_format(pixel_format, p.camera.width, p.camera.height)
    flat_ok = pixel_format in _lib.SENSOR_PIXEL_FORMATS
    if sources is None or len(sources) != n:
        raise ValueError("%s: one colour plane per pyramid" % who)
    if isinstance(pitch, bool) or not isinstance(pitch, (int, np.integer)):
        raise TypeError("%s: pitch must be an integer" % who)
    if len(set(id(p) for p in pyramids)) != n:
        raise ValueError("%s: the same pyramid twice" % who)
    arrays = [isinstance(a, np.ndarray) for a in sources]
    if any(arrays) != all(arrays):
        raise TypeError("%s: the planes of one call are all numpy arrays or all device addresses" % who)
    for p in pyramids:
        if p.ctx is not pyramids[0].ctx:
            raise ValueError("%s: pyramids of more than one context" % who)
        if getattr(p, "_lens", None) is not None:
            raise ValueError("%s: a pyramid that carries a lens takes raw sensor planes; attach rectified colour to a pyramid without one" % who)
    if all(arrays):
        if int(pitch) != 0:
            raise ValueError("%s: a numpy array brings its own row stride; pitch is for device addresses" % who)
        planes = [_colour_plane(a, p.camera.height, p.camera.width, ch, flat_ok) for a, p in zip(sources, pyramids)]
        tight = all(a.strides[0] == p.camera.width * ch for a, p in zip(planes, pyramids))
        if not tight and len(set(a.strides[0] for a in planes)) != 1:
            planes, tight = [np.ascontiguousarray(a) for a in planes], True   # (one pitch per call: mixed paddings go tight)
        row = 0 if tight else planes[0].strides[0]
        return fmt, row, 0, [a.ctypes.data for a in planes], planes, [np.array(a, copy=True) for a in planes]
    for a in sources:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or int(a) == 0:
            raise TypeError("%s: a colour plane is a numpy uint8 array or a non-null device address, not %r" % (who, a))
    for p in pyramids:
        _pitch(pitch, p.camera.width, ch)
    return fmt, int(pitch), 1, [int(a) for a in sources], None, [int(a) for a in sources]


def set_colour_batch(pyramids, sources, pixel_format="bgr8", pitch=0):
    """RgbdImagePyramid.set_colour for n pyramids in one launch (dvo_hip_frames_set_colour); they may differ in size."""
    pyramids = list(pyramids)
    fmt, row, on_device, addrs, keep, remember = _colour_sources(pyramids, sources, pixel_format, pitch)
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_set_colour(ctx.ptr, len(pyramids), _handles(pyramids), device_pointer_array(addrs), fmt, row, on_device))
    for p, r in zip(pyramids, remember):
        p._colour = (r, pixel_format, 0 if isinstance(r, np.ndarray) else int(pitch))


_DEPTH_FILTER_DEFAULTS = dict(radius=2, sigma_space=1.5, noise_a=0.0012, noise_b=0.0019, gate=3.0, edge_radius=1, edge_abs=0.01, edge_rel=0.03,
                              hole_radius=0)
_DEPTH_FILTER_INTS = {"radius": 3, "edge_radius": 2, "hole_radius": 2}   # field -> largest value


def depth_filter_default():
    """The fields of dvo_hip_depth_filter_default() as a dict (values recalled from published Kinect axial-noise fits, NOT verified
    by this project): what set_depth_filter starts from."""
    return dict(_DEPTH_FILTER_DEFAULTS)


def depth_filter_struct(**params):
    """dvo_hip_depth_filter from keyword arguments over depth_filter_default(); raises before anything reaches the library."""
    unknown = sorted(set(params) - set(_DEPTH_FILTER_DEFAULTS))
    if unknown:
        raise TypeError("set_depth_filter: unknown field %s" % ", ".join(unknown))
    values = dict(_DEPTH_FILTER_DEFAULTS)
    values.update(params)
    filt = _lib.DepthFilter()
    for name, v in values.items():
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("set_depth_filter: %s must be a real number" % name)
        if name in _DEPTH_FILTER_INTS:
            if int(v) != v:
                raise TypeError("set_depth_filter: %s must be an integer" % name)
            if not 0 <= int(v) <= _DEPTH_FILTER_INTS[name]:
                raise ValueError("set_depth_filter: %s must be 0..%d" % (name, _DEPTH_FILTER_INTS[name]))
            setattr(filt, name, int(v))
            continue
        with np.errstate(over="ignore"):
            v32 = np.float32(v)
        if not np.isfinite(v32):
            raise ValueError("set_depth_filter: %s must be finite" % name)
        setattr(filt, name, float(v32))
    if filt.radius > 0 and not filt.sigma_space > 0:
        raise ValueError("set_depth_filter: sigma_space must be > 0 when radius > 0")
    if not filt.gate > 0:
        raise ValueError("set_depth_filter: gate must be > 0")
    for name in ("noise_a", "noise_b", "edge_abs", "edge_rel"):
        if getattr(filt, name) < 0:
            raise ValueError("set_depth_filter: %s must not be negative" % name)
    if not (filt.noise_a > 0 or filt.noise_b > 0):
        raise ValueError("set_depth_filter: sigma(z) must be positive (noise_a and noise_b are both 0)")
    filt.reserved[:] = [0, 0]
    return filt


def set_level_selection(pyramid, level, accepted):
    """Explicit selection of one level (dvo_hip_frame_set_level_selection): `accepted`, a (height, width) array of that level, is the
    exact accepted set (non-zero = selected) until the pyramid's pixels change or another selection is requested; None drops it."""
    pyramid.build(level + 1)
    a, ctx = None, pyramid.ctx
    if accepted is not None:
        img = pyramid.level(level)
        a = np.ascontiguousarray(accepted, dtype=np.uint8)
        if a.shape != (img.height, img.width):
            raise ValueError("set_level_selection: accepted is (%d, %d)" % (img.height, img.width))
    ctx.check(ctx._lib.dvo_hip_frame_set_level_selection(ctx.ptr, pyramid.ptr, level, None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))))


# One record per kind of attachment.  name: the C entries are dvo_hip_frames_set_<name> and _clear_<name>, the public calls set_<name>_batch
# and clear_<name>_batch; attribute: where a pyramid remembers what it carries (None: nothing); replay(pyramid, remembered): hands it to a
# frame made anew; refuse(remembered): raises BEFORE the frame is made anew where that cannot work.  Lens, depth rig and depth filter are
# one struct per call: struct builds it, remember says what the attribute keeps of it, _attach / _detach are their whole set and clear.
Attachment = namedtuple("Attachment", "name attribute replay refuse struct remember", defaults=(None, None, None))


def _attach(kind, pyramids, *args, **params):
    struct = kind.struct(*args, **params)                    # (raises before anything reaches the library)
    if len(pyramids) < 1:
        raise ValueError("set_%s_batch: no pyramids" % kind.name)
    ctx = pyramids[0].ctx
    ctx.check(getattr(ctx._lib, "dvo_hip_frames_set_" + kind.name)(ctx.ptr, len(pyramids), _handles(pyramids), C.byref(struct)))
    for p in pyramids:
        setattr(p, kind.attribute, kind.remember(struct))    # (kept for a frame that is built again with more levels)


def _detach(kind, pyramids, who=None):
    if len(pyramids) < 1:
        raise ValueError("%s: no pyramids" % (who or "clear_%s_batch" % kind.name))
    ctx = pyramids[0].ctx
    ctx.check(getattr(ctx._lib, "dvo_hip_frames_clear_" + kind.name)(ctx.ptr, len(pyramids), _handles(pyramids)))
    for p in pyramids:
        setattr(p, kind.attribute, None)


def _refuse_device_mask(sel):
    if sel[0] is not None and not isinstance(sel[0][0], np.ndarray):      # (its mask would have to be read again from an address that may have been freed)
        raise ValueError("RgbdImagePyramid.build: the pyramid holds a selection from a device address; build it with all its levels "
                         "before set_selection, or clear_selection first")


def _replay_colour(pyramid, colour):                         # (from the host copy)
    if not isinstance(colour[0], np.ndarray):
        raise ValueError("RgbdImagePyramid.build: the pyramid holds colour from a device address; build it with all its levels "
                         "before set_colour, or clear_colour first")
    set_colour_batch([pyramid], [colour[0]], colour[1], colour[2])


_LENS = Attachment("lens", "_lens", lambda p, kept: _attach(_LENS, [p], *kept), struct=lens_struct,
                   remember=lambda lens: (list(lens.K_raw), list(lens.D), bool(lens.rectify_depth)))
_DEPTH_RIG = Attachment("depth_rig", "_depth_rig", lambda p, kept: _attach(_DEPTH_RIG, [p], *kept), struct=depth_rig_struct,
                        remember=lambda rig: (list(rig.K_depth), list(rig.T)))
_DEPTH_FILTER = Attachment("depth_filter", "_depth_filter", lambda p, kept: _attach(_DEPTH_FILTER, [p], **kept), struct=depth_filter_struct,
                           remember=lambda filt: {name: getattr(filt, name) for name in _DEPTH_FILTER_DEFAULTS})
_COLOUR = Attachment("colour", "_colour", _replay_colour)
# the order in which RgbdImagePyramid.build replays them
ATTACHMENTS = (Attachment("selection", "_selection", lambda p, kept: set_selection_batch([p], *kept), refuse=_refuse_device_mask),
               _LENS, _DEPTH_RIG, _DEPTH_FILTER, _COLOUR)


def clear_colour_batch(pyramids):
    _detach(_COLOUR, list(pyramids), "clear_colour")


def set_lens_batch(pyramids, K_raw, D, rectify_depth=True):
    """RgbdImagePyramid.set_lens for n pyramids of one context in one call (they then carry equal lenses, as one ingest call wants)."""
    _attach(_LENS, pyramids, K_raw, D, rectify_depth)


def clear_lens_batch(pyramids):
    _detach(_LENS, pyramids)


def set_depth_rig_batch(pyramids, K_depth, T):
    """RgbdImagePyramid.set_depth_rig for n pyramids of one context in one call (they then carry equal rigs, as one ingest call wants)."""
    _attach(_DEPTH_RIG, pyramids, K_depth, T)


def clear_depth_rig_batch(pyramids):
    _detach(_DEPTH_RIG, pyramids)


def set_depth_filter_batch(pyramids, **params):
    """RgbdImagePyramid.set_depth_filter for n pyramids of one context in one call (they then carry equal filters, as one ingest call wants)."""
    _attach(_DEPTH_FILTER, pyramids, **params)


def clear_depth_filter_batch(pyramids):
    _detach(_DEPTH_FILTER, pyramids)
