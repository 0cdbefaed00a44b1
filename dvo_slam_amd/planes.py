"""Below the frames: handle and address arrays (FrameSet, device_pointer_array), pinned host planes, the validators of planes and formats."""
import ctypes as C

import numpy as np

from . import _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _sensor_format(name, width, height):
    """a raw sensor format (_lib.SENSOR_PIXEL_FORMATS) for planes of width x height pixels: the library's own size rules, raised here"""
    fmt, ch = _lib.SENSOR_PIXEL_FORMATS[name], _lib.SENSOR_PIXEL_CHANNELS[name]
    if ch == 1 and (width < 2 or height < 2):
        raise ValueError("a Bayer plane needs width >= 2 and height >= 2, not %d x %d" % (width, height))
    if ch == 2 and width % 2 != 0:
        raise ValueError("a YUV 4:2:2 plane needs an even width, not %d" % width)
    return fmt, ch


def _pixel_format(name, width, height, mixed=False):
    """(DVO_HIP_PIXEL_*, bytes per pixel) of a colour or a raw sensor format for planes of width x height pixels; mixed: the image comes
    with a float depth plane, and may then also be "grey8" ([h, w, 1] uint8)"""
    formats, channels = (_lib.MIXED_PIXEL_FORMATS, _lib.MIXED_PIXEL_CHANNELS) if mixed else (_lib.PIXEL_FORMATS, _lib.PIXEL_CHANNELS)
    if isinstance(name, str) and name in _lib.SENSOR_PIXEL_FORMATS:
        return _sensor_format(name, width, height)
    if not isinstance(name, str) or name not in formats:
        raise ValueError("pixel_format must be one of %s, not %r" % (sorted(formats) + sorted(_lib.SENSOR_PIXEL_FORMATS), name))
    return formats[name], channels[name]


def _pitch(pitch, width, channels):
    pitch = int(pitch)
    if pitch != 0 and pitch < width * channels:
        raise ValueError("pitch %d < width * channels = %d" % (pitch, width * channels))
    return pitch


def _colour_plane(a, h, w, channels, flat_ok=False):
    """a colour image [h, w, channels] of uint8 with contiguous pixels (rows may be padded); flat_ok: a one-byte plane (a Bayer mosaic)
    may also come as [h, w]"""
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise TypeError("colour plane must be a numpy uint8 array")
    if flat_ok and channels == 1 and a.shape == (h, w):
        return a if a.strides[1] == 1 and a.strides[0] >= w else np.ascontiguousarray(a)
    if a.shape != (h, w, channels):
        raise ValueError("colour plane must have shape %s, not %s" % ((h, w, channels), a.shape))
    if a.strides[1:] != (channels, 1) or a.strides[0] < w * channels:
        a = np.ascontiguousarray(a)
    return a


def _depth_plane(a, h, w):
    if not isinstance(a, np.ndarray) or a.dtype != np.uint16:
        raise TypeError("depth plane must be a numpy uint16 array")
    if a.shape != (h, w):
        raise ValueError("depth plane must have shape %s, not %s" % ((h, w), a.shape))
    return np.ascontiguousarray(a)


def _depth_format(name):
    if not isinstance(name, str) or name not in _lib.DEPTH_FORMATS:
        raise ValueError("depth_format must be one of %s, not %r" % (sorted(_lib.DEPTH_FORMATS), name))
    return _lib.DEPTH_FORMATS[name]


def _f32_pitch(pitch, width, what):
    pitch = int(pitch)
    if pitch != 0 and pitch < width * 4:
        raise ValueError("%s pitch %d < width * 4 = %d" % (what, pitch, width * 4))
    if pitch % 4 != 0:
        raise ValueError("%s pitch %d is no multiple of 4" % (what, pitch))
    return pitch


def _f32_plane(a, h, w, what):
    """a float32 image [h, w] whose pixels are contiguous (rows may be padded by a multiple of 4 bytes), usable in place"""
    if not isinstance(a, np.ndarray) or a.dtype != np.float32:
        raise TypeError("%s plane must be a numpy float32 array" % what)
    if a.shape != (h, w):
        raise ValueError("%s plane must have shape %s, not %s" % (what, (h, w), a.shape))
    if a.strides[1] != 4 or a.strides[0] < w * 4 or a.strides[0] % 4 != 0:
        raise ValueError("%s plane must have contiguous pixels and rows at least width * 4 bytes apart: the transfer is asynchronous" % what)
    return a


def _one_pitch(planes, what):
    pitch = planes[0].strides[0]
    if any(a.strides[0] != pitch for a in planes):
        raise ValueError("every %s plane of a batch must have the same row stride" % what)
    return pitch


class FrameSet:
    """A fixed list of pyramids with its ctypes handle array built once: a streaming caller that re-ingests and aligns the
    same frame objects batch after batch does not rebuild 128-element pointer arrays on every call (the batch entry points
    accept a FrameSet wherever they accept a list of pyramids)."""

    def __init__(self, pyramids):
        self.pyramids = list(pyramids)
        self.n = len(self.pyramids)
        self.ctx = self.pyramids[0].ctx
        self.handles = (C.c_void_p * self.n)(*[p.ptr for p in self.pyramids])

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(self.pyramids)

    def __getitem__(self, i):
        return self.pyramids[i]


def _handles(frames):
    if isinstance(frames, FrameSet):
        return frames.handles
    return (C.c_void_p * len(frames))(*[p.ptr for p in frames])


def device_pointer_array(ptrs):
    """ctypes array of device addresses (built once by callers that stream from fixed buffers)"""
    return (C.c_void_p * len(ptrs))(*[C.c_void_p(int(x)) for x in ptrs])


def _addresses(planes, n, on_device):
    """the address array of a batch call's planes: one the caller built once (a C.Array) as it is, else of device addresses or of the host arrays'"""
    if isinstance(planes, C.Array):
        return planes
    return device_pointer_array(planes) if on_device else (C.c_void_p * n)(*[a.ctypes.data for a in planes])


class PinnedRawPlanes:
    """Page-locked host memory for the raw planes of n frames (dvo_hip_host_alloc), laid out per frame as [u16 depth][u8 grey]
    so that a frame moves to the device in one transfer.  `depth[i]` / `grey[i]` are numpy views a decoder writes into."""

    def __init__(self, ctx, n, width, height):
        self.ctx, self.n, self.npx = ctx, n, width * height
        stride = (self.npx * 3 + 1) & ~1                     # frames that follow each other at this stride move in one transfer
        ptr = C.c_void_p()
        ctx.check(ctx._lib.dvo_hip_host_alloc(ctx.ptr, n * stride, C.byref(ptr)))
        self.ptr = ptr
        raw = (C.c_uint8 * (n * stride)).from_address(ptr.value)
        block = np.frombuffer(raw, dtype=np.uint8).reshape(n, stride)
        self.depth = [block[i, :self.npx * 2].view(np.uint16).reshape(height, width) for i in range(n)]
        self.grey = [block[i, self.npx * 2:self.npx * 3].reshape(height, width) for i in range(n)]

    def close(self):
        if self.ptr is not None:
            self.depth = self.grey = None
            self.ctx._lib.dvo_hip_host_free(self.ctx.ptr, self.ptr)
            self.ptr = None
