"""dvo::core::RgbdImage, RgbdImagePyramid and RgbdCameraPyramid: the frames on the device and how they are created."""
import ctypes as C

import numpy as np

from . import _lib
from .context import default_context
from .planes import _colour_plane, _depth_plane, _fp, _pitch, _pixel_format
from .attachments import (ATTACHMENTS, clear_colour_batch, clear_depth_filter_batch, clear_depth_rig_batch, clear_lens_batch, clear_selection_batch,
                          set_colour_batch, set_depth_filter_batch, set_depth_rig_batch, set_lens_batch, set_selection_batch)


class RgbdImage:
    """One pyramid level: host mirrors of the device planes, downloaded lazily (rgbd_image.h:161-179)."""
    _PLANES = {"intensity": 0, "depth": 1, "intensity_dx": 2, "intensity_dy": 3, "depth_dx": 4, "depth_dy": 5}

    def __init__(self, pyramid, level):
        self._pyr, self._level = pyramid, level
        w, h = C.c_int(), C.c_int()
        K = np.zeros(4, np.float32)
        pyramid.ctx.check(pyramid.ctx._lib.dvo_hip_frame_info(pyramid.ptr, level, C.byref(w), C.byref(h), _fp(K)))
        self.width, self.height, self.K = w.value, h.value, K
        self.timestamp = pyramid._timestamp
        self._cache = {}

    def __getattr__(self, name):
        planes = type(self)._PLANES
        if name in planes:
            if name not in self._cache:
                out = np.empty((self.height, self.width), np.float32)
                ctx = self._pyr.ctx
                ctx.check(ctx._lib.dvo_hip_frame_download_plane(ctx.ptr, self._pyr.ptr, self._level, planes[name], _fp(out)))
                self._cache[name] = out
            return self._cache[name]
        raise AttributeError(name)

    def buildPointCloud(self):        # device side needs nothing: points are recomputed from Z
        pass

    def buildAccelerationStructure(self):   # built at frame creation
        pass


class RgbdImagePyramid:
    def __init__(self, camera, make_frame, levels, timestamp=0.0):
        self.camera, self.ctx = camera, camera.ctx
        self._make_frame = make_frame
        self._timestamp = timestamp
        self.levels = 0
        self.ptr = None
        self.build(levels)

    def build(self, num_levels):            # rgbd_image.cpp:156-172 (idempotent, only ever grows)
        if self.levels >= num_levels:
            return
        carried = [(kind, kept) for kind in ATTACHMENTS if (kept := getattr(self, kind.attribute, None)) is not None]
        for kind, kept in carried:
            if kind.refuse:
                kind.refuse(kept)
        if self.ptr:
            self.ctx._lib.dvo_hip_frame_destroy(self.ctx.ptr, self.ptr)
        self.ptr = self._make_frame(num_levels)
        self.levels = num_levels
        for kind, kept in carried:                           # (a new frame: what the old one carried is handed over again)
            kind.replay(self, kept)

    def set_selection(self, mask=None, min_depth=0.0, max_depth=float("inf"), pitch=0):
        """Caller selection of this frame's reference points (an extension over the reference API; include/dvo_hip.h,
        dvo_hip_frames_set_selection): a level-0 mask -- a (height, width) uint8 numpy array, or a device address (e.g.
        torch_tensor.data_ptr()) of height rows of `pitch` bytes (0 = width) -- and / or a depth range in metres.  Kept across
        re-ingests until replaced or cleared.  The mask is copied at once; a pyramid that holds a mask given by device address cannot
        grow more levels afterwards (build raises ValueError: the frame would be made anew from a mask that may be gone)."""
        set_selection_batch([self], [mask] if mask is not None else None, min_depth, max_depth, pitch)

    def clear_selection(self):
        clear_selection_batch([self])

    def set_lens(self, K_raw, D, rectify_depth=True):
        """Lens of this frame's camera (an extension over the reference API, whose nodes sit behind a CPU rectifier; include/dvo_hip.h,
        dvo_hip_frames_set_lens): K_raw = (fx, fy, ox, oy) of the raw image, D = 4, 5 or 8 OpenCV coefficients k1 k2 p1 p2 [k3 [k4 k5
        k6]].  Every later update_* of this pyramid takes its planes as raw camera planes and rectifies them on the device first.  Kept
        across re-ingests until replaced or cleared.  rectify_depth=False: the depth plane is taken pixel for pixel."""
        set_lens_batch([self], K_raw, D, rectify_depth)

    def clear_lens(self):
        clear_lens_batch([self])

    def set_depth_rig(self, K_depth, T):
        """Depth rig of this frame's sensors (an extension over the reference API, whose nodes sit behind a CPU depth_image_proc/register
        stage; include/dvo_hip.h, dvo_hip_frames_set_depth_rig): K_depth = (fx, fy, ox, oy) of the depth sensor's image, T = the 3 x 4 or
        4 x 4 transform [R | t] from depth-sensor to colour-camera coordinates in metres.  Every later update_* of this pyramid takes its
        depth plane as the depth sensor's own image and registers it into the colour camera on the device first.  Kept across
        re-ingests until replaced or cleared."""
        set_depth_rig_batch([self], K_depth, T)

    def clear_depth_rig(self):
        clear_depth_rig_batch([self])

    def set_depth_filter(self, **params):
        """Depth filter of this frame (an extension over the reference API, which has no such pass; include/dvo_hip.h,
        dvo_hip_frames_set_depth_filter): keyword arguments are the fields of dvo_hip_depth_filter -- radius, sigma_space, noise_a,
        noise_b, gate, edge_radius, edge_abs, edge_rel, hole_radius -- over depth_filter_default().  Every later update_* of this
        pyramid conditions its depth plane on the device first, behind the depth rig and the lens: flying pixels at depth edges and
        hole borders become NaN, the noise of kept pixels is smoothed.  Kept across re-ingests until replaced or cleared."""
        set_depth_filter_batch([self], **params)

    def clear_depth_filter(self):
        clear_depth_filter_batch([self])

    def set_colour(self, colour, pixel_format="bgr8", pitch=0):
        """Colour of this frame (include/dvo_hip.h, dvo_hip_frames_set_colour; the reference's level(0).rgb, benchmark_slam.cpp:89-90): a
        (height, width, 3 | 4) uint8 numpy array (rows may be padded), or a device address (e.g. torch_tensor.data_ptr()) of height rows
        of `pitch` bytes (0 = tight).  pixel_format: "bgr8" | "rgb8" | "bgra8" | "rgba8", or a raw sensor format (see
        RgbdCameraPyramid.create_colour; the colour stored is that of its BGR8 image).  What a KeyframeMap(colour=True) fuses.  Kept
        across re-ingests until replaced or cleared: re-attach after re-ingesting other content.  A pyramid with a lens refuses."""
        set_colour_batch([self], [colour], pixel_format, pitch)

    def clear_colour(self):
        clear_colour_batch([self])

    def colour(self, level=0):
        """The colour plane of `level` as the map's insertion sees it (dvo_hip_frame_download_colour): a (h_L, w_L) uint32 array of
        packed pixels 0x00RRGGBB, per channel the rounded mean of the 2^L x 2^L block of level 0."""
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
            raise TypeError("RgbdImagePyramid.colour: level must be an integer")
        if not 0 <= level < self.levels:
            raise ValueError("RgbdImagePyramid.colour: the pyramid has levels 0 .. %d" % (self.levels - 1))
        if getattr(self, "_colour", None) is None:           # (getattr: the tests hand in stand-ins)
            raise ValueError("RgbdImagePyramid.colour: the pyramid carries no colour (set_colour)")
        w, h = self.camera.width >> int(level), self.camera.height >> int(level)
        out = np.empty((h, w), np.uint32)
        self.ctx.check(self.ctx._lib.dvo_hip_frame_download_colour(self.ctx.ptr, self.ptr, int(level), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    compute = build                         # deprecated alias in the reference too

    def update_raw_device(self, grey_dev_ptr, depth_dev_ptr, depth_scale=1.0 / 5000.0):
        """Re-ingest new raw planes already in HBM into this pyramid (no allocation, asynchronous)."""
        self.ctx.check(self.ctx._lib.dvo_hip_frame_update_raw_device(self.ctx.ptr, self.ptr, C.c_void_p(grey_dev_ptr),
                                                                     C.c_void_p(depth_dev_ptr), depth_scale))

    def level(self, idx):
        assert idx < self.levels
        return RgbdImage(self, idx)

    def timestamp(self):
        return self._timestamp

    def __del__(self):
        try:
            if self.ptr and self.ctx.ptr:
                self.ctx._lib.dvo_hip_frame_destroy(self.ctx.ptr, self.ptr)
        except Exception:
            pass
        self.ptr = None


class RgbdCameraPyramid:
    """RgbdCameraPyramid(width, height, intrinsics) with intrinsics = (fx, fy, ox, oy)."""

    def __init__(self, base_width, base_height, base_intrinsics, ctx=None):
        self.ctx = ctx or default_context()
        self.width, self.height = int(base_width), int(base_height)
        self.K = np.ascontiguousarray(base_intrinsics, dtype=np.float32)
        assert self.K.shape == (4,)
        self.levels = 1

    def build(self, levels):                # rgbd_image.cpp:283-296
        self.levels = max(self.levels, int(levels))

    def _create(self, entry, timestamp, *planes):
        """The pyramid of a dvo_hip_frame_create_* entry; planes: its arguments between K and the level count (they hold what they point to)."""
        def make(levels):
            ptr = C.c_void_p()
            self.ctx.check(getattr(self.ctx._lib, entry)(self.ctx.ptr, self.width, self.height, _fp(self.K), *planes, levels, C.byref(ptr)))
            return ptr
        return RgbdImagePyramid(self, make, self.levels, timestamp)

    def create(self, base_intensity, base_depth, timestamp=0.0):
        """intensity: float32 0..255 (CV_32FC1), depth: float32 metres with NaN = invalid (asserts at rgbd_image.cpp:350,356)."""
        I, Z = np.ascontiguousarray(base_intensity), np.ascontiguousarray(base_depth)
        assert I.dtype == np.float32 and Z.dtype == np.float32, "intensity and depth must be float32 (CV_32FC1)"
        assert I.shape == (self.height, self.width) and Z.shape == I.shape
        return self._create("dvo_hip_frame_create_f32", timestamp, _fp(I), _fp(Z))

    def create_raw(self, grey_u8, depth_u16, depth_scale=1.0 / 5000.0, timestamp=0.0):
        """Ingest of raw sensor planes (benchmark_slam.cpp:46-93): conversion happens on the device."""
        G = np.ascontiguousarray(grey_u8, dtype=np.uint8)
        D = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        assert G.shape == (self.height, self.width) and D.shape == G.shape
        u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
        return self._create("dvo_hip_frame_create_raw", timestamp, G.ctypes.data_as(u8p), D.ctypes.data_as(u16p), depth_scale)

    def create_raw_device(self, grey_dev_ptr, depth_dev_ptr, depth_scale=1.0 / 5000.0, timestamp=0.0):
        """Raw planes already resident in HBM (device pointers, e.g. torch tensors' data_ptr())."""
        return self._create("dvo_hip_frame_create_raw_device", timestamp, C.c_void_p(grey_dev_ptr), C.c_void_p(depth_dev_ptr), depth_scale)

    def create_colour(self, colour_u8, depth_u16, pixel_format="bgr8", depth_scale=1.0 / 5000.0, timestamp=0.0):
        """Ingest of an 8-bit colour plane [h, w, 3 | 4] + the u16 depth plane: the CV_BGR2GRAY conversion the reference's callers run on
        the host (benchmark_slam.cpp:55-69) happens on the device (dvo_hip_frame_create_colour).  pixel_format: "bgr8" | "rgb8" |
        "bgra8" | "rgba8"; rows may be padded (a view with a larger row stride), pixels must be contiguous.  Or a raw sensor plane as the
        camera driver publishes it (_lib.SENSOR_PIXEL_FORMATS): a Bayer mosaic "bayer_rggb8" | "bayer_bggr8" | "bayer_gbrg8" |
        "bayer_grbg8", [h, w] or [h, w, 1] uint8, or YUV 4:2:2 "yuyv8" | "uyvy8", [h, w, 2] uint8 with an even w -- demosaicked / converted
        on the device (csrc/sensor_formats.h); so with every other pixel_format argument of this module."""
        fmt, ch = _pixel_format(pixel_format, self.width, self.height)
        Cl = _colour_plane(colour_u8, self.height, self.width, ch, flat_ok=pixel_format in _lib.SENSOR_PIXEL_FORMATS)
        D = _depth_plane(depth_u16, self.height, self.width)
        return self._create("dvo_hip_frame_create_colour", timestamp, Cl.ctypes.data_as(C.c_void_p), fmt, Cl.strides[0],
                            D.ctypes.data_as(C.POINTER(C.c_uint16)), depth_scale)

    def create_colour_device(self, colour_dev_ptr, pixel_format, pitch, depth_dev_ptr, depth_scale=1.0 / 5000.0, timestamp=0.0):
        """A colour plane already resident in HBM (device pointer, row pitch in bytes, 0 = tight) + the u16 depth plane."""
        fmt, ch = _pixel_format(pixel_format, self.width, self.height)
        pitch = _pitch(pitch, self.width, ch)
        return self._create("dvo_hip_frame_create_colour_device", timestamp, C.c_void_p(colour_dev_ptr), fmt, pitch, C.c_void_p(depth_dev_ptr),
                            depth_scale)

    def create_f32_device(self, intensity_dev_ptr, depth_dev_ptr, timestamp=0.0):
        """Float32 planes already resident in HBM (device pointers, both tight: e.g. torch tensors' data_ptr()): intensity 0..255,
        depth in metres with NaN = invalid -- create() without the trip through the host (dvo_hip_frame_create_f32_device).  The planes
        must stay valid until the pyramid's first use has been waited for."""
        for p in (intensity_dev_ptr, depth_dev_ptr):
            if not isinstance(p, (int, np.integer)) or isinstance(p, bool) or int(p) == 0 or int(p) % 4 != 0:
                raise ValueError("a float plane needs a non-null device address that is a multiple of 4, not %r" % (p,))
        return self._create("dvo_hip_frame_create_f32_device", timestamp, C.c_void_p(int(intensity_dev_ptr)), C.c_void_p(int(depth_dev_ptr)))
