"""Host-side mirror of the reference's dvo_core class API for the alignment hot path.

Same names, argument meaning and error behaviour as
  dvo::DenseTracker / Config / Result / Stats      dvo_core/include/dvo/dense_tracking.h:36-215
  dvo::core::RgbdCameraPyramid / RgbdImagePyramid  dvo_core/include/dvo/core/rgbd_image.h:99-262
  dvo::core::PointSelection                         dvo_core/include/dvo/core/point_selection.h:69-99
but every pixel operation runs on the MI355X through libdvo_hip.so (include/dvo_hip.h).  The
C++ facade with the identical role for C++ callers lives in include/dvo/.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import DvoHipError

TERMINATION = {0: "IterationsExceeded", 1: "IncrementTooSmall", 2: "LogLikelihoodDecreased", 3: "TooFewConstraints",
               -1: "unset"}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Context:
    """One device + one HIP stream + scratch (dvo_hip_context).  One per host thread."""

    def __init__(self, device=0):
        self._lib = _lib.lib()
        self.ptr = C.c_void_p()
        rc = self._lib.dvo_hip_context_create(device, C.byref(self.ptr))
        if rc != _lib.OK:
            raise DvoHipError(rc, self._lib.dvo_hip_last_error(None).decode())
        self.device = device

    def check(self, rc):
        if rc != _lib.OK:
            raise DvoHipError(rc, self._lib.dvo_hip_last_error(self.ptr).decode())

    def set_option(self, key, value):
        self.check(self._lib.dvo_hip_set_option(self.ptr, key.encode(), int(value)))

    def counter(self, key):
        """An event counter of the context ("resident_launches", "resident_timeouts")."""
        v = C.c_longlong(0)
        self.check(self._lib.dvo_hip_get_counter(self.ptr, key.encode(), C.byref(v)))
        return v.value

    @property
    def stream(self):
        return self._lib.dvo_hip_context_stream(self.ptr)

    def close(self):
        if getattr(self, "ptr", None):
            self._lib.dvo_hip_context_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_context = None


def default_context():
    global _default_context
    if _default_context is None:
        _default_context = Context(0)
    return _default_context


@dataclass
class Config:
    """dvo::DenseTracker::Config; defaults = dvo_core/src/dense_tracking_config.cpp:27-42."""
    FirstLevel: int = 3
    LastLevel: int = 1
    MaxIterationsPerLevel: int = 100
    Precision: float = 5e-7
    Mu: float = 0.0
    UseInitialEstimate: bool = False
    UseWeighting: bool = True            # dead for match(); kept so callers compile
    UseParallel: bool = False            # dead
    InfluenceFuntionType: int = 2        # TDistribution (dead)
    InfluenceFunctionParam: float = 5.0  # dead
    ScaleEstimatorType: int = 2          # TDistribution (dead)
    ScaleEstimatorParam: float = 5.0     # dead
    IntensityDerivativeThreshold: float = 0.0
    DepthDerivativeThreshold: float = 0.0

    def getNumLevels(self):
        return self.FirstLevel + 1

    def UseEstimateSmoothing(self):
        return self.Mu > 1e-6

    def IsSane(self):
        return self.FirstLevel >= self.LastLevel

    def to_c(self):
        return _lib.Config(self.FirstLevel, self.LastLevel, self.MaxIterationsPerLevel, int(self.UseInitialEstimate),
                           self.Precision, self.Mu, self.IntensityDerivativeThreshold, self.DepthDerivativeThreshold)


@dataclass
class IterationStats:
    Id: int = 0
    ValidConstraints: int = 0
    TDistributionLogLikelihood: float = 0.0
    TDistributionMean: np.ndarray = None
    TDistributionPrecision: np.ndarray = None
    PriorLogLikelihood: float = 0.0
    EstimateIncrement: np.ndarray = None
    EstimateInformation: np.ndarray = None

    def InformationEigenValues(self):
        return np.sort(np.linalg.eigvals(self.EstimateInformation).real)

    def InformationConditionNumber(self):
        ev = self.InformationEigenValues()
        return abs(ev[5] / ev[0])


@dataclass
class LevelStats:
    Id: int = 0
    MaxValidPixels: int = 0
    ValidPixels: int = 0
    TerminationCriterion: int = -1
    Iterations: list = field(default_factory=list)

    def HasIterationWithIncrement(self):   # dense_tracking_config.cpp:138-143
        need = 2 if self.TerminationCriterion in (2, 3) else 1
        return len(self.Iterations) >= need

    def LastIterationWithIncrement(self):
        assert self.HasIterationWithIncrement()
        return self.Iterations[-2] if self.TerminationCriterion == 2 else self.Iterations[-1]

    def LastIteration(self):
        return self.Iterations[-1]


@dataclass
class Stats:
    Levels: list = field(default_factory=list)


class Result:
    """dvo::DenseTracker::Result (dense_tracking.h:125-140, dense_tracking_config.cpp:96-121)."""

    def __init__(self):
        self.Transformation = np.full((4, 4), np.nan)
        self.Transformation[3] = [0, 0, 0, 1]
        self.Information = np.eye(6)
        self.LogLikelihood = np.finfo(np.float64).max
        self.Statistics = Stats()
        self.Entropy = self.ConditionNumber = self.ConstraintRatio = float("nan")
        self.ConstraintRatioAccepted = 0.0

    def isNaN(self):
        return not (np.isfinite(self.Transformation.sum()) and np.isfinite(self.Information.sum()))

    def setIdentity(self):
        self.Transformation = np.eye(4)
        self.Information = np.eye(6)
        self.LogLikelihood = 0.0

    def clearStatistics(self):
        self.Statistics.Levels = []


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
        sel = getattr(self, "_selection", None)
        if sel is not None and sel[0] is not None and not isinstance(sel[0][0], np.ndarray):
            # (the frame is made anew, and its mask would have to be read again from a device address that may have been freed)
            raise ValueError("RgbdImagePyramid.build: the pyramid holds a selection from a device address; build it with all its levels "
                             "before set_selection, or clear_selection first")
        if self.ptr:
            self.ctx._lib.dvo_hip_frame_destroy(self.ctx.ptr, self.ptr)
        self.ptr = self._make_frame(num_levels)
        self.levels = num_levels
        if sel is not None:                                  # (a new frame: the selection is handed over again, from the host copy)
            set_selection_batch([self], *sel)
        lens = getattr(self, "_lens", None)
        if lens is not None:                                 # (... and so is the lens)
            set_lens_batch([self], *lens)
        rig = getattr(self, "_depth_rig", None)
        if rig is not None:                                  # (... and the depth rig)
            set_depth_rig_batch([self], *rig)
        filt = getattr(self, "_depth_filter", None)
        if filt is not None:                                 # (... and the depth filter)
            set_depth_filter_batch([self], **filt)
        colour = getattr(self, "_colour", None)
        if colour is not None:                               # (... and the colour, from the host copy)
            if not isinstance(colour[0], np.ndarray):
                raise ValueError("RgbdImagePyramid.build: the pyramid holds colour from a device address; build it with all its levels "
                                 "before set_colour, or clear_colour first")
            set_colour_batch([self], [colour[0]], colour[1], colour[2])

    def set_selection(self, mask=None, min_depth=0.0, max_depth=float("inf"), pitch=0):
        """Caller selection of this frame's reference points (an extension over the reference API; include/dvo_hip.h,
        dvo_hip_frames_set_selection): a level-0 mask -- a (height, width) uint8 numpy array, or a device address (e.g.
        torch_tensor.data_ptr()) of height rows of `pitch` bytes (0 = width) -- and / or a depth range in metres.  Kept across
        re-ingests until replaced or cleared.  The mask is copied at once; a pyramid that holds a mask given by device address cannot
        grow more levels afterwards (build raises ValueError: the frame would be made anew from a mask that may be gone)."""
        set_selection_batch([self], [mask] if mask is not None else None, min_depth, max_depth, pitch)

    def clear_selection(self):
        self._selection = None
        self.ctx.check(self.ctx._lib.dvo_hip_frames_clear_selection(self.ctx.ptr, 1, (C.c_void_p * 1)(self.ptr)))

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
        if getattr(self, "_colour", None) is None:
            raise ValueError("RgbdImagePyramid.colour: the pyramid carries no colour (set_colour)")
        w, h = self.camera.width >> int(level), self.camera.height >> int(level)
        out = np.empty((h, w), np.uint32)
        self.ctx.check(self.ctx._lib.dvo_hip_frame_download_colour(self.ctx.ptr, self.ptr, int(level), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    compute = build                         # deprecated alias in the reference too

    def update_raw_device(self, grey_dev_ptr, depth_dev_ptr, depth_scale=1.0 / 5000.0):
        """Re-ingest new raw planes already in HBM into this pyramid (no allocation, asynchronous)."""
        import ctypes as C
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

    def create(self, base_intensity, base_depth, timestamp=0.0):
        """intensity: float32 0..255 (CV_32FC1), depth: float32 metres with NaN = invalid (asserts at rgbd_image.cpp:350,356)."""
        I = np.ascontiguousarray(base_intensity)
        Z = np.ascontiguousarray(base_depth)
        assert I.dtype == np.float32 and Z.dtype == np.float32, "intensity and depth must be float32 (CV_32FC1)"
        assert I.shape == (self.height, self.width) and Z.shape == I.shape

        def make(levels):
            ptr = C.c_void_p()
            self.ctx.check(self.ctx._lib.dvo_hip_frame_create_f32(self.ctx.ptr, self.width, self.height, _fp(self.K), _fp(I), _fp(Z),
                                                                   levels, C.byref(ptr)))
            return ptr
        return RgbdImagePyramid(self, make, self.levels, timestamp)

    def create_raw(self, grey_u8, depth_u16, depth_scale=1.0 / 5000.0, timestamp=0.0):
        """Ingest of raw sensor planes (benchmark_slam.cpp:46-93): conversion happens on the device."""
        G = np.ascontiguousarray(grey_u8, dtype=np.uint8)
        D = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        assert G.shape == (self.height, self.width) and D.shape == G.shape

        def make(levels):
            ptr = C.c_void_p()
            self.ctx.check(self.ctx._lib.dvo_hip_frame_create_raw(
                self.ctx.ptr, self.width, self.height, _fp(self.K), G.ctypes.data_as(C.POINTER(C.c_uint8)),
                D.ctypes.data_as(C.POINTER(C.c_uint16)), depth_scale, levels, C.byref(ptr)))
            return ptr
        return RgbdImagePyramid(self, make, self.levels, timestamp)

    def create_raw_device(self, grey_dev_ptr, depth_dev_ptr, depth_scale=1.0 / 5000.0, timestamp=0.0):
        """Raw planes already resident in HBM (device pointers, e.g. torch tensors' data_ptr())."""
        def make(levels):
            ptr = C.c_void_p()
            self.ctx.check(self.ctx._lib.dvo_hip_frame_create_raw_device(
                self.ctx.ptr, self.width, self.height, _fp(self.K), C.c_void_p(grey_dev_ptr), C.c_void_p(depth_dev_ptr),
                depth_scale, levels, C.byref(ptr)))
            return ptr
        return RgbdImagePyramid(self, make, self.levels, timestamp)


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

        def make(levels):
            ptr = C.c_void_p()
            self.ctx.check(self.ctx._lib.dvo_hip_frame_create_colour(
                self.ctx.ptr, self.width, self.height, _fp(self.K), C.c_void_p(Cl.ctypes.data), fmt, Cl.strides[0],
                D.ctypes.data_as(C.POINTER(C.c_uint16)), depth_scale, levels, C.byref(ptr)))
            return ptr
        return RgbdImagePyramid(self, make, self.levels, timestamp)

    def create_colour_device(self, colour_dev_ptr, pixel_format, pitch, depth_dev_ptr, depth_scale=1.0 / 5000.0, timestamp=0.0):
        """A colour plane already resident in HBM (device pointer, row pitch in bytes, 0 = tight) + the u16 depth plane."""
        fmt, ch = _pixel_format(pixel_format, self.width, self.height)
        pitch = _pitch(pitch, self.width, ch)

        def make(levels):
            ptr = C.c_void_p()
            self.ctx.check(self.ctx._lib.dvo_hip_frame_create_colour_device(
                self.ctx.ptr, self.width, self.height, _fp(self.K), C.c_void_p(colour_dev_ptr), fmt, pitch, C.c_void_p(depth_dev_ptr),
                depth_scale, levels, C.byref(ptr)))
            return ptr
        return RgbdImagePyramid(self, make, self.levels, timestamp)

    def create_f32_device(self, intensity_dev_ptr, depth_dev_ptr, timestamp=0.0):
        """Float32 planes already resident in HBM (device pointers, both tight: e.g. torch tensors' data_ptr()): intensity 0..255,
        depth in metres with NaN = invalid -- create() without the trip through the host (dvo_hip_frame_create_f32_device).  The planes
        must stay valid until the pyramid's first use has been waited for."""
        for p in (intensity_dev_ptr, depth_dev_ptr):
            if not isinstance(p, (int, np.integer)) or isinstance(p, bool) or int(p) == 0 or int(p) % 4 != 0:
                raise ValueError("a float plane needs a non-null device address that is a multiple of 4, not %r" % (p,))

        def make(levels):
            ptr = C.c_void_p()
            self.ctx.check(self.ctx._lib.dvo_hip_frame_create_f32_device(
                self.ctx.ptr, self.width, self.height, _fp(self.K), C.c_void_p(int(intensity_dev_ptr)), C.c_void_p(int(depth_dev_ptr)), levels,
                C.byref(ptr)))
            return ptr
        return RgbdImagePyramid(self, make, self.levels, timestamp)


def _sensor_format(name, width, height):
    """a raw sensor format (_lib.SENSOR_PIXEL_FORMATS) for planes of width x height pixels: the library's own size rules, raised here"""
    fmt, ch = _lib.SENSOR_PIXEL_FORMATS[name], _lib.SENSOR_PIXEL_CHANNELS[name]
    if ch == 1 and (width < 2 or height < 2):
        raise ValueError("a Bayer plane needs width >= 2 and height >= 2, not %d x %d" % (width, height))
    if ch == 2 and width % 2 != 0:
        raise ValueError("a YUV 4:2:2 plane needs an even width, not %d" % width)
    return fmt, ch


def _pixel_format(name, width, height):
    """(DVO_HIP_PIXEL_*, bytes per pixel) of a colour or a raw sensor format for planes of width x height pixels"""
    if isinstance(name, str) and name in _lib.SENSOR_PIXEL_FORMATS:
        return _sensor_format(name, width, height)
    if not isinstance(name, str) or name not in _lib.PIXEL_FORMATS:
        raise ValueError("pixel_format must be one of %s, not %r" % (sorted(_lib.PIXEL_FORMATS) + sorted(_lib.SENSOR_PIXEL_FORMATS), name))
    return _lib.PIXEL_FORMATS[name], _lib.PIXEL_CHANNELS[name]


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


_ROLES = {"current": 0, "reference": 1}


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


def _pointer_array(ptrs):
    return ptrs if isinstance(ptrs, C.Array) else device_pointer_array(ptrs)


def update_raw_device_batch(pyramids, grey_dev_ptrs, depth_dev_ptrs, depth_scale=1.0 / 5000.0, role=None, config=None):
    """Re-ingest raw planes (device pointers) into n existing pyramids of one camera, batched.  With role ("current" /
    "reference") and config: ingest and prepare_roles_batch in one pass over the raw planes (dvo_hip_frames_update_raw_device_as)."""
    n = len(pyramids)
    ctx = pyramids[0].ctx
    fr, g, z = _handles(pyramids), _pointer_array(grey_dev_ptrs), _pointer_array(depth_dev_ptrs)
    if role is None:
        ctx.check(ctx._lib.dvo_hip_frames_update_raw_device(ctx.ptr, n, fr, g, z, depth_scale))
    else:
        ccfg = config if isinstance(config, _lib.Config) else config.to_c()
        ctx.check(ctx._lib.dvo_hip_frames_update_raw_device_as(ctx.ptr, n, fr, g, z, depth_scale, _ROLES[role], C.byref(ccfg)))


def set_selection_batch(pyramids, masks=None, min_depth=0.0, max_depth=float("inf"), pitch=0):
    """RgbdImagePyramid.set_selection for n pyramids of one context in one call.  masks: None, or one entry per pyramid -- None (no
    mask), a (height, width) uint8 numpy array, or a device address; host arrays and device addresses are not mixed in one call."""
    n = len(pyramids)
    ctx = pyramids[0].ctx
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


def lens_struct(K_raw, D, rectify_depth=True):
    """dvo_hip_lens from K_raw (4 finite floats, fx and fy positive) and D (4, 5 or 8 finite floats, padded with zeros); raises before
    anything reaches the library."""
    for name, a in (("K_raw", K_raw), ("D", D)):
        if a is None or (isinstance(a, np.ndarray) and a.dtype.kind not in "fiu"):
            raise TypeError("set_lens: %s must be real numbers" % name)
    try:
        k = np.asarray(K_raw, np.float64)
        d = np.asarray(D, np.float64)
    except (TypeError, ValueError):
        raise TypeError("set_lens: K_raw and D must be sequences of real numbers")
    if k.shape != (4,):
        raise ValueError("set_lens: K_raw is (fx, fy, ox, oy)")
    if d.ndim != 1 or d.shape[0] not in (4, 5, 8):
        raise ValueError("set_lens: D has 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
    with np.errstate(over="ignore"):
        k32, d32 = k.astype(np.float32), d.astype(np.float32)
    if not (np.isfinite(k32).all() and np.isfinite(d32).all()):
        raise ValueError("set_lens: K_raw and D must be finite")
    if not (k32[0] > 0 and k32[1] > 0):
        raise ValueError("set_lens: fx_raw and fy_raw must be positive")
    if not isinstance(rectify_depth, (bool, int, np.bool_, np.integer)):
        raise TypeError("set_lens: rectify_depth is a bool")
    lens = _lib.Lens()
    lens.K_raw[:] = [float(v) for v in k32]
    lens.D[:] = [float(v) for v in d32] + [0.0] * (8 - d32.shape[0])
    lens.rectify_depth = 1 if rectify_depth else 0
    lens.reserved = 0
    return lens


def set_lens_batch(pyramids, K_raw, D, rectify_depth=True):
    """RgbdImagePyramid.set_lens for n pyramids of one context in one call (they then carry equal lenses, as one ingest call wants)."""
    lens = lens_struct(K_raw, D, rectify_depth)
    if len(pyramids) < 1:
        raise ValueError("set_lens_batch: no pyramids")
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_set_lens(ctx.ptr, len(pyramids), _handles(pyramids), C.byref(lens)))
    for p in pyramids:
        p._lens = (list(lens.K_raw), list(lens.D), bool(lens.rectify_depth))   # (kept for a frame that is built again with more levels)


def clear_lens_batch(pyramids):
    if len(pyramids) < 1:
        raise ValueError("clear_lens_batch: no pyramids")
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_clear_lens(ctx.ptr, len(pyramids), _handles(pyramids)))
    for p in pyramids:
        p._lens = None


def depth_rig_struct(K_depth, T):
    """dvo_hip_depth_rig from K_depth (4 finite floats, fx and fy positive) and T (3 x 4, 4 x 4 with a last row of 0 0 0 1, or 12 finite
    floats row-major: [R | t], depth sensor -> colour camera, metres); raises before anything reaches the library."""
    for name, a in (("K_depth", K_depth), ("T", T)):
        if a is None or (isinstance(a, np.ndarray) and a.dtype.kind not in "fiu"):
            raise TypeError("set_depth_rig: %s must be real numbers" % name)
    try:
        k = np.asarray(K_depth, np.float64)
        t = np.asarray(T, np.float64)
    except (TypeError, ValueError):
        raise TypeError("set_depth_rig: K_depth and T must be sequences of real numbers")
    if k.shape != (4,):
        raise ValueError("set_depth_rig: K_depth is (fx, fy, ox, oy)")
    if t.shape == (4, 4):
        if not np.array_equal(t[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("set_depth_rig: the last row of a 4 x 4 T is 0 0 0 1")
        t = t[:3]
    if t.shape == (12,):
        t = t.reshape(3, 4)
    if t.shape != (3, 4):
        raise ValueError("set_depth_rig: T is 3 x 4 (or 4 x 4, or 12 values row-major): [R | t]")
    with np.errstate(over="ignore"):
        k32, t32 = k.astype(np.float32), t.astype(np.float32)
    if not (np.isfinite(k32).all() and np.isfinite(t32).all()):
        raise ValueError("set_depth_rig: K_depth and T must be finite")
    if not (k32[0] > 0 and k32[1] > 0):
        raise ValueError("set_depth_rig: fx_d and fy_d must be positive")
    rig = _lib.DepthRig()
    rig.K_depth[:] = [float(v) for v in k32]
    rig.T[:] = [float(v) for v in t32.reshape(-1)]
    rig.reserved[:] = [0, 0]
    return rig


def set_depth_rig_batch(pyramids, K_depth, T):
    """RgbdImagePyramid.set_depth_rig for n pyramids of one context in one call (they then carry equal rigs, as one ingest call wants)."""
    rig = depth_rig_struct(K_depth, T)
    if len(pyramids) < 1:
        raise ValueError("set_depth_rig_batch: no pyramids")
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_set_depth_rig(ctx.ptr, len(pyramids), _handles(pyramids), C.byref(rig)))
    for p in pyramids:
        p._depth_rig = (list(rig.K_depth), list(rig.T))      # (kept for a frame that is built again with more levels)


def clear_depth_rig_batch(pyramids):
    if len(pyramids) < 1:
        raise ValueError("clear_depth_rig_batch: no pyramids")
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_clear_depth_rig(ctx.ptr, len(pyramids), _handles(pyramids)))
    for p in pyramids:
        p._depth_rig = None


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


def clear_colour_batch(pyramids):
    pyramids = list(pyramids)
    if len(pyramids) < 1:
        raise ValueError("clear_colour: no pyramids")
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_clear_colour(ctx.ptr, len(pyramids), _handles(pyramids)))
    for p in pyramids:
        p._colour = None


def _pose_array(poses, n, who, per="pyramid", counted="pyramids", maps="camera -> world", some=False, finite=False):
    """poses as a contiguous [n, 4, 4] float64 array (n None: as many as there are; one 4 x 4 matrix is one pose), or ValueError /
    TypeError.  per, counted, maps: what a pose belongs to, what n counts and what a pose maps, for the messages; some: an empty array
    is refused as a shape; finite: an entry that is not finite is refused"""
    try:
        T = np.ascontiguousarray(poses, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("%s: poses must be real numbers, one 4 x 4 matrix per %s" % (who, per))
    if T.ndim == 2 and n in (None, 1):
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4) or (some and T.shape[0] < 1):
        raise ValueError("%s: a pose is a 4 x 4 matrix (%s), got shape %s" % (who, maps, T.shape))
    if n is not None and T.shape[0] != n:
        raise ValueError("%s: %d %s but %d poses" % (who, n, counted, T.shape[0]))
    if finite and not np.all(np.isfinite(T)):
        raise ValueError("%s: a pose has an entry that is not finite" % who)
    return T


_VIEW_POSES = dict(per="view", some=True)                                                             # KeyframeMap.render*, render_into
_MERGE_POSES = dict(per="source", counted="sources", maps="source -> destination", finite=True)      # KeyframeMap.merge, move_submaps, absorb


_MAP_RECORD, _MAP_COLOUR_RECORD, _MAP_NORMAL_RECORD = np.dtype(_lib.MAP_RECORD), np.dtype(_lib.MAP_COLOUR_RECORD), np.dtype(_lib.MAP_NORMAL_RECORD)
_TORCH_DTYPES = {}                                           # numpy dtype -> torch dtype of the same bits, filled at the first device array


def _out_array(ctx, shape, dtype, device):
    """an uninitialised output array of a C-ABI call: a numpy array or -- device -- a torch tensor on the context's GPU, which has the
    signed type of the same width for an unsigned one and int32 words for a record type: the same bits"""
    if not device:
        return np.empty(shape, dtype)
    import torch
    if not _TORCH_DTYPES:
        _TORCH_DTYPES.update({np.dtype(np.float32): torch.float32, np.dtype(np.uint32): torch.int32, np.dtype(np.uint64): torch.int64,
                              np.dtype(np.uint16): torch.int16})
    dt = np.dtype(dtype)
    if dt.fields:
        shape, dt = (shape, dt.itemsize // 4), np.dtype(np.uint32)
    return torch.empty(shape, dtype=_TORCH_DTYPES[dt], device="cuda:%d" % ctx.device)


def _address(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _pyramids_at_level(pyramids, level, who, then=None, others=(), limit=None, ctx=None, foreign="the pyramids belong to different contexts"):
    """The pyramids of a call that reads them at one level, or ValueError / TypeError: a list that is not empty (limit: and no longer
    than that), an integer level that every pyramid -- and every one of `others` -- has, and one context: ctx, else the first pyramid's
    (False: any; foreign: what the message says of another).  then: called once the list has passed, before the level is looked at (the
    call's other arguments, which it refuses first); its value is returned."""
    if len(pyramids) < 1:
        raise ValueError("%s: no pyramids" % who)
    if limit is not None and len(pyramids) > limit:
        raise ValueError("%s: %d pyramids, one call takes %d" % (who, len(pyramids), limit))
    value = then() if then else None
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
        raise TypeError("%s: level must be an integer" % who)
    ctx = pyramids[0].ctx if ctx is None else ctx
    for p in list(pyramids) + list(others):
        if not 0 <= level < p.levels:
            raise ValueError("%s: a pyramid of %d levels has no level %d" % (who, p.levels, level))
        if ctx is not False and p.ctx is not ctx:
            raise ValueError("%s: %s" % (who, foreign))
    return value


def _level_outputs(pyramids, level, count, trailing, device):
    """count lists of one float32 output array [h, w] + trailing per pyramid at `level`, and their pointer arrays"""
    ctx = pyramids[0].ctx
    shapes = []
    for p in pyramids:
        w, h = C.c_int(), C.c_int()
        ctx.check(ctx._lib.dvo_hip_frame_info(p.ptr, level, C.byref(w), C.byref(h), None))
        shapes.append((h.value, w.value) + trailing)
    out = [[_out_array(ctx, s, np.float32, device) for s in shapes] for _ in range(count)]
    return out, [device_pointer_array([_address(a) for a in arrays]) for arrays in out]


def _map_frames_args(pyramids, poses, level, min_depth, max_depth, who):
    """(n, poses as a contiguous [n, 4, 4] float64 array) of a keyframe-map call, or ValueError / TypeError: nothing reaches the library
    with a pose that is not 4 x 4, mismatched lengths, a level a pyramid does not have or an empty depth range."""
    n = len(pyramids)
    T = _pyramids_at_level(pyramids, level, who, then=lambda: _pose_array(poses, n, who))
    if not float(min_depth) <= float(max_depth):
        raise ValueError("%s: need min_depth <= max_depth (no NaN)" % who)
    return n, T


def world_points_batch(pyramids, poses, level=0, min_depth=0.0, max_depth=float("inf"), device=False):
    """The organised world clouds of n keyframes (dvo_hip_frames_world_points; the reference's AsyncPointCloudBuilder::BuildJob::build):
    per pyramid an [h, w, 4] float32 array {P.x, P.y, P.z, I} of level `level` under its 4 x 4 pose (camera -> world); unusable pixels
    have NaN in x, y, z.  device=True: torch tensors on the GPU instead of numpy arrays."""
    return _organised_batch("world_points", pyramids, poses, level, min_depth, max_depth, device)


def _organised_batch(name, pyramids, poses, level, min_depth, max_depth, device):
    """world_points_batch() and normals_batch(): dvo_hip_frames_<name> into one [h, w, 4] float32 array per pyramid"""
    n, T = _map_frames_args(pyramids, poses, level, min_depth, max_depth, name + "_batch")
    ctx = pyramids[0].ctx
    (out,), (ptrs,) = _level_outputs(pyramids, level, 1, (4,), device)
    ctx.check(getattr(ctx._lib, "dvo_hip_frames_" + name)(ctx.ptr, n, _handles(pyramids), T.ctypes.data_as(C.POINTER(C.c_double)), int(level),
                                                          float(min_depth), float(max_depth), ptrs, 1 if device else 0))
    return out


def normals_batch(pyramids, poses, level=0, min_depth=0.0, max_depth=float("inf"), device=False):
    """The organised planes of world normals of n keyframes (dvo_hip_frames_normals; dvo_slam_amd/csrc/cloud_normal.h): per pyramid an
    [h, w, 4] float32 array {N.x, N.y, N.z, has} of level `level` under its 4 x 4 pose (camera -> world) -- the side of the surface that
    faces the camera, from the level's own depth plane; has is 1 where the pixel has a normal, else 0 and N is 0 (the border, unusable
    pixels, a neighbour without depth, a surface seen at a grazing angle or across a depth step).  Exactly what an insertion into
    KeyframeMap(normals=True) sees.  device=True: torch tensors on the GPU instead of numpy arrays."""
    return _organised_batch("normals", pyramids, poses, level, min_depth, max_depth, device)


_WARP_POSES = dict(per="item", counted="items", maps="source camera -> target camera", finite=True)   # warp_inverse_batch, warp_forward_batch


def warp_params_struct(mode="splat", occlusion_margin=0.05, min_depth=0.0, max_depth=float("inf")):
    """dvo_hip_warp_params from its fields (the defaults: dvo_hip_warp_params_default), or ValueError / TypeError: nothing reaches the
    library with a value it would refuse."""
    if not isinstance(mode, str):
        raise TypeError("warp: mode is a name, one of %s" % sorted(_lib.WARP_MODES))
    if mode not in _lib.WARP_MODES:
        raise ValueError("warp: unknown mode %r; known: %s" % (mode, sorted(_lib.WARP_MODES)))
    try:
        margin, lo, hi = float(occlusion_margin), float(min_depth), float(max_depth)
    except (TypeError, ValueError):
        raise TypeError("warp: occlusion_margin, min_depth and max_depth must be real numbers")
    if not margin >= 0.0:
        raise ValueError("warp: the occlusion margin must be >= 0 (no NaN)")
    if not lo <= hi:
        raise ValueError("warp: need min_depth <= max_depth (no NaN)")
    out = _lib.WarpParams()
    out.mode, out.occlusion_margin, out.min_depth, out.max_depth = _lib.WARP_MODES[mode], margin, lo, hi
    return out


def _warp_args(pyramids, others, transforms, level, who):
    """(n, transforms as a contiguous [n, 4, 4] float64 array) of a warp call, or ValueError / TypeError: nothing reaches the library with
    no items, mismatched lengths, a transform that is not 4 x 4 or not finite, a level a pyramid does not have, pyramids of different
    contexts or -- others: the second pyramid of every pair -- a pair whose sizes differ."""
    n = len(pyramids)

    def counts_and_transforms():
        if others is not None and len(others) != n:
            raise ValueError("%s: %d raster pyramids but %d sampled pyramids" % (who, n, len(others)))
        return _pose_array(transforms, n, who, **_WARP_POSES)

    T = _pyramids_at_level(pyramids, level, who, then=counts_and_transforms, others=others or ())
    for p, q in zip(pyramids, others or []):
        if (p.camera.width, p.camera.height) != (q.camera.width, q.camera.height):
            raise ValueError("%s: the pyramids of a pair differ in size" % who)
    return n, T


def _warp_planes(pyramids, level, count, device):
    """count lists of one [h, w] float32 output plane per pyramid, and their pointer arrays"""
    return _level_outputs(pyramids, level, count, (), device)


def warp_inverse_batch(raster_pyramids, sampled_pyramids, transforms, level=0, occlusion_margin=0.05, difference=False, device=False):
    """The sampled images seen in the raster images' pixel grids (dvo_hip_frames_warp_inverse; the reference's RgbdImage::warpIntensity
    with Interpolation::bilinearWithDepthBuffer).  Item i: every pixel of raster_pyramids[i] with depth is carried by transforms[i]
    (4 x 4, the raster camera -> the sampled camera) into sampled_pyramids[i] and takes its bilinear intensity there, over the taps that
    are not nearer than the point by more than occlusion_margin.  Returns (I, Z) -- with difference=True (I, Z, D), D = I - the raster
    image -- lists of one [h, w] float32 array of level `level` per item; NaN where a pixel has no depth, lands outside the image or
    behind the camera, or has no tap that counts.  device=True: torch tensors on the GPU instead of numpy arrays.
    Result.transformation is current -> reference: to see the current image in the reference's raster pass the reference pyramid as
    raster, the current one as sampled and numpy.linalg.inv(result.transformation)."""
    who = "warp_inverse_batch"
    n, T = _warp_args(raster_pyramids, sampled_pyramids, transforms, level, who)
    params = warp_params_struct(occlusion_margin=occlusion_margin)
    ctx = raster_pyramids[0].ctx
    out, ptrs = _warp_planes(raster_pyramids, level, 3 if difference else 2, device)
    ctx.check(ctx._lib.dvo_hip_frames_warp_inverse(ctx.ptr, n, _handles(raster_pyramids), _handles(sampled_pyramids),
                                                   T.ctypes.data_as(C.POINTER(C.c_double)), int(level), C.byref(params), ptrs[0], ptrs[1],
                                                   ptrs[2] if difference else None, 1 if device else 0))
    return tuple(out)


def warp_forward_batch(pyramids, transforms, level=0, mode="splat", min_depth=0.0, max_depth=float("inf"), device=False):
    """The images the frames predict at other poses (dvo_hip_frames_warp_forward; the reference's RgbdImage::warpDepthForwardAdvanced --
    mode "splat" -- and warpDepthForward / warpIntensityForward -- mode "nearest").  Item i: every pixel of pyramids[i] with a depth
    in [min_depth, max_depth] is carried by transforms[i] (4 x 4, the frame's camera -> the target camera) and drawn into a target of
    the frame's own size and intrinsics, the nearest surface per pixel.  Returns (I, Z), lists of one [h, w] float32 array of level
    `level` per item: depth in metres (NaN where nothing landed) and that surface's intensity (0 there) -- planes
    update_f32_device_batch takes.  device=True: torch tensors on the GPU instead of numpy arrays."""
    who = "warp_forward_batch"
    n, T = _warp_args(pyramids, None, transforms, level, who)
    params = warp_params_struct(mode=mode, min_depth=min_depth, max_depth=max_depth)
    ctx = pyramids[0].ctx
    out, ptrs = _warp_planes(pyramids, level, 2, device)
    ctx.check(ctx._lib.dvo_hip_frames_warp_forward(ctx.ptr, n, _handles(pyramids), T.ctypes.data_as(C.POINTER(C.c_double)), int(level),
                                                   C.byref(params), ptrs[0], ptrs[1], 1 if device else 0))
    return tuple(out)


COVIS_DTYPE = np.dtype(_lib.COVIS_RECORD)                         # dvo_hip_covis_record: 32 bytes
COVIS_MAX_PAIRS = 1 << 22                                         # what one dvo_hip_frames_covisibility call takes
_COVIS_POSES = dict(per="pair", counted="pairs", maps="a's camera -> b's camera", finite=True)   # covisibility_batch


def covis_params_struct(depth_tolerance=0.05, depth_tolerance_rel=0.0, min_depth=0.0, max_depth=float("inf")):
    """dvo_hip_covis_params from its fields (the defaults: dvo_hip_covis_params_default), or ValueError / TypeError: nothing reaches the
    library with a value it would refuse."""
    try:
        tol, rel, lo, hi = float(depth_tolerance), float(depth_tolerance_rel), float(min_depth), float(max_depth)
    except (TypeError, ValueError):
        raise TypeError("covisibility: depth_tolerance, depth_tolerance_rel, min_depth and max_depth must be real numbers")
    if not tol >= 0.0 or not rel >= 0.0:
        raise ValueError("covisibility: the depth tolerances must be >= 0 (no NaN)")
    if not lo <= hi:
        raise ValueError("covisibility: need min_depth <= max_depth (no NaN)")
    out = _lib.CovisParams()
    out.depth_tolerance, out.depth_tolerance_rel, out.min_depth, out.max_depth = tol, rel, lo, hi
    return out


def _covis_args(pyramids, pairs, transforms, level, who):
    """(pairs as a contiguous [n, 2] int32 array, transforms as a contiguous [n, 4, 4] float64 array) of a covisibility call, or
    ValueError / TypeError: nothing reaches the library with no pyramids or pairs, too many pairs, an index that names no pyramid, a
    transform that is not 4 x 4 or not finite, a level a pyramid does not have or pyramids of different contexts."""
    def pairs_and_transforms():
        try:
            P = np.asarray(pairs)
        except (TypeError, ValueError):
            raise TypeError("%s: pairs must be integers, one (a, b) per pair" % who)
        if P.dtype == bool or not np.issubdtype(P.dtype, np.integer):
            if P.size or P.dtype == bool:
                raise TypeError("%s: pairs must be integers, one (a, b) per pair" % who)
        if P.ndim == 1 and P.shape[0] == 2:
            P = P[None]
        if P.ndim != 2 or P.shape[1] != 2 or P.shape[0] < 1:
            raise ValueError("%s: pairs is an [n, 2] array of indices (a, b), n >= 1, got shape %s" % (who, P.shape))
        if P.shape[0] > COVIS_MAX_PAIRS:
            raise ValueError("%s: %d pairs, one call takes %d" % (who, P.shape[0], COVIS_MAX_PAIRS))
        if P.min() < 0 or P.max() >= len(pyramids):
            raise ValueError("%s: a pair names a pyramid outside 0 .. %d" % (who, len(pyramids) - 1))
        T = _pose_array(transforms, P.shape[0], who, **_COVIS_POSES)
        return np.ascontiguousarray(P, np.int32), T

    return _pyramids_at_level(pyramids, level, who, then=pairs_and_transforms)


def covisibility_batch(pyramids, pairs, transforms, level=2, depth_tolerance=0.05, depth_tolerance_rel=0.0, min_depth=0.0,
                       max_depth=float("inf"), device=False):
    """How much of one keyframe's surface another keyframe also sees, for many ordered pairs in one launch
    (dvo_hip_frames_covisibility; dvo_slam_amd/csrc/covisibility.h).  pairs: [n, 2] indices (a, b) into pyramids; transforms: [n, 4, 4],
    a's camera -> b's camera (for poses camera -> world: inv(pose_b) @ pose_a).  Every pixel of a with a depth in [min_depth, max_depth]
    counts as `valid`; carried into b's camera it is `in_view` when its nearest pixel lies in b's image, and there `unknown` (b has no
    depth), `occluded` (b sees a nearer surface), `seen_through` (b sees past it: a free-space conflict) or `consistent` (b's depth
    agrees within depth_tolerance + depth_tolerance_rel * depth), where `photo` sums |I_a - I_b| in sixteenths of a grey level.
    Returns a COVIS_DTYPE array of n records; device=True: a torch uint8 tensor [n, 32] on the GPU holding the same bytes.  a and b
    may differ in size and camera; a == b is allowed."""
    who = "covisibility_batch"
    P, T = _covis_args(pyramids, pairs, transforms, level, who)
    params = covis_params_struct(depth_tolerance, depth_tolerance_rel, min_depth, max_depth)
    ctx = pyramids[0].ctx
    n = P.shape[0]
    if device:
        import torch
        out = torch.empty((n, COVIS_DTYPE.itemsize), dtype=torch.uint8, device="cuda:%d" % ctx.device)
    else:
        out = np.empty(n, COVIS_DTYPE)
    a, b = np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(P[:, 1])
    i32p = C.POINTER(C.c_int32)
    ctx.check(ctx._lib.dvo_hip_frames_covisibility(ctx.ptr, len(pyramids), _handles(pyramids), n, a.ctypes.data_as(i32p), b.ctypes.data_as(i32p),
                                                   T.ctypes.data_as(C.POINTER(C.c_double)), int(level), C.byref(params),
                                                   C.c_void_p(_address(out)), 1 if device else 0))
    return out


def _covis_poses(pyramids, poses, who):
    """poses of keyframes as a [n, 4, 4] float64 array (camera -> world) and their inverses, or ValueError / TypeError"""
    if len(pyramids) < 1:
        raise ValueError("%s: no pyramids" % who)
    T = _pose_array(poses, len(pyramids), who, finite=True)
    try:
        return T, np.linalg.inv(T)
    except np.linalg.LinAlgError:
        raise ValueError("%s: a pose is singular" % who)


def covisibility_matrix(pyramids, poses, level=2, depth_tolerance=0.05, depth_tolerance_rel=0.0, min_depth=0.0, max_depth=float("inf"),
                        batch=None):
    """The covisibility of ALL ordered pairs of n keyframes under their poses ([n, 4, 4], camera -> world), the diagonal included, in
    one call: an [n, n] COVIS_DTYPE array whose entry [a, b] is a's surface as b sees it, T_ab = inv(pose_b) @ pose_a in float64 on the
    host.  overlap(M, M.T) is the symmetric overlap of every two keyframes.  batch: the function that counts (covisibility_batch; the
    tests put the host build of covisibility.h in its place)."""
    who = "covisibility_matrix"
    T, Tinv = _covis_poses(pyramids, poses, who)
    n = len(pyramids)
    a, b = (x.reshape(-1) for x in np.mgrid[0:n, 0:n])
    rec = (batch or covisibility_batch)(pyramids, np.stack([a, b], 1), Tinv[b] @ T[a], level=level, depth_tolerance=depth_tolerance,
                                        depth_tolerance_rel=depth_tolerance_rel, min_depth=min_depth, max_depth=max_depth)
    return np.asarray(rec).reshape(n, n)


def overlap(records_ab, records_ba):
    """min(consistent_ab / valid_a, consistent_ba / valid_b) in float64, elementwise: the share of each keyframe's surface the other one
    confirms, the smaller of the two -- 0 where either keyframe has no valid pixel."""
    ab, ba = np.asarray(records_ab), np.asarray(records_ba)
    if ab.dtype != COVIS_DTYPE or ba.dtype != COVIS_DTYPE:
        raise TypeError("overlap: records are COVIS_DTYPE arrays (covisibility_batch, covisibility_matrix)")
    if ab.shape != ba.shape:
        raise ValueError("overlap: the two directions differ in shape, %s and %s" % (ab.shape, ba.shape))

    def share(r):
        valid = r["valid"].astype(np.float64)
        return np.where(valid > 0, r["consistent"].astype(np.float64) / np.where(valid > 0, valid, 1.0), 0.0)

    both = (ab["valid"] > 0) & (ba["valid"] > 0)
    return np.where(both, np.minimum(share(ab), share(ba)), 0.0)


def radius_set(poses, query, max_distance):
    """The keyframes the reference's NearestNeighborConstraintSearch::findPossibleConstraints proposes for keyframe `query`: those whose
    translation lies within max_distance of the query's, the query itself included, in index order.  As the reference's radius search:
    float32 translations, squared distance <= max_distance squared."""
    t = np.ascontiguousarray(np.asarray(poses, np.float64)[:, :3, 3], np.float32)
    d = t - t[query]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.nonzero(d2 <= np.float32(float(max_distance) * float(max_distance)))[0]


def loop_closure_candidates(pyramids, poses, query, max_distance, min_overlap=0.0, level=2, depth_tolerance=0.05, depth_tolerance_rel=0.0,
                            min_depth=0.0, max_depth=float("inf"), batch=None):
    """The keyframes to validate keyframe `query` against: the reference's radius test on the translations (radius_set: the query itself
    passes it, as in the reference), then the covisibility of the survivors with the query in both directions, in ONE call, and of
    those the indices with overlap >= min_overlap, ordered by overlap descending and by index on ties.  poses: [n, 4, 4], camera ->
    world.  batch: as covisibility_matrix."""
    who = "loop_closure_candidates"
    T, Tinv = _covis_poses(pyramids, poses, who)
    n = len(pyramids)
    if isinstance(query, bool) or not isinstance(query, (int, np.integer)):
        raise TypeError("%s: query must be an integer" % who)
    if not 0 <= query < n:
        raise ValueError("%s: query names no pyramid of 0 .. %d" % (who, n - 1))
    try:
        radius, least = float(max_distance), float(min_overlap)
    except (TypeError, ValueError):
        raise TypeError("%s: max_distance and min_overlap must be real numbers" % who)
    if not radius >= 0.0:
        raise ValueError("%s: max_distance must be >= 0 (no NaN)" % who)
    if not 0.0 <= least <= 1.0:
        raise ValueError("%s: min_overlap is a share, 0 .. 1 (no NaN)" % who)
    covis_params_struct(depth_tolerance, depth_tolerance_rel, min_depth, max_depth)
    near = radius_set(T, query, radius)
    if near.size == 0:
        return np.zeros(0, np.int64)
    # the frames of the call: the survivors and the query, each once
    used = sorted(set(near.tolist()) | {int(query)})
    at = {k: i for i, k in enumerate(used)}
    q = np.full(near.size, at[int(query)])
    j = np.array([at[int(k)] for k in near])
    pairs = np.concatenate([np.stack([q, j], 1), np.stack([j, q], 1)])
    transforms = np.concatenate([Tinv[near] @ T[query], Tinv[query] @ T[near]])
    rec = np.asarray((batch or covisibility_batch)([pyramids[k] for k in used], pairs, transforms, level=level, depth_tolerance=depth_tolerance,
                                                   depth_tolerance_rel=depth_tolerance_rel, min_depth=min_depth, max_depth=max_depth))
    share = overlap(rec[:near.size], rec[near.size:])
    keep = share >= least
    order = np.lexsort((near[keep], -share[keep]))
    return near[keep][order].astype(np.int64)


FERN_DTYPE = np.dtype(_lib.FERN_RECORD)                            # dvo_hip_fern: 16 bytes
CODE_MATCH_DTYPE = np.dtype(_lib.CODE_MATCH_RECORD)                # dvo_hip_code_match: 8 bytes
CODE_NONE = 0xFFFFFFFF                                             # the id and the distance of a padding record
CODE_MASKED = 0xFFFF                                               # a dead or skipped entry in a distance matrix
CODE_MAX_K, CODE_MAX_QUERIES, CODE_MAX_CAPACITY = 64, 4096, 1 << 24


def _code_int(value, lo, hi, who, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError("%s: %s must be an integer" % (who, what))
    if not lo <= value <= hi:
        raise ValueError("%s: %s must be %d .. %d, got %d" % (who, what, lo, hi, value))
    return int(value)


class CodebookLogic:
    """What a keyframe code book does ABOVE its primitive calls (dvo_slam_amd/csrc/keyframe_codes.h): argument checks, harvesting, growth,
    save and load.  KeyframeCodebook puts the device calls under it; the CPU tests put the host build of the header there.  A subclass
    provides _open(m, capacity, seed, ferns) and _shut(), info(), ferns(), encode(), _add_frames(), _add_codes(), _remove(), codes() and
    _query(kind, what, level, k, skip_from, skip_to, distances, device)."""

    def __init__(self, ctx=None, m=512, capacity=4096, seed=0, ferns=None, z_lo=0.5, z_hi=5.0):
        who = type(self).__name__
        self.m = _code_int(m, 128, 2048, who, "m")
        if self.m % 128:
            raise ValueError("%s: m must be a multiple of 128, got %d" % (who, self.m))
        self.capacity = _code_int(capacity, 1, CODE_MAX_CAPACITY, who, "capacity")
        self.seed = _code_int(seed, 0, (1 << 64) - 1, who, "seed")
        self.z_range = (float(z_lo), float(z_hi))
        if ferns is None:
            if not (np.isfinite(self.z_range[0]) and np.isfinite(self.z_range[1]) and self.z_range[0] <= self.z_range[1]):
                raise ValueError("%s: need finite z_lo <= z_hi" % who)
        else:
            ferns = np.ascontiguousarray(ferns)
            if ferns.dtype != FERN_DTYPE or ferns.shape != (self.m,):
                raise ValueError("%s: ferns is a FERN_DTYPE array of m = %d entries" % (who, self.m))
        self.ctx = ctx
        self._dead = set()
        self._open(self.m, self.capacity, self.seed, ferns)

    words = property(lambda self: self.m // 8)
    size = property(lambda self: self.info()["size"])
    live = property(lambda self: self.info()["live"])

    def _codes_arg(self, codes, who):
        """raw codes as a contiguous [n, m / 8] uint32 array (one code: [m / 8]), or a torch tensor of that shape left as it is"""
        if hasattr(codes, "data_ptr"):
            if codes.dim() == 1:
                codes = codes[None]
            if codes.dim() != 2 or codes.shape[1] != self.words or codes.element_size() != 4 or not codes.is_contiguous() or codes.shape[0] < 1:
                raise ValueError("%s: device codes are a contiguous [n, %d] tensor of 32-bit words" % (who, self.words))
            return codes
        A = np.asarray(codes)
        if A.dtype != np.uint32:
            raise TypeError("%s: codes are uint32 words" % who)
        if A.ndim == 1:
            A = A[None]
        if A.ndim != 2 or A.shape[1] != self.words or A.shape[0] < 1:
            raise ValueError("%s: codes are an [n, %d] array, n >= 1, got shape %s" % (who, self.words, A.shape))
        return np.ascontiguousarray(A)

    def _ids_arg(self, ids, who, limit=None):
        A = np.atleast_1d(np.asarray(ids))
        if A.dtype == bool or not np.issubdtype(A.dtype, np.integer) or A.ndim != 1 or A.size < 1:
            raise TypeError("%s: ids are a list of integers, at least one" % who)
        size = self.size
        if A.min() < 0 or A.max() >= size:
            raise ValueError("%s: an id outside 0 .. %d" % (who, size - 1))
        if limit is not None and A.size > limit:
            raise ValueError("%s: %d ids, one call takes %d" % (who, A.size, limit))
        return np.ascontiguousarray(A, np.uint32)

    def _frames_arg(self, pyramids, level, who, limit=None):
        _pyramids_at_level(pyramids, level, who, limit=limit, ctx=False if self.ctx is None else self.ctx,
                           foreign="a pyramid of another context than the book's")
        return list(pyramids)

    def _query_args(self, n, k, skip, who):
        k = _code_int(k, 1, CODE_MAX_K, who, "k")
        if n > CODE_MAX_QUERIES:
            raise ValueError("%s: %d queries, one call takes %d" % (who, n, CODE_MAX_QUERIES))
        if skip is None:
            return k, None, None
        S = np.asarray(skip)
        if S.dtype == bool or not np.issubdtype(S.dtype, np.integer) or S.shape != (n, 2):
            raise ValueError("%s: skip is an [n, 2] array of integers (from, to), one row per query" % who)
        S = np.clip(S.astype(np.int64), 0, CODE_NONE)
        return k, np.ascontiguousarray(S[:, 0], np.uint32), np.ascontiguousarray(S[:, 1], np.uint32)

    def _room(self, n, who):
        if n > self.capacity - self.size:
            raise DvoHipError(_lib.ERR_CAPACITY, "%s: the book is full (capacity %d); grown() gives a larger one" % (who, self.capacity))

    # ---- entries -------------------------------------------------------------------------------------------------------------------------

    def add(self, pyramids, level):
        """Encodes the pyramids at `level` into the book's next slots; returns their ids (uint32).  DvoHipError ERR_CAPACITY when they do
        not fit: nothing is added."""
        frames = self._frames_arg(pyramids, level, "add")
        self._room(len(frames), "add")
        return self._add_frames(frames, int(level))

    def add_codes(self, codes):
        """Raw codes ([n, m / 8] uint32, or a torch tensor on the GPU) into the next slots: codes of another book with the same ferns."""
        A = self._codes_arg(codes, "add_codes")
        self._room(A.shape[0], "add_codes")
        return self._add_codes(A)

    def remove(self, ids):
        """The entries die: no answer names them again, their ids are not given again."""
        A = self._ids_arg(ids, "remove")
        self._remove(A)
        self._dead.update(int(i) for i in A)

    def dead(self):
        """the ids removed so far, ascending"""
        return np.array(sorted(self._dead), np.uint32)

    # ---- queries -------------------------------------------------------------------------------------------------------------------------

    def query(self, pyramids, level, k=1, skip=None, distances=False, device=False):
        """Per pyramid, encoded at `level`, the k live entries of least (distance, id): a CODE_MATCH_DTYPE array [n, k], padded with
        (CODE_NONE, CODE_NONE); skip: [n, 2] ids (from, to) left out per query, from <= id < to.  distances=True: (rows, D) with D the
        [n, size] uint16 matrix, CODE_MASKED where dead or skipped.  device=True: torch tensors on the GPU with the same bits -- the rows
        an int32 tensor [n, 2 k] with id and distance interleaved, the matrix an int16 tensor."""
        frames = self._frames_arg(pyramids, level, "query", CODE_MAX_QUERIES)
        k, lo, hi = self._query_args(len(frames), k, skip, "query")
        return self._query("frames", frames, int(level), k, lo, hi, bool(distances), bool(device))

    def query_codes(self, codes, k=1, skip=None, distances=False, device=False):
        """query() for raw codes"""
        A = self._codes_arg(codes, "query_codes")
        k, lo, hi = self._query_args(A.shape[0], k, skip, "query_codes")
        return self._query("codes", A, None, k, lo, hi, bool(distances), bool(device))

    def query_ids(self, ids, k=1, skip=None, distances=False, device=False):
        """query() for the book's own entries (dead ones may ask too); skip usually leaves out each entry's neighbours in time"""
        A = self._ids_arg(ids, "query_ids", CODE_MAX_QUERIES)
        k, lo, hi = self._query_args(A.shape[0], k, skip, "query_ids")
        return self._query("ids", A, None, k, lo, hi, bool(distances), bool(device))

    def distance_matrix(self, device=False):
        """All entries against all: [size, size] uint16, CODE_MASKED in the rows' dead columns (a dead entry's row is computed like any
        other), in rounds of CODE_MAX_QUERIES queries."""
        size = self.size
        if size < 1:
            return np.zeros((0, 0), np.uint16)
        parts = [self.query_ids(np.arange(q0, min(q0 + CODE_MAX_QUERIES, size)), k=1, distances=True, device=device)[1]
                 for q0 in range(0, size, CODE_MAX_QUERIES)]
        if len(parts) == 1:
            return parts[0]
        if device:
            import torch
            return torch.cat(parts)
        return np.concatenate(parts)

    def harvest(self, pyramid, level, min_distance):
        """Glocker's keyframe harvesting: the pyramid enters the book only if its nearest live code is at least min_distance ferns away
        (or the book has none).  Returns the new id, or None."""
        min_distance = _code_int(min_distance, 0, self.m + 1, "harvest", "min_distance")
        frames = self._frames_arg([pyramid], level, "harvest")
        code = self.encode(frames, level)
        if self.live > 0:
            nearest = self.query_codes(code, k=1)[0, 0]
            if nearest["id"] != CODE_NONE and nearest["distance"] < min_distance:
                return None
        return int(self.add_codes(code)[0])

    # ---- growth, save and load -------------------------------------------------------------------------------------------------------------

    def _like(self, capacity):
        return type(self)(self.ctx, m=self.m, capacity=capacity, seed=self.seed, ferns=self.ferns())

    def _refill(self, book, codes, dead):
        if len(codes):
            book.add_codes(codes)
        if len(dead):
            book.remove(dead)
        return book

    def grown(self, capacity=None):
        """A new book of `capacity` (default: twice this one's) with the same ferns, the same codes under the same ids, and the same
        entries dead: read_codes + add_codes.  This book is left as it is."""
        capacity = 2 * self.capacity if capacity is None else _code_int(capacity, max(self.size, 1), CODE_MAX_CAPACITY, "grown", "capacity")
        return self._refill(self._like(min(capacity, CODE_MAX_CAPACITY)), self.codes(), self.dead())

    def save(self, path):
        """m, the ferns, the codes and the dead ids as one .npz file"""
        with open(path, "wb") as f:
            np.savez(f, m=np.int64(self.m), capacity=np.int64(self.capacity), ferns=self.ferns(), codes=self.codes(), dead=self.dead())

    @classmethod
    def load(cls, path, ctx=None, capacity=None):
        """the book save() wrote, with at least its capacity"""
        with np.load(path) as z:
            m, ferns, codes, dead = int(z["m"]), z["ferns"], z["codes"], z["dead"]
            capacity = int(z["capacity"]) if capacity is None else capacity
        book = cls(ctx, m=m, capacity=max(capacity, len(codes), 1), ferns=ferns.astype(FERN_DTYPE))
        return book._refill(book, codes.astype(np.uint32).reshape(-1, m // 8), dead)


class KeyframeCodebook(CodebookLogic):
    """Keyframes retrieved by APPEARANCE, on the device (dvo_hip_codebook_*; Glocker et al., TVCG 2015): a frame becomes m 4-bit fern tests on
    a coarse pyramid level, similar views have codes that differ in few ferns, and a query is a search over all stored codes -- what
    names the keyframes to re-align against when no pose can be trusted (a lost tracker, a loop that closes after drift, two sessions to
    join).  ids are given in the order of adding.  ferns: a FERN_DTYPE table of the caller's, else fern_table(seed) of keyframe_codes.h."""

    def __init__(self, ctx=None, m=512, capacity=4096, seed=0, ferns=None, z_lo=0.5, z_hi=5.0):
        super().__init__(ctx or default_context(), m, capacity, seed, ferns, z_lo, z_hi)

    def _open(self, m, capacity, seed, ferns):
        self.ptr = C.c_void_p()
        table = None if ferns is None else C.c_void_p(ferns.ctypes.data)
        self.ctx.check(self.ctx._lib.dvo_hip_codebook_create(self.ctx.ptr, m, capacity, seed, table, self.z_range[0], self.z_range[1], C.byref(self.ptr)))

    def info(self):
        v = [C.c_int() for _ in range(4)]
        self.ctx.check(self.ctx._lib.dvo_hip_codebook_info(self.ctx.ptr, self.ptr, *[C.byref(x) for x in v]))
        return dict(zip(("m", "capacity", "size", "live"), (x.value for x in v)))

    def ferns(self):
        out = np.empty(self.m, FERN_DTYPE)
        self.ctx.check(self.ctx._lib.dvo_hip_codebook_ferns(self.ctx.ptr, self.ptr, C.c_void_p(out.ctypes.data)))
        return out

    def clear(self):
        self.ctx.check(self.ctx._lib.dvo_hip_codebook_clear(self.ctx.ptr, self.ptr))
        self._dead = set()

    def encode(self, pyramids, level, device=False):
        """The codes of the pyramids at `level` under the book's ferns, [n, m / 8] uint32 (device=True: a torch int32 tensor on the GPU);
        the book is not changed."""
        frames = self._frames_arg(pyramids, level, "encode")
        out = _out_array(self.ctx, (len(frames), self.words), np.uint32, device)
        self.ctx.check(self.ctx._lib.dvo_hip_frames_encode(self.ctx.ptr, self.ptr, len(frames), _handles(frames), int(level), C.c_void_p(_address(out)),
                                                           1 if device else 0))
        return out

    def _add_frames(self, frames, level):
        ids = np.empty(len(frames), np.uint32)
        self.ctx.check(self.ctx._lib.dvo_hip_codebook_add_frames(self.ctx.ptr, self.ptr, len(frames), _handles(frames), level,
                                                                 ids.ctypes.data_as(C.POINTER(C.c_uint32))))
        return ids

    def _add_codes(self, codes):
        ids = np.empty(codes.shape[0], np.uint32)
        self.ctx.check(self.ctx._lib.dvo_hip_codebook_add_codes(self.ctx.ptr, self.ptr, codes.shape[0], C.c_void_p(_address(codes)),
                                                                1 if hasattr(codes, "data_ptr") else 0, ids.ctypes.data_as(C.POINTER(C.c_uint32))))
        return ids

    def _remove(self, ids):
        self.ctx.check(self.ctx._lib.dvo_hip_codebook_remove(self.ctx.ptr, self.ptr, ids.size, ids.ctypes.data_as(C.POINTER(C.c_uint32))))

    def codes(self, first=0, n=None, device=False):
        """the stored codes of entries first .. first + n - 1 (default: all), dead ones included: [n, m / 8] uint32"""
        size = self.size
        first = _code_int(first, 0, size, "codes", "first")
        n = size - first if n is None else _code_int(n, 0, size - first, "codes", "n")
        out = _out_array(self.ctx, (n, self.words), np.uint32, device)
        if n > 0:
            self.ctx.check(self.ctx._lib.dvo_hip_codebook_read_codes(self.ctx.ptr, self.ptr, first, n, C.c_void_p(_address(out)), 1 if device else 0))
        return out

    def _query(self, kind, what, level, k, skip_from, skip_to, distances, device):
        L, u32p = self.ctx._lib, C.POINTER(C.c_uint32)
        n = len(what)
        # (device rows: an int32 tensor [n, 2 k], id and distance interleaved -- the bytes of the [n, k] records)
        rows = _out_array(self.ctx, (n, 2 * k), np.uint32, True) if device else np.empty((n, k), CODE_MATCH_DTYPE)
        D = _out_array(self.ctx, (n, self.size), np.uint16, device) if distances else None
        lo = None if skip_from is None else skip_from.ctypes.data_as(u32p)
        hi = None if skip_to is None else skip_to.ctypes.data_as(u32p)
        tail = (k, lo, hi, C.c_void_p(_address(rows)), None if D is None else C.c_void_p(_address(D)), 1 if device else 0)
        if kind == "frames":
            rc = L.dvo_hip_codebook_query_frames(self.ctx.ptr, self.ptr, n, _handles(what), level, *tail)
        elif kind == "codes":
            rc = L.dvo_hip_codebook_query_codes(self.ctx.ptr, self.ptr, n, C.c_void_p(_address(what)), 1 if hasattr(what, "data_ptr") else 0, *tail)
        else:
            rc = L.dvo_hip_codebook_query_ids(self.ctx.ptr, self.ptr, n, what.ctypes.data_as(u32p), *tail)
        self.ctx.check(rc)
        return (rows, D) if distances else rows

    def _shut(self):
        if getattr(self, "ptr", None) and self.ctx.ptr:
            self.ctx._lib.dvo_hip_codebook_destroy(self.ctx.ptr, self.ptr)
        self.ptr = None

    def close(self):
        self._shut()

    def __del__(self):
        try:
            self._shut()
        except Exception:
            pass


def _candidate_lists(rows, max_distance):
    """per row of a query's answer the (id, distance) list, best first, without padding and without what lies beyond max_distance"""
    rows = np.asarray(rows)
    return [[(int(r["id"]), int(r["distance"])) for r in row
             if r["id"] != CODE_NONE and (max_distance is None or r["distance"] <= max_distance)] for row in rows]


def relocalisation_candidates(book, pyramids, level, k=4, max_distance=None):
    """The keyframes to re-align a frame against when its pose cannot be trusted: per pyramid the (id, distance) list of the k stored
    codes nearest to its code at `level`, best first, those beyond max_distance ferns left out.  The recovery recipe: match_batch from
    the identity against the candidates, then covisibility_batch under the pose found to accept or reject."""
    if max_distance is not None:
        max_distance = _code_int(max_distance, 0, book.m, "relocalisation_candidates", "max_distance")
    return _candidate_lists(book.query(pyramids, level, k=k), max_distance)


def loop_closure_candidates_by_appearance(book, ids, window, k=4, max_distance=None):
    """Loop-closure candidates WITHOUT poses: per listed entry of the book the (id, distance) list of the k nearest stored codes, best
    first, with the entry's neighbours in time -- ids within `window` of its own, itself included -- skipped, and those beyond
    max_distance ferns left out.  loop_closure_candidates (radius test + covisibility) stays the proposal where poses can be trusted."""
    who = "loop_closure_candidates_by_appearance"
    window = _code_int(window, 0, CODE_MAX_CAPACITY, who, "window")
    if max_distance is not None:
        max_distance = _code_int(max_distance, 0, book.m, who, "max_distance")
    A = np.atleast_1d(np.asarray(ids)).astype(np.int64)
    skip = np.stack([np.maximum(A - window, 0), A + window + 1], 1)
    return _candidate_lists(book.query_ids(ids, k=k, skip=skip), max_distance)


def _rehash_capacity(capacity):
    """the capacity_slots of dvo_hip_map_rehash (None: 0, keep), or ValueError / TypeError"""
    if capacity is None:
        return 0
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)):
        raise TypeError("KeyframeMap.rehash: capacity must be an integer (or None: as it is)")
    capacity = int(capacity)
    if not 64 <= capacity <= 1 << 32 or capacity & (capacity - 1):
        raise ValueError("KeyframeMap.rehash: capacity must be a power of two, 64 .. 2^32")
    return capacity


RENDER_DEFAULTS = dict(min_depth=0.0, max_depth=float("inf"), splat=2.0, max_splat=7, min_points=1)   # dvo_hip_render_params_default


def render_params_struct(**params):
    """dvo_hip_render_params from keyword arguments (min_depth, max_depth, splat, max_splat, min_points; the rest as
    dvo_hip_render_params_default gives them), or ValueError / TypeError: nothing reaches the library with a value it would refuse."""
    unknown = set(params) - set(RENDER_DEFAULTS)
    if unknown:
        raise TypeError("render: unknown parameter(s) %s; known: %s" % (sorted(unknown), sorted(RENDER_DEFAULTS)))
    p = dict(RENDER_DEFAULTS, **params)
    for k in ("max_splat", "min_points"):
        if isinstance(p[k], bool) or not isinstance(p[k], (int, np.integer)):
            raise TypeError("render: %s must be an integer" % k)
    lo, hi, splat = float(p["min_depth"]), float(p["max_depth"]), float(p["splat"])
    if not lo <= hi:
        raise ValueError("render: need min_depth <= max_depth (no NaN)")
    if not 0.0 < splat <= 4.0:
        raise ValueError("render: splat must lie in (0, 4]")
    if not 1 <= p["max_splat"] <= 15 or p["max_splat"] % 2 == 0:
        raise ValueError("render: max_splat must be odd, 1 .. 15")
    if not 1 <= p["min_points"] < 1 << 32:
        raise ValueError("render: min_points must be at least 1")
    out = _lib.RenderParams()
    out.min_depth, out.max_depth, out.splat, out.max_splat, out.min_points = lo, hi, splat, int(p["max_splat"]), int(p["min_points"])
    return out


def _render_view_args(K, width, height, poses, who):
    """(K as float32[4], width, height, poses [n, 4, 4]) of KeyframeMap.render, or ValueError / TypeError"""
    for name, v in (("width", width), ("height", height)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("%s: %s must be an integer" % (who, name))
        if not 1 <= v <= 1 << 24:
            raise ValueError("%s: %s must be positive (and at most 2^24)" % (who, name))
    try:
        K = np.ascontiguousarray(K, dtype=np.float32)
    except (TypeError, ValueError):
        raise TypeError("%s: K must be four real numbers fx, fy, ox, oy" % who)
    if K.shape != (4,):
        raise ValueError("%s: K is fx, fy, ox, oy, got shape %s" % (who, K.shape))
    if not np.all(np.isfinite(K)) or not (K[0] > 0 and K[1] > 0):
        raise ValueError("%s: K must be finite with fx > 0 and fy > 0" % who)
    T = _pose_array(poses, None, who, **_VIEW_POSES)
    if int(width) * int(height) * T.shape[0] > (1 << 31) - 1:
        raise ValueError("%s: more than 2^31 - 1 pixels in one call" % who)
    return K, int(width), int(height), T


def _record_array(a, fields, words, who, what):
    """(address, number of records, on the device?) of a record array: a structured numpy array with the fields of the header -- made
    contiguous here, and kept alive by the caller's reference for the duration of the call -- or a contiguous torch int32 tensor of shape
    [n, words] on the GPU"""
    if isinstance(a, np.ndarray):
        if a.dtype != np.dtype(fields) or a.ndim != 1:
            raise TypeError("%s: %s is a one-dimensional numpy array of dtype %s" % (who, what, np.dtype(fields)))
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("%s: %s must be contiguous" % (who, what))
        return a.ctypes.data, a.shape[0], False
    if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):
        import torch
        if not a.is_cuda or a.dtype != torch.int32 or a.dim() != 2 or a.shape[1] != words or not a.is_contiguous():
            raise TypeError("%s: device %s is a contiguous torch int32 tensor of shape [n, %d] on the GPU" % (who, what, words))
        if a.data_ptr() % 16 != 0:
            raise ValueError("%s: device %s must be 16-byte aligned" % (who, what))
        return a.data_ptr(), int(a.shape[0]), True
    raise TypeError("%s: %s is a structured numpy array (export()) or a torch tensor on the GPU (export(device=True))" % (who, what))


class KeyframeMap:
    """A voxel-grid map of keyframes on the device (dvo_hip_map_*; the reference's PointCloudAggregator::build with an exact per-voxel
    centroid): insert() fuses one level of n pyramids under their poses, extract() returns one point per occupied voxel.  The result
    does not depend on the order of insertion.  capacity: slots of the table, rounded up to a power of two; keep it at least four
    times the number of voxels (stats())."""

    def __init__(self, ctx=None, leaf=0.01, capacity=1 << 22, colour=False, normals=False):
        """colour=True (dvo_hip_map_create_ex, DVO_HIP_MAP_COLOUR): the map fuses the colour its pyramids carry
        (RgbdImagePyramid.set_colour) per voxel; every pyramid it is given must then carry colour.  normals=True (DVO_HIP_MAP_NORMALS):
        the map fuses the surface normal of every point that has one (normals_batch) per voxel; its export() returns a third array."""
        if not isinstance(colour, (bool, np.bool_)):
            raise TypeError("KeyframeMap: colour must be a bool")
        if not isinstance(normals, (bool, np.bool_)):
            raise TypeError("KeyframeMap: normals must be a bool")
        leaf = float(leaf)
        if not (leaf > 0.0 and leaf < float("inf")):
            raise ValueError("KeyframeMap: the leaf size must be finite and > 0")
        if int(capacity) < 1:
            raise ValueError("KeyframeMap: capacity must be positive")
        self.ctx = ctx or default_context()
        self.leaf = leaf
        self.coloured = bool(colour)
        self.with_normals = bool(normals)
        self.ptr = C.c_void_p()
        if self.coloured or self.with_normals:
            flags = (_lib.MAP_COLOUR if self.coloured else 0) | (_lib.MAP_NORMALS if self.with_normals else 0)
            self.ctx.check(self.ctx._lib.dvo_hip_map_create_ex(self.ctx.ptr, leaf, int(capacity), flags, C.byref(self.ptr)))
        else:
            self.ctx.check(self.ctx._lib.dvo_hip_map_create(self.ctx.ptr, leaf, int(capacity), C.byref(self.ptr)))

    def _check_colour_of(self, pyramids, who):
        if getattr(self, "coloured", False):
            for p in pyramids:
                if getattr(p, "_colour", None) is None:
                    raise ValueError("%s: a coloured map takes pyramids that carry colour (set_colour)" % who)

    def _update(self, name, pyramids, level, min_depth, max_depth, *poses):
        """insert(), remove() and move(): the checks, then dvo_hip_map_<name> with one pose array per element of `poses`"""
        who = "KeyframeMap." + name
        n, T = len(pyramids), [_map_frames_args(pyramids, p, level, min_depth, max_depth, who)[1] for p in poses]
        if pyramids[0].ctx is not self.ctx:
            raise ValueError("%s: the pyramids belong to another context than the map" % who)
        self._check_colour_of(pyramids, who)
        self.ctx.check(getattr(self.ctx._lib, "dvo_hip_map_" + name)(self.ctx.ptr, self.ptr, n, _handles(pyramids),
                                                                     *[t.ctypes.data_as(C.POINTER(C.c_double)) for t in T],
                                                                     int(level), float(min_depth), float(max_depth)))

    def insert(self, pyramids, poses, level=0, min_depth=0.0, max_depth=float("inf")):
        """Every usable point of `level` of the pyramids under their 4 x 4 poses (camera -> world).  Raises DvoHipError with code
        ERR_CAPACITY if the table dropped points; the map keeps what it took."""
        self._update("insert", pyramids, level, min_depth, max_depth, poses)

    def remove(self, pyramids, poses, level=0, min_depth=0.0, max_depth=float("inf")):
        """The inverse of insert() (dvo_hip_map_remove): the same pyramids -- with the content they had then -- poses, level and depth range
        take their points out of the map again, exactly.  Raises DvoHipError with code ERR_INVALID if points found no voxel to leave
        (stats()["unmatched"]) or if the map has dropped points since its last clear() or rehash()."""
        self._update("remove", pyramids, level, min_depth, max_depth, poses)

    def move(self, pyramids, poses_old, poses_new, level=0, min_depth=0.0, max_depth=float("inf")):
        """After a pose-graph optimisation (dvo_hip_map_move): the pyramids leave the map under poses_old and enter it under poses_new in
        one launch, bit for bit remove(poses_old) followed by insert(poses_new); a pyramid whose pose stays is skipped."""
        self._update("move", pyramids, level, min_depth, max_depth, poses_old, poses_new)

    def rehash(self, capacity=None):
        """Rebuilds the table (dvo_hip_map_rehash) with `capacity` slots, a power of two of at least 64 (None: as many as it has): vacant
        slots are reclaimed, the voxels keep their sums.  Raises DvoHipError with code ERR_CAPACITY, the map unchanged, if they do not fit."""
        capacity = _rehash_capacity(capacity)
        self.ctx.check(self.ctx._lib.dvo_hip_map_rehash(self.ctx.ptr, self.ptr, capacity))

    def clear(self):
        self.ctx.check(self.ctx._lib.dvo_hip_map_clear(self.ctx.ptr, self.ptr))

    def stats(self):
        """dict: occupied, points, dropped, out_of_range, unusable, over_limit, capacity, updates, vacant, removed, unmatched"""
        s = _lib.MapStats()
        self.ctx.check(self.ctx._lib.dvo_hip_map_stats(self.ctx.ptr, self.ptr, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in _lib.MapStats._fields_ if name != "reserved"}

    def extract(self, sort=False, device=False, max_points=None, colour=False, normals=False):
        """(xyzi [n, 4] float32, counts [n] uint32, keys [n] uint64): one record per occupied voxel, in no particular order unless
        sort=True (by key, on the host).  device=True: torch tensors on the GPU (counts as int32, keys as int64: the same bits).
        colour=True (a coloured map only): a fourth array rgba [n] uint32, 0xFFRRGGBB per voxel (device=True: int32, the same bits).
        normals=True (a map with normals only): one more array, last, [n, 4] float32: the voxel's unit normal in world coordinates and
        the agreement of the fused normals in [0, 1]; zeros for a voxel none of whose points had a normal."""
        if colour and not getattr(self, "coloured", False):
            raise ValueError("KeyframeMap.extract: the map holds no colour (KeyframeMap(colour=True))")
        if normals and not getattr(self, "with_normals", False):
            raise ValueError("KeyframeMap.extract: the map holds no normals (KeyframeMap(normals=True))")
        if sort and device:
            raise ValueError("KeyframeMap.extract: sort=True orders on the host; extract to the host, or sort the device tensors by key")
        cap = self.stats()["occupied"] if max_points is None else int(max_points)
        got = C.c_size_t(0)
        m = max(cap, 1)
        xyzi, counts, keys = (_out_array(self.ctx, shape, dt, device) for shape, dt in (((m, 4), np.float32), (m, np.uint32), (m, np.uint64)))
        rgba = _out_array(self.ctx, m, np.uint32, device) if colour else None
        if normals:
            nrm = _out_array(self.ctx, (m, 4), np.float32, device)
            self.ctx.check(self.ctx._lib.dvo_hip_map_extract_normals(self.ctx.ptr, self.ptr, cap, _address(xyzi), _address(nrm),
                                                                     _address(rgba) if colour else None, _address(counts), _address(keys),
                                                                     1 if device else 0, C.byref(got)))
        elif colour:
            self.ctx.check(self.ctx._lib.dvo_hip_map_extract_colour(self.ctx.ptr, self.ptr, cap, _address(xyzi), _address(rgba), _address(counts),
                                                                    _address(keys), 1 if device else 0, C.byref(got)))
        else:
            self.ctx.check(self.ctx._lib.dvo_hip_map_extract(self.ctx.ptr, self.ptr, cap, _address(xyzi), _address(counts), _address(keys),
                                                             1 if device else 0, C.byref(got)))
        xyzi, counts, keys = xyzi[:got.value], counts[:got.value], keys[:got.value]
        extra = ([rgba[:got.value]] if colour else []) + ([nrm[:got.value]] if normals else [])
        if sort:
            order = np.argsort(keys, kind="stable")
            xyzi, counts, keys = xyzi[order], counts[order], keys[order]
            extra = [a[order] for a in extra]
        return (xyzi, counts, keys, *extra)

    # ---- sub-maps (dvo_hip_map_merge, _move_submaps, _export, _merge_records; dvo_slam_amd/csrc/cloud_map.h, Merge) ----

    def info(self):
        """dict: leaf (the float32 the map bins with), colour, capacity (dvo_hip_map_info); of a map with normals also normals=True (a
        map without them reports the three keys it always reported)"""
        leaf, flags, capacity = C.c_float(), C.c_uint(), C.c_uint64()
        self.ctx.check(self.ctx._lib.dvo_hip_map_info(self.ctx.ptr, self.ptr, C.byref(leaf), C.byref(flags), C.byref(capacity)))
        out = dict(leaf=float(leaf.value), colour=bool(flags.value & _lib.MAP_COLOUR), capacity=int(capacity.value))
        if flags.value & _lib.MAP_NORMALS:
            out["normals"] = True
        return out

    def _merge_sources(self, sources, poses, who):
        """(list of source maps, their poses as [n, 4, 4] float64 or None), or ValueError / TypeError: nothing reaches the library with a
        source it would refuse"""
        if isinstance(sources, KeyframeMap):
            sources = [sources]
        sources = list(sources)
        for s in sources:
            if not isinstance(s, KeyframeMap):
                raise TypeError("%s: a source is a KeyframeMap" % who)
            if s is self:
                raise ValueError("%s: a map cannot be merged into itself" % who)
            if getattr(s, "ptr", None) is None:
                raise ValueError("%s: a source map is closed" % who)
            if s.ctx is not self.ctx:
                raise ValueError("%s: a source map belongs to another context (export() there, absorb() here)" % who)
            if bool(getattr(s, "coloured", False)) != bool(getattr(self, "coloured", False)):
                raise ValueError("%s: a coloured and a grey map do not merge" % who)
            if bool(getattr(s, "with_normals", False)) != bool(getattr(self, "with_normals", False)):
                raise ValueError("%s: a map with normals and one without do not merge" % who)
            if poses is None and np.float32(s.leaf) != np.float32(self.leaf):
                raise ValueError("%s: a plain merge needs the destination's leaf size (a posed merge bins anew)" % who)
        T = None if poses is None else _pose_array(poses, len(sources), who, **_MERGE_POSES)
        return sources, T

    def merge(self, sources, signs=None, poses=None):
        """The voxel tables of other maps into this one in one launch (dvo_hip_map_merge).  poses None: a PLAIN merge -- same leaf; the
        result is bit for bit the map built from all their keyframes at once.  poses [n, 4, 4] (source -> this map's coordinates): a
        POSED merge -- every source voxel enters as its n points at its transformed centroid (the sub-map approximation).  signs: +1
        or -1 per source (None: all +1); -1 subtracts what a merge under the same pose added, exactly.  Raises DvoHipError with code
        ERR_CAPACITY if points were dropped, ERR_INVALID if points found no voxel to leave; the map keeps what the call did."""
        who = "KeyframeMap.merge"
        sources, T = self._merge_sources(sources, poses, who)
        n = len(sources)
        sg = None
        if signs is not None:
            signs = list(signs)
            if len(signs) != n:
                raise ValueError("%s: %d sources but %d signs" % (who, n, len(signs)))
            for s in signs:
                if isinstance(s, bool) or not isinstance(s, (int, np.integer)):
                    raise TypeError("%s: a sign is the integer +1 or -1" % who)
                if s not in (1, -1):
                    raise ValueError("%s: a sign is +1 or -1" % who)
            sg = (C.c_int * max(n, 1))(*[int(s) for s in signs])
        if n == 0:
            return
        self.ctx.check(self.ctx._lib.dvo_hip_map_merge(self.ctx.ptr, self.ptr, n, _handles(sources), sg,
                                                       None if T is None else T.ctypes.data_as(C.POINTER(C.c_double))))

    def subtract(self, sources, poses=None):
        """merge() with every sign -1: takes out what merge(sources, poses=poses) put in, exactly."""
        if isinstance(sources, KeyframeMap):
            sources = [sources]
        sources = list(sources)
        self.merge(sources, signs=[-1] * len(sources), poses=poses)

    def move_submaps(self, sources, poses_old, poses_new):
        """After a pose-graph optimisation (dvo_hip_map_move_submaps): the sub-maps leave this map under poses_old and enter it under
        poses_new in one launch, bit for bit subtract(poses_old) followed by merge(poses_new); a sub-map whose pose stays is skipped.
        No frame is read: the keyframes' pyramids may have been destroyed."""
        who = "KeyframeMap.move_submaps"
        if poses_old is None or poses_new is None:
            raise ValueError("%s: needs the old and the new poses" % who)
        sources, T_old = self._merge_sources(sources, poses_old, who)
        T_new = _pose_array(poses_new, len(sources), who, **_MERGE_POSES)
        if not sources:
            return
        dp = C.POINTER(C.c_double)
        self.ctx.check(self.ctx._lib.dvo_hip_map_move_submaps(self.ctx.ptr, self.ptr, len(sources), _handles(sources), T_old.ctypes.data_as(dp),
                                                              T_new.ctypes.data_as(dp)))

    def export(self, device=False):
        """(records, colour_records or None): the live voxels as raw records in no particular order (dvo_hip_map_export) -- structured
        numpy arrays with the fields key, n, sx, sy, sz, si, pad and (a coloured map) sr, sg, sb, pad.  device=True: torch int32 tensors
        of shape [n, 8] and [n, 4] on the GPU, the same bytes.  With info() they are the whole map: absorb() takes them back.
        A map with normals (dvo_hip_map_export_ex) returns THREE arrays: (records, colour_records or None, normal_records) -- the
        third with the fields snx, sny, snz, nn ([n, 4] on the GPU)."""
        coloured, with_normals = bool(getattr(self, "coloured", False)), bool(getattr(self, "with_normals", False))
        got = C.c_size_t(0)
        self.ctx.check(self.ctx._lib.dvo_hip_map_export(self.ctx.ptr, self.ptr, 0, None, None, 0, C.byref(got)))
        n = got.value
        records = _out_array(self.ctx, max(n, 1), _MAP_RECORD, device)
        colour = _out_array(self.ctx, max(n, 1), _MAP_COLOUR_RECORD, device) if coloured else None
        if not with_normals:
            if n > 0:
                self.ctx.check(self.ctx._lib.dvo_hip_map_export(self.ctx.ptr, self.ptr, n, _address(records), _address(colour) if coloured else None,
                                                                1 if device else 0, C.byref(got)))
            return records[:got.value], (colour[:got.value] if coloured else None)
        normals = _out_array(self.ctx, max(n, 1), _MAP_NORMAL_RECORD, device)
        if n > 0:
            self.ctx.check(self.ctx._lib.dvo_hip_map_export_ex(self.ctx.ptr, self.ptr, n, _address(records), _address(colour) if coloured else None,
                                                               _address(normals), 1 if device else 0, C.byref(got)))
        return records[:got.value], (colour[:got.value] if coloured else None), normals[:got.value]

    def absorb(self, records, colour=None, leaf=None, sign=1, pose=None, normals=None):
        """Raw voxel records -- what export() returned, here or in another context, or a table's raw dump -- into (sign +1) or out of
        (-1) the map (dvo_hip_map_merge_records).  leaf: the leaf size the records were binned with (None: this map's).  pose None:
        a plain merge, same leaf; a 4 x 4 pose (records' coordinates -> this map's): a posed one.  Equal keys are summed.
        normals: the normal records of export(), which a map with normals needs (dvo_hip_map_merge_records_ex) and no other takes."""
        who = "KeyframeMap.absorb"
        ptr, n, on_device = _record_array(records, _lib.MAP_RECORD, 8, who, "records")
        with_normals = bool(getattr(self, "with_normals", False))
        if with_normals and normals is None:
            raise ValueError("%s: a map with normals takes records with normal records" % who)
        if not with_normals and normals is not None:
            raise ValueError("%s: a map without normals takes no normal records" % who)
        nptr = None
        if normals is not None:
            nptr, nn, n_on_device = _record_array(normals, _lib.MAP_NORMAL_RECORD, 4, who, "normals")
            if nn != n or n_on_device != on_device:
                raise ValueError("%s: %d records but %d normal records (both on the host, or both on the device)" % (who, n, nn))
        coloured = bool(getattr(self, "coloured", False))
        if coloured and colour is None:
            raise ValueError("%s: a coloured map takes records with colour records" % who)
        if not coloured and colour is not None:
            raise ValueError("%s: a grey map takes no colour records" % who)
        cptr = None
        if colour is not None:
            cptr, cn, c_on_device = _record_array(colour, _lib.MAP_COLOUR_RECORD, 4, who, "colour")
            if cn != n or c_on_device != on_device:
                raise ValueError("%s: %d records but %d colour records (both on the host, or both on the device)" % (who, n, cn))
        if n > 1 << 32:
            raise ValueError("%s: at most 2^32 records" % who)
        if isinstance(sign, bool) or not isinstance(sign, (int, np.integer)):
            raise TypeError("%s: sign is the integer +1 or -1" % who)
        if sign not in (1, -1):
            raise ValueError("%s: sign is +1 or -1" % who)
        leaf = float(np.float32(self.leaf if leaf is None else leaf))
        if not (leaf > 0.0 and leaf < float("inf")):
            raise ValueError("%s: the leaf size must be finite and > 0" % who)
        if pose is None and np.float32(leaf) != np.float32(self.leaf):
            raise ValueError("%s: a plain merge needs the map's own leaf size (a posed merge bins anew)" % who)
        T = None if pose is None else _pose_array(pose, 1, who, **_MERGE_POSES)
        if n == 0:
            return
        Tp = None if T is None else T.ctypes.data_as(C.POINTER(C.c_double))
        if with_normals:
            self.ctx.check(self.ctx._lib.dvo_hip_map_merge_records_ex(self.ctx.ptr, self.ptr, n, ptr, cptr, nptr, 1 if on_device else 0, leaf, int(sign), Tp))
        else:
            self.ctx.check(self.ctx._lib.dvo_hip_map_merge_records(self.ctx.ptr, self.ptr, n, ptr, cptr, 1 if on_device else 0, leaf, int(sign), Tp))

    def save(self, path):
        """The map into a file (numpy.savez: leaf, flags, capacity and the exported records); KeyframeMap.load reads it back."""
        info = self.info()
        records, colour, *normals = self.export()
        flags = (_lib.MAP_COLOUR if info["colour"] else 0) | (_lib.MAP_NORMALS if info.get("normals") else 0)
        extra = dict(normals=normals[0]) if normals else {}        # (a map without normals writes the file it always wrote)
        with open(path, "wb") as f:
            np.savez(f, leaf=np.float32(info["leaf"]), flags=np.uint32(flags), capacity=np.uint64(info["capacity"]),
                     records=records, colour=colour if colour is not None else np.zeros(0, np.dtype(_lib.MAP_COLOUR_RECORD)), **extra)

    @classmethod
    def load(cls, path, ctx=None, capacity=None):
        """A new map with the voxels of a file written by save(); capacity None: the saved map's."""
        with np.load(path) as z:
            leaf, flags, saved_capacity = float(z["leaf"]), int(z["flags"]), int(z["capacity"])
            records, colour = z["records"], z["colour"]
            normals = z["normals"] if flags & _lib.MAP_NORMALS else None
        coloured = bool(flags & _lib.MAP_COLOUR)
        m = cls(ctx=ctx, leaf=leaf, capacity=saved_capacity if capacity is None else capacity, colour=coloured, normals=normals is not None)
        m.absorb(records, colour if coloured else None, normals=normals)
        return m

    def _render(self, name, first, K, width, height, poses, device, params):
        """render() and render_colour(): dvo_hip_map_<name> into planes of dtype `first` and float32 depth planes"""
        K, width, height, T = _render_view_args(K, width, height, poses, "KeyframeMap." + name)
        rp = render_params_struct(**params)
        n = T.shape[0]
        if device:
            pad = (width * height + 3) // 4 * 4             # (every view's plane 16-byte aligned: views apart by a multiple of 4 words)
            planes = [_out_array(self.ctx, n * pad, dt, True).as_strided((n, height, width), (pad, width, 1)) for dt in (first, np.float32)]
        else:
            planes = [_out_array(self.ctx, (n, height, width), dt, False) for dt in (first, np.float32)]
        ptrs = [device_pointer_array([_address(a[k]) for k in range(n)]) for a in planes]
        self.ctx.check(getattr(self.ctx._lib, "dvo_hip_map_" + name)(self.ctx.ptr, self.ptr, n, width, height, K.ctypes.data_as(C.POINTER(C.c_float)),
                                                                     T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rp), ptrs[0], ptrs[1],
                                                                     1 if device else 0))
        return tuple(planes)

    def render(self, K, width, height, poses, device=False, **params):
        """Views of the map (dvo_hip_map_render): the nearest voxel per pixel of a width x height pinhole camera K = fx, fy, ox, oy at
        each 4 x 4 pose (camera -> world).  Returns (I, Z), float32 arrays of shape (n, height, width): intensity (0 where nothing was
        seen) and depth in metres (NaN where nothing was seen).  device=True: torch tensors on the GPU, ordered on the context's stream.
        params: min_depth, max_depth, splat, max_splat, min_points (render_params_struct)."""
        return self._render("render", np.float32, K, width, height, poses, device, params)

    def render_colour(self, K, width, height, poses, device=False, **params):
        """Colour views of a coloured map (dvo_hip_map_render_colour): like render(), but returns (rgba, Z): uint32 words 0xFFRRGGBB of
        shape (n, height, width) -- 0 where nothing was seen -- and the depth planes, bit for bit render()'s.  device=True: torch
        tensors on the GPU (rgba as int32: the same bits)."""
        if not getattr(self, "coloured", False):
            raise ValueError("KeyframeMap.render_colour: the map holds no colour (KeyframeMap(colour=True))")
        return self._render("render_colour", np.uint32, K, width, height, poses, device, params)

    def render_normals(self, K, width, height, poses, device=False, **params):
        """Normals views of a map with normals (dvo_hip_map_render_normals): like render(), but returns (normals, Z): float32 records
        {n.x, n.y, n.z, has} of shape (n, height, width, 4) -- the nearest voxel's normal in the VIEW'S CAMERA coordinates (x right, y
        down, z forward; a surface facing the camera has n.z < 0) and 1, or zeros where nothing was seen or the voxel has no normal --
        and the depth planes, bit for bit render()'s.  The normals are dequantised from 10 bits per component and not renormalised:
        their length is within 2e-3 of 1.  device=True: torch tensors on the GPU."""
        who = "KeyframeMap.render_normals"
        if not getattr(self, "with_normals", False):
            raise ValueError("%s: the map holds no normals (KeyframeMap(normals=True))" % who)
        K, width, height, T = _render_view_args(K, width, height, poses, who)
        rp = render_params_struct(**params)
        n = T.shape[0]
        nrm = _out_array(self.ctx, (n, height, width, 4), np.float32, device)
        if device:
            pad = (width * height + 3) // 4 * 4             # (every view's plane 16-byte aligned)
            Z = _out_array(self.ctx, n * pad, np.float32, True).as_strided((n, height, width), (pad, width, 1))
        else:
            Z = _out_array(self.ctx, (n, height, width), np.float32, False)
        ptrs = [device_pointer_array([_address(a[k]) for k in range(n)]) for a in (nrm, Z)]
        self.ctx.check(self.ctx._lib.dvo_hip_map_render_normals(self.ctx.ptr, self.ptr, n, width, height, K.ctypes.data_as(C.POINTER(C.c_float)),
                                                                T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rp), ptrs[0], ptrs[1],
                                                                1 if device else 0))
        return nrm, Z

    def render_into(self, pyramids, poses, role=None, config=None, flags=0, **params):
        """Views of the map straight into existing pyramids of one camera (dvo_hip_map_render_frames): pyramid i becomes the frame that the
        planes render() gives for its own size and K at poses[i] would make, without the planes leaving the device.  role None: a plain
        update; "current" / "reference" with config: ingest and prepare in one pass.  flags: _lib.INGEST_NO_RAW_COPY."""
        who = "KeyframeMap.render_into"
        n = len(pyramids)
        if n < 1:
            raise ValueError("%s: no pyramids" % who)
        T = _pose_array(poses, n, who, **_VIEW_POSES)
        for p in pyramids:
            if p.ctx is not self.ctx:
                raise ValueError("%s: the pyramids belong to another context than the map" % who)
            if p.camera is not pyramids[0].camera:
                raise ValueError("%s: the pyramids of one call share a camera" % who)
            if getattr(p, "_lens", None) is not None or getattr(p, "_depth_rig", None) is not None or getattr(p, "_depth_filter", None) is not None:
                raise ValueError("%s: a pyramid that carries a lens, a depth rig or a depth filter takes raw sensor planes, not rendered ones" % who)
        if int(flags) & _lib.INGEST_DEFER:
            raise ValueError("%s: a render cannot be deferred" % who)
        rp = render_params_struct(**params)
        r, cfg = _colour_call_args(pyramids, role, config)
        self.ctx.check(self.ctx._lib.dvo_hip_map_render_frames(self.ctx.ptr, self.ptr, n, _handles(pyramids), T.ctypes.data_as(C.POINTER(C.c_double)),
                                                               C.byref(rp), r, cfg, int(flags)))

    def close(self):
        if getattr(self, "ptr", None) and self.ctx.ptr:
            self.ctx._lib.dvo_hip_map_destroy(self.ctx.ptr, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GRAPH_DEFAULTS = dict(max_iterations=50, cg_max_iterations=200, cg_tolerance=1e-8, min_relative_decrease=1e-9,
                      initial_damping_scale=1e-5)   # dvo_hip_graph_params_default


def graph_params_struct(**params):
    """dvo_hip_graph_params from keyword arguments (the rest as dvo_hip_graph_params_default gives them), or ValueError / TypeError:
    nothing reaches the library with a value it would refuse."""
    unknown = set(params) - set(GRAPH_DEFAULTS)
    if unknown:
        raise TypeError("PoseGraph.optimize: unknown parameter(s) %s; known: %s" % (sorted(unknown), sorted(GRAPH_DEFAULTS)))
    p = dict(GRAPH_DEFAULTS, **params)
    for k in ("max_iterations", "cg_max_iterations"):
        if isinstance(p[k], bool) or not isinstance(p[k], (int, np.integer)):
            raise TypeError("PoseGraph.optimize: %s must be an integer" % k)
    if p["max_iterations"] < 0 or not 1 <= p["cg_max_iterations"] <= 100000:
        raise ValueError("PoseGraph.optimize: need max_iterations >= 0 and 1 <= cg_max_iterations <= 100000")
    tol, dec, tau = float(p["cg_tolerance"]), float(p["min_relative_decrease"]), float(p["initial_damping_scale"])
    if not 0.0 < tol < 1.0:
        raise ValueError("PoseGraph.optimize: cg_tolerance must lie in (0, 1)")
    if not 0.0 <= dec < float("inf"):
        raise ValueError("PoseGraph.optimize: min_relative_decrease must be finite and >= 0")
    if not 0.0 < tau < float("inf"):
        raise ValueError("PoseGraph.optimize: initial_damping_scale must be finite and > 0")
    out = _lib.GraphParams()
    out.max_iterations, out.cg_max_iterations = int(p["max_iterations"]), int(p["cg_max_iterations"])
    out.cg_tolerance, out.min_relative_decrease, out.initial_damping_scale = tol, dec, tau
    return out


def _graph_report(rep, recs):
    """a dvo_hip_graph_report and the records of its trials as PoseGraph.optimize returns them"""
    out = {k: getattr(rep, k) for k in ("iterations", "accepted", "cg_iterations", "initial_cost", "final_cost", "final_damping")}
    out["status"] = _lib.GRAPH_STATUS[rep.status]
    out["records"] = [dict(cost_before=r.cost_before, cost_after=r.cost_after, damping=r.damping, cg_iterations=r.cg_iterations,
                           cg_status=_lib.GRAPH_CG_STATUS[r.cg_status], accepted=bool(r.accepted)) for r in recs]
    return out


def _graph_array(a, shape_tail, who, what):
    """a as a contiguous float64 array of shape (k,) + shape_tail with finite entries, or ValueError / TypeError"""
    try:
        a = np.ascontiguousarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("%s: %s must be real numbers" % (who, what))
    if a.ndim != 1 + len(shape_tail) or a.shape[1:] != shape_tail:
        raise ValueError("%s: %s must have shape (k,%s), got %s" % (who, what, " %s" % ", ".join(map(str, shape_tail)) if shape_tail else "", a.shape))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s: %s has a non-finite entry" % (who, what))
    return a


def _graph_indices(a, n, who, what):
    a = np.asarray(a)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise TypeError("%s: %s must be integers" % (who, what))
    if a.ndim != 1:
        raise ValueError("%s: %s must be one-dimensional" % (who, what))
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError("%s: a vertex index in %s is out of range" % (who, what))
    return np.ascontiguousarray(a, dtype=np.int32)


class PoseGraph:
    """The keyframe pose graph, optimised on the device (dvo_hip_graph_*; the reference's g2o graph of VertexSE3 / EdgeSE3 with an
    optional Cauchy kernel under Levenberg-Marquardt, dvo_slam/src/keyframe_graph.cpp:256-285, 840-845).  Poses are 4 x 4, camera ->
    world, as KeyframeMap takes them: poses() after optimize() is what KeyframeMap.move() wants as poses_new.  The information
    matrices (6 x 6, translation rows first) are taken as given, like the reference takes Result.Information.  The result depends on
    the order the edges are given in, and on nothing else: the same call gives the same bits."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self.ptr = C.c_void_p()
        self.n = self.m = 0
        self.delta, self._edges = np.zeros(0), None
        self.ctx.check(self.ctx._lib.dvo_hip_graph_create(self.ctx.ptr, C.byref(self.ptr)))

    def set_vertices(self, poses, fixed=None):
        """n poses [n, 4, 4]; fixed: n booleans, or None.  Drops the edges."""
        who = "PoseGraph.set_vertices"
        T = _graph_array(poses, (4, 4), who, "poses")
        if not 1 <= T.shape[0] <= _lib.GRAPH_MAX_VERTICES:
            raise ValueError("%s: need 1 .. 2^20 vertices" % who)
        f = None
        if fixed is not None:
            f = np.ascontiguousarray(np.asarray(fixed) != 0, dtype=np.uint8)
            if f.shape != (T.shape[0],):
                raise ValueError("%s: fixed must have one entry per vertex" % who)
        self.ctx.check(self.ctx._lib.dvo_hip_graph_set_vertices(self.ctx.ptr, self.ptr, T.shape[0], T.ctypes.data_as(C.POINTER(C.c_double)),
                                                                f.ctypes.data_as(C.POINTER(C.c_uint8)) if f is not None else None))
        self.n, self.m, self.delta, self._edges = T.shape[0], 0, np.zeros(0), None

    def set_poses(self, poses):
        """a new estimate for the same vertices and edges"""
        T = _graph_array(poses, (4, 4), "PoseGraph.set_poses", "poses")
        if self.n < 1 or T.shape[0] != self.n:
            raise ValueError("PoseGraph.set_poses: the graph has %d vertices, got %d poses" % (self.n, T.shape[0]))
        self.ctx.check(self.ctx._lib.dvo_hip_graph_set_poses(self.ctx.ptr, self.ptr, self.n, T.ctypes.data_as(C.POINTER(C.c_double))))

    def set_edges(self, from_, to, measurements, information, delta=None):
        """m edges from_[k] -> to[k] with measurements [m, 4, 4] and information [m, 6, 6]; delta: the Cauchy kernel's width per edge
        (a scalar for all of them; 0 or None = no kernel).  Replaces all earlier edges."""
        who = "PoseGraph.set_edges"
        if self.n < 1:
            raise ValueError("%s: set the vertices first" % who)
        i, j = _graph_indices(from_, self.n, who, "from_"), _graph_indices(to, self.n, who, "to")
        m = i.shape[0]
        if j.shape[0] != m or m > _lib.GRAPH_MAX_EDGES:
            raise ValueError("%s: from_ and to must have the same length, at most 2^22" % who)
        if np.any(i == j):
            raise ValueError("%s: an edge from a vertex to itself" % who)
        Z = _graph_array(measurements, (4, 4), who, "measurements") if m else np.zeros((0, 4, 4))
        W = _graph_array(information, (6, 6), who, "information") if m else np.zeros((0, 6, 6))
        if Z.shape[0] != m or W.shape[0] != m:
            raise ValueError("%s: one measurement and one information matrix per edge" % who)
        if delta is None or np.ndim(delta) == 0:
            delta = np.full(m, 0.0 if delta is None else delta)
        d = _graph_array(delta, (), who, "delta")
        if d.shape[0] != m or np.any(d < 0):
            raise ValueError("%s: one delta >= 0 per edge" % who)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self.ctx.check(self.ctx._lib.dvo_hip_graph_set_edges(self.ctx.ptr, self.ptr, m, i.ctypes.data_as(ip), j.ctypes.data_as(ip), Z.ctypes.data_as(dp),
                                                             W.ctypes.data_as(dp), d.ctypes.data_as(dp)))
        self.m, self.delta = m, d.copy()
        self._edges = (i.copy(), j.copy(), Z.copy(), W.copy())

    def optimize(self, **params):
        """Levenberg-Marquardt to the stop rules.  params: max_iterations, cg_max_iterations, cg_tolerance,
        min_relative_decrease, initial_damping_scale.  Returns a dict: status (a name of _lib.GRAPH_STATUS), iterations, accepted,
        cg_iterations, initial_cost, final_cost, final_damping, and records: one dict per trial (cost_before, cost_after, damping,
        cg_iterations, cg_status, accepted)."""
        prm = graph_params_struct(**params)
        if self.n < 1:
            raise ValueError("PoseGraph.optimize: set the vertices first")
        rep = _lib.GraphReport()
        recs = (_lib.GraphIteration * max(prm.max_iterations, 1))()
        self.ctx.check(self.ctx._lib.dvo_hip_graph_optimize(self.ctx.ptr, self.ptr, C.byref(prm), C.byref(rep), recs, prm.max_iterations))
        return _graph_report(rep, recs[:rep.iterations])

    @staticmethod
    def optimize_batch(graphs, params=None, max_records=None):
        """Many small graphs in ONE launch, one workgroup each (dvo_hip_graph_optimize_batch): every graph of the list is left as its
        own optimize() would have left it, bit for bit.  graphs: PoseGraph objects of one context, each once, each resident-sized (at
        most _lib.GRAPH_RESIDENT_MAX_VERTICES vertices and _lib.GRAPH_RESIDENT_MAX_EDGES edges).  params: a dict of optimize()'s
        parameters for all of them, or a list of one dict per graph; None = the defaults.  max_records: trials recorded per graph
        (None = every trial).  Returns a list of reports shaped like optimize()'s."""
        who = "PoseGraph.optimize_batch"
        graphs = list(graphs)
        if not graphs:
            raise ValueError("%s: no graph" % who)
        for g in graphs:
            if not isinstance(g, PoseGraph):
                raise TypeError("%s: graphs must be PoseGraph objects" % who)
        if len(set(id(g) for g in graphs)) != len(graphs):
            raise ValueError("%s: the same graph twice" % who)
        ctx = graphs[0].ctx
        for g in graphs:
            if g.ctx is not ctx:
                raise ValueError("%s: graphs of more than one context" % who)
            if g.n < 1:
                raise ValueError("%s: set the vertices first" % who)
            if g.n > _lib.GRAPH_RESIDENT_MAX_VERTICES or g.m > _lib.GRAPH_RESIDENT_MAX_EDGES:
                raise ValueError("%s: a graph of %d vertices and %d edges is beyond %d / %d; optimize() takes it" % (
                    who, g.n, g.m, _lib.GRAPH_RESIDENT_MAX_VERTICES, _lib.GRAPH_RESIDENT_MAX_EDGES))
        if params is None or isinstance(params, dict):
            params = [params or {}] * len(graphs)
        else:
            params = list(params)
            if len(params) != len(graphs):
                raise ValueError("%s: %d parameter sets for %d graphs" % (who, len(params), len(graphs)))
            for p in params:
                if not isinstance(p, dict):
                    raise TypeError("%s: params must be a dict or a list of dicts" % who)
        prm = (_lib.GraphParams * len(graphs))(*[graph_params_struct(**p) for p in params])
        if max_records is None:
            max_records = max(p.max_iterations for p in prm)
        if isinstance(max_records, bool) or not isinstance(max_records, (int, np.integer)):
            raise TypeError("%s: max_records must be an integer" % who)
        if max_records < 0:
            raise ValueError("%s: max_records must be >= 0" % who)
        max_records = int(max_records)
        reps = (_lib.GraphReport * len(graphs))()
        recs = (_lib.GraphIteration * max(len(graphs) * max_records, 1))()
        ptrs = (C.c_void_p * len(graphs))(*[g.ptr.value if isinstance(g.ptr, C.c_void_p) else g.ptr for g in graphs])
        ctx.check(ctx._lib.dvo_hip_graph_optimize_batch(ctx.ptr, len(graphs), ptrs, prm, reps, recs, max_records))
        return [_graph_report(rep, recs[k * max_records:k * max_records + min(rep.iterations, max_records)]) for k, rep in enumerate(reps)]

    def poses(self):
        """the current estimate, [n, 4, 4]"""
        if self.n < 1:
            raise ValueError("PoseGraph.poses: set the vertices first")
        T = np.empty((self.n, 4, 4))
        self.ctx.check(self.ctx._lib.dvo_hip_graph_get_poses(self.ctx.ptr, self.ptr, self.n, T.ctypes.data_as(C.POINTER(C.c_double))))
        return T

    def edge_stats(self):
        """(chi2 [m], weight [m]) at the current estimate: e^T Omega e and the kernel's weight, 1 where an edge has no kernel"""
        chi2, w = np.empty(self.m), np.empty(self.m)
        dp = C.POINTER(C.c_double)
        self.ctx.check(self.ctx._lib.dvo_hip_graph_edge_stats(self.ctx.ptr, self.ptr, self.m, chi2.ctypes.data_as(dp), w.ctypes.data_as(dp)))
        return chi2, w

    def linearise(self):
        """One stage, results to the host (dvo_hip_graph_linearise, a test hook): dict of error [m, 6], chi2 [m], weight [m], blocks
        [m, 3, 6, 6] (w Ji^T W Ji, w Ji^T W Jj, w Jj^T W Jj), gradient [m, 2, 6] and cost at the current estimate."""
        m, dp = self.m, C.POINTER(C.c_double)
        e, s, w, B, g, c = np.zeros((m, 6)), np.zeros(m), np.zeros(m), np.zeros((m, 3, 6, 6)), np.zeros((m, 2, 6)), C.c_double(0)
        self.ctx.check(self.ctx._lib.dvo_hip_graph_linearise(self.ctx.ptr, self.ptr, e.ctypes.data_as(dp), s.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                                             B.ctypes.data_as(dp), g.ctypes.data_as(dp), C.byref(c)))
        return dict(error=e, chi2=s, weight=w, blocks=B, gradient=g, cost=c.value)

    def multiply(self, damping, p):
        """One stage (dvo_hip_graph_multiply, a test hook): linearise, gather, factorise, then y = (H + damping I) p over the free vertices
        for p [n, 6].  dict of y [n, 6], pty, diagonal [n, 6, 6], rhs [n, 6], inverse [n, 6, 6]."""
        n, dp = self.n, C.POINTER(C.c_double)
        p = _graph_array(p, (6,), "PoseGraph.multiply", "p")
        if n < 1 or p.shape[0] != n or not 0.0 <= float(damping) < float("inf"):
            raise ValueError("PoseGraph.multiply: need one p per vertex and a finite damping >= 0")
        y, D, b, Mi, pty = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros((n, 6, 6)), C.c_double(0)
        self.ctx.check(self.ctx._lib.dvo_hip_graph_multiply(self.ctx.ptr, self.ptr, float(damping), p.ctypes.data_as(dp), y.ctypes.data_as(dp), C.byref(pty),
                                                            D.ctypes.data_as(dp), b.ctypes.data_as(dp), Mi.ctypes.data_as(dp)))
        return dict(y=y, pty=pty.value, diagonal=D, rhs=b, inverse=Mi)

    def remove_outliers(self, weight_threshold, n_max=-1):
        """The reference's removeOutlierConstraints (dvo_slam/src/keyframe_graph.cpp:643-674): among the edges that carry a kernel, those
        whose weight is below the threshold leave the graph, lowest first, at most n_max of them (-1: all).  Returns their indices."""
        if isinstance(n_max, bool) or not isinstance(n_max, (int, np.integer)):
            raise TypeError("PoseGraph.remove_outliers: n_max must be an integer")
        threshold = float(weight_threshold)
        if threshold != threshold:
            raise ValueError("PoseGraph.remove_outliers: the threshold is NaN")
        gone = select_outliers(self.edge_stats()[1], self.delta, threshold, int(n_max))
        if len(gone):
            keep = np.setdiff1d(np.arange(self.m), gone)
            i, j, Z, W = self._edges
            self.set_edges(i[keep], j[keep], Z[keep], W[keep], self.delta[keep])
        return gone

    def close(self):
        if getattr(self, "ptr", None) and self.ctx.ptr:
            self.ctx._lib.dvo_hip_graph_destroy(self.ctx.ptr, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def select_outliers(weights, delta, threshold, n_max=-1):
    """the edges remove_outliers takes: a kernel (delta > 0) and a weight below the threshold, lowest weight first (ties: lowest index),
    at most n_max (-1: all)"""
    weights, delta = np.asarray(weights, dtype=np.float64), np.asarray(delta, dtype=np.float64)
    candidates = np.nonzero((delta > 0) & (weights < threshold))[0]
    order = candidates[np.argsort(weights[candidates], kind="stable")]
    return order if n_max < 0 else order[:n_max]


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


def set_depth_filter_batch(pyramids, **params):
    """RgbdImagePyramid.set_depth_filter for n pyramids of one context in one call (they then carry equal filters, as one ingest call wants)."""
    filt = depth_filter_struct(**params)
    if len(pyramids) < 1:
        raise ValueError("set_depth_filter_batch: no pyramids")
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_set_depth_filter(ctx.ptr, len(pyramids), _handles(pyramids), C.byref(filt)))
    kept = {name: getattr(filt, name) for name in _DEPTH_FILTER_DEFAULTS}
    for p in pyramids:
        p._depth_filter = dict(kept)                         # (kept for a frame that is built again with more levels)


def clear_depth_filter_batch(pyramids):
    if len(pyramids) < 1:
        raise ValueError("clear_depth_filter_batch: no pyramids")
    ctx = pyramids[0].ctx
    ctx.check(ctx._lib.dvo_hip_frames_clear_depth_filter(ctx.ptr, len(pyramids), _handles(pyramids)))
    for p in pyramids:
        p._depth_filter = None


def set_level_selection(pyramid, level, accepted):
    """Explicit selection of one level (dvo_hip_frame_set_level_selection): `accepted`, a (height, width) array of that level, is the
    exact accepted set (non-zero = selected) until the pyramid's pixels change or another selection is requested; None drops it."""
    pyramid.build(level + 1)
    if accepted is None:
        pyramid.ctx.check(pyramid.ctx._lib.dvo_hip_frame_set_level_selection(pyramid.ctx.ptr, pyramid.ptr, level, None))
        return
    img = pyramid.level(level)
    a = np.ascontiguousarray(accepted, dtype=np.uint8)
    if a.shape != (img.height, img.width):
        raise ValueError("set_level_selection: accepted is (%d, %d)" % (img.height, img.width))
    pyramid.ctx.check(pyramid.ctx._lib.dvo_hip_frame_set_level_selection(pyramid.ctx.ptr, pyramid.ptr, level,
                                                                         a.ctypes.data_as(C.POINTER(C.c_uint8))))


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


def update_raw_host_batch(pyramids, grey_host, depth_host, depth_scale=1.0 / 5000.0, role=None, config=None):
    """Re-ingest raw planes from HOST arrays (uint8 / uint16, C-contiguous) into n existing pyramids: asynchronous DMA on the
    context's upload stream, then the batched build (dvo_hip_frames_update_raw).  The arrays must stay unchanged until
    upload_wait() or until a match on these pyramids has returned."""
    n = len(pyramids)
    ctx = pyramids[0].ctx
    vp = C.c_void_p
    fr = _handles(pyramids)
    if isinstance(grey_host, C.Array):          # addresses prepared once by the caller (device_pointer_array of host addresses)
        g, z = grey_host, depth_host
    else:
        for a, b in zip(grey_host, depth_host):
            assert a.dtype == np.uint8 and b.dtype == np.uint16 and a.flags.c_contiguous and b.flags.c_contiguous
        g = (vp * n)(*[vp(a.ctypes.data) for a in grey_host])
        z = (vp * n)(*[vp(a.ctypes.data) for a in depth_host])
    if role is None:
        ctx.check(ctx._lib.dvo_hip_frames_update_raw(ctx.ptr, n, fr, g, z, depth_scale))
    else:
        ccfg = config if isinstance(config, _lib.Config) else config.to_c()
        ctx.check(ctx._lib.dvo_hip_frames_update_raw_as(ctx.ptr, n, fr, g, z, depth_scale, _ROLES[role], C.byref(ccfg)))


def _colour_call_args(pyramids, role, config):
    if role is None:
        return -1, None
    if role not in _ROLES:
        raise ValueError("role must be 'current', 'reference' or None, not %r" % (role,))
    if config is None:
        raise ValueError("a role needs a config")
    return _ROLES[role], C.byref(config if isinstance(config, _lib.Config) else config.to_c())


def _depth_format(name):
    if not isinstance(name, str) or name not in _lib.DEPTH_FORMATS:
        raise ValueError("depth_format must be one of %s, not %r" % (sorted(_lib.DEPTH_FORMATS), name))
    return _lib.DEPTH_FORMATS[name]


def _mixed_pixel_format(name, width, height):
    """the image formats that come with a float depth plane: the colour formats, the raw sensor formats and "grey8" ([h, w, 1] uint8)"""
    if isinstance(name, str) and name in _lib.SENSOR_PIXEL_FORMATS:
        return _sensor_format(name, width, height)
    if not isinstance(name, str) or name not in _lib.MIXED_PIXEL_FORMATS:
        raise ValueError("pixel_format must be one of %s, not %r" % (sorted(_lib.MIXED_PIXEL_FORMATS) + sorted(_lib.SENSOR_PIXEL_FORMATS), name))
    return _lib.MIXED_PIXEL_FORMATS[name], _lib.MIXED_PIXEL_CHANNELS[name]


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


def update_f32_device_batch(pyramids, intensity_ptrs, depth_ptrs, intensity_pitch=0, depth_pitch=0, depth_scale=1.0, role=None, config=None,
                            flags=0):
    """Re-ingest float32 planes (device pointers: intensity 0..255, depth in metres * depth_scale with NaN = hole; one row pitch in bytes
    per kind for all, 0 = tight) into n existing pyramids of one camera (dvo_hip_frames_update_f32_device_as_ex).  role None: a plain
    update; "current" / "reference" with config: ingest and prepare in one pass.  flags: _lib.INGEST_DEFER | _lib.INGEST_NO_RAW_COPY."""
    pyr0 = pyramids[0]
    ipitch = _f32_pitch(intensity_pitch, pyr0.camera.width, "intensity")
    zpitch = _f32_pitch(depth_pitch, pyr0.camera.width, "depth")
    if len(intensity_ptrs) != len(pyramids) or len(depth_ptrs) != len(pyramids):
        raise ValueError("one intensity and one depth plane per pyramid")
    r, cfg = _colour_call_args(pyramids, role, config)
    n = len(pyramids)
    ctx = pyr0.ctx
    fr, i, z = _handles(pyramids), _pointer_array(intensity_ptrs), _pointer_array(depth_ptrs)
    ctx.check(ctx._lib.dvo_hip_frames_update_f32_device_as_ex(ctx.ptr, n, fr, i, ipitch, z, zpitch, depth_scale, r, cfg, int(flags)))


def update_f32_host_batch(pyramids, intensity_host, depth_host, depth_scale=1.0, role=None, config=None, flags=0):
    """Re-ingest float32 planes from HOST arrays ([h, w] float32 views with contiguous pixels; the row stride of each kind, the same for
    the whole batch, is taken from the views) into n existing pyramids: DMA on the context's upload stream, then the batched build
    (dvo_hip_frames_update_f32_as_ex).  The arrays must stay unchanged until upload_wait() or a match on these pyramids has returned.
    flags: _lib.INGEST_NO_RAW_COPY (a host ingest cannot be deferred)."""
    cam = pyramids[0].camera
    if len(intensity_host) != len(pyramids) or len(depth_host) != len(pyramids):
        raise ValueError("one intensity and one depth plane per pyramid")
    if int(flags) & _lib.INGEST_DEFER:
        raise ValueError("INGEST_DEFER takes device planes")
    ints = [_f32_plane(a, cam.height, cam.width, "intensity") for a in intensity_host]
    deps = [_f32_plane(b, cam.height, cam.width, "depth") for b in depth_host]
    ipitch, zpitch = _one_pitch(ints, "intensity"), _one_pitch(deps, "depth")
    r, cfg = _colour_call_args(pyramids, role, config)
    n = len(pyramids)
    ctx = pyramids[0].ctx
    vp = C.c_void_p
    i = (vp * n)(*[vp(a.ctypes.data) for a in ints])
    z = (vp * n)(*[vp(b.ctypes.data) for b in deps])
    ctx.check(ctx._lib.dvo_hip_frames_update_f32_as_ex(ctx.ptr, n, _handles(pyramids), i, ipitch, z, zpitch, depth_scale, r, cfg, int(flags)))


def update_colour_device_batch(pyramids, colour_dev_ptrs, depth_dev_ptrs, pixel_format="bgr8", pitch=0, depth_scale=1.0 / 5000.0, role=None,
                               config=None, flags=0, depth_format="u16", depth_pitch=0):
    """Re-ingest 8-bit colour planes (device pointers, one format and row pitch in bytes for all, 0 = tight) + u16 depth planes into n
    existing pyramids of one camera (dvo_hip_frames_update_colour_device_as_ex).  role None: a plain update; "current" / "reference"
    with config: ingest and prepare in one pass.  flags: _lib.INGEST_DEFER | _lib.INGEST_NO_RAW_COPY.
    depth_format "f32": the depth planes are float32 metres with NaN = hole and a row pitch of their own (depth_pitch, bytes, 0 = tight;
    dvo_hip_frames_update_colour_f32depth_device_as_ex); pixel_format may then also be "grey8".  Mind depth_scale: 1.0 for metres."""
    zf = _depth_format(depth_format) == _lib.DEPTH_F32
    pyr0 = pyramids[0]
    fmt, ch = (_mixed_pixel_format if zf else _pixel_format)(pixel_format, pyr0.camera.width, pyr0.camera.height)
    pitch = _pitch(pitch, pyr0.camera.width, ch)
    if zf:
        depth_pitch = _f32_pitch(depth_pitch, pyr0.camera.width, "depth")
    elif int(depth_pitch) != 0:
        raise ValueError("a u16 depth plane is tight: depth_pitch goes with depth_format 'f32'")
    if len(colour_dev_ptrs) != len(pyramids) or len(depth_dev_ptrs) != len(pyramids):
        raise ValueError("one colour and one depth plane per pyramid")
    r, cfg = _colour_call_args(pyramids, role, config)
    n = len(pyramids)
    ctx = pyr0.ctx
    fr, c, z = _handles(pyramids), _pointer_array(colour_dev_ptrs), _pointer_array(depth_dev_ptrs)
    if zf:
        ctx.check(ctx._lib.dvo_hip_frames_update_colour_f32depth_device_as_ex(ctx.ptr, n, fr, c, fmt, pitch, z, depth_pitch, depth_scale, r, cfg,
                                                                              int(flags)))
    else:
        ctx.check(ctx._lib.dvo_hip_frames_update_colour_device_as_ex(ctx.ptr, n, fr, c, fmt, pitch, z, depth_scale, r, cfg, int(flags)))


def update_colour_host_batch(pyramids, colour_host, depth_host, pixel_format="bgr8", depth_scale=1.0 / 5000.0, role=None, config=None, flags=0,
                             depth_format="u16"):
    """Re-ingest 8-bit colour planes from HOST arrays ([h, w, 3 | 4] uint8, one format; rows may be padded by the same stride) + u16 depth
    planes (C-contiguous) into n existing pyramids: DMA on the context's upload stream, then the batched build
    (dvo_hip_frames_update_colour_as_ex).  The arrays must stay unchanged until upload_wait() or a match on these pyramids has returned.
    depth_format "f32": the depth planes are [h, w] float32 views (metres, NaN = hole; rows may be padded by the same stride;
    dvo_hip_frames_update_colour_f32depth_as_ex); pixel_format may then also be "grey8" ([h, w, 1] uint8).  Mind depth_scale: 1.0 for metres."""
    zf = _depth_format(depth_format) == _lib.DEPTH_F32
    cam = pyramids[0].camera
    fmt, ch = (_mixed_pixel_format if zf else _pixel_format)(pixel_format, cam.width, cam.height)
    if len(colour_host) != len(pyramids) or len(depth_host) != len(pyramids):
        raise ValueError("one colour and one depth plane per pyramid")
    if zf and int(flags) & _lib.INGEST_DEFER:
        raise ValueError("INGEST_DEFER takes device planes")
    cols = [_colour_plane(a, cam.height, cam.width, ch, pixel_format in _lib.SENSOR_PIXEL_FORMATS) for a in colour_host]
    deps = [_f32_plane(b, cam.height, cam.width, "depth") if zf else _depth_plane(b, cam.height, cam.width) for b in depth_host]
    if any(a is not b for a, b in zip(cols, colour_host)) or any(a is not b for a, b in zip(deps, depth_host)):
        raise ValueError("host planes must be usable in place (pixels contiguous, depth C-contiguous): the transfer is asynchronous")
    pitch = cols[0].strides[0]
    if any(a.strides[0] != pitch for a in cols):
        raise ValueError("every colour plane of a batch must have the same row stride")
    r, cfg = _colour_call_args(pyramids, role, config)
    n = len(pyramids)
    ctx = pyramids[0].ctx
    vp = C.c_void_p
    c = (vp * n)(*[vp(a.ctypes.data) for a in cols])
    z = (vp * n)(*[vp(b.ctypes.data) for b in deps])
    if zf:
        ctx.check(ctx._lib.dvo_hip_frames_update_colour_f32depth_as_ex(ctx.ptr, n, _handles(pyramids), c, fmt, pitch, z, _one_pitch(deps, "depth"),
                                                                       depth_scale, r, cfg, int(flags)))
    else:
        ctx.check(ctx._lib.dvo_hip_frames_update_colour_as_ex(ctx.ptr, n, _handles(pyramids), c, fmt, pitch, z, depth_scale, r, cfg, int(flags)))


def upload_wait(ctx):
    ctx.check(ctx._lib.dvo_hip_upload_wait(ctx.ptr))


def prepare_roles_batch(pyramids, role, config):
    """Build the role planes of n pyramids ahead of time and asynchronously (dvo_hip_frames_prepare): role "current" = sampling
    planes, "reference" = point selection for config's thresholds.  Together with update_raw_device_batch this runs on the
    context's build stream, concurrently with a match started afterwards on other frames."""
    n = len(pyramids)
    ctx = pyramids[0].ctx
    fr = _handles(pyramids)
    ccfg = config.to_c()
    ctx.check(ctx._lib.dvo_hip_frames_prepare(ctx.ptr, n, fr, _ROLES[role], C.byref(ccfg)))


class PointSelection:
    """Reference-side selection cache (point_selection.h:69-99).  The selected list itself never leaves the GPU."""

    def __init__(self, pyramid=None, intensity_threshold=0.0, depth_threshold=0.0):
        self.pyramid = pyramid
        self.intensity_threshold, self.depth_threshold = intensity_threshold, depth_threshold

    def setRgbdImagePyramid(self, pyramid):
        self.pyramid = pyramid

    recycle = setRgbdImagePyramid

    def getRgbdImagePyramid(self):
        assert self.pyramid is not None
        return self.pyramid

    def getMaximumNumberOfPoints(self, level):     # point_selection.cpp:68-71
        c = self.pyramid.camera
        return int(c.width * c.height * 0.25 ** level)

    def select(self, level, want_mask=False):
        """Returns the number of selected points (and the uint8 mask if asked): the thresholds' selection combined with the
        pyramid's caller selection (RgbdImagePyramid.set_selection)."""
        p = self.pyramid
        p.build(level + 1)
        n = C.c_int()
        mask = None
        mp = None
        if want_mask:
            img = p.level(level)
            mask = np.zeros((img.height, img.width), np.uint8)
            mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        p.ctx.check(p.ctx._lib.dvo_hip_frame_select(p.ctx.ptr, p.ptr, level, self.intensity_threshold, self.depth_threshold,
                                                   C.byref(n), mp))
        return (n.value, mask) if want_mask else n.value


_RESULT_DTYPE = np.dtype([("transformation", np.float64, (16,)), ("information", np.float64, (36,)), ("loglik", np.float64),
                          ("n_levels", np.int32), ("n_iterations_total", np.int32),
                          ("entropy", np.float64), ("condition_number", np.float64), ("constraint_ratio", np.float64),
                          ("constraint_ratio_accepted", np.float64)])
assert _RESULT_DTYPE.itemsize == C.sizeof(_lib.Result)


def _unpack_stats(res, levels, iters):
    out = []
    for li in range(res.n_levels):
        L = levels[li]
        ls = LevelStats(L.id, L.max_valid_pixels, L.valid_pixels, L.termination)
        for k in range(L.n_iterations):
            s = iters[L.first_iteration_index + k]
            ls.Iterations.append(IterationStats(
                s.id, s.valid_constraints, s.tdist_loglik, np.array(s.tdist_mean), np.array(s.tdist_precision).reshape(2, 2),
                s.prior_loglik, np.array(s.increment), np.array(s.information).reshape(6, 6)))
        out.append(ls)
    return out


class DenseTracker:
    """dvo::DenseTracker (dense_tracking.h:142-162).  Not re-entrant, like the reference: one per thread."""
    _default_config = Config()

    @staticmethod
    def getDefaultConfig():
        return DenseTracker._default_config

    def __init__(self, config=None, ctx=None):
        self.ctx = ctx or default_context()
        self.reference_selection_ = PointSelection()
        self.configure(config or DenseTracker.getDefaultConfig())

    def configure(self, config):
        assert config.IsSane()                                   # dense_tracking.cpp:74
        self.cfg = Config(**config.__dict__)
        self.reference_selection_.intensity_threshold = config.IntensityDerivativeThreshold
        self.reference_selection_.depth_threshold = config.DepthDerivativeThreshold

    def configuration(self):
        return self.cfg

    def match(self, reference, current, result_or_transformation, with_stats=True):
        """match(RgbdImagePyramid|PointSelection reference, RgbdImagePyramid current, Result& | 4x4 ndarray (in/out)).
        Always returns True; failure shows as Result.isNaN() / termination criteria."""
        ref_pyr = reference.getRgbdImagePyramid() if isinstance(reference, PointSelection) else reference
        if isinstance(result_or_transformation, Result):
            self.match_batch([ref_pyr], [current], [result_or_transformation], with_stats=with_stats)
            return True
        T = result_or_transformation
        r = Result()
        r.Transformation = np.array(T, dtype=np.float64)
        self.match_batch([ref_pyr], [current], [r], with_stats=False)
        T[...] = r.Transformation
        return True

    def match_batch(self, references, currents, results, with_stats=False):
        """n independent alignments in one batched launch sequence (keyframe_graph.cpp:576-593 shape)."""
        n = len(references)
        assert len(currents) == n and len(results) == n
        cfg = self.cfg
        for r, c in zip(references, currents):
            r.build(cfg.getNumLevels())                           # dense_tracking.cpp:125, 133
            c.build(cfg.getNumLevels())
        cres = (_lib.Result * n)()
        for i, r in enumerate(results):
            if cfg.UseInitialEstimate:
                assert not r.isNaN(), "Provided initialization is NaN!"   # dense_tracking.cpp:139
            else:
                r.setIdentity()
            for k, v in enumerate(np.asarray(r.Transformation, dtype=np.float64).reshape(-1)):
                cres[i].transformation[k] = v
        vp = C.c_void_p
        refs = (vp * n)(*[p.ptr for p in references])
        curs = (vp * n)(*[p.ptr for p in currents])
        ccfg = cfg.to_c()
        nl = cfg.FirstLevel - cfg.LastLevel + 1
        cap_it = nl * cfg.MaxIterationsPerLevel
        if with_stats:
            levels = (_lib.LevelStats * (n * nl))()
            iters = (_lib.IterationStats * (n * cap_it))()
            rc = self.ctx._lib.dvo_hip_match_batch(self.ctx.ptr, n, refs, curs, C.byref(ccfg), cres, levels, nl, iters, cap_it)
        else:
            rc = self.ctx._lib.dvo_hip_match_batch(self.ctx.ptr, n, refs, curs, C.byref(ccfg), cres, None, 0, None, 0)
        self.ctx.check(rc)
        for i, r in enumerate(results):
            r.Transformation = np.array(cres[i].transformation).reshape(4, 4)
            r.Information = np.array(cres[i].information).reshape(6, 6)
            r.LogLikelihood = cres[i].loglik
            # keyframe-selection statistics computed on the device (extension over the reference's Result)
            r.Entropy, r.ConditionNumber = cres[i].entropy, cres[i].condition_number
            r.ConstraintRatio, r.ConstraintRatioAccepted = cres[i].constraint_ratio, cres[i].constraint_ratio_accepted
            if with_stats:   # appended, not cleared
                r.Statistics.Levels.extend(_unpack_stats(cres[i], levels[i * nl:(i + 1) * nl], iters[i * cap_it:(i + 1) * cap_it]))
        return True

    def match_batch_arrays(self, references, currents, T_init=None):
        """match_batch without per-pair Python objects: returns dict(T [n,4,4], information [n,6,6], loglik [n],
        n_iterations [n]).  T_init: optional [n,4,4] initial guesses (used when UseInitialEstimate)."""
        n = len(references)
        cfg = self.cfg
        if not (isinstance(references, FrameSet) and isinstance(currents, FrameSet)):   # a FrameSet's pyramids are final
            for r, c in zip(references, currents):
                r.build(cfg.getNumLevels())
                c.build(cfg.getNumLevels())
        cres = (_lib.Result * n)()
        view = np.frombuffer(cres, dtype=_RESULT_DTYPE)
        if cfg.UseInitialEstimate:
            assert T_init is not None and np.isfinite(T_init).all(), "Provided initialization is NaN!"
            view["transformation"][:] = np.asarray(T_init, dtype=np.float64).reshape(n, 16)
        else:
            view["transformation"][:] = np.eye(4).reshape(16)
        refs, curs = _handles(references), _handles(currents)
        ccfg = cfg.to_c()
        self.ctx.check(self.ctx._lib.dvo_hip_match_batch(self.ctx.ptr, n, refs, curs, C.byref(ccfg), cres, None, 0, None, 0))
        return dict(T=view["transformation"].reshape(n, 4, 4).copy(), information=view["information"].reshape(n, 6, 6).copy(),
                    loglik=view["loglik"].copy(), n_iterations=view["n_iterations_total"].copy(), entropy=view["entropy"].copy(),
                    condition_number=view["condition_number"].copy(), constraint_ratio=view["constraint_ratio"].copy(),
                    constraint_ratio_accepted=view["constraint_ratio_accepted"].copy())

    def level_iteration(self, reference, current, level, T34, P_prev=None, first=True, want_residuals=False):
        """One Gauss-Newton linearisation at a fixed estimate (parity entry point, dvo_hip_level_iteration)."""
        T34 = np.ascontiguousarray(np.asarray(T34, dtype=np.float32).reshape(-1)[:12])
        Pp = np.zeros(4, np.float32) if P_prev is None else np.ascontiguousarray(np.asarray(P_prev, np.float32).reshape(-1))
        out = _lib.IterationOut()
        img = current.level(level)
        res = np.empty((img.height, img.width, 2), np.float32) if want_residuals else None
        self.ctx.check(self.ctx._lib.dvo_hip_level_iteration(
            self.ctx.ptr, reference.ptr, current.ptr, level, self.cfg.IntensityDerivativeThreshold, self.cfg.DepthDerivativeThreshold,
            _fp(T34), _fp(Pp), int(first), C.byref(out), _fp(res) if want_residuals else None))
        d = dict(n=out.n, n_selected=out.n_selected, cov=np.array(out.scale_cov), P=np.array(out.precision).reshape(2, 2),
                 neg_ll=out.neg_loglik, A=np.array(out.A).reshape(6, 6), b=np.array(out.b))
        if want_residuals:
            d["residuals"] = res
        return d

    def time_residual_kernel(self, references, currents, level, reps=20, warm_iterations=3):
        """Average duration (ms) of one launch of the fused residual/Jacobian/reduce/log-likelihood kernel (HIP events), after
        `warm_iterations` Gauss-Newton steps on that level (converged transform, t-distribution weights on; 0 = identity)."""
        n = len(references)
        vp = C.c_void_p
        refs = (vp * n)(*[p.ptr for p in references])
        curs = (vp * n)(*[p.ptr for p in currents])
        ms = C.c_float()
        self.ctx.check(self.ctx._lib.dvo_hip_time_residual_kernel(self.ctx.ptr, n, refs, curs, level, warm_iterations, reps, C.byref(ms)))
        return ms.value

    def time_stream_mix(self, references, currents, level, reps=20, with_write=False):
        """Average duration (ms) of a kernel that only streams the planes the level's sweep reads (window sweep: 16 B per pixel, gathering
        sweep: 32 B; with_write: + 8 B written)."""
        n = len(references)
        vp = C.c_void_p
        refs = (vp * n)(*[p.ptr for p in references])
        curs = (vp * n)(*[p.ptr for p in currents])
        ms = C.c_float()
        self.ctx.check(self.ctx._lib.dvo_hip_time_stream_mix(self.ctx.ptr, n, refs, curs, level, int(with_write), reps, C.byref(ms)))
        return ms.value
