"""The voxel-grid map of keyframes on the device (capi_map.inc, cloud_map.h): insert, remove, move, merge, export and render."""
import ctypes as C

import numpy as np

from . import _lib
from .context import default_context
from .planes import _handles, device_pointer_array
from .ingest import _role_args
from .frame_calls import _MERGE_POSES, _VIEW_POSES, _address, _map_frames_args, _out_array, _pose_array

_MAP_RECORD, _MAP_COLOUR_RECORD, _MAP_NORMAL_RECORD = np.dtype(_lib.MAP_RECORD), np.dtype(_lib.MAP_COLOUR_RECORD), np.dtype(_lib.MAP_NORMAL_RECORD)


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
        nrm = _out_array(self.ctx, (m, 4), np.float32, device) if normals else None
        # (the three entries differ in the arrays they take between xyzi and counts)
        ca = [_address(rgba)] if colour else []
        entry, between = ("_normals", [_address(nrm)] + (ca or [None])) if normals else ("_colour", ca) if colour else ("", ca)
        self.ctx.check(getattr(self.ctx._lib, "dvo_hip_map_extract" + entry)(self.ctx.ptr, self.ptr, cap, _address(xyzi), *between, _address(counts),
                                                                             _address(keys), 1 if device else 0, C.byref(got)))
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
        normals = _out_array(self.ctx, max(n, 1), _MAP_NORMAL_RECORD, device) if with_normals else None
        if n > 0:                                            # (dvo_hip_map_export_ex: dvo_hip_map_export with the normal records behind the colour records)
            entry, ex = (self.ctx._lib.dvo_hip_map_export_ex, [_address(normals)]) if with_normals else (self.ctx._lib.dvo_hip_map_export, [])
            self.ctx.check(entry(self.ctx.ptr, self.ptr, n, _address(records), _address(colour) if coloured else None, *ex, 1 if device else 0, C.byref(got)))
        out = records[:got.value], (colour[:got.value] if coloured else None)
        return out + (normals[:got.value],) if with_normals else out

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

    def _render(self, name, first, K, width, height, poses, device, params, trailing=()):
        """render(), render_colour() and render_normals(): dvo_hip_map_<name> into planes of dtype `first` -- trailing: with that many
        values per pixel -- and float32 depth planes"""
        K, width, height, T = _render_view_args(K, width, height, poses, "KeyframeMap." + name)
        rp = render_params_struct(**params)
        n = T.shape[0]
        planes = []
        for dt, tail in ((first, trailing), (np.float32, ())):
            if device and not tail:
                pad = (width * height + 3) // 4 * 4         # (every view's plane 16-byte aligned: views apart by a multiple of 4 words)
                planes.append(_out_array(self.ctx, n * pad, dt, True).as_strided((n, height, width), (pad, width, 1)))
            else:
                planes.append(_out_array(self.ctx, (n, height, width) + tail, dt, device))
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
        if not getattr(self, "with_normals", False):
            raise ValueError("KeyframeMap.render_normals: the map holds no normals (KeyframeMap(normals=True))")
        return self._render("render_normals", np.float32, K, width, height, poses, device, params, trailing=(4,))

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
        r, cfg = _role_args(role, config)
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
