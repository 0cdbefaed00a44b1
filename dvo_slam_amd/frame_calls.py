"""Calls that read frames at one level under poses: world points, normals, warps, covisibility, and the checks the map and the code book share."""
import ctypes as C

import numpy as np

from . import _lib
from .planes import _handles, device_pointer_array


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
    out, ptrs = _level_outputs(raster_pyramids, level, 3 if difference else 2, (), device)
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
    out, ptrs = _level_outputs(pyramids, level, 2, (), device)
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
