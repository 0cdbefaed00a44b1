"""Keyframes retrieved by appearance (capi_codes.inc, keyframe_codes.h): the fern code book and the candidates it proposes."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DvoHipError
from .context import default_context
from .planes import _handles
from .frame_calls import _address, _out_array, _pyramids_at_level


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
