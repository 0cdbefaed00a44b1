"""The keyframe pose graph, optimised on the device (capi_graph.inc): parameters, reports, the graph and its outlier rule."""
import ctypes as C

import numpy as np

from . import _lib
from .context import default_context


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
