"""CPU tier: the pose-graph optimiser's arithmetic (dvo_slam_amd/csrc/pose_graph.h) without a GPU.
  * the host yardstick: the header compiled with g++ -Wall -Werror -ffp-contract=off plus the sequential Levenberg-Marquardt + PCG
    driver in HOST_SOURCE below, which walks the same incidence lists and the same adjacent-pair trees as the kernels
    (tests/test_gpu_pose_graph.py holds the device to it bit for bit);
  * independent of the header, in numpy: error, chi2, weight and rho against a restatement of g2o's definition (quaternion by the
    eigenvector method), the analytic Jacobians against central differences of that restatement, the gathered blocks against a dense
    H and b, the CG's step against its own stopping measure, the update's rigidity over 1000 steps;
  * convergence on a noise-free helix, a noisy one and one with planted false edges; the edge cases; the Python wrappers; the facade."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_slam_amd as d
from dvo_slam_amd import tracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dvo_slam_amd", "csrc")
EPS = np.finfo(np.float64).eps

HOST_SOURCE = r"""
#include <cstring>
#include <vector>
#include "pose_graph.h"
using namespace dvo_hip;
namespace {
struct Host {
  int n = 0, m = 0, cur = 0;
  bool any_free = false;
  std::vector<unsigned char> fixed;
  std::vector<int> from, to, start, inc;
  std::vector<double> Z, om, delta, E, V, poses[2], t;
  PgGraph view() {
    PgGraph g;
    g.n = n; g.m = m; g.fixed = fixed.data(); g.from = from.data(); g.to = to.data(); g.Z = Z.data(); g.omega = om.data();
    g.delta = delta.data(); g.inc_start = start.data(); g.inc = inc.data(); g.E = E.data(); g.V = V.data();
    return g;
  }
  void incidence() {
    start.assign(size_t(n) + 1, 0);
    inc.assign(size_t(m) * 2 + 1, 0);
    for (int k = 0; k < m; ++k) { start[size_t(from[k]) + 1] += 1; start[size_t(to[k]) + 1] += 1; }
    for (int v = 0; v < n; ++v) start[size_t(v) + 1] += start[size_t(v)];
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int k = 0; k < m; ++k) { inc[size_t(at[size_t(from[k])]++)] = k * 2; inc[size_t(at[size_t(to[k])]++)] = k * 2 + 1; }
    any_free = false;
    for (int v = 0; v < n; ++v) any_free = any_free || (!fixed[size_t(v)] && start[size_t(v) + 1] > start[size_t(v)]);
  }
  double linearise(int which, bool blocks) {
    std::vector<double> rho(size_t(m) + 1);
    const PgGraph g = view();
    for (int k = 0; k < m; ++k) rho[size_t(k)] = pg_linearise_edge(g, poses[which].data(), k, blocks);
    return pg_tree_sum(rho.data(), size_t(m));
  }
  double gather() {
    double top = 0.0;
    const PgGraph g = view();
    for (int v = 0; v < n; ++v) { const double x = pg_gather_vertex(g, v); top = x > top ? x : top; }
    return top;
  }
  // the solve as the launches of pose_graph.hip run it
  int solve(double lambda, double tolerance, int max_iterations, int* iterations) {
    const PgGraph g = view();
    PgCgState s;
    std::memset(&s, 0, sizeof s);
    t.assign(size_t(n), 0.0);
    for (int v = 0; v < n; ++v) { bool ok; t[size_t(v)] = pg_cg_init_vertex(g, v, lambda, &ok); if (!ok) s.cholesky_failed = 1; }
    double rz = pg_tree_sum(t.data(), size_t(n));
    int status = kPgCgRunning;
    for (int it = 0; it < max_iterations; ++it) {
      double beta, alpha;
      if (it == 0) s.rz0 = rz;
      status = pg_cg_before_multiply(s, it, rz, tolerance, &beta);
      if (status != kPgCgRunning) break;
      s.rz[it & 1] = rz;
      s.iterations = it + 1;
      const int p_new = (it & 1) == 0 ? kPgP0 : kPgP1, p_old = p_new == kPgP0 ? kPgP1 : kPgP0;
      for (int v = 0; v < n; ++v) t[size_t(v)] = pg_multiply_vertex(g, v, lambda, it == 0 ? kPgDirFirst : kPgDirNext, beta, p_old, p_new);
      const double pAp = pg_tree_sum(t.data(), size_t(n));
      status = pg_cg_step_length(s.rz[it & 1], pAp, &alpha);
      if (status != kPgCgRunning) break;
      for (int v = 0; v < n; ++v) t[size_t(v)] = pg_cg_update_vertex(g, v, alpha, p_new);
      rz = pg_tree_sum(t.data(), size_t(n));
    }
    *iterations = s.iterations;
    return status == kPgCgRunning ? kPgCgIterationCap : status;
  }
  double apply(double lambda, int in, int out) {
    const PgGraph g = view();
    for (int v = 0; v < n; ++v) t[size_t(v)] = pg_apply_vertex(g, v, lambda, poses[in].data(), poses[out].data());
    return pg_tree_sum(t.data(), size_t(n));
  }
  void rows(const std::vector<double>& a, int count, int first, int comps, double* out) {
    if (!out) return;
    for (int i = 0; i < count; ++i)
      for (int c = 0; c < comps; ++c) out[size_t(i) * comps + c] = a[size_t(first + c) * count + i];
  }
};
}  // namespace
extern "C" {
void* pgh_create(int n, const double* poses, const unsigned char* fixed) {
  Host* h = new Host();
  h->n = n;
  h->poses[0].assign(poses, poses + size_t(n) * 16);
  h->poses[1].assign(size_t(n) * 16, 0.0);
  h->fixed.assign(size_t(n), 0);
  if (fixed) for (int v = 0; v < n; ++v) h->fixed[size_t(v)] = fixed[v] ? 1 : 0;
  h->V.assign(size_t(n) * kPgVertexComps, 0.0);
  h->t.assign(size_t(n), 0.0);
  h->from.assign(1, 0); h->to.assign(1, 0); h->Z.assign(1, 0.0); h->om.assign(1, 0.0); h->delta.assign(1, 0.0); h->E.assign(1, 0.0);
  h->incidence();
  return h;
}
void pgh_destroy(void* p) { delete static_cast<Host*>(p); }
void pgh_set_poses(void* p, const double* poses) { Host* h = static_cast<Host*>(p); h->poses[h->cur].assign(poses, poses + size_t(h->n) * 16); }
void pgh_get_poses(void* p, double* out) { Host* h = static_cast<Host*>(p); std::memcpy(out, h->poses[h->cur].data(), size_t(h->n) * 16 * sizeof(double)); }
void pgh_set_edges(void* p, int m, const int* from, const int* to, const double* Z, const double* om, const double* delta) {
  Host* h = static_cast<Host*>(p);
  h->m = m;
  h->from.assign(from, from + m); h->to.assign(to, to + m); h->Z.assign(Z, Z + size_t(m) * 16); h->om.assign(om, om + size_t(m) * 36);
  h->delta.assign(size_t(m), 0.0);
  if (delta) h->delta.assign(delta, delta + m);
  h->from.push_back(0); h->to.push_back(0); h->Z.push_back(0.0); h->om.push_back(0.0); h->delta.push_back(0.0);
  h->E.assign(size_t(m) * kPgEdgeComps + 1, 0.0);
  h->incidence();
}
// prm: max_iterations, cg_max_iterations, cg_tolerance, min_relative_decrease, initial_damping_scale.  report: status, iterations,
// accepted, cg_iterations, initial_cost, final_cost, final_damping.  records: cost_before, cost_after, damping, cg_iterations,
// cg_status, accepted per trial.  The loop is capi_graph.inc's dvo_hip_graph_optimize.
void pgh_optimize(void* p, const double* prm, double* report, double* records, int max_records) {
  Host* h = static_cast<Host*>(p);
  const int max_iterations = int(prm[0]), cg_max = int(prm[1]);
  for (int i = 0; i < 7; ++i) report[i] = 0.0;
  report[0] = kPgNothingToDo;
  if (h->m == 0) return;
  double cost = h->linearise(h->cur, true);
  report[4] = report[5] = cost;
  if (!h->any_free) return;
  double top = h->gather();
  PgLm lm;
  pg_lm_begin(lm, cost, prm[4], top);
  report[0] = kPgIterationCap;
  for (int it = 0; it < max_iterations; ++it) {
    const double lambda = lm.lambda, before = lm.cost;
    const int other = h->cur ^ 1;
    int cg_iterations = 0, stop = -1;
    const int cg_status = h->solve(lambda, prm[2], cg_max, &cg_iterations);
    const double scale = h->apply(lambda, h->cur, other);
    const double after = h->linearise(other, false);
    const bool accepted = pg_lm_judge(lm, after, scale, cg_status, prm[3], &stop);
    if (it < max_records) {
      double* r = records + size_t(it) * 6;
      r[0] = before; r[1] = after; r[2] = lambda; r[3] = cg_iterations; r[4] = cg_status; r[5] = accepted ? 1.0 : 0.0;
    }
    report[1] += 1.0;
    report[3] += cg_iterations;
    if (accepted) { report[2] += 1.0; h->cur = other; }
    if (stop >= 0) { report[0] = stop; break; }
    if (accepted && it + 1 < max_iterations) { h->linearise(h->cur, true); h->gather(); }
  }
  report[5] = lm.cost;
  report[6] = lm.lambda;
}
void pgh_linearise(void* p, double* e, double* chi2, double* w, double* blocks, double* grad, double* cost) {
  Host* h = static_cast<Host*>(p);
  const double c = h->linearise(h->cur, true);
  h->rows(h->E, h->m, kPgE, 6, e); h->rows(h->E, h->m, kPgS, 1, chi2); h->rows(h->E, h->m, kPgW, 1, w);
  h->rows(h->E, h->m, kPgAii, 108, blocks); h->rows(h->E, h->m, kPgGi, 12, grad);
  if (cost) *cost = c;
}
void pgh_multiply(void* p, double lambda, const double* pin, double* y, double* pty, double* D, double* b, double* Minv) {
  Host* h = static_cast<Host*>(p);
  const int n = h->n;
  if (h->m > 0) h->linearise(h->cur, true);
  h->gather();
  const PgGraph g = h->view();
  for (int v = 0; v < n; ++v) { bool ok; pg_cg_init_vertex(g, v, lambda, &ok); }
  for (int v = 0; v < n; ++v)
    for (int c = 0; c < 6; ++c) h->V[size_t(kPgP0 + c) * n + v] = pin[size_t(v) * 6 + c];
  for (int v = 0; v < n; ++v) h->t[size_t(v)] = pg_multiply_vertex(g, v, lambda, kPgDirGiven, 0.0, kPgP1, kPgP0);
  if (pty) *pty = pg_tree_sum(h->t.data(), size_t(n));
  h->rows(h->V, n, kPgY, 6, y); h->rows(h->V, n, kPgD, 36, D); h->rows(h->V, n, kPgB, 6, b); h->rows(h->V, n, kPgMinv, 36, Minv);
}
// one solve at the current linearisation (after pgh_multiply): the step x (n x 6); returns the CG's status
int pgh_solve(void* p, double lambda, double tolerance, int max_iterations, double* x, int* iterations) {
  Host* h = static_cast<Host*>(p);
  const int status = h->solve(lambda, tolerance, max_iterations, iterations);
  h->rows(h->V, h->n, kPgX, 6, x);
  return status;
}
void pgh_error(const double* Xi, const double* Xj, const double* Z, double* e, double* Ji, double* Jj) { pg_error(Xi, Xj, Z, e, Ji, Jj); }
void pgh_update(const double* X, const double* dd, double* out) { pg_update(X, dd, out); }
double pgh_log1p(double x) { return pg_log1p(x); }
double pgh_tree_sum(const double* a, size_t count) { return pg_tree_sum(a, count); }
void pgh_robust(double s, double delta, double* rho, double* w) { pg_robust(s, delta, rho, w); }
int pgh_chol(const double* A, double* inv) { return pg_chol_inverse6(A, inv) ? 1 : 0; }
}
#ifdef PGH_MAIN
// stand-alone (the sanitiser build): a ring of 24 vertices with chords, one of them false, optimised under the kernel
#include <cstdio>
int main() {
  const int n = 24;
  std::vector<double> poses(size_t(n) * 16, 0.0), Z, om;
  std::vector<int> from, to;
  std::vector<unsigned char> fixed(size_t(n), 0);
  fixed[0] = 1;
  for (int v = 0; v < n; ++v) {
    double* X = &poses[size_t(v) * 16];
    X[0] = X[5] = X[10] = X[15] = 1.0;
    X[3] = 0.1 * v + 0.01 * (v % 3);
    X[7] = 0.02 * (v % 5);
  }
  for (int v = 0; v < n; ++v)
    for (int step = 1; step <= 5; step += 4) {
      const int j = (v + step) % n;
      if (j == v) continue;
      double M[16] = {1, 0, 0, 0.1 * (j - v), 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      if (v == 7 && step == 5) M[7] = 3.0;
      from.push_back(v); to.push_back(j);
      Z.insert(Z.end(), M, M + 16);
      for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) om.push_back(r == c ? 100.0 : 0.0);
    }
  std::vector<double> delta(from.size(), 5.0), report(7), records(50 * 6);
  void* h = pgh_create(n, poses.data(), fixed.data());
  pgh_set_edges(h, int(from.size()), from.data(), to.data(), Z.data(), om.data(), delta.data());
  const double prm[5] = {50, 200, 1e-8, 1e-9, 1e-5};
  pgh_optimize(h, prm, report.data(), records.data(), 50);
  pgh_get_poses(h, poses.data());
  std::printf("status %g iterations %g accepted %g cost %.17g -> %.17g\n", report[0], report[1], report[2], report[4], report[5]);
  pgh_destroy(h);
  return report[5] < report[4] ? 0 : 1;
}
#endif
"""

DEFAULTS = dict(max_iterations=50, cg_max_iterations=200, cg_tolerance=1e-8, min_relative_decrease=1e-9, initial_damping_scale=1e-5)


@functools.lru_cache(maxsize=None)
def host_lib():
    tmp = tempfile.mkdtemp(prefix="pose_graph_host_")
    src, out = os.path.join(tmp, "pose_graph_host.cpp"), os.path.join(tmp, "pose_graph_host.so")
    with open(src, "w") as f:
        f.write(HOST_SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, src, "-o", out])
    L = C.CDLL(out)
    dp, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int)
    L.pgh_create.argtypes, L.pgh_create.restype = [C.c_int, dp, C.POINTER(C.c_uint8)], vp
    L.pgh_destroy.argtypes, L.pgh_destroy.restype = [vp], None
    L.pgh_set_poses.argtypes, L.pgh_set_poses.restype = [vp, dp], None
    L.pgh_get_poses.argtypes, L.pgh_get_poses.restype = [vp, dp], None
    L.pgh_set_edges.argtypes, L.pgh_set_edges.restype = [vp, C.c_int, ip, ip, dp, dp, dp], None
    L.pgh_optimize.argtypes, L.pgh_optimize.restype = [vp, dp, dp, dp, C.c_int], None
    L.pgh_linearise.argtypes, L.pgh_linearise.restype = [vp, dp, dp, dp, dp, dp, dp], None
    L.pgh_multiply.argtypes, L.pgh_multiply.restype = [vp, C.c_double, dp, dp, dp, dp, dp, dp], None
    L.pgh_solve.argtypes, L.pgh_solve.restype = [vp, C.c_double, C.c_double, C.c_int, dp, ip], C.c_int
    L.pgh_error.argtypes, L.pgh_error.restype = [dp] * 6, None
    L.pgh_update.argtypes, L.pgh_update.restype = [dp] * 3, None
    L.pgh_log1p.argtypes, L.pgh_log1p.restype = [C.c_double], C.c_double
    L.pgh_tree_sum.argtypes, L.pgh_tree_sum.restype = [dp, C.c_size_t], C.c_double
    L.pgh_robust.argtypes, L.pgh_robust.restype = [C.c_double, C.c_double, dp, dp], None
    L.pgh_chol.argtypes, L.pgh_chol.restype = [dp, dp], C.c_int
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class HostGraph:
    """the yardstick behind the interface of dvo_slam_amd.PoseGraph (reports and records as that class returns them)"""

    def __init__(self):
        self.h, self.n, self.m = None, 0, 0

    def set_vertices(self, poses, fixed=None):
        self.close()
        T = np.ascontiguousarray(poses, np.float64)
        f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
        self.h = host_lib().pgh_create(T.shape[0], _p(T), None if f is None else f.ctypes.data_as(C.POINTER(C.c_uint8)))
        self.n, self.m, self.delta = T.shape[0], 0, np.zeros(0)

    def set_poses(self, poses):
        host_lib().pgh_set_poses(self.h, _p(np.ascontiguousarray(poses, np.float64)))

    def set_edges(self, from_, to, Z, W, delta=None):
        i, j = np.ascontiguousarray(from_, np.int32), np.ascontiguousarray(to, np.int32)
        m = len(i)
        Z, W = np.ascontiguousarray(Z, np.float64).reshape(m, 4, 4), np.ascontiguousarray(W, np.float64).reshape(m, 6, 6)
        dl = np.zeros(m) if delta is None else np.ascontiguousarray(np.broadcast_to(np.asarray(delta, np.float64), (m,)))
        ip = C.POINTER(C.c_int)
        host_lib().pgh_set_edges(self.h, m, i.ctypes.data_as(ip), j.ctypes.data_as(ip), _p(Z), _p(W), _p(dl))
        self.m, self.delta = m, dl.copy()

    def optimize(self, **params):
        p = dict(DEFAULTS, **params)
        prm = np.array([p[k] for k in ("max_iterations", "cg_max_iterations", "cg_tolerance", "min_relative_decrease", "initial_damping_scale")], np.float64)
        rep, recs = np.zeros(7), np.zeros((max(p["max_iterations"], 1), 6))
        host_lib().pgh_optimize(self.h, _p(prm), _p(rep), _p(recs), p["max_iterations"])
        out = dict(status=d._lib.GRAPH_STATUS[int(rep[0])], iterations=int(rep[1]), accepted=int(rep[2]), cg_iterations=int(rep[3]),
                   initial_cost=rep[4], final_cost=rep[5], final_damping=rep[6])
        out["records"] = [dict(cost_before=r[0], cost_after=r[1], damping=r[2], cg_iterations=int(r[3]), cg_status=d._lib.GRAPH_CG_STATUS[int(r[4])],
                               accepted=bool(r[5])) for r in recs[:int(rep[1])]]
        return out

    def poses(self):
        T = np.empty((self.n, 4, 4))
        host_lib().pgh_get_poses(self.h, _p(T))
        return T

    def linearise(self):
        """dict: error [m, 6], chi2, weight, blocks [m, 3, 6, 6] (ii, ij, jj), gradient [m, 2, 6], cost"""
        m = self.m
        e, s, w, B, g, c = np.zeros((m, 6)), np.zeros(m), np.zeros(m), np.zeros((m, 3, 6, 6)), np.zeros((m, 2, 6)), C.c_double(0)
        host_lib().pgh_linearise(self.h, _p(e), _p(s), _p(w), _p(B), _p(g), C.byref(c))
        return dict(error=e, chi2=s, weight=w, blocks=B, gradient=g, cost=c.value)

    def edge_stats(self):
        lin = self.linearise()
        return lin["chi2"], lin["weight"]

    def multiply(self, damping, p):
        """dict: y [n, 6], pty, diagonal [n, 6, 6], rhs [n, 6], inverse [n, 6, 6]"""
        n = self.n
        p = np.ascontiguousarray(p, np.float64)
        y, D, b, Mi, pty = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros((n, 6, 6)), C.c_double(0)
        host_lib().pgh_multiply(self.h, damping, _p(p), _p(y), C.byref(pty), _p(D), _p(b), _p(Mi))
        return dict(y=y, pty=pty.value, diagonal=D, rhs=b, inverse=Mi)

    def solve(self, damping, tolerance, max_iterations):
        x, it = np.zeros((self.n, 6)), C.c_int(0)
        status = host_lib().pgh_solve(self.h, damping, tolerance, max_iterations, _p(x), C.byref(it))
        return x, d._lib.GRAPH_CG_STATUS[status], it.value

    def remove_outliers(self, threshold, n_max=-1):
        return tracker.select_outliers(self.edge_stats()[1], self.delta, threshold, n_max)

    def close(self):
        if self.h:
            host_lib().pgh_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                                             # (interpreter shutdown)
            pass


# ---- numpy's own statement of the problem -------------------------------------------------------------------------------------------------

def quat_matrix(w, v):
    x, y, z = v
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def pose(t, v):
    """4 x 4 pose with translation t and the rotation of the quaternion (sqrt(1 - |v|^2), v), or (0, v / |v|) beyond |v| = 1"""
    v = np.asarray(v, np.float64)
    n2 = float(v @ v)
    w = np.sqrt(1 - n2) if n2 <= 1 else 0.0
    v = v if n2 <= 1 else v / np.sqrt(n2)
    X = np.eye(4)
    X[:3, :3], X[:3, 3] = quat_matrix(w, v), t
    return X


def np_quat_vector(R):
    """the vector part of R's unit quaternion with w >= 0, as the eigenvector of the largest eigenvalue of Bar-Itzhack's matrix"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    q = np.linalg.eigh(K)[1][:, -1]
    return q[:3] * (-1.0 if q[3] < 0 else 1.0)


def np_error(Xi, Xj, Z):
    D = np.linalg.inv(Z) @ np.linalg.inv(Xi) @ Xj
    return np.concatenate([D[:3, 3], np_quat_vector(D[:3, :3])])


def np_update(X, dd):
    return X @ pose(dd[:3], dd[3:])


def header_error(Xi, Xj, Z):
    e, Ji, Jj = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    host_lib().pgh_error(_p(np.ascontiguousarray(Xi)), _p(np.ascontiguousarray(Xj)), _p(np.ascontiguousarray(Z)), _p(e), _p(Ji), _p(Jj))
    return e, Ji, Jj


def header_update(X, dd):
    out = np.zeros((4, 4))
    host_lib().pgh_update(_p(np.ascontiguousarray(X)), _p(np.ascontiguousarray(dd, np.float64)), _p(out))
    return out


def random_pose(rng, spread=2.0, turn=0.6):
    v = rng.normal(size=3)
    return pose(rng.uniform(-spread, spread, 3), v / np.linalg.norm(v) * rng.uniform(0, turn))


def spd(rng, scale=100.0):
    A = rng.normal(size=(6, 6))
    return scale * (A @ A.T / 6 + np.eye(6))


# ---- the same for many poses at once: the graphs of edge_graphs() reach 196613 vertices, where one random_pose call per vertex takes seconds ----

def quat_matrices(w, v):
    """quat_matrix for w [k] and v [k, 3]: [k, 3, 3]; (w, v) of unit length, w of either sign"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    R = np.empty((len(w), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def poses_of(t, w, v):
    """[k, 4, 4] poses with translations t [k, 3] and the rotations of the unit quaternions (w [k], v [k, 3])"""
    X = np.zeros((len(w), 4, 4))
    X[:, :3, :3], X[:, :3, 3], X[:, 3, 3] = quat_matrices(w, v), t, 1.0
    return X


def random_poses(rng, k, spread=2.0, turn=0.6):
    """k poses as random_pose draws one"""
    v = rng.normal(size=(k, 3))
    v *= (rng.uniform(0, turn, k) / np.linalg.norm(v, axis=1))[:, None]
    return poses_of(rng.uniform(-spread, spread, (k, 3)), np.sqrt(1 - (v * v).sum(1)), v)


def spds(rng, k, scale=100.0):
    A = rng.normal(size=(k, 6, 6))
    return scale * (A @ A.transpose(0, 2, 1) / 6 + np.eye(6))


def ring_with_chords(n, m, rng):
    """(from, to) of m edges: the ring a -> a + 1 first, then random chords (repeats allowed, none from a vertex to itself)"""
    a = np.arange(min(n, m))
    i, j = a, (a + 1) % n
    if m > len(a):
        ci = rng.integers(0, n, m - len(a))
        i, j = np.concatenate([i, ci]), np.concatenate([j, (ci + rng.integers(1, n, m - len(a))) % n])
    return i.astype(np.int32), j.astype(np.int32)


def graph_of(n, i, j, seed, kernel_every=3):
    """The conventions of the GPU tier's random_graph, from arrays: n random poses, edges i -> j measured a few centimetres and 0.05 off,
    dense positive definite information, a kernel of width 2 on every third edge, every seventh vertex fixed (the first of fewer than four)"""
    rng = np.random.default_rng(seed)
    X = random_poses(rng, n)
    Z = np.linalg.inv(X[i]) @ X[j] @ random_poses(rng, len(i), 0.1, 0.05)
    fixed = np.arange(n) % 7 == 3 if n > 3 else np.arange(n) == 0
    return dict(start=X, fixed=fixed, edges=(i, j, Z, spds(rng, len(i))), delta=np.where(np.arange(len(i)) % kernel_every == 0, 2.0, 0.0))


# ---- the graphs of the convergence tests (tests/test_gpu_pose_graph.py runs the same three on the device) ---------------------------------

def helix(n):
    return np.stack([pose([np.cos(0.3 * k), np.sin(0.3 * k), 0.05 * k], np.array([0.0, 0.0, np.sin(0.15 * k)]) * 0.9 + [0.05, 0.02, 0.0]) for k in range(n)])


def edges_of(truth, steps, rng=None, sigma_t=0.0, sigma_r=0.0):
    """(from, to, Z, Omega): i -> i + s for s in steps, measured from `truth` with noise M(d), d ~ N(0, sigma)"""
    n = len(truth)
    i = np.array([a for s in steps for a in range(n - s)], np.int32)
    j = np.array([a + s for s in steps for a in range(n - s)], np.int32)
    Z = np.stack([np.linalg.inv(truth[a]) @ truth[b] for a, b in zip(i, j)])
    if rng is not None:
        Z = np.stack([np_update(z, np.concatenate([rng.normal(0, sigma_t, 3), rng.normal(0, sigma_r, 3)])) for z in Z])
    W = np.tile(np.diag([1e4] * 3 + [4e4] * 3), (len(i), 1, 1)) if sigma_t == 0 else np.tile(np.diag([1 / sigma_t ** 2] * 3 + [1 / sigma_r ** 2] * 3), (len(i), 1, 1))
    return i, j, Z, W


def noise_free_graph():
    """40 poses on a helix, edges i -> i + 1 and i -> i + 10, vertex 0 fixed, started 5 cm and 0.03 off"""
    rng = np.random.default_rng(7)
    truth = helix(40)
    i, j, Z, W = edges_of(truth, (1, 10))
    start = truth.copy()
    for k in range(1, 40):
        dt, dv = rng.normal(size=3), rng.normal(size=3)
        start[k] = np_update(truth[k], np.concatenate([0.05 * dt / np.linalg.norm(dt), 0.03 * dv / np.linalg.norm(dv)]))
    fixed = np.zeros(40, bool)
    fixed[0] = True
    return dict(truth=truth, start=start, fixed=fixed, edges=(i, j, Z, W), delta=None)


def noisy_graph():
    """60 poses, edges i -> i + 1, + 7, + 20 with noise sigma = 1 cm and 0.005, started from the integrated odometry"""
    rng = np.random.default_rng(11)
    truth = helix(60)
    i, j, Z, W = edges_of(truth, (1, 7, 20), rng, 0.01, 0.005)
    start = truth.copy()
    for k in range(1, 60):
        start[k] = start[k - 1] @ Z[k - 1]                           # (the first 59 edges are k - 1 -> k)
    fixed = np.zeros(60, bool)
    fixed[0] = True
    return dict(truth=truth, start=start, fixed=fixed, edges=(i, j, Z, W), delta=None)


PLANTED = ((3, 41), (12, 55), (25, 2), (48, 9))


def outlier_graph():
    """the noisy graph with four gross false edges, delta = 5 on every edge"""
    g = noisy_graph()
    i, j, Z, W = g["edges"]
    rng = np.random.default_rng(13)
    false_Z = np.stack([random_pose(rng, 3.0, 0.7) for _ in PLANTED])
    at = [20, 61, 100, 140]                                           # where they go: among the others, not at the end
    order = list(range(len(i)))
    for k, where in enumerate(at):
        order.insert(where, len(i) + k)
    i = np.concatenate([i, [a for a, _ in PLANTED]]).astype(np.int32)[order]
    j = np.concatenate([j, [b for _, b in PLANTED]]).astype(np.int32)[order]
    Z, W = np.concatenate([Z, false_Z])[order], np.concatenate([W, W[:4]])[order]
    g.update(edges=(i, j, Z, W), delta=5.0, planted=np.array(at))
    return g


def load(graph, g, start=None):
    graph.set_vertices(g["start"] if start is None else start, g["fixed"])
    graph.set_edges(*g["edges"], g["delta"])
    return graph


def max_position_error(poses, truth):
    return float(np.abs(poses[:, :3, 3] - truth[:, :3, 3]).max())


@functools.lru_cache(maxsize=None)
def yardstick_run(name):
    """(graph dict, report, final poses, final weights) of the yardstick on one of the three graphs: computed once, shared, not modified"""
    g = dict(noise_free=noise_free_graph, noisy=noisy_graph, outliers=outlier_graph)[name]()
    h = load(HostGraph(), g)
    report = h.optimize()
    return g, report, h.poses(), h.edge_stats()[1], h


# ---- the inputs of tests/test_gpu_pose_graph_edges.py: what each is there for is asserted on the yardstick below, without a GPU ------------

HALF_TURNS = (125.0, 170.0, 179.999, 180.0, 200.0)                   # degrees of the relative rotation error; 200 = 160 about the opposite axis
HALF_TURN_DELTAS = (0.0, 1e-3, 2.0, 1e6)


def half_turn_graph():
    """70 poses, the ring and 80 chords.  Five edges of six have an error Z^-1 X_i^-1 X_j that turns by HALF_TURNS in turn about an axis
    dominated by x, y, z in turn and lies 0.1 off, under a kernel of width HALF_TURN_DELTAS in turn (60 combinations, each at least
    twice); the sixth is an ordinary edge of graph_of.  Every angle is beyond 120 degrees, where the trace turns negative."""
    g = graph_of(70, *ring_with_chords(70, 150, np.random.default_rng(31)), 32)
    rng = np.random.default_rng(33)
    i, j, Z, W = g["edges"]
    at = np.nonzero(np.arange(150) % 6 != 5)[0]
    h = np.arange(len(at))
    half = np.radians(np.array(HALF_TURNS))[h % 5] / 2
    axis = np.array([[1.0, 0.2, -0.1], [0.15, 1.0, 0.25], [-0.2, 0.1, 1.0]])[h % 3] + rng.uniform(-0.05, 0.05, (len(at), 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    w = np.where(h % 5 == 3, 0.0, np.cos(half))                       # (exactly a half turn: w = 0, a symmetric matrix)
    t = rng.normal(size=(len(at), 3))
    error = poses_of(0.1 * t / np.linalg.norm(t, axis=1)[:, None], w, axis * np.where(h % 5 == 3, 1.0, np.sin(half))[:, None])
    Z, delta = Z.copy(), g["delta"].copy()
    Z[at] = np.linalg.inv(g["start"][i[at]]) @ g["start"][j[at]] @ np.linalg.inv(error)
    delta[at] = np.array(HALF_TURN_DELTAS)[h % 4]
    return dict(g, edges=(i, j, Z, W), delta=delta, half_turns=at)


def chain_graph(kind):
    """300 vertices, edges k -> k + 1, vertex 0 fixed, dense positive definite information.  "exact": poses and measurements whose
    error is exactly zero (translations by dyadic fractions).  Else the helix at its true poses, every measurement 1 cm and 0.01 off;
    "negative_last": the last edge (298 -> 299) carries -1e3 I, so the only blocks without a factor belong to vertices of the second
    workgroup; "indefinite_100": edge 100 carries 100 A, A the identity with A[0, 1] = A[1, 0] = 5."""
    n = 300
    rng = np.random.default_rng(41)
    i = np.arange(n - 1, dtype=np.int32)
    W = spds(rng, n - 1)
    if kind == "exact":
        X = np.tile(np.eye(4), (n, 1, 1))
        X[:, 0, 3], X[:, 1, 3] = 0.25 * np.arange(n), 0.125 * np.arange(n)
        Z = np.tile(pose([0.25, 0.125, 0.0], [0, 0, 0]), (n - 1, 1, 1))
    else:
        X = helix(n)
        dt, dv = rng.normal(size=(n - 1, 3)), rng.normal(size=(n - 1, 3))
        dv *= 0.01 / np.linalg.norm(dv, axis=1)[:, None]
        Z = np.linalg.inv(X[:-1]) @ X[1:] @ poses_of(0.01 * dt / np.linalg.norm(dt, axis=1)[:, None], np.sqrt(1 - (dv * dv).sum(1)), dv)
        if kind == "negative_last":
            W[298] = -1e3 * np.eye(6)
        if kind == "indefinite_100":
            W[100] = 100.0 * np.eye(6)
            W[100, 0, 1] = W[100, 1, 0] = 500.0
    return dict(start=X, fixed=np.arange(n) == 0, edges=(i, i + 1, Z, W), delta=None)


def no_edges(n):
    g = graph_of(n, np.zeros(0, np.int32), np.zeros(0, np.int32), 50 + n)
    return dict(g, delta=None)


# name: builder.  (n, m) and what the kernels do there: tests/test_gpu_pose_graph_edges.py
EDGE_GRAPHS = {
    "full_block": lambda: graph_of(256, *ring_with_chords(256, 256, np.random.default_rng(61)), 62),
    "three_blocks": lambda: graph_of(513, *ring_with_chords(513, 1281, np.random.default_rng(63)), 64),
    "ring_65537": lambda: graph_of(65537, *ring_with_chords(65537, 65537, np.random.default_rng(65)), 66),
    "few_vertices": lambda: graph_of(90, *ring_with_chords(90, 65537, np.random.default_rng(67)), 68),
    "ring_196613": lambda: graph_of(196613, *ring_with_chords(196613, 196613, np.random.default_rng(69)), 70),
    "half_turns": half_turn_graph,
    "no_edges_1": lambda: no_edges(1),
    "no_edges_300": lambda: no_edges(300),
    "two": lambda: graph_of(2, *ring_with_chords(2, 1, np.random.default_rng(71)), 72),
    "small": lambda: graph_of(90, *ring_with_chords(90, 260, np.random.default_rng(73)), 74),
    "ring_600": lambda: graph_of(600, *ring_with_chords(600, 1500, np.random.default_rng(75)), 76),
    "chain_exact": lambda: chain_graph("exact"),
    "chain_off": lambda: chain_graph("off"),
    "chain_negative_last": lambda: chain_graph("negative_last"),
    "chain_indefinite_100": lambda: chain_graph("indefinite_100"),
}

# name: (graph, parameters of optimize, the status the optimisation must end in or None, CG statuses that must occur in the records)
EDGE_RUNS = {
    "many_workgroups": ("ring_600", dict(max_iterations=8), None, ()),
    "long_tree": ("ring_65537", dict(max_iterations=2, cg_max_iterations=5), "iteration_cap", ("iteration_cap",)),
    "cg_cap_1": ("ring_600", dict(max_iterations=6, cg_max_iterations=1), None, ("iteration_cap",)),
    "cg_cap_2": ("ring_600", dict(max_iterations=6, cg_max_iterations=2), None, ("iteration_cap",)),
    "cg_cap_3": ("ring_600", dict(max_iterations=6, cg_max_iterations=3), None, ("iteration_cap",)),
    "cg_cap_4": ("ring_600", dict(max_iterations=6, cg_max_iterations=4), None, ("iteration_cap",)),
    "zero_rhs": ("chain_exact", dict(), "converged", ("zero_rhs",)),
    "cholesky_in_workgroup_1": ("chain_negative_last", dict(max_iterations=15), None, ("cholesky",)),
    "breakdown": ("chain_indefinite_100", dict(max_iterations=15), None, ("cholesky", "breakdown")),
    "damping_overflow": ("chain_off", dict(initial_damping_scale=1e300), "damping_overflow", ()),
    "lm_iteration_cap": ("chain_off", dict(max_iterations=3), "iteration_cap", ()),
    "large_steps": ("half_turns", dict(max_iterations=20), None, ()),
    "reuse_two": ("two", dict(max_iterations=2), None, ()),
    "reuse_three_blocks": ("three_blocks", dict(max_iterations=2), None, ()),
    "small": ("small", dict(), None, ()),
}


@functools.lru_cache(maxsize=None)
def edge_graph(name):
    """one of EDGE_GRAPHS as load() takes it: built once, shared, not modified"""
    return EDGE_GRAPHS[name]()


def edge_graphs():
    """every named input of the GPU tier's edge cases"""
    return {name: edge_graph(name) for name in EDGE_GRAPHS}


@functools.lru_cache(maxsize=None)
def edge_run(name):
    """(graph, report, final poses, final weights) of the yardstick on one of EDGE_RUNS: computed once, shared, not modified"""
    graph, params, _, _ = EDGE_RUNS[name]
    h = load(HostGraph(), edge_graph(graph))
    report = h.optimize(**params)
    out = edge_graph(graph), report, h.poses(), h.edge_stats()[1]
    h.close()
    return out


def quat_branches(g):
    """per edge, the branch pg_quat takes on the rotation of Z^-1 X_i^-1 X_j: 0 for a positive trace, else 1 + the index of the largest
    diagonal entry"""
    i, j, Z, _ = g["edges"]
    R = (np.linalg.inv(Z) @ np.linalg.inv(g["start"][i]) @ g["start"][j])[:, :3, :3]
    diagonal = np.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], 1)
    return np.where(diagonal.sum(1) > 0, 0, 1 + diagonal.argmax(1))


def test_the_batched_builder_makes_rigid_poses_and_a_long_ring_quickly():
    import time
    seconds = []
    while len(seconds) < 3 and min(seconds, default=1.0) >= 1.0:      # (the best of at most three: a busy machine is not a slow builder)
        t0 = time.perf_counter()
        g = EDGE_GRAPHS["ring_65537"]()
        seconds.append(time.perf_counter() - t0)
    X, (i, j, Z, W) = g["start"], g["edges"]
    print("65537 vertices and edges built in", seconds, "s")
    assert min(seconds) < 1.0                                         # (the loop over random_pose took 1.7 s)
    for T in (X, Z):
        R = T[:, :3, :3]
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 16 * EPS and np.all(np.linalg.det(R) > 0.99) and np.all(T[:, 3] == [0, 0, 0, 1])
    assert np.array_equal(i, np.arange(65537)) and np.array_equal(j, (np.arange(65537) + 1) % 65537)
    assert np.all(np.linalg.eigvalsh(W[:100]) >= 100.0 * (1 - 1e-12)) and np.array_equal(W, W.transpose(0, 2, 1))
    assert g["fixed"][3] and g["fixed"].sum() == (65537 + 3) // 7 and 0 < (g["delta"] > 0).sum() < len(i)
    rng = np.random.default_rng(9)
    one = random_poses(rng, 1)[0]
    assert np.abs(quat_matrices(np.array([0.5]), np.array([[0.5, -0.5, 0.5]]))[0] - quat_matrix(0.5, [0.5, -0.5, 0.5])).max() == 0 and one.shape == (4, 4)
    i, j = ring_with_chords(90, 65537, rng)
    assert np.all(i != j) and 1300 < np.bincount(np.concatenate([i, j]), minlength=90).min()


def test_the_edge_graphs_do_what_they_are_there_for():
    """Each input of the GPU tier's edge cases on the yardstick: the endings occur, the branches are taken.  A change to a generator that
    turns a case into an easy one fails here, without a GPU."""
    shapes = dict(full_block=(256, 256), three_blocks=(513, 1281), ring_65537=(65537, 65537), few_vertices=(90, 65537), ring_196613=(196613, 196613),
                  half_turns=(70, 150), no_edges_1=(1, 0), no_edges_300=(300, 0), two=(2, 1), small=(90, 260), ring_600=(600, 1500),
                  chain_exact=(300, 299), chain_off=(300, 299), chain_negative_last=(300, 299), chain_indefinite_100=(300, 299))
    for name, g in edge_graphs().items():
        i, j, Z, W = g["edges"]
        assert (len(g["start"]), len(i)) == shapes[name] and Z.shape == (len(i), 4, 4) and W.shape == (len(i), 6, 6) and np.all(i != j), name
        assert all(np.all(np.isfinite(a)) for a in (g["start"], Z, W)) and g["fixed"].shape == (len(g["start"]),), name
        assert i.dtype == j.dtype == np.int32 and (not len(i) or (min(i.min(), j.min()) >= 0 and max(i.max(), j.max()) < len(g["start"]))), name
    assert sorted(shapes) == sorted(EDGE_GRAPHS) and all(graph in EDGE_GRAPHS for graph, _, _, _ in EDGE_RUNS.values())
    for name, (graph, params, lm_status, cg_statuses) in EDGE_RUNS.items():
        g, report, poses, _ = edge_run(name)
        seen = [r["cg_status"] for r in report["records"]]
        print(name, report["status"], report["iterations"], report["accepted"], {s: seen.count(s) for s in sorted(set(seen))})
        assert lm_status is None or report["status"] == lm_status, name
        for status in cg_statuses:
            assert status in seen, (name, status)
        assert np.all(np.isfinite(poses)), name
    # across workgroups: three vertex blocks, an optimisation that moves
    report = edge_run("many_workgroups")[1]
    assert report["accepted"] >= 3 and report["final_cost"] < report["initial_cost"] and report["cg_iterations"] > 8 * 4
    # the long tree: the first trial accepted, so the second's damping went through the scale's tree
    records = edge_run("long_tree")[1]["records"]
    assert len(records) == 2 and records[0]["accepted"] and records[1]["damping"] != records[0]["damping"]
    assert [r["cg_iterations"] for r in records] == [5, 5]
    for cap in (1, 2, 3, 4):
        records = edge_run("cg_cap_%d" % cap)[1]["records"]
        assert len(records) == 6 and all(r["cg_status"] == "iteration_cap" and r["cg_iterations"] == cap for r in records)
    report = edge_run("zero_rhs")[1]
    assert report["initial_cost"] == 0.0 and report["iterations"] == 1 and report["accepted"] == 0
    # the blocks without a factor: vertices of the second workgroup only
    g = edge_graph("chain_negative_last")
    h = load(HostGraph(), g)
    damping = edge_run("cholesky_in_workgroup_1")[1]["records"][0]["damping"]
    out = h.multiply(damping, np.zeros((300, 6)))
    no_factor = np.nonzero(~out["inverse"].any(axis=(1, 2)) & ~g["fixed"])[0]
    assert len(no_factor) and no_factor.min() >= 256, no_factor
    h.close()
    seen = [r["cg_status"] for r in edge_run("cholesky_in_workgroup_1")[1]["records"]]
    assert seen[0] == "cholesky" and "converged" in seen              # (the damping grows past the block, then trials solve)
    assert edge_run("damping_overflow")[1]["iterations"] < 50 and edge_run("lm_iteration_cap")[1]["iterations"] == 3
    # the half turns: every branch of pg_quat, both ends of pg_log1p, a step beyond the unit quaternion
    g = edge_graph("half_turns")
    branches = np.bincount(quat_branches(g), minlength=4)
    print("pg_quat branches", branches)
    assert np.all(branches >= 5) and np.all(quat_branches(g)[g["half_turns"]] > 0)
    h = load(HostGraph(), g)
    ratio = h.linearise()["chi2"][g["delta"] > 0] / g["delta"][g["delta"] > 0] ** 2
    assert ratio.max() > 1e6 and ratio.min() < 1e-6
    h.multiply(0.0, np.zeros((70, 6)))
    x, status, _ = h.solve(edge_run("large_steps")[1]["records"][0]["damping"], DEFAULTS["cg_tolerance"], DEFAULTS["cg_max_iterations"])
    beyond = int(((x[:, 3:] ** 2).sum(1) > 1).sum())
    print("the first trial's step:", status, beyond, "vertices beyond |v| = 1")
    assert beyond >= 1
    h.close()
    R = edge_run("large_steps")[2][:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14
    for name in ("no_edges_1", "no_edges_300"):
        h = load(HostGraph(), edge_graph(name))
        assert h.optimize()["status"] == "nothing_to_do" and h.linearise()["cost"] == 0.0 and not h.multiply(3.7, np.ones((h.n, 6)))["y"].any()
        h.close()


# ---- the definitions, independent of the header --------------------------------------------------------------------------------------------

def test_error_chi2_weight_and_rho_equal_the_numpy_restatement():
    rng = np.random.default_rng(1)
    L = host_lib()
    cases = [(random_pose(rng), random_pose(rng), random_pose(rng)) for _ in range(40)]
    Xi = random_pose(rng)
    far = pose([0.3, -0.2, 0.1], np.array([0.6, 0.5, 0.4]) / np.linalg.norm([0.6, 0.5, 0.4]) * np.sin(np.radians(130) / 2))   # a relative turn of 130 degrees: w >= 0
    near_pi = pose([0.1, 0.2, 0.3], np.array([0.2, -0.7, 0.68]) / np.linalg.norm([0.2, -0.7, 0.68]) * np.sin(np.radians(179.9) / 2))
    cases += [(Xi, Xi @ far, np.eye(4)), (Xi, Xi @ near_pi, np.eye(4)), (Xi, Xi @ far @ far, np.eye(4))]      # the last: 260 degrees = -100: the sign flips
    for k, (a, b, z) in enumerate(cases):
        e, want = header_error(a, b, z)[0], np_error(a, b, z)
        # rounding: three 4 x 4 products of entries up to T = 1 + the largest translation, and a quaternion of unit length
        T = 1 + max(np.abs(x[:3, 3]).max() for x in (a, b, z))
        assert np.abs(e - want).max() <= 256 * EPS * T * T, (k, e, want)
        W = spd(rng)
        s = float(want @ W @ want)
        for delta in (0.0, 5.0, 0.01):
            rho, w = C.c_double(), C.c_double()
            L.pgh_robust(float(e @ W @ e), delta, C.byref(rho), C.byref(w))
            want_rho, want_w = (delta ** 2 * np.log1p(s / delta ** 2), 1 / (1 + s / delta ** 2)) if delta > 0 else (s, 1.0)
            assert abs(rho.value - want_rho) <= 1e-11 * abs(want_rho) + 1e-300 and abs(w.value - want_w) <= 1e-11 * want_w
    assert header_error(*cases[-3])[0][3:] @ header_error(*cases[-3])[0][3:] > np.sin(np.radians(45)) ** 2        # beyond 90 degrees
    assert np.linalg.norm(header_error(*cases[-2])[0][3:]) > 0.999999


def test_log1p_is_within_four_ulp_of_the_libm():
    L = host_lib()
    xs = np.concatenate([10.0 ** np.arange(-18, 19, 0.37), [0.0, 1.0, 0.4142135623730951, 1e-300, 3.0, 1e300], -1 + 10.0 ** np.arange(-12, 0, 0.9)])
    for x in xs:
        got, want = L.pgh_log1p(float(x)), np.log1p(x)
        assert abs(got - want) <= 4 * np.spacing(abs(want)), (x, got, want)
    assert np.isnan(L.pgh_log1p(-2.0)) and L.pgh_log1p(float("inf")) == float("inf")


def test_the_tree_sum_is_the_adjacent_pair_tree():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 64, 65, 255, 256, 257, 1000, 65536, 65537, 196613):      # (the last three: the sizes of edge_graphs())
        a = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, n)
        t = np.concatenate([a, np.zeros((1 << int(np.ceil(np.log2(n))) if n > 1 else 1) - n)])
        while len(t) > 1:
            t = t[0::2] + t[1::2]
        assert host_lib().pgh_tree_sum(_p(a), n) == t[0] + 0.0


def test_jacobians_agree_with_central_differences_of_the_numpy_error():
    """Central differences with step h of a function whose third derivatives are bounded by B and whose values by F carry a truncation
    error of at most h^2 B / 6 and a rounding error of at most eps F / h (two evaluations, each wrong by eps F at most, over 2 h) --
    times the factor G by which np_error's own rounding exceeds eps F: three matrix products and an eigenvector, taken as 16.
    F = T = 1 + the largest translation in the chain.  B: the rotation by the quaternion (sqrt(1 - |v|^2), v) turns by 2 asin |v|,
    so each derivative with respect to v brings a factor of at most 2, and the sqrt's own derivatives are bounded by 2 for |v| <= h:
    B <= 2^3 T + 8 = 16 T.  With h = 1e-5: 1e-10 * 16 T / 6 + 16 * 2.2e-16 T / 1e-5 = 6.2e-10 T."""
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(20):
        Xi, Xj, Z = random_pose(rng), random_pose(rng), random_pose(rng)
        T = 1 + max(np.abs(x[:3, 3]).max() for x in (Xi, Xj, Z)) * 3
        bound = h * h * 16 * T / 6 + 16 * EPS * T / h
        _, Ji, Jj = header_error(Xi, Xj, Z)
        for c in range(6):
            dd = np.zeros(6)
            dd[c] = h
            ci = (np_error(np_update(Xi, dd), Xj, Z) - np_error(np_update(Xi, -dd), Xj, Z)) / (2 * h)
            cj = (np_error(Xi, np_update(Xj, dd), Z) - np_error(Xi, np_update(Xj, -dd), Z)) / (2 * h)
            assert np.abs(Ji[:, c] - ci).max() <= bound and np.abs(Jj[:, c] - cj).max() <= bound, (c, np.abs(Ji[:, c] - ci).max(), np.abs(Jj[:, c] - cj).max(), bound)


def twelve_vertex_graph():
    rng = np.random.default_rng(4)
    n = 12
    X = np.stack([random_pose(rng) for _ in range(n)])
    pairs = [(a, (a + 1) % n) for a in range(n)] + [(0, 5), (7, 2), (3, 9), (11, 4), (5, 0), (2, 7)]
    i, j = np.array([a for a, _ in pairs], np.int32), np.array([b for _, b in pairs], np.int32)
    Z = np.stack([np.linalg.inv(X[a]) @ X[b] @ random_pose(rng, 0.1, 0.05) for a, b in pairs])
    W = np.stack([spd(rng) for _ in pairs])
    delta = np.where(np.arange(len(pairs)) % 3 == 0, 2.0, 0.0)
    fixed = np.zeros(n, bool)
    fixed[4] = True
    return X, fixed, i, j, Z, W, delta


def dense_system(X, fixed, i, j, Z, W, delta):
    """(H, b) over all 6 n unknowns from the header's per-edge e and J (held to numpy above), assembled by numpy"""
    n = len(X)
    H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for a, c, z, om, dl in zip(i, j, Z, W, delta):
        e, Ji, Jj = header_error(X[a], X[c], z)
        w = 1 / (1 + e @ om @ e / dl ** 2) if dl > 0 else 1.0
        J = np.zeros((6, 6 * n))
        J[:, 6 * a:6 * a + 6], J[:, 6 * c:6 * c + 6] = Ji, Jj
        H += w * J.T @ om @ J
        b -= w * J.T @ om @ e
    return H, b


def test_gathered_blocks_equal_the_dense_system_and_the_multiply_its_product():
    X, fixed, i, j, Z, W, delta = twelve_vertex_graph()
    n = len(X)
    H, b = dense_system(X, fixed, i, j, Z, W, delta)
    h = HostGraph()
    h.set_vertices(X, fixed)
    h.set_edges(i, j, Z, W, delta)
    lam = 0.37
    p = np.random.default_rng(5).normal(size=(n, 6))
    p[fixed] = 0.0
    out = h.multiply(lam, p)
    free = ~fixed
    scale = np.abs(H).max()
    tol = 64 * EPS * scale                                            # sums of at most 4 edges x 6 x 6 products per entry
    for v in range(n):
        blk = H[6 * v:6 * v + 6, 6 * v:6 * v + 6]
        if free[v]:
            assert np.abs(out["diagonal"][v] - blk).max() <= tol and np.abs(out["rhs"][v] - b[6 * v:6 * v + 6]).max() <= tol * np.abs(Z[:, :3, 3]).max() * 4
            assert np.abs(out["inverse"][v] @ (blk + lam * np.eye(6)) - np.eye(6)).max() <= 1e-10
        else:
            assert not out["diagonal"][v].any() and not out["rhs"][v].any() and not out["inverse"][v].any() and not out["y"][v].any()
    want = (H + lam * np.eye(6 * n)) @ p.reshape(-1)
    assert np.abs(out["y"].reshape(-1) - want)[np.repeat(free, 6)].max() <= 64 * EPS * scale * 6 * 5 * np.abs(p).max()
    assert abs(out["pty"] - p.reshape(-1)[np.repeat(free, 6)] @ want[np.repeat(free, 6)]) <= 1e-12 * abs(out["pty"])


def test_the_cg_step_meets_its_own_stopping_measure():
    X, fixed, i, j, Z, W, delta = twelve_vertex_graph()
    n = len(X)
    H, b = dense_system(X, fixed, i, j, Z, W, delta)
    h = HostGraph()
    h.set_vertices(X, fixed)
    h.set_edges(i, j, Z, W, delta)
    keep = np.repeat(~fixed, 6)
    for lam, tol in ((1.0, 1e-6), (1e-3, 1e-10), (50.0, 1e-3)):
        out = h.multiply(lam, np.zeros((n, 6)))
        x, status, iterations = h.solve(lam, tol, 500)
        assert status == "converged" and 0 < iterations < 500
        A = (H + lam * np.eye(6 * n))[keep][:, keep]
        Minv = np.zeros_like(A)
        at = 0
        for v in range(n):
            if not fixed[v]:
                Minv[at:at + 6, at:at + 6] = out["inverse"][v]
                at += 6
        r = b[keep] - A @ x.reshape(-1)[keep]
        assert np.sqrt(r @ Minv @ r) <= tol * np.sqrt(b[keep] @ Minv @ b[keep]) * (1 + 1e-6)
        assert not x[fixed].any()


def test_a_thousand_chained_updates_leave_a_rotation():
    rng = np.random.default_rng(6)
    X = random_pose(rng)
    for k in range(1000):
        X = header_update(X, rng.normal(size=6) * 0.2)
        if k % 250 == 249:
            X = header_update(X, np.array([0, 0, 0, 1.5, -0.7, 0.3]))    # |v|^2 > 1: normalised, w = 0: a half turn
    R = X[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1) <= 1e-15 and list(X[3]) == [0, 0, 0, 1]
    Y = random_pose(rng)
    dd = rng.normal(size=6) * 0.3
    assert np.abs(header_update(Y, dd) - np_update(Y, dd)).max() <= 64 * EPS * 3
    assert np.array_equal(header_update(Y, np.zeros(6)), Y) and np.array_equal(header_update(Y, np.array([0, np.nan, 0, 0, 0, 0])), Y)


# ---- convergence ------------------------------------------------------------------------------------------------------------------------------

def records_are_consistent(report):
    recs = report["records"]
    assert len(recs) == report["iterations"] and sum(r["accepted"] for r in recs) == report["accepted"]
    assert sum(r["cg_iterations"] for r in recs) == report["cg_iterations"]
    cost = report["initial_cost"]
    for r in recs:
        assert r["cost_before"] == cost and np.isfinite(r["cost_after"]) and r["damping"] > 0
        if r["accepted"]:
            assert r["cost_after"] < cost
            cost = r["cost_after"]
    assert report["final_cost"] == cost


def test_noise_free_helix_returns_to_the_ground_truth():
    g, report, poses, _, _ = yardstick_run("noise_free")
    print(report["status"], report["iterations"], report["accepted"], report["cg_iterations"], report["initial_cost"], report["final_cost"],
          max_position_error(poses, g["truth"]))
    assert max_position_error(g["start"], g["truth"]) > 0.02
    assert max_position_error(poses, g["truth"]) < 1e-9 and np.abs(poses - g["truth"]).max() < 1e-9
    assert report["status"] in ("converged", "stalled") and np.array_equal(poses[0], g["start"][0])
    records_are_consistent(report)


def test_noisy_graph_improves_on_the_odometry():
    g, report, poses, _, _ = yardstick_run("noisy")
    print(report["status"], report["iterations"], report["accepted"], report["initial_cost"], report["final_cost"],
          max_position_error(g["start"], g["truth"]), max_position_error(poses, g["truth"]))
    assert report["final_cost"] < report["initial_cost"] and report["accepted"] >= 1
    assert max_position_error(poses, g["truth"]) < max_position_error(g["start"], g["truth"])
    assert np.all(np.isfinite(poses))
    records_are_consistent(report)


def test_planted_false_edges_get_the_lowest_weights_and_are_removed():
    g, report, poses, weights, h = yardstick_run("outliers")
    planted = np.zeros(len(weights), bool)
    planted[g["planted"]] = True
    print(report["status"], report["iterations"], weights[planted].max(), weights[~planted].min())
    assert [(int(a), int(b)) for a, b in zip(g["edges"][0][planted], g["edges"][1][planted])] == list(PLANTED)
    assert weights[planted].max() < weights[~planted].min()
    assert sorted(h.remove_outliers(0.1)) == sorted(g["planted"])
    assert np.all(np.isfinite(poses)) and report["final_cost"] < report["initial_cost"]
    records_are_consistent(report)
    # lowest first, at most n_max, only edges with a kernel
    w = np.array([0.5, 0.01, 0.05, 0.02, 0.03])
    assert list(tracker.select_outliers(w, np.array([5.0, 5, 0, 5, 5]), 0.1)) == [1, 3, 4]
    assert list(tracker.select_outliers(w, np.full(5, 5.0), 0.1, 2)) == [1, 3] and list(tracker.select_outliers(w, np.full(5, 5.0), 0.1, 0)) == []


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------------------

def test_an_isolated_and_a_fixed_vertex_come_back_bit_for_bit():
    g = noisy_graph()
    start = np.concatenate([g["start"], [pose([5, 5, 5], [0.1, 0.2, 0.3])]])     # vertex 60 has no edge
    fixed = np.concatenate([g["fixed"], [False]])
    fixed[30] = True
    h = HostGraph()
    h.set_vertices(start, fixed)
    h.set_edges(*g["edges"])
    report = h.optimize(max_iterations=6)
    poses = h.poses()
    assert report["accepted"] >= 1 and not np.array_equal(poses[10], start[10])
    for v in (0, 30, 60):
        assert np.array_equal(poses[v], start[v])


def test_nothing_to_do_runs_no_iteration():
    g = noisy_graph()
    h = load(HostGraph(), dict(g, fixed=np.ones(60, bool)))
    report = h.optimize()
    assert report["iterations"] == 0 and report["status"] == "nothing_to_do" and report["initial_cost"] == report["final_cost"] > 0
    assert np.array_equal(h.poses(), g["start"])
    h.set_vertices(g["start"], g["fixed"])
    report = h.optimize()
    assert report["iterations"] == 0 and report["status"] == "nothing_to_do" and report["final_cost"] == 0 and np.array_equal(h.poses(), g["start"])


def test_duplicate_edges_equal_one_edge_with_the_summed_information():
    """Without a kernel the two graphs have the same H and b up to the rounding of w J^T (W1 + W2) J against the sum of two such
    products: 64 eps of the largest entry.  The optimised poses agree as far as both runs have converged: 1e-9."""
    X, fixed, i, j, Z, W, _ = twelve_vertex_graph()
    rng = np.random.default_rng(8)
    W2 = spd(rng)
    a, b = HostGraph(), HostGraph()
    a.set_vertices(X, fixed)
    b.set_vertices(X, fixed)
    a.set_edges(np.append(i, i[3]), np.append(j, j[3]), np.concatenate([Z, Z[3:4]]), np.concatenate([W, [W2]]))
    Wsum = W.copy()
    Wsum[3] += W2
    b.set_edges(i, j, Z, Wsum)
    p = rng.normal(size=(len(X), 6))
    ma, mb = a.multiply(0.5, p), b.multiply(0.5, p)
    scale = max(np.abs(mb["diagonal"]).max(), np.abs(mb["y"]).max())
    for key in ("diagonal", "rhs", "y"):
        assert np.abs(ma[key] - mb[key]).max() <= 64 * EPS * scale, key
    ca, cb = a.linearise()["cost"], b.linearise()["cost"]
    assert abs(ca - cb) <= 64 * EPS * cb
    ra, rb = a.optimize(), b.optimize()
    assert ra["status"] == rb["status"] and np.abs(a.poses() - b.poses()).max() < 1e-9


def test_a_singular_information_on_a_dangling_vertex_ends_in_a_status():
    g = noisy_graph()
    i, j, Z, W = g["edges"]
    start = np.concatenate([g["start"], [g["start"][59] @ pose([0.1, 0, 0], [0, 0, 0.01])]])
    fixed = np.concatenate([g["fixed"], [False]])
    for info in (np.zeros((6, 6)), np.diag([1e4, 0, 0, 0, 0, 0]), -np.eye(6)):
        h = HostGraph()
        h.set_vertices(start, fixed)
        h.set_edges(np.append(i, 59).astype(np.int32), np.append(j, 60).astype(np.int32), np.concatenate([Z, [pose([0.2, 0, 0], [0, 0, 0])]]),
                    np.concatenate([W, [info]]))
        report = h.optimize(max_iterations=15)
        assert report["status"] in d._lib.GRAPH_STATUS.values() and np.all(np.isfinite(h.poses())) and np.isfinite(report["final_cost"])
        assert all(r["cg_status"] in d._lib.GRAPH_CG_STATUS.values() for r in report["records"])


def test_a_vertex_whose_block_has_no_factor_rejects_the_trial():
    X = np.stack([np.eye(4), pose([1, 0, 0], [0, 0, 0])])
    h = HostGraph()
    h.set_vertices(X, [True, False])
    h.set_edges([0], [1], [pose([1.1, 0, 0], [0, 0, 0.01])], [-1e3 * np.eye(6)])
    report = h.optimize(max_iterations=3)
    assert [r["cg_status"] for r in report["records"]] == ["cholesky"] * 3 and report["accepted"] == 0 and np.array_equal(h.poses(), X)


# ---- the Python wrappers ------------------------------------------------------------------------------------------------------------------------

def test_python_wrappers_refuse_bad_arguments_before_the_library():
    g = d.PoseGraph.__new__(d.PoseGraph)
    g.ctx, g.ptr, g.n, g.m, g.delta, g._edges = object(), None, 0, 0, np.zeros(0), None   # (no library behind it: a call that got that far raises AttributeError)
    eye = np.stack([np.eye(4)] * 3)
    bad = eye.copy()
    bad[1, 0, 3] = np.nan
    for call in (lambda: g.set_vertices(np.eye(4)), lambda: g.set_vertices(np.zeros((0, 4, 4))), lambda: g.set_vertices(np.zeros((3, 3, 4))),
                 lambda: g.set_vertices(bad), lambda: g.set_vertices(eye, [True, False]), lambda: g.set_poses(eye), lambda: g.poses(),
                 lambda: g.set_edges([0], [1], eye[:1], np.eye(6)[None]), lambda: g.optimize()):
        with pytest.raises(ValueError):
            call()
    g.n = 3
    W = np.stack([np.eye(6)] * 2)
    for call in (lambda: g.set_edges([0, 1], [1, 3], eye[:2], W), lambda: g.set_edges([0, -1], [1, 2], eye[:2], W), lambda: g.set_edges([0, 1], [1, 1], eye[:2], W),
                 lambda: g.set_edges([0, 1], [1], eye[:2], W), lambda: g.set_edges([0, 1], [1, 2], eye[:1], W), lambda: g.set_edges([0, 1], [1, 2], eye[:2], W[:1]),
                 lambda: g.set_edges([0, 1], [1, 2], bad[:2], W), lambda: g.set_edges([0, 1], [1, 2], eye[:2], np.full((2, 6, 6), np.inf)),
                 lambda: g.set_edges([0, 1], [1, 2], eye[:2], W, -1.0), lambda: g.set_edges([0, 1], [1, 2], eye[:2], W, [1.0]),
                 lambda: g.set_edges([0, 1], [1, 2], eye[:2], W, [1.0, np.nan]), lambda: g.set_edges([[0, 1]], [[1, 2]], eye[:2], W),
                 lambda: g.set_poses(eye[:2]), lambda: g.set_poses(bad),
                 lambda: g.optimize(max_iterations=-1), lambda: g.optimize(cg_max_iterations=0), lambda: g.optimize(cg_tolerance=0.0),
                 lambda: g.optimize(cg_tolerance=1.0), lambda: g.optimize(min_relative_decrease=-1e-3), lambda: g.optimize(initial_damping_scale=0.0),
                 lambda: g.optimize(cg_tolerance=float("nan")), lambda: g.remove_outliers(float("nan"))):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: g.set_edges([0.0, 1.0], [1, 2], eye[:2], W), lambda: g.set_edges([True, False], [1, 2], eye[:2], W),
                 lambda: g.set_vertices([["a"] * 4] * 4), lambda: g.optimize(iterations=3), lambda: g.optimize(max_iterations=2.0),
                 lambda: g.optimize(cg_max_iterations=True), lambda: g.remove_outliers(0.1, n_max=1.5)):
        with pytest.raises(TypeError):
            call()
    p = d.graph_params_struct(max_iterations=7, cg_tolerance=1e-4)
    assert (p.max_iterations, p.cg_max_iterations, p.cg_tolerance, p.min_relative_decrease, p.initial_damping_scale) == (7, 200, 1e-4, 1e-9, 1e-5)
    assert tracker.GRAPH_DEFAULTS == DEFAULTS
    assert C.sizeof(d._lib.GraphParams) == 56 and C.sizeof(d._lib.GraphIteration) == 40 and C.sizeof(d._lib.GraphReport) == 72
    for name in ("dvo_hip_graph_create", "dvo_hip_graph_destroy", "dvo_hip_graph_set_vertices", "dvo_hip_graph_set_poses", "dvo_hip_graph_set_edges",
                 "dvo_hip_graph_params_default", "dvo_hip_graph_optimize", "dvo_hip_graph_get_poses", "dvo_hip_graph_edge_stats",
                 "dvo_hip_graph_linearise", "dvo_hip_graph_multiply"):
        assert name in d._lib.EXPORTS


def test_the_library_exports_the_graph_entry_points_and_its_defaults():
    d.build()
    L = C.CDLL(d.LIB_PATH)
    L.dvo_hip_graph_params_default.restype = d._lib.GraphParams
    p = L.dvo_hip_graph_params_default()
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    for name in d._lib.EXPORTS:
        assert hasattr(L, name), name


# ---- the C++ facade -----------------------------------------------------------------------------------------------------------------------------

def build_pose_graph_facade_check():
    out = os.path.join(tempfile.mkdtemp(prefix="pose_graph_facade_"), "pose_graph_facade_check")
    src = os.path.join(ROOT, "tests", "cpp", "pose_graph_facade_check.cpp")
    libdir = os.path.join(ROOT, "dvo_slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
                           "-L" + libdir, "-ldvo_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return out


def test_cpp_facade_maps_ids_and_loads_a_local_map():
    d.build()
    exe = build_pose_graph_facade_check()
    out = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
