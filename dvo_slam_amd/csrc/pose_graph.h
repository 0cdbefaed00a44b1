// pose_graph.h -- the arithmetic of the SE(3) pose-graph optimiser, stated once for the device (pose_graph.hip) and for a plain host
// compiler (tests/test_pose_graph.py builds it with g++ -Wall -Werror -ffp-contract=off as the yardstick).  DESIGN.md section 12.
//
// Problem: the reference back end's (dvo_slam/src/keyframe_graph.cpp:256-285, 624-628; dvo_slam/src/local_map.cpp:79-88): vertices
// are poses X (camera -> world, row-major 4 x 4 doubles), edge k = (from i, to j, measurement Z, information Omega, kernel width delta):
//   error   e = MQT(Z^-1 X_i^-1 X_j): translation, then the vector part of the rotation's unit quaternion with w >= 0
//   s = e^T Omega e;  Cauchy kernel (delta > 0): rho = delta^2 log1p(s / delta^2), weight w = 1 / (1 + s / delta^2);  else rho = s, w = 1
//   update  X <- X M(d): translation d[0:3], rotation of the quaternion (sqrt(1 - |v|^2), v), v = d[3:6]; |v|^2 > 1: v normalised, w = 0
//   H = sum w J^T Omega J, b = -sum w J^T Omega e (iteratively re-weighted least squares), J analytic with respect to that update.
// Omega's rows and columns are translation first, then rotation, and it is taken AS GIVEN: the reference hands Result.Information, which
// is in twist order, straight to setInformation (keyframe_graph.cpp:628), and so does a caller of this code.
// Only + - * / sqrt appear (pg_log1p, the kernel's logarithm in the reported cost, is built from them too): with contraction off
// and correctly rounded divide and square root, host and device compute the same bits.
//
// Order of every sum: a vertex takes its incident edges in ascending edge index (the incidence lists); a scalar over vertices or edges
// is the adjacent-pair binary tree over the index, padded with zeros to a power of two, plus 0.0 (pg_tree_sum).  The result is a
// function of the vertices and of the edges IN THE ORDER GIVEN; it is not independent of that order.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "hd_compat.h"

namespace dvo_hip {

constexpr int kPgBlock = 256;              // vertices or edges per workgroup: the leaves of one subtree of a scalar's tree
constexpr int kPgTreeLevels = 26;
constexpr int kPgMaxVertices = 1 << 20;    // 4096 partials per vertex scalar
constexpr int kPgMaxEdges = 1 << 22;       // 16384 partials of the cost
// a resident-sized graph: within both.  k_pg_resident (pose_graph.hip) optimises such a graph start to end in one workgroup, and
// keeps the at most 4 / 16 partials of a scalar in LDS
constexpr int kPgResidentMaxVertices = 1024;
constexpr int kPgResidentMaxEdges = 4096;
// ... and it STAGES a graph whose solve fits this much LDS (of the 160 KB of a compute unit): the vertex records, the edges' off-diagonal
// blocks and the index arrays, pg_resident_stage_bytes of them.  A larger resident-sized graph is solved from memory.
constexpr int kPgResidentStageBytes = 144 * 1024;

// the per-edge record, component-major: component c of edge k at E[c * m + k] (a wavefront's stores coalesce)
enum { kPgE = 0, kPgS = 6, kPgW = 7, kPgRho = 8, kPgAii = 9, kPgAij = 45, kPgAjj = 81, kPgGi = 117, kPgGj = 123, kPgEdgeComps = 129 };
// the per-vertex record, component-major: diagonal block D, right-hand side b, (D + lambda I)^-1, the CG's vectors
enum { kPgD = 0, kPgB = 36, kPgMinv = 42, kPgX = 78, kPgR = 84, kPgZ = 90, kPgY = 96, kPgP0 = 102, kPgP1 = 108, kPgVertexComps = 114 };

// the status of a CG solve and of an optimisation (dvo_hip.h: DVO_HIP_GRAPH_CG_*, DVO_HIP_GRAPH_*)
enum { kPgCgRunning = 0, kPgCgConverged = 1, kPgCgBreakdown = 2, kPgCgCholesky = 3, kPgCgZeroRhs = 4, kPgCgIterationCap = 5 };
enum { kPgConverged = 0, kPgIterationCap = 1, kPgDampingOverflow = 2, kPgStalled = 3, kPgNothingToDo = 4 };

struct PgGraph {
  int n, m;
  const unsigned char* fixed;      // n
  const int* from;                 // m
  const int* to;                   // m
  const double* Z;                 // m x 16
  const double* omega;             // m x 36
  const double* delta;             // m
  const int* inc_start;            // n + 1: the incidence list of vertex v is inc[inc_start[v] .. inc_start[v + 1])
  const int* inc;                  // 2 m entries, edge * 2 + side (0: v is the edge's `from`, 1: its `to`), ascending per vertex
  double* E;                       // kPgEdgeComps x m
  double* V;                       // kPgVertexComps x n
};

DVO_HD bool pg_finite(double x) { return x - x == 0.0; }

// at the head of a function the HOST side of the library runs too (the Levenberg-Marquardt schedule): capi.hip is not built with
// contraction off, the yardstick is
#if defined(__clang__)
#define DVO_PG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DVO_PG_NO_CONTRACT
#endif

DVO_HD size_t pg_pad_pow2(size_t count) {
  size_t p = 1;
  while (p < count) p *= 2;
  return p;
}

// the adjacent-pair tree over a[0 .. count), padded with zeros to `padded` (a power of two >= count) -- without the final + 0.0
DVO_HD double pg_tree_raw(const double* a, size_t count, size_t padded) {
  double st[kPgTreeLevels];
  int top = 0;
  for (size_t i = 0; i < padded; ++i) {
    double v = i < count ? a[i] : 0.0;
    int lvl = 0;
    for (size_t k = i; k & 1; k >>= 1, ++lvl) v = st[lvl] + v;
    st[lvl] = v;
    top = lvl;
  }
  return st[top];
}
DVO_HD double pg_tree_sum(const double* a, size_t count) { return pg_tree_raw(a, count, pg_pad_pow2(count)) + 0.0; }

// log(1 + x) from + - * / alone: 1 + x = m 2^k with m in [sqrt 1/2, sqrt 2], log m = 2 atanh((m - 1) / (m + 1)) as a series to
// z^23 (|z| <= 0.1716: truncation 2e-20 relative), plus the correction (x - ((1 + x) - 1)) / (1 + x) for the bits 1 + x rounded away
DVO_HD double pg_log1p(double x) {
  const double u = 1.0 + x;
  if (!pg_finite(u)) return u;
  if (!(u > 0.0)) return (u - u) / (u - u);
  const double c = (x - (u - 1.0)) / u;
  double m = u, k = 0.0;
  for (int i = 0; i < 1100 && m > 1.4142135623730951; ++i) { m *= 0.5; k += 1.0; }
  for (int i = 0; i < 1100 && m < 0.70710678118654752; ++i) { m *= 2.0; k -= 1.0; }
  const double z = (m - 1.0) / (m + 1.0), z2 = z * z;
  double sum = 1.0 / 23.0;
  for (int n = 21; n >= 1; n -= 2) sum = sum * z2 + 1.0 / double(n);
  return k * 0.69314718055994531 + (2.0 * z * sum + c);
}

// ---- poses ---------------------------------------------------------------------------------------------------------------------------

struct PgPose { double R[9], t[3]; };

DVO_HD void pg_load(const double* X, PgPose& P) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P.R[r * 3 + c] = X[r * 4 + c];
    P.t[r] = X[r * 4 + 3];
  }
}

// a^T b of two 3 x 3 matrices, a^T v
DVO_HD void pg_mul_tn(const double* a, const double* b, double* out) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) out[r * 3 + c] = (a[0 + r] * b[0 + c] + a[3 + r] * b[3 + c]) + a[6 + r] * b[6 + c];
}
DVO_HD void pg_mul_tv(const double* a, const double* v, double* out) {
  for (int r = 0; r < 3; ++r) out[r] = (a[0 + r] * v[0] + a[3 + r] * v[1]) + a[6 + r] * v[2];
}

// the unit quaternion (w, x, y, z), w >= 0, of a rotation matrix: the branch on the trace and the largest diagonal entry, then the norm
DVO_HD void pg_quat(const double* R, double* q) {
  const double tr = (R[0] + R[4]) + R[8];
  if (tr > 0.0) {
    double t = sqrt(tr + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (R[7] - R[5]) * t;
    q[2] = (R[2] - R[6]) * t;
    q[3] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = sqrt(((R[i * 4] - R[j * 4]) - R[k * 4]) + 1.0);
    q[1 + i] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[1 + j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[1 + k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const double s = (q[0] < 0.0 ? -1.0 : 1.0) / (n > 0.0 ? n : 1.0);
  for (int c = 0; c < 4; ++c) q[c] *= s;
}

DVO_HD void pg_quat_matrix(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// X_out = X M(d).  The rotation goes through the quaternion and its norm, so poses stay rigid over many steps; d == 0 (a fixed or
// isolated vertex) or a non-finite d leaves X as it is, bit for bit.
DVO_HD void pg_update(const double* X, const double* d, double* X_out) {
  bool zero = true, finite = true;
  for (int c = 0; c < 6; ++c) {
    zero = zero && d[c] == 0.0;
    finite = finite && pg_finite(d[c]);
  }
  if (zero || !finite) {
    for (int c = 0; c < 16; ++c) X_out[c] = X[c];
    return;
  }
  PgPose P;
  pg_load(X, P);
  double v[3] = {d[3], d[4], d[5]}, w;
  const double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  if (n2 > 1.0) {
    const double inv = 1.0 / sqrt(n2);
    for (int c = 0; c < 3; ++c) v[c] *= inv;
    w = 0.0;
  } else {
    w = sqrt(1.0 - n2);
  }
  double a[4], q[4], R[9];
  pg_quat(P.R, a);
  q[0] = ((a[0] * w - a[1] * v[0]) - a[2] * v[1]) - a[3] * v[2];
  q[1] = ((a[0] * v[0] + a[1] * w) + a[2] * v[2]) - a[3] * v[1];
  q[2] = ((a[0] * v[1] - a[1] * v[2]) + a[2] * w) + a[3] * v[0];
  q[3] = ((a[0] * v[2] + a[1] * v[1]) - a[2] * v[0]) + a[3] * w;
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const double s = 1.0 / (n > 0.0 ? n : 1.0);
  for (int c = 0; c < 4; ++c) q[c] *= s;
  pg_quat_matrix(q, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) X_out[r * 4 + c] = R[r * 3 + c];
    X_out[r * 4 + 3] = ((P.R[r * 3] * d[0] + P.R[r * 3 + 1] * d[1]) + P.R[r * 3 + 2] * d[2]) + P.t[r];
  }
  X_out[12] = X_out[13] = X_out[14] = 0.0;
  X_out[15] = 1.0;
}

// ---- an edge -------------------------------------------------------------------------------------------------------------------------

// e and the Jacobians of e with respect to the updates of X_i and X_j (row-major 6 x 6).  With D = Z^-1 X_i^-1 X_j = (Rd, td),
// A = X_i^-1 X_j = (Ra, ta), the unit quaternion (w, u) of Rd and Q = w I + [u]x:
//   Jj = [Rd 0; 0 Q],  Ji = [-Rz^T  2 Rz^T [ta]x; 0  -Q Ra^T]
DVO_HD void pg_error(const double* Xi, const double* Xj, const double* Z, double* e, double* Ji, double* Jj) {
  PgPose Pi, Pj, Pz;
  pg_load(Xi, Pi);
  pg_load(Xj, Pj);
  pg_load(Z, Pz);
  double Ra[9], Rd[9], dt[3], ta[3], u[3], q[4];
  pg_mul_tn(Pi.R, Pj.R, Ra);
  for (int c = 0; c < 3; ++c) dt[c] = Pj.t[c] - Pi.t[c];
  pg_mul_tv(Pi.R, dt, ta);
  pg_mul_tn(Pz.R, Ra, Rd);
  for (int c = 0; c < 3; ++c) u[c] = ta[c] - Pz.t[c];
  pg_mul_tv(Pz.R, u, e);
  pg_quat(Rd, q);
  e[3] = q[1]; e[4] = q[2]; e[5] = q[3];
  if (!Ji) return;
  for (int c = 0; c < 36; ++c) Ji[c] = Jj[c] = 0.0;
  const double Q[9] = {q[0], -q[3], q[2], q[3], q[0], -q[1], -q[2], q[1], q[0]};
  const double S[9] = {0.0, -ta[2], ta[1], ta[2], 0.0, -ta[0], -ta[1], ta[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      Jj[r * 6 + c] = Rd[r * 3 + c];
      Jj[(r + 3) * 6 + c + 3] = Q[r * 3 + c];
      Ji[r * 6 + c] = -Pz.R[c * 3 + r];
      Ji[r * 6 + c + 3] = 2.0 * ((Pz.R[0 + r] * S[0 + c] + Pz.R[3 + r] * S[3 + c]) + Pz.R[6 + r] * S[6 + c]);
      Ji[(r + 3) * 6 + c + 3] = -((Q[r * 3] * Ra[c * 3] + Q[r * 3 + 1] * Ra[c * 3 + 1]) + Q[r * 3 + 2] * Ra[c * 3 + 2]);
    }
}

DVO_HD double pg_chi2(const double* e, const double* omega) {
  double s = 0.0;
  for (int r = 0; r < 6; ++r) {
    double a = 0.0;
    for (int c = 0; c < 6; ++c) a += omega[r * 6 + c] * e[c];
    s += e[r] * a;
  }
  return s;
}

// g2o's Cauchy kernel: rho[0] and rho[1], the weight removeOutlierConstraints thresholds (keyframe_graph.cpp:643-674)
DVO_HD void pg_robust(double s, double delta, double* rho, double* w) {
  if (delta > 0.0) {
    const double d2 = delta * delta, q = s / d2;
    *rho = d2 * pg_log1p(q);
    *w = 1.0 / (1.0 + q);
  } else {
    *rho = s;
    *w = 1.0;
  }
}

// out = a^T b of row-major 6 x 6 matrices; symmetric: the upper triangle computed, the lower mirrored
DVO_HD void pg_mul6_tn(const double* a, const double* b, double* out, bool symmetric) {
  for (int r = 0; r < 6; ++r)
    for (int c = symmetric ? r : 0; c < 6; ++c) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += a[k * 6 + r] * b[k * 6 + c];
      out[r * 6 + c] = s;
      if (symmetric) out[c * 6 + r] = s;
    }
}

// Edge k at `poses` into the edge record: e, s, w, rho and -- with_blocks -- w Ji^T Omega Ji, w Ji^T Omega Jj, w Jj^T Omega Jj,
// -w Ji^T Omega e, -w Jj^T Omega e.  Returns rho.
DVO_HD double pg_linearise_edge(const PgGraph& g, const double* poses, int k, bool with_blocks) {
  const size_t m = size_t(g.m);
  double* E = g.E + k;
  const double* om = g.omega + size_t(k) * 36;
  double e[6], Ji[36], Jj[36], rho, w;
  pg_error(poses + size_t(g.from[k]) * 16, poses + size_t(g.to[k]) * 16, g.Z + size_t(k) * 16, e, with_blocks ? Ji : nullptr, Jj);
  const double s = pg_chi2(e, om);
  pg_robust(s, g.delta[k], &rho, &w);
  for (int c = 0; c < 6; ++c) E[(kPgE + c) * m] = e[c];
  E[kPgS * m] = s;
  E[kPgW * m] = w;
  E[kPgRho * m] = rho;
  if (!with_blocks) return rho;
  double W[36], Ti[36], Tj[36], We[6], B[36];
  for (int c = 0; c < 36; ++c) W[c] = w * om[c];
  for (int r = 0; r < 6; ++r) {
    double a = 0.0;
    for (int c = 0; c < 6; ++c) {
      double si = 0.0, sj = 0.0;
      for (int q = 0; q < 6; ++q) {
        si += W[r * 6 + q] * Ji[q * 6 + c];
        sj += W[r * 6 + q] * Jj[q * 6 + c];
      }
      Ti[r * 6 + c] = si;
      Tj[r * 6 + c] = sj;
      a += W[r * 6 + c] * e[c];
    }
    We[r] = a;
  }
  pg_mul6_tn(Ji, Ti, B, true);
  for (int c = 0; c < 36; ++c) E[(kPgAii + c) * m] = B[c];
  pg_mul6_tn(Ji, Tj, B, false);
  for (int c = 0; c < 36; ++c) E[(kPgAij + c) * m] = B[c];
  pg_mul6_tn(Jj, Tj, B, true);
  for (int c = 0; c < 36; ++c) E[(kPgAjj + c) * m] = B[c];
  for (int r = 0; r < 6; ++r) {
    double gi = 0.0, gj = 0.0;
    for (int q = 0; q < 6; ++q) {
      gi += Ji[q * 6 + r] * We[q];
      gj += Jj[q * 6 + r] * We[q];
    }
    E[(kPgGi + r) * m] = -gi;
    E[(kPgGj + r) * m] = -gj;
  }
  return rho;
}

// ---- a vertex ------------------------------------------------------------------------------------------------------------------------

// a vertex the solve moves: not fixed and with an edge
DVO_HD bool pg_vertex_free(const PgGraph& g, int v) { return !g.fixed[v] && g.inc_start[v + 1] > g.inc_start[v]; }

// D_v and b_v: the diagonal blocks and gradient parts of the incident edges, in incidence order.  Returns the largest diagonal entry
// of D_v (0 for a vertex that is not free, whose D and b are zero).
DVO_HD double pg_gather_vertex(const PgGraph& g, int v) {
  const size_t n = size_t(g.n), m = size_t(g.m);
  double* V = g.V + v;
  double acc[42];
  for (int c = 0; c < 42; ++c) acc[c] = 0.0;
  if (pg_vertex_free(g, v))
    for (int at = g.inc_start[v]; at < g.inc_start[v + 1]; ++at) {
      const int k = g.inc[at] >> 1, side = g.inc[at] & 1;
      const double* A = g.E + size_t(side ? kPgAjj : kPgAii) * m + k;
      const double* G = g.E + size_t(side ? kPgGj : kPgGi) * m + k;
      for (int c = 0; c < 36; ++c) acc[c] += A[c * m];
      for (int c = 0; c < 6; ++c) acc[36 + c] += G[c * m];
    }
  for (int c = 0; c < 42; ++c) V[(kPgD + c) * n] = acc[c];
  double top = 0.0;
  for (int c = 0; c < 6; ++c) top = acc[c * 7] > top ? acc[c * 7] : top;
  return top;
}

// The inverse of the symmetric positive definite 6 x 6 matrix A (its lower triangle is read) through its Cholesky factor; false and
// zeros when a pivot is not positive and finite.
DVO_HD bool pg_chol_inverse6(const double* A, double* inv) {
  double L[36];
  for (int c = 0; c < 36; ++c) { L[c] = 0.0; inv[c] = 0.0; }
  for (int j = 0; j < 6; ++j) {
    double d = A[j * 6 + j];
    for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
    if (!(d > 0.0) || !pg_finite(d)) return false;
    const double l = sqrt(d);
    L[j * 6 + j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double a = A[i * 6 + j];
      for (int k = 0; k < j; ++k) a -= L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = a / l;
    }
  }
  for (int col = 0; col < 6; ++col) {
    double y[6], x[6];
    for (int i = 0; i < 6; ++i) {
      double a = i == col ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) a -= L[i * 6 + k] * y[k];
      y[i] = a / L[i * 6 + i];
    }
    for (int i = 5; i >= 0; --i) {
      double a = y[i];
      for (int k = i + 1; k < 6; ++k) a -= L[k * 6 + i] * x[k];
      x[i] = a / L[i * 6 + i];
    }
    for (int i = 0; i < 6; ++i) inv[i * 6 + col] = x[i];
  }
  for (int c = 0; c < 36; ++c)
    if (!pg_finite(inv[c])) {
      for (int q = 0; q < 36; ++q) inv[q] = 0.0;
      return false;
    }
  return true;
}

// The start of a CG solve at vertex v: Minv = (D_v + lambda I)^-1 (zero for a vertex that is not free), x = 0, r = b, z = Minv r.
// Returns r^T z; *ok = false where the factorisation failed.
DVO_HD double pg_cg_init_vertex(const PgGraph& g, int v, double lambda, bool* ok) {
  const size_t n = size_t(g.n);
  double* V = g.V + v;
  double A[36], inv[36], r[6];
  *ok = true;
  if (pg_vertex_free(g, v)) {
    for (int c = 0; c < 36; ++c) A[c] = V[(kPgD + c) * n];
    for (int c = 0; c < 6; ++c) A[c * 7] += lambda;
    *ok = pg_chol_inverse6(A, inv);
  } else {
    for (int c = 0; c < 36; ++c) inv[c] = 0.0;
  }
  double rz = 0.0;
  for (int c = 0; c < 36; ++c) V[(kPgMinv + c) * n] = inv[c];
  for (int c = 0; c < 6; ++c) r[c] = V[(kPgB + c) * n];
  for (int c = 0; c < 6; ++c) {
    double z = 0.0;
    for (int q = 0; q < 6; ++q) z += inv[c * 6 + q] * r[q];
    V[(kPgX + c) * n] = 0.0;
    V[(kPgR + c) * n] = r[c];
    V[(kPgZ + c) * n] = z;
    rz += r[c] * z;
  }
  return rz;
}

// how a multiply finds its direction p: the first of a solve (p = z), a later one (p = z + beta p_old), or given (a test hook)
enum { kPgDirFirst = 0, kPgDirNext = 1, kPgDirGiven = 2 };

DVO_HD double pg_direction(const PgGraph& g, int v, int c, int mode, double beta, int p_old, int p_new) {
  const size_t n = size_t(g.n);
  const double* V = g.V + v;
  if (mode == kPgDirGiven) return V[(p_new + c) * n];
  const double z = V[(kPgZ + c) * n];
  return mode == kPgDirFirst ? z : z + beta * V[(p_old + c) * n];
}

// y_v = (D_v + lambda I) p_v + sum over the incidence list of B_k p_j (v is the edge's `from`) or B_k^T p_i (its `to`); zero for a
// vertex that is not free.  p_v goes to the vertex record at p_new, p of the neighbours is formed from z and p_old, which this
// launch only reads.  Returns p_v^T y_v.
DVO_HD double pg_multiply_vertex(const PgGraph& g, int v, double lambda, int mode, double beta, int p_old, int p_new) {
  const size_t n = size_t(g.n), m = size_t(g.m);
  double* V = g.V + v;
  double p[6], y[6];
  for (int c = 0; c < 6; ++c) {
    p[c] = pg_direction(g, v, c, mode, beta, p_old, p_new);
    y[c] = 0.0;
  }
  if (pg_vertex_free(g, v)) {
    for (int r = 0; r < 6; ++r) {
      double a = lambda * p[r];
      for (int c = 0; c < 6; ++c) a += V[(kPgD + r * 6 + c) * n] * p[c];
      y[r] = a;
    }
    for (int at = g.inc_start[v]; at < g.inc_start[v + 1]; ++at) {
      const int k = g.inc[at] >> 1, side = g.inc[at] & 1;
      const int other = side ? g.from[k] : g.to[k];
      const double* B = g.E + size_t(kPgAij) * m + k;
      double q[6];
      for (int c = 0; c < 6; ++c) q[c] = pg_direction(g, other, c, mode, beta, p_old, p_new);
      for (int r = 0; r < 6; ++r) {
        double a = 0.0;
        for (int c = 0; c < 6; ++c) a += B[(side ? c * 6 + r : r * 6 + c) * m] * q[c];
        y[r] += a;
      }
    }
  }
  double py = 0.0;
  for (int c = 0; c < 6; ++c) {
    if (mode != kPgDirGiven) V[(p_new + c) * n] = p[c];
    V[(kPgY + c) * n] = y[c];
    py += p[c] * y[c];
  }
  return py;
}

// x += alpha p, r -= alpha y, z = Minv r at vertex v.  Returns r^T z.
DVO_HD double pg_cg_update_vertex(const PgGraph& g, int v, double alpha, int p_at) {
  const size_t n = size_t(g.n);
  double* V = g.V + v;
  double r[6];
  for (int c = 0; c < 6; ++c) {
    V[(kPgX + c) * n] += alpha * V[(p_at + c) * n];
    r[c] = V[(kPgR + c) * n] - alpha * V[(kPgY + c) * n];
    V[(kPgR + c) * n] = r[c];
  }
  double rz = 0.0;
  for (int c = 0; c < 6; ++c) {
    double z = 0.0;
    for (int q = 0; q < 6; ++q) z += V[(kPgMinv + c * 6 + q) * n] * r[q];
    V[(kPgZ + c) * n] = z;
    rz += r[c] * z;
  }
  return rz;
}

// The step x_v applied to vertex v of `poses` into `out`.  Returns x_v^T (lambda x_v + b_v), the vertex's part of the gain's scale.
DVO_HD double pg_apply_vertex(const PgGraph& g, int v, double lambda, const double* poses, double* out) {
  const size_t n = size_t(g.n);
  const double* V = g.V + v;
  double d[6], scale = 0.0;
  for (int c = 0; c < 6; ++c) {
    d[c] = V[(kPgX + c) * n];
    scale += d[c] * (lambda * d[c] + V[(kPgB + c) * n]);
  }
  pg_update(poses + size_t(v) * 16, d, out + size_t(v) * 16);
  return scale;
}

// ---- the scalars of the CG ------------------------------------------------------------------------------------------------------------

// the state of a CG solve, on the device one record that workgroup 0 of each launch writes and the NEXT launch reads
struct PgCgState {
  double rz0;          // r^T z at the start: ||b||^2 in the M^-1 norm
  double rz[2];        // r^T z before multiply `it`, at it & 1
  int stop_multiply;   // kPgCg* as the vector kernel left it: a multiply that reads it != 0 returns at once
  int stop_vector;     // ... as the multiply left it, for the vector kernel of the same iteration
  int iterations;      // multiplies done
  int cholesky_failed; // a vertex's D + lambda I had no Cholesky factor
};

// what multiply `it` decides from rz = r^T z: go on (kPgCgRunning, *beta set) or stop with a status
DVO_HD int pg_cg_before_multiply(const PgCgState& s, int it, double rz, double tolerance, double* beta) {
  *beta = 0.0;
  if (s.cholesky_failed) return kPgCgCholesky;
  if (!pg_finite(rz) || rz < 0.0) return kPgCgBreakdown;
  if (it == 0) return rz > 0.0 ? kPgCgRunning : kPgCgZeroRhs;
  if (rz <= (tolerance * tolerance) * s.rz0) return kPgCgConverged;
  *beta = rz / s.rz[(it - 1) & 1];
  return pg_finite(*beta) ? kPgCgRunning : kPgCgBreakdown;
}

// ... and the vector kernel from p^T A p: the step length, or breakdown
DVO_HD int pg_cg_step_length(double rz, double pAp, double* alpha) {
  *alpha = 0.0;
  if (!(pAp > 0.0) || !pg_finite(pAp)) return kPgCgBreakdown;
  *alpha = rz / pAp;
  return pg_finite(*alpha) ? kPgCgRunning : kPgCgBreakdown;
}

// ---- the Levenberg-Marquardt schedule (g2o's OptimizationAlgorithmLevenberg defaults: tau 1e-5, lower 1/3, upper 2/3, 10 trials) ------

struct PgLm {
  double lambda, ni, cost;
  int rejected_in_a_row;
};

DVO_HD void pg_lm_begin(PgLm& lm, double cost, double initial_damping_scale, double max_diagonal) {
  DVO_PG_NO_CONTRACT
  lm.lambda = initial_damping_scale * (max_diagonal > 0.0 ? max_diagonal : 1.0);
  lm.ni = 2.0;
  lm.cost = cost;
  lm.rejected_in_a_row = 0;
}

// One trial judged: cost_new at the stepped poses, scale = sum x (lambda x + b), the CG's status.  Returns whether the step is
// accepted; lm holds the damping of the next trial.  *stop: -1 to go on, else the optimisation's status.
DVO_HD bool pg_lm_judge(PgLm& lm, double cost_new, double scale, int cg_status, double min_relative_decrease, int* stop) {
  DVO_PG_NO_CONTRACT
  const bool solved = cg_status == kPgCgConverged || cg_status == kPgCgIterationCap;
  const double gain = (lm.cost - cost_new) / (scale + 1e-3);
  const bool accepted = solved && pg_finite(cost_new) && pg_finite(gain) && gain > 0.0;
  *stop = -1;
  if (accepted) {
    double alpha = 2.0 * gain - 1.0;
    alpha = 1.0 - alpha * alpha * alpha;
    alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
    lm.lambda *= alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0;
    lm.ni = 2.0;
    lm.rejected_in_a_row = 0;
    if (lm.cost - cost_new <= min_relative_decrease * lm.cost) *stop = kPgConverged;
    lm.cost = cost_new;
  } else {
    lm.lambda *= lm.ni;
    lm.ni *= 2.0;
    lm.rejected_in_a_row += 1;
    if (cg_status == kPgCgZeroRhs) *stop = kPgConverged;
    else if (lm.rejected_in_a_row >= 10) *stop = kPgStalled;
  }
  if (*stop < 0 && !pg_finite(lm.lambda)) *stop = kPgDampingOverflow;
  return accepted;
}

// ---- the resident schedule: one graph, one workgroup, one launch (k_pg_resident) -------------------------------------------------------

DVO_HD size_t pg_resident_stage_bytes(int n, int m) {
  const size_t bytes = 8 * (size_t(kPgVertexComps) * size_t(n) + 36 * size_t(m)) + 4 * (size_t(n) + 1 + 4 * size_t(m)) + size_t(n);
  return (bytes + 15) / 16 * 16;
}

// what a workgroup of k_pg_resident is handed: the graph where it lies, both pose buffers, which holds the estimate, the parameters
struct PgResidentJob {
  PgGraph g;
  double* poses[2];
  int cur;                    // poses[cur] is the estimate
  int any_free;               // a vertex that is neither fixed nor without an edge
  int max_iterations, cg_max_iterations;
  double cg_tolerance, min_relative_decrease, initial_damping_scale;
};

// ... and what it leaves: the report's numbers (dvo_hip_graph_report) and the pose buffer the final estimate is in
struct PgResidentOut {
  int status, iterations, accepted, cg_iterations;
  double initial_cost, final_cost, final_damping;
  int cur, reserved;
};

// one trial, laid out like dvo_hip_graph_iteration
struct PgResidentIteration {
  double cost_before, cost_after, damping;
  int cg_iterations, cg_status, accepted, reserved;
};

}  // namespace dvo_hip
