// fbr_pg.h — the pose-graph arithmetic of include/fbr.h ("pose graph"), host and device, all in
// double: Exp / Log / Jr^-1 of SO(3), the residual and Jacobians of a factor, the 6x6 Cholesky, one
// level step of the block cyclic reduction with its index arithmetic, the Euler conversion, the
// per-node steps of the marginal covariances (k_pg_marginals.hip; on the CPU fbr_pg_host.h), the
// robust loop factors' rho and weight, and the per-entry steps of the direct solve (k_pg_direct.hip).
// k_posegraph.hip compiles these functions for the device and tests/native/pg_probe.cpp for the CPU,
// so the tests check the kernels' arithmetic without a GPU.  The contract is the project's own
// restatement of a pose-graph optimiser in GTSAM 4.0's default Pose3 chart; it is pinned by the
// NumPy model tests/pg_model.py, not against GTSAM.
//
// Must be compiled with -ffp-contract=off, as everything here.
//
// Every loop over a small local array has constant bounds and is unrolled, so the arrays stay in
// registers on the device (a runtime-indexed local array would go to scratch); the loops that are
// not unrolled (the marginals' row passes and dense steps) index memory only.
#pragma once
#include <math.h>
#include <stdint.h>

// Free of HIP headers under a plain host compiler, so that a stand-alone CPU program (sanitizers)
// can include it.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PG_HD __host__ __device__ inline
#else
#define PG_HD inline
#endif

namespace fbr {

enum { kPgPrior = 0, kPgBetween = 1, kPgGps = 2 };

struct PgFactor {
  int32_t type;  // kPg*
  int32_t i, j;  // nodes (j = -1 for prior and gps)
  int32_t loop;  // 1: a between factor with |i - j| != 1, a term of L; 0: a term of T
  double Z[12];  // the measurement: R row-major [9], t [3] (gps: t only)
  double w[6];   // 1 / sqrt(variance), tangent order [rotation; translation] (gps: w[0..2] = 0)
};

constexpr int kPgLin = 78;  // doubles of a linearised factor: r[6], J_i[36], J_j[36] (whitened, row-major)

// ---- 3x3 helpers (row-major) ----
PG_HD void pg_mul33(const double* A, const double* B, double* C) {  // C = A B
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
PG_HD void pg_mul33_tn(const double* A, const double* B, double* C) {  // C = A^T B
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
PG_HD void pg_mulv3(const double* A, const double* v, double* o) {  // o = A v
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2];
}
PG_HD void pg_mulv3_t(const double* A, const double* v, double* o) {  // o = A^T v
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = (A[r] * v[0] + A[3 + r] * v[1]) + A[6 + r] * v[2];
}
// I a + K b + K^2 c with K = [w]x (K^2 = w w^T - |w|^2 I)
PG_HD void pg_rodrigues(const double* w, double a, double b, double c, double* R) {
  const double x = w[0], y = w[1], z = w[2], t2 = (x * x + y * y) + z * z;
  R[0] = a + c * (x * x - t2); R[1] = c * (x * y) - b * z;   R[2] = c * (x * z) + b * y;
  R[3] = c * (x * y) + b * z;   R[4] = a + c * (y * y - t2); R[5] = c * (y * z) - b * x;
  R[6] = c * (x * z) - b * y;   R[7] = c * (y * z) + b * x;   R[8] = a + c * (z * z - t2);
}

// Exp of so(3): I + (sin t / t) K + ((1 - cos t) / t^2) K^2, the series below t^2 = 1e-12.
PG_HD void pg_exp(const double* w, double* R) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double a, b;
  if (t2 < 1e-12) {
    a = 1.0 - t2 / 6.0;
    b = 0.5 - t2 / 24.0;
  } else {
    const double t = sqrt(t2);
    a = sin(t) / t;
    b = (1.0 - cos(t)) / t2;
  }
  pg_rodrigues(w, 1.0, a, b, R);
}

// Log of SO(3).  v = vee(R - R^T) = 2 sin t * axis, c = (trace - 1) / 2, t = atan2(|v| / 2, c).
//   t^2 < 1e-12:  w = v / 2 * (1 + t^2 / 6)
//   c > -0.99:    w = v / 2 * t / sin t
//   otherwise (t near pi, sin t small): the axis from the symmetric part, (R + R^T) / 2 = c I +
//     (1 - c) a a^T: the largest a_p^2 = (R_pp - c) / (1 - c) gives a_p, the others follow from row
//     p; its sign is v's (either at t = pi exactly).  No branch divides by a vanishing quantity.
PG_HD void pg_log(const double* R, double* w) {
  const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
  const double s = 0.5 * sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double t = atan2(s, c);
  if (t * t < 1e-12) {
    const double k = 0.5 * (1.0 + t * t / 6.0);
    w[0] = k * v[0]; w[1] = k * v[1]; w[2] = k * v[2];
  } else if (c > -0.99) {
    const double k = 0.5 * t / s;
    w[0] = k * v[0]; w[1] = k * v[1]; w[2] = k * v[2];
  } else {
    const double d0 = R[0], d1 = R[4], d2 = R[8], omc = 1.0 - c;
    double a[3];
    if (d0 >= d1 && d0 >= d2) {
      a[0] = sqrt((d0 - c) / omc);
      a[1] = (R[1] + R[3]) / (2.0 * omc * a[0]);
      a[2] = (R[2] + R[6]) / (2.0 * omc * a[0]);
    } else if (d1 >= d2) {
      a[1] = sqrt((d1 - c) / omc);
      a[0] = (R[1] + R[3]) / (2.0 * omc * a[1]);
      a[2] = (R[5] + R[7]) / (2.0 * omc * a[1]);
    } else {
      a[2] = sqrt((d2 - c) / omc);
      a[0] = (R[2] + R[6]) / (2.0 * omc * a[2]);
      a[1] = (R[5] + R[7]) / (2.0 * omc * a[2]);
    }
    const double n = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const double sg = ((a[0] * v[0] + a[1] * v[1]) + a[2] * v[2]) < 0.0 ? -1.0 : 1.0;
    const double k = sg * t / n;
    w[0] = k * a[0]; w[1] = k * a[1]; w[2] = k * a[2];
  }
}

// Jr^-1(phi) = I + K / 2 + (1 / t^2 - cot(t / 2) / (2 t)) K^2, which is the contract's
// 1 / t^2 - (1 + cos t) / (2 t sin t) without its 0 / 0 at t = pi; 1 / 12 + t^2 / 720 below t^2 = 1e-6.
PG_HD void pg_jrinv(const double* phi, double* J) {
  const double t2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
  double k;
  if (t2 < 1e-6) {
    k = 1.0 / 12.0 + t2 / 720.0;
  } else {
    const double t = sqrt(t2), h = 0.5 * t;
    k = 1.0 / t2 - (cos(h) / sin(h)) / (2.0 * t);
  }
  pg_rodrigues(phi, 1.0, 0.5, k, J);
}

// Pose [12] = R row-major [9], t [3], from [roll, pitch, yaw, x, y, z]: R = Rz(yaw) Ry(pitch) Rx(roll).
PG_HD void pg_pose_from_euler(const double* e, double* X) {
  const double cr = cos(e[0]), sr = sin(e[0]), cp = cos(e[1]), sp = sin(e[1]), cy = cos(e[2]), sy = sin(e[2]);
  X[0] = cy * cp; X[1] = cy * sp * sr - sy * cr; X[2] = cy * sp * cr + sy * sr;
  X[3] = sy * cp; X[4] = sy * sp * sr + cy * cr; X[5] = sy * sp * cr - cy * sr;
  X[6] = -sp;     X[7] = cp * sr;                X[8] = cp * cr;
  X[9] = e[3]; X[10] = e[4]; X[11] = e[5];
}
// roll = atan2(R21, R22), pitch = asin(-R20) clamped, yaw = atan2(R10, R00)
PG_HD void pg_euler_from_pose(const double* X, double* e) {
  double s = -X[6];
  s = s > 1.0 ? 1.0 : s < -1.0 ? -1.0 : s;
  e[0] = atan2(X[7], X[8]);
  e[1] = asin(s);
  e[2] = atan2(X[3], X[0]);
  e[3] = X[9]; e[4] = X[10]; e[5] = X[11];
}
// A^-1 B of two poses
PG_HD void pg_between(const double* A, const double* B, double* D) {
  pg_mul33_tn(A, B, D);
  const double dt[3] = {B[9] - A[9], B[10] - A[10], B[11] - A[11]};
  pg_mulv3_t(A, dt, D + 9);
}
// T (+) [w; v] = (R Exp(w), t + R v)
PG_HD void pg_retract(const double* X, const double* d, double* Y) {
  double E[9], rv[3];
  pg_exp(d, E);
  pg_mul33(X, E, Y);
  pg_mulv3(X, d + 3, rv);
  Y[9] = X[9] + rv[0]; Y[10] = X[10] + rv[1]; Y[11] = X[11] + rv[2];
}

// The whitened residual r[6] of a factor and, with jac, its whitened Jacobians Ji, Jj [36]
// (row-major, tangent order [rotation; translation]; Jj is zero for prior and gps).  Xj is not read
// for prior and gps.  Derivation: include/fbr.h "pose graph".
PG_HD void pg_factor_eval(const PgFactor& f, const double* Xi, const double* Xj, bool jac, double* r, double* Ji,
                          double* Jj) {
  if (jac) {
#pragma unroll
    for (int k = 0; k < 36; ++k) Ji[k] = Jj[k] = 0.0;
  }
  if (f.type == kPgGps) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = 0.0;
      r[3 + k] = (Xi[9 + k] - f.Z[9 + k]) * f.w[3 + k];
    }
    if (jac) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) Ji[6 * (3 + a) + 3 + b] = Xi[3 * a + b] * f.w[3 + a];
    }
    return;
  }
  const bool between = f.type == kPgBetween;
  double D[12];  // T_i^-1 T_j, or T_i for a prior
  if (between) {
    pg_between(Xi, Xj, D);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) D[k] = Xi[k];
  }
  double E[9], phi[3], et[3];
  pg_mul33_tn(f.Z, D, E);  // E_R = Z_R^T D_R
  pg_log(E, phi);
  const double dt[3] = {D[9] - f.Z[9], D[10] - f.Z[10], D[11] - f.Z[11]};
  pg_mulv3_t(f.Z, dt, et);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r[k] = phi[k] * f.w[k];
    r[3 + k] = et[k] * f.w[3 + k];
  }
  if (!jac) return;
  double Jr[9];
  pg_jrinv(phi, Jr);
  double* Jn = between ? Jj : Ji;  // the "j half": d e_rot / d w = Jr^-1, d e_t / d v = E_R
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Jn[6 * a + b] = Jr[3 * a + b] * f.w[a];
      Jn[6 * (3 + a) + 3 + b] = E[3 * a + b] * f.w[3 + a];
    }
  if (!between) return;
  // the "i half": d e_rot / d w = -Jr^-1 D_R^T, d e_t / d w = Z_R^T [D_t]x, d e_t / d v = -Z_R^T
  const double S[9] = {0.0, -D[11], D[10], D[11], 0.0, -D[9], -D[10], D[9], 0.0};
  double ZS[9];
  pg_mul33_tn(f.Z, S, ZS);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double jd = (Jr[3 * a] * D[3 * b] + Jr[3 * a + 1] * D[3 * b + 1]) + Jr[3 * a + 2] * D[3 * b + 2];
      Ji[6 * a + b] = -jd * f.w[a];
      Ji[6 * (3 + a) + b] = ZS[3 * a + b] * f.w[3 + a];
      Ji[6 * (3 + a) + 3 + b] = -f.Z[3 * b + a] * f.w[3 + a];
    }
}

// ---- 6x6 Cholesky (row-major, lower): A = L L^T from A's lower triangle ----
// Returns false on a non-positive or non-finite pivot (the factor is then completed with that
// pivot taken as 1, so that nothing downstream divides by zero).
PG_HD bool pg_chol6(const double* A, double* L) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[6 * j + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = d - L[6 * j + k] * L[6 * j + k];
    if (!(d > 0.0) || !(d < INFINITY)) {
      ok = false;
      d = 1.0;
    }
    const double l = sqrt(d);
    L[6 * j + j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = s / l;
    }
#pragma unroll
    for (int i = 0; i < j; ++i) L[6 * i + j] = 0.0;
  }
  return ok;
}
// x = (L L^T)^-1 b, in place
PG_HD void pg_chol6_solve(const double* L, double* x) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = x[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[6 * i + k] * x[k];
    x[i] = s / L[6 * i + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s = s - L[6 * k + i] * x[k];
    x[i] = s / L[6 * i + i];
  }
}

// ---- block cyclic reduction of a symmetric positive definite block-tridiagonal system ----
// A level holds n nodes: node m's diagonal block D[m] and its coupling A[m] = T[m][m-1] to the node
// before it (A[0] unused), its right-hand side b[m] and solution x[m].  Arrays are
// structure-of-arrays: entry e of node m is X[e * n + m] (consecutive threads, consecutive
// addresses).  The odd nodes of a level are eliminated; the even node m = 2q becomes node q of the
// next level, which has (n + 1) / 2 nodes; the last level has one node.
//
// Factor, per level:
//   pg_cr_elim(k), k odd (or the single node of the last level): L[k] = chol(D[k]),
//     G[k] = D[k]^-1 A[k], H[k] = D[k]^-1 A[k+1]^T (zero when k + 1 == n)
//   pg_cr_update(q): next.D[q] = D[m] - A[m] H[m-1] - A[m+1]^T G[m+1],
//                    next.A[q] = -A[m] G[m-1]            (terms of absent neighbours dropped)
// Solve, per level down, then the last level's node, then per level up:
//   pg_cr_reduce(q):  next.b[q] = b[m] - H[m-1]^T b[m-1] - G[m+1]^T b[m+1]
//   pg_cr_top():      x[0] = D[0]^-1 b[0]
//   pg_cr_backsub(m): x[m] = next.x[m / 2] (m even);
//                     x[m] = D[m]^-1 b[m] - G[m] x[m-1] - H[m] x[m+1] (m odd, x[m+-1] from next.x)
// Each step reads only what earlier steps wrote: a level step is one kernel (or one loop on the CPU).
struct PgLevel {
  int64_t n;
  double *D, *A, *L, *G, *H;  // [36][n]
  double *b, *x;              // [6][n]
};

PG_HD void pg_ld36(const double* X, int64_t n, int64_t m, double* M) {
#pragma unroll
  for (int e = 0; e < 36; ++e) M[e] = X[e * n + m];
}
PG_HD void pg_st36(double* X, int64_t n, int64_t m, const double* M) {
#pragma unroll
  for (int e = 0; e < 36; ++e) X[e * n + m] = M[e];
}
PG_HD void pg_ld6(const double* X, int64_t n, int64_t m, double* v) {
#pragma unroll
  for (int e = 0; e < 6; ++e) v[e] = X[e * n + m];
}
PG_HD void pg_st6(double* X, int64_t n, int64_t m, const double* v) {
#pragma unroll
  for (int e = 0; e < 6; ++e) X[e * n + m] = v[e];
}

PG_HD bool pg_cr_is_elim(int64_t n, int64_t k) { return (k & 1) || n == 1; }

// false: a bad pivot
PG_HD bool pg_cr_elim(const PgLevel& lv, int64_t k) {
  const int64_t n = lv.n;
  double M[36], L[36];
  pg_ld36(lv.D, n, k, M);
  const bool ok = pg_chol6(M, L);
  pg_st36(lv.L, n, k, L);
  // column by column: G[:, c] = D^-1 A[k][:, c], H[:, c] = D^-1 A[k+1][c, :]^T
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double g[6], h[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      g[r] = k >= 1 ? lv.A[(6 * r + c) * n + k] : 0.0;
      h[r] = k + 1 < n ? lv.A[(6 * c + r) * n + k + 1] : 0.0;
    }
    pg_chol6_solve(L, g);
    pg_chol6_solve(L, h);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      lv.G[(6 * r + c) * n + k] = g[r];
      lv.H[(6 * r + c) * n + k] = h[r];
    }
  }
  return ok;
}

PG_HD void pg_cr_update(const PgLevel& lv, const PgLevel& nx, int64_t q) {
  const int64_t n = lv.n, m = 2 * q;
  double Dn[36], An[36];
  pg_ld36(lv.D, n, m, Dn);
#pragma unroll
  for (int e = 0; e < 36; ++e) An[e] = 0.0;
  if (m >= 1) {
    double Am[36], X[36];
    pg_ld36(lv.A, n, m, Am);
    pg_ld36(lv.H, n, m - 1, X);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s = s + Am[6 * r + k] * X[6 * k + c];
        Dn[6 * r + c] = Dn[6 * r + c] - s;
      }
    pg_ld36(lv.G, n, m - 1, X);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s = s + Am[6 * r + k] * X[6 * k + c];
        An[6 * r + c] = -s;
      }
  }
  if (m + 1 < n) {
    double Ap[36], X[36];
    pg_ld36(lv.A, n, m + 1, Ap);
    pg_ld36(lv.G, n, m + 1, X);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s = s + Ap[6 * k + r] * X[6 * k + c];
        Dn[6 * r + c] = Dn[6 * r + c] - s;
      }
  }
  pg_st36(nx.D, nx.n, q, Dn);
  pg_st36(nx.A, nx.n, q, An);
}

PG_HD void pg_cr_reduce(const PgLevel& lv, const PgLevel& nx, int64_t q) {
  const int64_t n = lv.n, m = 2 * q;
  double b[6], v[6];
  pg_ld6(lv.b, n, m, b);
  if (m >= 1) {
    pg_ld6(lv.b, n, m - 1, v);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s + lv.H[(6 * k + c) * n + m - 1] * v[k];
      b[c] = b[c] - s;
    }
  }
  if (m + 1 < n) {
    pg_ld6(lv.b, n, m + 1, v);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s + lv.G[(6 * k + c) * n + m + 1] * v[k];
      b[c] = b[c] - s;
    }
  }
  pg_st6(nx.b, nx.n, q, b);
}

PG_HD void pg_cr_top(const PgLevel& lv) {
  double L[36], x[6];
  pg_ld36(lv.L, lv.n, 0, L);
  pg_ld6(lv.b, lv.n, 0, x);
  pg_chol6_solve(L, x);
  pg_st6(lv.x, lv.n, 0, x);
}

PG_HD void pg_cr_backsub(const PgLevel& lv, const PgLevel& nx, int64_t m) {
  const int64_t n = lv.n;
  double x[6];
  if (!(m & 1)) {
    pg_ld6(nx.x, nx.n, m >> 1, x);
    pg_st6(lv.x, n, m, x);
    return;
  }
  double L[36], v[6];
  pg_ld36(lv.L, n, m, L);
  pg_ld6(lv.b, n, m, x);
  pg_chol6_solve(L, x);
  pg_ld6(nx.x, nx.n, (m - 1) >> 1, v);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s = s + lv.G[(6 * r + k) * n + m] * v[k];
    x[r] = x[r] - s;
  }
  if (m + 1 < n) {
    pg_ld6(nx.x, nx.n, (m + 1) >> 1, v);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s + lv.H[(6 * r + k) * n + m] * v[k];
      x[r] = x[r] - s;
    }
  }
  pg_st6(lv.x, n, m, x);
}

// Levels of an n-node system and their total node count (the arrays' extent in nodes).
PG_HD int pg_cr_levels(int64_t n, int64_t* total) {
  int levels = 1;
  int64_t t = n;
  while (n > 1) {
    n = (n + 1) / 2;
    t += n;
    ++levels;
  }
  if (total) *total = t;
  return levels;
}

// ---- per-node assembly and products (gathers in adjacency order; no atomics) ----
// adjacency entry = factor * 2 + side (side 0: the node is the factor's i, 1: its j)

// Node m's rows of the undamped T (diagonal block D0, coupling A = T[m][m-1]), of g = J^T r and of
// diag(H) (hd, the loop factors included), from the linearised factors in adjacency order.
PG_HD void pg_assemble_node(int64_t n, int64_t m, const PgFactor* fac, const double* lin, const int32_t* adj_off,
                            const int32_t* adj, double* D0, double* A, double* g, double* hd) {
  double D[36], C[36], gv[6], hv[6];
#pragma unroll
  for (int e = 0; e < 36; ++e) D[e] = C[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) gv[e] = hv[e] = 0.0;
  for (int32_t a = adj_off[m]; a < adj_off[m + 1]; ++a) {
    const int32_t k = adj[a] >> 1, side = adj[a] & 1;
    const double* r = lin + (int64_t)k * kPgLin;
    const double* Js = r + 6 + 36 * side;
    const double* Jo = r + 6 + 36 * (1 - side);
    const int32_t loop = fac[k].loop, other = side ? fac[k].i : fac[k].j;
    const bool band = !loop && fac[k].type == kPgBetween && (int64_t)other == m - 1;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0, d = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        s = s + Js[6 * q + c] * r[q];
        d = d + Js[6 * q + c] * Js[6 * q + c];
      }
      gv[c] = gv[c] + s;
      hv[c] = hv[c] + d;
    }
    if (!loop) {
#pragma unroll
      for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) s = s + Js[6 * q + rr] * Js[6 * q + c];
          D[6 * rr + c] = D[6 * rr + c] + s;
        }
    }
    if (band) {
#pragma unroll
      for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) s = s + Js[6 * q + rr] * Jo[6 * q + c];
          C[6 * rr + c] = C[6 * rr + c] + s;
        }
    }
  }
  pg_st36(D0, n, m, D);
  pg_st36(A, n, m, C);
  pg_st6(g, n, m, gv);
  pg_st6(hd, n, m, hv);
}

// Node m's rows of q = H p = T p + L p: the damped diagonal block D, the couplings A, and the loop
// factors of ladj (J_side^T (J_i p_i + J_j p_j), in adjacency order).  Returns p_m . q_m.
PG_HD double pg_hp_node(int64_t n, int64_t m, const PgFactor* fac, const double* lin, const int32_t* ladj_off,
                        const int32_t* ladj, const double* D, const double* A, const double* p, double* q) {
  double pm[6], v[6], o[6];
  pg_ld6(p, n, m, pm);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s = s + D[(6 * r + k) * n + m] * pm[k];
    o[r] = s;
  }
  if (m >= 1) {
    pg_ld6(p, n, m - 1, v);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s + A[(6 * r + k) * n + m] * v[k];
      o[r] = o[r] + s;
    }
  }
  if (m + 1 < n) {
    pg_ld6(p, n, m + 1, v);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s + A[(6 * k + r) * n + m + 1] * v[k];
      o[r] = o[r] + s;
    }
  }
  for (int32_t a = ladj_off[m]; a < ladj_off[m + 1]; ++a) {
    const int32_t k = ladj[a] >> 1, side = ladj[a] & 1;
    const double* Ji = lin + (int64_t)k * kPgLin + 6;
    const double* Jj = Ji + 36;
    double pi[6], pj[6], u[6];
    pg_ld6(p, n, fac[k].i, pi);
    pg_ld6(p, n, fac[k].j, pj);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s = s + Ji[6 * r + c] * pi[c];
#pragma unroll
      for (int c = 0; c < 6; ++c) s = s + Jj[6 * r + c] * pj[c];
      u[r] = s;
    }
    const double* Js = side ? Jj : Ji;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) s = s + Js[6 * r + c] * u[r];
      o[c] = o[c] + s;
    }
  }
  pg_st6(q, n, m, o);
  double d = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) d = d + pm[r] * o[r];
  return d;
}

// ---- marginal covariances (include/fbr.h "marginal covariances") ----
// Sigma = H^-1 with H = T0 + U^T U: T0 the undamped block-tridiagonal part, factored by the cyclic
// reduction above with lambda = 0, U [6K x 6N] the K loop factors' whitened Jacobians.
//   selected inversion of T0: per level and node P[m] = S[m][m], Q[m] = S[m][m-1] (S = that level's
//     inverse), walking up from the last level (pg_selinv_top, pg_selinv_up); level 0's P is P_i.
//   W = T0^-1 U^T: one cyclic-reduction solve per column (pg_cr_*_col; column c of a level's b and
//     x is the [6][n] vector at offset c * 6 * n, so W is [6K][6][N] and W_i^T is a strided view)
//   C = I + U W (pg_marg_c_entry), C = Lc Lc^T (pg_dense_chol_block, pg_dense_panel_row,
//     pg_dense_trail_entry), Y_i = Lc^-1 W_i^T in place (pg_marg_forward), and
//   Sigma_ii = P_i - Y_i^T Y_i (pg_marg_final).

// Row r of (L L^T)^-1 (= its column r)
PG_HD void pg_chol6_inv_row(const double* L, int r, double* x) {
#pragma unroll
  for (int e = 0; e < 6; ++e) x[e] = e == r ? 1.0 : 0.0;
  pg_chol6_solve(L, x);
}

// The last level's single node: P[0] = D^-1.
PG_HD void pg_selinv_top(const PgLevel& lv, double* P) {
  double L[36], x[6];
  pg_ld36(lv.L, lv.n, 0, L);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    pg_chol6_inv_row(L, r, x);
#pragma unroll
    for (int c = 0; c < 6; ++c) P[(6 * r + c) * lv.n] = x[c];
  }
}

// Node m of a level from the next level's nP, nQ (nn nodes).  Even m = 2q: P[m] = nP[q].  Odd k,
// a = (k - 1) / 2, Sl = nP[a], Sr = nP[a+1], Srl = nQ[a+1]:
//   Kl = S[k][k-1] = -G_k Sl - H_k Srl        Kr = S[k][k+1] = -G_k Srl^T - H_k Sr
//   P[k] = D_k^-1 - Kl G_k^T - Kr H_k^T       Q[k] = Kl        Q[k+1] = Kr^T
// (terms of an absent right neighbour dropped).  The odd node writes Q[k+1]: no two nodes write one
// block.  Q[0] is never written or read.
PG_HD void pg_selinv_up(const PgLevel& lv, const double* nP, const double* nQ, int64_t nn, double* P, double* Q,
                        int64_t m) {
  const int64_t n = lv.n;
  if (!(m & 1)) {
    double S[36];
    pg_ld36(nP, nn, m >> 1, S);
    pg_st36(P, n, m, S);
    return;
  }
  const int64_t a = (m - 1) >> 1;
  const bool right = m + 1 < n;
  // Two passes over the rows, neither unrolled, the first leaving Kl and Kr in Q: a thread holds
  // three 6x6 blocks at a time and not six (registers on the device).
  {
    double Sl[36], Srl[36], Sr[36];
    pg_ld36(nP, nn, a, Sl);
    if (right) {
      pg_ld36(nP, nn, a + 1, Sr);
      pg_ld36(nQ, nn, a + 1, Srl);
    } else {
#pragma unroll
      for (int e = 0; e < 36; ++e) Sr[e] = Srl[e] = 0.0;
    }
#pragma unroll 1
    for (int r = 0; r < 6; ++r) {
      double g[6], h[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        g[k] = lv.G[(6 * r + k) * n + m];
        h[k] = right ? lv.H[(6 * r + k) * n + m] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s = 0.0, t = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s = s + g[k] * Sl[6 * k + c];
#pragma unroll
        for (int k = 0; k < 6; ++k) s = s + h[k] * Srl[6 * k + c];
#pragma unroll
        for (int k = 0; k < 6; ++k) t = t + g[k] * Srl[6 * c + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) t = t + h[k] * Sr[6 * k + c];
        Q[(6 * r + c) * n + m] = -s;
        if (right) Q[(6 * c + r) * n + m + 1] = -t;
      }
    }
  }
  double G[36], H[36], L[36];
  pg_ld36(lv.G, n, m, G);
  pg_ld36(lv.L, n, m, L);
  if (right) {
    pg_ld36(lv.H, n, m, H);
  } else {
#pragma unroll
    for (int e = 0; e < 36; ++e) H[e] = 0.0;
  }
#pragma unroll 1
  for (int r = 0; r < 6; ++r) {
    double kl[6], kr[6], di[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      kl[c] = Q[(6 * r + c) * n + m];
      kr[c] = right ? Q[(6 * c + r) * n + m + 1] : 0.0;
    }
    pg_chol6_inv_row(L, r, di);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s + kl[k] * G[6 * c + k];
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s + kr[k] * H[6 * c + k];
      P[(6 * r + c) * n + m] = di[c] - s;
    }
  }
}

// The cyclic-reduction solve of right-hand-side column c: the steps above on the [6][n] vectors at
// offset c * 6 * n of each level's b and x.
PG_HD PgLevel pg_level_col(const PgLevel& lv, int64_t c) {
  PgLevel o = lv;
  o.b = lv.b + c * 6 * lv.n;
  o.x = lv.x + c * 6 * lv.n;
  return o;
}
PG_HD void pg_cr_reduce_col(const PgLevel& lv, const PgLevel& nx, int64_t q, int64_t c) {
  pg_cr_reduce(pg_level_col(lv, c), pg_level_col(nx, c), q);
}
PG_HD void pg_cr_top_col(const PgLevel& lv, int64_t c) { pg_cr_top(pg_level_col(lv, c)); }
PG_HD void pg_cr_backsub_col(const PgLevel& lv, const PgLevel& nx, int64_t m, int64_t c) {
  pg_cr_backsub(pg_level_col(lv, c), pg_level_col(nx, c), m);
}

// Entry e of node `side` (0: i, 1: j) of column col = 6 f + r of U^T, f the loop factor fk's rank
// among the loop factors: row r of its whitened J_side.
PG_HD double pg_marg_rhs_entry(const double* lin, int32_t fk, int r, int side, int e) {
  return lin[(int64_t)fk * kPgLin + 6 + 36 * side + 6 * r + e];
}

// C[row][col] = delta + U[row] . W[:, col], row = 6 f + r: J_i's row r against node i's six entries
// of column col, then J_j's against node j's.
PG_HD double pg_marg_c_entry(const PgFactor* fac, const double* lin, const int32_t* loops, const double* W, int64_t n,
                             int64_t row, int64_t col) {
  const int32_t fk = loops[row / 6];
  const int r = (int)(row % 6);
  const double* Ji = lin + (int64_t)fk * kPgLin + 6 + 6 * r;
  const double* Jj = Ji + 36;
  const double* w = W + col * 6 * n;
  const int64_t i = fac[fk].i, j = fac[fk].j;
  double s = row == col ? 1.0 : 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) s = s + Ji[e] * w[e * n + i];
#pragma unroll
  for (int e = 0; e < 6; ++e) s = s + Jj[e] * w[e * n + j];
  return s;
}

// ---- dense Cholesky of C [M][M] row-major, lower triangle, in place, blocked right-looking ----
constexpr int kPgPanel = 32;  // columns of a panel

// The panel's diagonal block Ld (nb x nb, leading dimension ld), right-looking: false on a bad pivot
// (taken as 1, as pg_chol6).  An entry's updates come in column order whichever way they are
// scheduled, so a parallel version gives the same bits.
PG_HD bool pg_dense_chol_block(double* Ld, int64_t ld, int nb) {
  bool ok = true;
  for (int j = 0; j < nb; ++j) {
    double d = Ld[j * ld + j];
    if (!(d > 0.0) || !(d < INFINITY)) {
      ok = false;
      d = 1.0;
    }
    const double l = sqrt(d);
    Ld[j * ld + j] = l;
    for (int i = j + 1; i < nb; ++i) Ld[i * ld + j] = Ld[i * ld + j] / l;
    for (int i = j + 1; i < nb; ++i)
      for (int k = j + 1; k <= i; ++k) Ld[i * ld + k] = Ld[i * ld + k] - Ld[i * ld + j] * Ld[k * ld + j];
  }
  return ok;
}
// Row i > the panel [j0, j0 + nb) of A: A[i][j0 ..] = A[i][j0 ..] Ld^-T, in place.
PG_HD void pg_dense_panel_row(double* A, int64_t M, int64_t j0, int nb, const double* Ld, int64_t ld, int64_t i) {
  double* a = A + i * M + j0;
  for (int k = 0; k < nb; ++k) {
    double s = a[k];
    for (int t = 0; t < k; ++t) s = s - a[t] * Ld[k * ld + t];
    a[k] = s / Ld[k * ld + k];
  }
}
// Trailing entry (i, j), j <= i, both past the panel: A[i][j] -= sum_k A[i][j0 + k] A[j][j0 + k].
PG_HD void pg_dense_trail_entry(double* A, int64_t M, int64_t j0, int nb, int64_t i, int64_t j) {
  double s = 0.0;
  for (int k = 0; k < nb; ++k) s = s + A[i * M + j0 + k] * A[j * M + j0 + k];
  A[i * M + j] = A[i * M + j] - s;
}

// Y = Lc^-1 W_i^T for entry e of node i, in place on W's lane (e, i): y[c] = W[(6 c + e) n + i].
// Eight rows at a time, so that y[k] is read once per eight rows; each row's sum in column order.
PG_HD void pg_marg_forward(const double* Lc, int64_t M, double* W, int64_t n, int64_t i, int e) {
  double* y = W + (int64_t)e * n + i;
  const int64_t st = 6 * n;
  for (int64_t r0 = 0; r0 < M; r0 += 8) {
    double acc[8];
    const double* Lr[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t row = r0 + u < M ? r0 + u : M - 1;  // rows past the end repeat the last one and are not stored
      Lr[u] = Lc + row * M;
      acc[u] = y[row * st];
    }
    for (int64_t k = 0; k < r0; ++k) {
      const double yk = y[k * st];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = acc[u] - Lr[u][k] * yk;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (r0 + u < M) {  // (so r0 + t < M too)
        double s = acc[u];
#pragma unroll
        for (int t = 0; t < u; ++t) s = s - Lr[u][r0 + t] * acc[t];
        acc[u] = s / Lr[u][r0 + u];
        y[(r0 + u) * st] = acc[u];
      }
    }
  }
}

// addGPSFactor's gate (mapOptmization.h:1561) on a node's marginal [36]: a GPS factor is wanted
// unless both poseCovariance(3,3) and (4,4) are below the threshold.
PG_HD int pg_gps_gate_wanted(const double* cov, double threshold) {
  return !(cov[6 * 3 + 3] < threshold && cov[6 * 4 + 4] < threshold) ? 1 : 0;
}

// Sigma_ii = P_i - Y_i^T Y_i into out [36] row-major: r <= c computed (the sum over Y's rows in
// order) and mirrored.
PG_HD void pg_marg_final(const double* P, const double* Y, int64_t M, int64_t n, int64_t i, double* out) {
  double s[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) s[k] = 0.0;
  for (int64_t col = 0; col < M; ++col) {
    double y[6];
    pg_ld6(Y + col * 6 * n, n, i, y);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) {
        const int k = 6 * r - r * (r - 1) / 2 + (c - r);  // (r, c)'s place among the 21 pairs
        s[k] = s[k] + y[r] * y[c];
      }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) {
      const double v = P[(6 * r + c) * n + i] - s[6 * r - r * (r - 1) / 2 + (c - r)];
      out[6 * r + c] = v;
      out[6 * c + r] = v;
    }
}

// ---- robust loop factors (include/fbr.h "robust loop factors") ----
enum { kPgRobustNone = 0, kPgRobustHuber = 1, kPgRobustCauchy = 2 };

// rho and the weight w = 2 rho'(s) of a factor whose whitened residual has s = |r|^2; k is the
// scale, in units of e = sqrt(s).  kPgRobustNone: rho = s / 2, w = 1.
PG_HD void pg_robust(int kind, double k, double s, double* rho, double* w) {
  if (kind == kPgRobustHuber) {
    const double e = sqrt(s);
    if (e <= k) {
      *rho = 0.5 * s;
      *w = 1.0;
    } else {
      *rho = k * (e - 0.5 * k);
      *w = k / e;
    }
  } else if (kind == kPgRobustCauchy) {
    const double q = s / (k * k);
    *rho = (0.5 * (k * k)) * log1p(q);
    *w = 1.0 / (1.0 + q);
  } else {
    *rho = 0.5 * s;
    *w = 1.0;
  }
}

// Factor f after its evaluation (fcost[f] = s / 2, and with jac its kPgLin doubles of lin): chi2[f]
// = s and wt[f] = w always; a loop factor's fcost becomes rho and, with jac, its r, J_i and J_j
// are scaled by sqrt(w) (GTSAM's noiseModel::Robust whitens this way).  Every other factor keeps
// rho = s / 2 and w = 1.
PG_HD void pg_robust_factor(const PgFactor* fac, int64_t f, int kind, double k, bool jac, double* lin, double* fcost,
                            double* chi2, double* wt) {
  const double s = 2.0 * fcost[f];
  double rho = fcost[f], w = 1.0;
  if (fac[f].loop) pg_robust(kind, k, s, &rho, &w);
  chi2[f] = s;
  wt[f] = w;
  if (!fac[f].loop) return;
  fcost[f] = rho;
  if (!jac) return;
  const double sw = sqrt(w);
  double* o = lin + f * kPgLin;
  for (int e = 0; e < kPgLin; ++e) o[e] = o[e] * sw;
}

// ---- the direct solve of a damped step (include/fbr.h "direct solve") ----
// H = T + U^T U with T the damped block-tridiagonal part, factored by the cyclic reduction above,
// and U the loop factors' whitened Jacobians, as in the marginals:
//   y = T^-1 (-g),  W = T^-1 U^T,  C = I + U W = Lc Lc^T  (the marginals' steps, on the damped T)
//   z = U y (pg_direct_z_entry),  Lc Lc^T s = z (pg_subst_*),  delta = y - W s (pg_direct_delta_entry).

// z[row] = U[row] . y, row = 6 f + r: J_i's row r against node i's six entries of y [6][n], then
// J_j's against node j's.
PG_HD double pg_direct_z_entry(const PgFactor* fac, const double* lin, const int32_t* loops, const double* y, int64_t n,
                               int64_t row) {
  const int32_t fk = loops[row / 6];
  const int r = (int)(row % 6);
  const double* Ji = lin + (int64_t)fk * kPgLin + 6 + 6 * r;
  const double* Jj = Ji + 36;
  const int64_t i = fac[fk].i, j = fac[fk].j;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) s = s + Ji[e] * y[e * n + i];
#pragma unroll
  for (int e = 0; e < 6; ++e) s = s + Jj[e] * y[e * n + j];
  return s;
}

// The two operations of a substitution that sweeps the columns: finish entry k, then take its term
// out of every entry that still waits for it.
PG_HD double pg_subst_pivot(double v, double d) { return v / d; }
PG_HD double pg_subst_sub(double v, double l, double s) { return v - l * s; }

// Lc Lc^T s = z in place on z [M] (Lc row-major, lower), column by column: forwards k = 0 .. M-1
// with Lc's column k on the rows below, backwards k = M-1 .. 0 with Lc's row k on the rows above.
// An entry takes its terms in the order in which they become known: ascending k forwards,
// descending k backwards.  k_pg_direct_subst spreads the inner loops over a workgroup; the
// operations per entry and their order are these.
PG_HD void pg_dense_subst(const double* Lc, int64_t M, double* z) {
  for (int64_t k = 0; k < M; ++k) {
    z[k] = pg_subst_pivot(z[k], Lc[k * M + k]);
    for (int64_t r = k + 1; r < M; ++r) z[r] = pg_subst_sub(z[r], Lc[r * M + k], z[k]);
  }
  for (int64_t k = M - 1; k >= 0; --k) {
    z[k] = pg_subst_pivot(z[k], Lc[k * M + k]);
    for (int64_t r = 0; r < k; ++r) z[r] = pg_subst_sub(z[r], Lc[k * M + r], z[k]);
  }
}

// delta[t] = y[t] - sum_col W[col][t] s[col], t = e n + m an entry of the [6][n] vectors, the sum
// over the columns in ascending order (M = 0: delta = y).
PG_HD double pg_direct_delta_entry(const double* y, const double* W, const double* s, int64_t M, int64_t n, int64_t t) {
  double acc = 0.0;
  for (int64_t col = 0; col < M; ++col) acc = acc + W[col * 6 * n + t] * s[col];
  return M > 0 ? y[t] - acc : y[t];
}

}  // namespace fbr
