// fbr_icp_solve.h — the transformation estimate of one ICP iteration (k_icp_solve, k_icp.hip):
// Umeyama without scaling from the 17 sums of the correspondences, with the 3x3 SVD it needs.
//
// Host and device: the kernel calls icp_umeyama() on the summed partials, and
// tests/native/host_probe.cpp compiles the same source for the CPU, where the tests compare it
// with a centred float64 reference on rank-deficient, mirrored and far-from-origin clouds.
//
// Must be compiled with -ffp-contract=off (the kernel and the probe then evaluate the same
// expressions).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBR_ICP_HD __host__ __device__
#else
#define FBR_ICP_HD
#endif

namespace fbr {

// determinant of a row-major 3x3
FBR_ICP_HD inline double icp_det3(const double m[9]) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// A = U diag(w) V^T of a 3x3 double matrix (row-major) by one-sided Jacobi, w descending.  A
// vanishing third singular value takes u2 = det(V) u0 x u1 (so det U = det V); lower ranks get an
// orthonormal completion.
FBR_ICP_HD inline void icp_svd3(const double A[9], double U[9], double w[3], double V[9]) {
  double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int k = 0; k < 9; ++k) a[k] = A[k];
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < 3; ++r) {
          al += a[3 * r + p] * a[3 * r + p];
          be += a[3 * r + q] * a[3 * r + q];
          ga += a[3 * r + p] * a[3 * r + q];
        }
        if (ga == 0.0 || ga * ga <= 1e-32 * al * be) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 3; ++r) {
          const double ap = a[3 * r + p], aq = a[3 * r + q];
          a[3 * r + p] = c * ap - s * aq;
          a[3 * r + q] = s * ap + c * aq;
          const double vp = v[3 * r + p], vq = v[3 * r + q];
          v[3 * r + p] = c * vp - s * vq;
          v[3 * r + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  for (int j = 0; j < 3; ++j) w[j] = sqrt(a[j] * a[j] + a[3 + j] * a[3 + j] + a[6 + j] * a[6 + j]);
  for (int pass = 0; pass < 3; ++pass)  // columns by descending singular value
    for (int j = 0; j + 1 < 3; ++j)
      if (w[j] < w[j + 1]) {
        const double tw = w[j];
        w[j] = w[j + 1];
        w[j + 1] = tw;
        for (int r = 0; r < 3; ++r) {
          const double ta = a[3 * r + j], tv = v[3 * r + j];
          a[3 * r + j] = a[3 * r + j + 1];
          a[3 * r + j + 1] = ta;
          v[3 * r + j] = v[3 * r + j + 1];
          v[3 * r + j + 1] = tv;
        }
      }
  for (int k = 0; k < 9; ++k) V[k] = v[k];
  const double tiny = 1e-14 * w[0];
  if (!(w[0] > 0.0)) {
    for (int k = 0; k < 9; ++k) U[k] = (k % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  for (int r = 0; r < 3; ++r) U[3 * r] = a[3 * r] / w[0];
  if (w[1] > tiny) {
    for (int r = 0; r < 3; ++r) U[3 * r + 1] = a[3 * r + 1] / w[1];
  } else {  // any unit vector orthogonal to u0
    const int m = fabs(U[0]) <= fabs(U[3]) ? (fabs(U[0]) <= fabs(U[6]) ? 0 : 2) : (fabs(U[3]) <= fabs(U[6]) ? 1 : 2);
    double e[3] = {0, 0, 0};
    e[m] = 1.0;
    const double d = U[3 * m];
    double nn = 0;
    for (int r = 0; r < 3; ++r) {
      e[r] -= d * U[3 * r];
      nn += e[r] * e[r];
    }
    nn = sqrt(nn);
    for (int r = 0; r < 3; ++r) U[3 * r + 1] = e[r] / nn;
  }
  if (w[2] > tiny && w[1] > tiny) {
    for (int r = 0; r < 3; ++r) U[3 * r + 2] = a[3 * r + 2] / w[2];
  } else {
    const double detv = v[0] * (v[4] * v[8] - v[5] * v[7]) - v[1] * (v[3] * v[8] - v[5] * v[6]) +
                        v[2] * (v[3] * v[7] - v[4] * v[6]);
    const double sg = detv < 0 ? -1.0 : 1.0;
    U[2] = sg * (U[3] * U[7] - U[6] * U[4]);
    U[5] = sg * (U[6] * U[1] - U[0] * U[7]);
    U[8] = sg * (U[0] * U[4] - U[3] * U[1]);
  }
}

// Umeyama without scaling from v = count, sum s (3), sum t (3), sum t_r s_c (9), sum d2 of at
// least one correspondence: T (row-major 3x4, rounded to float) with t ~ R s + tr.  S = diag(1, 1,
// det(U) det(V) < 0 ? -1 : 1), so R = U S V^T is a proper rotation whatever the rank of sigma: the
// sign of det(sigma) itself is rounding noise once the third singular value vanishes (a planar
// cloud), and icp_svd3's completion keeps det U = det V there.
FBR_ICP_HD inline void icp_umeyama(const double v[17], float T[12]) {
  const double n = v[0];
  double ms[3], mt[3], sig[9], U[9], w[3], V[9];
  for (int r = 0; r < 3; ++r) {
    ms[r] = v[1 + r] / n;
    mt[r] = v[4 + r] / n;
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sig[3 * r + c] = v[7 + 3 * r + c] / n - mt[r] * ms[c];
  icp_svd3(sig, U, w, V);
  const double S[3] = {1.0, 1.0, icp_det3(U) * icp_det3(V) < 0 ? -1.0 : 1.0};
  for (int r = 0; r < 3; ++r) {
    double R[3];
    for (int c = 0; c < 3; ++c)
      R[c] = (U[3 * r] * S[0] * V[3 * c] + U[3 * r + 1] * S[1] * V[3 * c + 1]) + U[3 * r + 2] * S[2] * V[3 * c + 2];
    const double t = mt[r] - ((R[0] * ms[0] + R[1] * ms[1]) + R[2] * ms[2]);
    for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[c];
    T[4 * r + 3] = (float)t;
  }
}

}  // namespace fbr
