// fbr_reg_info.h — the record arithmetic of include/fbr.h ("registration information"), host and
// device, all in double: the cyclic Jacobi of the 6x6 normal matrix, the covariance assembly with
// its floor, the chart map S = blockdiag(E, R^T) and the record itself (flags included) from a job's
// summed products.  k_reg_info.hip compiles these functions for the device and
// tests/native/info_probe.cpp for the CPU, so the tests check them without a GPU.
//
// Every matrix lives in caller-provided memory (InfoWork: LDS on the device, the stack on the host)
// and no function indexes a local array with a run-time index, so the device code needs no scratch.
// Must be compiled with -ffp-contract=off: every product and sum below is its own rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fbr_common.h"

namespace fbr {

constexpr int kInfoSweeps = 16;  // sweep limit of the Jacobi (a 6x6 matrix converges in 6 to 9)
constexpr int kInfoSums = 29;    // a job's summed products: 21 H upper, 6 g, the row count, rss

struct InfoWork {
  double A[36];  // the matrix under rotation
  double V[36];  // the accumulated rotations (columns = eigenvectors)
  double S[36];  // the chart map
  double M[36];  // S cov
};

__host__ __device__ inline bool info_finite(double v) { return v - v == 0.0; }

// eig ascending, evec row i = the unit eigenvector of eig[i].  Cyclic Jacobi by rows: in every
// sweep the rotations (p, q), p < q, in row-major order, each annihilating a_pq exactly
// (t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq), c = 1 / sqrt(t^2 + 1),
// s = t c); a sweep that finds every off-diagonal entry zero ends it, as does the sweep limit.
// From the fifth sweep on (sweep index > 3) an entry that no longer changes either of its diagonal
// neighbours at 100 x its size (|a_pp| + 100 |a_pq| == |a_pp|, and the same for a_qq) is set to zero
// without a rotation.  Returns the sweeps that rotated.
// Backward error: every rotation is an orthogonal similarity up to a few ulps of ||H||_F, so the
// computed eigenvalues are those of H + dH with ||dH||_F <= k 6 2^-52 ||H||_F for
// k = 15 kInfoSweeps rotations at most.
__host__ __device__ inline int info_jacobi6(const double* H, double* eig, double* evec, InfoWork* w) {
  double* A = w->A;
  double* V = w->V;
  for (int k = 0; k < 36; ++k) {
    A[k] = H[k];
    V[k] = (k % 7 == 0) ? 1.0 : 0.0;
  }
  int sweeps = 0;
  for (int sweep = 0; sweep < kInfoSweeps; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) off += fabs(A[p * 6 + q]);
    if (!(off > 0.0)) break;  // (a NaN ends it too)
    ++sweeps;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[p * 6 + q];
        if (apq == 0.0) continue;
        const double app = A[p * 6 + p], aqq = A[q * 6 + q];
        const double g = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
          A[p * 6 + q] = 0.0;
          A[q * 6 + p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[p * 6 + p] = app - t * apq;
        A[q * 6 + q] = aqq + t * apq;
        A[p * 6 + q] = 0.0;
        A[q * 6 + p] = 0.0;
        for (int r = 0; r < 6; ++r) {
          if (r != p && r != q) {
            const double arp = A[r * 6 + p], arq = A[r * 6 + q];
            const double np = c * arp - s * arq, nq = s * arp + c * arq;
            A[r * 6 + p] = np;
            A[p * 6 + r] = np;
            A[r * 6 + q] = nq;
            A[q * 6 + r] = nq;
          }
          const double vrp = V[r * 6 + p], vrq = V[r * 6 + q];
          V[r * 6 + p] = c * vrp - s * vrq;
          V[r * 6 + q] = s * vrp + c * vrq;
        }
      }
  }
  // ascending, equal values in their order on the diagonal: a stable insertion sort of (eig, row)
  for (int i = 0; i < 6; ++i) {
    eig[i] = A[i * 7];
    for (int r = 0; r < 6; ++r) evec[i * 6 + r] = V[r * 6 + i];
  }
  for (int i = 1; i < 6; ++i)
    for (int j = i; j > 0 && eig[j - 1] > eig[j]; --j) {
      const double e = eig[j];
      eig[j] = eig[j - 1];
      eig[j - 1] = e;
      for (int r = 0; r < 6; ++r) {
        const double v = evec[j * 6 + r];
        evec[j * 6 + r] = evec[(j - 1) * 6 + r];
        evec[(j - 1) * 6 + r] = v;
      }
    }
  return sweeps;
}

// R = Rz(yaw) Ry(pitch) Rx(roll) and E (fbr.h), in double from the float pose, as S = blockdiag(E, R^T).
__host__ __device__ inline void info_chart(const float* pose, double* S) {
  const double roll = (double)pose[0], pitch = (double)pose[1], yaw = (double)pose[2];
  const double cr = cos(roll), sr = sin(roll), cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
  for (int k = 0; k < 36; ++k) S[k] = 0.0;
  S[0] = 1.0;  S[2] = -sp;
  S[7] = cr;   S[8] = sr * cp;
  S[13] = -sr; S[14] = cr * cp;
  // R, transposed into the lower block
  const double r00 = cy * cp, r01 = cy * sp * sr - sy * cr, r02 = cy * sp * cr + sy * sr;
  const double r10 = sy * cp, r11 = sy * sp * sr + cy * cr, r12 = sy * sp * cr - cy * sr;
  const double r20 = -sp, r21 = cp * sr, r22 = cp * cr;
  S[21] = r00; S[22] = r10; S[23] = r20;
  S[27] = r01; S[28] = r11; S[29] = r21;
  S[33] = r02; S[34] = r12; S[35] = r22;
}

// cov = sum_i v_i v_i^T w_i, w_i = sigma2 / eig[i] above the floor, `unobserved` otherwise; the
// upper triangle is summed (i ascending) and mirrored.  Returns the rank.
__host__ __device__ inline int info_cov(const double* eig, const double* evec, double sigma2, double eig_floor,
                                        double unobserved, double* cov) {
  int rank = 0;
  for (int i = 0; i < 6; ++i) rank += eig[i] > eig_floor ? 1 : 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      double s = 0.0;
      for (int i = 0; i < 6; ++i) {
        const double wi = eig[i] > eig_floor ? sigma2 / eig[i] : unobserved;
        s += (evec[i * 6 + r] * evec[i * 6 + c]) * wi;
      }
      cov[r * 6 + c] = s;
      cov[c * 6 + r] = s;
    }
  return rank;
}

// out = S cov S^T (M = S cov first; the upper triangle is computed and mirrored).
__host__ __device__ inline void info_to_tangent(const double* S, const double* cov, double* M, double* out) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += S[r * 6 + k] * cov[k * 6 + c];
      M[r * 6 + c] = s;
    }
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += M[r * 6 + k] * S[c * 6 + k];
      out[r * 6 + c] = s;
      out[c * 6 + r] = s;
    }
}

__host__ __device__ inline void info_flagged(fbr_reg_info* r, double unobserved) {
  for (int k = 0; k < 36; ++k) {
    const double d = (k % 7 == 0) ? 1.0 : 0.0;
    r->H[k] = 0.0;
    r->evec[k] = d;
    r->cov[k] = d * unobserved;
    r->cov_tangent[k] = d * unobserved;
  }
  for (int k = 0; k < 6; ++k) {
    r->g[k] = 0.0;
    r->eig[k] = 0.0;
    r->var_tangent[k] = unobserved;
  }
  r->rss = 0.0;
  r->sigma2 = 0.0;
  r->rank = 0;
}

// The record of one job from its summed products acc[kInfoSums] (upper H by rows, g, count, rss).
// flags_in: FBR_INFO_NOT_REGISTERED or 0; the other flags are decided here.
__host__ __device__ inline void info_record(const double* acc, int n_rows_c, int n_rows_s, int n_query_c, int n_query_s,
                                            const float* pose, int flags_in, double eig_floor, double unobserved,
                                            double sigma2_param, fbr_reg_info* r, InfoWork* w) {
  r->n_rows[0] = n_rows_c;
  r->n_rows[1] = n_rows_s;
  r->n_query[0] = n_query_c;
  r->n_query[1] = n_query_s;
  const int n = n_rows_c + n_rows_s;
  int flags = flags_in;
  bool fin = true;
  for (int k = 0; k < 6; ++k) fin = fin && info_finite((double)pose[k]);
  if (!fin) flags |= FBR_INFO_BAD_POSE;
  if (!flags && n == 0) flags |= FBR_INFO_NO_ROWS;
  if (!flags && n < 6) flags |= FBR_INFO_FEW_ROWS;
  r->flags = flags;
  if (flags) {
    info_flagged(r, unobserved);
    return;
  }
  int q = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      r->H[a * 6 + b] = acc[q];
      r->H[b * 6 + a] = acc[q];
      ++q;
    }
  for (int k = 0; k < 6; ++k) r->g[k] = acc[21 + k];
  r->rss = acc[28];
  const int dof = n - 6 > 1 ? n - 6 : 1;
  r->sigma2 = sigma2_param > 0.0 ? sigma2_param : r->rss / (double)dof;
  info_jacobi6(r->H, r->eig, r->evec, w);
  r->rank = info_cov(r->eig, r->evec, r->sigma2, eig_floor, unobserved, r->cov);
  info_chart(pose, w->S);
  info_to_tangent(w->S, r->cov, w->M, r->cov_tangent);
  for (int k = 0; k < 6; ++k) r->var_tangent[k] = r->cov_tangent[k * 7];
}

}  // namespace fbr
