// fbr_sc.h — the scan-context arithmetic of include/fbr.h ("place recognition"), host and device:
// the polar bin of a point, the value a point offers its cell, a column's norm and the distance of
// two descriptors at one column shift.  k_scancontext.hip compiles these functions for the device
// and tests/native/sc_probe.cpp for the CPU, so the tests check the kernels' arithmetic without a
// GPU.  The contract is the project's own restatement of Scan Context (Kim & Kim, IROS 2018), not
// pinned against any third-party code.
//
// Must be compiled with -ffp-contract=off: every product and sum below is its own rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fbr_common.h"
#include "fbr_fdlibm.h"

namespace fbr {

constexpr int kScMaxRing = 32, kScMaxSector = 64, kScMaxK = 16;
constexpr float kScTwoPi = 6.2831854820251465f;  // (float)(2 pi)

__host__ __device__ inline bool sc_finite(float v) { return (f2bits(v) & 0x7f800000) != 0x7f800000; }

// The cell of a point, in float, operation by operation:
//   r      = sqrt_rn(x * x + y * y)                     (correctly rounded square root)
//   dropped unless x, y, z are finite and r < max_radius
//   ring   = min(n_ring - 1, (int)floorf((r / max_radius) * (float)n_ring))
//   theta  = fd_atan2f(y, x);  if (theta < 0) theta = theta + (float)(2 pi)
//   sector = min(n_sector - 1, (int)floorf((theta / (float)(2 pi)) * (float)n_sector))
// Returns ring * n_sector + sector, or -1 for a dropped point.
__host__ __device__ inline int sc_cell(float x, float y, float z, int n_ring, int n_sector, float max_radius) {
  if (!sc_finite(x) || !sc_finite(y) || !sc_finite(z)) return -1;
  const float r = sqrt_rn(x * x + y * y);
  if (!(r < max_radius)) return -1;
  int ring = (int)__builtin_floorf((r / max_radius) * (float)n_ring);
  if (ring > n_ring - 1) ring = n_ring - 1;
  float theta = fd_atan2f(y, x);
  if (theta < 0.0f) theta = theta + kScTwoPi;
  int sector = (int)__builtin_floorf((theta / kScTwoPi) * (float)n_sector);
  if (sector > n_sector - 1) sector = n_sector - 1;
  return ring * n_sector + sector;
}

// What a point offers its cell: max(z + lidar_height, 0) in float, as the bits of a non-negative
// float (never -0), so that an integer maximum of the bits is the float maximum.
__host__ __device__ inline uint32_t sc_value_bits(float z, float lidar_height) {
  const float t = z + lidar_height;
  return t > 0.0f ? (uint32_t)f2bits(t) : 0u;
}

// ||D[:, c]||: the square root of the double sum of squares, rings ascending.  D is [n_ring][n_sector].
__host__ __device__ inline double sc_column_norm(const float* D, int n_ring, int n_sector, int c) {
  double s = 0.0;
  for (int r = 0; r < n_ring; ++r) {
    const double v = (double)D[r * n_sector + c];
    s = s + v * v;
  }
  return sqrt(s);
}
__host__ __device__ inline double sc_inverse_norm(double norm) { return norm > 0.0 ? 1.0 / norm : 0.0; }

// d(s) of query Q against candidate C: columns c ascending; a column counts where both norms are
// > 0 (inverse norms qi / ci: 0 marks an empty column); cos_c = (sum_r Q[r][c] C[r][(c + s) mod
// n_sector]) * qi[c] * ci[(c + s) mod n_sector] with the sum in double, rings ascending;
// d = 1 - (sum_c cos_c) / n_eff, 1.0 when no column counts.
__host__ __device__ inline double sc_distance(const float* Q, const double* qi, const float* C, const double* ci,
                                              int n_ring, int n_sector, int s) {
  double sum = 0.0;
  int n_eff = 0;
  int cc = s;  // (c + s) mod n_sector
  for (int c = 0; c < n_sector; ++c) {
    const double a = qi[c];
    if (a > 0.0) {  // (the same for every shift: uniform across a wave)
      const double b = ci[cc];
      double dot = 0.0;
      for (int r = 0; r < n_ring; ++r) dot = dot + (double)Q[r * n_sector + c] * (double)C[r * n_sector + cc];
      if (b > 0.0) {
        sum = sum + (dot * a) * b;
        ++n_eff;
      }
    }
    cc = cc + 1 == n_sector ? 0 : cc + 1;
  }
  return n_eff ? 1.0 - sum / (double)n_eff : 1.0;
}

}  // namespace fbr
