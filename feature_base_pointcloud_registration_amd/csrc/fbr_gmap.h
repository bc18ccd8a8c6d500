// fbr_gmap.h — the grid and key arithmetic of the wide VoxelGrid (include/fbr.h, "global map"),
// host and device: k_gmap.hip compiles these functions for the device, tests/native/gmap_probe.cpp
// and tests/native/gmap_host_check.cpp for the CPU, so the tests check the kernels' arithmetic
// against the NumPy model (tests/gmap_model.py) without a GPU.
//
// PCL's VoxelGrid gives up when its cell count exceeds INT32_MAX ("Leaf size is too small") and
// returns its input; at a 0.2 m leaf that is roughly a 250 m cube.  The wide filter keeps PCL's
// grid (float min / max box, leaf inverse, min_b, div_b, ijk) and widens the key to 64 bits:
//   key = ijk0 + ijk1 * div0 + ijk2 * div0 * div1            (uint64)
// Where PCL does not overflow the key equals PCL's, so the wide filter then emits VgGrid's voxels
// (fbr_vg_sort.h) in VgGrid's order.  Where PCL overflows there is no PCL output to reproduce: the
// wide mode is the project's own extension.
//
// Limits, reported in status:
//   kGmapBound  some |bound * inv| >= 2^24: floorf(p * inv) is no longer an exact cell number
//   kGmapCells  div0 * div1 * div2 >= 2^63: the key (and the marker above it) needs 64 bits
// Within them every div_b is below 2^25.  ijk = (int)(floorf(p * inv) - (float)min_b) is PCL's
// expression and is kept as it is: it is exact while an axis spans fewer than 2^24 cells, beyond
// that the float difference rounds as PCL's own would.
//
// Must be compiled with -ffp-contract=off: every product and difference below is its own rounding.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBR_GMAP_HD __host__ __device__
#else
#define FBR_GMAP_HD
#endif

namespace fbr {

constexpr int32_t kGmapOk = 0, kGmapBound = 1, kGmapCells = 2;

struct GmapGrid {
  float inv;             // 1.0f / leaf
  int32_t min_b[3], max_b[3], div_b[3];
  uint64_t mul1, mul2;   // div0, div0 * div1
  int32_t pcl_overflow;  // PCL's dx * dy * dz > INT32_MAX held: PCL returns its input (set with every status)
  int32_t status;        // kGmap*; min_b .. mul2 and nbits are valid only with kGmapOk
  int32_t nbits;         // key bits: every key is below 2^nbits (1..63); 2^nbits marks a dropped point
  int32_t pad_;
};

FBR_GMAP_HD inline bool gmap_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN

// The grid of the box [mn, mx] (getMinMax3D of the cloud) at `leaf`, as VgGrid::init computes it.
FBR_GMAP_HD inline void gmap_grid_init(GmapGrid& G, const float mn[3], const float mx[3], float leaf) {
  G.inv = 1.0f / leaf;
  G.mul1 = G.mul2 = 0;
  G.pcl_overflow = 0;
  G.status = kGmapOk;
  G.nbits = 1;
  G.pad_ = 0;
  for (int d = 0; d < 3; ++d) G.min_b[d] = G.max_b[d] = G.div_b[d] = 0;
  // PCL: dx * dy * dz > INT32_MAX with d = (int64)((max - min) * inv) + 1, taken factor by factor so
  // that no float outside int64's range is cast and no product overflows (valid with every status)
  {
    int64_t cells = 1;
    for (int d = 0; d < 3 && !G.pcl_overflow; ++d) {
      const float f = (mx[d] - mn[d]) * G.inv;
      if (!(f < 2147483648.0f)) {  // also NaN
        G.pcl_overflow = 1;
      } else {
        const int64_t dd = (f > 0.0f ? (int64_t)f : 0) + 1;
        cells *= dd;  // <= 2^31 * 2^31
        if (cells > (int64_t)INT32_MAX) G.pcl_overflow = 1;
      }
    }
  }
  for (int d = 0; d < 3; ++d)  // also an infinite or NaN bound: nothing below is cast to an integer
    if (!(fabsf(mn[d] * G.inv) < 16777216.0f) || !(fabsf(mx[d] * G.inv) < 16777216.0f)) G.status = kGmapBound;
  if (G.status != kGmapOk) return;
  for (int d = 0; d < 3; ++d) {
    G.min_b[d] = (int32_t)floorf(mn[d] * G.inv);
    G.max_b[d] = (int32_t)floorf(mx[d] * G.inv);
    G.div_b[d] = G.max_b[d] - G.min_b[d] + 1;
    if (G.div_b[d] < 1) G.div_b[d] = 1;  // an empty box (mn > mx: no finite point)
  }
  G.mul1 = (uint64_t)G.div_b[0];
  G.mul2 = G.mul1 * (uint64_t)G.div_b[1];  // < 2^50
  // cells = mul2 * div2 >= 2^63  <=>  mul2 > floor((2^63 - 1) / div2)
  if (G.mul2 > (uint64_t)INT64_MAX / (uint64_t)G.div_b[2]) {
    G.status = kGmapCells;
    return;
  }
  const uint64_t maxk = G.mul2 * (uint64_t)G.div_b[2] - 1;
  int b = 1;
  while (b < 63 && (maxk >> b) != 0) ++b;
  G.nbits = b;
}

FBR_GMAP_HD inline uint64_t gmap_key(const GmapGrid& G, float x, float y, float z) {
  const int ijk0 = (int)(floorf(x * G.inv) - (float)G.min_b[0]);
  const int ijk1 = (int)(floorf(y * G.inv) - (float)G.min_b[1]);
  const int ijk2 = (int)(floorf(z * G.inv) - (float)G.min_b[2]);
  return (uint64_t)ijk0 + (uint64_t)ijk1 * G.mul1 + (uint64_t)ijk2 * G.mul2;
}

// The key of a point the filter drops (a non-finite coordinate): above every voxel key.
FBR_GMAP_HD inline uint64_t gmap_drop_key(const GmapGrid& G) { return (uint64_t)1 << G.nbits; }

// transformPointCloud's row order (k_kf_transform): ((T0 x + T1 y) + T2 z) + T3, intensity kept.
FBR_GMAP_HD inline void gmap_transform(const float T[12], float x, float y, float z, float* ox, float* oy, float* oz) {
  *ox = T[0] * x + T[1] * y + T[2] * z + T[3];
  *oy = T[4] * x + T[5] * y + T[6] * z + T[7];
  *oz = T[8] * x + T[9] * y + T[10] * z + T[11];
}

}  // namespace fbr
