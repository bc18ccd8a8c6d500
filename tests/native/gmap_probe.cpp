// Host-compiled probe of csrc/fbr_gmap.h (test infrastructure): the wide VoxelGrid's grid and key
// functions exactly as k_gmap.hip compiles them, built for the CPU so the tests can compare them
// with the NumPy model (tests/gmap_model.py) without a GPU.
#include <float.h>
#include <stdint.h>
#include <string.h>

#include "fbr_gmap.h"

namespace {

// getMinMax3D over the points with finite x, y, z (k_gmw_bounds' comparisons); false when there is none.
bool bounds(const float* xyzi, int64_t n, float mn[3], float mx[3]) {
  bool any = false;
  for (int d = 0; d < 3; ++d) {
    mn[d] = FLT_MAX;
    mx[d] = -FLT_MAX;
  }
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyzi + 4 * i;
    if (!(fbr::gmap_finite(p[0]) && fbr::gmap_finite(p[1]) && fbr::gmap_finite(p[2]))) continue;
    any = true;
    for (int d = 0; d < 3; ++d) {
      mn[d] = (p[d] < mn[d]) ? p[d] : mn[d];
      mx[d] = (mx[d] < p[d]) ? p[d] : mx[d];
    }
  }
  return any;
}

// out[13]: inv (bits), min_b[3], max_b[3], div_b[3], pcl_overflow, status, nbits; mul[2]: mul1, mul2
void pack(const fbr::GmapGrid& G, int32_t* out, uint64_t* mul) {
  memcpy(&out[0], &G.inv, 4);
  for (int d = 0; d < 3; ++d) {
    out[1 + d] = G.min_b[d];
    out[4 + d] = G.max_b[d];
    out[7 + d] = G.div_b[d];
  }
  out[10] = G.pcl_overflow;
  out[11] = G.status;
  out[12] = G.nbits;
  mul[0] = G.mul1;
  mul[1] = G.mul2;
}

}  // namespace

extern "C" {

void probe_gmap_grid_box(const float* mn, const float* mx, float leaf, int32_t* out, uint64_t* mul) {
  fbr::GmapGrid G;
  fbr::gmap_grid_init(G, mn, mx, leaf);
  pack(G, out, mul);
}

// The grid of a cloud of n (x, y, z, intensity) points; returns 0 when no point is finite.
int probe_gmap_grid(const float* xyzi, int64_t n, float leaf, int32_t* out, uint64_t* mul) {
  float mn[3], mx[3];
  if (!bounds(xyzi, n, mn, mx)) return 0;
  probe_gmap_grid_box(mn, mx, leaf, out, mul);
  return 1;
}

// keys[i] of every point (the drop key for a non-finite one); returns the grid's status, -1 when
// no point is finite.
int probe_gmap_keys(const float* xyzi, int64_t n, float leaf, uint64_t* keys) {
  float mn[3], mx[3];
  if (!bounds(xyzi, n, mn, mx)) return -1;
  fbr::GmapGrid G;
  fbr::gmap_grid_init(G, mn, mx, leaf);
  if (G.status != fbr::kGmapOk) return G.status;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyzi + 4 * i;
    const bool fin = fbr::gmap_finite(p[0]) && fbr::gmap_finite(p[1]) && fbr::gmap_finite(p[2]);
    keys[i] = fin ? fbr::gmap_key(G, p[0], p[1], p[2]) : fbr::gmap_drop_key(G);
  }
  return 0;
}

// transformPointCloud's row arithmetic on n points (T: row-major 3x4), intensity kept.
void probe_gmap_transform(const float* T, const float* xyzi, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) {
    fbr::gmap_transform(T, xyzi[4 * i], xyzi[4 * i + 1], xyzi[4 * i + 2], &out[4 * i], &out[4 * i + 1], &out[4 * i + 2]);
    out[4 * i + 3] = xyzi[4 * i + 3];
  }
}

}
