// Host-compiled probe of csrc/fbr_sc.h (test infrastructure): the scan-context bin, cell value,
// column norm and distance functions exactly as k_scancontext.hip compiles them, built for the CPU
// so the tests can compare them with the NumPy model (tests/sc_model.py) without a GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fbr_sc.h"

extern "C" {

// cell[i] = ring * n_sector + sector of point i, -1 when it is dropped.
void probe_sc_cells(const float* xyz, int64_t n, int n_ring, int n_sector, float max_radius, int32_t* cell) {
  for (int64_t i = 0; i < n; ++i)
    cell[i] = fbr::sc_cell(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], n_ring, n_sector, max_radius);
}

// The descriptor [n_ring][n_sector] of a cloud: the integer maximum of sc_value_bits per cell.
void probe_sc_descriptor(const float* xyz, int64_t n, int n_ring, int n_sector, float max_radius, float lidar_height,
                         float* desc) {
  std::vector<uint32_t> d((size_t)n_ring * n_sector, 0u);
  for (int64_t i = 0; i < n; ++i) {
    const int cell = fbr::sc_cell(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], n_ring, n_sector, max_radius);
    if (cell < 0) continue;
    const uint32_t v = fbr::sc_value_bits(xyz[3 * i + 2], lidar_height);
    if (v > d[(size_t)cell]) d[(size_t)cell] = v;
  }
  memcpy(desc, d.data(), sizeof(uint32_t) * d.size());
}

// d[s] = the distance of Q to C at every shift s < n_sector (the norms as k_sc_norms writes them).
void probe_sc_distances(const float* Q, const float* C, int n_ring, int n_sector, double* d) {
  std::vector<double> qi((size_t)n_sector), ci((size_t)n_sector);
  for (int c = 0; c < n_sector; ++c) {
    qi[(size_t)c] = fbr::sc_inverse_norm(fbr::sc_column_norm(Q, n_ring, n_sector, c));
    ci[(size_t)c] = fbr::sc_inverse_norm(fbr::sc_column_norm(C, n_ring, n_sector, c));
  }
  for (int s = 0; s < n_sector; ++s) d[s] = fbr::sc_distance(Q, qi.data(), C, ci.data(), n_ring, n_sector, s);
}

}
