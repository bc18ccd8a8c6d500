// Host-compiled probes of the device headers (test infrastructure): the same source the kernels
// use (fbr_fdlibm.h, fbr_sort.h, fbr_icp_solve.h), compiled for the CPU so the tests can compare it
// with the reference's real dependencies (glibc atan2f, libstdc++ std::sort) or a float64 model
// without a GPU.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "fbr_fdlibm.h"
#include "fbr_icp_solve.h"
#include "fbr_knobs.h"
#include "fbr_sincosf.h"
#include "fbr_sort.h"

extern "C" {

void probe_atan2f(const float* y, const float* x, float* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = fbr::fd_atan2f(y[i], x[i]);
}

// The host glibc sinf / cosf (the reference's libm) on an array.
void probe_glibc_sincosf(const float* x, float* s, float* c, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    s[i] = ::sinf(x[i]);
    c[i] = ::cosf(x[i]);
  }
}

// fbr_sincosf.h against the host glibc over every float whose bit pattern u satisfies
// lo <= u < hi with u % stride == 0 (threads split the range); returns the mismatch count.
uint64_t probe_sincosf_range(uint64_t lo, uint64_t hi, uint64_t stride, int threads) {
  std::atomic<uint64_t> bad{0};
  std::vector<std::thread> th;
  if (threads < 1) threads = 1;
  for (int t = 0; t < threads; ++t)
    th.emplace_back([&, t] {
      uint64_t b = 0;
      for (uint64_t u = lo + (uint64_t)t * stride; u < hi; u += (uint64_t)threads * stride) {
        const uint32_t ui = (uint32_t)u;
        float x;
        memcpy(&x, &ui, 4);
        const float r[4] = {::sinf(x), fbr::gl_sinf(x), ::cosf(x), fbr::gl_cosf(x)};
        uint32_t k[4];
        memcpy(k, r, sizeof(k));
        if (k[0] != k[1] && !(isnan(r[0]) && isnan(r[1]))) ++b;
        if (k[2] != k[3] && !(isnan(r[2]) && isnan(r[3]))) ++b;
      }
      bad += b;
    });
  for (auto& x : th) x.join();
  return bad;
}

// std::sort emulation on {value, index} pairs; writes the resulting index order.
void probe_sort(const float* values, int64_t n, int64_t* ind_out) {
  fbr::SmoothEntry* a = new fbr::SmoothEntry[n > 0 ? n : 1];
  for (int64_t i = 0; i < n; ++i) a[i] = fbr::SmoothEntry{values[i], (int)i};
  fbr::std_sort_emul(a, (int)n);
  for (int64_t i = 0; i < n; ++i) ind_out[i] = a[i].ind;
  delete[] a;
}

// k_icp_solve's transformation estimate (fbr_icp_solve.h) on n sets of the 17 correspondence sums:
// the row-major 3x4 float T of each.
void probe_icp_umeyama(const double* sums, float* T, int64_t n) {
  for (int64_t i = 0; i < n; ++i) fbr::icp_umeyama(sums + 17 * i, T + 12 * i);
}

// Every environment knob (fbr_knobs.h) as this process's environment gives it, in header order.
// The two cell sizes go out as 8 / metres (their inverse cell times 8), for mapping leaves of at
// least 0.3 m; the same two for smaller leaves follow the last knob.  Returns the count written.
int64_t probe_knobs(int64_t* out) {
  namespace k = fbr::knobs;
  int64_t n = 0;
  out[n++] = k::nsub(8);
  out[n++] = k::knn_tile();
  out[n++] = k::knn_tile_stats();
  out[n++] = k::vg_split();
  out[n++] = k::ingest_compact();
  out[n++] = k::copy_spin_us();
  out[n++] = k::compact_cells();
  out[n++] = k::gn_grid_cap();
  out[n++] = k::gn_one_item();
  out[n++] = k::gn_tail_one_item();
  out[n++] = k::gn_one_grid();
  out[n++] = k::packed_scans();
  out[n++] = k::feat_compact();
  out[n++] = k::feat_surf_win();
  out[n++] = k::feat_surf_window();
  out[n++] = k::owner_tags();
  out[n++] = k::owner_tmax();
  out[n++] = k::gn_tail_div();
  out[n++] = k::gn_lag();
  out[n++] = k::knn_flat();
  out[n++] = (int64_t)(8.0f * k::knn_cell_inv(true));
  out[n++] = (int64_t)(8.0f * k::knn_cell_x_inv(true));
  out[n++] = k::vg_large_min();
  out[n++] = k::vr_dbg();
  out[n++] = k::vg_inplace();
  out[n++] = k::vg_classes();
  out[n++] = k::fit_cache();
  out[n++] = k::grid_sparse();
  out[n++] = k::knn_lpq();
  out[n++] = k::feat_waves();
  out[n++] = k::direct_results();
  out[n++] = k::pinned_upload();
  out[n++] = k::stage_mb();
  out[n++] = k::stage_threads();
  out[n++] = k::ingest_xstream();
  out[n++] = k::ingest_nt();
  out[n++] = (int64_t)(8.0f * k::knn_cell_inv(false));
  out[n++] = (int64_t)(8.0f * k::knn_cell_x_inv(false));
  return n;
}

}
