// Host-compiled probe of csrc/fbr_reg_info.h (test infrastructure): the 6x6 Jacobi, the chart map,
// the covariance assembly and the record exactly as k_reg_info.hip compiles them, built for the CPU
// so the tests can compare them with the NumPy model (tests/info_model.py) without a GPU.
#include <stdint.h>

#include "fbr_reg_info.h"

extern "C" {

int probe_info_sweep_limit(void) { return fbr::kInfoSweeps; }

// eig[6] ascending, evec[36] rows; returns the sweeps that rotated.
int probe_info_jacobi(const double* H, double* eig, double* evec) {
  fbr::InfoWork w;
  return fbr::info_jacobi6(H, eig, evec, &w);
}

void probe_info_chart(const float* pose, double* S) { fbr::info_chart(pose, S); }

// The record of a job from its summed products acc[29] (21 H upper by rows, 6 g, the count, rss).
void probe_info_record(const double* acc, int rows_c, int rows_s, int query_c, int query_s, const float* pose, int flags,
                       double eig_floor, double unobserved, double sigma2, fbr_reg_info* out) {
  fbr::InfoWork w;
  fbr::info_record(acc, rows_c, rows_s, query_c, query_s, pose, flags, eig_floor, unobserved, sigma2, out, &w);
}

}
