// k_pg_direct.hip — the last three steps of the pose graph's direct solve (include/fbr.h "direct
// solve"): with y = T^-1 (-g) from k_posegraph.hip's cyclic-reduction solve and W, C =
// Lc Lc^T from k_pg_marginals.hip's launchers on the damped factor, the Woodbury step
// delta = y - W (Lc Lc^T)^-1 U y.  All arithmetic is double and is fbr_pg.h's, shared with the CPU
// driver (fbr_pg_host.h).
//
// k_pg_direct_z:     z = U y, one thread per row of U (a loop factor's J_i row, then its J_j row).
// k_pg_direct_subst: Lc Lc^T s = z in place, one workgroup sweeping the columns: row r belongs to
//   thread r % 256 in both passes, so an entry of z is only ever touched by one thread; the owner of
//   row k finishes z[k] and hands it over through LDS (two slots, one barrier per column), then every
//   thread takes Lc[r][k] z[k] (forwards) or Lc[k][r] z[k] (backwards) out of its rows.  An entry's
//   terms come in pg_dense_subst's order.  No workgroup waits on another.
// k_pg_direct_delta: x = y - W s, one thread per (tangent entry, node), node fastest-varying, so the
//   loads from W's [6][n] columns coalesce; the sum over the columns in ascending order.
// No float or double atomics; no host synchronisation between the launches.

#include "fbr_common.h"
#include "fbr_kernels.h"
#include "fbr_pg.h"

namespace fbr {

constexpr int kDrVec = 256;

__global__ void __launch_bounds__(kDrVec)
k_pg_direct_z(PgDirect d) {
  const int64_t row = (int64_t)blockIdx.x * kDrVec + threadIdx.x;
  if (row >= d.M) return;
  d.z[row] = pg_direct_z_entry(d.fac, d.lin, d.loops, d.y, d.n, row);
}

__global__ void __launch_bounds__(kDrVec)
k_pg_direct_subst(PgDirect d) {
  __shared__ double sz[2];
  const int tid = threadIdx.x;
  const int64_t M = d.M;
  const double* __restrict__ C = d.C;
  double* z = d.z;
  for (int64_t k = 0; k < M; ++k) {
    if (tid == (int)(k % kDrVec)) {
      const double v = pg_subst_pivot(z[k], C[k * M + k]);
      z[k] = v;
      sz[k & 1] = v;
    }
    __syncthreads();
    const double zk = sz[k & 1];
    const int64_t r0 = k + 1;
    for (int64_t r = r0 + (tid - (int)(r0 % kDrVec) + kDrVec) % kDrVec; r < M; r += kDrVec)
      z[r] = pg_subst_sub(z[r], C[r * M + k], zk);
  }
  __syncthreads();  // the forward pass's last slot is the backward pass's first
  for (int64_t k = M - 1; k >= 0; --k) {
    if (tid == (int)(k % kDrVec)) {
      const double v = pg_subst_pivot(z[k], C[k * M + k]);
      z[k] = v;
      sz[k & 1] = v;
    }
    __syncthreads();
    const double zk = sz[k & 1];
    for (int64_t r = tid; r < k; r += kDrVec) z[r] = pg_subst_sub(z[r], C[k * M + r], zk);
  }
}

__global__ void __launch_bounds__(kDrVec)
k_pg_direct_delta(PgDirect d) {
  const int64_t t = (int64_t)blockIdx.x * kDrVec + threadIdx.x;
  if (t >= 6 * d.n) return;
  d.x[t] = pg_direct_delta_entry(d.y, d.W, d.z, d.M, d.n, t);
}

static inline unsigned dr_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

void launch_pg_direct_z(hipStream_t s, const PgDirect& d) {
  if (d.M <= 0) return;
  fbr_launch(k_pg_direct_z, dim3(dr_blocks(d.M, kDrVec)), dim3(kDrVec), 0, s, d);
}

void launch_pg_direct_subst(hipStream_t s, const PgDirect& d) {
  if (d.M <= 0) return;
  fbr_launch(k_pg_direct_subst, dim3(1), dim3(kDrVec), 0, s, d);
}

void launch_pg_direct_delta(hipStream_t s, const PgDirect& d) {
  fbr_launch(k_pg_direct_delta, dim3(dr_blocks(6 * d.n, kDrVec)), dim3(kDrVec), 0, s, d);
}

}  // namespace fbr
