// k_pg_marginals.hip — the device side of the pose graph's marginal covariances (include/fbr.h
// "marginal covariances"): Sigma_ii = P_i - Y_i^T Y_i over the cyclic-reduction factor
// of the undamped block-tridiagonal part T0 that k_posegraph.hip's launch_pg_factor(lambda = 0)
// leaves in the levels.  All arithmetic is double and is fbr_pg.h's, shared with the CPU driver
// (fbr_pg_host.h).
//
// k_pg_selinv_up, k_pg_selinv_tail: the selected inverse, one thread per node per level, walking up;
//   levels are separated by kernel boundaries, the levels of at most 256 nodes run in one workgroup.
// k_pg_mr_rhs, k_pg_mr_reduce, k_pg_mr_solve_tail, k_pg_mr_backsub: W = T0^-1 U^T, a chunk of
//   columns at a time: one thread per (node, column), NODE fastest-varying (blockIdx.y is the
//   column): the G / H / L blocks are structure-of-arrays over the nodes (X[e * n + m]), so
//   consecutive nodes read consecutive addresses, and a column is the [6][n] vector the single
//   right-hand-side steps already take.  Column-fastest would have made every block load a
//   same-address broadcast but the b / x accesses strided by 6 n.  Level 0's x is W itself.
// k_pg_marg_c: C = I + U W, one thread per entry, gathered in a fixed order.
// k_pg_chol_panel, k_pg_chol_trail: the dense Cholesky of C, blocked right-looking, 32 columns per
//   panel: the panel's diagonal block factored in LDS and the rows below it solved against it by one
//   workgroup, then the trailing update by a grid of 16 x 16 tiles over the lower triangle; a kernel
//   boundary per panel; every entry's sum in column order.  A bad pivot sets PgState::numerical, as
//   k_pg_cr_elim's does.
// k_pg_marg_forward, k_pg_marg_forward_wg, k_pg_marg_final: Y_i = Lc^-1 W_i^T in place on W's lanes
//   of the requested nodes (one thread per node and entry; for up to 1,024 lanes a workgroup per
//   lane, same bytes), then P_i - Y_i^T Y_i into the output staging buffer.
// No float or double atomics anywhere; no host synchronisation between the launches.

#include <algorithm>

#include "fbr_common.h"
#include "fbr_kernels.h"
#include "fbr_pg.h"

namespace fbr {

constexpr int kMgThreads = 64;  // block-heavy kernels, as k_posegraph.hip's
constexpr int kMgVec = 256;
constexpr int kMgTail = 256;    // levels of at most this many nodes run in one workgroup
constexpr int kMgTile = 16;     // the trailing update's tile edge
constexpr int kMgFewLanes = 1024;  // up to this many (node, entry) lanes of Y get a workgroup each
static_assert(kMgTile * kMgTile == kMgVec && 2 * kMgVec == kMgTile * kPgPanel, "the trailing update's tile loads");

__global__ void __launch_bounds__(kMgThreads)
k_pg_selinv_up(PgMarg a, int l) {
  const int64_t m = (int64_t)blockIdx.x * kMgThreads + threadIdx.x;
  if (m >= a.lev[l].n) return;
  pg_selinv_up(a.lev[l], a.P[l + 1], a.Q[l + 1], a.lev[l + 1].n, a.P[l], a.Q[l], m);
}

// The last level's node, then the levels down to l0, each of at most kMgTail nodes.
__global__ void __launch_bounds__(kMgTail)
k_pg_selinv_tail(PgMarg a, int l0) {
  if (threadIdx.x == 0) pg_selinv_top(a.lev[a.nlev - 1], a.P[a.nlev - 1]);
  __syncthreads();
  for (int l = a.nlev - 2; l >= l0; --l) {
    if ((int64_t)threadIdx.x < a.lev[l].n)
      pg_selinv_up(a.lev[l], a.P[l + 1], a.Q[l + 1], a.lev[l + 1].n, a.P[l], a.Q[l], threadIdx.x);
    __syncthreads();
  }
}

// Level 0's b of columns [c0, c0 + nc): every entry written, zero away from the factor's two nodes.
__global__ void __launch_bounds__(kMgVec)
k_pg_mr_rhs(PgMarg a, int64_t c0, int64_t nc) {
  const int64_t t = (int64_t)blockIdx.x * kMgVec + threadIdx.x;
  if (t >= nc * 6 * a.n) return;
  const int64_t ce = t / a.n, m = t - ce * a.n, cc = ce / 6, col = c0 + cc;
  const int e = (int)(ce - cc * 6), r = (int)(col % 6);
  const int32_t fk = a.loops[col / 6];
  double v = 0.0;
  if (m == a.fac[fk].i) v = pg_marg_rhs_entry(a.lin, fk, r, 0, e);
  else if (m == a.fac[fk].j) v = pg_marg_rhs_entry(a.lin, fk, r, 1, e);
  a.lev[0].b[t] = v;
}

__global__ void __launch_bounds__(kMgThreads)
k_pg_mr_reduce(PgMarg a, int l) {
  const int64_t q = (int64_t)blockIdx.x * kMgThreads + threadIdx.x;
  if (q >= a.lev[l + 1].n) return;
  pg_cr_reduce_col(a.lev[l], a.lev[l + 1], q, blockIdx.y);
}

__global__ void __launch_bounds__(kMgThreads)
k_pg_mr_backsub(PgMarg a, int l) {
  const int64_t m = (int64_t)blockIdx.x * kMgThreads + threadIdx.x;
  if (m >= a.lev[l].n) return;
  pg_cr_backsub_col(a.lev[l], a.lev[l + 1], m, blockIdx.y);
}

// Column blockIdx.x through the levels from l0 on, as k_pg_cr_solve_tail.
__global__ void __launch_bounds__(kMgTail)
k_pg_mr_solve_tail(PgMarg a, int l0) {
  const int64_t c = blockIdx.x;
  for (int l = l0; l + 1 < a.nlev; ++l) {
    if ((int64_t)threadIdx.x < a.lev[l + 1].n) pg_cr_reduce_col(a.lev[l], a.lev[l + 1], threadIdx.x, c);
    __syncthreads();
  }
  if (threadIdx.x == 0) pg_cr_top_col(a.lev[a.nlev - 1], c);
  __syncthreads();
  for (int l = a.nlev - 2; l >= l0; --l) {
    if ((int64_t)threadIdx.x < a.lev[l].n) pg_cr_backsub_col(a.lev[l], a.lev[l + 1], threadIdx.x, c);
    __syncthreads();
  }
}

// Row fastest-varying: the threads of a wave share the column and read a few nodes' entries of it.
__global__ void __launch_bounds__(kMgVec)
k_pg_marg_c(PgMarg a) {
  const int64_t t = (int64_t)blockIdx.x * kMgVec + threadIdx.x;
  if (t >= a.M * a.M) return;
  const int64_t col = t / a.M, row = t - col * a.M;
  a.C[row * a.M + col] = pg_marg_c_entry(a.fac, a.lin, a.loops, a.W, a.n, row, col);
}

// Panel [j0, j0 + nb) of C: the diagonal block in LDS (pg_dense_chol_block's operations, an entry's
// updates in the same column order), written back, then the rows below solved against it.
__global__ void __launch_bounds__(kMgVec)
k_pg_chol_panel(double* __restrict__ C, int64_t M, int64_t j0, PgState* st) {
  __shared__ double sA[kPgPanel][kPgPanel + 1];
  const int nb = (int)(M - j0 < kPgPanel ? M - j0 : kPgPanel);
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kPgPanel * kPgPanel; idx += kMgVec) {
    const int r = idx / kPgPanel, c = idx % kPgPanel;
    sA[r][c] = (r < nb && c <= r) ? C[(j0 + r) * M + j0 + c] : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    if (tid == 0) {
      double d = sA[j][j];
      if (!(d > 0.0) || !(d < INFINITY)) {
        st->numerical = 1;
        d = 1.0;
      }
      sA[j][j] = sqrt(d);
    }
    __syncthreads();
    if (tid > j && tid < nb) sA[tid][j] = sA[tid][j] / sA[j][j];
    __syncthreads();
    for (int idx = tid; idx < kPgPanel * kPgPanel; idx += kMgVec) {
      const int i = idx / kPgPanel, k = idx % kPgPanel;
      if (i > j && i < nb && k > j && k <= i) sA[i][k] = sA[i][k] - sA[i][j] * sA[k][j];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kPgPanel * kPgPanel; idx += kMgVec) {
    const int r = idx / kPgPanel, c = idx % kPgPanel;
    if (r < nb && c <= r) C[(j0 + r) * M + j0 + c] = sA[r][c];
  }
  for (int64_t i = j0 + nb + tid; i < M; i += kMgVec) pg_dense_panel_row(C, M, j0, nb, &sA[0][0], kPgPanel + 1, i);
}

// C[i][j] -= sum_k C[i][j0 + k] C[j][j0 + k] for j1 <= j <= i < M, j1 = j0 + nb: a 16 x 16 tile per
// workgroup, its rows' and columns' panel entries staged in LDS (zero past nb: the sum is the same).
__global__ void __launch_bounds__(kMgVec)
k_pg_chol_trail(double* __restrict__ C, int64_t M, int64_t j0, int nb) {
  if (blockIdx.x > blockIdx.y) return;  // a tile above the diagonal (the whole workgroup)
  __shared__ double sI[kMgTile][kPgPanel + 1], sJ[kMgTile][kPgPanel + 1];
  const int64_t j1 = j0 + nb, i0 = j1 + (int64_t)blockIdx.y * kMgTile, c0 = j1 + (int64_t)blockIdx.x * kMgTile;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kMgTile * kPgPanel; idx += kMgVec) {
    const int r = idx / kPgPanel, k = idx % kPgPanel;
    sI[r][k] = (i0 + r < M && k < nb) ? C[(i0 + r) * M + j0 + k] : 0.0;
    sJ[r][k] = (c0 + r < M && k < nb) ? C[(c0 + r) * M + j0 + k] : 0.0;
  }
  __syncthreads();
  const int ty = tid / kMgTile, tx = tid % kMgTile;
  const int64_t i = i0 + ty, j = c0 + tx;
  if (i >= M || j > i) return;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kPgPanel; ++k) s = s + sI[ty][k] * sJ[tx][k];
  C[i * M + j] = C[i * M + j] - s;
}

__global__ void __launch_bounds__(kMgThreads)
k_pg_marg_forward(PgMarg a, const int64_t* __restrict__ uniq, int64_t n_uniq) {
  const int64_t t = (int64_t)blockIdx.x * kMgThreads + threadIdx.x;
  if (t >= 6 * n_uniq) return;
  const int e = (int)(t / n_uniq);
  const int64_t u = t - (int64_t)e * n_uniq;
  pg_marg_forward(a.C, a.M, a.W, a.n, uniq ? uniq[u] : u, e);
}

// The same substitution for a few lanes (the gate asks for one node): a workgroup per lane, the rows
// spread over its threads (row r belongs to thread r % 256), column by column: the owner of row k
// finishes y[k] and hands it over through LDS (two slots, so a step needs one barrier), then every
// thread subtracts C[r][k] y[k] from its rows below.  A row's terms come in the column order of
// pg_marg_forward, so the bytes are the same.
__global__ void __launch_bounds__(kMgVec)
k_pg_marg_forward_wg(PgMarg a, const int64_t* __restrict__ uniq, int64_t n_uniq) {
  __shared__ double sy[2];
  const int e = (int)(blockIdx.x / n_uniq);
  const int64_t u = blockIdx.x - (int64_t)e * n_uniq, i = uniq ? uniq[u] : u, st = 6 * a.n;
  double* y = a.W + (int64_t)e * a.n + i;
  const int tid = threadIdx.x;
  for (int64_t k = 0; k < a.M; ++k) {
    if (tid == (int)(k % kMgVec)) {
      const double v = y[k * st] / a.C[k * a.M + k];
      y[k * st] = v;
      sy[k & 1] = v;
    }
    __syncthreads();
    const double yk = sy[k & 1];
    const int64_t r0 = k + 1;
    for (int64_t r = r0 + (tid - (int)(r0 % kMgVec) + kMgVec) % kMgVec; r < a.M; r += kMgVec)
      y[r * st] = y[r * st] - a.C[r * a.M + k] * yk;
  }
}

__global__ void __launch_bounds__(kMgThreads)
k_pg_marg_final(PgMarg a, const int64_t* __restrict__ nodes, int64_t n_out, double* __restrict__ out) {
  const int64_t o = (int64_t)blockIdx.x * kMgThreads + threadIdx.x;
  if (o >= n_out) return;
  double cov[36];
  pg_marg_final(a.P[0], a.W, a.M, a.n, nodes ? nodes[o] : o, cov);
#pragma unroll
  for (int k = 0; k < 36; ++k) out[o * 36 + k] = cov[k];
}

static inline unsigned mg_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
static inline int mg_tail_level(const PgMarg& a) {
  int l = 0;
  while (a.lev[l].n > kMgTail) ++l;
  return l;
}

void launch_pg_selinv(hipStream_t s, const PgMarg& a) {
  const int l0 = mg_tail_level(a);
  fbr_launch(k_pg_selinv_tail, dim3(1), dim3(kMgTail), 0, s, a, l0);
  for (int l = l0 - 1; l >= 0; --l)
    fbr_launch(k_pg_selinv_up, dim3(mg_blocks(a.lev[l].n, kMgThreads)), dim3(kMgThreads), 0, s, a, l);
}

void launch_pg_marg_solve(hipStream_t s, const PgMarg& a0, int64_t c0, int64_t nc) {
  if (nc <= 0) return;
  PgMarg a = a0;
  a.lev[0].x = a0.W + c0 * 6 * a0.n;  // the chunk's columns of W
  const unsigned cols = (unsigned)nc;
  const int l0 = mg_tail_level(a);
  fbr_launch(k_pg_mr_rhs, dim3(mg_blocks(nc * 6 * a.n, kMgVec)), dim3(kMgVec), 0, s, a, c0, nc);
  for (int l = 0; l < l0; ++l)
    fbr_launch(k_pg_mr_reduce, dim3(mg_blocks(a.lev[l + 1].n, kMgThreads), cols), dim3(kMgThreads), 0, s, a, l);
  fbr_launch(k_pg_mr_solve_tail, dim3(cols), dim3(kMgTail), 0, s, a, l0);
  for (int l = l0 - 1; l >= 0; --l)
    fbr_launch(k_pg_mr_backsub, dim3(mg_blocks(a.lev[l].n, kMgThreads), cols), dim3(kMgThreads), 0, s, a, l);
}

void launch_pg_marg_c(hipStream_t s, const PgMarg& a) {
  if (a.M <= 0) return;
  fbr_launch(k_pg_marg_c, dim3(mg_blocks(a.M * a.M, kMgVec)), dim3(kMgVec), 0, s, a);
}

void launch_pg_marg_chol(hipStream_t s, const PgMarg& a) {
  for (int64_t j0 = 0; j0 < a.M; j0 += kPgPanel) {
    const int nb = (int)std::min<int64_t>(kPgPanel, a.M - j0);
    fbr_launch(k_pg_chol_panel, dim3(1), dim3(kMgVec), 0, s, a.C, a.M, j0, a.st);
    const unsigned nt = mg_blocks(a.M - j0 - nb, kMgTile);
    if (nt) fbr_launch(k_pg_chol_trail, dim3(nt, nt), dim3(kMgVec), 0, s, a.C, a.M, j0, nb);
  }
}

void launch_pg_marg_cov(hipStream_t s, const PgMarg& a, const int64_t* uniq, int64_t n_uniq, const int64_t* nodes,
                        int64_t n_out, double* out) {
  if (n_out <= 0) return;
  if (a.M > 0 && 6 * n_uniq <= kMgFewLanes)
    fbr_launch(k_pg_marg_forward_wg, dim3((unsigned)(6 * n_uniq)), dim3(kMgVec), 0, s, a, uniq, n_uniq);
  else if (a.M > 0)
    fbr_launch(k_pg_marg_forward, dim3(mg_blocks(6 * n_uniq, kMgThreads)), dim3(kMgThreads), 0, s, a, uniq, n_uniq);
  fbr_launch(k_pg_marg_final, dim3(mg_blocks(n_out, kMgThreads)), dim3(kMgThreads), 0, s, a, nodes, n_out, out);
}

}  // namespace fbr
