// k_posegraph.hip — the pose-graph optimiser's device side (include/fbr.h "pose graph", DESIGN
// §4.10): linearisation, the block-tridiagonal factor and solve by block cyclic reduction, and the
// vector kernels of the preconditioned conjugate gradients.  All arithmetic is double and is
// fbr_pg.h's, shared with the CPU probe.
//
// k_pg_linearize: one thread per factor: whitened residual, Jacobian blocks, 1/2 |r|^2.
// k_pg_robust:    only with a robust option, after k_pg_linearize: one thread per factor turns a loop
//   factor's cost into rho and scales its linearisation by sqrt(w); k_pg_loop_report gathers the loop
//   factors' |r|^2 and weights at the end of an optimise (fbr_pg_loop_weights).
// k_pg_assemble:  one thread per node gathers its factors (host-built adjacency, factor order) into
//   T's diagonal and sub-diagonal blocks, g = J^T r and diag(H).  No atomics.
// k_pg_damp, k_pg_cr_elim, k_pg_cr_update: level 0's damped diagonal, then per level the Cholesky of
//   the eliminated (odd) nodes with their two D^-1 A blocks, and the retained (even) nodes' Schur
//   update into the next level.  One thread per node, blocks in structure-of-arrays layout.
// k_pg_cr_reduce, k_pg_cr_backsub: the solve of one right-hand side with the kept per-level blocks.
//   Levels depend on each other only across kernel boundaries.
// k_pg_cr_factor_tail, k_pg_cr_solve_tail: once a level fits one workgroup (256 nodes), that level
//   and every level after it run in one launch, a level step ending at a __syncthreads(); a graph of
//   up to 256 nodes factors in one launch and solves in one.
// k_pg_hp: q = T p + L p per node, with the workgroups' partial p . q; k_pg_dot the same for r . z.
// k_pg_alpha, k_pg_decide: one thread sums the partials in index order and takes the PCG's scalar
//   decisions, so every sum has one fixed order; k_pg_decide publishes the progress word to
//   host-mapped memory.  The kernels of an iteration enqueued past the stop return at once.
// No float or double atomics anywhere.

#include "fbr_common.h"
#include "fbr_kernels.h"
#include "fbr_pace.h"
#include "fbr_pg.h"

namespace fbr {

constexpr int kPgThreads = 64;   // block-heavy kernels: one wave per workgroup spreads a chain over the CUs
constexpr int kPgVec = 256;      // vector kernels and reductions
constexpr int kPgTail = 256;     // levels of at most this many nodes run in one workgroup (k_pg_cr_*_tail)

// The workgroup's sum of v in a fixed order (a binary tree over the thread index), valid in thread 0.
__device__ inline double pg_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int off = kPgVec / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + off];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(kPgThreads)
k_pg_linearize(PgArgs a, const double* __restrict__ X, int jac) {
  const int64_t k = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
  if (k >= a.nf) return;
  const PgFactor f = a.fac[k];
  double Xi[12], Xj[12], r[6], Ji[36], Jj[36];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    Xi[e] = X[(int64_t)f.i * 12 + e];
    Xj[e] = f.j >= 0 ? X[(int64_t)f.j * 12 + e] : 0.0;
  }
  pg_factor_eval(f, Xi, Xj, jac != 0, r, Ji, Jj);
  double c = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) c = c + r[e] * r[e];
  a.fcost[k] = 0.5 * c;
  if (!jac) return;
  double* o = a.lin + k * kPgLin;
#pragma unroll
  for (int e = 0; e < 6; ++e) o[e] = r[e];
#pragma unroll
  for (int e = 0; e < 36; ++e) {
    o[6 + e] = Ji[e];
    o[42 + e] = Jj[e];
  }
}

// After k_pg_linearize when a robust cost is asked for: one thread per factor; a loop factor's cost
// becomes rho and, with jac, its linearisation is scaled by sqrt(w) (pg_robust_factor).
__global__ void __launch_bounds__(kPgThreads)
k_pg_robust(PgArgs a, int jac) {
  const int64_t k = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
  if (k >= a.nf) return;
  pg_robust_factor(a.fac, k, a.robust, a.robust_scale, jac != 0, a.lin, a.fcost, a.chi2, a.wt);
}

// The loop factors' |r|^2 and weight of the last evaluation, gathered for one small copy to the host:
// k_pg_robust's values, or 2 fcost and 1 without a robust option.
__global__ void __launch_bounds__(kPgVec)
k_pg_loop_report(PgArgs a) {
  const int64_t l = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  if (l >= a.nloops) return;
  const int32_t f = a.loops[l];
  const bool robust = a.robust != kPgRobustNone;
  a.report[l] = robust ? a.chi2[f] : 2.0 * a.fcost[f];
  a.report[a.nloops + l] = robust ? a.wt[f] : 1.0;
}

// partial[b] = the sum of v[b * 256 ..) in tree order
__global__ void __launch_bounds__(kPgVec)
k_pg_sum_partial(const double* __restrict__ v, int64_t n, double* __restrict__ partial) {
  __shared__ double sh[kPgVec];
  const int64_t i = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  const double s = pg_block_sum(i < n ? v[i] : 0.0, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void k_pg_cost_final(PgArgs a, int nb, int slot) {
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s = s + a.partial[b];
  a.st->cost[slot] = s;
}

__global__ void __launch_bounds__(kPgThreads)
k_pg_assemble(PgArgs a) {
  const int64_t m = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
  if (m >= a.n) return;
  pg_assemble_node(a.n, m, a.fac, a.lin, a.adj_off, a.adj, a.D0, a.lev[0].A, a.g, a.hd);
}

__global__ void __launch_bounds__(kPgVec)
k_pg_damp(PgArgs a, double lambda) {
  const int64_t i = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  if (i >= 36 * a.n) return;
  const int e = (int)(i / a.n);
  const int64_t m = i - (int64_t)e * a.n;
  double d = a.D0[i];
  if (e % 7 == 0) d = d + lambda * a.hd[(int64_t)(e / 7) * a.n + m];
  a.lev[0].D[i] = d;
  if (i == 0) a.st->numerical = 0;
}

__global__ void __launch_bounds__(kPgThreads)
k_pg_cr_elim(PgLevel lv, PgState* st) {
  const int64_t t = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
  const int64_t k = lv.n == 1 ? t : 2 * t + 1;
  if (k >= lv.n) return;
  if (!pg_cr_elim(lv, k)) st->numerical = 1;
}

__global__ void __launch_bounds__(kPgThreads)
k_pg_cr_update(PgLevel lv, PgLevel nx) {
  const int64_t q = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
  if (q >= nx.n) return;
  pg_cr_update(lv, nx, q);
}

__global__ void __launch_bounds__(kPgThreads)
k_pg_cr_reduce(PgLevel lv, PgLevel nx, const PgState* st) {
  if (st->stopped) return;
  const int64_t q = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
  if (q >= nx.n) return;
  pg_cr_reduce(lv, nx, q);
}

__global__ void __launch_bounds__(kPgThreads)
k_pg_cr_backsub(PgLevel lv, PgLevel nx, const PgState* st) {
  if (st->stopped) return;
  const int64_t m = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
  if (m >= lv.n) return;
  pg_cr_backsub(lv, nx, m);
}

// The levels from l0 on, each of at most kPgTail nodes, in one workgroup: the steps of the kernels
// above in the same order, a level step ending at a __syncthreads() instead of a kernel boundary.
__global__ void __launch_bounds__(kPgTail)
k_pg_cr_factor_tail(PgArgs a, int l0) {
  bool ok = true;
  for (int l = l0; l < a.nlev; ++l) {
    const PgLevel& lv = a.lev[l];
    const int64_t k = lv.n == 1 ? (int64_t)threadIdx.x : 2 * (int64_t)threadIdx.x + 1;
    if (k < lv.n) ok = pg_cr_elim(lv, k) && ok;
    __syncthreads();
    if (l + 1 < a.nlev) {
      if ((int64_t)threadIdx.x < a.lev[l + 1].n) pg_cr_update(lv, a.lev[l + 1], threadIdx.x);
      __syncthreads();
    }
  }
  if (!ok) a.st->numerical = 1;
}

__global__ void __launch_bounds__(kPgTail)
k_pg_cr_solve_tail(PgArgs a, int l0) {
  if (a.st->stopped) return;  // (the whole workgroup)
  for (int l = l0; l + 1 < a.nlev; ++l) {
    if ((int64_t)threadIdx.x < a.lev[l + 1].n) pg_cr_reduce(a.lev[l], a.lev[l + 1], threadIdx.x);
    __syncthreads();
  }
  if (threadIdx.x == 0) pg_cr_top(a.lev[a.nlev - 1]);
  __syncthreads();
  for (int l = a.nlev - 2; l >= l0; --l) {
    if ((int64_t)threadIdx.x < a.lev[l].n) pg_cr_backsub(a.lev[l], a.lev[l + 1], threadIdx.x);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kPgVec)
k_pg_pcg_start(PgArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  if (i == 0) {
    a.st->stopped = 0;
    a.st->iters = 0;
  }
  if (i >= 6 * a.n) return;
  const double r = -a.g[i];
  a.x[i] = 0.0;
  a.r[i] = r;
  a.lev[0].b[i] = r;
}

// partial[b] = the workgroup's part of u . v, per node (its six entries in order), tree over the nodes
__global__ void __launch_bounds__(kPgVec)
k_pg_dot(PgArgs a, const double* __restrict__ u, const double* __restrict__ v) {
  __shared__ double sh[kPgVec];
  if (a.st->stopped) return;  // (the whole grid)
  const int64_t m = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  double s = 0.0;
  if (m < a.n) {
#pragma unroll
    for (int e = 0; e < 6; ++e) s = s + u[e * a.n + m] * v[e * a.n + m];
  }
  s = pg_block_sum(s, sh);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

__device__ inline void pg_publish(const PgArgs& a, unsigned long long gen) {
  __threadfence_system();
  __hip_atomic_store(a.flag, pace::pack_progress(gen, (uint32_t)a.st->iters, (unsigned)a.st->stopped), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}

// After z = M^-1 r and the partials of r . z.  first: the start of a solve (rz0; beta = 0); otherwise
// the end of iteration `it`: beta, the stop test, the progress word.
__global__ void k_pg_decide(PgArgs a, int nb, int first, int it, int max_it, double tol2, unsigned long long gen) {
  PgState* st = a.st;
  if (st->stopped) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s = s + a.partial[b];
  if (first) {
    st->rz0 = s;
    st->rz[0] = s;
    st->beta = 0.0;
    if (!(s > 0.0) || !(s < INFINITY)) st->stopped = 1;  // a zero (or broken) gradient: the step is x = 0
  } else {
    st->beta = s / st->rz[it & 1];
    st->rz[(it + 1) & 1] = s;
    st->iters = it + 1;
    if (!(s > tol2 * st->rz0) || !(s < INFINITY) || it + 1 >= max_it) st->stopped = 1;
  }
  pg_publish(a, gen);
}

// p = z + beta p (after a stop p is not read again)
__global__ void __launch_bounds__(kPgVec)
k_pg_pupdate(PgArgs a) {
  if (a.st->stopped) return;
  const int64_t i = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  if (i >= 6 * a.n) return;
  const double beta = a.st->beta;
  a.p[i] = beta == 0.0 ? a.lev[0].x[i] : a.lev[0].x[i] + beta * a.p[i];
}

__global__ void __launch_bounds__(kPgVec)
k_pg_hp(PgArgs a) {
  __shared__ double sh[kPgVec];
  if (a.st->stopped) return;
  const int64_t m = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  double s = 0.0;
  if (m < a.n) s = pg_hp_node(a.n, m, a.fac, a.lin, a.ladj_off, a.ladj, a.lev[0].D, a.lev[0].A, a.p, a.q);
  s = pg_block_sum(s, sh);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

__global__ void k_pg_alpha(PgArgs a, int nb, int it, unsigned long long gen) {
  PgState* st = a.st;
  if (st->stopped) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s = s + a.partial[b];
  st->pq = s;
  if (!(s > 0.0) || !(s < INFINITY)) {  // H is not positive definite in floating point: keep x
    st->stopped = 1;
    pg_publish(a, gen);
    return;
  }
  st->alpha = st->rz[it & 1] / s;
}

// x += alpha p, r -= alpha q, and r as the next solve's right-hand side
__global__ void __launch_bounds__(kPgVec)
k_pg_xr(PgArgs a) {
  if (a.st->stopped) return;
  const int64_t i = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  if (i >= 6 * a.n) return;
  const double alpha = a.st->alpha;
  a.x[i] = a.x[i] + alpha * a.p[i];
  const double r = a.r[i] - alpha * a.q[i];
  a.r[i] = r;
  a.lev[0].b[i] = r;
}

__global__ void __launch_bounds__(kPgVec)
k_pg_retract(PgArgs a, const double* __restrict__ X, double* __restrict__ Xt) {
  const int64_t m = (int64_t)blockIdx.x * kPgVec + threadIdx.x;
  if (m >= a.n) return;
  double P[12], d[6], Y[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) P[e] = X[m * 12 + e];
  pg_ld6(a.x, a.n, m, d);
  pg_retract(P, d, Y);
#pragma unroll
  for (int e = 0; e < 12; ++e) Xt[m * 12 + e] = Y[e];
}

static inline unsigned pg_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
// the first level that fits one workgroup (the last level has one node: there is always one)
static inline int pg_tail_level(const PgArgs& a) {
  int l = 0;
  while (a.lev[l].n > kPgTail) ++l;
  return l;
}

void launch_pg_linearize(hipStream_t s, const PgArgs& a, const double* X, int jac, int slot) {
  if (a.nf <= 0) return;
  fbr_launch(k_pg_linearize, dim3(pg_blocks(a.nf, kPgThreads)), dim3(kPgThreads), 0, s, a, X, jac);
  if (a.robust != kPgRobustNone) fbr_launch(k_pg_robust, dim3(pg_blocks(a.nf, kPgThreads)), dim3(kPgThreads), 0, s, a, jac);
  const unsigned nb = pg_blocks(a.nf, kPgVec);
  fbr_launch(k_pg_sum_partial, dim3(nb), dim3(kPgVec), 0, s, (const double*)a.fcost, a.nf, a.partial);
  fbr_launch(k_pg_cost_final, dim3(1), dim3(1), 0, s, a, (int)nb, slot);
}

void launch_pg_assemble(hipStream_t s, const PgArgs& a) {
  fbr_launch(k_pg_assemble, dim3(pg_blocks(a.n, kPgThreads)), dim3(kPgThreads), 0, s, a);
}

void launch_pg_factor(hipStream_t s, const PgArgs& a, double lambda) {
  fbr_launch(k_pg_damp, dim3(pg_blocks(36 * a.n, kPgVec)), dim3(kPgVec), 0, s, a, lambda);
  const int l0 = pg_tail_level(a);
  for (int l = 0; l < l0; ++l) {  // (a level above the tail has more than one node, and a next level)
    const PgLevel& lv = a.lev[l];
    fbr_launch(k_pg_cr_elim, dim3(pg_blocks(lv.n / 2, kPgThreads)), dim3(kPgThreads), 0, s, lv, a.st);
    fbr_launch(k_pg_cr_update, dim3(pg_blocks(a.lev[l + 1].n, kPgThreads)), dim3(kPgThreads), 0, s, lv, a.lev[l + 1]);
  }
  fbr_launch(k_pg_cr_factor_tail, dim3(1), dim3(kPgTail), 0, s, a, l0);
}

// z (level 0's x) = T^-1 (level 0's b)
static void pg_solve(hipStream_t s, const PgArgs& a) {
  const int l0 = pg_tail_level(a);
  for (int l = 0; l < l0; ++l)
    fbr_launch(k_pg_cr_reduce, dim3(pg_blocks(a.lev[l + 1].n, kPgThreads)), dim3(kPgThreads), 0, s, a.lev[l], a.lev[l + 1],
               (const PgState*)a.st);
  fbr_launch(k_pg_cr_solve_tail, dim3(1), dim3(kPgTail), 0, s, a, l0);
  for (int l = l0 - 1; l >= 0; --l)
    fbr_launch(k_pg_cr_backsub, dim3(pg_blocks(a.lev[l].n, kPgThreads)), dim3(kPgThreads), 0, s, a.lev[l], a.lev[l + 1],
               (const PgState*)a.st);
}

void launch_pg_pcg_init(hipStream_t s, const PgArgs& a, unsigned long long gen) {
  const unsigned nv = pg_blocks(6 * a.n, kPgVec), nb = pg_blocks(a.n, kPgVec);
  fbr_launch(k_pg_pcg_start, dim3(nv), dim3(kPgVec), 0, s, a);
  pg_solve(s, a);
  fbr_launch(k_pg_dot, dim3(nb), dim3(kPgVec), 0, s, a, (const double*)a.r, (const double*)a.lev[0].x);
  fbr_launch(k_pg_decide, dim3(1), dim3(1), 0, s, a, (int)nb, 1, 0, 0, 0.0, gen);
  fbr_launch(k_pg_pupdate, dim3(nv), dim3(kPgVec), 0, s, a);
}

void launch_pg_loop_report(hipStream_t s, const PgArgs& a) {
  if (a.nloops <= 0) return;
  fbr_launch(k_pg_loop_report, dim3(pg_blocks(a.nloops, kPgVec)), dim3(kPgVec), 0, s, a);
}

// k_pg_pcg_start's right-hand side -g (and a cleared stop word: the solve's kernels run), one solve
void launch_pg_direct_y(hipStream_t s, const PgArgs& a) {
  fbr_launch(k_pg_pcg_start, dim3(pg_blocks(6 * a.n, kPgVec)), dim3(kPgVec), 0, s, a);
  pg_solve(s, a);
}

void launch_pg_pcg_iter(hipStream_t s, const PgArgs& a, int it, int max_it, double tol2, unsigned long long gen) {
  const unsigned nv = pg_blocks(6 * a.n, kPgVec), nb = pg_blocks(a.n, kPgVec);
  fbr_launch(k_pg_hp, dim3(nb), dim3(kPgVec), 0, s, a);
  fbr_launch(k_pg_alpha, dim3(1), dim3(1), 0, s, a, (int)nb, it, gen);
  fbr_launch(k_pg_xr, dim3(nv), dim3(kPgVec), 0, s, a);
  pg_solve(s, a);
  fbr_launch(k_pg_dot, dim3(nb), dim3(kPgVec), 0, s, a, (const double*)a.r, (const double*)a.lev[0].x);
  fbr_launch(k_pg_decide, dim3(1), dim3(1), 0, s, a, (int)nb, 0, it, max_it, tol2, gen);
  fbr_launch(k_pg_pupdate, dim3(nv), dim3(kPgVec), 0, s, a);
}

void launch_pg_retract(hipStream_t s, const PgArgs& a, const double* X, double* Xt) {
  fbr_launch(k_pg_retract, dim3(pg_blocks(a.n, kPgVec)), dim3(kPgVec), 0, s, a, X, Xt);
}

}  // namespace fbr
