// Host-compiled probe of the pose graph's direct solve and robust loop factors (test
// infrastructure): csrc/fbr_pg_host.h's drivers over csrc/fbr_pg.h's per-entry arithmetic, exactly
// as k_pg_direct.hip and k_posegraph.hip compile it, built for the CPU so the tests can compare it
// with the NumPy model (tests/pg_loops_model.py) without a GPU.
#include "fbr_pg_host.h"

using namespace fbr;

extern "C" {

int probe_pg_loops_factor_bytes() { return (int)sizeof(PgFactor); }

void probe_pg_robust(int kind, double k, double s, double* rho, double* w) { pg_robust(kind, k, s, rho, w); }

// pg_direct_lm_host: par = {max_iterations, rel_cost_tol, abs_cost_tol, lambda_init, lambda_factor,
// lambda_max}; info = {status, iterations, trials, cost_initial, cost_final, lambda}; chi2, w [nf].
int probe_pg_direct_optimize(int64_t n, const double* euler0, int64_t nf, const PgFactor* fac, const double* par,
                             int rhs_chunk, int robust, double robust_scale, double* poses_out, double* info, double* chi2,
                             double* w) {
  return pg_direct_lm_host(n, euler0, nf, fac, par, rhs_chunk, robust, robust_scale, poses_out, info, chi2, w);
}

// One direct step at the poses euler with damping lambda: delta [n][6].  0 ok, 3 a bad pivot.
int probe_pg_direct_step(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, double lambda, int rhs_chunk,
                         int robust, double robust_scale, double* delta) {
  return pg_direct_step_host(n, euler, nf, fac, lambda, rhs_chunk, robust, robust_scale, delta);
}

// The same step, and the damped system it solved as dense arrays, node-major: g [6n] as assembled,
// H [6n][6n] = the damped block-tridiagonal T from the assembled blocks plus U^T U from the loop
// factors' linearisation (their 6x6 products summed in factor order).
int probe_pg_direct_system(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, double lambda, int robust,
                           double robust_scale, double* delta, double* H, double* g) {
  PgHostDirect S(n, nf, fac, 0, robust, robust_scale);
  if (!S.graph_ok) return -1;
  std::vector<double> X((size_t)(12 * n));
  for (int64_t i = 0; i < n; ++i) pg_pose_from_euler(euler + 6 * i, &X[12 * i]);
  (void)S.evaluate(X.data(), true);
  const bool ok = S.step(lambda);
  const int64_t N = 6 * n;
  std::fill(H, H + N * N, 0.0);
  const PgLevel& l0 = S.LV.lev[0];
  for (int64_t m = 0; m < n; ++m) {
    pg_ld6(S.x.data(), n, m, delta + 6 * m);
    pg_ld6(S.g.data(), n, m, g + 6 * m);
    double D[36], A[36];
    pg_ld36(l0.D, n, m, D);
    pg_ld36(l0.A, n, m, A);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        H[(6 * m + r) * N + 6 * m + c] = D[6 * r + c];
        if (m >= 1) H[(6 * m + r) * N + 6 * (m - 1) + c] = H[(6 * (m - 1) + c) * N + 6 * m + r] = A[6 * r + c];
      }
  }
  for (int32_t fk : S.loops) {
    const double* J[2] = {&S.lin[kPgLin * fk + 6], &S.lin[kPgLin * fk + 42]};
    const int64_t node[2] = {fac[fk].i, fac[fk].j};
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) {
            double s = 0.0;
            for (int q = 0; q < 6; ++q) s = s + J[a][6 * q + r] * J[b][6 * q + c];
            H[(6 * node[a] + r) * N + 6 * node[b] + c] += s;
          }
  }
  return ok ? 0 : 3;
}

// pg_marginals_host with the loop factors' robust weights at the poses.
int probe_pg_marginals_robust(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, int rhs_chunk, int robust,
                              double robust_scale, double* cov) {
  return pg_marginals_host(n, euler, nf, fac, nullptr, 0, rhs_chunk, cov, robust, robust_scale);
}

}
