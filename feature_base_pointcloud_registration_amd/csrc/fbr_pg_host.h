// fbr_pg_host.h — the marginal covariances of include/fbr.h ("marginal covariances") and the
// Levenberg-Marquardt with the direct solve and the robust loop factors ("direct solve", "robust loop
// factors") on the host: fbr_pg.h's per-node steps in plain loops, in the order fbr_pg.hip enqueues
// the kernels of k_pg_marginals.hip, k_pg_direct.hip and k_posegraph.hip.  Host-only and free of HIP
// headers: tests/native/pg_marg_probe.cpp and pg_loops_probe.cpp load it into the tests,
// tests/native/pg_marg_check.cpp and pg_loops_check.cpp run it under the host sanitizers.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "fbr_pg.h"

namespace fbr {

struct PgHostLevels {  // the levels of an n-node system over one allocation; b and x hold `cols` columns
  std::vector<double> mem;
  std::vector<PgLevel> lev;
  PgHostLevels(int64_t n, int64_t cols) {
    int64_t tot = 0;
    const int nl = pg_cr_levels(n, &tot);
    mem.assign((size_t)(tot * (36 * 5 + 12 * cols)), 0.0);
    double* w = mem.data();
    int64_t ln = n;
    for (int l = 0; l < nl; ++l, ln = (ln + 1) / 2) {
      PgLevel v;
      v.n = ln;
      v.D = w; w += 36 * ln;
      v.A = w; w += 36 * ln;
      v.L = w; w += 36 * ln;
      v.G = w; w += 36 * ln;
      v.H = w; w += 36 * ln;
      v.b = w; w += 6 * ln * cols;
      v.x = w; w += 6 * ln * cols;
      lev.push_back(v);
    }
  }
};

// W = T^-1 U^T [M][6][n] with the factor in lev, `chunk` columns per pass (launch_pg_marg_solve);
// column cc of a pass uses column cc of the levels' b and x.
inline void pg_host_w(std::vector<PgLevel>& lev, int64_t n, int64_t M, int64_t chunk, const int32_t* loops,
                      const PgFactor* fac, const double* lin, double* W) {
  const size_t nl = lev.size();
  for (int64_t c0 = 0; c0 < M; c0 += chunk) {
    const int64_t nc = std::min(chunk, M - c0);
    std::fill(lev[0].b, lev[0].b + 6 * n * nc, 0.0);
    for (int64_t cc = 0; cc < nc; ++cc) {
      const int64_t col = c0 + cc;
      const int32_t fk = loops[col / 6];
      const int r = (int)(col % 6);
      for (int side = 0; side < 2; ++side) {
        const int64_t node = side ? fac[fk].j : fac[fk].i;
        for (int e = 0; e < 6; ++e) lev[0].b[(cc * 6 + e) * n + node] = pg_marg_rhs_entry(lin, fk, r, side, e);
      }
    }
    for (int64_t cc = 0; cc < nc; ++cc) {
      for (size_t l = 0; l + 1 < nl; ++l)
        for (int64_t q = 0; q < lev[l + 1].n; ++q) pg_cr_reduce_col(lev[l], lev[l + 1], q, cc);
      pg_cr_top_col(lev[nl - 1], cc);
      for (size_t l = nl - 1; l-- > 0;)
        for (int64_t m = 0; m < lev[l].n; ++m) pg_cr_backsub_col(lev[l], lev[l + 1], m, cc);
    }
    memcpy(W + c0 * 6 * n, lev[0].x, sizeof(double) * 6 * n * nc);
  }
}

// C = I + U W [M][M] and its Cholesky factor in place (launch_pg_marg_c, launch_pg_marg_chol);
// false on a bad pivot.
inline bool pg_host_c_chol(int64_t n, int64_t M, const int32_t* loops, const PgFactor* fac, const double* lin,
                           const double* W, double* C) {
  bool ok = true;
  for (int64_t r = 0; r < M; ++r)
    for (int64_t c = 0; c < M; ++c) C[r * M + c] = pg_marg_c_entry(fac, lin, loops, W, n, r, c);
  for (int64_t j0 = 0; j0 < M; j0 += kPgPanel) {
    const int nb = (int)std::min<int64_t>(kPgPanel, M - j0);
    ok = pg_dense_chol_block(&C[j0 * M + j0], M, nb) && ok;
    for (int64_t i = j0 + nb; i < M; ++i) pg_dense_panel_row(C, M, j0, nb, &C[j0 * M + j0], M, i);
    for (int64_t i = j0 + nb; i < M; ++i)
      for (int64_t j = j0 + nb; j <= i; ++j) pg_dense_trail_entry(C, M, j0, nb, i, j);
  }
  return ok;
}

// The factors at the poses X [n][12], as launch_pg_linearize: fcost [nf], with jac lin [nf][kPgLin],
// and with a robust option the loop factors re-weighted and chi2, wt [nf] written.  Returns the cost.
inline double pg_host_evaluate(int64_t nf, const PgFactor* fac, const double* X, bool jac, int robust, double scale,
                               double* lin, double* fcost, double* chi2, double* wt) {
  for (int64_t k = 0; k < nf; ++k) {
    double r[6], Ji[36], Jj[36], zero[12] = {0};
    pg_factor_eval(fac[k], X + 12 * fac[k].i, fac[k].j >= 0 ? X + 12 * fac[k].j : zero, jac, r, Ji, Jj);
    double c = 0.0;
    for (int e = 0; e < 6; ++e) c = c + r[e] * r[e];
    fcost[k] = 0.5 * c;
    if (jac) {
      double* o = lin + kPgLin * k;
      memcpy(o, r, sizeof(r));
      memcpy(o + 6, Ji, sizeof(Ji));
      memcpy(o + 42, Jj, sizeof(Jj));
    }
  }
  if (robust != kPgRobustNone)
    for (int64_t k = 0; k < nf; ++k) pg_robust_factor(fac, k, robust, scale, jac, lin, fcost, chi2, wt);
  double cost = 0.0;
  for (int64_t k = 0; k < nf; ++k) cost = cost + fcost[k];
  return cost;
}

// Sigma_ii of the nodes `nodes` (null: every node in order, n_out = n) at the poses euler [n][6],
// into cov [n_out][36].  rhs_chunk <= 0: every column in one pass.  Returns 0 (FBR_PG_CONVERGED),
// 3 (FBR_PG_NUMERICAL: a bad pivot of T0 or of C; cov is zeroed), -1 for a node no factor touches
// or a node index out of range.  robust, robust_scale: the loop factors carry their weights at these
// poses (fbr_pg_marginals after a robust optimise).
inline int pg_marginals_host(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, const int64_t* nodes,
                             int64_t n_out, int rhs_chunk, double* cov, int robust = kPgRobustNone,
                             double robust_scale = 0.0) {
  if (!nodes) n_out = n;
  for (int64_t o = 0; nodes && o < n_out; ++o)
    if (nodes[o] < 0 || nodes[o] >= n) return -1;
  std::vector<int32_t> off((size_t)n + 1, 0), loops;
  for (int64_t k = 0; k < nf; ++k) {
    ++off[fac[k].i + 1];
    if (fac[k].j >= 0) ++off[fac[k].j + 1];
    if (fac[k].loop) loops.push_back((int32_t)k);
  }
  for (int64_t m = 0; m < n; ++m) {
    if (off[m + 1] == 0) return -1;
    off[m + 1] += off[m];
  }
  std::vector<int32_t> adj((size_t)off[n]), cur(off.begin(), off.end() - 1);
  for (int64_t k = 0; k < nf; ++k) {
    adj[cur[fac[k].i]++] = (int32_t)(2 * k);
    if (fac[k].j >= 0) adj[cur[fac[k].j]++] = (int32_t)(2 * k + 1);
  }
  const int64_t K = (int64_t)loops.size(), M = 6 * K;
  const int64_t chunk = rhs_chunk > 0 ? std::min<int64_t>(rhs_chunk, std::max<int64_t>(M, 1)) : std::max<int64_t>(M, 1);
  // linearise at the poses, assemble the undamped T0, factor it
  std::vector<double> X((size_t)(12 * n)), lin((size_t)(kPgLin * nf)), D0((size_t)(36 * n)), hd((size_t)(6 * n)),
      g((size_t)(6 * n));
  for (int64_t i = 0; i < n; ++i) pg_pose_from_euler(euler + 6 * i, &X[12 * i]);
  {
    std::vector<double> fcost((size_t)nf), chi2((size_t)nf), wt((size_t)nf);
    (void)pg_host_evaluate(nf, fac, X.data(), true, robust, robust_scale, lin.data(), fcost.data(), chi2.data(), wt.data());
  }
  PgHostLevels LV(n, chunk);
  std::vector<PgLevel>& lev = LV.lev;
  const size_t nl = lev.size();
  for (int64_t m = 0; m < n; ++m)
    pg_assemble_node(n, m, fac, lin.data(), off.data(), adj.data(), D0.data(), lev[0].A, g.data(), hd.data());
  memcpy(lev[0].D, D0.data(), sizeof(double) * 36 * n);
  bool ok = true;
  for (size_t l = 0; l < nl; ++l) {
    for (int64_t k = 0; k < lev[l].n; ++k)
      if (pg_cr_is_elim(lev[l].n, k)) ok = pg_cr_elim(lev[l], k) && ok;
    if (l + 1 < nl)
      for (int64_t q = 0; q < lev[l + 1].n; ++q) pg_cr_update(lev[l], lev[l + 1], q);
  }
  // selected inversion, walking up
  std::vector<std::vector<double>> P(nl), Q(nl);
  for (size_t l = 0; l < nl; ++l) {
    P[l].assign((size_t)(36 * lev[l].n), 0.0);
    Q[l].assign((size_t)(36 * lev[l].n), 0.0);
  }
  pg_selinv_top(lev[nl - 1], P[nl - 1].data());
  for (size_t l = nl - 1; l-- > 0;)
    for (int64_t m = 0; m < lev[l].n; ++m)
      pg_selinv_up(lev[l], P[l + 1].data(), Q[l + 1].data(), lev[l + 1].n, P[l].data(), Q[l].data(), m);
  // W = T0^-1 U^T, `chunk` columns per pass
  std::vector<double> W((size_t)(std::max<int64_t>(M, 1) * 6 * n), 0.0), C((size_t)(M * M), 0.0);
  pg_host_w(lev, n, M, chunk, loops.data(), fac, lin.data(), W.data());
  // C = I + U W and its Cholesky factor
  ok = pg_host_c_chol(n, M, loops.data(), fac, lin.data(), W.data(), C.data()) && ok;
  // Y_i = Lc^-1 W_i^T in place, Sigma_ii = P_i - Y_i^T Y_i
  for (int64_t o = 0; o < n_out; ++o) {
    const int64_t i = nodes ? nodes[o] : o;
    bool done = false;  // a node named twice: its lane already holds Y
    for (int64_t p = 0; nodes && p < o; ++p) done = done || nodes[p] == i;
    if (!done)
      for (int e = 0; e < 6; ++e) pg_marg_forward(C.data(), M, W.data(), n, i, e);
    pg_marg_final(P[0].data(), W.data(), M, n, i, cov + 36 * o);
  }
  if (!ok) {
    std::fill(cov, cov + 36 * n_out, 0.0);
    return 3;
  }
  return 0;
}

// ---- the optimiser with the direct solve and the robust loop factors ----
// One graph's arrays and the steps of fbr_pg.hip's pg_run with solver = FBR_PG_SOLVER_DIRECT, in
// the order the launches are enqueued.
struct PgHostDirect {
  int64_t n, nf, K, M, chunk;
  const PgFactor* fac;
  int robust;
  double scale;
  bool graph_ok = true;  // every node has a factor
  std::vector<int32_t> off, adj, loops;
  std::vector<double> lin, fcost, chi2, wt, D0, hd, g, x, W, C, z;
  PgHostLevels LV;  // `chunk` columns for W, and one more for y

  PgHostDirect(int64_t n_, int64_t nf_, const PgFactor* fac_, int rhs_chunk, int robust_, double scale_)
      : n(n_), nf(nf_), K(count_loops(nf_, fac_)), M(6 * K),
        chunk(rhs_chunk > 0 ? std::min<int64_t>(rhs_chunk, std::max<int64_t>(M, 1)) : std::max<int64_t>(M, 1)), fac(fac_),
        robust(robust_), scale(scale_), off((size_t)n_ + 1, 0), lin((size_t)(kPgLin * nf_)), fcost((size_t)nf_),
        chi2((size_t)nf_), wt((size_t)nf_, 1.0), D0((size_t)(36 * n_)), hd((size_t)(6 * n_)), g((size_t)(6 * n_)),
        x((size_t)(6 * n_)), W((size_t)(M * 6 * n_)), C((size_t)(M * M)), z((size_t)M), LV(n_, chunk + 1) {
    for (int64_t k = 0; k < nf; ++k) {
      ++off[fac[k].i + 1];
      if (fac[k].j >= 0) ++off[fac[k].j + 1];
      if (fac[k].loop) loops.push_back((int32_t)k);
    }
    for (int64_t m = 0; m < n; ++m) {
      if (off[m + 1] == 0) graph_ok = false;
      off[m + 1] += off[m];
    }
    adj.resize((size_t)off[n]);
    std::vector<int32_t> cur(off.begin(), off.end() - 1);
    for (int64_t k = 0; k < nf; ++k) {
      adj[cur[fac[k].i]++] = (int32_t)(2 * k);
      if (fac[k].j >= 0) adj[cur[fac[k].j]++] = (int32_t)(2 * k + 1);
    }
  }
  static int64_t count_loops(int64_t nf, const PgFactor* fac) {
    int64_t K = 0;
    for (int64_t k = 0; k < nf; ++k) K += fac[k].loop;
    return K;
  }

  // launch_pg_linearize (with jac: and launch_pg_assemble)
  double evaluate(const double* X, bool jac) {
    const double cost = pg_host_evaluate(nf, fac, X, jac, robust, scale, lin.data(), fcost.data(), chi2.data(), wt.data());
    if (jac)
      for (int64_t m = 0; m < n; ++m)
        pg_assemble_node(n, m, fac, lin.data(), off.data(), adj.data(), D0.data(), LV.lev[0].A, g.data(), hd.data());
    return cost;
  }

  // One damped step into x [6][n]: launch_pg_factor and pg_direct.  false: a bad pivot of T or of C.
  bool step(double lambda) {
    std::vector<PgLevel>& lev = LV.lev;
    const size_t nl = lev.size();
    PgLevel& l0 = lev[0];
    for (int64_t i = 0; i < 36 * n; ++i) {
      const int e = (int)(i / n);
      l0.D[i] = e % 7 == 0 ? D0[i] + lambda * hd[(int64_t)(e / 7) * n + (i - (int64_t)e * n)] : D0[i];
    }
    bool ok = true;
    for (size_t l = 0; l < nl; ++l) {
      for (int64_t k = 0; k < lev[l].n; ++k)
        if (pg_cr_is_elim(lev[l].n, k)) ok = pg_cr_elim(lev[l], k) && ok;
      if (l + 1 < nl)
        for (int64_t q = 0; q < lev[l + 1].n; ++q) pg_cr_update(lev[l], lev[l + 1], q);
    }
    // y = T^-1 (-g) in the levels' last column
    const int64_t yc = chunk;
    double* yb = pg_level_col(l0, yc).b;
    for (int64_t i = 0; i < 6 * n; ++i) yb[i] = -g[i];
    for (size_t l = 0; l + 1 < nl; ++l)
      for (int64_t q = 0; q < lev[l + 1].n; ++q) pg_cr_reduce_col(lev[l], lev[l + 1], q, yc);
    pg_cr_top_col(lev[nl - 1], yc);
    for (size_t l = nl - 1; l-- > 0;)
      for (int64_t m = 0; m < lev[l].n; ++m) pg_cr_backsub_col(lev[l], lev[l + 1], m, yc);
    const double* y = pg_level_col(l0, yc).x;
    if (M > 0) {
      pg_host_w(lev, n, M, chunk, loops.data(), fac, lin.data(), W.data());
      ok = pg_host_c_chol(n, M, loops.data(), fac, lin.data(), W.data(), C.data()) && ok;
      for (int64_t row = 0; row < M; ++row) z[row] = pg_direct_z_entry(fac, lin.data(), loops.data(), y, n, row);
      pg_dense_subst(C.data(), M, z.data());
    }
    for (int64_t t = 0; t < 6 * n; ++t) x[t] = pg_direct_delta_entry(y, W.data(), z.data(), M, n, t);
    return ok;
  }
};

// fbr_pg_optimize with solver = FBR_PG_SOLVER_DIRECT on the host.  euler0 [n][6] the stored poses;
// par = {max_iterations, rel_cost_tol, abs_cost_tol, lambda_init, lambda_factor, lambda_max};
// rhs_chunk <= 0: every column of W in one pass; poses_out [n][6]; info = {status, iterations,
// trials, cost_initial, cost_final, lambda}; chi2_out, w_out [nf] (optional): every factor's |r|^2
// and weight at the result poses.  Status: fbr.h's FBR_PG_*.  Returns -1 when a node has no factor.
inline int pg_direct_lm_host(int64_t n, const double* euler0, int64_t nf, const PgFactor* fac, const double* par,
                             int rhs_chunk, int robust, double robust_scale, double* poses_out, double* info,
                             double* chi2_out, double* w_out) {
  const int max_it = (int)par[0];
  const double rel_tol = par[1], abs_tol = par[2], lfac = par[4], lmax = par[5];
  PgHostDirect S(n, nf, fac, rhs_chunk, robust, robust_scale);
  if (!S.graph_ok) return -1;
  std::vector<double> X0((size_t)(12 * n)), X, Xt((size_t)(12 * n));
  for (int64_t i = 0; i < n; ++i) pg_pose_from_euler(euler0 + 6 * i, &X0[12 * i]);
  X = X0;
  double cost = S.evaluate(X.data(), true), lambda = par[3];
  info[3] = info[4] = cost;
  int status = -1, iterations = 0, trials = 0;
  if (cost == 0.0) status = 0;
  else if (!(cost < INFINITY)) status = 3;
  else if (max_it <= 0) status = 1;
  while (status < 0) {
    const bool ok = S.step(lambda);
    for (int64_t m = 0; m < n; ++m) {
      double d[6];
      pg_ld6(S.x.data(), n, m, d);
      pg_retract(&X[12 * m], d, &Xt[12 * m]);
    }
    const double trial = S.evaluate(Xt.data(), false);
    ++trials;
    if (!ok) {
      status = 3;
      break;
    }
    if (trial < cost) {
      X.swap(Xt);
      const double dec = cost - trial, rel = dec / cost;
      cost = trial;
      ++iterations;
      lambda /= lfac;
      if (rel < rel_tol || dec < abs_tol) status = 0;
      else if (iterations >= max_it) status = 1;
      else (void)S.evaluate(X.data(), true);
    } else {
      lambda *= lfac;
      if (lambda > lmax) status = 2;
    }
  }
  // the per-factor values at the result poses: the last evaluation's unless that was a rejected trial's
  if (status == 3) (void)S.evaluate(X0.data(), false);
  else if (status == 2) (void)S.evaluate(X.data(), false);
  for (int64_t k = 0; k < nf; ++k) {
    if (chi2_out) chi2_out[k] = robust != kPgRobustNone ? S.chi2[k] : 2.0 * S.fcost[k];
    if (w_out) w_out[k] = S.wt[k];
  }
  for (int64_t i = 0; i < n; ++i) {
    if (status == 3) memcpy(poses_out + 6 * i, euler0 + 6 * i, sizeof(double) * 6);
    else pg_euler_from_pose(&X[12 * i], poses_out + 6 * i);
  }
  if (status != 3) info[4] = cost;
  info[0] = status;
  info[1] = iterations;
  info[2] = trials;
  info[5] = lambda;
  return 0;
}

// One direct step at the poses euler [n][6] with damping lambda: delta [n][6] (node-major).  Returns
// 0, 3 for a bad pivot of T or of C, -1 when a node has no factor.
inline int pg_direct_step_host(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, double lambda, int rhs_chunk,
                               int robust, double robust_scale, double* delta) {
  PgHostDirect S(n, nf, fac, rhs_chunk, robust, robust_scale);
  if (!S.graph_ok) return -1;
  std::vector<double> X((size_t)(12 * n));
  for (int64_t i = 0; i < n; ++i) pg_pose_from_euler(euler + 6 * i, &X[12 * i]);
  (void)S.evaluate(X.data(), true);
  const bool ok = S.step(lambda);
  for (int64_t m = 0; m < n; ++m) pg_ld6(S.x.data(), n, m, delta + 6 * m);
  return ok ? 0 : 3;
}

}  // namespace fbr
