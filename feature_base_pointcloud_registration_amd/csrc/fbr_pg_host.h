// fbr_pg_host.h — the marginal covariances of include/fbr.h ("marginal covariances") on the host:
// fbr_pg.h's per-node steps in plain loops, in the order fbr_pg.hip enqueues k_pg_marginals.hip's
// kernels.  Host-only and free of HIP headers: tests/native/pg_marg_probe.cpp loads it into the
// tests, tests/native/pg_marg_check.cpp runs it under the host sanitizers.
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

// Sigma_ii of the nodes `nodes` (null: every node in order, n_out = n) at the poses euler [n][6],
// into cov [n_out][36].  rhs_chunk <= 0: every column in one pass.  Returns 0 (FBR_PG_CONVERGED),
// 3 (FBR_PG_NUMERICAL: a bad pivot of T0 or of C; cov is zeroed), -1 for a node no factor touches
// or a node index out of range.
inline int pg_marginals_host(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, const int64_t* nodes,
                             int64_t n_out, int rhs_chunk, double* cov) {
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
  for (int64_t k = 0; k < nf; ++k) {
    double zero[12] = {0};
    double* o = &lin[kPgLin * k];
    pg_factor_eval(fac[k], &X[12 * fac[k].i], fac[k].j >= 0 ? &X[12 * fac[k].j] : zero, true, o, o + 6, o + 42);
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
  for (int64_t c0 = 0; c0 < M; c0 += chunk) {
    const int64_t nc = std::min(chunk, M - c0);
    std::fill(lev[0].b, lev[0].b + 6 * n * nc, 0.0);
    for (int64_t cc = 0; cc < nc; ++cc) {
      const int64_t col = c0 + cc;
      const int32_t fk = loops[col / 6];
      const int r = (int)(col % 6);
      for (int side = 0; side < 2; ++side) {
        const int64_t node = side ? fac[fk].j : fac[fk].i;
        for (int e = 0; e < 6; ++e) lev[0].b[(cc * 6 + e) * n + node] = pg_marg_rhs_entry(lin.data(), fk, r, side, e);
      }
    }
    for (int64_t cc = 0; cc < nc; ++cc) {
      for (size_t l = 0; l + 1 < nl; ++l)
        for (int64_t q = 0; q < lev[l + 1].n; ++q) pg_cr_reduce_col(lev[l], lev[l + 1], q, cc);
      pg_cr_top_col(lev[nl - 1], cc);
      for (size_t l = nl - 1; l-- > 0;)
        for (int64_t m = 0; m < lev[l].n; ++m) pg_cr_backsub_col(lev[l], lev[l + 1], m, cc);
    }
    memcpy(&W[(size_t)(c0 * 6 * n)], lev[0].x, sizeof(double) * 6 * n * nc);
  }
  // C = I + U W and its Cholesky factor
  for (int64_t r = 0; r < M; ++r)
    for (int64_t c = 0; c < M; ++c) C[r * M + c] = pg_marg_c_entry(fac, lin.data(), loops.data(), W.data(), n, r, c);
  for (int64_t j0 = 0; j0 < M; j0 += kPgPanel) {
    const int nb = (int)std::min<int64_t>(kPgPanel, M - j0);
    ok = pg_dense_chol_block(&C[j0 * M + j0], M, nb) && ok;
    for (int64_t i = j0 + nb; i < M; ++i) pg_dense_panel_row(C.data(), M, j0, nb, &C[j0 * M + j0], M, i);
    for (int64_t i = j0 + nb; i < M; ++i)
      for (int64_t j = j0 + nb; j <= i; ++j) pg_dense_trail_entry(C.data(), M, j0, nb, i, j);
  }
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

}  // namespace fbr
