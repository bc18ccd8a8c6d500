// Host-compiled probe of csrc/fbr_pg.h (test infrastructure): the pose-graph arithmetic exactly as
// k_posegraph.hip compiles it, built for the CPU so the tests can compare it with the NumPy model
// (tests/pg_model.py) without a GPU: a factor's residual and Jacobians, the 6x6 Cholesky, the block
// cyclic reduction run level by level, and a host Levenberg-Marquardt + PCG built from the same
// functions in the order fbr_pg.hip enqueues the kernels.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fbr_pg.h"

using namespace fbr;

namespace {

// The levels of an n-node system over one allocation.
struct Levels {
  std::vector<double> mem;
  std::vector<PgLevel> lev;
  explicit Levels(int64_t n) {
    int64_t tot = 0;
    const int nl = pg_cr_levels(n, &tot);
    mem.assign((size_t)(tot * (36 * 5 + 12)), 0.0);
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
      v.b = w; w += 6 * ln;
      v.x = w; w += 6 * ln;
      lev.push_back(v);
    }
  }
};

bool cr_factor(std::vector<PgLevel>& lev) {
  bool ok = true;
  for (size_t l = 0; l < lev.size(); ++l) {
    const PgLevel& lv = lev[l];
    for (int64_t k = 0; k < lv.n; ++k)
      if (pg_cr_is_elim(lv.n, k)) ok = pg_cr_elim(lv, k) && ok;
    if (l + 1 < lev.size())
      for (int64_t q = 0; q < lev[l + 1].n; ++q) pg_cr_update(lv, lev[l + 1], q);
  }
  return ok;
}

void cr_solve(std::vector<PgLevel>& lev) {
  const size_t nl = lev.size();
  for (size_t l = 0; l + 1 < nl; ++l)
    for (int64_t q = 0; q < lev[l + 1].n; ++q) pg_cr_reduce(lev[l], lev[l + 1], q);
  pg_cr_top(lev[nl - 1]);
  for (size_t l = nl - 1; l-- > 0;)
    for (int64_t m = 0; m < lev[l].n; ++m) pg_cr_backsub(lev[l], lev[l + 1], m);
}

double dot(const std::vector<double>& a, const double* b) {
  double s = 0.0;
  for (size_t i = 0; i < a.size(); ++i) s = s + a[i] * b[i];
  return s;
}

}  // namespace

extern "C" {

int probe_pg_factor_bytes() { return (int)sizeof(PgFactor); }

void probe_pg_exp(const double* w, double* R) { pg_exp(w, R); }
void probe_pg_log(const double* R, double* w) { pg_log(R, w); }
void probe_pg_pose_from_euler(const double* e, double* X) { pg_pose_from_euler(e, X); }
void probe_pg_euler_from_pose(const double* X, double* e) { pg_euler_from_pose(X, e); }

void probe_pg_factor(const PgFactor* f, const double* Xi, const double* Xj, double* r, double* Ji, double* Jj) {
  pg_factor_eval(*f, Xi, Xj, true, r, Ji, Jj);
}

int probe_pg_chol6(const double* A, double* L) { return pg_chol6(A, L) ? 1 : 0; }
void probe_pg_chol6_solve(const double* L, double* x) { pg_chol6_solve(L, x); }

// T x = b for the block-tridiagonal T with diagonal blocks D[n][36] and couplings A[n][36]
// (A[m] = T[m][m-1], A[0] ignored), b and x [n][6]; returns 0 on a bad pivot.
int probe_pg_tridiag_solve(int64_t n, const double* D, const double* A, const double* b, double* x) {
  Levels L(n);
  PgLevel& l0 = L.lev[0];
  for (int64_t m = 0; m < n; ++m) {
    pg_st36(l0.D, n, m, D + 36 * m);
    pg_st36(l0.A, n, m, A + 36 * m);
    pg_st6(l0.b, n, m, b + 6 * m);
  }
  const bool ok = cr_factor(L.lev);
  cr_solve(L.lev);
  for (int64_t m = 0; m < n; ++m) pg_ld6(l0.x, n, m, x + 6 * m);
  return ok ? 1 : 0;
}

// The optimiser of fbr_pg.hip on the host.  euler0 [n][6] the stored poses; par = {max_iterations,
// max_pcg_iterations, rel_cost_tol, abs_cost_tol, pcg_rel_tol, lambda_init, lambda_factor,
// lambda_max}; poses_out [n][6]; info = {status, iterations, trials, pcg_iterations, cost_initial,
// cost_final, lambda, max PCG iterations of one solve}.  Status: fbr.h's FBR_PG_* (0 converged,
// 1 iterations, 2 stalled, 3 numerical).  Returns -1 when a node has no factor.
int probe_pg_optimize(int64_t n, const double* euler0, int64_t nf, const PgFactor* fac, const double* par,
                      double* poses_out, double* info) {
  const int max_it = (int)par[0], max_pcg = (int)par[1];
  const double rel_tol = par[2], abs_tol = par[3], tol2 = par[4] * par[4], lfac = par[6], lmax = par[7];
  std::vector<int32_t> off((size_t)n + 1, 0), loff((size_t)n + 1, 0);
  for (int64_t k = 0; k < nf; ++k) {
    ++off[fac[k].i + 1];
    if (fac[k].j >= 0) ++off[fac[k].j + 1];
    if (fac[k].loop) {
      ++loff[fac[k].i + 1];
      ++loff[fac[k].j + 1];
    }
  }
  for (int64_t m = 0; m < n; ++m) {
    if (off[m + 1] == 0) return -1;
    off[m + 1] += off[m];
    loff[m + 1] += loff[m];
  }
  std::vector<int32_t> adj((size_t)off[n]), ladj((size_t)loff[n]), cur(off.begin(), off.end() - 1),
      lcur(loff.begin(), loff.end() - 1);
  for (int64_t k = 0; k < nf; ++k) {
    adj[cur[fac[k].i]++] = (int32_t)(2 * k);
    if (fac[k].j >= 0) adj[cur[fac[k].j]++] = (int32_t)(2 * k + 1);
    if (fac[k].loop) {
      ladj[lcur[fac[k].i]++] = (int32_t)(2 * k);
      ladj[lcur[fac[k].j]++] = (int32_t)(2 * k + 1);
    }
  }
  std::vector<double> X((size_t)(12 * n)), Xt((size_t)(12 * n)), lin((size_t)(kPgLin * nf)), D0((size_t)(36 * n)),
      hd((size_t)(6 * n)), g((size_t)(6 * n)), x((size_t)(6 * n)), r((size_t)(6 * n)), p((size_t)(6 * n)),
      q((size_t)(6 * n));
  Levels LV(n);
  PgLevel& l0 = LV.lev[0];
  for (int64_t i = 0; i < n; ++i) pg_pose_from_euler(euler0 + 6 * i, &X[12 * i]);

  auto evaluate = [&](const std::vector<double>& P, bool jac) {
    double cost = 0.0;
    for (int64_t k = 0; k < nf; ++k) {
      double rr[6], Ji[36], Jj[36], zero[12] = {0};
      const double* Xj = fac[k].j >= 0 ? &P[12 * fac[k].j] : zero;
      pg_factor_eval(fac[k], &P[12 * fac[k].i], Xj, jac, rr, Ji, Jj);
      double c = 0.0;
      for (int e = 0; e < 6; ++e) c = c + rr[e] * rr[e];
      cost = cost + 0.5 * c;
      if (jac) {
        double* o = &lin[kPgLin * k];
        memcpy(o, rr, sizeof(rr));
        memcpy(o + 6, Ji, sizeof(Ji));
        memcpy(o + 42, Jj, sizeof(Jj));
      }
    }
    return cost;
  };
  auto assemble = [&]() {
    for (int64_t m = 0; m < n; ++m)
      pg_assemble_node(n, m, fac, lin.data(), off.data(), adj.data(), D0.data(), l0.A, g.data(), hd.data());
  };

  double cost = evaluate(X, true), lambda = par[5];
  assemble();
  info[4] = info[5] = cost;
  int status = -1, iterations = 0, trials = 0, pcg_total = 0, pcg_max = 0;
  if (cost == 0.0) status = 0;
  else if (!(cost < INFINITY)) status = 3;
  else if (max_it <= 0) status = 1;
  while (status < 0) {
    for (int64_t i = 0; i < 36 * n; ++i) {
      const int e = (int)(i / n);
      l0.D[i] = e % 7 == 0 ? D0[i] + lambda * hd[(int64_t)(e / 7) * n + (i - (int64_t)e * n)] : D0[i];
    }
    const bool ok = cr_factor(LV.lev);
    // PCG, as launch_pg_pcg_init / launch_pg_pcg_iter
    int iters = 0;
    for (int64_t i = 0; i < 6 * n; ++i) {
      x[i] = 0.0;
      r[i] = -g[i];
      l0.b[i] = r[i];
    }
    cr_solve(LV.lev);
    double rz = dot(r, l0.x);
    const double rz0 = rz;
    bool stopped = !(rz0 > 0.0) || !(rz0 < INFINITY);
    if (!stopped) memcpy(p.data(), l0.x, sizeof(double) * 6 * n);
    for (int it = 0; it < max_pcg && !stopped; ++it) {
      double pq = 0.0;
      for (int64_t m = 0; m < n; ++m)
        pq = pq + pg_hp_node(n, m, fac, lin.data(), loff.data(), ladj.data(), l0.D, l0.A, p.data(), q.data());
      if (!(pq > 0.0) || !(pq < INFINITY)) break;
      const double alpha = rz / pq;
      for (int64_t i = 0; i < 6 * n; ++i) {
        x[i] = x[i] + alpha * p[i];
        r[i] = r[i] - alpha * q[i];
        l0.b[i] = r[i];
      }
      cr_solve(LV.lev);
      const double s = dot(r, l0.x), beta = s / rz;
      rz = s;
      iters = it + 1;
      if (!(s > tol2 * rz0) || !(s < INFINITY) || it + 1 >= max_pcg) stopped = true;
      if (!stopped)
        for (int64_t i = 0; i < 6 * n; ++i) p[i] = l0.x[i] + beta * p[i];
    }
    for (int64_t m = 0; m < n; ++m) {
      double d[6];
      pg_ld6(x.data(), n, m, d);
      pg_retract(&X[12 * m], d, &Xt[12 * m]);
    }
    const double trial = evaluate(Xt, false);
    ++trials;
    pcg_total += iters;
    pcg_max = std::max(pcg_max, iters);
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
      else {
        (void)evaluate(X, true);
        assemble();
      }
    } else {
      lambda *= lfac;
      if (lambda > lmax) status = 2;
    }
  }
  for (int64_t i = 0; i < n; ++i) {
    if (status == 3) memcpy(poses_out + 6 * i, euler0 + 6 * i, sizeof(double) * 6);
    else pg_euler_from_pose(&X[12 * i], poses_out + 6 * i);
  }
  if (status != 3) info[5] = cost;
  info[0] = status;
  info[1] = iterations;
  info[2] = trials;
  info[3] = pcg_total;
  info[6] = lambda;
  info[7] = pcg_max;
  return 0;
}

}
