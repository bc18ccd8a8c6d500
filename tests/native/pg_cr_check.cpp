// pg_cr_check.cpp — the block cyclic reduction of csrc/fbr_pg.h over exactly sized heap arrays.
//
// A stand-alone program (tests/test_pg_model.py builds it with -fsanitize=address,undefined and runs
// it): every level's arrays are separate allocations of exactly their size, so an index past a
// level's end is a heap overflow the sanitizer reports.  It solves a diagonally dominant
// block-tridiagonal system at sizes around every level boundary, checks the residual, prints
// "pg_cr_check: ok" and exits 0, or names the size that failed and exits 1.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "fbr_pg.h"

using namespace fbr;

namespace {

struct Level {
  std::unique_ptr<double[]> D, A, L, G, H, b, x;
  PgLevel v;
  explicit Level(int64_t n)
      : D(new double[36 * n]()), A(new double[36 * n]()), L(new double[36 * n]()), G(new double[36 * n]()),
        H(new double[36 * n]()), b(new double[6 * n]()), x(new double[6 * n]()) {
    v = PgLevel{n, D.get(), A.get(), L.get(), G.get(), H.get(), b.get(), x.get()};
  }
};

double rnd(uint64_t* s) {  // xorshift, in [-1, 1)
  *s ^= *s << 13;
  *s ^= *s >> 7;
  *s ^= *s << 17;
  return (double)(*s >> 11) / 4503599627370496.0 - 1.0;
}

bool check(int64_t n) {
  int64_t tot = 0;
  const int nl = pg_cr_levels(n, &tot);
  std::vector<std::unique_ptr<Level>> lev;
  int64_t ln = n, sum = 0;
  for (int l = 0; l < nl; ++l, ln = (ln + 1) / 2) {
    lev.emplace_back(new Level(ln));
    sum += ln;
  }
  if (sum != tot || lev.back()->v.n != 1) return false;
  uint64_t seed = 88172645463325252ull + (uint64_t)n;
  PgLevel& l0 = lev[0]->v;
  std::vector<double> D((size_t)(36 * n)), A((size_t)(36 * n)), b((size_t)(6 * n));
  for (int64_t m = 0; m < n; ++m) {
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c <= r; ++c) {
        const double v = r == c ? 20.0 + rnd(&seed) : rnd(&seed);
        D[36 * m + 6 * r + c] = D[36 * m + 6 * c + r] = v;
      }
    for (int e = 0; e < 36; ++e) A[36 * m + e] = m ? rnd(&seed) : 0.0;
    for (int e = 0; e < 6; ++e) b[6 * m + e] = rnd(&seed);
    pg_st36(l0.D, n, m, &D[36 * m]);
    pg_st36(l0.A, n, m, &A[36 * m]);
    pg_st6(l0.b, n, m, &b[6 * m]);
  }
  bool ok = true;
  for (int l = 0; l < nl; ++l) {
    const PgLevel& lv = lev[l]->v;
    for (int64_t k = 0; k < lv.n; ++k)
      if (pg_cr_is_elim(lv.n, k)) ok = pg_cr_elim(lv, k) && ok;
    if (l + 1 < nl)
      for (int64_t q = 0; q < lev[l + 1]->v.n; ++q) pg_cr_update(lv, lev[l + 1]->v, q);
  }
  for (int l = 0; l + 1 < nl; ++l)
    for (int64_t q = 0; q < lev[l + 1]->v.n; ++q) pg_cr_reduce(lev[l]->v, lev[l + 1]->v, q);
  pg_cr_top(lev[nl - 1]->v);
  for (int l = nl - 2; l >= 0; --l)
    for (int64_t m = 0; m < lev[l]->v.n; ++m) pg_cr_backsub(lev[l]->v, lev[l + 1]->v, m);
  double worst = 0.0;
  for (int64_t m = 0; m < n; ++m) {
    double x[6], xp[6] = {0}, xn[6] = {0};
    pg_ld6(l0.x, n, m, x);
    if (m) pg_ld6(l0.x, n, m - 1, xp);
    if (m + 1 < n) pg_ld6(l0.x, n, m + 1, xn);
    for (int r = 0; r < 6; ++r) {
      double s = -b[6 * m + r];
      for (int c = 0; c < 6; ++c) {
        s += D[36 * m + 6 * r + c] * x[c] + A[36 * m + 6 * r + c] * xp[c];
        if (m + 1 < n) s += A[36 * (m + 1) + 6 * c + r] * xn[c];
      }
      worst = std::fmax(worst, std::fabs(s));
    }
  }
  return ok && worst < 1e-12;
}

}  // namespace

int main() {
  const int64_t sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 257, 1000};
  for (int64_t n : sizes)
    if (!check(n)) {
      std::printf("pg_cr_check: n = %lld failed\n", (long long)n);
      return 1;
    }
  std::printf("pg_cr_check: ok\n");
  return 0;
}
