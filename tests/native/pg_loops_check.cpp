// Stand-alone check of the direct Levenberg-Marquardt's host driver (csrc/fbr_pg_host.h over
// csrc/fbr_pg.h) for the host sanitizers: a 33-node circle with a tight prior, stored poses that
// disagree with the odometry, and K = 0, 2 and 6 loops (6 K = 36 crosses a 32-column panel of the
// dense factor), generated here; every graph in one pass of W and with rhs_chunk 7 and 1, without
// a robust option and with both kinds, one loop of the largest graph being a false one; a single
// node; a singular T.  It loads no Python and needs no GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off
//       -I feature_base_pointcloud_registration_amd/csrc -o pg_loops_check tests/native/pg_loops_check.cpp
// Exit status 0 and "pg_loops_check ok" when every check holds.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fbr_pg_host.h"

using namespace fbr;

namespace {

PgFactor between(int i, int j, const double* Xi, const double* Xj, double wr, double wt) {
  PgFactor f{};
  f.type = kPgBetween;
  f.i = i;
  f.j = j;
  f.loop = (i - j == 1 || j - i == 1) ? 0 : 1;
  pg_between(Xi, Xj, f.Z);
  for (int k = 0; k < 3; ++k) {
    f.w[k] = wr;
    f.w[3 + k] = wt;
  }
  return f;
}

int fail(const char* what) {
  printf("pg_loops_check FAILED: %s\n", what);
  return 1;
}

}  // namespace

int main() {
  const int n = 33;
  std::vector<double> eul((size_t)(6 * n)), start((size_t)(6 * n)), X((size_t)(12 * n));
  for (int i = 0; i < n; ++i) {
    const double th = 2.0 * 3.14159265358979323846 * i / n;
    double* e = &eul[6 * i];
    e[0] = 0.02 * sin(3 * th);
    e[1] = 0.03 * cos(2 * th);
    e[2] = th + 1.5;
    e[3] = 30.0 * cos(th);
    e[4] = 30.0 * sin(th);
    e[5] = 0.5 * sin(th);
    pg_pose_from_euler(e, &X[12 * i]);
    // the stored poses: a drift that grows along the run
    for (int k = 0; k < 6; ++k) start[6 * i + k] = e[k];
    start[6 * i + 2] += 2e-3 * i;
    start[6 * i + 3] += 0.02 * i * cos(5 * th);
    start[6 * i + 4] += 0.02 * i * sin(7 * th);
  }
  PgFactor prior{};
  prior.type = kPgPrior;
  prior.i = 0;
  prior.j = -1;
  memcpy(prior.Z, &X[0], sizeof(prior.Z));
  for (int k = 0; k < 6; ++k) prior.w[k] = 1e2;
  std::vector<PgFactor> chain;
  chain.push_back(prior);
  for (int i = 1; i < n; ++i) chain.push_back(between(i - 1, i, &X[12 * (i - 1)], &X[12 * i], 1e3, 1e2));
  const int loops[6][2] = {{32, 0}, {20, 5}, {7, 9}, {31, 1}, {0, 30}, {25, 12}};
  const double par[6] = {30, 1e-10, 1e-10, 1e-5, 10.0, 1e10};

  for (int K : {0, 2, 6}) {
    std::vector<PgFactor> fac(chain);
    for (int l = 0; l < K; ++l) fac.push_back(between(loops[l][0], loops[l][1], &X[12 * loops[l][0]], &X[12 * loops[l][1]], 3.0, 3.0));
    if (K == 6) {  // a false loop: "the same place" for two nodes a third of the circle apart
      PgFactor& f = fac.back();
      memset(f.Z, 0, sizeof(f.Z));
      f.Z[0] = f.Z[4] = f.Z[8] = 1.0;
    }
    const int64_t nf = (int64_t)fac.size();
    for (int robust : {kPgRobustNone, kPgRobustHuber, kPgRobustCauchy}) {
      const double scale = robust == kPgRobustHuber ? 1.345 : 3.0;
      std::vector<double> ref((size_t)(6 * n)), out((size_t)(6 * n)), chi2((size_t)nf), w((size_t)nf), chi2b((size_t)nf),
          wb((size_t)nf);
      double info[6], infob[6];
      if (pg_direct_lm_host(n, start.data(), nf, fac.data(), par, 0, robust, scale, ref.data(), info, chi2.data(), w.data()))
        return fail("a node without a factor");
      if (info[0] != 0.0 && info[0] != 1.0) return fail("status of the optimise");
      if (!(info[4] <= info[3]) || !(info[1] >= 1.0)) return fail("the cost did not fall");
      for (int64_t k = 0; k < nf; ++k) {
        if (!(w[k] > 0.0 && w[k] <= 1.0) || !(chi2[k] >= 0.0)) return fail("a weight outside (0, 1] or a negative chi-square");
        if (!fac[k].loop && w[k] != 1.0) return fail("a factor that is no loop was re-weighted");
        if (robust == kPgRobustNone && w[k] != 1.0) return fail("a weight without a robust option");
      }
      if (K == 6 && robust != kPgRobustNone && !(w[nf - 1] < 0.5)) return fail("the false loop kept its weight");
      for (int chunk : {7, 1}) {
        if (pg_direct_lm_host(n, start.data(), nf, fac.data(), par, chunk, robust, scale, out.data(), infob, chi2b.data(),
                              wb.data()))
          return fail("a chunked optimise");
        if (memcmp(ref.data(), out.data(), sizeof(double) * 6 * n) || memcmp(info, infob, sizeof(info)) ||
            memcmp(chi2.data(), chi2b.data(), sizeof(double) * nf) || memcmp(w.data(), wb.data(), sizeof(double) * nf))
          return fail("rhs_chunk changed the bytes");
      }
      // the weighted marginals at the result
      std::vector<double> cov((size_t)(36 * n));
      if (pg_marginals_host(n, ref.data(), nf, fac.data(), nullptr, 0, 7, cov.data(), robust, scale) != 0)
        return fail("status of the weighted marginals");
      for (int i = 0; i < n; ++i)
        for (int r = 0; r < 6; ++r)
          if (!(cov[36 * i + 7 * r] > 0.0)) return fail("a diagonal entry of a marginal is not positive");
      printf("K = %d robust %d: %g steps, cost %.9g -> %.9g\n", K, robust, info[1], info[3], info[4]);
    }
  }
  // a single step without damping on a graph without a prior: T is singular
  std::vector<PgFactor> free_graph(chain.begin() + 1, chain.end());
  free_graph.push_back(between(32, 0, &X[12 * 32], &X[0], 3.0, 3.0));
  std::vector<double> delta((size_t)(6 * n));
  if (pg_direct_step_host(n, start.data(), (int64_t)free_graph.size(), free_graph.data(), 0.0, 0, kPgRobustNone, 0.0,
                          delta.data()) != 3)
    return fail("a singular T was not reported");
  // a node no factor touches
  if (pg_direct_step_host(n + 1, start.data(), (int64_t)chain.size(), chain.data(), 1e-5, 0, kPgRobustNone, 0.0,
                          delta.data()) != -1)
    return fail("a node without a factor was accepted");
  // a single node
  double one[6], info1[6];
  if (pg_direct_lm_host(1, start.data() + 6, 1, &prior, par, 0, kPgRobustHuber, 1.345, one, info1, nullptr, nullptr) ||
      info1[0] != 0.0)
    return fail("one node");
  printf("pg_loops_check ok\n");
  return 0;
}
