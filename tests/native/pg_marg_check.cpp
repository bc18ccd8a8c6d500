// Stand-alone check of the marginal covariances' host driver (csrc/fbr_pg_host.h over csrc/fbr_pg.h)
// for the host sanitizers: a 33-node circle with a tight prior and the loops (32, 0), (20, 5),
// (7, 9), generated here, through every code path of the driver (all nodes, a subset with a repeat,
// rhs_chunk 7 and 1, a graph without a prior).  It loads no Python and needs no GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off
//       -I feature_base_pointcloud_registration_amd/csrc -o pg_marg_check tests/native/pg_marg_check.cpp
// Exit status 0 and "pg_marg_check ok" when every check holds.
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
  printf("pg_marg_check FAILED: %s\n", what);
  return 1;
}

}  // namespace

int main() {
  const int n = 33;
  std::vector<double> eul((size_t)(6 * n)), X((size_t)(12 * n));
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
  }
  std::vector<PgFactor> chain, fac;
  for (int i = 1; i < n; ++i) chain.push_back(between(i - 1, i, &X[12 * (i - 1)], &X[12 * i], 1e3, 1e2));
  PgFactor prior{};
  prior.type = kPgPrior;
  prior.i = 0;
  prior.j = -1;
  memcpy(prior.Z, &X[0], sizeof(prior.Z));
  for (int k = 0; k < 6; ++k) prior.w[k] = 1e2;
  fac.push_back(prior);
  fac.insert(fac.end(), chain.begin(), chain.end());
  const int loops[3][2] = {{32, 0}, {20, 5}, {7, 9}};
  for (const auto& l : loops) fac.push_back(between(l[0], l[1], &X[12 * l[0]], &X[12 * l[1]], 3.0, 3.0));

  std::vector<double> full((size_t)(36 * n)), other((size_t)(36 * n));
  if (pg_marginals_host(n, eul.data(), (int64_t)fac.size(), fac.data(), nullptr, 0, 0, full.data()) != 0)
    return fail("status of the all-nodes call");
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < 6; ++r) {
      if (!(full[36 * i + 7 * r] > 0.0)) return fail("a diagonal entry is not positive");
      for (int c = 0; c < 6; ++c)
        if (full[36 * i + 6 * r + c] != full[36 * i + 6 * c + r]) return fail("a block is not symmetric");
    }
  for (int chunk : {7, 1}) {
    if (pg_marginals_host(n, eul.data(), (int64_t)fac.size(), fac.data(), nullptr, 0, chunk, other.data()) != 0)
      return fail("status of a chunked call");
    if (memcmp(full.data(), other.data(), sizeof(double) * 36 * n)) return fail("rhs_chunk changed the bytes");
  }
  const int64_t nodes[4] = {32, 0, 16, 32};
  std::vector<double> sub(36 * 4);
  if (pg_marginals_host(n, eul.data(), (int64_t)fac.size(), fac.data(), nodes, 4, 0, sub.data()) != 0)
    return fail("status of the subset call");
  for (int o = 0; o < 4; ++o)
    if (memcmp(&sub[36 * o], &full[36 * nodes[o]], sizeof(double) * 36)) return fail("a subset row differs");
  const int64_t bad = 33;
  if (pg_marginals_host(n, eul.data(), (int64_t)fac.size(), fac.data(), &bad, 1, 0, sub.data()) != -1)
    return fail("a node index out of range was accepted");
  // without the prior T0 is singular: status 3 and a zeroed output
  std::vector<PgFactor> free_graph(fac.begin() + 1, fac.end());
  if (pg_marginals_host(n, eul.data(), (int64_t)free_graph.size(), free_graph.data(), nullptr, 0, 0, other.data()) != 3)
    return fail("a graph without a prior was not reported");
  for (double v : other)
    if (v != 0.0) return fail("the output of a failed call is not zeroed");
  // a single node
  double one[36];
  if (pg_marginals_host(1, eul.data(), 1, &prior, nullptr, 0, 0, one) != 0 || !(one[0] > 0.0)) return fail("one node");
  printf("pg_marg_check ok: Sigma(32)[3][3] = %.9g, [4][4] = %.9g\n", full[36 * 32 + 21], full[36 * 32 + 28]);
  return 0;
}
