// Host-compiled probe of the marginal covariances (test infrastructure): csrc/fbr_pg_host.h's driver
// over csrc/fbr_pg.h's per-node steps, exactly as k_pg_marginals.hip compiles them, built for the CPU
// so the tests can compare it with the NumPy model (tests/pg_marg_model.py) without a GPU.
#include "fbr_pg_host.h"

using namespace fbr;

extern "C" {

int probe_pg_marg_factor_bytes() { return (int)sizeof(PgFactor); }

// cov [n_out][36] of the nodes `nodes` (null: every node, n_out ignored) at the poses euler [n][6].
// Returns pg_marginals_host's status: 0 ok, 3 numerical (cov zeroed), -1 bad graph or node index.
int probe_pg_marginals(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, const int64_t* nodes,
                       int64_t n_out, int rhs_chunk, double* cov) {
  return pg_marginals_host(n, euler, nf, fac, nodes, n_out, rhs_chunk, cov);
}

// fbr_pg_gps_gate on the host: the last node's marginal, cov_xy = its (3,3) and (4,4).
int probe_pg_gps_gate(int64_t n, const double* euler, int64_t nf, const PgFactor* fac, double threshold, int* wanted,
                      double* cov_xy) {
  const int64_t last = n - 1;
  double cov[36];
  const int rc = pg_marginals_host(n, euler, nf, fac, &last, 1, 0, cov);
  // (no covariance: unbounded, as fbr_pg_gps_gate reports it)
  cov_xy[0] = rc == 0 ? cov[6 * 3 + 3] : INFINITY;
  cov_xy[1] = rc == 0 ? cov[6 * 4 + 4] : INFINITY;
  *wanted = rc == 0 ? pg_gps_gate_wanted(cov, threshold) : 1;
  return rc;
}

}
