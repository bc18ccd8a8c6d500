// fbr_pg.hip — the pose-graph optimiser over the keyframe store (include/fbr.h "pose graph"): the
// factor list, the Levenberg-Marquardt driver of k_posegraph.hip's kernels, and correctPoses.
#include "fbr_ctx.h"

namespace {

bool variances_ok(const double* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!(v[k] > 0.0) || !(v[k] < INFINITY)) return false;
  return true;
}
bool node_ok(const fbr_ctx* c, int64_t i) { return i >= 0 && i < (int64_t)c->kf_poses.size(); }

void keypose_euler(const fbr_keypose& k, double e[6]) {
  e[0] = (double)k.roll; e[1] = (double)k.pitch; e[2] = (double)k.yaw;
  e[3] = (double)k.x; e[4] = (double)k.y; e[5] = (double)k.z;
}

int add_between(fbr_ctx* c, int64_t i, int64_t j, const double Z[12], const double var[6]) {
  if (!node_ok(c, i) || !node_ok(c, j) || i == j || !variances_ok(var, 6)) return FBR_ERR_INVALID_ARG;
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(Z[k])) return FBR_ERR_INVALID_ARG;
  PgFactor f{};
  f.type = kPgBetween;
  f.i = (int32_t)i;
  f.j = (int32_t)j;
  f.loop = (i - j == 1 || j - i == 1) ? 0 : 1;
  std::memcpy(f.Z, Z, sizeof(f.Z));
  for (int k = 0; k < 6; ++k) f.w[k] = 1.0 / std::sqrt(var[k]);
  c->pg_factors.push_back(f);
  return FBR_OK;
}

// The device arrays of one optimise, carved out of c->d_pg_work (doubles) and c->d_pg_adj.
struct PgPlan {
  PgArgs a;
  double *X, *Xt;
};

int pg_prepare(fbr_ctx* c, int64_t n, int robust, double robust_scale, PgPlan* pl) {
  const std::vector<PgFactor>& F = c->pg_factors;
  const int64_t nf = (int64_t)F.size();
  // adjacency in factor order: every factor, and the loop factors alone
  std::vector<int32_t> adj((size_t)(2 * (n + 1)), 0);
  int32_t* off = adj.data();
  int32_t* loff = adj.data() + n + 1;
  for (const PgFactor& f : F) {
    ++off[f.i + 1];
    if (f.j >= 0) ++off[f.j + 1];
    if (f.loop) {
      ++loff[f.i + 1];
      ++loff[f.j + 1];
    }
  }
  for (int64_t m = 0; m < n; ++m) {
    if (off[m + 1] == 0) return FBR_ERR_STATE;  // a node no factor touches
    off[m + 1] += off[m];
    loff[m + 1] += loff[m];
  }
  const int64_t na = off[n], nla = loff[n], nloops = nla / 2;
  adj.resize((size_t)(2 * (n + 1) + na + nla + nloops));
  off = adj.data();
  loff = adj.data() + n + 1;
  int32_t* ent = adj.data() + 2 * (n + 1);
  int32_t* lent = ent + na;
  int32_t* loops = lent + nla;  // the loop factors' indices
  std::vector<int32_t> cur(off, off + n), lcur(loff, loff + n);
  for (int64_t k = 0; k < nf; ++k) {
    const PgFactor& f = F[k];
    ent[cur[f.i]++] = (int32_t)(2 * k);
    if (f.j >= 0) ent[cur[f.j]++] = (int32_t)(2 * k + 1);
    if (f.loop) {
      lent[lcur[f.i]++] = (int32_t)(2 * k);
      lent[lcur[f.j]++] = (int32_t)(2 * k + 1);
      *loops++ = (int32_t)k;
    }
  }
  int64_t tot = 0;
  const int nlev = pg_cr_levels(n, &tot);
  if (nlev > kPgMaxLevels || nf >= ((int64_t)1 << 30) || n >= ((int64_t)1 << 30)) return FBR_ERR_CAPACITY;
  const int64_t nbmax = (std::max(n, nf) + 255) / 256;
  const int64_t words = 24 * n + (kPgLin + 1) * nf + 36 * n + 12 * n + 24 * n + nbmax + tot * (36 * 5 + 12) + 2 * nf + 2 * nloops;
  int rc = grow(c->d_pg_work, words, 0, c->stream);
  if (!rc) rc = grow(c->d_pg_adj, (int64_t)adj.size(), 0, c->stream);
  if (!rc) rc = grow(c->d_pg_fac, std::max<int64_t>(nf, 1), 0, c->stream);
  if (rc) return rc;
  if (!c->d_pg_state && dalloc(c->d_pg_state, 1)) return FBR_ERR_HIP;
  if (!c->pg_flag && c->pg_flag.alloc(1)) return FBR_ERR_HIP;
  CK(hipMemcpyAsync(c->d_pg_adj, adj.data(), sizeof(int32_t) * adj.size(), hipMemcpyHostToDevice, c->stream));
  CK(hipMemcpyAsync(c->d_pg_fac, F.data(), sizeof(PgFactor) * nf, hipMemcpyHostToDevice, c->stream));
  CK(hipMemsetAsync(c->d_pg_state, 0, sizeof(PgState), c->stream));
  CK(fbr_sync(c->stream));  // the pageable copies
  double* w = c->d_pg_work;
  auto take = [&w](int64_t count) {
    double* p = w;
    w += count;
    return p;
  };
  PgArgs& a = pl->a;
  a = PgArgs{};
  a.n = n;
  a.nf = nf;
  a.fac = c->d_pg_fac;
  a.adj_off = c->d_pg_adj;
  a.ladj_off = c->d_pg_adj + n + 1;
  a.adj = c->d_pg_adj + 2 * (n + 1);
  a.ladj = a.adj + na;
  pl->X = take(12 * n);
  pl->Xt = take(12 * n);
  a.lin = take(kPgLin * nf);
  a.fcost = take(nf);
  a.D0 = take(36 * n);
  a.hd = take(6 * n);
  a.g = take(6 * n);
  a.x = take(6 * n);
  a.r = take(6 * n);
  a.p = take(6 * n);
  a.q = take(6 * n);
  a.partial = take(nbmax);
  a.st = c->d_pg_state;
  a.flag = c->pg_flag.dev();
  a.nlev = nlev;
  int64_t ln = n;
  for (int l = 0; l < nlev; ++l, ln = (ln + 1) / 2) {
    PgLevel& lv = a.lev[l];
    lv.n = ln;
    lv.D = take(36 * ln);
    lv.A = take(36 * ln);
    lv.L = take(36 * ln);
    lv.G = take(36 * ln);
    lv.H = take(36 * ln);
    lv.b = take(6 * ln);
    lv.x = take(6 * ln);
  }
  a.robust = robust;
  a.robust_scale = robust_scale;
  a.chi2 = take(nf);
  a.wt = take(nf);
  a.loops = a.ladj + nla;
  a.nloops = nloops;
  a.report = take(2 * nloops);
  return FBR_OK;
}

// One damped solve: every iteration is enqueued without waiting; the host only looks at the
// progress word k_pg_decide writes (and lets the device catch up when it is more than a few
// iterations behind), and iterations enqueued past the stop return at once.
void pg_pcg(fbr_ctx* c, const PgArgs& a, const fbr_pg_params& P) {
  const unsigned long long gen = (++c->pg_gen) & 0xFFFFFFFFull;
  const double tol2 = P.pcg_rel_tol * P.pcg_rel_tol;
  constexpr int kLead = 4;  // iterations the host may run ahead of the device
  TIMED(c, "pg_pcg", launch_pg_pcg_init(c->stream, a, gen));
  for (int it = 0; it < P.max_pcg_iterations; ++it) {
    if (run_ahead(c->pg_flag.host(), gen, it, kLead, debug_counters().flag_polls)) break;
    TIMED(c, "pg_pcg", launch_pg_pcg_iter(c->stream, a, it, P.max_pcg_iterations, tol2, gen));
  }
}

int pg_read_state(fbr_ctx* c, PgState* st) {
  CK(hipGetLastError());
  CK(hipMemcpyAsync(st, c->d_pg_state, sizeof(PgState), hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  return FBR_OK;
}

constexpr int kPgMargChunk = 48;                             // fbr_pg_marginal_params.rhs_chunk's default
constexpr int64_t kPgMargMaxWork = (int64_t)2 << 30;         // ... and max_work_bytes' (2 GiB)
constexpr int64_t kPgDirectMaxWorkMb = 2048;                 // fbr_pg_params.max_work_mb's default

// The direct solve (fbr_pg_params.solver = FBR_PG_SOLVER_DIRECT): W and C as the marginals build
// them, here over the optimise's own damped levels, and k_pg_direct.hip's three steps.
struct PgDirectPlan {
  PgMarg m;
  PgDirect d;
  int64_t chunk;
};

// The doubles of its work space: W, the chunk's b of every level and x of the levels after the
// first, C and z (in double: the products overflow an int64 long after the bound).  None without loops.
double pg_direct_words(int64_t n, int64_t K, int64_t* chunk) {
  const int64_t M = 6 * K;
  int64_t tot = 0;
  (void)pg_cr_levels(n, &tot);
  *chunk = std::min<int64_t>(kPgMargChunk, std::max<int64_t>(M, 1));
  if (M == 0) return 0.0;
  return 6.0 * (double)M * (double)n + 6.0 * (double)*chunk * (double)(2 * tot - n) + (double)M * (double)M + (double)M;
}

int pg_direct_prepare(fbr_ctx* c, const PgArgs& a, PgDirectPlan* dp) {
  const int64_t n = a.n, K = a.nloops, M = 6 * K;
  const int64_t words = (int64_t)pg_direct_words(n, K, &dp->chunk);
  PgMarg& m = dp->m;
  PgDirect& d = dp->d;
  m = PgMarg{};
  d = PgDirect{};
  d.n = n;
  d.M = M;
  d.fac = a.fac;
  d.lin = a.lin;
  d.y = a.lev[0].x;
  d.x = a.x;
  if (M == 0) return FBR_OK;  // the step is y: no W, no C
  const int rc = grow(c->d_pg_direct, words, 0, c->stream);
  if (rc) return rc;
  m.n = n;
  m.K = K;
  m.M = M;
  m.nlev = a.nlev;
  m.fac = a.fac;
  m.lin = a.lin;
  m.loops = a.loops;
  m.st = a.st;
  double* w = c->d_pg_direct;
  auto take = [&w](int64_t count) {
    double* p = w;
    w += count;
    return p;
  };
  for (int l = 0; l < a.nlev; ++l) {
    m.lev[l] = a.lev[l];
    m.lev[l].b = take(6 * dp->chunk * a.lev[l].n);
    m.lev[l].x = l ? take(6 * dp->chunk * a.lev[l].n) : nullptr;  // level 0's x is the chunk's part of W
  }
  m.W = take(6 * M * n);
  m.C = take(M * M);
  d.z = take(M);
  d.loops = m.loops;
  d.W = m.W;
  d.C = m.C;
  return FBR_OK;
}

// One damped solve after launch_pg_factor, into a.x; nothing waits.  A bad pivot of C sets
// PgState::numerical as one of T does.
void pg_direct(fbr_ctx* c, const PgArgs& a, const PgDirectPlan& dp) {
  const PgMarg& m = dp.m;
  TIMED(c, "pg_direct_y", launch_pg_direct_y(c->stream, a));
  for (int64_t c0 = 0; c0 < m.M; c0 += dp.chunk)
    TIMED(c, "pg_marg_solve", launch_pg_marg_solve(c->stream, m, c0, std::min(dp.chunk, m.M - c0)));
  TIMED(c, "pg_marg_c", launch_pg_marg_c(c->stream, m));
  TIMED(c, "pg_marg_chol", launch_pg_marg_chol(c->stream, m));
  TIMED(c, "pg_direct_z", launch_pg_direct_z(c->stream, dp.d));
  TIMED(c, "pg_direct_subst", launch_pg_direct_subst(c->stream, dp.d));
  TIMED(c, "pg_direct_delta", launch_pg_direct_delta(c->stream, dp.d));
}

int pg_run(fbr_ctx* c, const fbr_pg_params& P, fbr_pg_result* out) {
  const int64_t n = (int64_t)c->kf_poses.size();
  out->n_nodes = (int32_t)n;
  out->n_factors = (int32_t)c->pg_factors.size();
  for (const PgFactor& f : c->pg_factors) out->n_loop_factors += f.loop;
  out->lambda = P.lambda_init;
  c->pg_result_n = -1;
  if (n == 0) {
    out->status = FBR_PG_EMPTY;
    return FBR_OK;
  }
  const bool direct = P.solver == FBR_PG_SOLVER_DIRECT;
  if (direct) {  // before anything is allocated
    int64_t chunk = 0;
    const double mb = (double)(P.max_work_mb > 0 ? (int64_t)P.max_work_mb : kPgDirectMaxWorkMb);
    if (8.0 * pg_direct_words(n, out->n_loop_factors, &chunk) > mb * 1048576.0) return FBR_ERR_CAPACITY;
  }
  PgPlan pl;
  int rc = pg_prepare(c, n, P.robust, (double)P.robust_scale, &pl);
  if (rc) return rc;
  const PgArgs& a = pl.a;
  PgDirectPlan dp;
  if (direct && (rc = pg_direct_prepare(c, a, &dp))) return rc;
  std::vector<double> X0((size_t)(12 * n)), init((size_t)(6 * n));
  for (int64_t i = 0; i < n; ++i) {
    keypose_euler(c->kf_poses[i], &init[6 * i]);
    pg_pose_from_euler(&init[6 * i], &X0[12 * i]);
  }
  double *X = pl.X, *Xt = pl.Xt;
  CK(hipMemcpyAsync(X, X0.data(), sizeof(double) * 12 * n, hipMemcpyHostToDevice, c->stream));
  TIMED(c, "pg_linearize", launch_pg_linearize(c->stream, a, X, 1, 0));
  TIMED(c, "pg_assemble", launch_pg_assemble(c->stream, a));
  PgState st;
  rc = pg_read_state(c, &st);
  if (rc) return rc;
  double cost = st.cost[0], lambda = P.lambda_init;
  out->cost_initial = out->cost_final = cost;
  int status = -1;
  if (cost == 0.0) status = FBR_PG_CONVERGED;
  else if (!(cost < INFINITY)) status = FBR_PG_NUMERICAL;
  else if (P.max_iterations <= 0) status = FBR_PG_ITERATIONS;
  while (status < 0) {
    TIMED(c, "pg_factor", launch_pg_factor(c->stream, a, lambda));
    if (direct) pg_direct(c, a, dp);
    else pg_pcg(c, a, P);
    TIMED(c, "pg_retract", launch_pg_retract(c->stream, a, X, Xt));
    TIMED(c, "pg_linearize", launch_pg_linearize(c->stream, a, Xt, 0, 1));
    rc = pg_read_state(c, &st);
    if (rc) return rc;
    ++out->trials;
    out->pcg_iterations += st.iters;
    if (st.numerical) {
      status = FBR_PG_NUMERICAL;
      break;
    }
    const double trial = st.cost[1];
    if (trial < cost) {  // (false for a NaN)
      std::swap(X, Xt);
      const double dec = cost - trial, rel = dec / cost;
      cost = trial;
      ++out->iterations;
      lambda /= P.lambda_factor;
      if (rel < P.rel_cost_tol || dec < P.abs_cost_tol) status = FBR_PG_CONVERGED;
      else if (out->iterations >= P.max_iterations) status = FBR_PG_ITERATIONS;
      else {
        TIMED(c, "pg_linearize", launch_pg_linearize(c->stream, a, X, 1, 0));
        TIMED(c, "pg_assemble", launch_pg_assemble(c->stream, a));
      }
    } else {
      lambda *= P.lambda_factor;
      if (lambda > P.lambda_max) status = FBR_PG_STALLED;
    }
  }
  out->status = status;
  out->lambda = lambda;
  // fbr_pg_loop_weights: the per-factor values of the evaluation at the result poses.  That is the
  // last one enqueued unless it was a rejected trial's; then the result poses are evaluated again.
  const int64_t nf = a.nf;
  if (status == FBR_PG_NUMERICAL || status == FBR_PG_STALLED) {
    if (status == FBR_PG_NUMERICAL) CK(hipMemcpyAsync(X, X0.data(), sizeof(double) * 12 * n, hipMemcpyHostToDevice, c->stream));
    TIMED(c, "pg_linearize", launch_pg_linearize(c->stream, a, X, 0, 1));
  }
  const int64_t K = a.nloops;
  std::vector<double> report((size_t)(2 * K));
  if (K) {  // (a graph without loops launches and copies nothing more)
    TIMED(c, "pg_loop_report", launch_pg_loop_report(c->stream, a));
    CK(hipMemcpyAsync(report.data(), a.report, sizeof(double) * 2 * K, hipMemcpyDeviceToHost, c->stream));
  }
  c->pg_result.assign((size_t)(6 * n), 0.0);
  if (status == FBR_PG_NUMERICAL) {  // the optimised poses are the initial ones
    CK(fbr_sync(c->stream));
    c->pg_result = init;
  } else {
    out->cost_final = cost;
    CK(hipMemcpyAsync(X0.data(), X, sizeof(double) * 12 * n, hipMemcpyDeviceToHost, c->stream));
    CK(fbr_sync(c->stream));
    for (int64_t i = 0; i < n; ++i) {
      pg_euler_from_pose(&X0[12 * i], &c->pg_result[6 * i]);
      double A[12], D[12], phi[3];
      pg_pose_from_euler(&init[6 * i], A);
      pg_between(A, &X0[12 * i], D);
      pg_log(D, phi);
      const double* t = &X0[12 * i + 9];
      const double dx = t[0] - init[6 * i + 3], dy = t[1] - init[6 * i + 4], dz = t[2] - init[6 * i + 5];
      out->max_translation_change = std::max(out->max_translation_change, std::sqrt((dx * dx + dy * dy) + dz * dz));
      out->max_rotation_change =
          std::max(out->max_rotation_change, std::sqrt((phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2]));
    }
  }
  c->pg_loop_index.clear();
  for (int64_t k = 0; k < nf; ++k)
    if (c->pg_factors[k].loop) c->pg_loop_index.push_back((int32_t)k);
  c->pg_loop_chi2.assign(report.begin(), report.begin() + K);
  c->pg_loop_w.assign(report.begin() + K, report.end());
  c->pg_result_robust = P.robust;
  c->pg_result_scale = (double)P.robust_scale;
  c->pg_result_n = n;
  c->pg_result_nf = (int64_t)c->pg_factors.size();
  return FBR_OK;
}

// Sigma_ii of the requested nodes at the last optimise's poses (include/fbr.h "marginal
// covariances").  Everything is enqueued without waiting; the host reads the result and the status
// word once, at the end.
int pg_marginals_run(fbr_ctx* c, const fbr_pg_marginal_params& P, const int64_t* nodes, int64_t n_nodes, double* cov_out,
                     int64_t cap, fbr_pg_marginal_result* out) {
  const int64_t n = (int64_t)c->kf_poses.size();
  if (c->pg_result_n < 0 || c->pg_result_n != n || c->pg_result_nf != (int64_t)c->pg_factors.size()) return FBR_ERR_STATE;
  const int64_t n_out = nodes ? n_nodes : n;
  for (int64_t o = 0; nodes && o < n_out; ++o)
    if (nodes[o] < 0 || nodes[o] >= n) return FBR_ERR_INVALID_ARG;
  std::vector<int32_t> loops;
  for (size_t k = 0; k < c->pg_factors.size(); ++k)
    if (c->pg_factors[k].loop) loops.push_back((int32_t)k);
  const int64_t K = (int64_t)loops.size(), M = 6 * K;
  out->n_nodes = (int32_t)n;
  out->n_loop_factors = (int32_t)K;
  out->n_out = (int32_t)n_out;
  if (n_out > cap) return FBR_ERR_CAPACITY;
  if (n_out == 0) {
    out->status = FBR_PG_EMPTY;
    return FBR_OK;
  }
  int64_t tot = 0;
  (void)pg_cr_levels(n, &tot);
  const int64_t chunk = std::min(std::min<int64_t>(P.rhs_chunk > 0 ? P.rhs_chunk : kPgMargChunk, std::max<int64_t>(M, 1)),
                                 kPgMargMaxChunk);
  const int64_t max_work = P.max_work_bytes > 0 ? P.max_work_bytes : kPgMargMaxWork;
  // P and Q of every level, W, the chunk's b of every level and x of the levels after the first, C,
  // the output staging buffer (in double first: the products overflow an int64 long after the bound)
  const double words_d = 72.0 * (double)tot + 6.0 * (double)std::max<int64_t>(M, 1) * (double)n +
                         6.0 * (double)chunk * (double)(2 * tot - n) + (double)M * (double)M + 36.0 * (double)n_out;
  if (8.0 * words_d > (double)max_work) {
    out->work_bytes = words_d < 1e18 ? (int64_t)(8.0 * words_d) : INT64_MAX;
    return FBR_ERR_CAPACITY;
  }
  const int64_t words = 72 * tot + 6 * std::max<int64_t>(M, 1) * n + 6 * chunk * (2 * tot - n) + M * M + 36 * n_out;
  out->work_bytes = 8 * words;
  PgPlan pl;
  int rc = pg_prepare(c, n, c->pg_result_robust, c->pg_result_scale, &pl);
  if (rc) return rc;
  const PgArgs& a = pl.a;
  // the distinct requested nodes in ascending order: Y is computed in place, once per node
  std::vector<int64_t> idx;
  int64_t n_uniq = n_out;
  if (nodes) {
    idx.assign(nodes, nodes + n_out);
    std::vector<int64_t> u(idx);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    n_uniq = (int64_t)u.size();
    idx.insert(idx.end(), u.begin(), u.end());
  }
  rc = grow(c->d_pg_marg, words, 0, c->stream);
  if (!rc) rc = grow(c->d_pg_loops, std::max<int64_t>(K, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_pg_nodes, std::max<int64_t>((int64_t)idx.size(), 1), 0, c->stream);
  if (rc) return rc;
  std::vector<double> X0((size_t)(12 * n));
  for (int64_t i = 0; i < n; ++i) pg_pose_from_euler(&c->pg_result[6 * i], &X0[12 * i]);
  CK(hipMemcpyAsync(pl.X, X0.data(), sizeof(double) * 12 * n, hipMemcpyHostToDevice, c->stream));
  if (K) CK(hipMemcpyAsync(c->d_pg_loops, loops.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, c->stream));
  if (nodes) CK(hipMemcpyAsync(c->d_pg_nodes, idx.data(), sizeof(int64_t) * idx.size(), hipMemcpyHostToDevice, c->stream));
  CK(fbr_sync(c->stream));  // the pageable copies
  PgMarg m{};
  m.n = n;
  m.K = K;
  m.M = M;
  m.nlev = a.nlev;
  m.fac = a.fac;
  m.lin = a.lin;
  m.loops = c->d_pg_loops;
  m.st = a.st;
  double* w = c->d_pg_marg;
  auto take = [&w](int64_t count) {
    double* p = w;
    w += count;
    return p;
  };
  for (int l = 0; l < a.nlev; ++l) {
    m.lev[l] = a.lev[l];
    m.P[l] = take(36 * a.lev[l].n);
    m.Q[l] = take(36 * a.lev[l].n);
    m.lev[l].b = take(6 * chunk * a.lev[l].n);
    m.lev[l].x = l ? take(6 * chunk * a.lev[l].n) : nullptr;  // level 0's x is the chunk's part of W
  }
  m.W = take(6 * std::max<int64_t>(M, 1) * n);
  m.C = take(M * M);
  double* d_out = take(36 * n_out);
  const int64_t* d_nodes = nodes ? (const int64_t*)c->d_pg_nodes : nullptr;
  TIMED(c, "pg_linearize", launch_pg_linearize(c->stream, a, pl.X, 1, 0));
  TIMED(c, "pg_assemble", launch_pg_assemble(c->stream, a));
  TIMED(c, "pg_factor", launch_pg_factor(c->stream, a, 0.0));  // lambda = 0: D = D0 + 0 * hd, the undamped T0
  TIMED(c, "pg_selinv", launch_pg_selinv(c->stream, m));
  for (int64_t c0 = 0; c0 < M; c0 += chunk)
    TIMED(c, "pg_marg_solve", launch_pg_marg_solve(c->stream, m, c0, std::min(chunk, M - c0)));
  TIMED(c, "pg_marg_c", launch_pg_marg_c(c->stream, m));
  TIMED(c, "pg_marg_chol", launch_pg_marg_chol(c->stream, m));
  TIMED(c, "pg_marg_cov", launch_pg_marg_cov(c->stream, m, d_nodes ? d_nodes + n_out : nullptr, n_uniq, d_nodes, n_out, d_out));
  CK(hipGetLastError());
  PgState st;
  CK(hipMemcpyAsync(cov_out, d_out, sizeof(double) * 36 * n_out, hipMemcpyDeviceToHost, c->stream));
  CK(hipMemcpyAsync(&st, c->d_pg_state, sizeof(PgState), hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  out->status = FBR_PG_CONVERGED;
  if (st.numerical) {
    out->status = FBR_PG_NUMERICAL;
    std::memset(cov_out, 0, sizeof(double) * 36 * n_out);
  }
  return FBR_OK;
}

bool pg_params_ok(const fbr_pg_params* p) {
  return p && p->max_pcg_iterations >= 1 && p->rel_cost_tol >= 0.0 && p->abs_cost_tol >= 0.0 && p->pcg_rel_tol >= 0.0 &&
         p->lambda_init > 0.0 && p->lambda_init < INFINITY && p->lambda_factor > 1.0 && p->lambda_factor < INFINITY &&
         p->lambda_max > 0.0 && (p->solver == FBR_PG_SOLVER_PCG || p->solver == FBR_PG_SOLVER_DIRECT) &&
         (p->robust == FBR_PG_ROBUST_NONE ||
          ((p->robust == FBR_PG_ROBUST_HUBER || p->robust == FBR_PG_ROBUST_CAUCHY) && p->robust_scale > 0.0f &&
           p->robust_scale < INFINITY)) &&
         p->max_work_mb >= 0;
}

}  // namespace

extern "C" {

void fbr_pg_params_default(fbr_pg_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = 30;
  p->max_pcg_iterations = 200;
  p->rel_cost_tol = 1e-5;  // GTSAM's relativeErrorTol / absoluteErrorTol
  p->abs_cost_tol = 1e-5;
  p->pcg_rel_tol = 1e-8;
  p->lambda_init = 1e-5;
  p->lambda_factor = 10.0;
  p->lambda_max = 1e10;
}

int fbr_pg_reset(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  c->pg_factors.clear();
  return FBR_OK;
}

int fbr_pg_add_prior(fbr_ctx* c, int64_t node, const float pose[6], const double variances[6]) {
  if (!c || !pose || !variances || !node_ok(c, node) || !variances_ok(variances, 6)) return FBR_ERR_INVALID_ARG;
  PgFactor f{};
  f.type = kPgPrior;
  f.i = (int32_t)node;
  f.j = -1;
  double e[6];
  for (int k = 0; k < 6; ++k) {
    if (!std::isfinite(pose[k])) return FBR_ERR_INVALID_ARG;
    e[k] = (double)pose[k];
    f.w[k] = 1.0 / std::sqrt(variances[k]);
  }
  pg_pose_from_euler(e, f.Z);
  c->pg_factors.push_back(f);
  return FBR_OK;
}

int fbr_pg_add_between(fbr_ctx* c, int64_t i, int64_t j, const float between[16], const double variances[6]) {
  if (!c || !between || !variances) return FBR_ERR_INVALID_ARG;
  double Z[12];
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) Z[3 * r + q] = (double)between[4 * r + q];
    Z[9 + r] = (double)between[4 * r + 3];
  }
  return add_between(c, i, j, Z, variances);
}

int fbr_pg_add_between_poses(fbr_ctx* c, int64_t i, int64_t j, const float pose_i[6], const float pose_j[6],
                             const double variances[6]) {
  if (!c || !pose_i || !pose_j || !variances) return FBR_ERR_INVALID_ARG;
  double ei[6], ej[6], A[12], B[12], Z[12];
  for (int k = 0; k < 6; ++k) {
    ei[k] = (double)pose_i[k];
    ej[k] = (double)pose_j[k];
  }
  pg_pose_from_euler(ei, A);
  pg_pose_from_euler(ej, B);
  pg_between(A, B, Z);
  return add_between(c, i, j, Z, variances);
}

int fbr_pg_add_gps(fbr_ctx* c, int64_t node, const double xyz[3], const double variances[3]) {
  if (!c || !xyz || !variances || !node_ok(c, node) || !variances_ok(variances, 3)) return FBR_ERR_INVALID_ARG;
  PgFactor f{};
  f.type = kPgGps;
  f.i = (int32_t)node;
  f.j = -1;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(xyz[k])) return FBR_ERR_INVALID_ARG;
    f.Z[9 + k] = xyz[k];
    f.w[3 + k] = 1.0 / std::sqrt(variances[k]);
  }
  c->pg_factors.push_back(f);
  return FBR_OK;
}

int fbr_pg_add_loop(fbr_ctx* c, const fbr_loop_result* r, int* added) {
  if (added) *added = 0;
  if (!c || !r) return FBR_ERR_INVALID_ARG;
  if (r->status != FBR_LOOP_CLOSED) return FBR_OK;
  const double score = (double)(float)r->icp.fitness;  // noiseScore (:746)
  const double var[6] = {score, score, score, score, score, score};
  const int rc = fbr_pg_add_between(c, r->latest_id, r->closest_id, r->between, var);
  if (!rc && added) *added = 1;
  return rc;
}

int fbr_pg_factor_count(fbr_ctx* c, int64_t* n) {
  if (!c || !n) return FBR_ERR_INVALID_ARG;
  *n = (int64_t)c->pg_factors.size();
  return FBR_OK;
}

int fbr_pg_optimize(fbr_ctx* c, const fbr_pg_params* p, fbr_pg_result* out) {
  if (!c || !out || !pg_params_ok(p)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  std::memset(out, 0, sizeof(*out));
  return pg_run(c, *p, out);
}

int fbr_pg_poses(fbr_ctx* c, double* poses_out, int64_t cap, int64_t* n) {
  if (!c || !n || cap < 0 || (cap && !poses_out)) return FBR_ERR_INVALID_ARG;
  if (c->pg_result_n < 0) return FBR_ERR_STATE;
  *n = c->pg_result_n;
  if (cap < c->pg_result_n) return FBR_ERR_CAPACITY;
  std::memcpy(poses_out, c->pg_result.data(), sizeof(double) * 6 * c->pg_result_n);
  return FBR_OK;
}

int fbr_pg_loop_weights(fbr_ctx* c, int32_t* factor_index_out, double* chi2_out, double* weight_out, int64_t cap, int64_t* n) {
  if (!c || !n || cap < 0 || (cap && (!factor_index_out || !chi2_out || !weight_out))) return FBR_ERR_INVALID_ARG;
  if (c->pg_result_n < 0) return FBR_ERR_STATE;
  const int64_t K = (int64_t)c->pg_loop_index.size();
  *n = K;
  if (cap < K) return FBR_ERR_CAPACITY;
  if (K) {
    std::memcpy(factor_index_out, c->pg_loop_index.data(), sizeof(int32_t) * K);
    std::memcpy(chi2_out, c->pg_loop_chi2.data(), sizeof(double) * K);
    std::memcpy(weight_out, c->pg_loop_w.data(), sizeof(double) * K);
  }
  return FBR_OK;
}

void fbr_pg_marginal_params_default(fbr_pg_marginal_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));  // rhs_chunk = 0 and max_work_bytes = 0: the defaults (48 columns, 2 GiB)
}

int fbr_pg_marginals(fbr_ctx* c, const fbr_pg_marginal_params* p, const int64_t* nodes, int64_t n_nodes, double* cov_out,
                     int64_t cap, fbr_pg_marginal_result* out) {
  if (!c || !p || !out || cap < 0 || (cap && !cov_out) || (nodes && n_nodes < 0) || p->rhs_chunk < 0 ||
      p->max_work_bytes < 0)
    return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  std::memset(out, 0, sizeof(*out));
  return pg_marginals_run(c, *p, nodes, n_nodes, cov_out, cap, out);
}

int fbr_pg_gps_gate(fbr_ctx* c, double pose_cov_threshold, int* wanted, double cov_xy[2]) {
  if (!c || !wanted || !(pose_cov_threshold == pose_cov_threshold)) return FBR_ERR_INVALID_ARG;
  fbr_pg_marginal_params p;
  fbr_pg_marginal_params_default(&p);
  fbr_pg_marginal_result r;
  const int64_t last = (int64_t)c->kf_poses.size() - 1;
  if (last < 0) return FBR_ERR_STATE;
  double cov[36];
  const int rc = fbr_pg_marginals(c, &p, &last, 1, cov, 1, &r);
  if (rc) return rc;
  const bool known = r.status == FBR_PG_CONVERGED;  // no covariance: unbounded, and the factor is wanted
  *wanted = known ? pg_gps_gate_wanted(cov, pose_cov_threshold) : 1;
  if (cov_xy) {
    cov_xy[0] = known ? cov[6 * 3 + 3] : INFINITY;
    cov_xy[1] = known ? cov[6 * 4 + 4] : INFINITY;
  }
  return FBR_OK;
}

int fbr_pg_apply(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (c->pg_result_n < 0 || c->pg_result_n != (int64_t)c->kf_poses.size()) return FBR_ERR_STATE;
  for (int64_t i = 0; i < c->pg_result_n; ++i) {  // correctPoses (:1746-1757)
    const double* e = &c->pg_result[6 * i];
    fbr_keypose p = c->kf_poses[i];
    p.roll = (float)e[0];
    p.pitch = (float)e[1];
    p.yaw = (float)e[2];
    p.x = (float)e[3];
    p.y = (float)e[4];
    p.z = (float)e[5];
    const int rc = fbr_keyframes_set_pose(c, i, &p);
    if (rc) return rc;
  }
  return FBR_OK;
}

}  // extern "C"
