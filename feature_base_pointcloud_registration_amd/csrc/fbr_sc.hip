// fbr_sc.hip — scan-context place recognition (include/fbr.h, "place recognition"): the descriptor
// store over the keyframe pools, the exhaustive search (k_scancontext.hip), the top-k selection on
// the candidates' records, and the loop closure that takes its candidate and its source pose from a
// match.  The host never touches a descriptor: per query it reads the N 16-byte candidate records
// from the pinned result block, one device-to-host copy.
#include "fbr_ctx.h"
#include "fbr_sc.h"

namespace {

bool sc_params_ok(const fbr_sc_params* sp) {
  return sp && sp->n_ring >= 1 && sp->n_ring <= kScMaxRing && sp->n_sector >= 2 && sp->n_sector <= kScMaxSector &&
         sp->max_radius > 0.0f && std::isfinite(sp->max_radius) && std::isfinite(sp->lidar_height) &&
         sp->dist_threshold >= 0.0f;
}

bool same_descriptor(const fbr_sc_params& a, const fbr_sc_params& b) {
  return a.n_ring == b.n_ring && a.n_sector == b.n_sector && a.max_radius == b.max_radius &&
         a.lidar_height == b.lidar_height;
}

int sc_query_slot(fbr_ctx* c) {
  if (!c->d_sc_q && dalloc(c->d_sc_q, (size_t)kScMaxRing * kScMaxSector)) return FBR_ERR_HIP;
  if (!c->d_sc_qn && dalloc(c->d_sc_qn, (size_t)kScMaxSector)) return FBR_ERR_HIP;
  return FBR_OK;
}

ScPools sc_pools(fbr_ctx* c) {
  ScPools p;
  p.p[0] = c->d_kf_c;
  p.p[1] = c->d_kf_s;
  p.p[2] = c->d_sc_cloud;
  return p;
}

// Zeroes the slots [slot0, slot0 + nslots) of `desc`, describes `segs` into them and writes their
// column norms; returns with the stream drained (the segments are copied from pageable memory).
int sc_describe_segs(fbr_ctx* c, const fbr_sc_params& sp, const std::vector<ScSeg>& segs, uint32_t* desc, double* norms,
                     int64_t slot0, int64_t nslots) {
  const int64_t cells = (int64_t)sp.n_ring * sp.n_sector;
  int64_t max_cnt = 0;
  for (const ScSeg& g : segs) max_cnt = std::max(max_cnt, g.count);
  if (max_cnt > kScMaxCloud || segs.size() > (size_t)INT32_MAX) return FBR_ERR_CAPACITY;
  const int rc = grow(c->d_sc_segs, std::max<int64_t>((int64_t)segs.size(), 1), 0, c->stream);
  if (rc) return rc;
  CK(hipMemsetAsync(desc + slot0 * cells, 0, sizeof(uint32_t) * cells * nslots, c->stream));
  if (!segs.empty())
    CK(hipMemcpyAsync(c->d_sc_segs, segs.data(), sizeof(ScSeg) * segs.size(), hipMemcpyHostToDevice, c->stream));
  TIMED(c, "sc_describe", launch_sc_describe(c->stream, sc_pools(c), c->d_sc_segs, (int)segs.size(), max_cnt, sp.n_ring,
                                             sp.n_sector, sp.max_radius, sp.lidar_height, desc));
  TIMED(c, "sc_norms", launch_sc_norms(c->stream, desc + slot0 * cells, nslots, sp.n_ring, sp.n_sector,
                                       norms + slot0 * sp.n_sector));
  CK(hipGetLastError());
  CK(fbr_sync(c->stream));
  return FBR_OK;
}

// The descriptor of a host cloud into the query slot.
int sc_describe_query(fbr_ctx* c, const fbr_sc_params& sp, const fbr_point_xyzi* corner, int64_t n_corner,
                      const fbr_point_xyzi* surf, int64_t n_surf) {
  int rc = sc_query_slot(c);
  if (!rc) rc = grow(c->d_sc_cloud, std::max<int64_t>(n_corner + n_surf, 1), 0, c->stream);
  if (rc) return rc;
  if (n_corner) CK(hipMemcpyAsync(c->d_sc_cloud, corner, sizeof(float4) * n_corner, hipMemcpyHostToDevice, c->stream));
  if (n_surf)
    CK(hipMemcpyAsync(c->d_sc_cloud + n_corner, surf, sizeof(float4) * n_surf, hipMemcpyHostToDevice, c->stream));
  std::vector<ScSeg> segs;
  if (n_corner + n_surf) segs.push_back(ScSeg{0, n_corner + n_surf, 0, 2, 0});
  return sc_describe_segs(c, sp, segs, c->d_sc_q, c->d_sc_qn, 0, 1);
}

int sc_update(fbr_ctx* c, const fbr_sc_params& sp, int64_t* n_described) {
  if (c->sc_n && !same_descriptor(c->sc_P, sp)) c->sc_n = 0;
  c->sc_P = sp;
  const int64_t N = (int64_t)c->kf_poses.size(), cells = (int64_t)sp.n_ring * sp.n_sector;
  if (c->sc_n > N) c->sc_n = 0;
  const int64_t first = c->sc_n;
  if (n_described) *n_described = N - first;
  if (N == first) return FBR_OK;
  int rc = grow(c->d_sc_desc, N * cells, first * cells, c->stream);
  if (!rc) rc = grow(c->d_sc_norm, N * sp.n_sector, first * sp.n_sector, c->stream);
  if (rc) return rc;
  std::vector<ScSeg> segs;
  segs.reserve((size_t)(2 * (N - first)));
  for (int64_t k = first; k < N; ++k) {
    if (c->kf_c_cnt[k]) segs.push_back(ScSeg{c->kf_c_off[k], c->kf_c_cnt[k], k, 0, 0});
    if (c->kf_s_cnt[k]) segs.push_back(ScSeg{c->kf_s_off[k], c->kf_s_cnt[k], k, 1, 0});
  }
  rc = sc_describe_segs(c, sp, segs, c->d_sc_desc, c->d_sc_norm, first, N - first);
  if (rc) return rc;
  c->sc_n = N;
  return FBR_OK;
}

// The query (device descriptor + norms) against the stored descriptors [0, n): the records arrive
// in h_sc_rec, the one copy of the query.
int sc_search(fbr_ctx* c, const fbr_sc_params& sp, const uint32_t* d_q, const double* d_qn, int64_t n) {
  if (n <= 0) return FBR_OK;
  int rc = grow(c->d_sc_rec, n, 0, c->stream);
  if (rc) return rc;
  if (!c->h_sc_rec.grow(n, 0, [](ScRec*, const ScRec*, int64_t) { return true; })) return alloc_failed();
  TIMED(c, "sc_search", launch_sc_search(c->stream, d_q, d_qn, c->d_sc_desc, c->d_sc_norm, n, sp.n_ring, sp.n_sector,
                                         c->d_sc_rec));
  CK(hipGetLastError());
  CK(hipMemcpyAsync(c->h_sc_rec, c->d_sc_rec, sizeof(ScRec) * n, hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  return FBR_OK;
}

bool rec_before(const ScRec* rec, int64_t a, int64_t b) {  // (distance, keyframe index) ascending
  return rec[a].distance < rec[b].distance || (rec[a].distance == rec[b].distance && a < b);
}

void sc_fill_match(const fbr_ctx* c, const fbr_sc_params& sp, int64_t k, fbr_sc_match* m) {
  std::memset(m, 0, sizeof(*m));
  const ScRec& r = c->h_sc_rec.get()[k];
  m->keyframe = (int32_t)k;
  m->shift = r.shift;
  m->distance = r.distance;
  const fbr_keypose& kp = c->kf_poses[k];
  const float stored[6] = {kp.roll, kp.pitch, kp.yaw, kp.x, kp.y, kp.z};
  const float turn[6] = {0.0f, 0.0f, (float)((double)r.shift * 6.283185307179586 / (double)sp.n_sector), 0.0f, 0.0f, 0.0f};
  float K[16], R[16], G[16];
  fbr_affine_from_pose(stored, K);
  fbr_affine_from_pose(turn, R);
  affine_mul(K, R, G);
  fbr_pose_from_affine(G, m->pose_guess);
}

// fbr_sc_detect_loop_closure's body: the best eligible candidate in *best (-1: none), found or not
int sc_detect(fbr_ctx* c, double stamp, const fbr_loop_params* lp, const fbr_sc_params& sp, int64_t* best) {
  *best = -1;
  int rc = sc_update(c, sp, nullptr);
  if (rc) return rc;
  const int64_t N = c->sc_n, cells = (int64_t)sp.n_ring * sp.n_sector;
  if (N < 2) return FBR_OK;
  rc = sc_search(c, sp, c->d_sc_desc + (N - 1) * cells, c->d_sc_norm + (N - 1) * sp.n_sector, N - 1);
  if (rc) return rc;
  const ScRec* rec = c->h_sc_rec.get();
  for (int64_t i = 0; i < N - 1; ++i) {
    if (!(std::fabs(c->kf_poses[i].time - stamp) > (double)lp->search_time_diff)) continue;
    if (*best < 0 || rec_before(rec, i, *best)) *best = i;
  }
  return FBR_OK;
}

}  // namespace

extern "C" {

void fbr_sc_params_default(fbr_sc_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_ring = 20;
  p->n_sector = 60;
  p->max_radius = 80.0f;
  p->lidar_height = 2.0f;
  p->dist_threshold = 0.2f;  // between the synthetic fixtures' matches and non-matches; unmeasured on real data
}

int fbr_sc_describe(fbr_ctx* c, const fbr_sc_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                    const fbr_point_xyzi* surf, int64_t n_surf, float* desc_out) {
  if (!c || !sc_params_ok(sp) || n_corner < 0 || n_surf < 0 || (n_corner && !corner) || (n_surf && !surf))
    return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  const int rc = sc_describe_query(c, *sp, corner, n_corner, surf, n_surf);
  if (rc) return rc;
  if (desc_out)
    CK(fbr_memcpy_sync(desc_out, c->d_sc_q, sizeof(float) * sp->n_ring * sp->n_sector, hipMemcpyDeviceToHost));
  return FBR_OK;
}

int fbr_sc_update(fbr_ctx* c, const fbr_sc_params* sp, int64_t* n_described) {
  if (!c || !sc_params_ok(sp)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  return sc_update(c, *sp, n_described);
}

int fbr_sc_descriptor(fbr_ctx* c, int64_t keyframe, float* desc_out) {
  if (!c || !desc_out || keyframe < 0) return FBR_ERR_INVALID_ARG;
  if (keyframe >= c->sc_n || c->sc_n > (int64_t)c->kf_poses.size()) return FBR_ERR_STATE;
  CK(enter(c));
  const int64_t cells = (int64_t)c->sc_P.n_ring * c->sc_P.n_sector;
  CK(fbr_memcpy_sync(desc_out, c->d_sc_desc + keyframe * cells, sizeof(float) * cells, hipMemcpyDeviceToHost));
  return FBR_OK;
}

int fbr_sc_query(fbr_ctx* c, const fbr_sc_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                 const fbr_point_xyzi* surf, int64_t n_surf, int k, fbr_sc_match* out, int* n_out) {
  if (!c || !sc_params_ok(sp) || n_corner < 0 || n_surf < 0 || (n_corner && !corner) || (n_surf && !surf) || k < 1 ||
      k > kScMaxK || !out || !n_out)
    return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  *n_out = 0;
  int rc = sc_update(c, *sp, nullptr);
  if (rc || c->sc_n == 0) return rc;
  rc = sc_describe_query(c, *sp, corner, n_corner, surf, n_surf);
  if (!rc) rc = sc_search(c, *sp, c->d_sc_q, c->d_sc_qn, c->sc_n);
  if (rc) return rc;
  const ScRec* rec = c->h_sc_rec.get();
  std::vector<int64_t> order((size_t)c->sc_n);
  for (int64_t i = 0; i < c->sc_n; ++i) order[(size_t)i] = i;
  const int64_t m = std::min<int64_t>(k, c->sc_n);
  std::partial_sort(order.begin(), order.begin() + m, order.end(),
                    [rec](int64_t a, int64_t b) { return rec_before(rec, a, b); });
  for (int64_t i = 0; i < m; ++i) sc_fill_match(c, *sp, order[(size_t)i], &out[i]);
  *n_out = (int)m;
  return FBR_OK;
}

int fbr_sc_detect_loop_closure(fbr_ctx* c, double stamp, const fbr_loop_params* lp, const fbr_sc_params* sp,
                               int32_t* latest_id, int32_t* closest_id, fbr_sc_match* match) {
  if (!c || !lp || !sc_params_ok(sp) || !latest_id || !closest_id) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  *latest_id = *closest_id = -1;
  if (match) {
    std::memset(match, 0, sizeof(*match));
    match->keyframe = -1;
  }
  int64_t best;
  const int rc = sc_detect(c, stamp, lp, *sp, &best);
  if (rc || best < 0) return rc;
  if (match) sc_fill_match(c, *sp, best, match);
  if (c->h_sc_rec.get()[best].distance < (double)sp->dist_threshold) {
    *latest_id = (int32_t)(c->sc_n - 1);
    *closest_id = (int32_t)best;
  }
  return FBR_OK;
}

int fbr_perform_loop_closure_sc(fbr_ctx* c, double stamp, const fbr_loop_params* lp, const fbr_sc_params* sp,
                                fbr_loop_result* out, fbr_sc_match* match) {
  if (!c || !out || !loop_params_ok(lp) || !sc_params_ok(sp)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  std::memset(out, 0, sizeof(*out));
  out->status = FBR_LOOP_NO_CANDIDATE;
  out->latest_id = out->closest_id = -1;
  fbr_sc_match m;
  std::memset(&m, 0, sizeof(m));
  m.keyframe = -1;
  int64_t best;
  const int rc = sc_detect(c, stamp, lp, *sp, &best);
  if (!rc && best >= 0) sc_fill_match(c, *sp, best, &m);
  if (match) *match = m;
  if (rc || best < 0 || !(m.distance < (double)sp->dist_threshold)) return rc;
  return loop_perform(c, lp, (int32_t)(c->sc_n - 1), (int32_t)best, m.pose_guess, out);
}

}  // extern "C"
