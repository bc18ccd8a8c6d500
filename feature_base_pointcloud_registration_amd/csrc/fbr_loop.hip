// fbr_loop.hip — loop closure on the keyframe store: the candidate search, the ICP driver
// (k_icp.hip) and fbr_selftest_nn1.
#include "fbr_ctx.h"

// ---------------------------------------------------------------------------------------------
// loop closure: detectLoopClosure / performLoopClosure (mapOptmization.h:606-782), k_icp.hip
// ---------------------------------------------------------------------------------------------
namespace {

// detectLoopClosure's candidate (:616-644): radius search around the last key pose (the conventions
// of extractNearby above), the first hit older than search_time_diff.
bool loop_candidate(const fbr_ctx* c, double stamp, const fbr_loop_params* lp, int32_t* latest, int32_t* closest) {
  *latest = *closest = -1;
  const int64_t N = (int64_t)c->kf_poses.size();
  if (N == 0) return false;
  const fbr_keypose& back = c->kf_poses.back();
  const float r2 = (float)((double)lp->search_radius * (double)lp->search_radius);
  std::vector<std::pair<float, int64_t>> hits;
  for (int64_t i = 0; i < N; ++i) {
    const fbr_keypose& q = c->kf_poses[i];
    float d = 0.0f, diff;
    diff = back.x - q.x; d += diff * diff;
    diff = back.y - q.y; d += diff * diff;
    diff = back.z - q.z; d += diff * diff;
    if (d < r2) hits.emplace_back(d, i);
  }
  std::stable_sort(hits.begin(), hits.end(),
                   [](const std::pair<float, int64_t>& a, const std::pair<float, int64_t>& b) { return a.first < b.first; });
  int64_t cand = -1;
  for (const auto& h : hits)
    if (std::fabs(c->kf_poses[h.second].time - stamp) > (double)lp->search_time_diff) {  // :632
      cand = h.second;
      break;
    }
  if (cand < 0 || cand == N - 1) return false;  // :639-644
  *latest = (int32_t)(N - 1);
  *closest = (int32_t)cand;
  return true;
}

// Scratch, the grid over the target and the argument block of one ICP call; leaves the state
// initialised on the stream.  cell_hint: the target's point spacing (a VoxelGrid leaf).
int icp_prepare(fbr_ctx* c, const float4* d_src, int64_t ns, const float4* d_tgt, int64_t nt, float cell_hint, IcpArgs* a) {
  if (ns >= ((int64_t)1 << 30) || nt >= ((int64_t)1 << 28)) return FBR_ERR_CAPACITY;
  const int64_t nblk = (ns + 255) / 256;
  int rc = grow(c->d_icp_x, std::max<int64_t>(ns, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_icp_key, std::max<int64_t>(ns, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_icp_far, ns + 1, 0, c->stream);
  if (!rc) rc = grow(c->d_icp_partial, std::max<int64_t>(nblk, 1) * kIcpSums, 0, c->stream);
  if (rc) return rc;
  if (!c->d_icp_state && !c->d_icp_state.alloc_bytes(sizeof(IcpState) + sizeof(fbr_icp_result))) return alloc_failed();
  if (!c->icp_flag && c->icp_flag.alloc(1)) return FBR_ERR_HIP;
  *a = IcpArgs{};
  a->src = d_src;
  a->x = c->d_icp_x;
  a->n = ns;
  a->tgt = d_tgt;
  a->nt = nt;
  a->key = c->d_icp_key;
  a->far_list = c->d_icp_far;
  a->far_cnt = c->d_icp_far + ns;
  a->partial = c->d_icp_partial;
  a->st = c->d_icp_state;
  a->flag = c->icp_flag.dev();
  a->gate2 = INFINITY;
  // cubic cells of the power of two at or above the hint; doubled while outliers would make the
  // box sparse or mostly empty, and without a grid (every query brute force) if that does not end
  if (nt > 0) {
    float cell = 1.0f / 64.0f;
    const float hint = cell_hint > 0.0f ? cell_hint : 0.5f;
    while (cell < hint && cell < 64.0f) cell *= 2.0f;
    for (int tries = 0; tries < 8; ++tries, cell *= 2.0f) {
      rc = grid_build_device(c->stream, c->arena, d_tgt, nt, 1.0f / cell, 1.0f / cell, false, c->icp_grid);
      if (rc == FBR_ERR_CAPACITY) {  // (nt is in range: the box has too many cells even for chunks)
        rc = FBR_OK;
        continue;
      }
      if (rc) return rc;
      const GridDesc& g = c->icp_grid.g;
      if (!g.sparse && (int64_t)g.n_cells <= std::max<int64_t>((int64_t)1 << 22, 64 * nt)) {
        a->use_grid = 1;
        break;
      }
    }
  }
  a->grid = c->icp_grid.view();
  launch_icp_init(c->stream, *a);
  return FBR_OK;
}

// icp.align + getFitnessScore on device clouds.  Every iteration is enqueued without waiting; the
// host only looks at the stop word k_icp_solve writes (and lets the device catch up when it is more
// than a few iterations behind), and iterations enqueued past the stop return at once.
int icp_run(fbr_ctx* c, const float4* d_src, int64_t ns, const float4* d_tgt, int64_t nt, const fbr_icp_params& ip,
            float cell_hint, fbr_icp_result* out) {
  IcpArgs a;
  const int rc = icp_prepare(c, d_src, ns, d_tgt, nt, cell_hint, &a);
  if (rc) return rc;
  const double md = (double)ip.max_correspondence_distance;
  a.gate2 = md * md;
  const unsigned long long gen = (++c->icp_gen) & 0xFFFFFFFFull;
  constexpr int kLead = 4;  // iterations the host may run ahead of the device
  for (int it = 0; it < std::max(1, ip.max_iterations); ++it) {
    if (run_ahead(c->icp_flag.host(), gen, it, kLead, debug_counters().flag_polls)) break;
    TIMED(c, "icp_nn", launch_icp_nn(c->stream, a, 0, it == 0));
    TIMED(c, "icp_nn_far", launch_icp_far(c->stream, a, 0));
    TIMED(c, "icp_solve", launch_icp_solve(c->stream, a, ip.max_iterations, ip.transformation_epsilon,
                                           ip.euclidean_fitness_epsilon, gen));
  }
  IcpArgs f = a;  // getFitnessScore: final * source against the target, no gate
  f.gate2 = INFINITY;
  fbr_icp_result* d_res = reinterpret_cast<fbr_icp_result*>(c->d_icp_state + 1);
  TIMED(c, "icp_nn", launch_icp_nn(c->stream, f, 1, 0));
  TIMED(c, "icp_nn_far", launch_icp_far(c->stream, f, 1));
  TIMED(c, "icp_solve", launch_icp_finish(c->stream, f, d_res));
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, d_res, sizeof(fbr_icp_result), hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  return FBR_OK;
}

int icp_upload(fbr_ctx* c, GrowDev<float4>& dst, const fbr_point_xyzi* src, int64_t n) {
  const int rc = grow(dst, std::max<int64_t>(n, 1), 0, c->stream);
  if (rc) return rc;
  if (n) CK(hipMemcpyAsync(dst, src, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
  CK(fbr_sync(c->stream));
  return FBR_OK;
}

bool icp_params_ok(const fbr_icp_params& ip) {
  return ip.max_correspondence_distance >= 0.0f && ip.transformation_epsilon >= 0.0 && ip.euclidean_fitness_epsilon >= 0.0;
}

// gtsam::Pose3(Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)) as a row-major 3x4, in double
void pose3_double(const float p[6], double m[12]) {
  const double cr = std::cos((double)p[0]), sr = std::sin((double)p[0]), cp = std::cos((double)p[1]),
               sp = std::sin((double)p[1]), cy = std::cos((double)p[2]), sy = std::sin((double)p[2]);
  m[0] = cy * cp; m[1] = cy * sp * sr - sy * cr; m[2] = cy * sp * cr + sy * sr; m[3] = (double)p[3];
  m[4] = sy * cp; m[5] = sy * sp * sr + cy * cr; m[6] = sy * sp * cr - cy * sr; m[7] = (double)p[4];
  m[8] = -sp;     m[9] = cp * sr;                m[10] = cp * cr;               m[11] = (double)p[5];
}

}  // namespace

namespace fbr {
namespace internal {

bool loop_params_ok(const fbr_loop_params* lp) {
  return lp && lp->search_radius >= 0 && lp->search_num >= 0 && lp->icp_leaf_size >= 0 && icp_params_ok(lp->icp);
}

int loop_perform(fbr_ctx* c, const fbr_loop_params* lp, int32_t latest, int32_t closest, const float* latest_pose,
                 fbr_loop_result* out) {
  // latestKeyFrameCloud (:650-651) and nearHistoryKeyFrameCloud (:656-665): transformPointCloud of
  // the stored clouds, corner then surf per keyframe.  Segments by pool: [source corner, target
  // corners..., source surf, target surfs...]
  std::vector<KfSeg> cseg, sseg;
  int64_t n_src = 0, n_raw = 0, max_cnt = 0;
  auto add = [&](int k, int64_t* off, const float* tr_override) {
    const fbr_keypose& pose = c->kf_poses[k];
    const float tr[6] = {pose.roll, pose.pitch, pose.yaw, pose.x, pose.y, pose.z};
    float m[16];
    fbr_affine_from_pose(tr_override ? tr_override : tr, m);
    KfSeg g;
    for (int q = 0; q < 12; ++q) g.T[q] = m[q];
    g.src = c->kf_c_off[k];
    g.count = c->kf_c_cnt[k];
    g.dst = *off;
    *off += g.count;
    cseg.push_back(g);
    max_cnt = std::max(max_cnt, g.count);
    g.src = c->kf_s_off[k];
    g.count = c->kf_s_cnt[k];
    g.dst = *off;
    *off += g.count;
    sseg.push_back(g);
    max_cnt = std::max(max_cnt, g.count);
  };
  add(latest, &n_src, latest_pose);
  for (int64_t k = (int64_t)closest - lp->search_num; k <= (int64_t)closest + lp->search_num; ++k) {
    if (k < 0 || k > latest) continue;  // :659
    add((int)k, &n_raw, nullptr);
  }
  const int nseg = (int)cseg.size();  // 1 source segment + the target's, per pool
  std::vector<KfSeg> segs(cseg);
  segs.insert(segs.end(), sseg.begin(), sseg.end());
  int rc = grow(c->d_icp_src, std::max<int64_t>(n_src, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_icp_raw, std::max<int64_t>(n_raw, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_icp_tgt, std::max<int64_t>(n_raw, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_icp_segs, (int64_t)segs.size(), 0, c->stream);
  if (rc) return rc;
  CK(hipMemcpyAsync(c->d_icp_segs, segs.data(), sizeof(KfSeg) * segs.size(), hipMemcpyHostToDevice, c->stream));
  launch_kf_transform(c->stream, c->d_kf_c, c->d_icp_segs, 1, max_cnt, c->d_icp_src);
  launch_kf_transform(c->stream, c->d_kf_s, c->d_icp_segs + nseg, 1, max_cnt, c->d_icp_src);
  launch_kf_transform(c->stream, c->d_kf_c, c->d_icp_segs + 1, nseg - 1, max_cnt, c->d_icp_raw);
  launch_kf_transform(c->stream, c->d_kf_s, c->d_icp_segs + nseg + 1, nseg - 1, max_cnt, c->d_icp_raw);
  CK(hipGetLastError());
  CK(fbr_sync(c->stream));  // the pageable copy of `segs`
  // downSizeFilterICP (:698-701)
  const float leaf = lp->icp_leaf_size > 0.0f ? lp->icp_leaf_size : c->P.mapping_surf_leaf_size;
  int64_t n_tgt = 0;
  rc = voxel_grid_dev(c, c->d_icp_raw, n_raw, leaf, c->d_icp_tgt, &n_tgt);
  if (rc) return rc;
  rc = icp_run(c, c->d_icp_src, n_src, c->d_icp_tgt, n_tgt, lp->icp, leaf, &out->icp);
  if (rc) return rc;
  out->latest_id = latest;
  out->closest_id = closest;
  out->n_source = (int32_t)n_src;
  out->n_target = (int32_t)n_tgt;
  out->status = !out->icp.converged ? FBR_LOOP_NOT_CONVERGED
                : out->icp.fitness > (double)lp->fitness_score ? FBR_LOOP_REJECTED_FITNESS
                                                               : FBR_LOOP_CLOSED;  // :715
  // tCorrect = correctionLidarFrame * tWrong (:729-741), Eigen::Affine3f product in float
  const fbr_keypose& kl = c->kf_poses[latest];
  const fbr_keypose& kc = c->kf_poses[closest];
  const float stored[6] = {kl.roll, kl.pitch, kl.yaw, kl.x, kl.y, kl.z};
  float W[16], G[16];
  fbr_affine_from_pose(latest_pose ? latest_pose : stored, W);
  affine_mul(out->icp.transform, W, G);
  fbr_pose_from_affine(G, out->pose_corrected);
  const float to[6] = {kc.roll, kc.pitch, kc.yaw, kc.x, kc.y, kc.z};
  std::memcpy(out->pose_closest, to, sizeof(to));
  // poseFrom.between(poseTo) = poseFrom^-1 * poseTo (:743-758), in double as gtsam::Pose3
  double A[12], B[12];
  pose3_double(out->pose_corrected, A);
  pose3_double(out->pose_closest, B);
  const double dt[3] = {B[3] - A[3], B[7] - A[7], B[11] - A[11]};
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q)
      out->between[4 * r + q] = (float)((A[r] * B[q] + A[4 + r] * B[4 + q]) + A[8 + r] * B[8 + q]);
    out->between[4 * r + 3] = (float)((A[r] * dt[0] + A[4 + r] * dt[1]) + A[8 + r] * dt[2]);
  }
  out->between[12] = out->between[13] = out->between[14] = 0.0f;
  out->between[15] = 1.0f;
  return FBR_OK;
}

}  // namespace internal
}  // namespace fbr

extern "C" {

void fbr_loop_params_default(fbr_loop_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->search_radius = 15.0f;     // params.yaml:72-75
  p->search_time_diff = 30.0f;
  p->search_num = 25;
  p->fitness_score = 0.3f;
  p->icp_leaf_size = 0.0f;      // downSizeFilterICP: mappingSurfLeafSize (mapOptmization.h:192)
  p->icp.max_correspondence_distance = 100.0f;  // mapOptmization.h:690-693
  p->icp.max_iterations = 100;
  p->icp.transformation_epsilon = 1e-6;
  p->icp.euclidean_fitness_epsilon = 1e-6;
}

int fbr_detect_loop_closure(fbr_ctx* c, double stamp, const fbr_loop_params* lp, int32_t* latest_id, int32_t* closest_id) {
  if (!c || !lp || !latest_id || !closest_id || !(lp->search_radius >= 0)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  (void)loop_candidate(c, stamp, lp, latest_id, closest_id);
  return FBR_OK;
}

int fbr_perform_loop_closure(fbr_ctx* c, double stamp, const fbr_loop_params* lp, fbr_loop_result* out) {
  if (!c || !out || !loop_params_ok(lp)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  std::memset(out, 0, sizeof(*out));
  out->status = FBR_LOOP_NO_CANDIDATE;
  out->latest_id = out->closest_id = -1;
  int32_t latest, closest;
  if (!loop_candidate(c, stamp, lp, &latest, &closest)) return FBR_OK;
  return loop_perform(c, lp, latest, closest, nullptr, out);
}

int fbr_icp_align(fbr_ctx* c, const fbr_point_xyzi* source, int64_t n_source, const fbr_point_xyzi* target,
                  int64_t n_target, const fbr_icp_params* ip, fbr_icp_result* out) {
  if (!c || !ip || !out || n_source < 0 || n_target < 0 || (n_source && !source) || (n_target && !target) ||
      !icp_params_ok(*ip))
    return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  std::memset(out, 0, sizeof(*out));
  int rc = icp_upload(c, c->d_icp_src, source, n_source);
  if (!rc) rc = icp_upload(c, c->d_icp_tgt, target, n_target);
  if (rc) return rc;
  return icp_run(c, c->d_icp_src, n_source, c->d_icp_tgt, n_target, *ip, c->P.mapping_surf_leaf_size, out);
}

int fbr_selftest_nn1(fbr_ctx* c, const fbr_point_xyzi* target, int64_t n_target, const fbr_point_xyzi* query,
                     int64_t n_query, float max_distance, int32_t* index, float* d2) {
  if (!c || n_target < 0 || n_query < 0 || (n_target && !target) || (n_query && (!query || !index || !d2)) ||
      !(max_distance >= 0.0f))
    return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  int rc = icp_upload(c, c->d_icp_src, query, n_query);
  if (!rc) rc = icp_upload(c, c->d_icp_tgt, target, n_target);
  IcpArgs a;
  if (!rc) rc = icp_prepare(c, c->d_icp_src, n_query, c->d_icp_tgt, n_target, c->P.mapping_surf_leaf_size, &a);
  if (rc) return rc;
  a.gate2 = (double)max_distance * (double)max_distance;
  a.flag = nullptr;
  TIMED(c, "icp_nn", launch_icp_nn(c->stream, a, 0, 1));
  TIMED(c, "icp_nn_far", launch_icp_far(c->stream, a, 0));
  CK(hipGetLastError());
  std::vector<unsigned long long> key((size_t)n_query);
  if (n_query) CK(hipMemcpyAsync(key.data(), a.key, sizeof(unsigned long long) * n_query, hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  for (int64_t i = 0; i < n_query; ++i) {
    const uint32_t bits = (uint32_t)(key[i] >> 32);
    float d;
    std::memcpy(&d, &bits, sizeof(d));
    if (key[i] != ~0ull && (double)d <= a.gate2) {
      index[i] = (int32_t)(uint32_t)key[i];
      d2[i] = d;
    } else {
      index[i] = -1;
      d2[i] = FLT_MAX;
    }
  }
  return FBR_OK;
}

}  // extern "C"
