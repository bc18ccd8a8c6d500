// fbr_loop.hip — loop closure on the keyframe store: the candidate search, the ICP driver
// (k_icp.hip) for one pair and for chunks of pairs (fbr_loop_plan.h), and fbr_selftest_nn1.
#include "fbr_ctx.h"
#include "fbr_loop_plan.h"

// ---------------------------------------------------------------------------------------------
// loop closure: detectLoopClosure / performLoopClosure (mapOptmization.h:606-782), k_icp.hip
// ---------------------------------------------------------------------------------------------
namespace {

// detectLoopClosure's candidate (:616-644): radius search around the last key pose (the conventions
// of extractNearby above), the first hit older than search_time_diff.
// The rule for keyframe `last` as the last keyframe (the store holding keyframes 0 .. last): the
// candidate, or -1.  `hits` is scratch.
int64_t loop_candidate_of(const fbr_ctx* c, int64_t last, double stamp, const fbr_loop_params* lp,
                          std::vector<std::pair<float, int64_t>>& hits) {
  const int64_t N = last + 1;
  const fbr_keypose& back = c->kf_poses[last];
  const float r2 = (float)((double)lp->search_radius * (double)lp->search_radius);
  hits.clear();
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
  return cand == N - 1 ? -1 : cand;  // :639-644
}

bool loop_candidate(const fbr_ctx* c, double stamp, const fbr_loop_params* lp, int32_t* latest, int32_t* closest) {
  *latest = *closest = -1;
  const int64_t N = (int64_t)c->kf_poses.size();
  if (N == 0) return false;
  std::vector<std::pair<float, int64_t>> hits;
  const int64_t cand = loop_candidate_of(c, N - 1, stamp, lp, hits);
  if (cand < 0) return false;
  *latest = (int32_t)(N - 1);
  *closest = (int32_t)cand;
  return true;
}

// The search grid over a target: cubic cells of the power of two at or above the hint (the target's
// point spacing, a VoxelGrid leaf); doubled while outliers would make the box sparse or mostly
// empty, and no grid (*use_grid = 0: every query brute force) if that does not end.
int icp_target_grid(fbr_ctx* c, const float4* d_tgt, int64_t nt, float cell_hint, DevGrid& grid, int* use_grid) {
  *use_grid = 0;
  if (nt <= 0) return FBR_OK;
  float cell = 1.0f / 64.0f;
  const float hint = cell_hint > 0.0f ? cell_hint : 0.5f;
  while (cell < hint && cell < 64.0f) cell *= 2.0f;
  for (int tries = 0; tries < 8; ++tries, cell *= 2.0f) {
    const int rc = grid_build_device(c->stream, c->arena, d_tgt, nt, 1.0f / cell, 1.0f / cell, false, grid);
    if (rc == FBR_ERR_CAPACITY) continue;  // (nt is in range: the box has too many cells even for chunks)
    if (rc) return rc;
    const GridDesc& g = grid.g;
    if (!g.sparse && (int64_t)g.n_cells <= std::max<int64_t>((int64_t)1 << 22, 64 * nt)) {
      *use_grid = 1;
      break;
    }
  }
  return FBR_OK;
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
  rc = icp_target_grid(c, d_tgt, nt, cell_hint, c->icp_grid, &a->use_grid);
  if (rc) return rc;
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

// ---- many pairs per launch (fbr_loop_plan.h, k_icp.hip's batch kernels) -----------------------------
namespace lpn = fbr::loop_plan;
static_assert(lpn::kPartialDoubles == kIcpSums, "fbr_loop_plan.h counts the partial rows of k_icp.hip");
static_assert(sizeof(lpn::BlockRef) == sizeof(int2), "the block table is an int2 array on the device");

// Grows the pools of a chunk.  with_raw: the chunk builds its targets from a raw concatenation
// (loop closure); the sources are built or uploaded into d_lb_src, the targets into d_lb_tgt.
int lb_grow(fbr_ctx* c, const lpn::Chunk& ch, bool with_raw) {
  const int64_t ns = std::max<int64_t>(ch.src_total, 1), nt = std::max<int64_t>(ch.tgt_total, 1);
  int rc = grow(c->d_lb_src, ns, 0, c->stream);
  if (!rc) rc = grow(c->d_lb_x, ns, 0, c->stream);
  if (!rc) rc = grow(c->d_lb_key, ns, 0, c->stream);
  if (!rc) rc = grow(c->d_lb_far, ns, 0, c->stream);
  if (!rc) rc = grow(c->d_lb_partial, std::max<int64_t>(ch.nblocks, 1) * kIcpSums, 0, c->stream);
  if (!rc) rc = grow(c->d_lb_tgt, nt, 0, c->stream);
  if (!rc && with_raw) rc = grow(c->d_lb_raw, nt, 0, c->stream);
  return rc;
}

// icp_run for the pairs of one chunk, whose sources stand in d_lb_src and whose targets in d_lb_tgt
// at their slots: nt[p] target points each, cell_hint as icp_run's.  Every pair's ICP advances in
// the same launches; the host paces itself on the launches done and stops when every pair has.
int icp_run_chunk(fbr_ctx* c, const lpn::PairSize* sizes, const std::vector<lpn::PairSlot>& slots,
                  const std::vector<lpn::BlockRef>& table, const int64_t* nt, const fbr_icp_params& ip, float cell_hint,
                  fbr_icp_result* out) {
  const int64_t P = (int64_t)slots.size();
  for (int64_t p = 0; p < P; ++p)
    if (sizes[p].ns >= ((int64_t)1 << 30) || nt[p] >= ((int64_t)1 << 28)) return FBR_ERR_CAPACITY;
  if (!c->icp_flag && c->icp_flag.alloc(1)) return FBR_ERR_HIP;
  if ((int64_t)c->icp_grids.size() < P) c->icp_grids.resize((size_t)P);
  // the meta block: what the host writes (argument blocks, block table, splits) in one copy, then
  // what only the device writes
  auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
  const int64_t o_args = 0, o_fit = o_args + up(sizeof(IcpArgs) * P), o_table = o_fit + up(sizeof(IcpArgs) * P),
                o_split = o_table + up(sizeof(int2) * (int64_t)table.size()), host_bytes = o_split + up(sizeof(int32_t) * P),
                o_ctl = host_bytes, o_state = o_ctl + up(sizeof(IcpBatchCtl)), o_res = o_state + up(sizeof(IcpState) * P),
                o_cnt = o_res + up(sizeof(fbr_icp_result) * P), total = o_cnt + up(sizeof(int32_t) * P);
  int rc = grow(c->d_lb_meta, total, 0, c->stream);
  if (rc) return rc;
  uint8_t* meta = c->d_lb_meta;
  std::vector<uint8_t> h((size_t)host_bytes, 0);
  IcpArgs* ha = reinterpret_cast<IcpArgs*>(h.data() + o_args);
  IcpArgs* hf = reinterpret_cast<IcpArgs*>(h.data() + o_fit);
  int32_t* hs = reinterpret_cast<int32_t*>(h.data() + o_split);
  if (!table.empty()) std::memcpy(h.data() + o_table, table.data(), sizeof(lpn::BlockRef) * table.size());
  const double md = (double)ip.max_correspondence_distance;
  IcpBatch b{};
  for (int64_t p = 0; p < P; ++p) {
    const lpn::PairSlot& s = slots[p];
    IcpArgs a{};
    a.src = c->d_lb_src + s.src_off;
    a.x = c->d_lb_x + s.src_off;
    a.n = sizes[p].ns;
    a.tgt = c->d_lb_tgt + s.tgt_off;
    a.nt = nt[p];
    a.key = c->d_lb_key + s.src_off;
    a.far_list = c->d_lb_far + s.src_off;
    a.far_cnt = reinterpret_cast<int32_t*>(meta + o_cnt) + p;
    a.partial = c->d_lb_partial + s.blk0 * kIcpSums;
    a.st = reinterpret_cast<IcpState*>(meta + o_state) + p;
    a.flag = nullptr;  // the launch publishes, not the pair
    rc = icp_target_grid(c, a.tgt, a.nt, cell_hint, c->icp_grids[(size_t)p], &a.use_grid);
    if (rc) return rc;
    a.grid = c->icp_grids[(size_t)p].view();
    a.gate2 = md * md;
    ha[p] = a;
    a.gate2 = INFINITY;  // getFitnessScore: final * source against the target, no gate
    hf[p] = a;
    hs[p] = icp_far_split(a.nt);
    b.max_split = std::max(b.max_split, hs[p]);
  }
  CK(hipMemcpyAsync(meta, h.data(), (size_t)host_bytes, hipMemcpyHostToDevice, c->stream));
  b.args = reinterpret_cast<const IcpArgs*>(meta + o_args);
  b.args_fit = reinterpret_cast<const IcpArgs*>(meta + o_fit);
  b.table = reinterpret_cast<const int2*>(meta + o_table);
  b.nsplit = reinterpret_cast<const int32_t*>(meta + o_split);
  b.npairs = (int)P;
  b.nblocks = (int)table.size();
  b.ctl = reinterpret_cast<IcpBatchCtl*>(meta + o_ctl);
  b.flag = c->icp_flag.dev();
  fbr_icp_result* d_res = reinterpret_cast<fbr_icp_result*>(meta + o_res);
  launch_icp_init_batch(c->stream, b);
  const unsigned long long gen = (++c->icp_gen) & 0xFFFFFFFFull;
  constexpr int kLead = 4;  // launches the host may run ahead of the device
  for (int it = 0; it < std::max(1, ip.max_iterations); ++it) {
    if (run_ahead(c->icp_flag.host(), gen, it, kLead, debug_counters().flag_polls)) break;
    TIMED(c, "icp_nn", launch_icp_nn_batch(c->stream, b, 0, it == 0));
    TIMED(c, "icp_nn_far", launch_icp_far_batch(c->stream, b, 0));
    TIMED(c, "icp_solve", launch_icp_solve_batch(c->stream, b, ip.max_iterations, ip.transformation_epsilon,
                                                 ip.euclidean_fitness_epsilon, gen));
  }
  TIMED(c, "icp_nn", launch_icp_nn_batch(c->stream, b, 1, 0));
  TIMED(c, "icp_nn_far", launch_icp_far_batch(c->stream, b, 1));
  TIMED(c, "icp_solve", launch_icp_finish_batch(c->stream, b, d_res));
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, d_res, sizeof(fbr_icp_result) * P, hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));  // (also: `h` outlives its copy)
  return FBR_OK;
}

}  // namespace

namespace fbr {
namespace internal {

bool loop_params_ok(const fbr_loop_params* lp) {
  return lp && lp->search_radius >= 0 && lp->search_num >= 0 && lp->icp_leaf_size >= 0 && icp_params_ok(lp->icp);
}

static void loop_finish(fbr_ctx* c, const fbr_loop_params* lp, int32_t latest, int32_t closest, const float* latest_pose,
                        int64_t n_src, int64_t n_tgt, fbr_loop_result* out);

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
  loop_finish(c, lp, latest, closest, latest_pose, n_src, n_tgt, out);
  return FBR_OK;
}

// What performLoopClosure makes of the ICP's result (out->icp): the status, tCorrect and the factor.
static void loop_finish(fbr_ctx* c, const fbr_loop_params* lp, int32_t latest, int32_t closest, const float* latest_pose,
                        int64_t n_src, int64_t n_tgt, fbr_loop_result* out) {
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
}

}  // namespace internal
}  // namespace fbr

namespace {

// The keyframes of a pair's target: closest +- search_num inside [0, latest] (:659).
inline void loop_window(const fbr_loop_params* lp, const fbr_loop_pair& pr, int64_t* k0, int64_t* k1) {
  *k0 = std::max<int64_t>((int64_t)pr.closest_id - lp->search_num, 0);
  *k1 = std::min<int64_t>((int64_t)pr.closest_id + lp->search_num, pr.latest_id);
}

// loop_perform for the pairs of one chunk.  The preparation stays pair by pair but for the
// transforms (one launch per pool and destination for all pairs); the ICPs advance together.
int loop_perform_chunk(fbr_ctx* c, const fbr_loop_params* lp, const fbr_loop_pair* pairs, const lpn::PairSize* sizes,
                       const lpn::Chunk& ch, fbr_loop_result* out) {
  std::vector<lpn::PairSlot> slots;
  std::vector<lpn::BlockRef> table;
  lpn::layout_chunk(sizes, ch.count, &slots, &table);
  int rc = lb_grow(c, ch, true);
  if (rc) return rc;
  // segments by launch: [source corners, source surfs, target corners, target surfs], the clouds of a
  // pair in loop_perform's order (corner then surf per keyframe) from the pair's offset
  std::vector<KfSeg> seg[4];
  int64_t max_cnt[4] = {0, 0, 0, 0};
  auto add = [&](int k, int which, int64_t* off, const float* tr_override) {
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
    seg[which].push_back(g);
    max_cnt[which] = std::max(max_cnt[which], g.count);
    g.src = c->kf_s_off[k];
    g.count = c->kf_s_cnt[k];
    g.dst = *off;
    *off += g.count;
    seg[which + 1].push_back(g);
    max_cnt[which + 1] = std::max(max_cnt[which + 1], g.count);
  };
  for (int64_t p = 0; p < ch.count; ++p) {
    const fbr_loop_pair& pr = pairs[p];
    int64_t off = slots[p].src_off;
    add(pr.latest_id, 0, &off, pr.use_guess ? pr.pose_guess : nullptr);
    off = slots[p].tgt_off;
    int64_t k0, k1;
    loop_window(lp, pr, &k0, &k1);
    for (int64_t k = k0; k <= k1; ++k) add((int)k, 2, &off, nullptr);
  }
  std::vector<KfSeg> segs;
  int64_t first[4];
  for (int w = 0; w < 4; ++w) {
    first[w] = (int64_t)segs.size();
    segs.insert(segs.end(), seg[w].begin(), seg[w].end());
  }
  rc = grow(c->d_lb_segs, std::max<int64_t>((int64_t)segs.size(), 1), 0, c->stream);
  if (rc) return rc;
  CK(hipMemcpyAsync(c->d_lb_segs, segs.data(), sizeof(KfSeg) * segs.size(), hipMemcpyHostToDevice, c->stream));
  for (int w = 0; w < 4; ++w)
    launch_kf_transform(c->stream, (w & 1) ? c->d_kf_s : c->d_kf_c, c->d_lb_segs + first[w], (int)seg[w].size(), max_cnt[w],
                        w < 2 ? c->d_lb_src : c->d_lb_raw);
  CK(hipGetLastError());
  CK(fbr_sync(c->stream));  // the pageable copy of `segs`
  // downSizeFilterICP (:698-701), one target at a time
  const float leaf = lp->icp_leaf_size > 0.0f ? lp->icp_leaf_size : c->P.mapping_surf_leaf_size;
  std::vector<int64_t> n_tgt((size_t)ch.count, 0);
  for (int64_t p = 0; p < ch.count; ++p) {
    rc = voxel_grid_dev(c, c->d_lb_raw + slots[p].tgt_off, sizes[p].nt, leaf, c->d_lb_tgt + slots[p].tgt_off, &n_tgt[p]);
    if (rc) return rc;
  }
  std::vector<fbr_icp_result> res((size_t)ch.count);
  rc = icp_run_chunk(c, sizes, slots, table, n_tgt.data(), lp->icp, leaf, res.data());
  if (rc) return rc;
  for (int64_t p = 0; p < ch.count; ++p) {
    const fbr_loop_pair& pr = pairs[p];
    std::memset(&out[p], 0, sizeof(out[p]));
    out[p].icp = res[p];
    loop_finish(c, lp, pr.latest_id, pr.closest_id, pr.use_guess ? pr.pose_guess : nullptr, sizes[p].ns, n_tgt[p], &out[p]);
  }
  return FBR_OK;
}

// Frees what a batch call's chunk left in the per-pair grids beyond `keep` pairs, so a large call
// does not pin its grids until the context goes.
void lb_trim_grids(fbr_ctx* c, size_t keep) {
  for (size_t p = keep; p < c->icp_grids.size(); ++p) free_grid(c->icp_grids[p]);
  if (c->icp_grids.size() > keep) c->icp_grids.resize(keep);
}

}  // namespace

extern "C" {

int fbr_loop_candidates(fbr_ctx* c, const fbr_loop_params* lp, int32_t first_keyframe, fbr_loop_pair* pairs, int64_t cap,
                        int64_t* n_pairs) {
  if (!c || !lp || !n_pairs || cap < 0 || (cap > 0 && !pairs) || first_keyframe < 0 || !(lp->search_radius >= 0))
    return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  const int64_t N = (int64_t)c->kf_poses.size();
  std::vector<std::pair<float, int64_t>> hits;
  int64_t n = 0;
  for (int64_t i = first_keyframe; i < N; ++i) {
    const int64_t cand = loop_candidate_of(c, i, c->kf_poses[i].time, lp, hits);
    if (cand < 0) continue;
    if (n < cap) {
      fbr_loop_pair pr;
      std::memset(&pr, 0, sizeof(pr));
      pr.latest_id = (int32_t)i;
      pr.closest_id = (int32_t)cand;
      pairs[n] = pr;
    }
    ++n;
  }
  *n_pairs = n;
  return n > cap ? FBR_ERR_CAPACITY : FBR_OK;
}

int fbr_perform_loop_closures(fbr_ctx* c, const fbr_loop_params* lp, const fbr_loop_pair* pairs, int64_t n_pairs,
                              int32_t chunk_pairs, fbr_loop_result* out) {
  if (!c || !loop_params_ok(lp) || n_pairs < 0 || chunk_pairs < 0 || (n_pairs > 0 && (!pairs || !out)))
    return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  const int64_t N = (int64_t)c->kf_poses.size();
  std::vector<lpn::PairSize> sizes((size_t)n_pairs);
  for (int64_t p = 0; p < n_pairs; ++p) {
    const fbr_loop_pair& pr = pairs[p];
    if (pr.latest_id < 0 || pr.latest_id >= N || pr.closest_id < 0 || pr.closest_id >= N || pr.latest_id == pr.closest_id)
      return FBR_ERR_INVALID_ARG;
    int64_t k0, k1, nt = 0;
    loop_window(lp, pr, &k0, &k1);
    for (int64_t k = k0; k <= k1; ++k) nt += c->kf_c_cnt[k] + c->kf_s_cnt[k];
    sizes[p] = lpn::PairSize{c->kf_c_cnt[pr.latest_id] + c->kf_s_cnt[pr.latest_id], nt};
  }
  int64_t most = 0;
  for (const lpn::Chunk& ch : lpn::plan_chunks(sizes.data(), n_pairs, chunk_pairs, knobs::loop_batch_bytes())) {
    const int rc = loop_perform_chunk(c, lp, pairs + ch.first, sizes.data() + ch.first, ch, out + ch.first);
    if (rc) return rc;
    most = std::max(most, ch.count);
  }
  lb_trim_grids(c, (size_t)std::min<int64_t>(most, 64));
  return FBR_OK;
}

int fbr_icp_align_batch(fbr_ctx* c, const fbr_point_xyzi* const* sources, const int64_t* n_sources,
                        const fbr_point_xyzi* const* targets, const int64_t* n_targets, int64_t n_pairs,
                        const fbr_icp_params* ip, int32_t chunk_pairs, fbr_icp_result* out) {
  if (!c || !ip || n_pairs < 0 || chunk_pairs < 0 || !icp_params_ok(*ip) ||
      (n_pairs > 0 && (!sources || !n_sources || !targets || !n_targets || !out)))
    return FBR_ERR_INVALID_ARG;
  std::vector<lpn::PairSize> sizes((size_t)n_pairs);
  for (int64_t p = 0; p < n_pairs; ++p) {
    if (n_sources[p] < 0 || n_targets[p] < 0 || (n_sources[p] && !sources[p]) || (n_targets[p] && !targets[p]))
      return FBR_ERR_INVALID_ARG;
    sizes[p] = lpn::PairSize{n_sources[p], n_targets[p]};
  }
  CK(enter(c));
  int64_t most = 0;
  std::vector<lpn::PairSlot> slots;
  std::vector<lpn::BlockRef> table;
  std::vector<int64_t> nt;
  for (const lpn::Chunk& ch : lpn::plan_chunks(sizes.data(), n_pairs, chunk_pairs, knobs::loop_batch_bytes())) {
    lpn::layout_chunk(sizes.data() + ch.first, ch.count, &slots, &table);
    int rc = lb_grow(c, ch, false);
    if (rc) return rc;
    nt.assign((size_t)ch.count, 0);
    for (int64_t p = 0; p < ch.count; ++p) {
      const int64_t q = ch.first + p;
      nt[p] = n_targets[q];
      if (n_sources[q])
        CK(hipMemcpyAsync(c->d_lb_src + slots[p].src_off, sources[q], sizeof(float4) * n_sources[q], hipMemcpyHostToDevice, c->stream));
      if (n_targets[q])
        CK(hipMemcpyAsync(c->d_lb_tgt + slots[p].tgt_off, targets[q], sizeof(float4) * n_targets[q], hipMemcpyHostToDevice, c->stream));
    }
    CK(fbr_sync(c->stream));
    std::memset(out + ch.first, 0, sizeof(fbr_icp_result) * ch.count);
    rc = icp_run_chunk(c, sizes.data() + ch.first, slots, table, nt.data(), *ip, c->P.mapping_surf_leaf_size, out + ch.first);
    if (rc) return rc;
    most = std::max(most, ch.count);
  }
  lb_trim_grids(c, (size_t)std::min<int64_t>(most, 64));
  return FBR_OK;
}

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
