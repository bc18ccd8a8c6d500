// fbr_score.hip — pose scoring (include/fbr.h "pose scoring"): the scan's clouds go to HBM once per
// call, the poses in chunks of fbr_score_params.pose_chunk (their affines and crop boxes are computed
// on the host, 72 B per pose), each chunk is two launches (k_score.hip) and one copy of its records
// back; fbr_pose_search generates its lattice on the host and selects the best records there.
#include "fbr_ctx.h"

namespace {

constexpr int64_t kScoreChunk = 1024;                 // default poses per launch
constexpr int64_t kScoreMaxItems = (int64_t)1 << 30;  // work items of one launch (a grid dimension)
constexpr int64_t kScoreMaxKeys = (int64_t)1 << 25;   // keys of one launch (256 MiB)

bool score_params_ok(const fbr_score_params* sp) {
  return sp && sp->gate > 0.0f && sp->gate <= 1.0f && sp->pose_chunk >= 0 && (sp->use_crop == 0 || sp->use_crop == 1);
}

bool clouds_ok(const fbr_point_xyzi* corner, int64_t n_corner, const fbr_point_xyzi* surf, int64_t n_surf) {
  return n_corner >= 0 && n_surf >= 0 && (!n_corner || corner) && (!n_surf || surf);
}

// Cells covering 1 m: the cell sizes are powers of two between 2 m and 0.125 m (fbr_knobs.h)
int cells_per_metre(float inv) { return inv <= 1.0f ? 1 : (int)inv; }

// The records of poses [0, n_poses) into scores (and the keys into keys, when not null).
int score_run(fbr_ctx* c, const fbr_score_params& sp, const fbr_point_xyzi* corner, int64_t n_corner,
              const fbr_point_xyzi* surf, int64_t n_surf, const float* poses, int64_t n_poses, fbr_pose_score* scores,
              uint64_t* keys) {
  const int64_t npts = n_corner + n_surf;
  if (npts > INT32_MAX / 2) return FBR_ERR_CAPACITY;
  const int64_t ipc = (n_corner + 255) / 256, ipp = ipc + (n_surf + 255) / 256;
  int64_t chunk = std::min<int64_t>(sp.pose_chunk > 0 ? sp.pose_chunk : kScoreChunk, n_poses);
  if (ipp) chunk = std::min(chunk, std::max<int64_t>(1, kScoreMaxItems / ipp));
  if (keys && npts) chunk = std::min(chunk, std::max<int64_t>(1, kScoreMaxKeys / npts));
  int rc = grow(c->d_score_cloud, std::max<int64_t>(npts, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_score_T, chunk * kScorePose, 0, c->stream);
  if (!rc) rc = grow(c->d_score_partial, std::max<int64_t>(chunk * ipp, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_score_out, chunk, 0, c->stream);
  if (!rc && keys) rc = grow(c->d_score_keys, std::max<int64_t>(chunk * npts, 1), 0, c->stream);
  if (rc) return rc;
  if (n_corner) CK(hipMemcpyAsync(c->d_score_cloud, corner, sizeof(float4) * n_corner, hipMemcpyHostToDevice, c->stream));
  if (n_surf)
    CK(hipMemcpyAsync(c->d_score_cloud + n_corner, surf, sizeof(float4) * n_surf, hipMemcpyHostToDevice, c->stream));
  ScoreArgs a{};
  a.corner = c->d_score_cloud;
  a.surf = c->d_score_cloud + n_corner;
  a.nc = (int32_t)n_corner;
  a.ns = (int32_t)n_surf;
  a.ipc = (int32_t)ipc;
  a.ipp = (int32_t)ipp;
  a.T = c->d_score_T;
  a.mc = c->grid_c.view();
  a.ms = c->grid_s.view();
  a.R = cells_per_metre(c->grid_s.g.inv_cell);  // both grids share the cell sizes (build_map_grids)
  a.RX = cells_per_metre(c->grid_s.g.inv_x);
  a.g2 = sp.gate * sp.gate;
  a.use_crop = sp.use_crop && !c->map_nocrop ? 1 : 0;
  a.partial = c->d_score_partial;
  a.keys = keys ? c->d_score_keys.get() : nullptr;
  a.out = c->d_score_out;
  const float* h = c->P.crop_half;
  std::vector<float> T((size_t)(chunk * kScorePose));
  for (int64_t p0 = 0; p0 < n_poses; p0 += chunk) {
    const int64_t np = std::min(chunk, n_poses - p0);
    for (int64_t k = 0; k < np; ++k) {
      float m[16], *t = &T[(size_t)(k * kScorePose)];
      fbr_affine_from_pose(poses + (p0 + k) * 6, m);
      for (int q = 0; q < 12; ++q) t[q] = m[q];
      for (int q = 0; q < 3; ++q) {  // registration's box, as k_gn_init stores it
        t[12 + q] = (-h[q]) + m[4 * q + 3];
        t[15 + q] = h[q] + m[4 * q + 3];
      }
    }
    a.n_poses = (int32_t)np;
    CK(hipMemcpyAsync(c->d_score_T, T.data(), sizeof(float) * np * kScorePose, hipMemcpyHostToDevice, c->stream));
    TIMED(c, "score_nn", launch_score_nn(c->stream, a));
    TIMED(c, "score_sum", launch_score_sum(c->stream, a));
    CK(hipGetLastError());
    CK(hipMemcpyAsync(scores + p0, c->d_score_out, sizeof(fbr_pose_score) * np, hipMemcpyDeviceToHost, c->stream));
    if (keys && npts)
      CK(hipMemcpyAsync(keys + p0 * npts, c->d_score_keys, sizeof(uint64_t) * np * npts, hipMemcpyDeviceToHost, c->stream));
    CK(fbr_sync(c->stream));  // T and the scratch are reused by the next chunk
  }
  return FBR_OK;
}

// The offsets of one lattice axis, ascending; false for a negative or non-finite half or step.
bool axis_offsets(float half, float step, std::vector<float>& out) {
  out.clear();
  if (!(half >= 0.0f) || !(step >= 0.0f) || !std::isfinite(half) || !std::isfinite(step)) return false;
  if (half == 0.0f || step == 0.0f) {
    out.push_back(0.0f);
    return true;
  }
  const float k = std::floor(half / step);
  if (!(k <= (float)FBR_POSE_SEARCH_MAX)) return false;  // 2 k + 1 offsets alone pass the cap
  for (int64_t i = -(int64_t)k; i <= (int64_t)k; ++i) out.push_back((float)i * step);
  return true;
}

}  // namespace

extern "C" {

void fbr_score_params_default(fbr_score_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->gate = 1.0f;
  p->use_crop = 1;
}

int fbr_score_poses(fbr_ctx* c, const fbr_score_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                    const fbr_point_xyzi* surf, int64_t n_surf, const float* poses, int64_t n_poses,
                    fbr_pose_score* scores_out, uint64_t* nn_keys_out) {
  if (!c || !score_params_ok(sp) || !clouds_ok(corner, n_corner, surf, n_surf) || n_poses < 0 ||
      (n_poses && (!poses || !scores_out)))
    return FBR_ERR_INVALID_ARG;
  if (!c->has_map) return FBR_ERR_STATE;
  if (n_poses == 0) return FBR_OK;
  CK(enter(c));
  return score_run(c, *sp, corner, n_corner, surf, n_surf, poses, n_poses, scores_out, nn_keys_out);
}

int fbr_pose_search(fbr_ctx* c, const fbr_score_params* sp, const fbr_point_xyzi* corner, int64_t n_corner,
                    const fbr_point_xyzi* surf, int64_t n_surf, const float* seeds, int64_t n_seeds,
                    const fbr_pose_lattice* lattice, int64_t top_k, float* poses_out, fbr_pose_score* scores_out,
                    int64_t* index_out, int64_t* n_out) {
  if (!c || !score_params_ok(sp) || !clouds_ok(corner, n_corner, surf, n_surf) || n_seeds < 0 || (n_seeds && !seeds) ||
      !lattice || top_k < 0 || (top_k && !poses_out) || !n_out)
    return FBR_ERR_INVALID_ARG;
  std::vector<float> off[4];
  int64_t per_seed = 1;
  for (int ax = 0; ax < 4; ++ax) {
    if (!axis_offsets(lattice->half[ax], lattice->step[ax], off[ax])) return FBR_ERR_INVALID_ARG;
    per_seed *= (int64_t)off[ax].size();
    if (per_seed > FBR_POSE_SEARCH_MAX) return FBR_ERR_INVALID_ARG;
  }
  if (n_seeds > FBR_POSE_SEARCH_MAX || per_seed * n_seeds > FBR_POSE_SEARCH_MAX) return FBR_ERR_INVALID_ARG;
  if (!c->has_map) return FBR_ERR_STATE;
  *n_out = 0;
  const int64_t n = per_seed * n_seeds;
  if (n == 0 || top_k == 0) return FBR_OK;
  CK(enter(c));
  std::vector<float> hyp((size_t)(n * 6));
  float* p = hyp.data();
  for (int64_t s = 0; s < n_seeds; ++s) {
    const float* seed = seeds + s * 6;
    for (float dyaw : off[3])
      for (float dz : off[2])
        for (float dy : off[1])
          for (float dx : off[0]) {
            p[0] = seed[0];
            p[1] = seed[1];
            p[2] = seed[2] + dyaw;
            p[3] = seed[3] + dx;
            p[4] = seed[4] + dy;
            p[5] = seed[5] + dz;
            p += 6;
          }
  }
  std::vector<fbr_pose_score> sc((size_t)n);
  const int rc = score_run(c, *sp, corner, n_corner, surf, n_surf, hyp.data(), n, sc.data(), nullptr);
  if (rc) return rc;
  std::vector<int64_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
  const int64_t m = std::min(top_k, n);
  std::partial_sort(order.begin(), order.begin() + m, order.end(), [&sc](int64_t a, int64_t b) {
    const double fa = sc[(size_t)a].fitness, fb = sc[(size_t)b].fitness;
    return fa < fb || (fa == fb && a < b);
  });
  for (int64_t i = 0; i < m; ++i) {
    const int64_t k = order[(size_t)i];
    std::memcpy(poses_out + i * 6, &hyp[(size_t)(k * 6)], sizeof(float) * 6);
    if (scores_out) scores_out[i] = sc[(size_t)k];
    if (index_out) index_out[i] = k;
  }
  *n_out = m;
  return FBR_OK;
}

}  // extern "C"
