// fbr_map.hip — the registration map: the start-up VoxelGrid and the kNN grids of fbr_set_map (and of
// set_map_device, the same steps on clouds already in HBM, for fbr_global_map_install), the
// keyframe store and the local map fbr_extract_surrounding_keyframes builds from it, and the
// pose / affine helpers.
#include "fbr_ctx.h"

namespace {

// ---------------------------------------------------------------------------------------------
// map grid (built once per fbr_set_map; see k_register.hip for why this replaces the KD-trees)
// ---------------------------------------------------------------------------------------------
// kNN grid cell sizes (powers of two, so cell coordinates and edges are exact), chosen from the
// map density the mapping leaf implies (one point per leaf voxel at most): 1 m along y and z and
// 0.25 m along x for surf leaves >= 0.3 m (the 0.4 m default), 0.5 m / 0.125 m for denser maps
// (measured).  FBR_KNN_CELL / FBR_KNN_CELL_X override (fbr_knobs.h); both maps share them.
void grid_cell_sizes(const fbr_params& P, float* inv_yz, float* inv_x) {
  const bool sparse = P.mapping_surf_leaf_size >= 0.3f;
  *inv_yz = knobs::knn_cell_inv(sparse);
  *inv_x = knobs::knn_cell_x_inv(sparse);
}

// One-segment device VoxelGrid of a host cloud (map start-up filter, fbr_voxel_grid): upload,
// voxel_grid_dev, download.
int voxel_grid_once(fbr_ctx* c, const fbr_point_xyzi* in, int64_t n, float leaf, std::vector<fbr_point_xyzi>& out) {
  out.clear();
  if (n <= 0) return FBR_OK;
  // a host cloud with a non-finite point is not dense: PCL's VoxelGrid (and getMinMax3D) skip such
  // points (voxel_grid.cpp, is_dense false), which is the filter over the finite points alone
  for (int64_t i = 0; i < n; ++i)
    if (!(std::isfinite(in[i].x) && std::isfinite(in[i].y) && std::isfinite(in[i].z))) {
      std::vector<fbr_point_xyzi> fin;
      fin.reserve(n);
      for (int64_t j = 0; j < n; ++j)
        if (std::isfinite(in[j].x) && std::isfinite(in[j].y) && std::isfinite(in[j].z)) fin.push_back(in[j]);
      return voxel_grid_once(c, fin.data(), (int64_t)fin.size(), leaf, out);
    }
  if (n > INT32_MAX / 4) return FBR_ERR_CAPACITY;
  Dev<float4> d_in, d_out;
  if (dalloc(d_in, n) || dalloc(d_out, n)) return FBR_ERR_HIP;
  CK(hipMemcpyAsync(d_in, in, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
  int64_t nout = 0;
  const int rc = voxel_grid_dev(c, d_in, n, leaf, d_out, &nout);
  if (rc) return rc;
  out.resize(nout);
  if (nout) CK(fbr_memcpy_sync(out.data(), d_out, sizeof(float4) * nout, hipMemcpyDeviceToHost));
  return FBR_OK;
}

}  // namespace

namespace fbr {
namespace internal {

// One-segment device VoxelGrid of a device-resident cloud into a device buffer of n points.
int voxel_grid_dev(fbr_ctx* c, const float4* d_in, int64_t n, float leaf, float4* d_out, int64_t* n_out) {
  *n_out = 0;
  if (n <= 0) return FBR_OK;
  if (n > INT32_MAX / 4) return FBR_ERR_CAPACITY;
  // d_cnt: {input count, output count, look-back error word (k_voxel_grid_split: a part that gave
  // up its look-back flags it, whichever part writes the count)}; the large filter writes its
  // output count alone and reports a failure itself
  // the host words of the queued copies stand before the handles, so they outlive every copy: a
  // handle's release waits for the device
  const int32_t nn = (int32_t)n;
  int32_t ce[2] = {0, 0};  // output count, error word
  Dev<int32_t> d_cnt;
  Dev<uint32_t> d_sc;
  if (n >= knobs::vg_large_min()) {
    if (dalloc(d_cnt, 1)) return FBR_ERR_HIP;
    const int rc = voxel_grid_large(c->stream, c->arena, d_in, n, leaf, 0, c->P.exact_voxel_order ? 1 : 0, d_out, d_cnt);
    if (rc) return rc;
    CK(hipMemcpyAsync(ce, d_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  } else {
    if (dalloc(d_cnt, 3) || dalloc(d_sc, kVgScratch * n)) return FBR_ERR_HIP;
    VgArgs a{};
    a.s[0].in = d_in;
    a.s[0].stride_in = n;
    a.s[0].cnt_in = d_cnt;
    a.s[0].cap = n;
    a.s[0].out = d_out;
    a.s[0].stride_out = n;
    a.s[0].cnt_out = d_cnt + 1;
    a.s[0].scratch = d_sc;
    a.s[0].leaf = leaf;
    a.s[0].nseg = 1;
    a.s[0].exact = c->P.exact_voxel_order ? 1 : 0;
    a.err = d_cnt + 2;
    CK(hipMemcpyAsync(d_cnt, &nn, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    CK(hipMemsetAsync(d_cnt + 2, 0, sizeof(int32_t), c->stream));
    launch_voxel_grid(c->stream, a);
    CK(hipMemcpyAsync(ce, d_cnt + 1, sizeof(ce), hipMemcpyDeviceToHost, c->stream));
  }
  CK(fbr_sync(c->stream));
  if (ce[0] < 0 || ce[1] != 0) return FBR_ERR_HIP;
  *n_out = ce[0];
  return FBR_OK;
}

}  // namespace internal
}  // namespace fbr

// ---------------------------------------------------------------------------------------------
// keyframe local map helpers (fbr_extract_surrounding_keyframes)
// ---------------------------------------------------------------------------------------------
namespace {

// Both kNN grids of a map (corner, surf) on the device, with one cell size and one layout (the
// kNN kernel is specialised on both): the shared cell sizes of grid_cell_sizes, dense unless a
// map's occupied box is too large, then hashed chunks for both.
int build_map_grids(fbr_ctx* c, const float4* d_corner, int64_t nc, const float4* d_surf, int64_t ns) {
  float inv, invx;
  grid_cell_sizes(c->P, &inv, &invx);
  int rc = grid_build_device(c->stream, c->arena, d_corner, nc, invx, inv, false, c->grid_c);
  if (!rc) rc = grid_build_device(c->stream, c->arena, d_surf, ns, invx, inv, c->grid_c.g.sparse != 0, c->grid_s);
  if (!rc && c->grid_s.g.sparse && !c->grid_c.g.sparse)
    rc = grid_build_device(c->stream, c->arena, d_corner, nc, invx, inv, true, c->grid_c);
  // block-tile kNN buffers (dense 0.5 m x 0.125 m grids only): per-block arrays for every stream
  // a sub-batch may run on, zeroed once (k_bin_tile re-zeroes the counts it used)
  c->d_bin.reset();
  c->bin_nb = c->bin_nb_c = 0;
  if (!rc && knn_tile_applies(c->grid_c.g, c->grid_s.g)) {
    c->bin_nb_c = knn_tile_blocks(c->grid_c.g);
    c->bin_nb = c->bin_nb_c + knn_tile_blocks(c->grid_s.g);
    const int64_t slots = (int64_t)c->max_items * 256;
    const bool ok = c->bin_nb < (int64_t)1 << 30 &&
                    (c->d_fb_list || c->d_fb_list.alloc(3 * slots)) && c->d_bin.alloc(kMaxSub * 3 * c->bin_nb) &&
                    hipMemsetAsync(c->d_bin, 0, sizeof(int32_t) * kMaxSub * 3 * c->bin_nb, c->stream) == hipSuccess;
    if (!ok) {  // the grid search serves every query (alloc() itself reports nothing)
      (void)hipGetLastError();
      c->d_bin.reset();
      c->bin_nb = c->bin_nb_c = 0;
    }
  }
  return rc;
}

// pointDistance (utility.h:312-315) of two key poses
float key_distance(const fbr_keypose& a, const fbr_keypose& b) {
  return std::sqrt((a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z));
}

}  // namespace

namespace fbr {
namespace internal {

// fbr_set_map's steps on device-resident clouds: the start-up VoxelGrids, then the grids.  The DS
// maps stay in d_inst_c / d_inst_s; fbr_get_map fills the host copies from them on demand.
int set_map_device(fbr_ctx* c, const float4* d_corner, int64_t n_corner, const float4* d_surf, int64_t n_surf) {
  c->crop_cached = false;
  c->map_nocrop = false;
  c->map_c_host.clear();
  c->map_s_host.clear();
  c->map_host_stale = false;
  c->has_map = false;
  c->inst_c_n = c->inst_s_n = 0;
  if (dalloc(c->d_inst_c, std::max<int64_t>(n_corner, 1)) || dalloc(c->d_inst_s, std::max<int64_t>(n_surf, 1)))
    return FBR_ERR_HIP;
  int rc = voxel_grid_dev(c, d_corner, n_corner, c->P.mapping_corner_leaf_size, c->d_inst_c, &c->inst_c_n);
  if (!rc) rc = voxel_grid_dev(c, d_surf, n_surf, c->P.mapping_surf_leaf_size, c->d_inst_s, &c->inst_s_n);
  if (!rc) rc = build_map_grids(c, c->d_inst_c, c->inst_c_n, c->d_inst_s, c->inst_s_n);
  c->has_map = rc == FBR_OK;
  c->map_host_stale = rc == FBR_OK;
  return rc;
}

}  // namespace internal
}  // namespace fbr

extern "C" {

int fbr_set_map(fbr_ctx* c, const fbr_point_xyzi* corner, int64_t n_corner, const fbr_point_xyzi* surf,
                int64_t n_surf) {
  if (!c || n_corner < 0 || n_surf < 0 || (n_corner && !corner) || (n_surf && !surf)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  c->crop_cached = false;
  c->map_nocrop = false;
  c->map_host_stale = false;  // an installed map (fbr_global_map_install) is replaced
  c->d_inst_c.reset();
  c->d_inst_s.reset();
  int rc = voxel_grid_once(c, corner, n_corner, c->P.mapping_corner_leaf_size, c->map_c_host);
  if (!rc) rc = voxel_grid_once(c, surf, n_surf, c->P.mapping_surf_leaf_size, c->map_s_host);
  // the DS maps (map-index order) go to HBM once; the grids are built there
  Dev<float4> d_c, d_s;
  const int64_t nc = (int64_t)c->map_c_host.size(), ns = (int64_t)c->map_s_host.size();
  if (!rc && (dalloc(d_c, std::max<int64_t>(nc, 1)) || dalloc(d_s, std::max<int64_t>(ns, 1)))) rc = FBR_ERR_HIP;
  if (!rc && nc && hipMemcpy(d_c, c->map_c_host.data(), sizeof(float4) * nc, hipMemcpyHostToDevice) != hipSuccess)
    rc = FBR_ERR_HIP;
  if (!rc && ns && hipMemcpy(d_s, c->map_s_host.data(), sizeof(float4) * ns, hipMemcpyHostToDevice) != hipSuccess)
    rc = FBR_ERR_HIP;
  if (!rc) rc = build_map_grids(c, d_c, nc, d_s, ns);
  c->has_map = rc == FBR_OK;
  return rc;
}

int fbr_map_grid_info(fbr_ctx* c, int64_t info[8]) {
  if (!c || !info) return FBR_ERR_INVALID_ARG;
  if (!c->has_map) return FBR_ERR_NO_MAP;
  const GridDesc& g = c->grid_s.g;
  info[0] = g.sparse;
  info[1] = g.dims[0];
  info[2] = g.dims[1];
  info[3] = g.dims[2];
  info[4] = (int64_t)g.dims[0] * g.dims[1] * g.dims[2];  // cells of the occupied box
  info[5] = g.sparse ? (int64_t)c->grid_c.g.n_cells + g.n_cells : info[4];  // chunks (sparse) / cells
  info[6] = c->grid_c.g.n_points;
  info[7] = g.n_points;
  return FBR_OK;
}

int fbr_get_map(fbr_ctx* c, int64_t* n_corner, int64_t* n_surf, fbr_point_xyzi* corner, fbr_point_xyzi* surf) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (!c->has_map) return FBR_ERR_NO_MAP;
  if (c->map_nocrop) {  // keyframe local map (device-resident)
    CK(enter(c));
    if (n_corner) *n_corner = c->kds_c_n;
    if (n_surf) *n_surf = c->kds_s_n;
    if (corner && c->kds_c_n) CK(fbr_memcpy_sync(corner, c->d_kds_c, sizeof(float4) * c->kds_c_n, hipMemcpyDeviceToHost));
    if (surf && c->kds_s_n) CK(fbr_memcpy_sync(surf, c->d_kds_s, sizeof(float4) * c->kds_s_n, hipMemcpyDeviceToHost));
    return FBR_OK;
  }
  if (c->map_host_stale) {  // installed from the device (fbr_global_map_install): fetched on first use
    CK(enter(c));
    c->map_c_host.resize((size_t)c->inst_c_n);
    c->map_s_host.resize((size_t)c->inst_s_n);
    if (c->inst_c_n)
      CK(fbr_memcpy_sync(c->map_c_host.data(), c->d_inst_c, sizeof(float4) * c->inst_c_n, hipMemcpyDeviceToHost));
    if (c->inst_s_n)
      CK(fbr_memcpy_sync(c->map_s_host.data(), c->d_inst_s, sizeof(float4) * c->inst_s_n, hipMemcpyDeviceToHost));
    c->map_host_stale = false;
  }
  if (n_corner) *n_corner = (int64_t)c->map_c_host.size();
  if (n_surf) *n_surf = (int64_t)c->map_s_host.size();
  if (corner) std::memcpy(corner, c->map_c_host.data(), sizeof(fbr_point_xyzi) * c->map_c_host.size());
  if (surf) std::memcpy(surf, c->map_s_host.data(), sizeof(fbr_point_xyzi) * c->map_s_host.size());
  return FBR_OK;
}

int fbr_voxel_grid(fbr_ctx* c, const fbr_point_xyzi* in, int64_t n, float leaf, fbr_point_xyzi* out, int64_t* n_out) {
  if (!c || n < 0 || (n && !in) || !(leaf > 0)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  std::vector<fbr_point_xyzi> o;
  int rc = voxel_grid_once(c, in, n, leaf, o);
  if (rc) return rc;
  if (out) std::memcpy(out, o.data(), sizeof(fbr_point_xyzi) * o.size());
  if (n_out) *n_out = (int64_t)o.size();
  return FBR_OK;
}

// pcl::getTransformation(x, y, z, roll, pitch, yaw) (pcl/common/impl/eigen.hpp), float, with
// glibc's sinf / cosf (fbr_sincosf.h).
void fbr_affine_from_pose(const float pose[6], float m[16]) {
  const float roll = pose[0], pitch = pose[1], yaw = pose[2];
  const float A = fbr::gl_cosf(yaw), B = fbr::gl_sinf(yaw), C = fbr::gl_cosf(pitch), D = fbr::gl_sinf(pitch),
              E = fbr::gl_cosf(roll), F = fbr::gl_sinf(roll), DE = D * E, DF = D * F;
  m[0] = A * C; m[1] = A * DF - B * E; m[2] = B * F + A * DE; m[3] = pose[3];
  m[4] = B * C; m[5] = A * E + B * DF; m[6] = B * DE - A * F; m[7] = pose[4];
  m[8] = -D;    m[9] = C * F;          m[10] = C * E;         m[11] = pose[5];
  m[12] = 0.0f; m[13] = 0.0f; m[14] = 0.0f; m[15] = 1.0f;
}

// pcl::getTranslationAndEulerAngles (pcl/common/impl/eigen.hpp), float.
void fbr_pose_from_affine(const float m[16], float pose[6]) {
  pose[3] = m[3];
  pose[4] = m[7];
  pose[5] = m[11];
  pose[0] = std::atan2(m[9], m[10]);
  pose[1] = std::asin(-m[8]);
  pose[2] = std::atan2(m[4], m[0]);
}

void fbr_keyframe_params_default(fbr_keyframe_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->search_radius = 50.0f;  // params.yaml:66-71
  p->pose_density = 2.0f;
  p->loop_closure = 0;
  p->submap_size = 25;
  p->recent_window = 10.0;   // mapOptmization.h:900
}

int fbr_keyframes_add(fbr_ctx* c, const fbr_keypose* pose, const fbr_point_xyzi* corner, int64_t n_corner,
                      const fbr_point_xyzi* surf, int64_t n_surf) {
  if (!c || !pose || n_corner < 0 || n_surf < 0 || (n_corner && !corner) || (n_surf && !surf)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  int rc = grow(c->d_kf_c, c->kf_c_used + n_corner, c->kf_c_used, c->stream);
  if (!rc) rc = grow(c->d_kf_s, c->kf_s_used + n_surf, c->kf_s_used, c->stream);
  if (rc) return rc;
  if (n_corner)
    CK(hipMemcpyAsync(c->d_kf_c + c->kf_c_used, corner, sizeof(float4) * n_corner, hipMemcpyHostToDevice, c->stream));
  if (n_surf) CK(hipMemcpyAsync(c->d_kf_s + c->kf_s_used, surf, sizeof(float4) * n_surf, hipMemcpyHostToDevice, c->stream));
  CK(fbr_sync(c->stream));
  fbr_keypose p = *pose;
  p.intensity = (float)c->kf_poses.size();  // "this can be used as index" (:1687, :1694)
  c->kf_poses.push_back(p);
  c->kf_c_off.push_back(c->kf_c_used);
  c->kf_c_cnt.push_back(n_corner);
  c->kf_s_off.push_back(c->kf_s_used);
  c->kf_s_cnt.push_back(n_surf);
  c->kf_c_used += n_corner;
  c->kf_s_used += n_surf;
  return FBR_OK;
}

int fbr_keyframes_set_pose(fbr_ctx* c, int64_t index, const fbr_keypose* pose) {
  if (!c || !pose || index < 0 || index >= (int64_t)c->kf_poses.size()) return FBR_ERR_INVALID_ARG;
  fbr_keypose& k = c->kf_poses[index];  // correctPoses (:1746-1757): x, y, z, roll, pitch, yaw
  k.x = pose->x;
  k.y = pose->y;
  k.z = pose->z;
  k.roll = pose->roll;
  k.pitch = pose->pitch;
  k.yaw = pose->yaw;
  return FBR_OK;
}

int fbr_keyframes_count(fbr_ctx* c, int64_t* n) {
  if (!c || !n) return FBR_ERR_INVALID_ARG;
  *n = (int64_t)c->kf_poses.size();
  return FBR_OK;
}

int fbr_keyframes_reset(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  c->kf_poses.clear();
  c->kf_c_off.clear();
  c->kf_c_cnt.clear();
  c->kf_s_off.clear();
  c->kf_s_cnt.clear();
  c->kf_c_used = c->kf_s_used = 0;
  c->sc_n = 0;  // the scan-context descriptors go with their keyframes (fbr_sc.hip)
  c->pg_factors.clear();  // ... and so do the pose graph's factors and its result (fbr_pg.hip)
  c->pg_result_n = -1;
  gmap_drop(c);  // ... and the global map built from them (fbr_gmap.hip)
  return FBR_OK;
}

int fbr_extract_surrounding_keyframes(fbr_ctx* c, double stamp, const fbr_keyframe_params* kp, int64_t* n_corner_map,
                                      int64_t* n_surf_map, int32_t* n_frames) {
  if (!c || !kp || !(kp->search_radius >= 0) || !(kp->pose_density > 0)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  if (n_frames) *n_frames = 0;
  const int64_t N = (int64_t)c->kf_poses.size();
  if (N == 0) {  // extractSurroundingKeyFrames (:967-968): nothing to extract, map unchanged
    if (n_corner_map) *n_corner_map = c->map_nocrop ? c->kds_c_n : 0;
    if (n_surf_map) *n_surf_map = c->map_nocrop ? c->kds_s_n : 0;
    return FBR_OK;
  }
  const fbr_keypose& back = c->kf_poses.back();
  std::vector<fbr_keypose> toExtract;  // cloudToExtract (x, y, z, intensity = key index)
  if (kp->loop_closure) {  // extractForLoopClosure (:857-870)
    for (int64_t i = N - 1; i >= 0; --i) {
      if ((int)toExtract.size() <= kp->submap_size) toExtract.push_back(c->kf_poses[i]);
      else break;
    }
  } else {  // extractNearby (:872-907)
    // kdtreeSurroundingKeyPoses->radiusSearch(back, radius): d2 = ((dx dx + dy dy) + dz dz) < r^2,
    // sorted by distance (ties by index)
    const float r2 = (float)((double)kp->search_radius * (double)kp->search_radius);
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
    std::vector<fbr_point_xyzi> sur(hits.size());
    for (size_t k = 0; k < hits.size(); ++k) {
      const fbr_keypose& q = c->kf_poses[hits[k].second];
      sur[k] = fbr_point_xyzi{q.x, q.y, q.z, q.intensity};
    }
    std::vector<fbr_point_xyzi> ds;  // downSizeFilterSurroundingKeyPoses (leaf surroundingKeyframeDensity)
    const int rc = voxel_grid_once(c, sur.data(), (int64_t)sur.size(), kp->pose_density, ds);
    if (rc) return rc;
    for (const fbr_point_xyzi& p : ds) {
      fbr_keypose k{};
      k.x = p.x;
      k.y = p.y;
      k.z = p.z;
      k.intensity = p.intensity;
      toExtract.push_back(k);
    }
    for (int64_t i = N - 1; i >= 0; --i) {  // the last recent_window seconds of keyframes (:896-904)
      if (stamp - c->kf_poses[i].time < kp->recent_window) toExtract.push_back(c->kf_poses[i]);
      else break;
    }
  }
  // extractCloud (:909-955): transform + concatenate the selected keyframes' clouds, then DS
  std::vector<KfSeg> segs;
  int64_t tot_c = 0, tot_s = 0, max_cnt = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (const fbr_keypose& e : toExtract) {
      if (key_distance(e, back) > kp->search_radius) continue;  // :924-925
      const int k = (int)e.intensity;                              // :927
      if (k < 0 || k >= N) return FBR_ERR_STATE;
      const fbr_keypose& pose = c->kf_poses[k];
      KfSeg g;
      const float tr[6] = {pose.roll, pose.pitch, pose.yaw, pose.x, pose.y, pose.z};
      float m[16];
      fbr_affine_from_pose(tr, m);  // pcl::getTransformation(x, y, z, roll, pitch, yaw), host libm
      for (int q = 0; q < 12; ++q) g.T[q] = m[q];
      if (pass == 0) {
        g.src = c->kf_c_off[k];
        g.count = c->kf_c_cnt[k];
        g.dst = tot_c;
        tot_c += g.count;
      } else {
        g.src = c->kf_s_off[k];
        g.count = c->kf_s_cnt[k];
        g.dst = tot_s;
        tot_s += g.count;
      }
      max_cnt = std::max(max_cnt, g.count);
      segs.push_back(g);
    }
  }
  const int nseg_c = (int)(segs.size() / 2);
  if (n_frames) *n_frames = (int32_t)toExtract.size();
  int rc = grow(c->d_kraw_c, std::max<int64_t>(tot_c, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_kraw_s, std::max<int64_t>(tot_s, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_kf_segs, std::max<int64_t>((int64_t)segs.size(), 1), 0, c->stream);
  if (rc) return rc;
  if (!segs.empty())
    CK(hipMemcpyAsync(c->d_kf_segs, segs.data(), sizeof(KfSeg) * segs.size(), hipMemcpyHostToDevice, c->stream));
  launch_kf_transform(c->stream, c->d_kf_c, c->d_kf_segs, nseg_c, max_cnt, c->d_kraw_c);
  launch_kf_transform(c->stream, c->d_kf_s, c->d_kf_segs + nseg_c, (int)segs.size() - nseg_c, max_cnt, c->d_kraw_s);
  CK(hipGetLastError());
  c->d_kds_c.reset();
  c->d_kds_s.reset();
  if (dalloc(c->d_kds_c, std::max<int64_t>(tot_c, 1)) || dalloc(c->d_kds_s, std::max<int64_t>(tot_s, 1))) {
    (void)fbr_sync(c->stream);  // the pageable copy of `segs` must finish before it goes out of scope
    return FBR_ERR_HIP;
  }
  // downSizeFilterCorner / downSizeFilterSurf (:946-954)
  rc = voxel_grid_dev(c, c->d_kraw_c, tot_c, c->P.mapping_corner_leaf_size, c->d_kds_c, &c->kds_c_n);
  if (!rc) rc = voxel_grid_dev(c, c->d_kraw_s, tot_s, c->P.mapping_surf_leaf_size, c->d_kds_s, &c->kds_s_n);
  // the kNN grids (both maps share one cell size, as in fbr_set_map)
  if (!rc) rc = build_map_grids(c, c->d_kds_c, c->kds_c_n, c->d_kds_s, c->kds_s_n);
  c->has_map = rc == FBR_OK;
  c->map_nocrop = rc == FBR_OK;
  c->crop_cached = false;
  c->map_c_host.clear();
  c->map_s_host.clear();
  c->map_host_stale = false;
  c->d_inst_c.reset();
  c->d_inst_s.reset();
  if (rc) return rc;
  if (n_corner_map) *n_corner_map = c->kds_c_n;
  if (n_surf_map) *n_surf_map = c->kds_s_n;
  return FBR_OK;
}

}  // extern "C"
