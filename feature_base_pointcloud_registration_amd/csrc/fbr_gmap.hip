// fbr_gmap.hip — the global map (include/fbr.h, "global map"): built from the keyframe store at its
// current key poses, kept in HBM, read back, installed as the registration map, and saved as the
// reference's files.  Reference: visualizeGlobalMapThread's save block, mapOptmization.h:485-521.
//
// A build, per cloud (corner, surf):
//   1. the entries: every non-empty keyframe cloud in index order, with pcl::getTransformation of
//      its key pose (fbr_affine_from_pose, host libm), as fbr_extract_surrounding_keyframes does;
//   2. gmap_bounds over the pool through the entries (no concatenation is written): the finite
//      points' box, the count of the others, PCL's grid and its overflow condition;
//   3. PCL would overflow and the caller asked for the wide mode: voxel_grid_wide, straight from
//      the pool (k_gmap.hip);
//      otherwise: the concatenation (launch_kf_transform), less its non-finite points, through
//      voxel_grid_dev, which every other entry point uses and which returns its input on overflow;
//   4. the raw concatenation is kept only when the caller asked for it.
#include "fbr_ctx.h"

namespace {

// One cloud of a build.  The outputs are the context's handles.
struct GmCloud {
  const float4* pool;
  const KfSeg* d_segs;
  int nseg;
  int64_t n, max_count;
  float leaf;
};

int shrink_into(fbr_ctx* c, Dev<float4>& big, int64_t n, Dev<float4>& out) {
  out.reset();
  if (dalloc(out, std::max<int64_t>(n, 1))) return FBR_ERR_HIP;
  if (n) CK(hipMemcpyAsync(out, big, sizeof(float4) * n, hipMemcpyDeviceToDevice, c->stream));
  CK(fbr_sync(c->stream));
  big.reset();
  return FBR_OK;
}

// The concatenation of g's entries less the non-finite points, in raw (n_raw points).
int materialise(fbr_ctx* c, const GmCloud& g, int64_t n_dropped, Dev<float4>& raw, int64_t* n_raw) {
  Dev<float4> all;
  if (dalloc(all, std::max<int64_t>(g.n, 1))) return FBR_ERR_HIP;
  launch_kf_transform(c->stream, g.pool, g.d_segs, g.nseg, g.max_count, all);
  CK(hipGetLastError());
  *n_raw = g.n - n_dropped;
  if (n_dropped == 0) {
    CK(fbr_sync(c->stream));
    raw = std::move(all);
    return FBR_OK;
  }
  if (dalloc(raw, std::max<int64_t>(*n_raw, 1))) return FBR_ERR_HIP;
  const int rc = gmap_compact_finite(c->stream, c->arena, all, g.n, raw, *n_raw);
  CK(fbr_sync(c->stream));  // `all` goes out of scope
  return rc;
}

int build_cloud(fbr_ctx* c, const GmCloud& g, bool wide, bool keep_raw, Dev<float4>& out, int64_t* n_out, Dev<float4>& raw,
                int64_t* n_raw, int32_t* overflow, int32_t* used_wide, int64_t* n_dropped) {
  *n_out = *n_raw = *n_dropped = 0;
  *overflow = *used_wide = 0;
  if (g.n <= 0) {
    if (dalloc(out, 1) || (keep_raw && dalloc(raw, 1))) return FBR_ERR_HIP;
    return FBR_OK;
  }
  const GmapSrc src{g.pool, g.d_segs, g.nseg, 1, g.n, g.max_count};
  GmapInfo info;
  int rc = gmap_bounds(c->stream, c->arena, src, g.leaf, &info);
  if (rc) return rc;
  *n_dropped = info.n_dropped;
  *overflow = info.has_grid ? info.G.pcl_overflow : 0;
  if (wide && *overflow) {
    GmapInfo done;
    rc = voxel_grid_wide(c->stream, c->arena, src, g.leaf, &info,
                         [&](int64_t n) -> float4* { return out.alloc((size_t)std::max<int64_t>(n, 1)) ? out.get() : nullptr; }, &done);
    if (rc) return rc;
    *n_out = done.n_out;
    *used_wide = 1;
    if (keep_raw) return materialise(c, g, info.n_dropped, raw, n_raw);
    *n_raw = g.n - info.n_dropped;
    return FBR_OK;
  }
  rc = materialise(c, g, info.n_dropped, raw, n_raw);
  if (rc) return rc;
  Dev<float4> ds;
  if (dalloc(ds, std::max<int64_t>(*n_raw, 1))) return FBR_ERR_HIP;
  rc = voxel_grid_dev(c, raw, *n_raw, g.leaf, ds, n_out);  // PCL's overflow: output = input
  if (rc) return rc;
  rc = shrink_into(c, ds, *n_out, out);
  if (!keep_raw) raw.reset();
  return rc;
}

int download(std::vector<fbr_point_xyzi>& h, const float4* d, int64_t n) {
  h.resize((size_t)n);
  if (n) CK(fbr_memcpy_sync(h.data(), d, sizeof(float4) * n, hipMemcpyDeviceToHost));
  return FBR_OK;
}

}  // namespace

namespace fbr {
namespace internal {

void gmap_drop(fbr_ctx* c) {
  c->gm_built = c->gm_has_raw = false;
  c->d_gm_c.reset();
  c->d_gm_s.reset();
  c->d_gm_raw_c.reset();
  c->d_gm_raw_s.reset();
  c->gm_c_n = c->gm_s_n = c->gm_raw_c_n = c->gm_raw_s_n = 0;
  c->gm_poses.clear();
}

}  // namespace internal
}  // namespace fbr

extern "C" {

void fbr_gmap_params_default(fbr_gmap_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));  // the context's mapping leaves, PCL semantics, no raw clouds
}

int fbr_global_map_build(fbr_ctx* c, const fbr_gmap_params* gp, fbr_gmap_result* res) {
  if (!c) return FBR_ERR_INVALID_ARG;
  fbr_gmap_params P;
  fbr_gmap_params_default(&P);
  if (gp) P = *gp;
  if ((P.wide != 0 && P.wide != 1) || (P.keep_raw != 0 && P.keep_raw != 1)) return FBR_ERR_INVALID_ARG;
  const float leaf_c = P.corner_leaf > 0 ? P.corner_leaf : c->P.mapping_corner_leaf_size;
  const float leaf_s = P.surf_leaf > 0 ? P.surf_leaf : c->P.mapping_surf_leaf_size;
  if (!(leaf_c > 0) || !(leaf_s > 0) || !std::isfinite(leaf_c) || !std::isfinite(leaf_s)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  CK(fbr_sync(c->stream));
  gmap_drop(c);
  fbr_gmap_result R;
  std::memset(&R, 0, sizeof(R));
  if (res) *res = R;
  const int64_t N = (int64_t)c->kf_poses.size();
  R.n_keyframes = N;
  // the entries, corner then surf: non-empty clouds in keyframe order
  std::vector<KfSeg> segs[2];
  int64_t tot[2] = {0, 0}, max_cnt[2] = {0, 0};
  for (int64_t k = 0; k < N; ++k) {
    const fbr_keypose& pose = c->kf_poses[k];
    const float tr[6] = {pose.roll, pose.pitch, pose.yaw, pose.x, pose.y, pose.z};
    float m[16];
    fbr_affine_from_pose(tr, m);  // pcl::getTransformation(x, y, z, roll, pitch, yaw), host libm
    for (int w = 0; w < 2; ++w) {
      KfSeg g;
      g.src = w == 0 ? c->kf_c_off[k] : c->kf_s_off[k];
      g.count = w == 0 ? c->kf_c_cnt[k] : c->kf_s_cnt[k];
      if (g.count <= 0) continue;
      g.dst = tot[w];
      for (int q = 0; q < 12; ++q) g.T[q] = m[q];
      tot[w] += g.count;
      max_cnt[w] = std::max(max_cnt[w], g.count);
      segs[w].push_back(g);
    }
  }
  const int64_t ns0 = (int64_t)segs[0].size(), ns1 = (int64_t)segs[1].size();
  if (ns0 > INT32_MAX || ns1 > INT32_MAX) return FBR_ERR_CAPACITY;
  int rc = grow(c->d_gm_segs, std::max<int64_t>(ns0 + ns1, 1), 0, c->stream);
  if (rc) return rc;
  if (ns0) CK(fbr_memcpy_sync(c->d_gm_segs, segs[0].data(), sizeof(KfSeg) * ns0, hipMemcpyHostToDevice));
  if (ns1) CK(fbr_memcpy_sync(c->d_gm_segs + ns0, segs[1].data(), sizeof(KfSeg) * ns1, hipMemcpyHostToDevice));
  const GmCloud gc{c->d_kf_c, c->d_gm_segs, (int)ns0, tot[0], max_cnt[0], leaf_c};
  const GmCloud gs{c->d_kf_s, c->d_gm_segs + ns0, (int)ns1, tot[1], max_cnt[1], leaf_s};
  int64_t drop_c = 0, drop_s = 0;
  rc = build_cloud(c, gc, P.wide != 0, P.keep_raw != 0, c->d_gm_c, &c->gm_c_n, c->d_gm_raw_c, &c->gm_raw_c_n,
                   &R.corner_overflow, &R.corner_wide, &drop_c);
  if (!rc)
    rc = build_cloud(c, gs, P.wide != 0, P.keep_raw != 0, c->d_gm_s, &c->gm_s_n, c->d_gm_raw_s, &c->gm_raw_s_n,
                     &R.surf_overflow, &R.surf_wide, &drop_s);
  if (rc) {
    (void)fbr_sync(c->stream);
    gmap_drop(c);
    return rc;
  }
  c->gm_built = true;
  c->gm_has_raw = P.keep_raw != 0;
  c->gm_poses = c->kf_poses;
  R.n_corner_raw = c->gm_raw_c_n;
  R.n_surf_raw = c->gm_raw_s_n;
  R.n_corner = c->gm_c_n;
  R.n_surf = c->gm_s_n;
  R.n_dropped = drop_c + drop_s;
  if (res) *res = R;
  return FBR_OK;
}

int fbr_global_map_get(fbr_ctx* c, int64_t* n_corner, int64_t* n_surf, fbr_point_xyzi* corner, fbr_point_xyzi* surf) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (!c->gm_built) return FBR_ERR_STATE;
  CK(enter(c));
  if (n_corner) *n_corner = c->gm_c_n;
  if (n_surf) *n_surf = c->gm_s_n;
  if (corner && c->gm_c_n) CK(fbr_memcpy_sync(corner, c->d_gm_c, sizeof(float4) * c->gm_c_n, hipMemcpyDeviceToHost));
  if (surf && c->gm_s_n) CK(fbr_memcpy_sync(surf, c->d_gm_s, sizeof(float4) * c->gm_s_n, hipMemcpyDeviceToHost));
  return FBR_OK;
}

int fbr_global_map_install(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (!c->gm_built) return FBR_ERR_STATE;
  CK(enter(c));
  return set_map_device(c, c->d_gm_c, c->gm_c_n, c->d_gm_s, c->gm_s_n);
}

int fbr_global_map_save(fbr_ctx* c, const char* dir, int32_t flags) {
  if (!c || !dir || (flags & ~FBR_GMAP_SAVE_GLOBAL)) return FBR_ERR_INVALID_ARG;
  if (!c->gm_built) return FBR_ERR_STATE;
  CK(enter(c));
  const std::string d = std::string(dir) + "/";
  std::vector<fbr_point_xyzi> h;
  int rc = download(h, c->d_gm_c, c->gm_c_n);
  if (!rc) rc = fbr_pcd_write_ascii((d + "cloudCorner.pcd").c_str(), h.data(), (int64_t)h.size());
  if (!rc) rc = download(h, c->d_gm_s, c->gm_s_n);
  if (!rc) rc = fbr_pcd_write_ascii((d + "cloudSurf.pcd").c_str(), h.data(), (int64_t)h.size());
  if (rc) return rc;
  h.resize(c->gm_poses.size());
  for (size_t k = 0; k < h.size(); ++k) {
    const fbr_keypose& q = c->gm_poses[k];
    h[k] = fbr_point_xyzi{q.x, q.y, q.z, q.intensity};
  }
  rc = fbr_pcd_write_ascii((d + "trajectory.pcd").c_str(), h.data(), (int64_t)h.size());
  if (!rc) rc = fbr_pcd_write_poses_ascii((d + "transformations.pcd").c_str(), c->gm_poses.data(), (int64_t)c->gm_poses.size());
  if (rc || !(flags & FBR_GMAP_SAVE_GLOBAL) || !c->gm_has_raw) return rc;
  // globalMapCloud = globalCornerCloud + globalSurfCloud (:507-508), both unfiltered
  std::vector<fbr_point_xyzi> g((size_t)(c->gm_raw_c_n + c->gm_raw_s_n));
  if (c->gm_raw_c_n) CK(fbr_memcpy_sync(g.data(), c->d_gm_raw_c, sizeof(float4) * c->gm_raw_c_n, hipMemcpyDeviceToHost));
  if (c->gm_raw_s_n)
    CK(fbr_memcpy_sync(g.data() + c->gm_raw_c_n, c->d_gm_raw_s, sizeof(float4) * c->gm_raw_s_n, hipMemcpyDeviceToHost));
  return fbr_pcd_write_ascii((d + "cloudGlobal.pcd").c_str(), g.data(), (int64_t)g.size());
}

int fbr_selftest_voxel_wide(fbr_ctx* c, const fbr_point_xyzi* in, int64_t n, float leaf, fbr_point_xyzi* out, int64_t* n_out) {
  if (!c || n < 0 || (n && !in) || !(leaf > 0) || !n_out) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  *n_out = 0;
  // a host cloud with a non-finite point is not dense: the filter runs over the finite points alone
  std::vector<fbr_point_xyzi> fin;
  fin.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    if (std::isfinite(in[i].x) && std::isfinite(in[i].y) && std::isfinite(in[i].z)) fin.push_back(in[i]);
  const int64_t m = (int64_t)fin.size();
  if (m == 0) return FBR_OK;
  if (m > (int64_t)INT32_MAX) return FBR_ERR_CAPACITY;
  Dev<float4> d_in, d_out;
  Dev<KfSeg> d_seg;
  if (dalloc(d_in, m) || dalloc(d_seg, 1)) return FBR_ERR_HIP;
  KfSeg g{};
  g.count = m;
  CK(fbr_memcpy_sync(d_in, fin.data(), sizeof(float4) * m, hipMemcpyHostToDevice));
  CK(fbr_memcpy_sync(d_seg, &g, sizeof(g), hipMemcpyHostToDevice));
  const GmapSrc src{d_in, d_seg, 1, 0, m, m};
  GmapInfo info;
  const int rc = voxel_grid_wide(c->stream, c->arena, src, leaf, nullptr,
                                 [&](int64_t k) -> float4* { return d_out.alloc((size_t)std::max<int64_t>(k, 1)) ? d_out.get() : nullptr; },
                                 &info);
  if (rc) return rc;
  if (out && info.n_out) CK(fbr_memcpy_sync(out, d_out, sizeof(float4) * info.n_out, hipMemcpyDeviceToHost));
  *n_out = info.n_out;
  return FBR_OK;
}

}  // extern "C"
