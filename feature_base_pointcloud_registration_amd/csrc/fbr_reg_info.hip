// fbr_reg_info.hip — registration information (include/fbr.h "registration information"): the
// clouds of fbr_reg_info_poses go to HBM once per call, the poses in chunks of
// fbr_info_params.pose_chunk; fbr_batch_info takes the latest launch's down-sampled clouds, counts,
// result poses and statuses from where the launch left them.  Each chunk is two launches
// (k_reg_info.hip) and one copy of its records back.  Everything runs on the primary stream over
// scratch of its own (fbr_ctx.h d_info_*).
//
// A cloud is summed in canonical order: its points sorted by the bit patterns of (x, y, z,
// intensity) before they go to the kernels (canonical_order, on the host: a call is a diagnostic
// read-out, not part of a launch chain).  A record therefore depends on which points a cloud holds
// and not on the order a VoxelGrid emitted them in: the batch's down-samples are in Morton voxel
// order, fbr_voxel_grid's in PCL key order, and both give the same bytes.
#include "fbr_ctx.h"

namespace {

constexpr int64_t kInfoChunk = 1024;                 // default jobs per launch
constexpr int64_t kInfoMaxItems = (int64_t)1 << 30;  // work items of one launch (a grid dimension)

bool info_params_ok(const fbr_info_params* ip) {
  return ip && std::isfinite(ip->eig_floor) && ip->eig_floor > 0.0 && std::isfinite(ip->unobserved_variance) &&
         ip->unobserved_variance > 0.0 && std::isfinite(ip->sigma2) && ip->sigma2 >= 0.0 && ip->pose_chunk >= 0;
}

// The canonical order of a cloud: ascending (x, y, z, intensity) compared as unsigned bit patterns
// (a total order on every float, NaNs included; equal points are equal rows, so ties do not matter).
void canonical_order(float4* p, int64_t n) {
  std::sort(p, p + n, [](const float4& a, const float4& b) {
    uint32_t ka[4], kb[4];
    std::memcpy(ka, &a, 16);
    std::memcpy(kb, &b, 16);
    for (int k = 0; k < 4; ++k)
      if (ka[k] != kb[k]) return ka[k] < kb[k];
    return false;
  });
}

// What every launch of a call shares: the map, the box, the parameters.
InfoArgs info_args(fbr_ctx* c, const fbr_info_params& ip) {
  InfoArgs a{};
  a.mc = c->grid_c.view();
  a.ms = c->grid_s.view();
  for (int k = 0; k < 3; ++k) a.crop_half[k] = c->P.crop_half[k];
  a.nocrop = c->map_nocrop ? 1 : 0;
  a.eig_floor = ip.eig_floor;
  a.unobserved = ip.unobserved_variance;
  a.sigma2 = ip.sigma2;
  return a;
}

int64_t info_chunk(const fbr_info_params& ip, int64_t n_jobs, int64_t ipp) {
  int64_t chunk = std::min<int64_t>(ip.pose_chunk > 0 ? ip.pose_chunk : kInfoChunk, n_jobs);
  if (ipp) chunk = std::min(chunk, std::max<int64_t>(1, kInfoMaxItems / ipp));
  return std::max<int64_t>(chunk, 1);
}

// One chunk: a (its job-indexed pointers already at the chunk's first job) -> out[0 .. n).
int info_launch(fbr_ctx* c, InfoArgs& a, int64_t n, fbr_reg_info* out) {
  a.n_jobs = (int32_t)n;
  a.partial = c->d_info_partial;
  a.out = c->d_info_out;
  TIMED(c, "reg_info_items", launch_reg_info_items(c->stream, a));
  TIMED(c, "reg_info_jobs", launch_reg_info_jobs(c->stream, a));
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, c->d_info_out, sizeof(fbr_reg_info) * n, hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));  // the scratch is reused by the next chunk
  return FBR_OK;
}

}  // namespace

extern "C" {

void fbr_info_params_default(fbr_info_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->eig_floor = 100.0;
  p->unobserved_variance = 1e4;
}

int fbr_reg_info_poses(fbr_ctx* c, const fbr_info_params* ip, const fbr_point_xyzi* corner, int64_t n_corner,
                       const fbr_point_xyzi* surf, int64_t n_surf, const float* poses, int64_t n_poses,
                       fbr_reg_info* out) {
  if (!c || !info_params_ok(ip) || n_corner < 0 || n_surf < 0 || (n_corner && !corner) || (n_surf && !surf) ||
      n_poses < 0 || (n_poses && (!poses || !out)))
    return FBR_ERR_INVALID_ARG;
  if (!c->has_map) return FBR_ERR_STATE;
  if (n_poses == 0) return FBR_OK;
  const int64_t npts = n_corner + n_surf;
  if (npts > INT32_MAX / 2) return FBR_ERR_CAPACITY;
  CK(enter(c));
  const int64_t ipc = (n_corner + 255) / 256, ipp = ipc + (n_surf + 255) / 256;
  const int64_t chunk = info_chunk(*ip, n_poses, ipp);
  int rc = grow(c->d_info_cloud, std::max<int64_t>(npts, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_info_pose, chunk * 6, 0, c->stream);
  if (!rc) rc = grow(c->d_info_partial, std::max<int64_t>(chunk * ipp * kInfoPartial, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_info_out, chunk, 0, c->stream);
  if (rc) return rc;
  std::vector<float4> host((size_t)std::max<int64_t>(npts, 1));  // outlives the copy: every chunk ends in a sync
  if (n_corner) std::memcpy(host.data(), corner, sizeof(float4) * n_corner);
  if (n_surf) std::memcpy(host.data() + n_corner, surf, sizeof(float4) * n_surf);
  canonical_order(host.data(), n_corner);
  canonical_order(host.data() + n_corner, n_surf);
  if (npts) CK(hipMemcpyAsync(c->d_info_cloud, host.data(), sizeof(float4) * npts, hipMemcpyHostToDevice, c->stream));
  InfoArgs a = info_args(c, *ip);
  a.corner = c->d_info_cloud;
  a.surf = c->d_info_cloud + n_corner;
  a.nc = (int32_t)n_corner;
  a.ns = (int32_t)n_surf;
  a.ipc = (int32_t)ipc;
  a.ipp = (int32_t)ipp;
  a.poses = c->d_info_pose;
  for (int64_t p0 = 0; p0 < n_poses; p0 += chunk) {
    const int64_t np = std::min(chunk, n_poses - p0);
    CK(hipMemcpyAsync(c->d_info_pose, poses + p0 * 6, sizeof(float) * 6 * np, hipMemcpyHostToDevice, c->stream));
    rc = info_launch(c, a, np, out + p0);
    if (rc) return rc;
  }
  return FBR_OK;
}

int fbr_batch_info(fbr_ctx* c, const fbr_info_params* ip, fbr_reg_info* out) {
  if (!c || !info_params_ok(ip) || !out) return FBR_ERR_INVALID_ARG;
  if (c->staged_B <= 0 || c->last_slot < 0 || !c->has_map) return FBR_ERR_STATE;
  CK(enter(c));
  int rc = batch_quiesce(c);
  if (rc) return rc;
  CK(fbr_sync(c->stream));
  for (const GnRun& r : c->run)
    for (int k = 0; k < r.nsub; ++k) CK(fbr_sync(r.s[k].sub.st));
  // the launch's slot keeps its down-sampled clouds, counts, result poses and statuses until the
  // slot's next launch; the clouds come to the host for their canonical order, the rest is read in place
  const int64_t B = c->staged_B, w0 = (int64_t)c->last_slot * c->Bcap, HW = c->HW;
  std::vector<int32_t> cnt((size_t)(2 * B));
  CK(hipMemcpyAsync(cnt.data(), c->d_ncds + w0, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
  CK(hipMemcpyAsync(cnt.data() + B, c->d_nsds + w0, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  int64_t mc = 0, ms = 0;
  for (int64_t j = 0; j < 2 * B; ++j) {
    cnt[(size_t)j] = (int32_t)std::min<int64_t>(std::max<int32_t>(cnt[(size_t)j], 0), HW);
    (j < B ? mc : ms) = std::max<int64_t>(j < B ? mc : ms, cnt[(size_t)j]);
  }
  const int64_t ipc = (mc + 255) / 256, ipp = ipc + (ms + 255) / 256;
  const int64_t chunk = info_chunk(*ip, B, ipp);
  rc = grow(c->d_info_cloud, std::max<int64_t>(chunk * (mc + ms), 1), 0, c->stream);
  if (!rc) rc = grow(c->d_info_partial, std::max<int64_t>(chunk * ipp * kInfoPartial, 1), 0, c->stream);
  if (!rc) rc = grow(c->d_info_out, chunk, 0, c->stream);
  if (rc) return rc;
  std::vector<float4> host((size_t)std::max<int64_t>(chunk * (mc + ms), 1));
  for (int64_t j0 = 0; j0 < B; j0 += chunk) {
    const int64_t nj = std::min(chunk, B - j0), w = w0 + j0;
    // job k's corner points at host[k * mc], its surf points at host[nj * mc + k * ms]
    float4* hs = host.data() + nj * mc;
    for (int64_t k = 0; k < nj; ++k) {
      const int64_t nc = cnt[(size_t)(j0 + k)], ns = cnt[(size_t)(B + j0 + k)];
      if (nc)
        CK(hipMemcpyAsync(host.data() + k * mc, c->d_cornerDS + (w + k) * HW, sizeof(float4) * nc, hipMemcpyDeviceToHost,
                          c->stream));
      if (ns) CK(hipMemcpyAsync(hs + k * ms, c->d_surfDS + (w + k) * HW, sizeof(float4) * ns, hipMemcpyDeviceToHost, c->stream));
    }
    CK(fbr_sync(c->stream));
    // a sort per cloud, the jobs dealt out to a few host threads (as the ingest packs its chunks)
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(8, nj / 16));
    auto order = [&](int t) {
      for (int64_t k = t; k < nj; k += nt) {
        canonical_order(host.data() + k * mc, cnt[(size_t)(j0 + k)]);
        canonical_order(hs + k * ms, cnt[(size_t)(B + j0 + k)]);
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(order, t);
    order(0);
    for (auto& x : th) x.join();
    if (nj * (mc + ms))
      CK(hipMemcpyAsync(c->d_info_cloud, host.data(), sizeof(float4) * nj * (mc + ms), hipMemcpyHostToDevice, c->stream));
    InfoArgs a = info_args(c, *ip);
    a.corner = c->d_info_cloud;
    a.surf = c->d_info_cloud + nj * mc;
    a.stride_c = mc;
    a.stride_s = ms;
    a.nc = (int32_t)mc;
    a.ns = (int32_t)ms;
    a.ncnt = c->d_ncds + w;
    a.nscnt = c->d_nsds + w;
    a.ipc = (int32_t)ipc;
    a.ipp = (int32_t)ipp;
    a.poses = c->d_pose_out + w * 6;
    a.stats = c->d_stats + w;
    a.err = c->d_err + w;
    rc = info_launch(c, a, nj, out + j0);  // ends in a sync: host is free for the next chunk
    if (rc) return rc;
  }
  return FBR_OK;
}

int fbr_reg_info_variances(const fbr_reg_info* info, const double* floor, double* variances_out) {
  if (!info || !variances_out) return FBR_ERR_INVALID_ARG;
  for (int k = 0; k < 6; ++k) {
    const double v = info->var_tangent[k];
    variances_out[k] = floor && floor[k] > v ? floor[k] : v;
  }
  return FBR_OK;
}

}  // extern "C"
