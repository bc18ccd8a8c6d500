// k_reg_info.hip — registration information (include/fbr.h "registration information", DESIGN
// §4.13): the Gauss-Newton normal matrix of a scan at a given pose, and the record made from it.
//
//   k_reg_info_items  one workgroup per (job, kind, block of 256 queries), the shape of the
//                     Gauss-Newton items.  One lane per query: q = T p, the 5-NN walk of
//                     fbr_grid_search.h (knn5_grid, the per-row loop, no warm start), the fit of the
//                     five neighbours and the row (fbr_gn.h: corner_fit / surf_fit, res_apply_row),
//                     with no fit cache.  The 21 + 6 products, the row count and b^2 are formed in
//                     double and summed in a fixed tree: the transposed butterfly of res_reduce
//                     inside each wave, then the four waves in order.  One partial per item.
//   k_reg_info_jobs   one wave per job: lanes 0..28 sum the job's partials in item order (corner
//                     items, then surf items), lane 0 runs fbr_reg_info.h's record (the 6x6 Jacobi in
//                     double, the covariance, the chart) on matrices in LDS, the wave writes it out.
//
// A job is a pose of fbr_reg_info_poses (every job reads the same clouds: stride 0) or a job of the
// latest batch launch (its own down-sampled clouds and counts).  No float or double atomics: a
// record depends on its pose, its clouds and the map alone.
#include "fbr_gn.h"
#include "fbr_reg_info.h"

namespace fbr {

namespace {

__device__ __forceinline__ bool info_pose_finite(const float* p) {
  bool ok = true;
  for (int k = 0; k < 6; ++k) ok = ok && (__float_as_uint(p[k]) & 0x7f800000u) != 0x7f800000u;
  return ok;
}

// FBR_INFO_NOT_REGISTERED or 0 (batch jobs; a pose of fbr_reg_info_poses has neither array)
__device__ __forceinline__ int info_job_flags(const InfoArgs& a, int job) {
  const bool bad = (a.stats && a.stats[job].status != FBR_REG_OK) || (a.err && a.err[job] != 0);
  return bad ? FBR_INFO_NOT_REGISTERED : 0;
}

// Product k of one row: 0-20 the upper H triangle, 21-26 g, 27 the count, 28 b^2, 29-31 zero.
__device__ __forceinline__ double info_product(int k, const float* row, float b, bool ok) {
  if (k < 28) return res_product(k, row, b, ok);
  if (k == 28) return (double)b * (double)b;
  return 0.0;
}

template <int R, int RX, bool kSparse>
__global__ void __launch_bounds__(kResThreads) k_reg_info_items(InfoArgs a) {
  __shared__ double red[kResThreads / 64][kInfoPartial];
  __shared__ GnState g;  // pose, T, trig and the crop box of the job: what the residual pass reads
  const int tid = (int)threadIdx.x;
  const int job = (int)blockIdx.x / a.ipp, it = (int)blockIdx.x - job * a.ipp;
  const bool corner = it < a.ipc;  // block-uniform, as everything up to the barrier
  const int first = (corner ? it : it - a.ipc) * kResThreads;
  const int n = corner ? (a.ncnt ? min(a.ncnt[job], a.nc) : a.nc) : (a.nscnt ? min(a.nscnt[job], a.ns) : a.ns);
  if (first >= n) return;  // the job has no such item: k_reg_info_jobs reads none beyond its counts
  const float* pose = a.poses + (int64_t)job * 6;
  if (info_job_flags(a, job) || !info_pose_finite(pose)) return;  // flagged by k_reg_info_jobs, no partial read
  if (tid == 0) {
    for (int k = 0; k < 6; ++k) g.pose[k] = pose[k];
    pose_to_T(g.pose, g.T, g.trig);
    for (int k = 0; k < 3; ++k) {  // registration's box, as k_gn_init stores it
      g.crop_min[k] = a.nocrop ? -FLT_MAX : -a.crop_half[k] + g.pose[3 + k];
      g.crop_max[k] = a.nocrop ? FLT_MAX : a.crop_half[k] + g.pose[3 + k];
    }
  }
  __syncthreads();
  float row[6] = {0, 0, 0, 0, 0, 0}, b = 0.0f;
  bool rok = false;
  const int i = first + tid;
  if (i < n) {
    const float4 p = corner ? a.corner[(int64_t)job * a.stride_c + i] : a.surf[(int64_t)job * a.stride_s + i];
    const float4 t = associate(g.T, p);
    const MapGrid& mg = corner ? a.mc : a.ms;
    Knn5 nn;
    unsigned ks[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    knn5_grid<R, RX, false, kSparse, 1>(mg, t.x, t.y, t.z, g.crop_min, g.crop_max, __int_as_float(0x7f800000), nn, ks);
    (void)ks;
    if (nn.k[4] < kKnnEmpty) {
      Nbr5 nb;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float4 q = mg.by_id[knn_id(nn.k[k])];
        nb.x[k] = q.x; nb.y[k] = q.y; nb.z[k] = q.z;
      }
      float fit[6];
      if (corner ? corner_fit(nb, fit) : surf_fit(nb, fit)) rok = res_apply_row(g, corner, fit, p, t.x, t.y, t.z, row, b);
    }
  }
  // the fixed tree: res_reduce's transposed butterfly over 32 values, then the waves in order
  const int lane = tid & 63, wave = tid >> 6;
  double v[16];
  const bool up5 = (lane & 32) != 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double lo = info_product(j, row, b, rok), hi = info_product(j + 16, row, b, rok);
    v[j] = (up5 ? hi : lo) + __shfl_xor(up5 ? lo : hi, 32);
  }
  res_halve<8, 16>(v, lane);
  res_halve<4, 8>(v, lane);
  res_halve<2, 4>(v, lane);
  res_halve<1, 2>(v, lane);
  v[0] += __shfl_xor(v[0], 1);
  const int ridx = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 +
                   ((lane >> 1) & 1);
  if (!(lane & 1)) red[wave][ridx] = v[0];
  __syncthreads();
  if (tid < kInfoPartial) {
    double s = 0.0;
    for (int w = 0; w < kResThreads / 64; ++w) s += red[w][tid];
    a.partial[(int64_t)blockIdx.x * kInfoPartial + tid] = s;
  }
}

struct InfoJobLds {
  double acc[kInfoPartial];
  double rows_c;
  InfoWork w;
  fbr_reg_info rec;
};

__global__ void __launch_bounds__(64) k_reg_info_jobs(InfoArgs a) {
  __shared__ InfoJobLds s;
  const int job = (int)blockIdx.x, lane = (int)threadIdx.x;
  const float* pose = a.poses + (int64_t)job * 6;
  const int flags = info_job_flags(a, job);
  const bool ran = !flags && info_pose_finite(pose);  // the item kernel wrote this job's partials
  const int nc = a.ncnt ? min(a.ncnt[job], a.nc) : a.nc, ns = a.nscnt ? min(a.nscnt[job], a.ns) : a.ns;
  // (the launch's item counts come from its largest job, so the minima change nothing)
  const int ic = min((nc + kResThreads - 1) / kResThreads, a.ipc), is = min((ns + kResThreads - 1) / kResThreads, a.ipp - a.ipc);
  const double* part = a.partial + (int64_t)job * a.ipp * kInfoPartial;
  if (lane < kInfoPartial) {
    double sum = 0.0;
    if (ran) {
      for (int it = 0; it < ic; ++it) sum += part[(int64_t)it * kInfoPartial + lane];
      if (lane == 27) s.rows_c = sum;  // the corner rows: the count so far
      for (int it = 0; it < is; ++it) sum += part[(int64_t)(a.ipc + it) * kInfoPartial + lane];
    } else if (lane == 27) {
      s.rows_c = 0.0;
    }
    s.acc[lane] = sum;
  }
  __syncthreads();
  if (lane == 0) {
    const int rc = (int)s.rows_c, rs = (int)s.acc[27] - rc;
    info_record(s.acc, rc, rs, ran ? nc : 0, ran ? ns : 0, pose, flags, a.eig_floor, a.unobserved, a.sigma2, &s.rec, &s.w);
  }
  __syncthreads();
  static_assert(sizeof(fbr_reg_info) % 8 == 0, "the record is copied as 64-bit words");
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&s.rec);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.out + job);
  for (int k = lane; k < (int)(sizeof(fbr_reg_info) / 8); k += 64) dst[k] = src[k];
}

template <int R, bool kSparse>
void launch_items_r(hipStream_t s, const InfoArgs& a, dim3 grid) {
  const float invx = a.mc.g.inv_x;  // == a.ms.g.inv_x
  if (invx > 4.0f) fbr_launch(k_reg_info_items<R, 8, kSparse>, grid, dim3(kResThreads), 0, s, a);       // 0.125 m
  else if (invx > 2.0f) fbr_launch(k_reg_info_items<R, 4, kSparse>, grid, dim3(kResThreads), 0, s, a);  // 0.25 m
  else if (invx > 1.0f) fbr_launch(k_reg_info_items<R, 2, kSparse>, grid, dim3(kResThreads), 0, s, a);  // 0.5 m
  else fbr_launch(k_reg_info_items<R, 1, kSparse>, grid, dim3(kResThreads), 0, s, a);                  // >= 1 m
}

template <bool kSparse>
void launch_items(hipStream_t s, const InfoArgs& a, dim3 grid) {
  const float inv = a.mc.g.inv_cell;  // == a.ms.g.inv_cell: y / z cells, as launch_gn_knn_f picks R
  if (inv > 2.0f) launch_items_r<4, kSparse>(s, a, grid);
  else if (inv > 1.0f) launch_items_r<2, kSparse>(s, a, grid);
  else launch_items_r<1, kSparse>(s, a, grid);
}

}  // namespace

void launch_reg_info_items(hipStream_t s, const InfoArgs& a) {
  if (a.n_jobs <= 0 || a.ipp <= 0) return;
  const dim3 grid((unsigned)((int64_t)a.n_jobs * a.ipp));
  if (a.mc.g.sparse || a.ms.g.sparse) launch_items<true>(s, a, grid);
  else launch_items<false>(s, a, grid);
}

void launch_reg_info_jobs(hipStream_t s, const InfoArgs& a) {
  if (a.n_jobs <= 0) return;
  fbr_launch(k_reg_info_jobs, dim3((unsigned)a.n_jobs), dim3(64), 0, s, a);
}

}  // namespace fbr
