// k_score.hip — pose scoring (include/fbr.h "pose scoring"): one scan's feature points
// against the registration map at many poses in one launch.
//
//   k_score_nn   one lane per (pose, point): q = T p in pointAssociateToMap's order, then the exact
//                nearest map point inside the distance gate over the map's kNN grid (dense or hashed
//                chunks), as the key (d2 bits << 32) | map index.  A workgroup is one work item
//                (pose, class, block of 256 points), the shape of the Gauss-Newton items; it writes
//                one partial: the inlier count and the inliers' d2 summed in double in a fixed tree
//                (a butterfly inside each wave, the four waves in order).
//   k_score_sum  one lane per pose: the pose's partials in item order, then the fbr_pose_score record.
//
// The search is nn1_grid (fbr_grid_search.h): strict pruning, so among equal distances the lowest
// map index wins; a run-time row window, one key carried.
// No float or double atomics: a pose's record depends on the pose, the clouds and the map alone.
#include <math.h>

#include "fbr_grid_search.h"

namespace fbr {

namespace {

template <bool kSparse>
__global__ void __launch_bounds__(256) k_score_nn(ScoreArgs a) {
  __shared__ double sh_sum[4];
  __shared__ int sh_cnt[4];
  const int pose = (int)blockIdx.x / a.ipp, it = (int)blockIdx.x - pose * a.ipp;
  const bool corner = it < a.ipc;  // block-uniform
  const int n = corner ? a.nc : a.ns;
  const int i = (corner ? it : it - a.ipc) * 256 + (int)threadIdx.x;
  unsigned long long key = kNnNone;
  if (i < n) {
    const float4 p = corner ? a.corner[i] : a.surf[i];
    const float* T = a.T + (int64_t)pose * kScorePose;
    const float4 q = associate(T, p);
    key = nn1_grid<kSparse>(corner ? a.mc : a.ms, a.R, a.RX, q.x, q.y, q.z, a.g2, a.use_crop != 0, T + 12);
    if (a.keys) a.keys[(int64_t)pose * (a.nc + a.ns) + (corner ? 0 : a.nc) + i] = key;
  }
  const bool in = key != kNnNone;
  double s = in ? (double)knn_d(key) : 0.0;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const int cnt = __popcll(__ballot(in));
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh_sum[wave] = s;
    sh_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScorePartial r;
    r.sum = ((sh_sum[0] + sh_sum[1]) + sh_sum[2]) + sh_sum[3];
    r.n_in = ((sh_cnt[0] + sh_cnt[1]) + sh_cnt[2]) + sh_cnt[3];
    r.pad = 0;
    a.partial[blockIdx.x] = r;
  }
}

__global__ void __launch_bounds__(256) k_score_sum(ScoreArgs a) {
  const int pose = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (pose >= a.n_poses) return;
  const ScorePartial* part = a.partial + (int64_t)pose * a.ipp;
  fbr_pose_score r;
  r.n[0] = a.nc;
  r.n[1] = a.ns;
  r.n_in[0] = r.n_in[1] = 0;
  r.sum_d2[0] = r.sum_d2[1] = 0.0;
  for (int it = 0; it < a.ipp; ++it) {
    const int k = it < a.ipc ? 0 : 1;
    r.n_in[k] += part[it].n_in;
    r.sum_d2[k] += part[it].sum;
  }
  const int n_total = a.nc + a.ns, n_in = r.n_in[0] + r.n_in[1];
  r.fitness = n_total > 0 ? ((r.sum_d2[0] + r.sum_d2[1]) + (double)(n_total - n_in) * (double)a.g2) / (double)n_total : DBL_MAX;
  a.out[pose] = r;
}

}  // namespace

void launch_score_nn(hipStream_t s, const ScoreArgs& a) {
  if (a.n_poses <= 0 || a.ipp <= 0) return;
  const dim3 grid((unsigned)((int64_t)a.n_poses * a.ipp));
  if (a.mc.g.sparse || a.ms.g.sparse) fbr_launch(k_score_nn<true>, grid, dim3(256), 0, s, a);
  else fbr_launch(k_score_nn<false>, grid, dim3(256), 0, s, a);
}

void launch_score_sum(hipStream_t s, const ScoreArgs& a) {
  if (a.n_poses <= 0) return;
  fbr_launch(k_score_sum, dim3((unsigned)((a.n_poses + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace fbr
