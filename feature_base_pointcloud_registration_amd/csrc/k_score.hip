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
// The search prunes with the float lower bounds of fbr_gn.h (axis_lb: composed in the distance's own
// operation order they never exceed the d2 computed for any point of the cell), strictly: a cell
// whose bound equals the best d2 so far is still scanned, so among equal distances the lowest map
// index wins, as the 64-bit minimum says.  The cells are visited near side first along z, then y
// (rank_offset): the bounds do not decrease along a rank, so the first one past the cut ends its
// loop.  Unlike the 5-NN search the row window is a run-time loop (R, RX are launch arguments, not
// template parameters): one key is carried instead of five, nothing is unrolled into registers.
// No float or double atomics: a pose's record depends on the pose, the clouds and the map alone.
#include <math.h>

#include "fbr_gn.h"

namespace fbr {

namespace {

constexpr unsigned long long kScoreNone = ~0ull;

// The nearest map point of q with d2 < g2 among the points inside the crop box (crop = false: among
// all of them), or kScoreNone.  R / RX: cells covering 1 m along y, z / along x (g2 <= 1).
template <bool kSparse>
__device__ __forceinline__ unsigned long long score_nn1(const MapGrid& m, int R, int RX, float qx, float qy, float qz,
                                                        float g2, bool crop, const float* box) {
  if (m.g.n_points <= 0) return kScoreNone;
  const float inv = m.g.inv_cell, c = 1.0f / inv, invx = m.g.inv_x, cxs = 1.0f / invx;
  const float sx = qx * invx, sy = qy * inv, sz = qz * inv;
  const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
  // a non-finite q fails here too; cell indices beyond 1e7 are not exact in float, and such a query
  // is further than 1 m from every cell of the grid
  if (!(fabsf(fx) < 1e7f && fabsf(fy) < 1e7f && fabsf(fz) < 1e7f)) return kScoreNone;
  const int cx = (int)fx - (int)m.g.origin[0], cy = (int)fy - (int)m.g.origin[1], cz = (int)fz - (int)m.g.origin[2];
  const int X = m.g.dims[0], Y = m.g.dims[1], Z = m.g.dims[2];
  if (cx < -RX || cy < -R || cz < -R || cx >= X + RX || cy >= Y + R || cz >= Z + R) return kScoreNone;
  const int sgy = (sy - fy) >= 0.5f ? 1 : -1, sgz = (sz - fz) >= 0.5f ? 1 : -1;
  const float bx0 = box[0], by0 = box[1], bz0 = box[2], bx1 = box[3], by1 = box[4], bz1 = box[5];
  const float xlo = (fx - (float)RX) * cxs, xhi = (fx + (float)(RX + 1)) * cxs;  // a row's x extent at most
  const bool xin = xlo >= bx0 && xhi <= bx1;
  // empty = (bits(g2), 0): only a point with d2 < g2 is below it, whatever its index
  const unsigned long long empty = (unsigned long long)(unsigned)__float_as_int(g2) << 32;
  unsigned long long best = empty;
  float bestd = g2;
  // "bound <= best d2 and bound < g2": past either, no point of the cell can become the key
  auto past = [&](float lb) { return lb > bestd || lb >= g2; };
  for (int kz = 0; kz <= 2 * R; ++kz) {
    const int oz = rank_offset(kz, sgz);
    const float lz = axis_lb(qz, fz, oz, c), lz2 = lz * lz;
    if (past(lz2)) break;
    const int z = cz + oz;
    if (z < 0 || z >= Z) continue;
    const float zlo = (fz + (float)oz) * c;
    for (int ky = 0; ky <= 2 * R; ++ky) {
      const int oy = rank_offset(ky, sgy);
      const float ly = axis_lb(qy, fy, oy, c), ly2 = ly * ly;
      float lb = 0.0f;
      lb += ly2;
      lb += lz2;
      if (past(lb)) break;
      const int y = cy + oy;
      if (y < 0 || y >= Y) continue;
      int xa = 0, xb = 0;
      bool go_a = true, go_b = true;
      for (int o = 1; o <= RX; ++o) {
        const float la = axis_lb(qx, fx, -o, cxs), lp = axis_lb(qx, fx, o, cxs);
        float ta = 0.0f, tb = 0.0f;
        ta += la * la; ta += ly2; ta += lz2;
        tb += lp * lp; tb += ly2; tb += lz2;
        go_a = go_a && !past(ta);
        go_b = go_b && !past(tb);
        if (go_a) xa = -o;
        if (go_b) xb = o;
      }
      const int x0 = max(cx + xa, 0), x1 = min(cx + xb, X - 1);
      if (x0 > x1) continue;
      int b, e;
      if (!row_range<kSparse>(m, y, z, x0, x1, b, e)) continue;
      // the whole row inside the crop box (pcl::CropBox, inclusive): no per-point test
      const float ylo = (fy + (float)oy) * c;
      const bool inside = !crop || (xin & (ylo >= by0) & (ylo + c <= by1) & (zlo >= bz0) & (zlo + c <= bz1));
      for (int i = b; i < e; ++i) {
        const float4 p = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(m.pts) + (uint32_t)i * 16u);
        float dist = 0.0f, diff;
        diff = qx - p.x; dist += diff * diff;  // flann::L2_Simple
        diff = qy - p.y; dist += diff * diff;
        diff = qz - p.z; dist += diff * diff;
        unsigned hi = (unsigned)__float_as_int(dist);
        if (!inside && crop_out(p, bx0, by0, bz0, bx1, by1, bz1)) hi = 0x7f800000u;
        const unsigned long long key = ((unsigned long long)hi << 32) | (unsigned)__float_as_int(p.w);
        best = key < best ? key : best;
      }
      bestd = knn_d(best);
    }
  }
  return best < empty ? best : kScoreNone;
}

template <bool kSparse>
__global__ void __launch_bounds__(256) k_score_nn(ScoreArgs a) {
  __shared__ double sh_sum[4];
  __shared__ int sh_cnt[4];
  const int pose = (int)blockIdx.x / a.ipp, it = (int)blockIdx.x - pose * a.ipp;
  const bool corner = it < a.ipc;  // block-uniform
  const int n = corner ? a.nc : a.ns;
  const int i = (corner ? it : it - a.ipc) * 256 + (int)threadIdx.x;
  unsigned long long key = kScoreNone;
  if (i < n) {
    const float4 p = corner ? a.corner[i] : a.surf[i];
    const float* T = a.T + (int64_t)pose * kScorePose;
    // pointAssociateToMap: three products and three sums per coordinate, each rounded
    const float qx = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
    const float qy = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
    const float qz = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
    key = score_nn1<kSparse>(corner ? a.mc : a.ms, a.R, a.RX, qx, qy, qz, a.g2, a.use_crop != 0, T + 12);
    if (a.keys) a.keys[(int64_t)pose * (a.nc + a.ns) + (corner ? 0 : a.nc) + i] = key;
  }
  const bool in = key != kScoreNone;
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
