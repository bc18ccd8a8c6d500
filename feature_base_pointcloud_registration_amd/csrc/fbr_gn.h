// fbr_gn.h — device side of the Gauss-Newton step (A13-A15): the kNN pass over the map grids
// (gn_knn_block: the query at the job's pose, its warm-start bound, the search, the result write),
// the line and plane fits, the residual rows, the normal-equation reduction, the 6x6 solve and the
// host launchers of the kNN pass.  The search itself (keys, grid geometry, knn5_grid) is
// fbr_grid_search.h.  Shared by k_register.hip (init, residual, solve, finalize), k_knn_tile.hip and
// the k_knn_*.hip translation units, which instantiate the kNN kernels per cell radius R and fused
// flag (the instantiations compile in parallel; one file holding all of them took ~8 minutes).  See
// k_register.hip for the design notes and reference citations (mapOptmization.h:1002-1243,
// :1403-1442).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "fbr_common.h"
#include "fbr_grid_search.h"
#include "fbr_imu.h"
#include "fbr_kernels.h"
#include "fbr_knobs.h"
#include "fbr_solvers.h"

namespace fbr {

constexpr int kSolveThreads = 128;  // k_gn_solve: wave 0 sums + solves, wave 1 the iteration-0 degeneracy
constexpr int kPartial = 32;  // doubles per item partial: 21 AtA upper + 6 AtB + count

// cornerOptimization body (:1016-1121): coefficient row for one corner query, false if rejected.
struct Nbr5 {
  float x[5], y[5], z[5];
};

// The part of a correspondence that depends only on its 5 map neighbours: the corner line (two
// points 0.1 along the principal axis through the mean, after the eigenvalue-ratio gate) or the
// plane (pa, pb, pc, pd after the 0.2 m check).  A query whose kNN returns the same 5 neighbours as
// in the previous Gauss-Newton iteration reuses it (bit-identical: same inputs, same operations);
// only the query-dependent residual below is recomputed.  f[0..5]; false = rejected.
__device__ bool corner_fit(const Nbr5& nn, float* f) {
  float cx = 0, cy = 0, cz = 0;
  for (int j = 0; j < 5; j++) { cx += nn.x[j]; cy += nn.y[j]; cz += nn.z[j]; }
  cx /= 5.0f; cy /= 5.0f; cz /= 5.0f;
  float a11 = 0, a12 = 0, a13 = 0, a22 = 0, a23 = 0, a33 = 0;
  for (int j = 0; j < 5; j++) {
    const float ax = nn.x[j] - cx, ay = nn.y[j] - cy, az = nn.z[j] - cz;
    a11 += ax * ax; a12 += ax * ay; a13 += ax * az;
    a22 += ay * ay; a23 += ay * az;
    a33 += az * az;
  }
  a11 /= 5.0f; a12 /= 5.0f; a13 /= 5.0f; a22 /= 5.0f; a23 /= 5.0f; a33 /= 5.0f;
  float A1[9] = {a11, a12, a13, a12, a22, a23, a13, a23, a33};
  float D1[3], V1[9];
  jacobi_eigen<3>(A1, D1, V1);
  if (!(D1[0] > 3.0f * D1[1])) return false;
  f[0] = (float)((double)cx + 0.1 * (double)V1[0]);
  f[1] = (float)((double)cy + 0.1 * (double)V1[1]);
  f[2] = (float)((double)cz + 0.1 * (double)V1[2]);
  f[3] = (float)((double)cx - 0.1 * (double)V1[0]);
  f[4] = (float)((double)cy - 0.1 * (double)V1[1]);
  f[5] = (float)((double)cz - 0.1 * (double)V1[2]);
  return true;
}

// cornerOptimization's residual (:1083-1112) of query (x0, y0, z0) against the fitted line.
__device__ bool corner_apply(const float* f, float x0, float y0, float z0, float4& coeff) {
  const float x1 = f[0], y1 = f[1], z1 = f[2], x2 = f[3], y2 = f[4], z2 = f[5];
  const float a012 = sqrt_rn(((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) * ((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) +
                                ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)) * ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)) +
                                ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)) * ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)));
  const float l12 = sqrt_rn((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2));
  const float la = ((y1 - y2) * ((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) +
                    (z1 - z2) * ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1))) / a012 / l12;
  const float lb = -((x1 - x2) * ((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)) -
                     (z1 - z2) * ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1))) / a012 / l12;
  const float lc = -((x1 - x2) * ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)) +
                     (y1 - y2) * ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1))) / a012 / l12;
  const float ld2 = a012 / l12;
  const float s = (float)(1.0 - 0.9 * (double)fabsf(ld2));
  coeff = make_float4(s * la, s * lb, s * lc, s * ld2);
  return (double)s > 0.1;
}

// surfOptimization's plane (:1145-1186): f[0..3] = (pa, pb, pc, pd); false when a neighbour is
// more than 0.2 from it.
__device__ bool surf_fit(const Nbr5& nn, float* f) {
  float A0[5][3], B0[5], X0[3];
  for (int j = 0; j < 5; j++) { A0[j][0] = nn.x[j]; A0[j][1] = nn.y[j]; A0[j][2] = nn.z[j]; B0[j] = -1.0f; }
  colpiv_solve53(A0, B0, X0);
  float pa = X0[0], pb = X0[1], pc = X0[2], pd = 1.0f;
  const float ps = sqrt_rn(pa * pa + pb * pb + pc * pc);
  pa /= ps; pb /= ps; pc /= ps; pd /= ps;
  for (int j = 0; j < 5; j++)
    if ((double)fabsf(pa * nn.x[j] + pb * nn.y[j] + pc * nn.z[j] + pd) > 0.2) return false;
  f[0] = pa; f[1] = pb; f[2] = pc; f[3] = pd;
  return true;
}

// surfOptimization's residual (:1198-1211) of query (x0, y0, z0) against the plane.
__device__ bool surf_apply(const float* f, float x0, float y0, float z0, float4& coeff) {
  const float pa = f[0], pb = f[1], pc = f[2], pd = f[3];
  const float pd2 = pa * x0 + pb * y0 + pc * z0 + pd;
  const float s = (float)(1.0 - 0.9 * (double)fabsf(pd2) /
                                    (double)sqrt_rn(sqrt_rn(x0 * x0 + y0 * y0 + z0 * z0)));
  coeff = make_float4(s * pa, s * pb, s * pc, s * pd2);
  return (double)s > 0.1;
}

// Normal-equation product k of one row: 0-20 the upper AtA triangle, 21-26 AtB, 27 the count,
// 28-31 zero (compile-time k after unrolling).
__device__ __forceinline__ double res_product(int k, const float* row, float b, bool ok) {
  constexpr int kR[21] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5};
  constexpr int kC[21] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 2, 3, 4, 5, 3, 4, 5, 4, 5, 5};
  if (k < 21) return (double)row[kR[k]] * (double)row[kC[k]];
  if (k < 27) return (double)row[k - 21] * (double)b;
  if (k == 27) return ok ? 1.0 : 0.0;
  return 0.0;
}

// One transposed-butterfly step: H values per lane -> H/2 (the lower lane of each OFF pair keeps
// the first half, the upper lane the second).
template <int H, int OFF>
__device__ __forceinline__ void res_halve(double* v, int lane) {
  const bool up = (lane & OFF) != 0;
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const double lo = v[j], hi = v[j + H];
    v[j] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, OFF);
  }
}

// The residual of query (x0, y0, z0) against its fitted line / plane (corner_apply / surf_apply)
// and its LMOptimization row (:1286-1332); false when the correspondence is rejected.
__device__ __forceinline__ bool res_apply_row(const GnState& g, bool corner, const float* fit, const float4& p, float x0,
                                              float y0, float z0, float* row, float& b) {
  float4 c;
  const bool ok = corner ? corner_apply(fit, x0, y0, z0, c) : surf_apply(fit, x0, y0, z0, c);
  if (ok) {
    // camera-frame swap
    const float srx = g.trig[0], crx = g.trig[1], sry = g.trig[2], cry = g.trig[3], srz = g.trig[4], crz = g.trig[5];
    const float pox = p.y, poy = p.z, poz = p.x;
    const float cox = c.y, coy = c.z, coz = c.x;
    const float arx = (crx * sry * srz * pox + crx * crz * sry * poy - srx * sry * poz) * cox +
                      (-srx * srz * pox - crz * srx * poy - crx * poz) * coy +
                      (crx * cry * srz * pox + crx * cry * crz * poy - cry * srx * poz) * coz;
    const float ary = ((cry * srx * srz - crz * sry) * pox + (sry * srz + cry * crz * srx) * poy + crx * cry * poz) * cox +
                      ((-cry * crz - srx * sry * srz) * pox + (cry * srz - crz * srx * sry) * poy - crx * sry * poz) * coz;
    const float arz = ((crz * srx * sry - cry * srz) * pox + (-cry * crz - srx * sry * srz) * poy) * cox +
                      (crx * crz * pox - crx * srz * poy) * coy +
                      ((sry * srz + cry * crz * srx) * pox + (crz * sry - cry * srx * srz) * poy) * coz;
    row[0] = arz; row[1] = arx; row[2] = ary; row[3] = coz; row[4] = cox; row[5] = coy;
    b = -c.w;
  }
  return ok;
}

// cornerOptimization / surfOptimization + the LMOptimization row (:1286-1332) of one query whose 5
// neighbours are the map points nb[0..4] (map indices); false when the correspondence is rejected.
// fc / fs: the query's fit cache (fit floats at stride kResThreads, state 0 none / 1 fitted /
// 2 rejected); same: the neighbours equal the previous iteration's, whose fit the cache holds.
__device__ __forceinline__ bool res_row(const GnState& g, const float4* by_id, const int32_t* nb, int stride,
                                        bool corner, const float4& p, float x0, float y0, float z0, float* row,
                                        float& b, float* fc, int8_t* fs, bool same) {
  float fit[6];
  bool fit_ok;
  const int8_t st = same ? *fs : (int8_t)0;
  if (st != 0) {
    fit_ok = st == 1;
    if (fit_ok) {
#pragma unroll
      for (int k = 0; k < 6; ++k) fit[k] = fc[k * kResThreads];
    }
  } else {
    Nbr5 nn;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float4 q = by_id[nb[k * stride]];
      nn.x[k] = q.x; nn.y[k] = q.y; nn.z[k] = q.z;
    }
    fit_ok = corner ? corner_fit(nn, fit) : surf_fit(nn, fit);
    *fs = fit_ok ? 1 : 2;
    if (fit_ok) {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (corner || k < 4) fc[k * kResThreads] = fit[k];
    }
  }
  if (!fit_ok) return false;
  return res_apply_row(g, corner, fit, p, x0, y0, z0, row, b);
}

// The item's fp64 normal-equation partial (21 upper AtA entries, 6 AtB, count; 4 zero pads):
// every lane of the workgroup calls this with its row (zeros when it has none).  The wave sum is a
// transposed butterfly: at each halving step a lane keeps half of its values and trades the other
// half with its partner, so 32 values cost 32 shuffles instead of 6 per value.  Lane l (bit 0
// clear) ends with the wave sum of value ridx(l) (its bits 5..1 reversed); the 4 wave sums are
// added in LDS.  (A matrix-core form of this partial, v_mfma_f64_16x16x4 over the rows staged in
// LDS, bought 3 % of the kernel in round 4: the kernel is bound by its gathers and fits.)
__device__ __forceinline__ void res_reduce(double (*red)[28], int tid, const float* row, float b, bool ok,
                                           double* out) {
  const int lane = tid & 63, wave = tid >> 6;
  double v[16];
  const bool up5 = (lane & 32) != 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double lo = res_product(j, row, b, ok), hi = res_product(j + 16, row, b, ok);
    v[j] = (up5 ? hi : lo) + __shfl_xor(up5 ? lo : hi, 32);
  }
  res_halve<8, 16>(v, lane);
  res_halve<4, 8>(v, lane);
  res_halve<2, 4>(v, lane);
  res_halve<1, 2>(v, lane);
  v[0] += __shfl_xor(v[0], 1);
  const int ridx = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 +
                   ((lane >> 1) & 1);
  if (!(lane & 1) && ridx < 28) red[wave][ridx] = v[0];
  __syncthreads();
  if (tid < 28) {
    double s = 0.0;
    for (int w = 0; w < kResThreads / 64; ++w) s += red[w][tid];
    out[tid] = s;
  }
  __syncthreads();
}

// The warm-start bound of a query at (x0, y0, z0): the largest distance to the previous iteration's 5
// neighbours oid[] (knn5_grid's `bound`), in the search's own distance arithmetic.
__device__ __forceinline__ float warm_bound(const float4* by_id, const int32_t* oid, float x0, float y0, float z0) {
  float mx = 0.0f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float4 q = by_id[oid[k]];
    float dist = 0.0f, diff;
    diff = x0 - q.x; dist += diff * diff;
    diff = y0 - q.y; dist += diff * diff;
    diff = z0 - q.z; dist += diff * diff;
    mx = fmaxf(mx, dist);
  }
  return mx;
}

// kNN pass: one lane per query, writes the 5 neighbour map indices (slot 0 = -1: no correspondence).
// R = grid cells per side covering radius 1 (both map grids share one cell size).  kFused: the
// same lane goes on to its residual row and the workgroup reduces the item's normal-equation
// partial (k_gn_residual's work, without re-reading the query and its neighbour indices).
// LPQ > 1 (wide mode, launches with few queries: single scans, tiny batches; neither fused nor
// flat): a workgroup covers 256 / LPQ queries of an item with LPQ lanes each, so a query's search
// chain is LPQ times shorter; lane `sub` == 0 of each query writes the results.
// One virtual workgroup v (item v / LPQ, query group v % LPQ) of the kNN pass (k_gn_knn's body).
template <int R, int RX, bool kFused, bool kFlat, bool kSparse, int LPQ>
__device__ __forceinline__ void gn_knn_block(const GnArgs& a, int v, int use_prev, double (*red)[28], int2* rows) {
  constexpr int QPB = kResThreads / LPQ;  // queries per workgroup
  const int sub = (int)threadIdx.x % LPQ;
  const int it = v / LPQ;
  const int tid = (v % LPQ) * QPB + (int)threadIdx.x / LPQ;  // query slot within the item
  const int4 item = a.items[it];
  const int job = item.x;
  const GnState& g = a.gn[job];
  if (!g.active) return;  // block-uniform
  float row[6] = {0, 0, 0, 0, 0, 0}, b = 0.0f;
  bool rok = false;
  if (tid < item.w) {
    const bool corner = item.y == 0;
    const float4 p = corner ? a.cornerDS[job * a.capc + item.z + tid] : a.surfDS[job * a.caps + item.z + tid];
    const float4 t = associate(g.T, p);
    const float x0 = t.x, y0 = t.y, z0 = t.z;
    const MapGrid& mg = corner ? a.mc : a.ms;
    int32_t* o = a.nbr + (int64_t)it * 5 * kResThreads + tid;
    float bound = __int_as_float(0x7f800000);
    int32_t oid[5] = {-1, -1, -1, -1, -1};
    const bool have_prev = use_prev && o[0] >= 0;
    if (have_prev) {  // warm start: the previous iteration's neighbours of this query
#pragma unroll
      for (int k = 0; k < 5; ++k) oid[k] = o[k * kResThreads];
      bound = warm_bound(mg.by_id, oid, x0, y0, z0);
    }
    Knn5 nn;
    unsigned ks[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    knn5_grid<R, RX, kFlat, kSparse, LPQ>(mg, x0, y0, z0, g.crop_min, g.crop_max, bound, nn, ks, rows, sub);
    if constexpr (LPQ > 1) knn5_merge<LPQ>(nn);
    const bool ok = nn.k[4] < kKnnEmpty;
    (void)ks;
    int32_t ids[5];
    bool same = have_prev && ok && a.fit_cache;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      ids[k] = knn_id(nn.k[k]);
      same = same && ids[k] == oid[k];
    }
    if (LPQ > 1) __builtin_amdgcn_wave_barrier();  // every lane of the query read o[] (warm start)
    if (sub == 0)
#pragma unroll
      for (int k = 0; k < 5; ++k) o[k * kResThreads] = ok ? ids[k] : -1;
    const int64_t q = (int64_t)it * kResThreads + tid;
    if (!kFused && sub == 0) a.nsame[q] = same ? 1 : 0;
#ifdef FBR_KNN_STATS
    ks[5] = ok;
    ks[6] = corner;
    ks[8] = have_prev;
    ks[9] = same;
    for (int k = 0; k < 10; ++k) atomicAdd(&a.knn_stats[k], (unsigned long long)ks[k]);
    if (kFlat && use_prev) {
      atomicAdd(&a.knn_stats[10], 1ull);
      atomicAdd(&a.knn_stats[11], (unsigned long long)ks[10]);
      atomicAdd(&a.knn_stats[12 + (ks[10] < 32 ? ks[10] : ks[10] < 64 ? 32 : 33)], 1ull);
      atomicAdd(&a.knn_stats[46], (unsigned long long)ks[3]);
      atomicAdd(&a.knn_stats[47], (unsigned long long)ks[11]);
    }
#endif
    if (kFused && ok)
      rok = res_row(g, mg.by_id, ids, 1, corner, p, x0, y0, z0, row, b, a.fitc + (int64_t)it * 6 * kResThreads + tid,
                    a.fits + q, same);
  }
  if (kFused) res_reduce(red, tid, row, b, rok, a.partial + (int64_t)it * kPartial);
}

// kLoop = false: virtual workgroup base + blockIdx.x only (one_item launches, k_gn_knn); true: a
// grid-stride loop from base (k_gn_loop_knn: single scans, wide mode, the items past a one-item grid).
template <int R, int RX, bool kFused, bool kFlat, bool kSparse, int LPQ, bool kLoop>
__device__ __forceinline__ void gn_knn_kernel(const GnArgs& a, int use_prev, int base) {
  static_assert(LPQ == 1 || (!kFused && !kFlat), "wide mode is the plain kNN pass");
  __shared__ double red[kFused ? kResThreads / 64 : 1][28];
  __shared__ int2 rows[kFlat ? (2 * R + 1) * (2 * R + 1) : 1][kResThreads];
  const int nitems = a.nitems[0];
  if constexpr (kLoop) {
    for (int v = base + blockIdx.x; v < nitems * LPQ; v += gridDim.x)
      gn_knn_block<R, RX, kFused, kFlat, kSparse, LPQ>(a, v, use_prev, red, &rows[0][threadIdx.x]);
  } else {
    const int v = base + (int)blockIdx.x;
    if (v < nitems * LPQ) gn_knn_block<R, RX, kFused, kFlat, kSparse, LPQ>(a, v, use_prev, red, &rows[0][threadIdx.x]);
  }
}
template <int R, int RX, bool kFused, bool kFlat, bool kSparse, int LPQ = 1>
__global__ void __launch_bounds__(kResThreads) k_gn_knn(GnArgs a, int use_prev, int base) {
  gn_knn_kernel<R, RX, kFused, kFlat, kSparse, LPQ, false>(a, use_prev, base);
}
template <int R, int RX, bool kFused, bool kFlat, bool kSparse, int LPQ = 1>
__global__ void __launch_bounds__(kResThreads) k_gn_loop_knn(GnArgs a, int use_prev, int base) {
  gn_knn_kernel<R, RX, kFused, kFlat, kSparse, LPQ, true>(a, use_prev, base);
}

// Items past a one-item launch's grid: a loop launch of at most GnArgs::rest_grid (default 2048)
// workgroups from `grid` (they return at once when the grid covered every item; while other
// streams' kernels hold the CUs, even returning workgroups wait for slots, so the host keeps the
// loop launch small when it sized the grid from a previous run's count).
constexpr int kRestGrid = 2048;
template <typename Kmain, typename Krest, typename... Args>
void launch_one_item(hipStream_t s, const GnArgs& a, int grid, int total, size_t lds, Kmain kmain, Krest krest,
                     Args... args) {
  if (a.one_item == 1 && grid < total) {
    if (a.one_part != 2) fbr_launch(kmain, dim3(grid), dim3(kResThreads), lds, s, args..., 0);
    if (a.one_part != 1)
      fbr_launch(krest, dim3(std::min(a.rest_grid > 0 ? a.rest_grid : kRestGrid, total - grid)), dim3(kResThreads), lds,
                 s, args..., grid);
  } else if (a.one_part != 2) {
    fbr_launch(a.one_item ? kmain : krest, dim3(grid), dim3(kResThreads), lds, s, args..., 0);
  }
}

// pcl::getTransformation (x,y,z,roll,pitch,yaw) in float with glibc's sinf / cosf
// (fbr_sincosf.h: the FMA variant restated bit for bit).
__device__ void pose_to_T(const float* tr, float* T, float* trig) {
  const float roll = tr[0], pitch = tr[1], yaw = tr[2];
  const float A = gl_cosf(yaw), B = gl_sinf(yaw), C = gl_cosf(pitch), D = gl_sinf(pitch), E = gl_cosf(roll),
              F = gl_sinf(roll);
  const float DE = D * E, DF = D * F;
  T[0] = A * C; T[1] = A * DF - B * E; T[2] = B * F + A * DE; T[3] = tr[3];
  T[4] = B * C; T[5] = A * E + B * DF; T[6] = B * DE - A * F; T[7] = tr[4];
  T[8] = -D;    T[9] = C * F;          T[10] = C * E;         T[11] = tr[5];
  // LMOptimization (:1259-1264): srx, crx (pitch), sry, cry (yaw), srz, crz (roll)
  trig[0] = D; trig[1] = C; trig[2] = B; trig[3] = A; trig[4] = F; trig[5] = E;
}

// The residual rows of work item `it` and its normal-equation partial (k_gn_residual's body).
// (Round 6 measured packing an item's refits into the first waves -- list them in LDS, fit, barrier,
// apply: -15 % VALU instructions per dispatch but +6 % duration alone, the two extra barriers
// exposing the gathers' latency; profiles/r06b_residual_refit_compaction_ab.txt.)
__device__ __forceinline__ void gn_residual_item(const GnArgs& a, int it, double (*red)[28]) {
  const int tid = threadIdx.x;
  const int4 item = a.items[it];
  const int job = item.x;
  const GnState& g = a.gn[job];
  if (!g.active) return;  // block-uniform
  float row[6] = {0, 0, 0, 0, 0, 0}, b = 0.0f;
  bool ok = false;
  const int32_t* nb = a.nbr + (int64_t)it * 5 * kResThreads + tid;
  if (tid < item.w && nb[0] >= 0) {
    const bool corner = item.y == 0;
    const float4 p = corner ? a.cornerDS[job * a.capc + item.z + tid] : a.surfDS[job * a.caps + item.z + tid];
    const float4 t = associate(g.T, p);
    const int64_t q = (int64_t)it * kResThreads + tid;
    ok = res_row(g, corner ? a.mc.by_id : a.ms.by_id, nb, kResThreads, corner, p, t.x, t.y, t.z, row, b,
                 a.fitc + (int64_t)it * 6 * kResThreads + tid, a.fits + q, a.nsame[q] != 0);
  }
  res_reduce(red, tid, row, b, ok, a.partial + (int64_t)it * kPartial);
}

// The normal equations of one job in float, as LMOptimization forms them (matAtA / matAtB).
__device__ __forceinline__ void gn_normal_eq(const double* acc, float* AtA, float* X) {
  int q = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      AtA[r * 6 + c] = (float)acc[q];
      AtA[c * 6 + r] = (float)acc[q];
      ++q;
    }
  for (int r = 0; r < 6; ++r) X[r] = (float)acc[21 + r];
}

// Iteration-0 degeneracy projection (:1280-1305): 6x6 Jacobi, eigenvalues < 100 zero rows of V2,
// matP = V^-1 * V2 by LU.  It depends only on AtA, so the second wave of k_gn_solve computes it
// (the Jacobi rotations spread over its lanes, jacobi_eigen_wave) while the first solves
// AtA X = AtB.  All 64 lanes of the wave call it; matP / degenerate are written by lane 0.  A
// matrix whose eigenvalues are certified above 100 (eig_above_certified: an LDL^T test with a
// 1e-3 ||A|| margin, the common case) skips the Jacobi and the LU: degenerate = 0, and matP is
// then never read (gn_solve_job applies it only when degenerate).
struct EigenLds {
  float A[36], V[36], W[6];
  int R[6], C[6];
};
__device__ void gn_degeneracy(const double* acc, EigenLds& e, float* matP, int* degenerate) {
  const int lane = threadIdx.x & 63;
  if (lane < 36) {
    const int r = lane / 6, c = lane % 6, lo = r < c ? r : c, hi = r < c ? c : r;
    e.A[lane] = (float)acc[lo * 6 - lo * (lo - 1) / 2 + (hi - lo)];  // upper-triangle order
  }
  wave_lds_sync();
  if (eig_above_certified<6>(e.A, 100.0f)) {  // every eigenvalue >= 100: not degenerate, matP unused
    if (lane == 0) *degenerate = 0;
    return;
  }
  jacobi_eigen_wave<6>(e.A, e.W, e.V, e.R, e.C);
  if (lane != 0) return;
  float E[6], V[36], V2[36], Vi[36];
  for (int k = 0; k < 6; ++k) E[k] = e.W[k];
  for (int k = 0; k < 36; ++k) V[k] = e.V[k];
  for (int k = 0; k < 36; ++k) V2[k] = V[k];
  int deg = 0;
  for (int i = 5; i >= 0; i--) {
    if (E[i] < 100.0f) {
      for (int j = 0; j < 6; j++) V2[i * 6 + j] = 0.0f;
      deg = 1;
    } else {
      break;
    }
  }
  *degenerate = deg;
  if (!lu_inv6(V, Vi))
    for (int k = 0; k < 36; ++k) Vi[k] = 0.0f;
  float P[36];
  for (int k = 0; k < 36; ++k) P[k] = 0.0f;
  gemm_f32_acc64<6, 6, 6>(Vi, V2, P);
  for (int k = 0; k < 36; ++k) matP[k] = P[k];
}

// matAtA X = matAtB by OpenCV's float Householder QR (:1276); X = 0 if singular.
__device__ void gn_qr_step(const double* acc, float* X) {
  float AtA[36];
  gn_normal_eq(acc, AtA, X);
  if (!qr_solve6(AtA, X))
    for (int k = 0; k < 6; ++k) X[k] = 0.0f;
}

// One job's LMOptimization step on one lane (acc = the job's summed normal-equation products,
// X = gn_qr_step's solution, matP0 / deg0 = gn_degeneracy's result at iteration 0).
__device__ void gn_solve_job(const GnArgs& a, int job, const double* acc, float* X, const float* matP0, int deg0) {
  GnState& g = a.gn[job];
  const int iterCount = g.iter;
  g.iter = iterCount + 1;
  const int sel = (int)acc[27];
  g.n_sel = sel;
  if (a.knn_T) {  // diagnostic read-back: the transform and the trig this iteration's passes ran at
    for (int k = 0; k < 12; ++k) a.knn_T[job * 12 + k] = g.T[k];
    for (int k = 0; k < 6; ++k) a.knn_T[a.B * 12 + job * 6 + k] = g.trig[k];
  }
  if (a.trace) {
    // filled below after the update; pre-fill with the current pose for the early-return case
    for (int k = 0; k < 6; ++k) a.trace[((int64_t)job * a.max_iter + iterCount) * 6 + k] = g.pose[k];
  }
  if (sel < 50) {  // :1268 return false
    if (g.iter >= a.max_iter) g.active = 0;
    return;
  }
  // the local cv::Mat matP (:1278) is zero after iteration 0
  if (iterCount == 0) g.degenerate = deg0;
  if (g.degenerate) {
    float X2[6];
    for (int k = 0; k < 6; ++k) X2[k] = X[k];
    if (iterCount == 0) {
      float P[36];
      for (int k = 0; k < 36; ++k) P[k] = matP0[k];
      gemm_f32_acc64<6, 6, 1>(P, X2, X);
    } else {
      float P[36];
      for (int k = 0; k < 36; ++k) P[k] = 0.0f;
      gemm_f32_acc64<6, 6, 1>(P, X2, X);
    }
  }
  for (int k = 0; k < 6; ++k) g.pose[k] += X[k];
  if (a.trace)
    for (int k = 0; k < 6; ++k) a.trace[((int64_t)job * a.max_iter + iterCount) * 6 + k] = g.pose[k];
  const double r0 = (double)(X[0] * 57.29578f), r1 = (double)(X[1] * 57.29578f), r2 = (double)(X[2] * 57.29578f);
  const float deltaR = (float)sqrt(r0 * r0 + r1 * r1 + r2 * r2);
  const double t0 = (double)(X[3] * 100.0f), t1 = (double)(X[4] * 100.0f), t2 = (double)(X[5] * 100.0f);
  const float deltaT = (float)sqrt(t0 * t0 + t1 * t1 + t2 * t2);
  if ((double)deltaR < 0.05 && (double)deltaT < 0.05) {
    g.converged = 1;
    g.active = 0;
  } else if (g.iter >= a.max_iter) {
    g.active = 0;
  }
  pose_to_T(g.pose, g.T, g.trig);
}

// One job's LMOptimization step by the first two waves of a workgroup (k_gn_solve's body; extra
// waves only pass the barriers).
struct SolveLds {
  double acc[28];
  float matP0[36];
  int deg0;
  EigenLds eig;
};
__device__ __forceinline__ void gn_solve_block(const GnArgs& a, int job, SolveLds& s) {
  const int tid = threadIdx.x;
  GnState& g = a.gn[job];
  if (!g.active) return;  // block-uniform
  const int iter0 = g.iter == 0;  // read before lane 0 updates it (ordered by the barriers)
  if (tid < 28) {
    double sum = 0.0;
    const int i0 = a.item_range[2 * job], i1 = a.item_range[2 * job + 1];
#pragma unroll 8
    for (int it = i0; it < i1; ++it) sum += a.partial[(int64_t)it * kPartial + tid];
    s.acc[tid] = sum;
  }
  __syncthreads();
  float X[6];
  const bool solve = (int)s.acc[27] >= 50;
  if (tid >= 64 && tid < 128 && iter0 && solve) gn_degeneracy(s.acc, s.eig, s.matP0, &s.deg0);
  if (tid == 0 && solve) gn_qr_step(s.acc, X);
  __syncthreads();
  if (tid == 0) gn_solve_job(a, job, s.acc, X, s.matP0, s.deg0);
  __syncthreads();
}

// Host launchers of the kNN pass.  launch_gn_knn_r<R, F> is instantiated in k_knn_*.hip.
template <int R, bool F, bool L, bool S, int LPQ = 1>
void launch_gn_knn_rls(hipStream_t s, const GnArgs& a, int grid, int use_prev) {
  const float invx = a.mc.g.inv_x;  // == a.ms.g.inv_x
  grid *= LPQ;
  const int total = a.max_items * LPQ;
  // one-item launches at one lane per query (wide mode loops)
  constexpr bool kOne = LPQ == 1;
  auto go = [&](auto rx) {
    constexpr int RX = decltype(rx)::value;
    knn_launch_desc() = KnnLaunchDesc{R, RX, L ? 1 : 0, S ? 1 : 0, LPQ, F ? 1 : 0, 0};
    if constexpr (kOne)
      launch_one_item(s, a, grid, total, 0, k_gn_knn<R, RX, F, L, S, LPQ>, k_gn_loop_knn<R, RX, F, L, S, LPQ>, a,
                      use_prev);
    else if (a.one_part != 2)
      fbr_launch((k_gn_loop_knn<R, RX, F, L, S, LPQ>), dim3(grid), dim3(kResThreads), 0, s, a, use_prev, 0);
  };
  if (invx > 4.0f) go(std::integral_constant<int, 8>{});       // 0.125 m
  else if (invx > 2.0f) go(std::integral_constant<int, 4>{});  // 0.25 m
  else if (invx > 1.0f) go(std::integral_constant<int, 2>{});  // 0.5 m
  else go(std::integral_constant<int, 1>{});                  // >= 1 m
}
// Dense or hashed-chunk map grids (one flag for both maps: fbr_set_map builds them alike).
template <int R, bool F, bool L, int LPQ = 1>
void launch_gn_knn_rl(hipStream_t s, const GnArgs& a, int grid, int use_prev) {
  if (a.mc.g.sparse || a.ms.g.sparse) launch_gn_knn_rls<R, F, L, true, LPQ>(s, a, grid, use_prev);
  else launch_gn_knn_rls<R, F, L, false, LPQ>(s, a, grid, use_prev);
}

// Lanes per query of the plain kNN pass (FBR_KNN_LPQ = 1 or 8; default 8 for sub-batches of at
// most 2 jobs, where one lane per query leaves the chip idle and the launch is one query's chain).
inline int knn_lpq(int jobs) {
  if (const int forced = knobs::knn_lpq()) return forced;
  return jobs <= 2 ? 8 : 1;
}

template <int R, bool F>
void launch_gn_knn_r(hipStream_t s, const GnArgs& a, int grid, int use_prev) {
  if constexpr (!F) {
    if (knn_lpq(a.B) == 8) return launch_gn_knn_rl<R, F, false, 8>(s, a, grid, use_prev);
  }
  // flat queue for the 1 m cells from iteration 1 (round 4 measured it slower in iteration 0, with
  // no warm-start bound, and for the 0.5 m cells, whose 25-row queue costs occupancy)
  if constexpr (R == 1 && !F) {
    if (use_prev && knobs::knn_flat()) return launch_gn_knn_rl<R, F, true>(s, a, grid, use_prev);
  }
  launch_gn_knn_rl<R, F, false>(s, a, grid, use_prev);
}

}  // namespace fbr
