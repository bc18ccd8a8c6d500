// fbr_grid_search.h — the neighbour search over a MapGrid (k_grid.hip) in one place: the key
// format and the 5-NN list, the crop-box test, the grid geometry and its float lower bounds, the
// row-inside-box test, the per-point key, and the two walks: knn5_grid (the Gauss-Newton 5-NN,
// fbr_gn.h / k_knn_*.hip / k_knn_tile.hip) and nn1_grid (the gated nearest point, k_score.hip).
// Both walks start with the same query prologue (the cell of q, the exactness guard, the window
// test, the near-side signs, xin) and prune a row's x extent the same way; a change to either is a
// change to both.  They differ where the result depends on it: the 5-NN's cut is
// min(k[4], bound, kBelowOne), the 1-NN's is strict on its best d2 and on the gate, so that among
// equal distances the lowest map index wins in both.
// See k_register.hip for the design notes and the reference citations.
#pragma once
#include "fbr_common.h"
#include "fbr_kernels.h"

namespace fbr {

// The 5 nearest as sorted 64-bit keys (float bits of d2) << 32 | map index: d2 >= +0, so the
// unsigned key order is exactly FLANN's (d2, index) order.  A key is built from a scanned point
// without any instruction (hi = the distance register, lo = the w bit pattern).  Empty slots hold
// kKnnEmpty = (bits(1.0f), 0): a point is only inserted with d2 < 1.0 (:1027, :1154).
constexpr unsigned long long kKnnEmpty = (unsigned long long)0x3f800000u << 32;
constexpr float kBelowOne = 0.99999994f;  // nextafterf(1.0f, 0.0f)

struct Knn5 {
  unsigned long long k[5];
};

__device__ __forceinline__ float knn_d(unsigned long long k) { return __int_as_float((int)(k >> 32)); }
__device__ __forceinline__ int knn_id(unsigned long long k) { return (int)(unsigned)k; }

// The sorted insertion of a key into the 5-NN list as v_min_f64 / v_max_f64 over the keys read as
// doubles: a key's high word is the
// bits of a float d2 >= +0 (at most +inf = 0x7f800000 for a point outside the crop box), so every
// key is a non-negative finite double (a subnormal when d2 = 0; the kernels keep f64 denormals,
// amdhsa_float_denorm_mode_16_64 3) and double order is the key's unsigned order.  9 v_min_f64 /
// v_max_f64 instead of 5 64-bit compares, 20 selects and the wait states between them.  Written as
// inline asm: the compiler's fmin / fmax quiet-NaN canonicalisation of the loop-carried keys would
// add a v_max_f64 per slot.
// The slots do not chain: with k sorted, the new k[t] is min(k[t], max(k[t-1], x)) (x below k[t-1]
// shifts k[t-1] up, else x or k[t] stays), so every slot is two operations deep, visited from the top
// so each max reads the old k[t-1].
__device__ __forceinline__ void knn_insert_f64(Knn5& r, unsigned long long xk) {
  const double x = __longlong_as_double((long long)xk);
  double k[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) k[t] = __longlong_as_double((long long)r.k[t]);
#pragma unroll
  for (int t = 4; t > 0; --t) {
    double m;
    asm("v_max_f64 %0, %1, %2" : "=v"(m) : "v"(k[t - 1]), "v"(x));
    asm("v_min_f64 %0, %0, %1" : "+v"(k[t]) : "v"(m));
  }
  asm("v_min_f64 %0, %0, %1" : "+v"(k[0]) : "v"(x));
#pragma unroll
  for (int t = 0; t < 5; ++t) r.k[t] = (unsigned long long)__double_as_longlong(k[t]);
}
// Branch-free sorted insertion with selects: the "less than slot t" flags are monotone over t, so
// every slot takes its own key, its left neighbour's, or the new one (5 compares + 20 selects).
__device__ __forceinline__ void knn_insert_sel(Knn5& r, unsigned long long x) {
  bool lt[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) lt[t] = x < r.k[t];
#pragma unroll
  for (int t = 4; t > 0; --t) r.k[t] = lt[t - 1] ? r.k[t - 1] : (lt[t] ? x : r.k[t]);  // lt[t-1] implies lt[t]
  r.k[0] = lt[0] ? x : r.k[0];
}
// Which form a kernel uses (round 5, profiles/r05aj_*, r05ak_knn_f64_insert_ab.txt): the f64 form
// for the 1 m (C2) and 0.25 m cells, where it took gn_knn 2.29 -> 2.00 ms per B = 1024 step
// (flat dispatch VALU 1.745e8 -> 1.342e8) and C2 109.5k -> 112-113k scans/s; the selects for the
// 0.5 m cells (C3, C5), whose per-row kernel at 85 -> 90 VGPRs lost 2.5 % on C3 with the f64 form
// (C5 gained 1.5 %).  FBR_KNN_F64_R2=1 builds the f64 form there too.
#ifndef FBR_KNN_F64_R2
#define FBR_KNN_F64_R2 0
#endif
template <int R>
__device__ __forceinline__ void knn_insert(Knn5& r, unsigned long long x) {
  if constexpr (R != 2 || FBR_KNN_F64_R2) knn_insert_f64(r, x);
  else knn_insert_sel(r, x);
}

// Wide mode: the LPQ lanes of a query (consecutive lanes) exchange their lists in a butterfly and
// each keeps the 5 smallest keys of the union (the lanes scanned disjoint point sets, so keys are
// distinct and the result is the 5 nearest of the whole scanned set).
template <int LPQ>
__device__ __forceinline__ void knn5_merge(Knn5& r) {
#pragma unroll
  for (int off = 1; off < LPQ; off <<= 1) {
    unsigned long long o[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const unsigned lo = __shfl_xor((unsigned)r.k[t], off), hi = __shfl_xor((unsigned)(r.k[t] >> 32), off);
      o[t] = ((unsigned long long)hi << 32) | lo;
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) knn_insert_f64(r, o[t]);
  }
}

// pcl::CropBox's inclusive test (p outside [bmin, bmax] on some axis) as one compare: for finite
// floats b - x > 0 exactly when x < b (the difference of distinct floats is never rounded to 0,
// denormals are kept), so "outside" is the largest of the six excesses being positive; 6 subtractions
// and 2 three-way maxima instead of 6 compares whose masks the compiler combined in 16-bit registers.
struct CropBox {
  float x0, y0, z0, x1, y1, z1;
};
__device__ __forceinline__ bool crop_out(const float4& p, const CropBox& b) {
  const float ex = fmaxf(fmaxf(b.x0 - p.x, p.x - b.x1), fmaxf(b.y0 - p.y, p.y - b.y1));
  return fmaxf(ex, fmaxf(b.z0 - p.z, p.z - b.z1)) > 0.0f;
}

// Lower bound of |q - p| along one axis for a point p in the cell at offset o from q's cell
// (cells are [k*c, (k+1)*c) with c a power of two, so every edge is exact).  Rounding is
// monotone, so fl(edge - q) <= |fl(q - p)| and the bound composed in the distance's own
// operation order never exceeds the distance computed for any point of that cell.
__device__ __forceinline__ float axis_lb(float q, float fcell, int o, float c) {
  if (o == 0) return 0.0f;
  if (o > 0) return (fcell + (float)o) * c - q;
  return q - (fcell + (float)(o + 1)) * c;
}

__device__ __forceinline__ int rank_offset(int k, int s) { return k == 0 ? 0 : ((k & 1) ? s * ((k + 1) >> 1) : -s * (k >> 1)); }

// Sparse grids (k_grid.hip): the chunk of (z, y, x / kChunkX), or -1.  The table is at most half
// full, so a free slot ends every probe sequence.
__device__ __forceinline__ int chunk_find(const MapGrid& m, int z, int y, int xc) {
  const unsigned long long key = chunk_key(z, y, xc);
  uint32_t h = chunk_hash(key) & m.g.hmask;
  for (uint32_t probe = 0; probe <= m.g.hmask; ++probe) {
    const unsigned long long k = m.hkeys[h];
    if (k == key) return m.hvals[h];
    if (k == kChunkEmpty) break;
    h = (h + 1) & m.g.hmask;
  }
  return -1;
}

// Point range [b, e) of the cells x0..x1 (x1 - x0 < 2 * kChunkX) of row (y, z).  The two chunks
// are adjacent in the (z, y, x) sort, so their points form one contiguous range.
template <bool kSparse>
__device__ __forceinline__ bool row_range(const MapGrid& m, int y, int z, int x0, int x1, int& b, int& e) {
  if constexpr (!kSparse) {
    const int rowbase = (z * m.g.dims[1] + y) * m.g.dims[0];
    b = m.cell_start[rowbase + x0];
    e = m.cell_start[rowbase + x1 + 1];
    return true;
  } else {
    const int ca = x0 / kChunkX, cb = x1 / kChunkX;
    const int ia = chunk_find(m, z, y, ca);
    const int ib = cb == ca ? ia : chunk_find(m, z, y, cb);
    if (ia < 0 && ib < 0) return false;
    constexpr int S = kChunkX + 1;
    b = ia >= 0 ? m.cell_start[ia * S + (x0 - ca * kChunkX)] : m.cell_start[ib * S];
    e = ib >= 0 ? m.cell_start[ib * S + (x1 - cb * kChunkX) + 1] : m.cell_start[ia * S + kChunkX];
    return true;
  }
}

#ifdef FBR_KNN_STATS
// Diagnostic builds only (tools/knn_stats.py): [queries, rows considered, rows scanned, points
// scanned, points inserted, accepted queries, corner queries, wave iterations of the point loop,
// warm-started queries, queries whose neighbours equal the previous iteration's], accumulated into
// GnArgs::knn_stats (one device buffer for every kNN translation unit); then, for the flat walk,
// [flat queries, points within the static cut], a histogram of that count per flat query (bins
// 0..31, 32..63, >= 64) at [12, 46), [points scanned, wave trips] at [46, 48)
#define FBR_KS(i, v) ks[i] += (v)
#else
#define FBR_KS(i, v) \
  do {               \
  } while (0)
#endif

// ---- the pieces both walks are built from ----
// Only those whose use leaves every kernel's machine code as it was when the walk spelt them out
// (profiles/grid_search_refactor.md); the query prologue and the x-extent pruning of a row are
// therefore written in each walk.

// The whole row of cells at offset (oy, oz) from q's cell (fy, fz; cells of size c) inside the crop
// box (pcl::CropBox, inclusive): no per-point test.  xin: the row's x extent is inside.
__device__ __forceinline__ bool row_inside(float fy, float fz, float c, const CropBox& box, bool xin, int oy, int oz) {
  const float ylo = (fy + (float)oy) * c, zlo = (fz + (float)oz) * c;
  return xin & (ylo >= box.y0) & (ylo + c <= box.y1) & (zlo >= box.z0) & (zlo + c <= box.z1);
}

// The key of map point p for query q: d2 in flann::L2_Simple order, and pcl::CropBox (inclusive) as
// one mask: a point outside gets d2 = +inf (never inserted); `inside` (the row or tile lies inside
// the box) skips the test.  The distance unconditionally, the box test only where needed: the
// compiler otherwise sinks the distance under a branch on the test's result.
__device__ __forceinline__ unsigned long long point_key(float qx, float qy, float qz, const float4& p, bool inside,
                                                        const CropBox& box) {
  float dist = 0.0f, diff;
  diff = qx - p.x; dist += diff * diff;  // flann::L2_Simple
  diff = qy - p.y; dist += diff * diff;
  diff = qz - p.z; dist += diff * diff;
  unsigned hi = (unsigned)__float_as_int(dist);
  if (!inside && crop_out(p, box)) hi = 0x7f800000u;
  return ((unsigned long long)hi << 32) | (unsigned)__float_as_int(p.w);
}

// ---- the 5-NN walk ----

constexpr int kResThreads = 256;  // lanes of a Gauss-Newton workgroup = queries of a work item; the stride of the
                                  // flat walk's LDS queue

// Exact kNN-5 among map points inside the crop box with d2 < 1.0, ordered by (d2, map index):
// the neighbour set FLANN's exact search returns on the cropped cloud whenever the reference
// keeps the correspondence (pointSearchSqDis[4] < 1.0, :1027/:1154).  R = cells per side covering
// radius 1 (compile time: the row loop is fully unrolled).  Cell rows (y,z) are visited in
// near-side-first rank order; a row, and the cells of a row, are skipped once their lower-bound
// distance exceeds the current 5th distance or reaches 1.0.  Rows entirely inside the crop box
// skip the per-point box test.
// `bound` is an upper bound of the 5th-neighbour distance known before the search (the largest
// distance to the previous iteration's 5 neighbours, 5 distinct candidates of the same crop box):
// cells whose lower bound exceeds it cannot hold any of the 5 nearest, ties included, so they are
// pruned from the start instead of only once 5 points have been inserted.
// kFlat: the rows are pruned once up front with `bound` (the warm start, tight from iteration 1
// on) and their point ranges queued in LDS (`rows`, stride kResThreads); one loop then walks a
// lane's queued points across rows.  A wave then runs for its longest lane's total instead of the
// sum over rows of each row's longest lane (lanes of a wave scan different rows: the per-row loop
// kept ~30 % of the lanes busy).  Pruning with a larger cut only scans more cells, and the 5-NN
// list is a function of the scanned set, so both forms give the same neighbours.
// LPQ > 1 (wide mode, small launches): LPQ lanes share a query and lane `sub` scans the points of
// absolute map index = sub (mod LPQ) (knn5_merge combines the lists).  A lane prunes with its own
// 5th distance, which is never below the merged one (its list holds the 5 nearest of a subset),
// so every point of the merged 5 nearest is still scanned by its lane.
template <int R, int RX, bool kFlat = false, bool kSparse = false, int LPQ = 1>
__device__ void knn5_grid(const MapGrid& m, float qx, float qy, float qz, const float* bmin, const float* bmax,
                          float bound, Knn5& r, unsigned* ks, int2* rows = nullptr, int sub = 0) {
  constexpr int K = 2 * R + 1;  // rows per side in y and z; RX = cells per side along x
#pragma unroll
  for (int t = 0; t < 5; ++t) r.k[t] = kKnnEmpty;
  const float inv = m.g.inv_cell, c = 1.0f / inv, invx = m.g.inv_x, cxs = 1.0f / invx;
  const float sx = qx * invx, sy = qy * inv, sz = qz * inv;
  const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
  // a non-finite q fails here too; cell indices beyond 1e7 are not exact in float, and such a query
  // is further than 1 m from every cell of the grid
  if (!(fabsf(fx) < 1e7f && fabsf(fy) < 1e7f && fabsf(fz) < 1e7f)) return;
  const int cx = (int)fx - (int)m.g.origin[0], cy = (int)fy - (int)m.g.origin[1], cz = (int)fz - (int)m.g.origin[2];
  const int X = m.g.dims[0], Y = m.g.dims[1], Z = m.g.dims[2];
  if (cx < -RX || cy < -R || cz < -R || cx >= X + RX || cy >= Y + R || cz >= Z + R) return;
  const int sgy = (sy - fy) >= 0.5f ? 1 : -1, sgz = (sz - fz) >= 0.5f ? 1 : -1;
  // squared per-axis lower bounds: y/z by visit rank, x by offset (negative / positive side)
  float ly2[K], lz2[K], lxm2[RX + 1], lxp2[RX + 1];
  int oyk[K], ozk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    // flat queue: rows in one fixed order for every lane (the queued set does not depend on it), so
    // lanes of a wave that share rows walk them in step
    oyk[k] = kFlat ? k - R : rank_offset(k, sgy);
    ozk[k] = kFlat ? k - R : rank_offset(k, sgz);
    const float ly = axis_lb(qy, fy, oyk[k], c), lz = axis_lb(qz, fz, ozk[k], c);
    ly2[k] = ly * ly;
    lz2[k] = lz * lz;
  }
#pragma unroll
  for (int o = 1; o <= RX; ++o) {
    const float a = axis_lb(qx, fx, -o, cxs), b = axis_lb(qx, fx, o, cxs);
    lxm2[o] = a * a;
    lxp2[o] = b * b;
  }
  // the crop box in registers (per job: wave-uniform)
  const CropBox box{bmin[0], bmin[1], bmin[2], bmax[0], bmax[1], bmax[2]};
  const float xlo = (fx - (float)RX) * cxs, xhi = (fx + (float)(RX + 1)) * cxs;  // row x extent (max)
  const bool xin = xlo >= box.x0 && xhi <= box.x1;
  int nrow = 0;  // kFlat: rows queued
  int total = 0;  // kFlat: points queued
#pragma unroll
  for (int ksum = 0; ksum <= 2 * (K - 1); ++ksum) {
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int kz = ksum - ky;
      if (kz < 0 || kz >= K) continue;  // compile time
      const int y = cy + oyk[ky], z = cz + ozk[kz];
      FBR_KS(1, 1);
      float lb = 0.0f;
      lb += ly2[ky];
      lb += lz2[kz];
      // "lb <= cut and lb < 1.0" as one compare: the largest float below 1.0 caps the cut
      const float cut = fminf(fminf(knn_d(r.k[4]), bound), kBelowOne);
      if (y < 0 || y >= Y || z < 0 || z >= Z || lb > cut) continue;
      int xa = 0, xb = 0;
      bool go_a = true, go_b = true;
#pragma unroll
      for (int o = 1; o <= RX; ++o) {
        float ta = 0.0f, tb = 0.0f;
        ta += lxm2[o]; ta += ly2[ky]; ta += lz2[kz];
        tb += lxp2[o]; tb += ly2[ky]; tb += lz2[kz];
        go_a = go_a && !(ta > cut);
        go_b = go_b && !(tb > cut);
        if (go_a) xa = -o;
        if (go_b) xb = o;
      }
      const int x0 = max(cx + xa, 0), x1 = min(cx + xb, X - 1);
      if (x0 > x1) continue;
      int b, e;
      if (!row_range<kSparse>(m, y, z, x0, x1, b, e)) continue;
      FBR_KS(2, 1);
      FBR_KS(3, e - b);
      const bool inside = row_inside(fy, fz, c, box, xin, oyk[ky], ozk[kz]);
      if constexpr (kFlat) {
        if (e > b) rows[nrow++ * kResThreads] = make_int2(b, inside ? (int)((unsigned)e | 0x80000000u) : e);
        total += e - b;
        continue;
      }
      // one point load in flight within the row (the row's last point re-requests itself)
      const int i0 = LPQ == 1 ? b : b + ((sub - b) & (LPQ - 1));
      float4 p = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(m.pts) + (uint32_t)(i0 < e ? i0 : b) * 16u);
      for (int i = i0; i < e; i += LPQ) {
        const int nx = i + LPQ < e ? i + LPQ : i;
        const float4 pn = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(m.pts) + (uint32_t)nx * 16u);
        const unsigned long long key = point_key(qx, qy, qz, p, inside, box);
        FBR_KS(4, knn_d(key) < knn_d(r.k[4]) ? 1 : 0);
#ifdef FBR_KNN_STATS
        if (__lane_id() == __ffsll((long long)__ballot(1)) - 1) ks[7] += 1;  // one per wave iteration
#endif
        knn_insert<R>(r, key);
        p = pn;
      }
    }
  }
  if constexpr (kFlat) {
    // counted walk: one trip per queued point (the lane's total), the row advance a short branch
    // (a while loop that tests for the next row first: +16 % per dispatch, r04ae).  The row offset
    // is a 32-bit byte offset (maps below 2^28 points): the load takes the SGPR base + VGPR offset
    // form, one shift instead of a 64-bit address per point.
    int2 q = rows[0];  // unread when nothing is queued
    int j = 0, i = q.x, e = q.y & 0x7fffffff;
    bool inside = q.y < 0;
    // one point load in flight: trip t + 1's point is requested before trip t's is tested (the
    // last trip re-requests its own point, so no index runs past a row)
    auto ld = [&](int k) __attribute__((always_inline)) {
      return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(m.pts) + (uint32_t)k * 16u);
    };
    float4 p = ld(total > 0 ? i : 0);
    for (int t = 0; t < total; ++t) {
      const bool in_cur = inside;
      const int cur = i;
      if (++i == e && t + 1 < total) {  // next queued row (every queued row is non-empty)
        q = rows[++j * kResThreads];
        i = q.x;
        e = q.y & 0x7fffffff;
        inside = q.y < 0;
      }
      const float4 pn = ld(t + 1 < total ? i : cur);
      const unsigned long long key = point_key(qx, qy, qz, p, in_cur, box);
      FBR_KS(4, knn_d(key) < knn_d(r.k[4]) ? 1 : 0);
      FBR_KS(10, knn_d(key) <= fminf(bound, kBelowOne) ? 1 : 0);  // within the static cut
#ifdef FBR_KNN_STATS
      if (__lane_id() == __ffsll((long long)__ballot(1)) - 1) {
        ks[7] += 1;  // one per wave iteration
        ks[11] += 1;
      }
#endif
      knn_insert<R>(r, key);
      p = pn;
    }
  }
}

// ---- the gated 1-NN walk ----

constexpr unsigned long long kNnNone = ~0ull;

// The nearest map point of q with d2 < g2 among the points inside the crop box `box` (min, max;
// crop = false: among all of them) as the key (d2 bits << 32) | map index, or kNnNone.  R / RX:
// cells covering 1 m along y, z / along x (g2 <= 1).  It prunes strictly: a cell whose bound
// equals the best d2 so far is still scanned, so among equal distances the lowest map index wins,
// as the 64-bit minimum says.  The cells are visited near side first along z, then y: the bounds
// do not decrease along a rank, so the first one past the cut ends its loop.  Unlike the 5-NN
// search the row window is a run-time loop (R, RX are arguments, not template parameters): one
// key is carried instead of five, nothing is unrolled into registers.
template <bool kSparse>
__device__ __forceinline__ unsigned long long nn1_grid(const MapGrid& m, int R, int RX, float qx, float qy, float qz,
                                                       float g2, bool crop, const float* box) {
  if (m.g.n_points <= 0) return kNnNone;
  const float inv = m.g.inv_cell, c = 1.0f / inv, invx = m.g.inv_x, cxs = 1.0f / invx;
  const float sx = qx * invx, sy = qy * inv, sz = qz * inv;
  const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
  if (!(fabsf(fx) < 1e7f && fabsf(fy) < 1e7f && fabsf(fz) < 1e7f)) return kNnNone;  // as in knn5_grid
  const int cx = (int)fx - (int)m.g.origin[0], cy = (int)fy - (int)m.g.origin[1], cz = (int)fz - (int)m.g.origin[2];
  const int X = m.g.dims[0], Y = m.g.dims[1], Z = m.g.dims[2];
  if (cx < -RX || cy < -R || cz < -R || cx >= X + RX || cy >= Y + R || cz >= Z + R) return kNnNone;
  const int sgy = (sy - fy) >= 0.5f ? 1 : -1, sgz = (sz - fz) >= 0.5f ? 1 : -1;
  const CropBox bx{box[0], box[1], box[2], box[3], box[4], box[5]};
  const float xlo = (fx - (float)RX) * cxs, xhi = (fx + (float)(RX + 1)) * cxs;  // a row's x extent at most
  const bool xin = xlo >= bx.x0 && xhi <= bx.x1;
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
      const bool inside = !crop || row_inside(fy, fz, c, bx, xin, oy, oz);
      for (int i = b; i < e; ++i) {
        const float4 p = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(m.pts) + (uint32_t)i * 16u);
        // point_key's body spelt out: through the helper this kernel's instructions come out in
        // another order, measured 0.8 to 1.7 % slower (profiles/grid_search_refactor.md)
        float dist = 0.0f, diff;
        diff = qx - p.x; dist += diff * diff;  // flann::L2_Simple
        diff = qy - p.y; dist += diff * diff;
        diff = qz - p.z; dist += diff * diff;
        unsigned hi = (unsigned)__float_as_int(dist);
        if (!inside && crop_out(p, bx)) hi = 0x7f800000u;
        const unsigned long long key = ((unsigned long long)hi << 32) | (unsigned)__float_as_int(p.w);
        best = key < best ? key : best;
      }
      bestd = knn_d(best);
    }
  }
  return best < empty ? best : kNnNone;
}

}  // namespace fbr
