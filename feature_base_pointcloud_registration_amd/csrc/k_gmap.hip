// k_gmap.hip — the wide VoxelGrid: PCL's grid with 64-bit keys, for clouds whose cell count exceeds
// PCL's INT32_MAX limit (a whole-trajectory map; see fbr_gmap.h for the arithmetic and its limits).
//
// The input is a concatenation that is never written out: a table of KfSeg entries over a point
// pool (the keyframe store), each copied to its offset and, with xform, transformed by its key
// pose in registers, in k_kf_transform's operation order.  A host cloud is one untransformed entry.
//
//   k_gmw_bounds  getMinMax3D of the transformed points (ordered-uint atomic min / max: the result
//                 does not depend on the order) and the count of points with a non-finite
//                 coordinate; the host builds the grid from the six bounds (gmap_grid_init)
//   k_gmw_keys    (key, concatenation index) per point; a non-finite point gets the drop key
//   vg_sorted_runs (fbr_vg_runs.h): the stable sort over the bits the grid needs (a voxel's points
//                 stay in index order) and the voxel index of every run of equal keys
//   k_gmw_emit    one centroid per run, its points re-transformed from the pool and summed in index
//                 order: vg_run_centroid, the arithmetic of k_voxel_large.hip's emit
// HBM-bound: the pool is read twice in stream order (16 B per point) and once gathered by the
// emit; keys and indices cost 12 B per point written, sorted and read.  No float atomics: two calls
// return the same bytes.
#include "fbr_gmap.h"
#include "fbr_vg_runs.h"

namespace fbr {

namespace {

// Point i of entry g of the concatenation.
__device__ __forceinline__ float4 gm_point(const float4* __restrict__ pool, const KfSeg& g, int xform, int64_t i) {
  const float4 p = pool[g.src + i];
  if (!xform) return p;
  float4 q;
  gmap_transform(g.T, p.x, p.y, p.z, &q.x, &q.y, &q.z);
  q.w = p.w;
  return q;
}
__device__ __forceinline__ bool gm_finite(const float4& p) { return gmap_finite(p.x) && gmap_finite(p.y) && gmap_finite(p.z); }

struct GmwBounds {
  uint32_t mm[6];                // ordered-uint min x, y, z, max x, y, z
  unsigned long long n_dropped;  // points with a non-finite coordinate
};

// grid (x: chunks of an entry, y: entries)
__global__ void __launch_bounds__(256) k_gmw_bounds(const float4* __restrict__ pool, const KfSeg* __restrict__ segs, int nseg, int xform, GmwBounds* B) {
  const int s = blockIdx.y;
  if (s >= nseg) return;
  const KfSeg g = segs[s];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  unsigned dropped = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.count; i += (int64_t)gridDim.x * 256) {
    const float4 p = gm_point(pool, g, xform, i);
    if (!gm_finite(p)) {
      ++dropped;
      continue;
    }
    const float v[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int d = 0; d < 3; ++d) {  // getMinMax3D's comparisons
      mn[d] = (v[d] < mn[d]) ? v[d] : mn[d];
      mx[d] = (mx[d] < v[d]) ? v[d] : mx[d];
    }
  }
  for (int o = 32; o > 0; o >>= 1) dropped += __shfl_xor(dropped, o);
  vg_merge_bounds(mn, mx, B->mm);
  if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&B->n_dropped, (unsigned long long)dropped);
}

__global__ void __launch_bounds__(256) k_gmw_keys(const float4* __restrict__ pool, const KfSeg* __restrict__ segs, int nseg, int xform, GmapGrid G,
                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int s = blockIdx.y;
  if (s >= nseg) return;
  const KfSeg g = segs[s];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.count; i += (int64_t)gridDim.x * 256) {
    const float4 p = gm_point(pool, g, xform, i);
    keys[g.dst + i] = gm_finite(p) ? gmap_key(G, p.x, p.y, p.z) : gmap_drop_key(G);
    vals[g.dst + i] = (uint32_t)(g.dst + i);
  }
}

// The entry that holds concatenation index idx: the last one with dst <= idx (entries are in
// ascending dst order and none is empty).  cur is the caller's previous entry, tried first.
__device__ __forceinline__ int gm_find_seg(const KfSeg* __restrict__ segs, int nseg, int64_t idx, int cur) {
  if (idx >= segs[cur].dst && idx < segs[cur].dst + segs[cur].count) return cur;
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].dst <= idx) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(256)
k_gmw_emit(const float4* __restrict__ pool, const KfSeg* __restrict__ segs, int nseg, int xform, int64_t n, uint64_t drop_key,
           const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ vox,
           float4* __restrict__ out, int64_t n_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (!vg_run_head(keys, i)) continue;
    if (keys[i] == drop_key) continue;  // the run of dropped points (the last one)
    const int64_t o = (int64_t)vox[i];
    if (o >= n_out) continue;  // cannot happen: the output holds every voxel before the dropped run
    int sg = 0;  // the entry of the run's previous point
    int64_t end;
    out[o] = vg_run_centroid(keys, n, i, [&](int64_t j) {
      sg = gm_find_seg(segs, nseg, (int64_t)vals[j], sg);
      return gm_point(pool, segs[sg], xform, (int64_t)vals[j] - segs[sg].dst);
    }, &end);
  }
}

// Entries in ascending dst order, none empty, every [src, src + count) inside the pool is the
// caller's contract; the launches cover nseg in slices of the grid's y limit.
template <typename K, typename... A>
void gm_launch_segs(K kernel, hipStream_t s, const GmapSrc& src, A... args) {
  const int per = (int)std::max<int64_t>(8, 4096 / std::max(src.nseg, 1));
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((src.max_count + 255) / 256, per));
  for (int s0 = 0; s0 < src.nseg; s0 += 65535) {
    const int k = std::min(65535, src.nseg - s0);
    fbr_launch(kernel, dim3(gx, k), dim3(256), 0, s, src.pool, src.segs + s0, k, src.xform, args...);
  }
}

__global__ void __launch_bounds__(256) k_gmw_finite(const float4* __restrict__ in, int64_t n, uint32_t* __restrict__ keep) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    keep[i] = gm_finite(in[i]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_gmw_compact(const float4* __restrict__ in, int64_t n, const uint32_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ pos, float4* __restrict__ out, int64_t n_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (keep[i] && (int64_t)pos[i] < n_out) out[pos[i]] = in[i];
}

}  // namespace

int gmap_compact_finite(hipStream_t s, DevArena& ar, const float4* in, int64_t n, float4* out, int64_t n_out) {
  if (n <= 0) return FBR_OK;
  if (n > (int64_t)INT32_MAX) return FBR_ERR_CAPACITY;
  const size_t N = (size_t)n;
  size_t tb = 0;
  uint32_t* null32 = nullptr;
  if (rocprim::exclusive_scan(nullptr, tb, null32, null32, 0u, N, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return FBR_ERR_HIP;
  tb = std::max<size_t>(tb, 16);
  if (arena_reserve(ar, 2 * arena_bytes(4 * N) + arena_bytes(tb), s) != hipSuccess) return FBR_ERR_HIP;
  uint32_t* keep = arena_take<uint32_t>(ar, 4 * N);
  uint32_t* pos = arena_take<uint32_t>(ar, 4 * N);
  void* tmp = arena_take<void>(ar, tb);
  if (!keep || !pos || !tmp) return FBR_ERR_HIP;
  const int grid = vg_pass_grid(n);
  fbr_launch(k_gmw_finite, dim3(grid), dim3(256), 0, s, in, n, keep);
  if (rocprim::exclusive_scan(tmp, tb, keep, pos, 0u, N, rocprim::plus<uint32_t>(), s) != hipSuccess) return FBR_ERR_HIP;
  fbr_launch(k_gmw_compact, dim3(grid), dim3(256), 0, s, in, n, (const uint32_t*)keep, (const uint32_t*)pos, out, n_out);
  return hipGetLastError() == hipSuccess ? FBR_OK : FBR_ERR_HIP;
}

int gmap_bounds(hipStream_t s, DevArena& ar, const GmapSrc& src, float leaf, GmapInfo* info) {
  *info = GmapInfo{};
  if (src.n <= 0 || src.nseg <= 0) return FBR_OK;
  if (arena_reserve(ar, arena_bytes(sizeof(GmwBounds)), s) != hipSuccess) return FBR_ERR_HIP;
  GmwBounds* d_b = arena_take<GmwBounds>(ar, sizeof(GmwBounds));
  if (!d_b) return FBR_ERR_HIP;
  // min / max accumulators: ordered-uint encodings of +inf-like (all ones) and -inf-like (0)
  GmwBounds h{};
  for (int d = 0; d < 3; ++d) h.mm[d] = 0xFFFFFFFFu;
  if (hipMemcpyAsync(d_b, &h, sizeof(h), hipMemcpyHostToDevice, s) != hipSuccess) return FBR_ERR_HIP;
  gm_launch_segs(k_gmw_bounds, s, src, d_b);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, d_b, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return FBR_ERR_HIP;
  info->n_dropped = (int64_t)h.n_dropped;
  if (info->n_dropped >= src.n) return FBR_OK;  // no finite point: no grid
  float mn[3], mx[3];
  for (int d = 0; d < 3; ++d) {
    mn[d] = ord2f(h.mm[d]);
    mx[d] = ord2f(h.mm[3 + d]);
  }
  gmap_grid_init(info->G, mn, mx, leaf);
  info->has_grid = 1;
  return FBR_OK;
}

int voxel_grid_wide(hipStream_t s, DevArena& ar, const GmapSrc& src, float leaf, const GmapInfo* bounds,
                    const std::function<float4*(int64_t)>& alloc_out, GmapInfo* info) {
  if (src.n > (int64_t)INT32_MAX) return FBR_ERR_CAPACITY;  // the indices are 32-bit
  GmapInfo I;
  if (bounds) {
    I = *bounds;
  } else {
    const int rc = gmap_bounds(s, ar, src, leaf, &I);
    if (rc) return rc;
  }
  I.n_out = 0;
  *info = I;
  if (src.n <= 0 || !I.has_grid) return FBR_OK;
  if (I.G.status != kGmapOk) return FBR_ERR_CAPACITY;
  const int64_t n = src.n;
  VgRuns<uint64_t> R;
  // sorted over the voxel keys' bits and the drop key's above them
  const int rc = vg_sorted_runs(s, ar, 0, n, (unsigned)I.G.nbits + 1, [&](VgRuns<uint64_t>& r) {
    gm_launch_segs(k_gmw_keys, s, src, I.G, r.k0, r.v0);
    return FBR_OK;
  }, R);
  if (rc) return rc;
  // runs of equal keys = vox[n - 1] + head[n - 1] (at most n <= INT32_MAX: the sum cannot wrap);
  // the dropped points, if any, are the last run
  uint32_t last[2] = {0, 0};
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(&last[0], R.vox + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(&last[1], R.head + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return FBR_ERR_HIP;
  const int64_t n_out = (int64_t)last[0] + (int64_t)last[1] - (I.n_dropped > 0 ? 1 : 0);
  if (n_out < 0 || n_out > n) return FBR_ERR_HIP;
  float4* out = alloc_out(n_out);
  if (!out) return FBR_ERR_HIP;
  fbr_launch(k_gmw_emit, dim3(vg_pass_grid(n)), dim3(256), 0, s, src.pool, src.segs, src.nseg, src.xform, n, gmap_drop_key(I.G),
             (const uint64_t*)R.keys, (const uint32_t*)R.vals, (const uint32_t*)R.vox, out, n_out);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return FBR_ERR_HIP;
  info->n_out = n_out;
  return FBR_OK;
}

}  // namespace fbr
