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
//   rocprim::radix_sort_pairs over the bits the grid needs (stable: a voxel's points stay in index order)
//   k_gmw_heads, rocprim::exclusive_scan: voxel index of every run of equal keys
//   k_gmw_emit    one centroid per run, its points re-transformed from the pool and summed in index
//                 order: k_vgl_emit's arithmetic (k_voxel.hip), float sum / float count
// HBM-bound: the pool is read twice in stream order (16 B per point) and once gathered by the
// emit; keys and indices cost 12 B per point written, sorted and read.  No float atomics: two calls
// return the same bytes.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fbr_common.h"
#include "fbr_gmap.h"
#include "fbr_kernels.h"

#include <algorithm>
#include <cstring>

namespace fbr {

namespace {

__device__ __forceinline__ uint32_t gm_f2ord(float f) {  // order-preserving float -> uint
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float gm_ord2f(uint32_t u) {
  const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

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
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    for (int o = 32; o > 0; o >>= 1) {
      const float a = __shfl_xor(mn[d], o), b = __shfl_xor(mx[d], o);
      mn[d] = (a < mn[d]) ? a : mn[d];
      mx[d] = (mx[d] < b) ? b : mx[d];
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&B->mm[d], gm_f2ord(mn[d]));
      atomicMax(&B->mm[3 + d], gm_f2ord(mx[d]));
    }
  }
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

__global__ void __launch_bounds__(256) k_gmw_heads(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ head) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
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
    if (!(i == 0 || keys[i] != keys[i - 1])) continue;
    const uint64_t key = keys[i];
    if (key == drop_key) continue;  // the run of dropped points (the last one)
    const int64_t o = (int64_t)vox[i];
    if (o >= n_out) continue;  // cannot happen: the output holds every voxel before the dropped run
    int sg = gm_find_seg(segs, nseg, (int64_t)vals[i], 0);
    float4 c = gm_point(pool, segs[sg], xform, (int64_t)vals[i] - segs[sg].dst);
    int64_t j = i + 1;
    while (j < n && keys[j] == key) {
      sg = gm_find_seg(segs, nseg, (int64_t)vals[j], sg);
      const float4 p = gm_point(pool, segs[sg], xform, (int64_t)vals[j] - segs[sg].dst);
      c.x += p.x;
      c.y += p.y;
      c.z += p.z;
      c.w += p.w;
      ++j;
    }
    const float cnt = (float)(j - i);
    out[o] = make_float4(c.x / cnt, c.y / cnt, c.z / cnt, c.w / cnt);
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
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
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
    mn[d] = gm_ord2f(h.mm[d]);
    mx[d] = gm_ord2f(h.mm[3 + d]);
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
  const size_t N = (size_t)n;
  const unsigned end_bit = (unsigned)I.G.nbits + 1;  // the voxel keys and the drop key above them
  size_t tb_sort = 0, tb_scan = 0;
  uint64_t* null64 = nullptr;
  uint32_t* null32 = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, tb_sort, null64, null64, null32, null32, N, 0, end_bit, s) != hipSuccess ||
      rocprim::exclusive_scan(nullptr, tb_scan, null32, null32, 0u, N, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return FBR_ERR_HIP;
  const size_t tb = std::max<size_t>(std::max(tb_sort, tb_scan), 16);
  if (arena_reserve(ar, 2 * arena_bytes(8 * N) + 4 * arena_bytes(4 * N) + arena_bytes(tb), s) != hipSuccess)
    return FBR_ERR_HIP;
  uint64_t* k0 = arena_take<uint64_t>(ar, 8 * N);
  uint64_t* k1 = arena_take<uint64_t>(ar, 8 * N);
  uint32_t* v0 = arena_take<uint32_t>(ar, 4 * N);
  uint32_t* v1 = arena_take<uint32_t>(ar, 4 * N);
  uint32_t* head = arena_take<uint32_t>(ar, 4 * N);
  uint32_t* vox = arena_take<uint32_t>(ar, 4 * N);
  void* tmp = arena_take<void>(ar, tb);
  if (!k0 || !k1 || !v0 || !v1 || !head || !vox || !tmp) return FBR_ERR_HIP;  // arena sizing slip
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
  gm_launch_segs(k_gmw_keys, s, src, I.G, k0, v0);
  if (rocprim::radix_sort_pairs(tmp, tb_sort, k0, k1, v0, v1, N, 0, end_bit, s) != hipSuccess) return FBR_ERR_HIP;
  fbr_launch(k_gmw_heads, dim3(grid), dim3(256), 0, s, (const uint64_t*)k1, n, head);
  if (rocprim::exclusive_scan(tmp, tb_scan, head, vox, 0u, N, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return FBR_ERR_HIP;
  // runs of equal keys = vox[n - 1] + head[n - 1] (at most n <= INT32_MAX: the sum cannot wrap);
  // the dropped points, if any, are the last run
  uint32_t last[2] = {0, 0};
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(&last[0], vox + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(&last[1], head + (n - 1), 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return FBR_ERR_HIP;
  const int64_t n_out = (int64_t)last[0] + (int64_t)last[1] - (I.n_dropped > 0 ? 1 : 0);
  if (n_out < 0 || n_out > n) return FBR_ERR_HIP;
  float4* out = alloc_out(n_out);
  if (!out) return FBR_ERR_HIP;
  fbr_launch(k_gmw_emit, dim3(grid), dim3(256), 0, s, src.pool, src.segs, src.nseg, src.xform, n, gmap_drop_key(I.G),
             (const uint64_t*)k1, (const uint32_t*)v1, (const uint32_t*)vox, out, n_out);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return FBR_ERR_HIP;
  info->n_out = n_out;
  return FBR_OK;
}

}  // namespace fbr
