// fbr_vg_runs.h — the tail the two device-wide VoxelGrids share (k_voxel_large.hip: PCL's 32-bit
// keys; k_gmap.hip: 64-bit keys): rocprim's stable radix sort of the (key, index) pairs, a head
// flag per run of equal keys, their exclusive scan (the run's voxel index) and the centroid of a
// run, its points summed in index order.  Where PCL does not overflow the two filters must return
// the same bytes (tests/test_global_map.py), so this arithmetic stands here once.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "fbr_common.h"
#include "fbr_kernels.h"

namespace fbr {

// Order-preserving float <-> uint, for bounds kept by atomicMin / atomicMax (neutral elements: all
// ones / 0).  The host decodes too (gmap_bounds).
__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(uint32_t u) { return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// Merges a wave's per-lane bounds into mm[6] (ordered-uint min x, y, z, max x, y, z): getMinMax3D's
// comparisons, so the result does not depend on the order.
__device__ __forceinline__ void vg_merge_bounds(float (&mn)[3], float (&mx)[3], uint32_t* mm) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    for (int o = 32; o > 0; o >>= 1) {
      const float a = __shfl_xor(mn[d], o), b = __shfl_xor(mx[d], o);
      mn[d] = (a < mn[d]) ? a : mn[d];
      mx[d] = (mx[d] < b) ? b : mx[d];
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&mm[d], f2ord(mn[d]));
      atomicMax(&mm[3 + d], f2ord(mx[d]));
    }
  }
}

// Workgroups of a 256-thread grid-stride pass over n elements.
inline int vg_pass_grid(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 4096); }

template <typename K>
__device__ __forceinline__ bool vg_run_head(const K* keys, int64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

template <typename K>
__global__ void __launch_bounds__(256) k_vg_heads(const K* __restrict__ keys, int64_t n, uint32_t* __restrict__ head) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    head[i] = vg_run_head(keys, i) ? 1u : 0u;
}

template <typename K>  // uint32_t or uint64_t
struct VgRuns {
  K *k0, *keys;          // the pairs as the caller wrote them / sorted by key, stable
  uint32_t *v0, *vals;
  uint32_t *head, *vox;  // 1 at the first pair of a run / the run's index
};

// Carves R's arrays of n pairs from the arena (asked for `extra` bytes more: the caller's own
// slices, taken inside fill), has fill(R) enqueue the kernels that write k0 / v0 (the other four
// arrays are free scratch until it returns; it returns an FBR_* code), sorts by key bits
// [0, end_bit) and numbers the runs.  All on s; no synchronisation unless the arena grows.
template <typename K, typename Fill>
int vg_sorted_runs(hipStream_t s, DevArena& ar, size_t extra, int64_t n, unsigned end_bit, Fill&& fill, VgRuns<K>& R) {
  const size_t N = (size_t)n;
  size_t tb_sort = 0, tb_scan = 0;
  K* nullk = nullptr;
  uint32_t* null32 = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, tb_sort, nullk, nullk, null32, null32, N, 0, end_bit, s) != hipSuccess ||
      rocprim::exclusive_scan(nullptr, tb_scan, null32, null32, 0u, N, rocprim::plus<uint32_t>(), s) != hipSuccess)
    return FBR_ERR_HIP;
  const size_t tb = std::max<size_t>(std::max(tb_sort, tb_scan), 16);
  if (arena_reserve(ar, extra + 2 * arena_bytes(sizeof(K) * N) + 4 * arena_bytes(4 * N) + arena_bytes(tb), s) != hipSuccess)
    return FBR_ERR_HIP;
  R.k0 = arena_take<K>(ar, sizeof(K) * N);
  R.keys = arena_take<K>(ar, sizeof(K) * N);
  R.v0 = arena_take<uint32_t>(ar, 4 * N);
  R.vals = arena_take<uint32_t>(ar, 4 * N);
  R.head = arena_take<uint32_t>(ar, 4 * N);
  R.vox = arena_take<uint32_t>(ar, 4 * N);
  void* tmp = arena_take<void>(ar, tb);
  if (!R.k0 || !R.keys || !R.v0 || !R.vals || !R.head || !R.vox || !tmp) return FBR_ERR_HIP;  // arena sizing slip
  const int rc = fill(R);
  if (rc != FBR_OK) return rc;
  if (rocprim::radix_sort_pairs(tmp, tb_sort, R.k0, R.keys, R.v0, R.vals, N, 0, end_bit, s) != hipSuccess) return FBR_ERR_HIP;
  fbr_launch(k_vg_heads<K>, dim3(vg_pass_grid(n)), dim3(256), 0, s, (const K*)R.keys, n, R.head);
  // head flags -> voxel index, out of place (the in-place scan raced: repeat calls differed)
  const hipError_t e = rocprim::exclusive_scan(tmp, tb_scan, R.head, R.vox, 0u, N, rocprim::plus<uint32_t>(), s);
  return e == hipSuccess ? FBR_OK : FBR_ERR_HIP;
}

// Centroid of the run of equal keys that starts at sorted position i; *end gets the run's end.
// point(j) is the point of sorted position j: the float sum in that order, divided by the float
// count (PCL's centroid, the segmented kernels' arithmetic).
template <typename K, typename P>
__device__ __forceinline__ float4 vg_run_centroid(const K* __restrict__ keys, int64_t n, int64_t i, P&& point, int64_t* end) {
  const K key = keys[i];
  float4 c = point(i);
  int64_t j = i + 1;
  for (; j < n && keys[j] == key; ++j) {
    const float4 p = point(j);
    c = make_float4(c.x + p.x, c.y + p.y, c.z + p.z, c.w + p.w);
  }
  const float cnt = (float)(j - i);
  *end = j;
  return make_float4(c.x / cnt, c.y / cnt, c.z / cnt, c.w / cnt);
}

}  // namespace fbr
