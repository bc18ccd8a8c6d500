// k_voxel_large.hip — A9: the device-wide VoxelGrid of one large cloud (the start-up map filter,
// the keyframe local map, fbr_voxel_grid): the per-segment kernels (k_voxel.hip) give a whole
// workgroup to a segment, which leaves the chip idle for a single cloud of 10^5-10^7 points.
// Same semantics (PCL box, overflow fallback, key, float centroids in ascending key order); the
// (key, index) sort is rocprim's stable LSD radix sort (fbr_vg_runs.h), so points inside a voxel
// are summed in index order exactly as in the segmented kernels.
#include "fbr_introsort.h"
#include "fbr_vg_runs.h"
#include "fbr_vg_sort.h"

namespace fbr {

__global__ void __launch_bounds__(256) k_vgl_minmax(const float4* __restrict__ in, int64_t n, uint32_t* mm) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float4 p = in[i];
    const float v[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int d = 0; d < 3; ++d) {  // getMinMax3D's comparisons (NaN never replaces)
      mn[d] = (v[d] < mn[d]) ? v[d] : mn[d];
      mx[d] = (mx[d] < v[d]) ? v[d] : mx[d];
    }
  }
  vg_merge_bounds(mn, mx, mm);
}

struct VglState {
  VgGrid G;
  int32_t nvox;
};

__global__ void k_vgl_grid(const uint32_t* mm, float leaf, int morton, VglState* st) {
  float mn[3], mx[3];
  for (int d = 0; d < 3; ++d) {
    mn[d] = ord2f(mm[d]);
    mx[d] = ord2f(mm[3 + d]);
  }
  st->G.init(mn, mx, leaf, morton != 0);
}

__global__ void __launch_bounds__(256)
k_vgl_keys(const float4* __restrict__ in, int64_t n, const VglState* __restrict__ st, int exact, uint32_t* keys,
           uint32_t* vals) {
  const VgGrid G = st->G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    keys[i] = G.overflow ? 0u : (exact ? G.pcl_key(in[i]) : G.key(in[i]));
    vals[i] = (uint32_t)i;
  }
}

// std::sort's partition phase over the whole cloud (fbr_introsort.h) by one workgroup: PCL's
// order inside the voxels for the stable device-wide radix sort that follows.  n / 17 + 2 frames
// per list in fa / fb.
__global__ void __launch_bounds__(1024)
k_vgl_isort(uint32_t* keys, uint32_t* vals, int32_t* posL, int32_t* posR, int* fa, int* fb, int n) {
  __shared__ int sh[64];
  is_partition_phase<1024>(keys, vals, posL, posR, n, fa, fb, sh);
}

__global__ void __launch_bounds__(256) k_vgl_outkeys(uint32_t* keys, int64_t n, const VglState* __restrict__ st) {
  const VgGrid G = st->G;
  if (!G.morton || G.overflow) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    keys[i] = G.out_key(keys[i]);
}

__global__ void __launch_bounds__(256)
k_vgl_emit(const float4* __restrict__ in, int64_t n, const VglState* __restrict__ st, const uint32_t* __restrict__ keys,
           const uint32_t* __restrict__ vals, const uint32_t* __restrict__ vox, float4* __restrict__ out,
           int32_t* __restrict__ nout) {
  const bool overflow = st->G.overflow;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (overflow) {  // PCL: "Leaf size is too small" -> output = input
      out[i] = in[i];
      if (i == 0) *nout = (int32_t)n;
      continue;
    }
    if (!vg_run_head(keys, i)) continue;
    int64_t j;
    out[vox[i]] = vg_run_centroid(keys, n, i, [&](int64_t k) { return in[vals[k]]; }, &j);
    if (j == n) *nout = (int32_t)vox[i] + 1;
  }
}

int voxel_grid_large(hipStream_t s, DevArena& ar, const float4* in, int64_t n, float leaf, int morton, int exact,
                     float4* out, int32_t* d_nout) {
  if (n <= 0) return hipMemsetAsync(d_nout, 0, sizeof(int32_t), s) == hipSuccess ? FBR_OK : FBR_ERR_HIP;
  if (n > (int64_t)INT32_MAX) return FBR_ERR_CAPACITY;
  const int grid = vg_pass_grid(n);
  VglState* st = nullptr;
  VgRuns<uint32_t> R;
  const size_t own = arena_bytes(6 * sizeof(uint32_t)) + arena_bytes(sizeof(VglState));  // mm, st
  const int rc = vg_sorted_runs(s, ar, own, n, 32, [&](VgRuns<uint32_t>& r) {
    uint32_t* mm = arena_take<uint32_t>(ar, 6 * sizeof(uint32_t));
    st = arena_take<VglState>(ar, sizeof(VglState));
    // min / max accumulators: ordered-uint encodings of +inf-like (all ones) and -inf-like (0)
    if (!mm || !st || hipMemsetD32Async((hipDeviceptr_t)mm, 0xFFFFFFFFu, 3, s) != hipSuccess ||
        hipMemsetD32Async((hipDeviceptr_t)(mm + 3), 0u, 3, s) != hipSuccess)
      return FBR_ERR_HIP;
    fbr_launch(k_vgl_minmax, dim3(grid), dim3(256), 0, s, in, n, mm);
    fbr_launch(k_vgl_grid, dim3(1), dim3(1), 0, s, mm, leaf, morton, st);
    fbr_launch(k_vgl_keys, dim3(grid), dim3(256), 0, s, in, n, st, exact, r.k0, r.v0);
    if (exact) {  // scratch: head / vox (positions) and keys / vals (frame lists), all free until the sort
      fbr_launch(k_vgl_isort, dim3(1), dim3(1024), 0, s, r.k0, r.v0, (int32_t*)r.head, (int32_t*)r.vox, (int*)r.keys,
                 (int*)r.vals, (int)n);
      fbr_launch(k_vgl_outkeys, dim3(grid), dim3(256), 0, s, r.k0, n, st);
    }
    return FBR_OK;
  }, R);
  if (rc == FBR_OK) fbr_launch(k_vgl_emit, dim3(grid), dim3(256), 0, s, in, n, st, R.keys, R.vals, R.vox, out, d_nout);
  return rc;
}

}  // namespace fbr
