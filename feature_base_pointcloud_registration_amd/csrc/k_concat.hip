// k_concat.hip — the per-job feature clouds from the per-ring ones.
#include "fbr_common.h"
#include "fbr_kernels.h"

namespace fbr {

// Ring-ordered concatenation of the per-ring corner picks and per-ring surf DS outputs
// (cornerCloud / surfaceCloud of featureExtraction.h).  One wave per (job, ring), 4 rings per
// workgroup: the wave sums the counts of the rings before its own (lanes over rings, a shuffle
// reduction) and copies its ring's corner picks and surf DS points to their offsets; the last
// ring's wave writes the job totals.
__global__ void __launch_bounds__(256)
k_concat(int H, int W, const float4* corner_slot, const int32_t* corner_cnt, const float4* surf_ring,
         const int32_t* surf_ring_cnt, float4* corner_all, int64_t capc, int32_t* n_corner, float4* surf_all,
         int64_t caps, int32_t* n_surf, float* ring_box) {
  const int lane = threadIdx.x & 63, rpj = (H + 3) / 4;
  const int job = blockIdx.x / rpj, r = (blockIdx.x % rpj) * 4 + (threadIdx.x >> 6);
  if (r >= H) return;
  const int32_t* cc = corner_cnt + job * H;
  const int32_t* sc = surf_ring_cnt + job * H;
  int oc = 0, os = 0;
  for (int k = lane; k < r; k += 64) {
    oc += cc[k];
    os += sc[k];
  }
  for (int o = 32; o > 0; o >>= 1) {
    oc += __shfl_xor(oc, o);
    os += __shfl_xor(os, o);
  }
  const int nc = cc[r], ns = sc[r];
  if (r == H - 1 && lane == 0) {
    n_corner[job] = oc + nc;
    n_surf[job] = os + ns;
  }
  const float4* cs = corner_slot + ((int64_t)job * H + r) * kCornerPerRing;
  const float4* ss = surf_ring + ((int64_t)job * H + r) * W;
  float bx[2][6];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      bx[c][d] = FLT_MAX;
      bx[c][3 + d] = -FLT_MAX;
    }
  auto grow = [&](float (&b)[6], const float4& p) {
    const float v[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      b[d] = (v[d] < b[d]) ? v[d] : b[d];
      b[3 + d] = (b[3 + d] < v[d]) ? v[d] : b[3 + d];
    }
  };
  for (int i = lane; i < nc; i += 64) {
    const float4 p = cs[i];
    corner_all[job * capc + oc + i] = p;
    grow(bx[0], p);
  }
  for (int i = lane; i < ns; i += 64) {
    const float4 p = ss[i];
    surf_all[job * caps + os + i] = p;
    grow(bx[1], p);
  }
  if (!ring_box) return;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d)
      for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(bx[c][d], o), b = __shfl_xor(bx[c][3 + d], o);
        bx[c][d] = (a < bx[c][d]) ? a : bx[c][d];
        bx[c][3 + d] = (bx[c][3 + d] < b) ? b : bx[c][3 + d];
      }
  if (lane < kRingBox) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < kRingBox; ++k)
      if (lane == k) v = bx[k / 6][k % 6];
    ring_box[((int64_t)job * H + r) * kRingBox + lane] = v;
  }
}

void launch_concat(hipStream_t s, int B, int H, int W, const float4* corner_slot, const int32_t* corner_cnt,
                   const float4* surf_ring, const int32_t* surf_ring_cnt, float4* corner_all, int64_t capc,
                   int32_t* n_corner, float4* surf_all, int64_t caps, int32_t* n_surf, float* ring_box) {
  if (B <= 0 || H <= 0) return;
  fbr_launch(k_concat, dim3(B * ((H + 3) / 4)), dim3(256), 0, s, H, W, corner_slot, corner_cnt, surf_ring,
                     surf_ring_cnt, corner_all, capc, n_corner, surf_all, caps, n_surf, ring_box);
}

}  // namespace fbr
