// k_scancontext.hip — place recognition on the keyframe store: scan-context descriptors and the
// exhaustive search over every stored descriptor and every column shift (include/fbr.h, "place
// recognition").  The arithmetic is fbr_sc.h's, shared with the CPU probe.
//
// k_sc_describe: one workgroup per (segment, 4096-point pass).  A segment is one cloud in one of
//   three pools (the keyframe corner pool, the keyframe surf pool, an uploaded query cloud) and a
//   destination slot; a keyframe is two segments with one slot.  The cell maxima of a pass are
//   reduced in an LDS tile (n_ring x n_sector words) with LDS atomicMax on the bits of the
//   non-negative values; the tile's non-zero cells go to the zero-initialised slot with a global
//   integer atomicMax, so a cloud of several passes merges there.  A maximum does not depend on the
//   order of its operands: the slot's bytes are the same for any point order and any schedule.
//   HBM: 16 B read per point.
// k_sc_norms: one thread per (slot, column): the column norm in double beside the descriptor.
// k_sc_search: one wave per candidate, lane = shift (n_sector <= 64).  The query and its inverse
//   column norms are staged in LDS once per workgroup; each wave stages its candidate ring-major
//   [ring][sector] and the candidate's inverse norms.  Lane s reads column (c + s) mod n_sector: unit
//   word stride across the wave, no bank conflicts.  A wave reduction over (distance, shift) leaves
//   the candidate's record.  HBM: n_ring n_sector 4 + n_sector 8 bytes per candidate.
//   No float or double atomics anywhere.

#include "fbr_common.h"
#include "fbr_kernels.h"
#include "fbr_sc.h"

namespace fbr {

constexpr int kScPass = 4096;  // points of one workgroup's pass (256 threads x 16)

__global__ void __launch_bounds__(256)
k_sc_describe(ScPools pools, const ScSeg* __restrict__ segs, int nseg, int n_ring, int n_sector, float max_radius,
              float lidar_height, uint32_t* __restrict__ desc) {
  __shared__ uint32_t tile[kScMaxRing * kScMaxSector];
  const int s = blockIdx.x;
  if (s >= nseg) return;
  const ScSeg g = segs[s];
  const int64_t i0 = (int64_t)blockIdx.y * kScPass;
  if (i0 >= g.count) return;  // (the whole workgroup)
  const int cells = n_ring * n_sector;
  for (int k = threadIdx.x; k < cells; k += 256) tile[k] = 0u;
  __syncthreads();
  const float4* __restrict__ pool = pools.p[g.pool];
  const int64_t i1 = i0 + kScPass < g.count ? i0 + kScPass : g.count;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float4 p = pool[g.src + i];
    const int cell = sc_cell(p.x, p.y, p.z, n_ring, n_sector, max_radius);
    if (cell >= 0 && cell < cells) {
      const uint32_t v = sc_value_bits(p.z, lidar_height);
      if (v) atomicMax(&tile[cell], v);
    }
  }
  __syncthreads();
  uint32_t* __restrict__ out = desc + g.slot * cells;
  for (int k = threadIdx.x; k < cells; k += 256) {
    const uint32_t v = tile[k];
    if (v) atomicMax(&out[k], v);
  }
}

__global__ void __launch_bounds__(256)
k_sc_norms(const uint32_t* __restrict__ desc, int64_t nslots, int n_ring, int n_sector, double* __restrict__ norms) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nslots * n_sector) return;
  const int64_t slot = t / n_sector;
  const int c = (int)(t - slot * n_sector);
  norms[t] = sc_column_norm(reinterpret_cast<const float*>(desc) + slot * n_ring * n_sector, n_ring, n_sector, c);
}

constexpr int kScWaves = 4;  // candidates a workgroup searches at once

// Dynamic LDS: [1 + kScWaves][n_sector] double inverse norms, then [1 + kScWaves][cells] float tiles
// (index 0 the query's, 1 + w wave w's candidate).
__global__ void __launch_bounds__(64 * kScWaves)
k_sc_search(const uint32_t* __restrict__ qdesc, const double* __restrict__ qnorm, const uint32_t* __restrict__ desc,
            const double* __restrict__ norms, int64_t n, int n_ring, int n_sector, ScRec* __restrict__ rec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
  const int cells = n_ring * n_sector;
  double* inv = reinterpret_cast<double*>(sc_lds);
  float* tiles = reinterpret_cast<float*>(inv + (1 + kScWaves) * n_sector);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < cells; k += 64 * kScWaves) tiles[k] = __builtin_bit_cast(float, qdesc[k]);
  for (int k = threadIdx.x; k < n_sector; k += 64 * kScWaves) inv[k] = sc_inverse_norm(qnorm[k]);
  float* ctile = tiles + (1 + wave) * cells;
  double* cinv = inv + (1 + wave) * n_sector;
  // every wave of a workgroup makes the same number of rounds: the barriers below are uniform
  for (int64_t base = (int64_t)blockIdx.x * kScWaves; base < n; base += (int64_t)gridDim.x * kScWaves) {
    const int64_t cand = base + wave;
    __syncthreads();  // the query is staged / the previous round's tiles are read
    if (cand < n) {
      const uint32_t* __restrict__ src = desc + cand * cells;
      for (int k = lane; k < cells; k += 64) ctile[k] = __builtin_bit_cast(float, src[k]);
      if (lane < n_sector) cinv[lane] = sc_inverse_norm(norms[cand * n_sector + lane]);
    }
    __syncthreads();
    if (cand < n) {
      double d = INFINITY;
      int sh = lane;
      if (lane < n_sector) d = sc_distance(tiles, inv, ctile, cinv, n_ring, n_sector, lane);
      for (int off = 32; off > 0; off >>= 1) {  // the minimum, ties to the lowest shift
        const double od = __shfl_xor(d, off, 64);
        const int os = __shfl_xor(sh, off, 64);
        if (od < d || (od == d && os < sh)) {
          d = od;
          sh = os;
        }
      }
      if (lane == 0) {
        ScRec r;
        r.distance = d;
        r.shift = sh;
        r.pad = 0;
        rec[cand] = r;
      }
    }
  }
}

void launch_sc_describe(hipStream_t s, const ScPools& pools, const ScSeg* segs, int nseg, int64_t max_count, int n_ring,
                        int n_sector, float max_radius, float lidar_height, uint32_t* desc) {
  if (nseg <= 0 || max_count <= 0) return;
  // max_count <= kScMaxCloud (the caller checks); a pass beyond a segment's own count returns at once
  const int passes = (int)((max_count + kScPass - 1) / kScPass);
  fbr_launch(k_sc_describe, dim3(nseg, passes), dim3(256), 0, s, pools, segs, nseg, n_ring, n_sector, max_radius,
             lidar_height, desc);
}

void launch_sc_norms(hipStream_t s, const uint32_t* desc, int64_t nslots, int n_ring, int n_sector, double* norms) {
  if (nslots <= 0) return;
  const int64_t blocks = (nslots * n_sector + 255) / 256;
  fbr_launch(k_sc_norms, dim3((unsigned)blocks), dim3(256), 0, s, desc, nslots, n_ring, n_sector, norms);
}

static size_t sc_search_lds_bytes(int n_ring, int n_sector) {
  return (size_t)(1 + kScWaves) * ((size_t)n_sector * sizeof(double) + (size_t)n_ring * n_sector * sizeof(float));
}

void launch_sc_search(hipStream_t s, const uint32_t* qdesc, const double* qnorm, const uint32_t* desc, const double* norms,
                      int64_t n, int n_ring, int n_sector, ScRec* rec) {
  if (n <= 0) return;
  const int grid = (int)std::min<int64_t>((n + kScWaves - 1) / kScWaves, 2048);
  fbr_launch(k_sc_search, dim3(grid), dim3(64 * kScWaves), (uint32_t)sc_search_lds_bytes(n_ring, n_sector), s, qdesc, qnorm,
             desc, norms, n, n_ring, n_sector, rec);
}

}  // namespace fbr
