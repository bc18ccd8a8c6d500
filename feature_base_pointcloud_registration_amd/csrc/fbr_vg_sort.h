// fbr_vg_sort.h — device-only: what the one-workgroup VoxelGrid kernels share (k_voxel.hip,
// k_voxel_ring.hip, k_voxel_large.hip's grid, the radix selftests of k_selftest.hip): PCL's grid
// and key (VgGrid), the block bounds, the wave-chunk radix sorts and the run emit.
#pragma once
#include "fbr_common.h"
#include "fbr_kernels.h"

namespace fbr {

constexpr int kVgIpKpl = 18;  // k_voxel_grid_ip: segments up to 1024 * 18 points sort in LDS
constexpr int kVgIpSmallT = 256, kVgIpSmallKpl = 16;  // its small size class (launch_voxel_grid)

// Stable LSD radix sort of one segment by one workgroup of T threads ("wave chunks"): wave w owns
// the contiguous chunk [c0, c1) of the (key, index) array; per pass each wave builds an LDS digit
// histogram of its chunk, one digit-major / wave-minor exclusive scan gives every (digit, wave)
// its output base, and each wave scatters its chunk in index order (8..9 ballots give each lane
// its rank among equal digits in the 64-element step).  Waves in chunk order and steps in index
// order make the sort stable.  Keys and indices live in LDS when the segment fits (per-ring
// filters, u16 indices), otherwise in a per-segment global scratch (mapping DS, 1024 threads).

__device__ __forceinline__ uint32_t spread3_10(uint32_t v) {  // 10 bits -> every third bit
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// ---- shared pieces of the two VoxelGrid front ends ----

// Block-wide float min / max (getMinMax3D) of per-thread partials; mm = [NW][6] LDS.
template <int T>
__device__ void vg_block_minmax(float (&mn)[3], float (&mx)[3], float* mm) {
  constexpr int NW = T / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < 3; ++d)
    for (int o = 32; o > 0; o >>= 1) {
      const float a = __shfl_xor(mn[d], o), b = __shfl_xor(mx[d], o);
      mn[d] = (a < mn[d]) ? a : mn[d];
      mx[d] = (mx[d] < b) ? b : mx[d];
    }
  if (lane == 0)
    for (int d = 0; d < 3; ++d) {
      mm[w * 6 + d] = mn[d];
      mm[w * 6 + 3 + d] = mx[d];
    }
  __syncthreads();
  for (int d = 0; d < 3; ++d) {
    mn[d] = mm[d];
    mx[d] = mm[3 + d];
    for (int ww = 1; ww < NW; ++ww) {
      const float a = mm[ww * 6 + d], b = mm[ww * 6 + 3 + d];
      mn[d] = (a < mn[d]) ? a : mn[d];
      mx[d] = (mx[d] < b) ? b : mx[d];
    }
  }
}

// getMinMax3D of segment seg (its first n points): from the producer's ring boxes when the set
// has them (k_concat; bounds are exact under any merge order), else from the points.  All threads
// get the result.
template <int T>
__device__ void vg_seg_bounds(const VgSet& S, int seg, int n, const float4* in, float (&mn)[3], float (&mx)[3],
                              float* mm) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = FLT_MAX;
    mx[d] = -FLT_MAX;
  }
  if (S.box && (int64_t)S.cnt_in[seg] <= S.cap) {  // boxes cover exactly the segment's points
    const float* bx = S.box + (int64_t)seg * S.box_stride;
    for (int k = threadIdx.x; k < S.box_n; k += T) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float a = bx[(int64_t)k * kRingBox + d], b = bx[(int64_t)k * kRingBox + 3 + d];
        mn[d] = (a < mn[d]) ? a : mn[d];
        mx[d] = (mx[d] < b) ? b : mx[d];
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += T) {
      const float4 p = in[i];
      const float v[3] = {p.x, p.y, p.z};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        mn[d] = (v[d] < mn[d]) ? v[d] : mn[d];
        mx[d] = (mx[d] < v[d]) ? v[d] : mx[d];
      }
    }
  }
  vg_block_minmax<T>(mn, mx, mm);
}

// PCL applyFilter's grid (leaf inverse, min_b, div_b) and the key function.
struct VgGrid {
  float inv;
  int min_b[3];
  uint32_t mul1, mul2;
  bool morton, overflow;
  int nbits;
  __device__ void init(const float (&mn)[3], const float (&mx)[3], float leaf, bool want_morton) {
    inv = 1.0f / leaf;
    const int64_t dx = (int64_t)((mx[0] - mn[0]) * inv) + 1;
    const int64_t dy = (int64_t)((mx[1] - mn[1]) * inv) + 1;
    const int64_t dz = (int64_t)((mx[2] - mn[2]) * inv) + 1;
    overflow = dx * dy * dz > (int64_t)INT32_MAX;  // PCL: "Leaf size is too small" -> output = input
    int div_b[3];
    for (int d = 0; d < 3; ++d) {
      min_b[d] = (int)floorf(mn[d] * inv);
      const int max_b = (int)floorf(mx[d] * inv);
      div_b[d] = max_b - min_b[d] + 1;
    }
    mul1 = (uint32_t)div_b[0];
    mul2 = (uint32_t)div_b[0] * (uint32_t)div_b[1];
    morton = want_morton && div_b[0] <= 1024 && div_b[1] <= 1024 && div_b[2] <= 1024;
    nbits = 32;
    if (morton) {
      int b = 1;
      for (int d = 0; d < 3; ++d)
        if (div_b[d] > 1) b = max(b, 32 - __clz((uint32_t)(div_b[d] - 1)));
      nbits = 3 * b;
    } else {
      const uint64_t nkeys = (uint64_t)div_b[0] * (uint64_t)div_b[1] * (uint64_t)div_b[2];
      if (nkeys <= 0xFFFFFFFFull) {
        const uint32_t maxk = (uint32_t)(nkeys - 1);
        nbits = maxk == 0 ? 1 : 32 - __clz(maxk);
      }
    }
  }
  // PCL's key (the one std::sort compares), whatever the output order
  __device__ __forceinline__ uint32_t pcl_key(const float4& p) const {
    const int ijk0 = (int)(floorf(p.x * inv) - (float)min_b[0]);
    const int ijk1 = (int)(floorf(p.y * inv) - (float)min_b[1]);
    const int ijk2 = (int)(floorf(p.z * inv) - (float)min_b[2]);
    return (uint32_t)ijk0 + (uint32_t)ijk1 * mul1 + (uint32_t)ijk2 * mul2;
  }
  // the output-order key of a PCL key (its Morton code in Morton mode; ijk < div_b decodes uniquely)
  __device__ __forceinline__ uint32_t out_key(uint32_t k) const {
    if (!morton) return k;
    const uint32_t k2 = k / mul2, r = k - k2 * mul2, k1 = r / mul1, k0 = r - k1 * mul1;
    return spread3_10(k0) | (spread3_10(k1) << 1) | (spread3_10(k2) << 2);
  }
  __device__ __forceinline__ uint32_t key(const float4& p) const {
    const int ijk0 = (int)(floorf(p.x * inv) - (float)min_b[0]);
    const int ijk1 = (int)(floorf(p.y * inv) - (float)min_b[1]);
    const int ijk2 = (int)(floorf(p.z * inv) - (float)min_b[2]);
    return morton ? (spread3_10((uint32_t)ijk0) | (spread3_10((uint32_t)ijk1) << 1) | (spread3_10((uint32_t)ijk2) << 2))
                  : (uint32_t)ijk0 + (uint32_t)ijk1 * mul1 + (uint32_t)ijk2 * mul2;
  }
};

// LDS-mode buffers are accessed through address-space-3 pointers: the ping-pong selection by a
// loop-carried index otherwise leaves generic pointers, i.e. flat_* instead of ds_* accesses.
#define FBR_LDS_AS __attribute__((address_space(3)))
template <bool L, typename X>
__device__ __forceinline__ auto lds_if(X* p) {
  if constexpr (L) return (FBR_LDS_AS X*)p;
  else return p;
}

// Stable LSD radix sort of kb[0]/vb[0] (n pairs) over the low nbits key bits; returns the index
// (0/1) of the buffers holding the sorted pairs.  Ends with a barrier.
template <int T, typename V, int MAXD = 9, bool KV_LDS = true>
__device__ int vg_radix_sort(uint32_t* (&kb)[2], V* (&vb)[2], int n, int nbits, uint32_t* hist, uint32_t* wsum,
                             int dbg = 0) {
  constexpr int NW = T / 64, NB = 1 << MAXD;  // digits of <= MAXD bits; hist rows of NB counters
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int passes = dbg == 1 ? 0 : (nbits + MAXD - 1) / MAXD;
  const int dbits = passes > 0 ? (nbits + passes - 1) / passes : MAXD;
  const int nbins = 1 << dbits;
  const int chunk = (((n + NW - 1) / NW) + 63) & ~63;
  const int c0 = min(n, w * chunk), c1 = min(n, c0 + chunk);
  // Counters live at hist[w * NB + d] (lanes of one wave hit distinct banks); the exclusive scan
  // runs over them in digit-major, wave-minor order, which gives every (digit, wave) its output
  // base (waves in chunk order -> stable)
  constexpr int PER = NB * NW / T;
  int cur = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = dbits * pass;
    const uint32_t dmask = (uint32_t)nbins - 1u;
    const int tot = nbins * NW;
    const auto kin = lds_if<KV_LDS>(kb[cur]);
    const auto vin = lds_if<KV_LDS>(vb[cur]);
    const auto kout = lds_if<KV_LDS>(kb[cur ^ 1]);
    const auto vout = lds_if<KV_LDS>(vb[cur ^ 1]);
    for (int b = tid; b < tot; b += T) hist[(b % NW) * NB + b / NW] = 0u;
    __syncthreads();
    // per-wave digit counts: one add per distinct digit of a 64-step, by the lowest lane holding it
    // (ballot peer masks; per-element LDS atomics serialise on the long equal-digit runs that
    // spatially ordered keys have in their upper digits)
    for (int i0 = c0; i0 < c1; i0 += 64) {
      const int i = i0 + lane;
      const bool valid = i < c1;
      const uint32_t d = valid ? (kin[i] >> shift) & dmask : 0u;
      uint64_t peers = __ballot(valid);
      for (int b = 0; b < dbits; ++b) {
        const uint64_t bal = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? bal : ~bal;
      }
      if (valid && (peers & ((1ull << lane) - 1ull)) == 0ull) hist[w * NB + d] += (uint32_t)__popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
      uint32_t v[PER], loc = 0;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int idx = tid * PER + k;
        v[k] = idx < tot ? hist[(idx % NW) * NB + idx / NW] : 0u;
        loc += v[k];
      }
      uint32_t inc = loc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
      }
      if (lane == 63) wsum[w] = inc;
      __syncthreads();
      uint32_t run = inc - loc;
      for (int ww = 0; ww < w; ++ww) run += wsum[ww];
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int idx = tid * PER + k;
        if (idx < tot) hist[(idx % NW) * NB + idx / NW] = run;
        run += v[k];
      }
    }
    __syncthreads();
    for (int i0 = c0; i0 < c1; i0 += 64) {
      const int i = i0 + lane;
      const bool valid = i < c1;
      const uint32_t key = valid ? kin[i] : 0u;
      const uint32_t d = (key >> shift) & dmask;
      uint64_t peers = __ballot(valid);
      for (int b = 0; b < dbits; ++b) {
        const uint64_t bal = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? bal : ~bal;
      }
      const int rank = __popcll(peers & ((1ull << lane) - 1ull));
      uint32_t* hc = &hist[w * NB + d];
      const uint32_t base = valid ? *hc : 0u;
      if (valid) {
        kout[base + rank] = key;
        vout[base + rank] = vin[i];
      }
      __builtin_amdgcn_wave_barrier();
      if (valid && rank == 0) *hc = base + (uint32_t)__popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}

// Stable in-place LSD radix sort of an LDS-resident segment (n <= T * KPL pairs): every wave keeps
// its chunk (KPL 64-element steps) in registers, so a pass reads the whole chunk before the barrier
// and scatters straight into the same LDS arrays after it -- no ping-pong buffer, no global scratch.
// The ranking is vg_radix_sort's (wave chunks in order, ballot peer masks), so the sort is stable.
// 8-bit digits (hist holds (NW + 1) * 256 counters).  Ends with a barrier.  Always inlined: with
// two callers (the exact and default kernels) the compiler outlined it, and the call frame put
// 80 B per lane in scratch (spilled on every call: ~50 MB of writes per B = 1024 launch).
// kLeader (diagnostic, fbr_selftest_radix_sort only): 1 = per-wave digit counts by the lowest lane
// of each digit's ballot peer group instead of LDS atomics; 2 = that, plus round 3's wave-uniform
// early exit (`if (c0 + 64 * k >= c1) break;`) in the count and scatter loops: the exact form that
// mis-sorted in round 3.
template <int T, int KPL, int kLeader = 0>
__device__ __attribute__((always_inline)) void vg_radix_sort_inplace(FBR_LDS_AS uint32_t* keys, FBR_LDS_AS uint16_t* vals, int n, int nbits,
                                      uint32_t* hist, uint32_t* wsum) {
  constexpr int NW = T / 64, NB = 256, PER = NB * NW / T;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int passes = (nbits + 7) / 8;
  const int dbits = passes > 0 ? (nbits + passes - 1) / passes : 8;
  const uint32_t dmask = (1u << dbits) - 1u;
  const int nbins = 1 << dbits, tot = nbins * NW;
  const int chunk = (((n + NW - 1) / NW) + 63) & ~63;
  const int c0 = min(n, w * chunk), c1 = min(n, c0 + chunk);
  // The product form (kLeader 0) leaves the load, count and scatter loops at the wave's first
  // empty step (a C2 surf cloud fills 14 of its waves' 18 steps, a corner cloud 5 of 16, a part of
  // the split kernel fewer), and an empty step still costs its ballots.  (Round 5 replayed this
  // exit three ways without a mis-sort)
  constexpr bool kSkip = kLeader == 0;
  uint32_t kr[KPL], vr[KPL];
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = dbits * pass;
#pragma unroll
    for (int k = 0; k < KPL; ++k) {
      if constexpr (kSkip)
        if (c0 + 64 * k >= c1) break;  // wave-uniform
      const int i = c0 + 64 * k + lane;
      kr[k] = i < c1 ? keys[i] : 0u;
      vr[k] = i < c1 ? vals[i] : 0u;
    }
    for (int b = tid; b < tot; b += T) hist[(b % NW) * NB + b / NW] = 0u;
    __syncthreads();  // every wave holds its chunk: the scatter below may overwrite any position
    if constexpr (kLeader != 0) {
#pragma unroll
      for (int k = 0; k < KPL; ++k) {
        if constexpr (kLeader == 2)
          if (c0 + 64 * k >= c1) break;  // wave-uniform
        const bool valid = c0 + 64 * k + lane < c1;
        const uint32_t d = (kr[k] >> shift) & dmask;
        uint64_t peers = __ballot(valid);
        for (int b = 0; b < dbits; ++b) {
          const uint64_t bal = __ballot((d >> b) & 1u);
          peers &= ((d >> b) & 1u) ? bal : ~bal;
        }
        if (valid && (peers & ((1ull << lane) - 1ull)) == 0ull) hist[w * NB + d] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
      }
    } else {
#pragma unroll
      for (int k = 0; k < KPL; ++k) {
        if constexpr (kSkip)
          if (c0 + 64 * k >= c1) break;  // wave-uniform
        if (c0 + 64 * k + lane < c1) atomicAdd(&hist[w * NB + ((kr[k] >> shift) & dmask)], 1u);
      }
    }
    __syncthreads();
    {
      uint32_t v[PER], loc = 0;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int idx = tid * PER + k;
        v[k] = idx < tot ? hist[(idx % NW) * NB + idx / NW] : 0u;
        loc += v[k];
      }
      uint32_t inc = loc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
      }
      if (lane == 63) wsum[w] = inc;
      __syncthreads();
      uint32_t run = inc - loc;
      for (int ww = 0; ww < w; ++ww) run += wsum[ww];
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int idx = tid * PER + k;
        if (idx < tot) hist[(idx % NW) * NB + idx / NW] = run;
        run += v[k];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KPL; ++k) {
      if constexpr (kLeader == 2 || kSkip)
        if (c0 + 64 * k >= c1) break;  // wave-uniform: the rest of the chunk is empty
      const bool valid = c0 + 64 * k + lane < c1;
      const uint32_t d = (kr[k] >> shift) & dmask;
      uint64_t peers = __ballot(valid);
      for (int b = 0; b < dbits; ++b) {
        const uint64_t bal = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? bal : ~bal;
      }
      const int rank = __popcll(peers & ((1ull << lane) - 1ull));
      uint32_t* hc = &hist[w * NB + d];
      const uint32_t base = valid ? *hc : 0u;
      if (valid) {
        keys[base + rank] = kr[k];
        vals[base + rank] = (uint16_t)vr[k];
      }
      __builtin_amdgcn_wave_barrier();
      if (valid && rank == 0) *hc = base + (uint32_t)__popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
}

// Stable radix sort of kb[0]/vb[0] (n pairs), then one centroid per run of equal keys in
// ascending key order: out[v] = mean of in[vals of the run].  Returns the voxel count (all threads).
template <int T, typename V, int MAXD = 9, bool KV_LDS = true>
__device__ int vg_sort_emit(uint32_t* (&kb)[2], V* (&vb)[2], int n, int nbits, uint32_t* hist, uint32_t* wsum,
                            const float4* in, float4* out, int dbg = 0, unsigned long long* t_sorted = nullptr);

// One centroid per run of equal keys of the sorted pairs ks / vs (n), in ascending key order.
// hist must hold NW KB (the per-wave point stage), and with kStage NW * 2176 B: the centroids then
// collect in a per-wave LDS ring of kEmitRing and leave as whole 128-B lines (a step completes a
// few scattered centroids, and partial-line stores cost the L2 a write each time the line is
// evicted half written).  Returns the voxel count (all threads).
constexpr int kEmitRing = 72;  // >= 7 unflushed + 65 written in one step (see the flush below)
template <int T, bool kStage = false, typename KP, typename VP>
__device__ int vg_emit(KP ks, VP vs, int n, uint32_t* hist, uint32_t* wsum, const float4* in, float4* out) {
  constexpr int NW = T / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int chunk = (((n + NW - 1) / NW) + 63) & ~63;
  const int c0 = min(n, w * chunk), c1 = min(n, c0 + chunk);
  // ---- voxels in ascending key order: heads of equal-key runs, centroid = float sum / count ----
  int nh = 0;
  for (int i0 = c0; i0 < c1; i0 += 64) {
    const int i = i0 + lane;
    nh += __popcll(__ballot(i < c1 && (i == 0 || ks[i] != ks[i - 1])));
  }
  if (lane == 0) wsum[w] = (uint32_t)nh;
  __syncthreads();
  int pos = 0;
  for (int ww = 0; ww < w; ++ww) pos += (int)wsum[ww];
  int total = pos;
  for (int ww = w; ww < NW; ++ww) total += (int)wsum[ww];
  // Runs of equal keys are summed in sorted order (the serial float sum of the reference) out of a
  // per-wave LDS stage of the current 64-step (the digit histogram is free after the sort): every
  // lane gathers its own sorted point (one parallel gather per step), a run's first lane adds the
  // following staged points up to the next key break (independent LDS reads, no load chain), and
  // a run still open at the end of the step is carried into the next step by lane 0 -- past c1 if
  // it continues into the next wave's chunk.
  float4* stg = reinterpret_cast<float4*>(hist) + w * 64;  // NW*1 KB <= (NW+1)*NB*4 B
  bool carry_open = false;
  float4 carry = make_float4(0.f, 0.f, 0.f, 0.f);
  int carry_start = 0, carry_out = 0;
  // kStage: this wave's voxels are [pos0, pos0 + nh); those below fl have been stored.  Every
  // index below the frontier (the open carry's, else pos) is written after a step, and a step
  // writes indices <= frontier + 64, so the live ring entries span < 8 + 65 <= kEmitRing.
  float4* ost = reinterpret_cast<float4*>(hist) + NW * 64 + w * kEmitRing;
  const int pos0 = pos;
  int fl = pos0 & ~7;
  auto flush = [&](int fe) {  // store ring entries [fl, fe) (wave-uniform fe)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int b = fl; b < fe; b += 64) {
      const int idx = b + lane;
      if (idx < fe && idx >= pos0) out[idx] = ost[idx % kEmitRing];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    fl = fe;
  };
  // the gathers run one step ahead (the loop is otherwise one dependent HBM/L2 round trip per step)
  float4 pnext = c0 + lane < n && c0 < c1 ? in[vs[c0 + lane]] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i0 = c0; i0 < c1 || carry_open; i0 += 64) {
    const int i = i0 + lane;
    const bool valid = i < n;
    const uint32_t key = valid ? ks[i] : 0u;
    const bool brk_i = !valid || i == 0 || ks[i - 1] != key;  // a run starts here (or no point)
    const bool head = valid && i < c1 && brk_i;
    const bool cont = carry_open && lane == 0;  // continues the carried run (brk_i is false)
    const uint64_t brk = __ballot(brk_i), hb = __ballot(head);
    const float4 p = valid ? pnext : make_float4(0.f, 0.f, 0.f, 0.f);
    pnext = i + 64 < n ? in[vs[i + 64]] : make_float4(0.f, 0.f, 0.f, 0.f);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    stg[lane] = p;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint64_t after = lane == 63 ? 0ull : (brk >> (lane + 1)) << (lane + 1);
    const int nb = after ? __ffsll((unsigned long long)after) - 1 : 64;  // next break after this lane
    float4 c = p;
    if (cont) {
      c.x = carry.x + p.x;
      c.y = carry.y + p.y;
      c.z = carry.z + p.z;
      c.w = carry.w + p.w;
    }
    const bool starter = head || cont;
    if (starter)
      for (int k = lane + 1; k < nb; k += 4) {  // four staged reads in flight, adds in order
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = stg[min(k + u, 63)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (k + u < nb) {
            c.x += q[u].x;
            c.y += q[u].y;
            c.z += q[u].z;
            c.w += q[u].w;
          }
      }
    const bool spills = starter && nb == 64 && i0 + 64 < n && ks[i0 + 64] == key;
    const int start = cont ? carry_start : i;
    const int oidx = cont ? carry_out : pos + __popcll(hb & ((1ull << lane) - 1ull));
    if (starter && !spills) {
      const float cnt = (float)(i0 + nb - start);
      const float4 r = make_float4(c.x / cnt, c.y / cnt, c.z / cnt, c.w / cnt);
      if constexpr (kStage) ost[oidx % kEmitRing] = r;
      else out[oidx] = r;
    }
    const uint64_t sp = __ballot(spills);
    carry_open = sp != 0ull;
    if (carry_open) {
      const int src = __ffsll((unsigned long long)sp) - 1;
      carry = make_float4(__shfl(c.x, src), __shfl(c.y, src), __shfl(c.z, src), __shfl(c.w, src));
      carry_start = __shfl(start, src);
      carry_out = __shfl(oidx, src);
    }
    pos += __popcll(hb);
    if constexpr (kStage) {
      const int fe = (carry_open ? carry_out : pos) & ~7;
      if (fe > fl) flush(fe);
    }
  }
  if constexpr (kStage) flush(pos);
  return total;
}

template <int T, typename V, int MAXD, bool KV_LDS>
__device__ int vg_sort_emit(uint32_t* (&kb)[2], V* (&vb)[2], int n, int nbits, uint32_t* hist, uint32_t* wsum,
                            const float4* in, float4* out, int dbg, unsigned long long* t_sorted) {
  const int cur = vg_radix_sort<T, V, MAXD, KV_LDS>(kb, vb, n, nbits, hist, wsum, dbg);
  if (t_sorted && threadIdx.x == 0) *t_sorted = __builtin_amdgcn_s_memtime();
  if (dbg == 2) return 0;
  return vg_emit<T>(lds_if<KV_LDS>(kb[cur]), lds_if<KV_LDS>(vb[cur]), n, hist, wsum, in, out);
}

}  // namespace fbr
