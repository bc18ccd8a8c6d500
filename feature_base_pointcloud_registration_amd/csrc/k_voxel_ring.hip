// k_voxel_ring.hip — A9: the per-ring surf VoxelGrid (featureExtraction.h:288-292, leaf
// odometrySurfLeafSize), one workgroup per (job, ring).  Two kernels with the same output:
// k_voxel_ring (512 threads; also the exact-order instance) and k_voxel_ring_q (four waves per
// ring, default order).  Semantics, grid and sort: k_voxel.hip's header, fbr_vg_sort.h.
#include "fbr_introsort.h"
#include "fbr_vg_sort.h"

#include <type_traits>

namespace fbr {

// Per-ring front end (featureExtraction.h:279-292): the surf candidates of (job, ring) are the
// points k of the ring's non-empty segments [sp, ep] (sp < ep, :195-200) with cloudLabel[k] <= 0,
// in index order, read straight from the projected cloud and the label mask (the label of
// index 4 may be stale across scans exactly as the reference's cloudLabel[4]).  One register
// pass feeds min/max, the keys and the compaction; the sort runs in LDS (u16 ring offsets).
template <int T, int KPT, bool kExact>
__global__ void __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(KPT <= 4 && !kExact ? 8 : 1)))
k_voxel_ring(VgRing A) {
  constexpr int NW = T / 64, MAXD = 8;  // 8-bit digits: 3 passes cover the <= 24-bit ring keys
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int slot = blockIdx.x, job = slot / A.H;
#ifdef FBR_VR_STAMPS  // diagnostic build only (tools/vr_stamps.py): phase boundaries of wave 0
  unsigned long long ts[5] = {__builtin_amdgcn_s_memtime(), 0, 0, 0, 0};
#define VR_TS(i) (ts[i] = __builtin_amdgcn_s_memtime())
#define VR_TS_PTR (&ts[3])
#else
#define VR_TS(i) ((void)0)
#define VR_TS_PTR nullptr
#endif
  uint32_t* hist = (uint32_t*)smem;
  uint32_t* wsum = hist + (NW + 1) * (1 << MAXD);
  float* mm = (float*)(wsum + NW);
  int* cnts = (int*)(mm + NW * 6);  // [KPT][NW]
  const int s = A.start_ring[slot], e = A.end_ring[slot];
  float4* out = A.out + (int64_t)slot * A.stride_out;
  if (e <= s) {
    if (tid == 0) A.cnt_out[slot] = 0;
    return;
  }
  int sp6[6], ep6[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    sp6[j] = (s * (6 - j) + e * j) / 6;
    ep6[j] = (s * (5 - j) + e * (j + 1)) / 6 - 1;
  }
  const float4* CL = A.cloud + (int64_t)job * A.HW + s;
  const int8_t* LB = A.label + (int64_t)job * A.HW;
  // segment j is [sp_j, sp_{j+1} - 1] (ep_j = sp_{j+1} - 1, ep_5 = e - 1): when all six are
  // non-empty (sp < ep) they tile [s, e - 1]
  bool all6 = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) all6 = all6 && sp6[j] < ep6[j];
  bool cd[KPT];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  // Every label and point load issued before any is used (one round trip; clamped indices, and an
  // empty asm taking the values, or the compiler sinks each point load under its label test: a
  // chain of 2 * KPT dependent round trips).  The exact instance keeps its round-5 loads: the
  // hoisted form cost its partition phase's register allocation 25 % (voxel_ring 10.3 -> 12.8 ms per
  // B = 1024 step, profiles/r06y_voxel_ring_loads_ab.txt).
  int lbr[KPT];
  float4 pr[KPT];
  if constexpr (!kExact) {
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const int kc = min(s + r * T + tid, e - 1);
      lbr[r] = LB[kc];
      pr[r] = CL[kc - s];
    }
#pragma unroll
    for (int r = 0; r < KPT; ++r) asm volatile("" ::"v"(lbr[r]), "v"(pr[r].x), "v"(pr[r].y), "v"(pr[r].z));
  }
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int k = s + r * T + tid;
    bool in = false;
    if (all6) {
      in = k <= ep6[5];
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) in |= sp6[j] < ep6[j] && k >= sp6[j] && k <= ep6[j];
    }
    float4 p;
    if constexpr (kExact) {
      const int8_t lab = in ? LB[k] : (int8_t)1;
      p = in ? CL[k - s] : make_float4(0.f, 0.f, 0.f, 0.f);
      cd[r] = lab <= 0;
    } else {
      p = pr[r];
      cd[r] = in && lbr[r] <= 0;
    }
    if (cd[r]) {
      const float v[3] = {p.x, p.y, p.z};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        mn[d] = (v[d] < mn[d]) ? v[d] : mn[d];
        mx[d] = (mx[d] < v[d]) ? v[d] : mx[d];
      }
    }
  }
  // compaction positions in index order: per step r, waves in order
  uint64_t bal[KPT];
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    bal[r] = __ballot(cd[r]);
    if (lane == 0) cnts[r * NW + w] = __popcll(bal[r]);
  }
  vg_block_minmax<T>(mn, mx, mm);  // (its barrier also publishes cnts)
  int n = 0, pos[KPT];
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    int before = 0, all = 0;
    for (int ww = 0; ww < NW; ++ww) {
      const int c = cnts[r * NW + ww];
      before += ww < w ? c : 0;
      all += c;
    }
    pos[r] = n + before + __popcll(bal[r] & ((1ull << lane) - 1ull));
    n += all;
  }
  if (n == 0 || A.dbg == 3) {
    if (tid == 0) A.cnt_out[slot] = 0;
    return;
  }
  VR_TS(1);
  VgGrid G;
  G.init(mn, mx, A.leaf, false);
  unsigned char* q = smem + ((((unsigned char*)(cnts + KPT * NW) - smem) + 15) & ~15);  // keeps the LDS address space
  const int cap = (int)A.cap;
  uint32_t* kb[2];   // [0]: candidate keys in index order, then run keys; sort ping-pong
  uint16_t* vb[2];   // run ids; sort ping-pong
  kb[0] = (uint32_t*)q;
  kb[1] = kb[0] + cap;
  vb[0] = (uint16_t*)(kb[1] + cap);
  vb[1] = vb[0] + cap;
  uint16_t* off = vb[1] + cap;  // [cap] ring offset of the t-th candidate
  uint16_t* rst = off + cap;    // [cap + 1] first candidate of each run, rst[R] = n
  if (G.overflow) {  // output = input, in index order
#pragma unroll
    for (int r = 0; r < KPT; ++r)
      if (cd[r]) out[pos[r]] = CL[r * T + tid];
    if (tid == 0) A.cnt_out[slot] = n;
    return;
  }
#pragma unroll
  for (int r = 0; r < KPT; ++r)
    if (cd[r]) {
      kb[0][pos[r]] = G.key(CL[r * T + tid]);  // re-read (L2): no point registers live across the barrier
      off[pos[r]] = (uint16_t)(r * T + tid);   // offset from the ring start s
    }
  __syncthreads();
  if constexpr (kExact) {
    // PCL's order inside a voxel: std::sort's partition phase on (key, offset) (fbr_introsort.h);
    // everything below treats the permuted sequence as the input order, and its stable run sort
    // completes std::sort.  Scratch: the free ping-pong half kb[1] (positions, u16), the digit
    // histogram (frame lists) and wsum.. (the workgroup's scan slots).
    FBR_LDS_AS uint16_t* pl = (FBR_LDS_AS uint16_t*)kb[1];
    FBR_LDS_AS int* fr = (FBR_LDS_AS int*)hist;
    // frames above 512 points are partitioned by the whole workgroup (the top levels of a ring)
    is_partition_phase<T, FBR_LDS_AS uint32_t*, FBR_LDS_AS uint16_t*, FBR_LDS_AS uint16_t*, FBR_LDS_AS int*, 512>(
        (FBR_LDS_AS uint32_t*)kb[0], (FBR_LDS_AS uint16_t*)off, pl, pl + cap, n, fr, fr + 3 * (cap / 17 + 2), (int*)wsum);
  }
  VR_TS(2);
  // Runs of equal keys in index order (points adjacent along the ring share voxels: ~6.6
  // candidates per run on C2, and nearly one run per voxel).  Only the runs are sorted; the
  // stable sort keeps a voxel's runs in index order, so its points are still summed in index order.
  const int chunk = (((n + NW - 1) / NW) + 63) & ~63;
  const int c0 = min(n, w * chunk), c1 = min(n, c0 + chunk);
  uint32_t rkey[KPT];
  uint64_t hb[KPT];
  int nrun = 0;
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int t = c0 + 64 * k + lane;
    const bool valid = t < c1;
    const uint32_t key = valid ? kb[0][t] : 0u;
    hb[k] = __ballot(valid && (t == 0 || kb[0][t - 1] != key));
    rkey[k] = key;
    nrun += __popcll(hb[k]);
  }
  if (lane == 0) wsum[w] = (uint32_t)nrun;
  __syncthreads();  // every candidate key is read before the run keys overwrite them
  int rq = 0, R = 0;
  for (int ww = 0; ww < NW; ++ww) {
    const int cw = (int)wsum[ww];
    rq += ww < w ? cw : 0;
    R += cw;
  }
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    if ((hb[k] >> lane) & 1ull) {
      const int qq = rq + __popcll(hb[k] & ((1ull << lane) - 1ull));
      kb[0][qq] = rkey[k];
      vb[0][qq] = (uint16_t)qq;
      rst[qq] = (uint16_t)(c0 + 64 * k + lane);
    }
    rq += __popcll(hb[k]);
  }
  if (tid == 0) rst[R] = (uint16_t)n;
  __syncthreads();
  const int cur = vg_radix_sort<T, uint16_t, MAXD>(kb, vb, R, G.nbits, hist, wsum, A.dbg);
  VR_TS(3);
  if (A.dbg == 2) {
    if (tid == 0) A.cnt_out[slot] = 0;
    return;
  }
  // voxels = groups of equal keys in sorted run order: voxel index of each group's first run and
  // the next run of the same voxel, scattered by run id into the free ping-pong halves
  const FBR_LDS_AS uint32_t* ks = (const FBR_LDS_AS uint32_t*)kb[cur];
  const FBR_LDS_AS uint16_t* vs = (const FBR_LDS_AS uint16_t*)vb[cur];
  FBR_LDS_AS int32_t* nxt = (FBR_LDS_AS int32_t*)kb[cur ^ 1];
  FBR_LDS_AS uint16_t* vox = (FBR_LDS_AS uint16_t*)vb[cur ^ 1];
  const int rchunk = (((R + NW - 1) / NW) + 63) & ~63;
  const int r0 = min(R, w * rchunk), r1 = min(R, r0 + rchunk);
  int nh = 0;
  for (int i0 = r0; i0 < r1; i0 += 64) {
    const int i = i0 + lane;
    nh += __popcll(__ballot(i < r1 && (i == 0 || ks[i] != ks[i - 1])));
  }
  if (lane == 0) wsum[w] = (uint32_t)nh;
  __syncthreads();
  int vpos = 0, total = 0;
  for (int ww = 0; ww < NW; ++ww) {
    const int cw = (int)wsum[ww];
    vpos += ww < w ? cw : 0;
    total += cw;
  }
  for (int i0 = r0; i0 < r1; i0 += 64) {
    const int i = i0 + lane;
    const bool valid = i < r1;
    const uint32_t key = valid ? ks[i] : 0u;
    const bool head = valid && (i == 0 || ks[i - 1] != key);
    const uint64_t bh = __ballot(head);
    if (valid) {
      const int rid = vs[i];
      vox[rid] = head ? (uint16_t)(vpos + __popcll(bh & ((1ull << lane) - 1ull))) : (uint16_t)0xFFFFu;
      nxt[rid] = (i + 1 < R && ks[i + 1] == key) ? (int32_t)vs[i + 1] : -1;
    }
    vpos += __popcll(bh);
  }
  __syncthreads();
  // one lane per voxel (at its first run, in index order): the reference's serial float sum over
  // the voxel's points in index order, four loads in flight
  for (int rid = tid; rid < R; rid += T) {
    const int v = vox[rid];
    if (v == 0xFFFF) continue;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0;
    for (int qq = rid; qq >= 0; qq = nxt[qq]) {
      const int t0 = rst[qq], t1 = rst[qq + 1];
      for (int t = t0; t < t1; t += 4) {
        float4 pp[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pp[u] = CL[off[min(t + u, t1 - 1)]];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (t + u < t1) {
            if (cnt == 0) {
              c = pp[u];
            } else {
              c.x += pp[u].x;
              c.y += pp[u].y;
              c.z += pp[u].z;
              c.w += pp[u].w;
            }
            ++cnt;
          }
      }
    }
    const float fc = (float)cnt;
    out[v] = make_float4(c.x / fc, c.y / fc, c.z / fc, c.w / fc);
  }
  if (tid == 0) A.cnt_out[slot] = total;
#ifdef FBR_VR_STAMPS
  VR_TS(4);
  if (tid == 0 && A.stamps)
    for (int i = 0; i < 5; ++i) A.stamps[(int64_t)slot * 12 + i] = ts[i];
#endif
#undef VR_TS
#undef VR_TS_PTR
}

// ---- register helpers of the four-wave per-ring surf filter (k_voxel_ring_q below) ----
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t x, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)x, m), hi = __shfl_xor((uint32_t)(x >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}

// Ascending bitonic sort of 64 * E distinct u64 values held lane-major (element g = lane * E + e):
// compare-exchanges inside a lane for distances below E, xor lane exchanges above.  The values are
// below kF64KeyMax (a run key < 2^32 shifted by 16, or the padding kF64KeyMax), so the exchanges
// take their minima / maxima on the f64 unit (key_min / key_max, fbr_common.h).
template <int E>
__device__ __forceinline__ void wave_bitonic_u64(uint64_t (&v)[E], int lane) {
  constexpr int N = 64 * E;
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= E) {
        const int m = j / E;
        const bool lower = (lane & m) == 0;
        const bool asc = ((lane * E) & k) == 0;  // k > j >= E: the same for all e of the lane
        const bool take_min = lower == asc;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const uint64_t o = shfl_xor_u64(v[e], m);
          v[e] = take_min ? key_min(o, v[e]) : key_max(o, v[e]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (e & j) continue;
          const bool asc = ((lane * E + e) & k) == 0;
          const uint64_t a = v[e], b = v[e | j];
          const uint64_t lo = key_min(a, b), hi = key_max(a, b);
          v[e] = asc ? lo : hi;
          v[e | j] = asc ? hi : lo;
        }
      }
    }
  }
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// Sorted run ids sid[0, R) and voxel starts vst[0, V] (vst[V] = R) from the register-sorted values.
template <int E>
__device__ int vr_sort_runs(const uint32_t* kb, int R, uint16_t* sid, uint16_t* vst, int lane) {
  uint64_t v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int g = lane * E + e;
    v[e] = g < R ? (((uint64_t)kb[g] << 16) | (uint64_t)g) : kF64KeyMax;
  }
  wave_bitonic_u64<E>(v, lane);
  const uint32_t lo = __shfl_up((uint32_t)v[E - 1], 1), hi = __shfl_up((uint32_t)(v[E - 1] >> 32), 1);
  const uint64_t prev_last = ((uint64_t)hi << 32) | lo;
  bool hd[E];
  int nh = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int g = lane * E + e;
    const uint64_t pk = e ? (v[e - 1] >> 16) : (prev_last >> 16);
    hd[e] = g < R && (g == 0 || (v[e] >> 16) != pk);
    nh += hd[e] ? 1 : 0;
  }
  int inc = nh;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o);
    if (lane >= o) inc += y;
  }
  const int V = __shfl(inc, 63);
  int vi = inc - nh;
  wave_lds_sync();  // every lane read its kb values (sid overwrites them)
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int g = lane * E + e;
    if (g < R) sid[g] = (uint16_t)(v[e] & 0xFFFFull);
    if (hd[e]) vst[vi++] = (uint16_t)g;
  }
  if (lane == 0) vst[V] = (uint16_t)R;
  wave_lds_sync();
  return V;
}

// ---- the per-ring surf filter, four waves per ring (default order) ----
// The same filter as k_voxel_ring for the index-order sums with a ring's memory round trips cut to
// about three: each of the 4 waves loads a quarter of the ring's labels and points in one go (up
// to 8 steps of 64, kept in registers for the key pass: one load per point), the run keys and
// starts are compacted with workgroup prefixes, wave 0 sorts the (key << 16 | run id) values in
// registers (R <= 512; run ids are in index order, so equal keys keep it: the stable order; above,
// the four waves rank them by counting), and every thread sums about one voxel in index order.  A
// ring holds ~1.5k candidates in ~230 runs of equal keys (C2).  (Round 4 also measured one wave
// per ring: 2.3x fewer VALU instructions than the 512-thread kernel but ~14 dependent round trips
// per ring, slower overall; removed in round 5.)
// Occupancy (round 5): the ring's waves mostly wait on their few dependent memory round trips, so
// more rings per CU pay.  Pass A keeps only x, y, z of its points (80 -> 72 VGPRs: still 6-7 waves
// per SIMD, no change), and KQ = 8 is held to 64 VGPRs (8 waves per SIMD) at the cost of 44 B of
// spills: voxel_ring 1.37 -> 1.22 ms per B = 1024 step, 106.4k -> 109.3k scans/s interleaved
// (profiles/r05af_voxel_ring_occupancy_ab.txt).  KQ = 16 (rings of 2049-4096 points) keeps its own
// allocation (the compiler's choice for this attribute pair: 118 VGPRs, 28 B of spills).  The
// allocation is sensitive to the attribute's spelling: (8) on both instances or (8, 8) here gives
// 64 VGPRs; a separate kernel per KQ or (8, 8) with another maximum for KQ = 16 missed the target
// (69 VGPRs, 7 waves) on this compiler.
// PT = Pt3 (VgRing::c12, batch launches whose clouds carry no fourth word): both reads of a point
// fetch 12 B, and the emit and the overflow copy write the w = 0 that such a cloud's float4 holds
// (a sum of +0.0f over cnt >= 1 is +0.0f): the same bits out.
__device__ __forceinline__ float4 vr_f4(const float4& p) { return p; }
__device__ __forceinline__ float4 vr_f4(const Pt3& p) { return make_float4(p.x, p.y, p.z, 0.0f); }

template <int KQ, typename PT = float4>  // steps of 64 points per wave: 4 * 64 * KQ >= the ring capacity
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KQ <= 8 ? 8 : 1, KQ <= 8 ? 8 : 10)))
k_voxel_ring_q(VgRing A) {
  constexpr bool k12 = std::is_same<PT, Pt3>::value;
  constexpr int NW = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float mmx[NW][6];
  __shared__ int cntw[NW], runw[NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int slot = blockIdx.x, job = slot / A.H;
  const int s = A.start_ring[slot], e = A.end_ring[slot];
  float4* out = A.out + (int64_t)slot * A.stride_out;
  if (e <= s) {
    if (tid == 0) A.cnt_out[slot] = 0;
    return;
  }
  int sp6[6], ep6[6];
  bool all6 = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    sp6[j] = (s * (6 - j) + e * j) / 6;
    ep6[j] = (s * (5 - j) + e * (j + 1)) / 6 - 1;
    all6 = all6 && sp6[j] < ep6[j];
  }
  auto in_seg = [&](int k) {  // the non-empty segments [sp, ep] (:195-200), inside [s, e - 1]
    if (all6) return k <= ep6[5];
    bool in = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) in |= sp6[j] < ep6[j] && k >= sp6[j] && k <= ep6[j];
    return in;
  };
  const PT* CL = reinterpret_cast<const PT*>(A.cloud + (int64_t)job * A.HW) + s;
  const int8_t* LB = A.label + (int64_t)job * A.HW + s;
  const int len = min(e - s, (int)A.cap);
  const uint64_t lt = (1ull << lane) - 1ull;
  // ---- pass A: this wave's quarter [q0, q1) in one round of loads, kept in registers ----
  const int qlen = (((len + NW - 1) / NW) + 63) & ~63;
  const int q0 = min(len, w * qlen), q1 = min(len, q0 + qlen);
  // Every label and point load of the wave is issued before any is used: loads of a clamped index
  // (no branch), then an empty asm that takes all the values.  Without it the compiler sank each
  // point load under its label test, a chain of 2 * KQ dependent round trips per wave.
  PT pt[KQ];
  bool cd[KQ];
  int lb[KQ];
#pragma unroll
  for (int u = 0; u < KQ; ++u) {
    const int ic = min(q0 + 64 * u + lane, len - 1);
    lb[u] = LB[ic];
    pt[u] = CL[ic];
  }
#pragma unroll
  for (int u = 0; u < KQ; ++u) asm volatile("" ::"v"(lb[u]), "v"(pt[u].x), "v"(pt[u].y), "v"(pt[u].z));
#pragma unroll
  for (int u = 0; u < KQ; ++u) cd[u] = q0 + 64 * u + lane < q1 && lb[u] <= 0;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  int nw = 0;
#pragma unroll
  for (int u = 0; u < KQ; ++u) {
    cd[u] = cd[u] && in_seg(s + q0 + 64 * u + lane);
    if (cd[u]) {
      const float v[3] = {pt[u].x, pt[u].y, pt[u].z};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        mn[d] = (v[d] < mn[d]) ? v[d] : mn[d];
        mx[d] = (mx[d] < v[d]) ? v[d] : mx[d];
      }
    }
    nw += __popcll(__ballot(cd[u]));
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
    for (int o = 32; o > 0; o >>= 1) {
      const float a = __shfl_xor(mn[d], o), b = __shfl_xor(mx[d], o);
      mn[d] = (a < mn[d]) ? a : mn[d];
      mx[d] = (mx[d] < b) ? b : mx[d];
    }
  if (lane == 0) {
    for (int d = 0; d < 3; ++d) {
      mmx[w][d] = mn[d];
      mmx[w][3 + d] = mx[d];
    }
    cntw[w] = nw;
  }
  __syncthreads();
  int n = 0, base = 0;
#pragma unroll
  for (int ww = 0; ww < NW; ++ww) {
    base += ww < w ? cntw[ww] : 0;
    n += cntw[ww];
  }
  if (n == 0) {
    if (tid == 0) A.cnt_out[slot] = 0;
    return;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = mmx[0][d];
    mx[d] = mmx[0][3 + d];
#pragma unroll
    for (int ww = 1; ww < NW; ++ww) {
      mn[d] = (mmx[ww][d] < mn[d]) ? mmx[ww][d] : mn[d];
      mx[d] = (mx[d] < mmx[ww][3 + d]) ? mmx[ww][3 + d] : mx[d];
    }
  }
  VgGrid G;
  G.init(mn, mx, A.leaf, false);
  const int cap = (int)A.cap;
  uint32_t* kb = (uint32_t*)smem;             // [cap + 1] candidate keys, then run keys; then sid / vst (u16)
  uint16_t* off = (uint16_t*)(kb + cap + 1);  // [cap] ring offset of the t-th candidate
  uint16_t* rst = off + cap;                  // [cap + 1] first candidate of each run
  // ---- pass B: keys in index order (or, on PCL's overflow, the candidates themselves) ----
#pragma unroll
  for (int u = 0; u < KQ; ++u) {
    const uint64_t b = __ballot(cd[u]);
    const int pos = base + __popcll(b & lt);
    if (cd[u]) {
      if (G.overflow) {  // PCL: "Leaf size is too small" -> output = input, in index order
        out[pos] = vr_f4(CL[q0 + 64 * u + lane]);  // re-read: only x, y, z stay live from pass A
      } else {
        kb[pos] = G.key(vr_f4(pt[u]));
        off[pos] = (uint16_t)(q0 + 64 * u + lane);
      }
    }
    base += __popcll(b);
  }
  if (G.overflow) {
    if (tid == 0) A.cnt_out[slot] = n;
    return;
  }
  __syncthreads();
  // ---- pass C: run heads (keys read before the barrier, run keys written after it) ----
  const int tq = (((n + NW - 1) / NW) + 63) & ~63;
  const int t0w = min(n, w * tq), t1w = min(n, t0w + tq);
  constexpr int KR = KQ;  // n <= len: each wave's share of candidates fits KR steps as well
  uint32_t rk[KR];
  uint64_t hb[KR];
  int nr = 0;
#pragma unroll
  for (int u = 0; u < KR; ++u) {
    const int t = t0w + 64 * u + lane;
    const bool valid = t < t1w;
    const uint32_t key = valid ? kb[t] : 0u;
    const uint32_t prev = (valid && t > 0) ? kb[t - 1] : 0u;
    rk[u] = key;
    hb[u] = __ballot(valid && (t == 0 || key != prev));
    nr += __popcll(hb[u]);
  }
  if (lane == 0) runw[w] = nr;
  __syncthreads();
  int R = 0, rq = 0;
#pragma unroll
  for (int ww = 0; ww < NW; ++ww) {
    rq += ww < w ? runw[ww] : 0;
    R += runw[ww];
  }
#pragma unroll
  for (int u = 0; u < KR; ++u) {
    if ((hb[u] >> lane) & 1ull) {
      const int r = rq + __popcll(hb[u] & lt);
      kb[r] = rk[u];
      rst[r] = (uint16_t)(t0w + 64 * u + lane);
    }
    rq += __popcll(hb[u]);
  }
  if (tid == 0) rst[R] = (uint16_t)n;
  __syncthreads();
  // ---- sort the runs (stable by run id), voxel starts ----
  uint16_t* sid = (uint16_t*)kb;  // [R]
  uint16_t* vst = sid + cap + 1;  // [V + 1]
  __shared__ int vcount;
  if (R <= 512) {
    if (w == 0) {
      const int V = R <= 256 ? vr_sort_runs<4>(kb, R, sid, vst, lane) : vr_sort_runs<8>(kb, R, sid, vst, lane);
      if (lane == 0) vcount = V;
    }
  } else {
    // rank by counting over all 4 waves into the output slot, then wave 0 marks the voxels
    uint64_t* scr = reinterpret_cast<uint64_t*>(out);
    for (int r = tid; r < R; r += 256) {
      const uint32_t key = kb[r];
      int rank = 0;
      for (int j = 0; j < R; ++j) {
        const uint32_t kj = kb[j];
        rank += (kj < key || (kj == key && j < r)) ? 1 : 0;
      }
      scr[rank] = ((uint64_t)key << 16) | (uint64_t)r;
    }
    __syncthreads();  // (also orders the global scratch writes before the reads below)
    if (w == 0) {
      int V = 0;
      for (int g0 = 0; g0 < R; g0 += 64) {
        const int g = g0 + lane;
        const uint64_t x = g < R ? scr[g] : ~0ull;
        const uint64_t px = (g > 0 && g < R) ? scr[g - 1] : ~0ull;
        const bool hd = g < R && (g == 0 || (x >> 16) != (px >> 16));
        const uint64_t b = __ballot(hd);
        wave_lds_sync();
        if (g < R) sid[g] = (uint16_t)(x & 0xFFFFull);
        if (hd) vst[V + __popcll(b & lt)] = (uint16_t)g;
        V += __popcll(b);
      }
      if (lane == 0) {
        vst[V] = (uint16_t)R;
        vcount = V;
      }
    }
  }
  __syncthreads();  // (the scratch reads above precede the emit's stores to the same slot)
  const int V = vcount;
  // ---- one thread per voxel: the float sum of its points in index order (runs in id order) ----
  for (int vv = tid; vv < V; vv += 256) {
    const int g0 = vst[vv], g1 = vst[vv + 1];
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0;
    for (int g = g0; g < g1; ++g) {
      const int rid = sid[g];
      const int ta = rst[rid], tb = rst[rid + 1];
      for (int t = ta; t < tb; t += 8) {  // a run's points, 8 gathers in flight
        PT pp[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pp[u] = CL[off[min(t + u, tb - 1)]];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (t + u < tb) {
            if (cnt == 0) {
              c = vr_f4(pp[u]);
            } else {
              c.x += pp[u].x;
              c.y += pp[u].y;
              c.z += pp[u].z;
              if constexpr (!k12) c.w += pp[u].w;
            }
            ++cnt;
          }
      }
    }
    const float fc = (float)cnt;
    if constexpr (k12) out[vv] = make_float4(c.x / fc, c.y / fc, c.z / fc, 0.0f);
    else out[vv] = make_float4(c.x / fc, c.y / fc, c.z / fc, c.w / fc);
  }
  if (tid == 0) A.cnt_out[slot] = V;
}

// The per-ring filter of the default order: four waves per ring, except launches of at most 256
// rings (single scans), where the 512-thread kernel finishes a ring sooner (C2 single scan: 19.8 vs
// 34.3 us, profiles/r04u_latency_scan_timeline.txt) and the chip has room for the extra threads.
bool vr_four_waves(int nseg) { return nseg > 256; }

bool vr_takes_four_waves(const VgRing& a) {
  return !a.exact && (a.kernel < 0 ? vr_four_waves(a.B * a.H) : a.kernel == 2) && a.dbg == 0 && a.cap <= 4096;
}

size_t voxel_ring_lds_bytes(const VgRing& a, int threads, int kpt) {
  const int nw = threads / 64;
  size_t b = sizeof(uint32_t) * ((size_t)(nw + 1) * 256 + nw) + sizeof(float) * nw * 6 + sizeof(int) * kpt * nw;
  b = (b + 15) & ~(size_t)15;
  // keys / run ids ping-pong + candidate offsets + run starts
  return b + (size_t)a.cap * 2 * (sizeof(uint32_t) + sizeof(uint16_t)) + (size_t)(2 * a.cap + 1) * sizeof(uint16_t) + 16;
}

void launch_voxel_ring(hipStream_t s, const VgRing& a) {
  const int nseg = a.B * a.H;
  if (nseg <= 0) return;
  // 512 threads, KPT = ceil(W / 512) points per thread (instances up to W = 4096)
  const int kpt = (int)((a.cap + 511) / 512);
  auto go = [&](auto ex) {
    constexpr bool E = decltype(ex)::value;
    if (kpt <= 2)
      fbr_launch((k_voxel_ring<512, 2, E>), dim3(nseg), dim3(512), voxel_ring_lds_bytes(a, 512, 2), s, a);
    else if (kpt <= 4)
      fbr_launch((k_voxel_ring<512, 4, E>), dim3(nseg), dim3(512), voxel_ring_lds_bytes(a, 512, 4), s, a);
    else
      fbr_launch((k_voxel_ring<512, 8, E>), dim3(nseg), dim3(512), voxel_ring_lds_bytes(a, 512, 8), s, a);
  };
  if (a.exact) {
    go(std::true_type{});
  } else if (vr_takes_four_waves(a)) {
    const size_t lds = (((size_t)a.cap + 1) * 4 + (size_t)a.cap * 2 + ((size_t)a.cap + 1) * 2 + 15) & ~(size_t)15;
    if (a.c12) {
      if (a.cap <= 4 * 64 * 8) fbr_launch((k_voxel_ring_q<8, Pt3>), dim3(nseg), dim3(256), lds, s, a);
      else fbr_launch((k_voxel_ring_q<16, Pt3>), dim3(nseg), dim3(256), lds, s, a);
    } else {
      if (a.cap <= 4 * 64 * 8) fbr_launch(k_voxel_ring_q<8>, dim3(nseg), dim3(256), lds, s, a);
      else fbr_launch(k_voxel_ring_q<16>, dim3(nseg), dim3(256), lds, s, a);
    }
  } else {
    go(std::false_type{});
  }
}

}  // namespace fbr
