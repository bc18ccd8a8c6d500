// k_voxel.hip — A9: pcl::VoxelGrid<PointXYZI>::filter as a segmented device kernel.
//
// Used for every down-sample on the path: the per-ring surf filter (featureExtraction.h:288-292,
// leaf odometrySurfLeafSize), downsampleCurrentScan (mapOptmization.h:981-993, leaves
// mappingCornerLeafSize / mappingSurfLeafSize) and the start-up map filter (:251-257).
// Semantics follow PCL 1.8 applyFilter: float min/max box, int64 overflow check (output = input),
// key = ijk0 + ijk1*div_x + ijk2*div_x*div_y with ijk = int(floor(p*inv_leaf) - float(min_b)),
// voxels emitted in ascending key order, centroid = float sum of x,y,z,intensity / count.
// PCL sorts (key, index) with the unstable std::sort, so the order of points inside one voxel —
// and hence the last bits of the centroid sum — is introsort-specific.  The kernels reproduce it
// (fbr_introsort.h) when fbr_params.exact_voxel_order = 1: std::sort's partition phase on (PCL key, index), then
// their stable radix sort of that sequence, which is std::sort's result; centroids are bit-exact.
// By default the partition phase is skipped (points summed in index order, centroids to float
// rounding, at about twice the exact mode's throughput).
//
// Morton mode (downsampleCurrentScan only): the same voxels and centroids, emitted in Morton order
// of (i,j,k) so that consecutive output points are spatially compact.  The order of the mapping
// DS clouds only fixes the summation order of AtA (accumulated in fp64, so immaterial); it makes
// every 64-query wave of the registration kernels touch a compact patch of the map grid.
//
// One 256-thread workgroup per segment.  The (key, index) pairs are sorted by an LSD radix sort
// (8-bit digits, only as many passes as the key range needs) whose ping-pong buffers live in a
// per-segment global scratch (L2-resident at these sizes); stability inside a 256-element tile
// comes from wave ballot peer masks.
//
// This unit holds the segmented kernels.  The grid, the sorts and the emit they share with the
// per-ring filters (k_voxel_ring.hip) are fbr_vg_sort.h; one large cloud on the whole device is
// k_voxel_large.hip.
#include "fbr_introsort.h"
#include "fbr_knobs.h"
#include "fbr_vg_sort.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>

namespace fbr {

// Generic front end: segments of a VgArgs (per-job mapping DS, start-up map filter, fbr_voxel_grid).
template <int T, typename V, bool LDS, bool kExact>
__global__ void __launch_bounds__(T) k_voxel_grid(VgArgs A) {
  constexpr int NW = T / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  int seg = blockIdx.x;
  const bool second = seg >= A.s[0].nseg;
  const VgSet S = second ? A.s[1] : A.s[0];
  if (second) seg -= A.s[0].nseg;
  uint32_t* hist = (uint32_t*)smem;  // [NW + 1][512]: per-wave digit counters + digit totals
  uint32_t* wsum = hist + (NW + 1) * 512;
  float* mm = (float*)(wsum + NW);
  int* misc = (int*)(mm + NW * 6);
  const int n = (int)min((int64_t)S.cnt_in[seg], S.cap);
  const float4* in = S.in + (int64_t)seg * S.stride_in;
  float4* out = S.out + (int64_t)seg * S.stride_out;
  if (n <= 0) {
    if (tid == 0) S.cnt_out[seg] = 0;
    return;
  }
  float mn[3], mx[3];
  vg_seg_bounds<T>(S, seg, n, in, mn, mx, mm);
  VgGrid G;
  G.init(mn, mx, S.leaf, S.morton != 0);
  if (G.overflow) {
    for (int i = tid; i < n; i += T) out[i] = in[i];
    if (tid == 0) S.cnt_out[seg] = n;
    return;
  }
  uint32_t* kb[2];
  V* vb[2];
  if constexpr (LDS) {
    unsigned char* q = smem + ((((unsigned char*)(misc + 4) - smem) + 15) & ~15);  // keeps the LDS address space
    const int cap = (int)S.cap;
    kb[0] = (uint32_t*)q;
    kb[1] = kb[0] + cap;
    vb[0] = (V*)(kb[1] + cap);
    vb[1] = vb[0] + cap;
  } else {
    uint32_t* sc = S.scratch + (int64_t)seg * kVgScratch * S.cap;
    kb[0] = sc;
    kb[1] = sc + S.cap;
    vb[0] = (V*)(sc + 2 * S.cap);
    vb[1] = (V*)(sc + 3 * S.cap);
  }
  for (int i = tid; i < n; i += T) {
    kb[0][i] = kExact ? G.pcl_key(in[i]) : G.key(in[i]);
    vb[0][i] = (V)i;
  }
  __syncthreads();
  if constexpr (kExact) {  // PCL's order inside a voxel: std::sort's partition phase, then the stable sort
    const int cap = (int)S.cap, nf = 3 * (cap / 17 + 2);
    if constexpr (LDS) {
      FBR_LDS_AS uint16_t* pl = (FBR_LDS_AS uint16_t*)kb[1];  // the free ping-pong half
      FBR_LDS_AS int* fr = (FBR_LDS_AS int*)hist;
      is_partition_phase<T>((FBR_LDS_AS uint32_t*)kb[0], (FBR_LDS_AS V*)vb[0], pl, pl + cap, n, fr, fr + nf, (int*)wsum);
    } else {
      int* fr = (int*)(S.scratch + (int64_t)seg * kVgScratch * S.cap + 4 * S.cap);
      is_partition_phase<T>(kb[0], vb[0], (int32_t*)kb[1], (int32_t*)vb[1], n, fr, fr + nf, (int*)wsum);
    }
    if (G.morton) {
      for (int i = tid; i < n; i += T) kb[0][i] = G.out_key(kb[0][i]);
      __syncthreads();
    }
  }
  const int total = vg_sort_emit<T, V, 9, LDS>(kb, vb, n, G.nbits, hist, wsum, in, out);
  if (tid == 0) S.cnt_out[seg] = total;
}

// Mapping-DS front end (downsampleCurrentScan, one 1024-thread workgroup per job cloud): segments
// of up to T * KPL points sort in place in LDS (keys u32 + u16 indices, vg_radix_sort_inplace), so
// the only global writes are the centroids; larger segments take the global-scratch ping-pong of
// k_voxel_grid.  Same semantics and output as k_voxel_grid.
#ifdef FBR_VG_STAMPS
// Diagnostic builds only: s_memtime at the phase boundaries of k_voxel_grid_ip's workgroup 0
// (start, grid set-up, keys, sort, emit), read by fbr_diag_vg_stamps.
__device__ unsigned long long fbr_vg_stamps[8];
#define FBR_VG_STAMP(k)                                                                       \
  do {                                                                                        \
    __syncthreads();                                                                          \
    if (blockIdx.x == 0 && threadIdx.x == 0) fbr_vg_stamps[k] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define FBR_VG_STAMP(k) \
  do {                  \
  } while (0)
#endif

template <int T, int KPL, bool kExact>
__global__ void __launch_bounds__(T) k_voxel_grid_ip(VgArgs A) {
  constexpr int NW = T / 64, LCAP = T * KPL;
  static_assert(NW * (64 + kEmitRing) * 16 <= (NW + 1) * 512 * 4, "vg_emit's point stage + centroid ring exceed hist");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  int seg = blockIdx.x;
  const bool second = seg >= A.s[0].nseg;
  const VgSet S = second ? A.s[1] : A.s[0];
  if (second) seg -= A.s[0].nseg;
  uint32_t* hist = (uint32_t*)smem;  // [NW + 1][512] (global path) / [NW + 1][256] (in place)
  uint32_t* wsum = hist + (NW + 1) * 512;
  float* mm = (float*)(wsum + NW);
  int* misc = (int*)(mm + NW * 6);
  FBR_VG_STAMP(0);
  const int n = (int)min((int64_t)S.cnt_in[seg], S.cap);
  const float4* in = S.in + (int64_t)seg * S.stride_in;
  float4* out = S.out + (int64_t)seg * S.stride_out;
  if (n <= 0) {
    if (tid == 0) S.cnt_out[seg] = 0;
    return;
  }
  float mn[3], mx[3];
  vg_seg_bounds<T>(S, seg, n, in, mn, mx, mm);
  VgGrid G;
  G.init(mn, mx, S.leaf, S.morton != 0);
  FBR_VG_STAMP(1);
  if (G.overflow) {
    for (int i = tid; i < n; i += T) out[i] = in[i];
    if (tid == 0) S.cnt_out[seg] = n;
    return;
  }
  int total;
  if (n <= LCAP) {
    unsigned char* q = smem + ((((unsigned char*)(misc + 4) - smem) + 15) & ~15);
    FBR_LDS_AS uint32_t* keys = (FBR_LDS_AS uint32_t*)q;
    FBR_LDS_AS uint16_t* vals = (FBR_LDS_AS uint16_t*)((FBR_LDS_AS uint32_t*)q + LCAP);
    for (int i = tid; i < n; i += T) {
      keys[i] = kExact ? G.pcl_key(in[i]) : G.key(in[i]);
      vals[i] = (uint16_t)i;
    }
    __syncthreads();
    if constexpr (kExact) {  // PCL's order inside a voxel: std::sort's partition phase, then the stable sort
      int32_t* sc = (int32_t*)(S.scratch + (int64_t)seg * kVgScratch * S.cap);  // positions (global)
      FBR_LDS_AS int* fr = (FBR_LDS_AS int*)hist;
      is_partition_phase<T>(keys, vals, sc, sc + S.cap, n, fr, fr + 3 * (LCAP / 17 + 2), (int*)wsum);
      if (G.morton) {
        for (int i = tid; i < n; i += T) keys[i] = G.out_key(keys[i]);
        __syncthreads();
      }
    }
    FBR_VG_STAMP(2);
    vg_radix_sort_inplace<T, KPL>(keys, vals, n, G.nbits, hist, wsum);
    FBR_VG_STAMP(3);
    total = vg_emit<T, true>(keys, vals, n, hist, wsum, in, out);  // hist: (NW + 1) * 2 KB
    FBR_VG_STAMP(4);
  } else {
    uint32_t* sc = S.scratch + (int64_t)seg * kVgScratch * S.cap;
    uint32_t* kb[2] = {sc, sc + S.cap};
    uint32_t* vb[2] = {sc + 2 * S.cap, sc + 3 * S.cap};
    for (int i = tid; i < n; i += T) {
      kb[0][i] = kExact ? G.pcl_key(in[i]) : G.key(in[i]);
      vb[0][i] = (uint32_t)i;
    }
    __syncthreads();
    if constexpr (kExact) {
      int* fr = (int*)(sc + 4 * S.cap);
      is_partition_phase<T>(kb[0], vb[0], (int32_t*)kb[1], (int32_t*)vb[1], n, fr, fr + 3 * ((int)S.cap / 17 + 2),
                            (int*)wsum);
      if (G.morton) {
        for (int i = tid; i < n; i += T) kb[0][i] = G.out_key(kb[0][i]);
        __syncthreads();
      }
    }
    total = vg_sort_emit<T, uint32_t, 9, false>(kb, vb, n, G.nbits, hist, wsum, in, out);
  }
  if (tid == 0) S.cnt_out[seg] = total;
}

// Few segments (single-scan calls: one corner and one surf cloud) leave all but two CUs idle in
// k_voxel_grid_ip.  Here P workgroups share a segment (block = seg * P + part): each computes the
// grid and a histogram of the keys' top bits over the whole cloud (the same in every part), keeps
// the points of its key range (the bins between the n * part / P and n * (part + 1) / P quantiles)
// in index order, sorts them in LDS and emits their voxels.  Equal keys share a bin, so every voxel
// lies in one part, and the parts' key ranges are ascending: part p's voxels go after the voxels of
// parts < p.  Each part publishes its voxel count as (gen << 32 | count) in flags[block], then reads
// the lower parts' counts (decoupled look-back: a lower block was dispatched earlier, so it runs to
// completion; the wait is bounded anyway, and gives up with a zero count rather than hang).  Same
// output as k_voxel_grid_ip (`test_split_voxel_grid_is_bit_identical`).  Default-order mode only.
template <int T, int KPL>
__global__ void __launch_bounds__(T) k_voxel_grid_split(VgArgs A, int P, unsigned long long* flags, unsigned gen) {
  constexpr int NW = T / 64, LCAP = T * KPL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int blk = blockIdx.x, part = blk % P;
  int seg = blk / P;
  const bool second = seg >= A.s[0].nseg;
  const VgSet S = second ? A.s[1] : A.s[0];
  if (second) seg -= A.s[0].nseg;
  uint32_t* hist = (uint32_t*)smem;  // [NW + 1][256] in-place sort counters; 1024 key bins before
  uint32_t* wsum = hist + (NW + 1) * 512;
  float* mm = (float*)(wsum + NW);
  int* misc = (int*)(mm + NW * 6);
  const int n = (int)min((int64_t)S.cnt_in[seg], S.cap);
  const float4* in = S.in + (int64_t)seg * S.stride_in;
  float4* out = S.out + (int64_t)seg * S.stride_out;
  if (n <= 0) {
    if (tid == 0 && part == 0) S.cnt_out[seg] = 0;
    return;
  }
  float mn[3], mx[3];
  vg_seg_bounds<T>(S, seg, n, in, mn, mx, mm);
  VgGrid G;
  G.init(mn, mx, S.leaf, S.morton != 0);
  if (G.overflow) {  // PCL's "leaf size too small": output = input
    if (part == 0) {
      for (int i = tid; i < n; i += T) out[i] = in[i];
      if (tid == 0) S.cnt_out[seg] = n;
    }
    return;
  }
  if (n > LCAP) {  // over the LDS capacity: part 0 alone, k_voxel_grid_ip's global-scratch path
    if (part != 0) return;
    uint32_t* sc = S.scratch + (int64_t)seg * kVgScratch * S.cap;
    uint32_t* kb[2] = {sc, sc + S.cap};
    uint32_t* vb[2] = {sc + 2 * S.cap, sc + 3 * S.cap};
    for (int i = tid; i < n; i += T) {
      kb[0][i] = G.key(in[i]);
      vb[0][i] = (uint32_t)i;
    }
    __syncthreads();
    const int total = vg_sort_emit<T, uint32_t, 9, false>(kb, vb, n, G.nbits, hist, wsum, in, out);
    if (tid == 0) S.cnt_out[seg] = total;
    return;
  }
  // ---- key histogram over the top hb bits (every part computes the same) ----
  const int hb = min(10, G.nbits), sh = G.nbits - hb, nbin = 1 << hb;
  for (int b = tid; b < nbin; b += T) hist[b] = 0u;
  __syncthreads();
  // wave w owns the contiguous chunk [c0, c1) of the cloud (at most KPL steps of 64: n <= LCAP)
  // and keeps its keys in registers for the compaction below (one read of the cloud)
  const int per = (((n + NW - 1) / NW) + 63) & ~63;
  const int c0 = min(n, w * per), c1 = min(n, c0 + per);
  uint32_t kv[KPL];
#pragma unroll
  for (int k = 0; k < KPL; ++k) {
    const int i = c0 + 64 * k + lane;
    kv[k] = 0u;
    if (i < c1) {
      kv[k] = G.key(in[i]);
      atomicAdd(&hist[kv[k] >> sh], 1u);
    }
  }
  __syncthreads();
  // this part's bin range [b0, b1): the first bins whose inclusive prefix exceeds n * part / P
  // and n * (part + 1) / P (inclusive scan over the bins, one bin per thread, T >= 1024)
  {
    const uint32_t c = tid < nbin ? hist[tid] : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(inc, off);
      if (lane >= off) inc += y;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t pre = 0;
    for (int k = 0; k < w; ++k) pre += wsum[k];
    inc += pre;  // inclusive prefix of bin tid
    const uint32_t lo = (uint32_t)(((int64_t)n * part) / P), hi = (uint32_t)(((int64_t)n * (part + 1)) / P);
    // bin tid starts the range of part q when inc(tid - 1) <= n q / P < inc(tid): the bins of
    // part q are those whose exclusive prefix lies in [n q / P, n (q + 1) / P) -- every bin lands in
    // exactly one part, in order
    const uint32_t ex = inc - c;
    const bool mine = tid < nbin && c > 0 && ex >= lo && (part == P - 1 || ex < hi);
    __syncthreads();
    if (tid == 0) { misc[0] = nbin; misc[1] = -1; }
    __syncthreads();
    if (mine) atomicMin(&misc[0], tid);
    if (mine) atomicMax(&misc[1], tid);
    __syncthreads();
  }
  const int b0 = misc[0], b1 = misc[1];  // empty range: b0 = nbin, b1 = -1
  // ---- this part's points in index order: every wave counts its chunk's points, one prefix over
  // the waves, then each wave writes its chunk in order (chunks are in index order): two barriers
  // (a block-wide pass per 1024 points took two per pass) ----
  unsigned char* q = smem + ((((unsigned char*)(misc + 4) - smem) + 15) & ~15);
  FBR_LDS_AS uint32_t* keys = (FBR_LDS_AS uint32_t*)q;
  FBR_LDS_AS uint16_t* vals = (FBR_LDS_AS uint16_t*)((FBR_LDS_AS uint32_t*)q + LCAP);
  const uint64_t lt = (1ull << lane) - 1ull;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < KPL; ++k) {
    const int i = c0 + 64 * k + lane;
    const int b = (int)(kv[k] >> sh);
    cnt += __popcll(__ballot(i < c1 && b >= b0 && b <= b1));
  }
  if (lane == 0) wsum[w] = (uint32_t)cnt;
  __syncthreads();
  int pre = 0, nk = 0;
  for (int k = 0; k < NW; ++k) {
    if (k < w) pre += (int)wsum[k];
    nk += (int)wsum[k];
  }
#pragma unroll
  for (int k = 0; k < KPL; ++k) {
    const int i = c0 + 64 * k + lane;
    const int b = (int)(kv[k] >> sh);
    const bool keep = i < c1 && b >= b0 && b <= b1;
    const uint64_t m = __ballot(keep);
    if (keep) {
      const int pos = pre + __popcll(m & lt);
      keys[pos] = kv[k];
      vals[pos] = (uint16_t)i;
    }
    pre += __popcll(m);
  }
  __syncthreads();
  if (nk > 0) vg_radix_sort_inplace<T, KPL>(keys, vals, nk, G.nbits, hist, wsum);
  // ---- voxel count, publish, look back ----
  int heads = 0;
  for (int i = tid; i < nk; i += T) heads += (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) heads += __shfl_xor(heads, off);
  __syncthreads();
  if (lane == 0) wsum[w] = (uint32_t)heads;
  __syncthreads();
  if (tid == 0) {
    uint32_t V = 0;
    for (int k = 0; k < NW; ++k) V += wsum[k];
    __hip_atomic_store(&flags[blk], ((unsigned long long)gen << 32) | V, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t off = 0;
    bool lost = false;
    for (int j = blk - part; j < blk; ++j) {
      unsigned long long f = 0;
      for (int spin = 0; spin < (1 << 24); ++spin) {
        f = __hip_atomic_load(&flags[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(f >> 32) == gen) break;
        __builtin_amdgcn_s_sleep(2);
      }
      if ((unsigned)(f >> 32) == gen) off += (uint32_t)f;
      else lost = true;
    }
    // a lower part never published (the wait is a safety bound, it does not happen when the lower
    // blocks run): the offsets are unknown, so the segment is reported failed, never short
    if (lost && A.err) atomicOr(&A.err[seg], kVgErrLookback);
    misc[2] = (int)off;
    misc[3] = (int)V;
    misc[1] = lost ? 1 : 0;
  }
  __syncthreads();
  const int off = misc[2], V = misc[3];
  const bool lost = misc[1] != 0;
  if (nk > 0 && !lost) vg_emit<T, true>(keys, vals, nk, hist, wsum, in, out + off);
  if (tid == 0 && part == P - 1) S.cnt_out[seg] = lost ? (A.err ? 0 : -1) : off + V;
}

size_t voxel_lds_bytes(const VgArgs& a, int threads, bool lds_mode) {
  const int nw = threads / 64;
  size_t b = sizeof(uint32_t) * ((size_t)(nw + 1) * 512 + nw) + sizeof(float) * nw * 6 + sizeof(int) * 4;
  b = (b + 15) & ~(size_t)15;
  if (lds_mode) {
    int64_t cap = 0;
    for (int k = 0; k < 2; ++k)
      if (a.s[k].nseg > 0) cap = std::max<int64_t>(cap, a.s[k].cap);
    b += (size_t)cap * 2 * (sizeof(uint32_t) + sizeof(uint16_t)) + 16;
  }
  return b;
}

// Size classes of a two-set launch (batch mapping DS).  The 1024 x 18 instance needs 146 KB of LDS,
// so a CU holds one workgroup of it and nothing else that uses LDS.  A set of small capacity (the
// corner clouds: at most kCornerPerRing picks per ring, and about a third of that in practice) gets
// its own launch of a 256-thread instance that sorts 256 * 16 = 4,096 points in 35 KB: four
// workgroups per CU.  Larger clouds of such a set take that instance's global-scratch branch.
// FBR_VG_CLASSES: 0 = one launch of the large instance for both sets, 1 = the small set's launch
// first (default), 2 = last.  (kVgIpKpl, kVgIpSmallT, kVgIpSmallKpl: fbr_vg_sort.h)
constexpr int64_t kVgIpSmallSetCap = 4 * kVgIpSmallT * kVgIpSmallKpl;
constexpr int kVgSplitSlots = 16;   // k_voxel_grid_split: segments x parts per launch
constexpr int kVgSplitRing = 1024;  // flag regions: a launch's own region (concurrent launches)
constexpr int kVgSplitMaxDevices = 64;

void launch_voxel_grid(hipStream_t s, const VgArgs& a) {
  const int nseg = a.s[0].nseg + a.s[1].nseg;
  if (nseg <= 0) return;
  int64_t cap = 0;
  for (int k = 0; k < 2; ++k)
    if (a.s[k].nseg > 0) cap = std::max<int64_t>(cap, a.s[k].cap);
  const bool exact = a.s[0].exact || a.s[1].exact;  // both sets share the context's mode
  // few segments (single-scan calls): P workgroups per segment (FBR_VG_SPLIT = P, default 8: C2 latency
  // -10 us against 4, profiles/r05w_latency_knob_sweep.txt; 1 off)
  const int P = knobs::vg_split();
  if (!exact && P > 1 && cap > kVgLdsCap && knobs::vg_inplace() && nseg * P <= kVgSplitSlots) {
    // look-back flags of the current device (agent-scope atomics must stay on the device that runs
    // the kernel: contexts on several GPUs in one process each get their own)
    static std::mutex mu;
    static unsigned long long* dev_flags[kVgSplitMaxDevices] = {};
    static bool dev_failed[kVgSplitMaxDevices] = {};
    int dev = -1;
    unsigned long long* flags = nullptr;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kVgSplitMaxDevices) {
      std::lock_guard<std::mutex> lk(mu);
      if (!dev_flags[dev] && !dev_failed[dev]) {
        unsigned long long* f = nullptr;
        const size_t bytes = sizeof(unsigned long long) * kVgSplitSlots * kVgSplitRing;
        if (hipMalloc(&f, bytes) == hipSuccess && hipMemset(f, 0, bytes) == hipSuccess) dev_flags[dev] = f;
        else dev_failed[dev] = true;  // the one-workgroup kernel below serves this device
      }
      flags = dev_flags[dev];
    }
    static std::atomic<unsigned> gen{0};
    if (flags) {
      const unsigned g = gen.fetch_add(1) + 1;  // never 0 (the zeroed flags)
      const size_t lds = voxel_lds_bytes(a, 1024, false) + (size_t)1024 * kVgIpKpl * (sizeof(uint32_t) + sizeof(uint16_t));
      fbr_launch((k_voxel_grid_split<1024, kVgIpKpl>), dim3(nseg * P), dim3(1024), lds, s, a, P,
                 flags + (size_t)(g % kVgSplitRing) * kVgSplitSlots, g);
      return;
    }
  }
  auto go = [&](auto ex) {
    constexpr bool E = decltype(ex)::value;
    if (cap <= kVgLdsCap) {
      fbr_launch((k_voxel_grid<256, uint16_t, true, E>), dim3(nseg), dim3(256), voxel_lds_bytes(a, 256, true), s, a);
    } else if (knobs::vg_inplace()) {
      constexpr size_t pair = sizeof(uint32_t) + sizeof(uint16_t);
      const size_t lds = voxel_lds_bytes(a, 1024, false) + (size_t)1024 * kVgIpKpl * pair;
      // Two sets (the mapping DS of a batch: surf and corner clouds), one of them of the small
      // class: one launch per set, the instance by the set's own capacity.  Sets of one class
      // share a launch (two launches of one instance only serialise them on the stream).
      const int cls = knobs::vg_classes();
      int small = -1;
      for (int k = 0; k < 2 && cls != 0; ++k)
        if (a.s[0].nseg > 0 && a.s[1].nseg > 0 && a.s[k].cap <= kVgIpSmallSetCap && a.s[k].cap < a.s[1 - k].cap) small = k;
      if (small < 0) {
        fbr_launch((k_voxel_grid_ip<1024, kVgIpKpl, E>), dim3(nseg), dim3(1024), lds, s, a);
        return;
      }
      const int first = cls == 1 ? small : 1 - small;
      for (int k : {first, 1 - first}) {
        VgArgs one{};
        one.s[0] = a.s[k];
        one.err = a.err;
        if (k == small)
          fbr_launch((k_voxel_grid_ip<kVgIpSmallT, kVgIpSmallKpl, E>), dim3(one.s[0].nseg), dim3(kVgIpSmallT),
                     voxel_lds_bytes(one, kVgIpSmallT, false) + (size_t)kVgIpSmallT * kVgIpSmallKpl * pair, s, one);
        else
          fbr_launch((k_voxel_grid_ip<1024, kVgIpKpl, E>), dim3(one.s[0].nseg), dim3(1024), lds, s, one);
      }
    } else {
      fbr_launch((k_voxel_grid<1024, uint32_t, false, E>), dim3(nseg), dim3(1024), voxel_lds_bytes(a, 1024, false),
                 s, a);
    }
  };
  if (exact) go(std::true_type{});
  else go(std::false_type{});
}

// Selftest of vg_radix_sort_inplace (fbr_selftest_radix_sort variants 3 .. 6, k_selftest.hip): one
// workgroup sorts one array.  It stands in this unit, not with the other selftests, because
// k_voxel_grid_ip's code depends on it: every other caller passes the sort a count it has bounded
// (0 < n <= T * KPL), and with those alone the compiler's interprocedural value propagation narrows
// n inside the sort before it is inlined (signed min / division become unsigned, loop guards fold)
// and all four k_voxel_grid_ip instances compile differently (1024 x 18: 5,230 -> 5,224
// instructions, 99 -> 101 VGPRs).  This caller's n is a kernel argument, which keeps the code
// that was measured.  kLeader: see vg_radix_sort_inplace.
template <int kLeader, int T = 1024, int KPL = kVgIpKpl>
__global__ void __launch_bounds__(T) k_selftest_radix_ip(uint32_t* keys, uint32_t* vals, int n, int nbits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = T / 64, LCAP = T * KPL;
  uint32_t* hist = (uint32_t*)smem;
  uint32_t* wsum = hist + (NW + 1) * 512;
  unsigned char* q = (unsigned char*)(wsum + NW);
  q = smem + (((q - smem) + 15) & ~15);
  FBR_LDS_AS uint32_t* k = (FBR_LDS_AS uint32_t*)q;
  FBR_LDS_AS uint16_t* v = (FBR_LDS_AS uint16_t*)((FBR_LDS_AS uint32_t*)q + LCAP);
  for (int i = threadIdx.x; i < n; i += T) {
    k[i] = keys[i];
    v[i] = (uint16_t)i;
  }
  __syncthreads();
  vg_radix_sort_inplace<T, KPL, kLeader>(k, v, n, nbits, hist, wsum);
  for (int i = threadIdx.x; i < n; i += T) {
    keys[i] = k[i];
    vals[i] = v[i];
  }
}

void launch_selftest_radix_ip(int variant, uint32_t* keys, uint32_t* vals, int n, int nbits) {
  auto lds = [](int T, int kpl) { return ((((size_t)(T / 64 + 1) * 512 + T / 64) * 4 + 15) & ~(size_t)15) + (size_t)T * kpl * 6; };
  const size_t big = lds(1024, kVgIpKpl);
  if (variant == 6)
    hipLaunchKernelGGL((k_selftest_radix_ip<0, kVgIpSmallT, kVgIpSmallKpl>), dim3(1), dim3(kVgIpSmallT),
                       lds(kVgIpSmallT, kVgIpSmallKpl), 0, keys, vals, n, nbits);
  else if (variant == 3) hipLaunchKernelGGL(k_selftest_radix_ip<0>, dim3(1), dim3(1024), big, 0, keys, vals, n, nbits);
  else if (variant == 4) hipLaunchKernelGGL(k_selftest_radix_ip<1>, dim3(1), dim3(1024), big, 0, keys, vals, n, nbits);
  else hipLaunchKernelGGL(k_selftest_radix_ip<2>, dim3(1), dim3(1024), big, 0, keys, vals, n, nbits);
}

}  // namespace fbr

#ifdef FBR_VG_STAMPS
extern "C" int fbr_diag_vg_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fbr::fbr_vg_stamps), sizeof(unsigned long long) * 8) == hipSuccess ? 0 : -1;
}
#endif
