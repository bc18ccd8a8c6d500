// k_features.hip — A6-A8: calculateSmoothness, markOccludedPoints, extractFeatures per ring.
//
// Reference: /root/reference/src/featureExtraction.h:109-131 (curvature), :134-176 (occlusion and
// parallel-beam marks), :178-294 (6 segments per ring: std::sort, 20 corners, surf picks with
// +-5 neighbour suppression, surf candidates label <= 0).
//
// One wave (64 lanes) owns one (job, ring).  Rings are independent: every read or write of
// ring i stays inside [startRingIndex-12, endRingIndex+11), so the wave stages that window of the
// flattened arrays in LDS.  The only cross-ring object is the stale
// cloudSmoothness[4] slot (never recomputed, :113) and cloudNeighborPicked[0..4]; they live in
// StreamState and are carried only in stream mode.
//
// Every per-index flag (occlusion marks, column gaps > 10, cloudNeighborPicked, cloudLabel,
// curvature above/below the thresholds) is a bit in 64-bit words over the window, produced by wave
// ballots; marks and suppression become shifted ORs.
//   * curvature: the reference's left-to-right f32 sum, no FMA.
//   * occlusion: the sequential loop only ever writes 1s, so cloudNeighborPicked is the OR of the
//     marks covering each index: picked = C | OR_{d=0..5} A>>d | OR_{d=1..6} B<<d.
//   * sort: per segment, an LDS bitonic sort of (curvature bits, position) keys — std::sort's order
//     whenever the segment has no tied (or NaN) curvature; a segment with ties reproduces libstdc++'s
//     introsort partition phase wave-parallel and sorts its result stably (sort_tied), one with NaNs
//     runs the exact emulation (fbr_sort.h) on one lane.
//   * picks: the corner walk (descending, ep first, 20 per segment) and the surf walk (ascending,
//     ep last) are greedy: a candidate is taken iff no earlier-visited taken candidate suppresses
//     it.  Suppression reach (+-5 indices, stopped by a column gap > 10) depends only on
//     pointColInd and is symmetric, so the walk is a greedy independent set in visit-priority
//     order.  The wave resolves it in rounds on wave-uniform bitmasks: a candidate becomes "taken"
//     once every higher-priority conflicting candidate is "not taken", and "not taken" once one of
//     them is taken — final decisions, identical to the sequential walk.  The corner cap keeps the
//     first 20 taken in visit order.  The segment holding the stale slot keeps the sequential walk
//     (its stale index may duplicate a member).  Only candidates take part, so the rounds run over
//     a dense numbering of them ("compact walks" below): the corner walk over the list of its
//     candidates, the batch surf walk over the window re-based at its first frozen member.
// Outputs: label (the feature mask) and per-ring corner slots in visit order; the per-ring surf
// candidates (label <= 0, index order) are read from the mask by the per-ring VoxelGrid.
//
// The unit, top down (k_features at the end reads as this list):
//   carve                      FeatLds from fbr_feat_layout.h (LDS, the ring's scratch slot, region B)
//   flag_pass, picked_init     phase 2: the bit arrays and the window's curvature
//   per segment (make_seg):
//     stage_segment            the segment's curvature into LDS (or CurvPf's registers, prefetched)
//     cm_pass                  conflict masks by curvature comparison (cm_member): the direct path
//     walk_segment (wave 0):   sorted_order where the order is introsort's (stale slot, ties);
//                              stale_segment, or corner_walk (corner_compact / corner_generic),
//                              corner_visit_order, corner_cap, then surf_walk (surf_compact /
//                              surf_generic)
//   write_outputs
// The phases are __forceinline__ functions over explicit state (FeatLds, Ring, Seg, Walk, CurvPf).
// FeatLds, Ring and Seg are passed by value: of the forms measured that one kept every instance's
// registers and scratch at or below the single-body kernel's and its time (profiles/features_refactor.md).
#include "fbr_common.h"
#include "fbr_kernels.h"
#include "fbr_knobs.h"
#include "fbr_sort.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace fbr {

// Diagnostic builds (tools/feat_stamps.py, tools/feat_ablate.py); the shipped library has none.
#ifdef FBR_FEAT_STAMPS
constexpr bool kStamps = true;  // per-phase s_memtime cycle sums per ring into FeatArgs::stamps
#else
constexpr bool kStamps = false;
#endif
#ifdef FBR_FEAT_SKIP_STALE
constexpr bool kSkipStale = true;  // ablations: wrong results, only the kernel time is used
#else
constexpr bool kSkipStale = false;
#endif
#ifdef FBR_FEAT_SKIP_CM
constexpr bool kSkipCm = true;
#else
constexpr bool kSkipCm = false;
#endif
#ifdef FBR_FEAT_SKIP_CORNER
constexpr bool kSkipCorner = true;
#else
constexpr bool kSkipCorner = false;
#endif
#ifdef FBR_FEAT_SKIP_SURF
constexpr bool kSkipSurf = true;
#else
constexpr bool kSkipSurf = false;
#endif

struct Stamps {  // mark(i): the cycles since the previous mark into sum i
  unsigned long long acc[kStamps ? 12 : 1], last;
  __device__ __forceinline__ void start() {
    if constexpr (kStamps) {
      for (int i = 0; i < 12; ++i) acc[i] = 0;
      last = __builtin_amdgcn_s_memtime();
    }
  }
  __device__ __forceinline__ void mark(int i) {
    if constexpr (kStamps) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      acc[i] += t - last;
      last = t;
    }
  }
};

// Synchronisation of code that one wave runs on its own (the single-wave kernel, or wave 0 of the
// multi-wave kernel while the helper waves wait at the next workgroup barrier): a workgroup-scope
// fence (every earlier LDS / global access of the wave has completed) and a wave barrier (no code
// motion across it).  For a one-wave workgroup this is what __syncthreads amounts to.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

namespace {
using featlay::kWin;
using featlay::kWinBytes;
constexpr uint64_t kPadKey = kF64KeyMax;  // above every (curvature bits << 16 | position) key
constexpr int kSurfWindow = 64;  // batch surf walk: members resolved left of ep (FeatArgs::surf_full)
static_assert(sizeof(SortFrame) == featlay::kSortFrameBytes && kSortStack == featlay::kSortStackFrames &&
                  sizeof(SmoothEntry) == featlay::kEntryBytes && kCornerPerSeg == featlay::kCornersKept,
              "fbr_feat_layout.h sizes the sort stack, the entries and the taken-corner list");
}  // namespace

// Window bit-words (index i of the window <-> bit i&63 of word i>>6).
struct Bits {
  uint64_t* w;
  __device__ __forceinline__ bool get(int i) const { return (w[i >> 6] >> (i & 63)) & 1ull; }
  __device__ __forceinline__ void set_serial(int i) const { w[i >> 6] |= 1ull << (i & 63); }
};

struct FeatLds {
  int wlo, L, nw;
  float* gcurv;       // [Lcap] the ring window's curvature, in the ring's global scratch slot
  float* scurv;       // [segcap + 16] LDS copy of the current segment's [sp-6, ep+7) curvature
  int sbase;          // window index of scurv[0]
  Bits gap;           // |col[i+1]-col[i]| > 10
  Bits picked, labpos, labneg, edgec, surfc;
  Bits occa, occb, occc;
  uint32_t* cm;       // [segcap] conflict masks (corner_cm / surf_cm / apply_pick read the fields)
  unsigned char* rb;  // region B; its tenants are B's spans (rb_at)
  featlay::RegionB B;
  uint64_t* tmask;    // [WMAX] taken mask copy for the cap scan; word 15: the cm member list's length
  // sorted path (stale-slot segment, relevant ties): per-ring global scratch slot; its member order
  // and ranks are region B's sorder / rankc
  uint64_t* keys;     // [kseg]
  SmoothEntry* seg;   // [segcap] serial-path entries
  SmoothEntry* tmp;   // [segcap] materialisation scratch
  SortFrame* sstack;  // [kSortStack] introsort emulation stack (tie segments, lane 0)
};

template <typename T>
__device__ __forceinline__ T* rb_at(const FeatLds S, featlay::Span sp) {
  return (T*)(S.rb + sp.off);  // offset arithmetic: keeps the LDS address space (ds_*, not flat_*)
}

__host__ __device__ static inline featlay::Caps caps_of(const FeatArgs& a) { return {a.lcap, a.segcap, a.kseg, a.nwcap}; }

// The pointers of S from the layout (fbr_feat_layout.h): LDS from smem, the sorted path's buffers
// and the window's curvature from the ring's slot of FeatArgs::gscratch.
__device__ __forceinline__ void carve(FeatLds& S, const FeatArgs& a, unsigned char* smem, int slot) {
  const featlay::Lds l = featlay::lds_of(caps_of(a), 1);  // the offsets are the same for every wave count
  const featlay::Slot gs = featlay::slot_of(caps_of(a));
  S.scurv = (float*)(smem + l.scurv);
  uint64_t* words = (uint64_t*)(smem + l.bits);
  const int nwcap = a.nwcap;
  S.gap.w = words;
  S.picked.w = words + 1 * nwcap;
  S.labpos.w = words + 2 * nwcap;
  S.labneg.w = words + 3 * nwcap;
  S.edgec.w = words + 4 * nwcap;
  S.surfc.w = words + 5 * nwcap;
  S.occa.w = words + 6 * nwcap;
  S.occb.w = words + 7 * nwcap;
  S.occc.w = words + 8 * nwcap;
  S.tmask = (uint64_t*)(smem + l.tmask);
  S.sstack = (SortFrame*)(smem + l.sstack);
  S.cm = (uint32_t*)(smem + l.cm);
  S.rb = smem + l.rb;
  S.B = featlay::RegionB{a.segcap};
  unsigned char* g = a.gscratch + (int64_t)slot * a.gslot_bytes;
  S.keys = (uint64_t*)(g + gs.keys);
  S.seg = (SmoothEntry*)(g + gs.seg);
  S.tmp = (SmoothEntry*)(g + gs.tmp);
  S.gcurv = (float*)(g + gs.gcurv);
  S.sbase = 0;
}

// What every phase reads of its ring (wave-uniform).
struct Ring {
  int job, n, s, e;  // nvalid of the job, start / end ring index
  const float* R;    // the job's range, column and cloud arrays
  const int32_t* C;
  const float4* CL;
  StreamState* st;
  float4* corner_out;  // the ring's corner slots
};

// A segment's constants.
struct Seg {
  int j, sp, ep, m;  // segment index, first and last point (ep is never sorted), members u in [0, m]
  int li0;           // window index of member 0
  int slen;          // entries of S.scurv
  bool has_stale;    // holds the stale cloudSmoothness[4] slot: the sequential walks
  bool seg_full;     // the whole surf walk is observable
  int swin, lastj;   // batch surf window; the ring's last non-empty segment
};

// The walks' state of a segment.
struct Walk {
  bool direct;  // priorities from curvature comparisons (no tie so far), else the sorted path
  int nc_pre;   // corner candidates listed in region B's cand_list, -1: not listed
  int T;        // taken corners
  int ccode;    // path record of the corner walk
};

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }
// Bits [lo & 63, 63] / [0, hi & 63] of a word.
__device__ __forceinline__ uint64_t mask_from(int lo) { return ~0ull << (lo & 63); }
__device__ __forceinline__ uint64_t mask_upto(int hi) { return (hi & 63) == 63 ? ~0ull : ((1ull << ((hi & 63) + 1)) - 1ull); }

// 64 window bits [lo, lo+64) of a bit array; bits at negative window indices read as 1 (the
// suppression loops stop there) and bits past the array as 0.
__device__ __forceinline__ uint64_t bits64(const Bits& b, int lo, int nw) {
  const int w = lo >> 6, sh = lo & 63;  // arithmetic shift: floor for negative lo
  const uint64_t a = (w >= 0 && w < nw) ? b.w[w] : (w < 0 ? ~0ull : 0ull);
  const uint64_t c = (w + 1 >= 0 && w + 1 < nw) ? b.w[w + 1] : (w + 1 < 0 ? ~0ull : 0ull);
  return sh ? ((a >> sh) | (c << (64 - sh))) : a;
}

// Forward / backward suppression reach of window index li (<= 5 each): consecutive indices
// without a column gap > 10 (:230-240 / :262-274), from the gap bit words.
__device__ __forceinline__ int reach_fwd(const FeatLds S, int li) {
  const uint64_t x = bits64(S.gap, li, S.nw);      // bit d = gap at li+d
  return __builtin_ctzll(x | 0x20ull);              // zeros before the first gap, capped at 5
}
__device__ __forceinline__ int reach_bwd(const FeatLds S, int li) {
  const uint64_t x = bits64(S.gap, li - 64, S.nw);  // bit 63-d = gap at li-1-d
  return __builtin_clzll(x | (1ull << 58));        // capped at 5
}

// Bits [off, off+64) of the 192-bit value w0 | w1 << 64 | w2 << 128 (0 <= off < 128).
__device__ __forceinline__ uint64_t win64(uint64_t w0, uint64_t w1, uint64_t w2, int off) {
  if (off < 64) return off ? ((w0 >> off) | (w1 << (64 - off))) : w0;
  off -= 64;
  return off ? ((w1 >> off) | (w2 << (64 - off))) : w1;
}

// Mark cloudNeighborPicked over [li-bwd, li+fwd] (the suppression loops :227-240 / :259-274).
__device__ __forceinline__ void or_range(const Bits& b, int lo, int hi) {
  const int w0 = lo >> 6, w1 = hi >> 6;
  const uint64_t m0 = mask_from(lo), m1 = mask_upto(hi);
  if (w0 == w1) {
    atomicOr((unsigned long long*)&b.w[w0], (unsigned long long)(m0 & m1));
  } else {
    atomicOr((unsigned long long*)&b.w[w0], (unsigned long long)m0);
    atomicOr((unsigned long long*)&b.w[w1], (unsigned long long)m1);
  }
}

// S.cm[u] of member u: bits 0-9 the neighbours in reach that the corner walk visits before u (bit
// 5+d for d in [-5,-1], bit 4+d for d in [1,5]), bits 10-19 every neighbour in reach, bits 20-23 /
// 24-27 the forward / backward reach.  The surf walk visits in the reverse order.
__device__ __forceinline__ uint32_t corner_cm(const FeatLds S, int u) { return S.cm[u] & 1023u; }
__device__ __forceinline__ uint32_t surf_cm(const FeatLds S, int u) {
  const uint32_t c = S.cm[u];
  return ((c >> 10) & 1023u) & ~(c & 1023u);
}
// Member u is picked: its label bit (labpos / labneg) and cloudNeighborPicked over its reach.
__device__ __forceinline__ void apply_pick(const FeatLds S, const Bits& lab, const Seg g, int u) {
  const int li = g.sp + u - S.wlo;
  const uint32_t c = S.cm[u];
  atomicOr((unsigned long long*)&lab.w[li >> 6], 1ull << (li & 63));
  or_range(S.picked, li - (int)((c >> 24) & 15u), li + (int)((c >> 20) & 15u));
}

// cloudCurvature at window index li: the segment's LDS copy, or the global slot outside it (the
// stale cloudSmoothness[4] index may point anywhere in the ring window).
__device__ __forceinline__ float curv_at(const FeatLds S, int li, int slen) {
  const int k = li - S.sbase;
  return (k >= 0 && k < slen) ? S.scurv[k] : S.gcurv[li];
}
// Member u's curvature (inside the staged window).
__device__ __forceinline__ float member_curv(const FeatLds S, const Seg g, int u) {
  return S.scurv[g.sp + u - S.wlo - S.sbase];
}
// cloudSmoothness[pos] as the segment's sort meets it: position 4 holds the stale slot.
__device__ __forceinline__ SmoothEntry entry_at(const FeatLds S, const StreamState* st, int pos) {
  return (pos == 4) ? SmoothEntry{st->smooth4_value, st->smooth4_ind} : SmoothEntry{S.scurv[pos - S.wlo - S.sbase], pos};
}
__device__ __forceinline__ uint64_t sort_key(float v, int t) { return ((uint64_t)__float_as_uint(v) << 16) | (uint64_t)t; }

// A picked corner's point: the float4 record, or with FeatArgs::c12 (wave-uniform) the Pt3 record at
// the same index from the job's base and the w = 0 such a launch's float4 cloud would hold.
__device__ __forceinline__ float4 cloud_point(const float4* CL, int c12, int i) {
  if (c12) {
    const Pt3 p = reinterpret_cast<const Pt3*>(CL)[i];
    return make_float4(p.x, p.y, p.z, 0.0f);
  }
  return CL[i];
}

// cloudNeighborPicked of li and its reach, one bit at a time (index -1, col[-1], is scratch).
__device__ __forceinline__ void suppress_serial(const FeatLds S, int li) {
  S.picked.set_serial(li);
  const int f = reach_fwd(S, li), b = reach_bwd(S, li);
  for (int l = 1; l <= f; ++l) S.picked.set_serial(li + l);
  for (int l = 1; l <= b; ++l) S.picked.set_serial(li - l);
}

// Sequential walks (the reference loops verbatim) over S.seg[0..m] (seg[m] = the unsorted ep entry).
__device__ __forceinline__ void serial_walks(const FeatLds S, int slen, const SmoothEntry* ent, const FeatArgs& a, int job, int m,
                             const float4* CL, float4* corner_out, int& corner_cnt) {
  int largestPickedNum = 0;
  for (int k = m; k >= 0; k--) {  // corners, k = ep .. sp (:208-242)
    const int ind = ent[k].ind;
    const int li = ind - S.wlo;
    if (li < 0 || li + 5 >= S.L) { atomicOr(&a.err[job], 4); return; }
    if (!S.picked.get(li) && curv_at(S, li, slen) > a.edge_thr) {
      largestPickedNum++;
      if (largestPickedNum <= kCornerPerSeg) {
        S.labpos.set_serial(li);
        corner_out[corner_cnt++] = cloud_point(CL, a.c12, ind);
      } else {
        break;
      }
      suppress_serial(S, li);
    }
  }
  for (int k = 0; k <= m; k++) {  // surf, k = sp .. ep (:245-276)
    const int ind = ent[k].ind;
    const int li = ind - S.wlo;
    if (li < 0 || li + 5 >= S.L) { atomicOr(&a.err[job], 4); return; }
    if (!S.picked.get(li) && curv_at(S, li, slen) < a.surf_thr) {
      S.labneg.set_serial(li);
      suppress_serial(S, li);
    }
  }
}

// 10 neighbour bits of member (64*w + lane) from the wave-uniform masks of words w-1, w, w+1:
// bit 5+d for d in [-5,-1], bit 4+d for d in [1,5] (the cm encoding).
__device__ __forceinline__ uint32_t win10(uint64_t a, uint64_t b, uint64_t c, int lane) {
  const int start = 59 + lane;  // bit (64 + lane - 5) of the 192-bit concatenation a | b<<64 | c<<128
  uint64_t x;
  if (start < 64) {
    x = (a >> start) | (b << (64 - start));
  } else {
    const int s2 = start - 64;
    x = (b >> s2) | (s2 ? (c << (64 - s2)) : 0ull);
  }
  const uint32_t w11 = (uint32_t)(x & 0x7FFull);
  return (w11 & 0x1Fu) | ((w11 >> 6) << 5);
}

// Greedy rounds.  cmbits(u) = 10-bit mask of the higher-priority conflicting members of u.
// und: candidate members on entry; on exit tak = the members the sequential walk takes.
// frz (optional): frozen members -- candidates outside the resolved window, kept undecided: they
// block the members they outrank and are never decided themselves; the rounds then stop when a
// round decides nothing (members whose outcome depends on a frozen one stay in und).
template <int WMAX, typename CmF>
__device__ __forceinline__ void greedy_rounds(int m, int lane, uint64_t (&und)[WMAX], uint64_t (&tak)[WMAX], CmF cmbits,
                              const FeatArgs& a, int job, const uint64_t* frz = nullptr) {
  const int nwm = (m >> 6) + 1;
  uint32_t cmr[WMAX];
#pragma unroll
  for (int w = 0; w < WMAX; ++w) cmr[w] = (w < nwm && 64 * w + lane <= m) ? cmbits(64 * w + lane) : 0u;
  for (int round = 0;; ++round) {
    bool any = false, progress = false;
#pragma unroll
    for (int w = 0; w < WMAX; ++w) {
      const uint64_t live = frz ? und[w] & ~frz[w] : und[w];
      if (w < nwm && live != 0ull) {  // words whose candidates are all decided are skipped
        bool nt = false, tk = false;
        const bool mine = (live >> lane) & 1ull;
        if (mine) {
          const uint32_t wt = win10(w > 0 ? tak[w - 1] : 0ull, tak[w], w + 1 < WMAX ? tak[w + 1] : 0ull, lane);
          const uint32_t wu = win10(w > 0 ? und[w - 1] : 0ull, und[w], w + 1 < WMAX ? und[w + 1] : 0ull, lane);
          if (wt & cmr[w]) nt = true;
          else if (!(wu & cmr[w])) tk = true;
        }
        const uint64_t bt = __ballot(tk);
        tak[w] |= bt;
        // members suppressed by a member taken just now are decided in the same round (a
        // monotone-priority run then resolves 6 members per round instead of 3)
        if (bt != 0ull && mine && !tk && !nt) {
          const uint32_t wt = win10(w > 0 ? tak[w - 1] : 0ull, tak[w], w + 1 < WMAX ? tak[w + 1] : 0ull, lane);
          nt = (wt & cmr[w]) != 0u;
        }
        const uint64_t bn = __ballot(nt);
        und[w] &= ~(bt | bn);
        progress |= (bt | bn) != 0ull;
        any |= (frz ? und[w] & ~frz[w] : und[w]) != 0ull;
      }
    }
    if (!any || (frz && !progress)) break;
    if (round > 4 * (m + 2)) {  // unreachable: each round decides the best-ranked undecided
      if (lane == 0) atomicOr(&a.err[job], 8);
      break;
    }
  }
}

// ---- compact walks ----
// Only candidates ever enter und / tak, so the greedy independent set depends only on the
// conflicts among candidates: the rounds can run over any dense numbering of them.  A numbering
// that keeps member order keeps every conflict within +-5 positions, so a candidate's
// higher-priority conflicts are 11 bits placed at its position in a one- or two-word set, and a
// round is two ANDs against the wave-uniform tak / und words per candidate.
struct U128 {
  uint64_t lo, hi;
};

// rel (11 bits: bit 5 + k <-> position pos + k) placed in the 128-bit position set.
__device__ __forceinline__ U128 place11(uint32_t rel, int pos) {
  const int s = pos - 5;
  U128 r;
  if (s < 0) {
    r.lo = (uint64_t)(rel >> (-s));
    r.hi = 0ull;
  } else if (s < 64) {
    r.lo = (uint64_t)rel << s;
    r.hi = s > 53 ? (uint64_t)rel >> (64 - s) : 0ull;
  } else {
    r.lo = 0ull;
    r.hi = (uint64_t)rel << (s - 64);
  }
  return r;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// Bits of the segment members [64k, 64k + 64) (members above m cleared) from a per-lane copy of
// window bit words: lane l holds the word of window index li0 + 64 * l, sh = li0 & 63, li0 the
// window index of member 0.  Wave-uniform: a segment's flags without a ballot per 64 members.
__device__ __forceinline__ uint64_t member_bits(uint64_t wv, int sh, int k, int m) {
  const uint64_t lo = readlane64(wv, k), hi = readlane64(wv, k + 1);
  const uint64_t x = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
  const int rem = m - 64 * k;  // the chunk's last member
  return rem >= 63 ? x : (rem < 0 ? 0ull : x & ((2ull << rem) - 1ull));
}

// The members 64k + l of the set bits l of `set` appended to dst[cnt ..] in member order; returns
// the new count.
__device__ __forceinline__ int list_append(uint16_t* dst, int cnt, uint64_t set, int k, int lane) {
  if ((set >> lane) & 1ull) dst[cnt + __popcll(set & lanes_below(lane))] = (uint16_t)(64 * k + lane);
  return cnt + __popcll(set);
}

// A candidate within reach of ep (member u >= m - 4) that the window rounds left undecided.
__device__ __forceinline__ bool open_near_ep(int u, int m, uint64_t live, int lane) {
  return u >= m - 4 && u <= m && ((live >> lane) & 1ull);
}

// greedy_rounds' rule over NH position words: lane l owns positions l (cf[0]) and 64 + l (cf[1]).
// frz0: frozen positions of word 0 (they stay in und0 and block the positions they outrank); the
// rounds stop when nothing live is left or a round decides nothing.
template <int NH>
__device__ __forceinline__ void compact_rounds(int lane, uint64_t& und0, uint64_t& und1, uint64_t& tak0, uint64_t& tak1,
                                               const U128 (&cf)[NH], uint64_t frz0, int cap, const FeatArgs& a, int job) {
  for (int round = 0;; ++round) {
    bool progress = false;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const uint64_t live = h == 0 ? und0 & ~frz0 : und1;
      if (live != 0ull) {
        const bool mine = (live >> lane) & 1ull;
        const uint64_t clo = cf[h].lo, chi = NH > 1 ? cf[h].hi : 0ull;
        bool nt = false, tk = false;
        if (mine) {
          if (((tak0 & clo) | (tak1 & chi)) != 0ull) nt = true;
          else if (((und0 & clo) | (und1 & chi)) == 0ull) tk = true;
        }
        const uint64_t bt = __ballot(tk);
        if (h == 0) tak0 |= bt;
        else tak1 |= bt;
        // suppressed by a position taken just now: decided in the same round (as greedy_rounds)
        if (bt != 0ull && mine && !tk && !nt) nt = ((tak0 & clo) | (tak1 & chi)) != 0ull;
        const uint64_t bn = __ballot(nt);
        if (h == 0) und0 &= ~(bt | bn);
        else und1 &= ~(bt | bn);
        progress |= (bt | bn) != 0ull;
      }
    }
    if (((und0 & ~frz0) | und1) == 0ull || !progress) break;
    if (round > cap) {  // unreachable: each round decides the best-ranked live position or none
      if (lane == 0) atomicOr(&a.err[job], 8);
      break;
    }
  }
}

// libstdc++ 11 std::sort on a segment with tied curvatures, wave-parallel.  The final
// __insertion_sort / __unguarded_insertion_sort pass is stable, so std::sort's result is the
// stable sort of the array as the introsort partition phase leaves it.  That phase is reproduced
// exactly: __unguarded_partition(lo, hi, pivot) swaps the k-th element (from the left) that is
// not < pivot with the k-th element (from the right) that is not > pivot while the former lies
// left of the latter, and returns min(g_K, r_{K-1}) for the first k = K where that fails
// (swapped elements stop the scans).  Checked against std::sort on tie-heavy arrays
// (tests/test_oracle_pinning.py).  Depth exhaustion falls back to the serial heap sort.
__device__ __forceinline__ int wave_partition(SmoothEntry* a, int lo, int hi, float p, uint16_t* posL, uint16_t* posR,
                                              int lane) {
  int cntL = 0;
  for (int b = lo; b < hi; b += 64) {
    const int i = b + lane;
    const bool isL = i < hi && !(a[i].v < p);
    const uint64_t bl = __ballot(isL);
    if (isL) posL[cntL + __popcll(bl & lanes_below(lane))] = (uint16_t)i;
    cntL += __popcll(bl);
  }
  int cntR = 0;
  for (int t = hi - 1; t >= lo; t -= 64) {
    const int i = t - lane;
    const bool isR = i >= lo && !(p < a[i].v);
    const uint64_t br = __ballot(isR);
    if (isR) posR[cntR + __popcll(br & lanes_below(lane))] = (uint16_t)i;
    cntR += __popcll(br);
  }
  wsync();
  const int mn = min(cntL, cntR);
  int K1 = 0;  // swaps performed = number of k with g_k < r_k (a prefix of k)
  for (int k0 = 0; k0 < mn; k0 += 64) {
    const int k = k0 + lane;
    const uint64_t bo = __ballot(k < mn && posL[k] < posR[k]);
    K1 += __popcll(bo);
    if (bo != ~0ull) break;
  }
  for (int k = lane; k < K1; k += 64) {
    const int x = posL[k], y = posR[k];
    const SmoothEntry t = a[x];
    a[x] = a[y];
    a[y] = t;
  }
  int cut = K1 < cntL ? posL[K1] : INT_MAX;
  if (K1 > 0) cut = min(cut, posR[K1 - 1]);
  wsync();
  return min(cut, hi);
}

__device__ __forceinline__ void wave_introsort_partitions(SmoothEntry* a, int n, SortFrame* stack, uint16_t* posL,
                                                          uint16_t* posR, int lane) {
  int sp = 0;
  stack[sp++] = SortFrame{0, n, 2 * sm_lg(n)};  // every lane writes / reads the same frames
  while (sp > 0) {
    const SortFrame f = stack[--sp];
    int first = f.first, last = f.last, depth = f.depth;
    while (last - first > 16) {
      if (depth == 0) {  // std::partial_sort(first, last, last)
        if (lane == 0) sm_heap_sort(a, first, last);
        wsync();
        break;
      }
      --depth;
      const int mid = first + (last - first) / 2;
      if (lane == 0) sm_move_median_to_first(a, first, first + 1, mid, last - 1);
      wsync();
      const int cut = wave_partition(a, first + 1, last, a[first].v, posL, posR, lane);
      if (sp < kSortStack) stack[sp++] = SortFrame{cut, last, depth};
      last = cut;
    }
  }
  wsync();
}

// One compare-exchange stage of bitonic_sort_keys at register distance JR (element distance 64 * JR).
template <int KPL, int JR>
__device__ __forceinline__ void bitonic_register_step(uint64_t (&k)[KPL], int k2, int lane) {
#pragma unroll
  for (int r = 0; r < KPL; ++r) {
    if constexpr (JR < KPL) {
      if ((r & JR) == 0 && r + JR < KPL) {
        const int e = 64 * r + lane;
        const bool up = (e & k2) == 0;
        const uint64_t x = k[r], y = k[(r + JR) % KPL];
        const uint64_t mn = key_min(x, y), mx = key_max(x, y);
        k[r] = up ? mn : mx;
        k[(r + JR) % KPL] = up ? mx : mn;
      }
    }
  }
}

// Bitonic sort of kpow (power of two, <= 128 * QP) 64-bit keys held in registers: element
// e = 64 * r + lane sits in register r of its lane, so a compare-exchange at distance j2 < 64 is a
// lane shuffle and one at j2 >= 64 is between two registers of the same lane.  keys[] is read
// once and written once (it was a global-scratch network with a wave sync per stage).  The keys
// are below 2^48, so the exchanges run on the f64 unit (key_min / key_max, fbr_common.h).
template <int QP>
__device__ __forceinline__ void bitonic_sort_keys(uint64_t* keys, int kpow, int lane) {
  constexpr int KPL = 2 * QP;
  uint64_t k[KPL];
#pragma unroll
  for (int r = 0; r < KPL; ++r) k[r] = 64 * r + lane < kpow ? keys[64 * r + lane] : kPadKey;
  for (int k2 = 2; k2 <= kpow; k2 <<= 1) {
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      if (j2 >= 64) {  // register distance (a compile-time index per case)
        switch (j2 >> 6) {
          case 1: bitonic_register_step<KPL, 1>(k, k2, lane); break;
          case 2: bitonic_register_step<KPL, 2>(k, k2, lane); break;
          case 4: bitonic_register_step<KPL, 4>(k, k2, lane); break;
          case 8: bitonic_register_step<KPL, 8>(k, k2, lane); break;
          default: break;
        }
      } else {
        const bool lower = (lane & j2) == 0;
#pragma unroll
        for (int r = 0; r < KPL; ++r) {
          const int e = 64 * r + lane;
          const bool up = (e & k2) == 0;
          const uint64_t x = k[r];
          const uint32_t ylo = __shfl_xor((uint32_t)x, j2), yhi = __shfl_xor((uint32_t)(x >> 32), j2);
          const uint64_t y = ((uint64_t)yhi << 32) | ylo;
          const uint64_t mn = key_min(x, y), mx = key_max(x, y);
          k[r] = (lower == up) ? mn : mx;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < KPL; ++r)
    if (64 * r + lane < kpow) keys[64 * r + lane] = k[r];
  wsync();
}

// The stale-slot segment's walks (the reference loops of serial_walks) with the wave's lanes as
// the picked-word window: lane i holds picked word w_lo + i, so a test is one readlane of a
// wave-uniform word and a suppression range is one masked OR per lane.  Every entry's window
// index, candidate tests and suppression reach are computed lane-parallel first (info[k]); the
// walks then visit the entries in order on wave-uniform values, record the taken corners and
// write the picked / label words back.  Returns false (nothing written) when an entry lies
// outside the ring window or the window spans more than 64 words; the caller then runs
// serial_walks (which reports the error, as the reference's out-of-range access has no answer).
__device__ __forceinline__ bool stale_walks_fast(const FeatLds S, int slen, const SmoothEntry* ent, const FeatArgs& a, int m,
                                 const float4* CL, float4* corner_out, int& corner_cnt, uint32_t* info,
                                 int32_t* tlist, int lane) {
  int lo_li = INT_MAX, hi_li = INT_MIN;
  bool bad = false;
  for (int k0 = 0; k0 <= m; k0 += 64) {
    const int k = k0 + lane;
    if (k <= m) {
      const int li = ent[k].ind - S.wlo;
      uint32_t v = 0u;
      if (li >= 0 && li + 5 < S.L) {
        const float cv = curv_at(S, li, slen);
        const int f = reach_fwd(S, li), b = reach_bwd(S, li);
        v = (uint32_t)li | ((uint32_t)f << 16) | ((uint32_t)b << 19) | ((cv > a.edge_thr) ? 1u << 22 : 0u) |
            ((cv < a.surf_thr) ? 1u << 23 : 0u);
        lo_li = min(lo_li, li - b);
        hi_li = max(hi_li, li + f);
      } else {
        bad = true;
      }
      info[k] = v;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo_li = min(lo_li, __shfl_xor(lo_li, o));
    hi_li = max(hi_li, __shfl_xor(hi_li, o));
  }
  wsync();
  if (__any(bad) || lo_li < 0) return false;
  const int w_lo = lo_li >> 6;
  if ((hi_li >> 6) - w_lo >= 64) return false;
  const int myw = w_lo + lane;
  uint64_t pv = myw < S.nw ? S.picked.w[myw] : 0ull;
  auto is_picked = [&](int li) __attribute__((always_inline)) {
    return (readlane64(pv, (li >> 6) - w_lo) >> (li & 63)) & 1ull;
  };
  auto mark = [&](int lo, int hi) __attribute__((always_inline)) {  // picked over [lo, hi]
    const int w0 = (lo >> 6) - w_lo, w1 = (hi >> 6) - w_lo;
    uint64_t mm = (lane >= w0 && lane <= w1) ? ~0ull : 0ull;
    if (lane == w0) mm &= mask_from(lo);
    if (lane == w1) mm &= mask_upto(hi);
    pv |= mm;
  };
  // corners: k = ep .. sp (:208-242); the walks visit only the entries that pass the curvature
  // test (a ballot per 64 entries: the others are no-ops in the reference loops)
  int taken = 0;
  bool stop = false;
  for (int c0 = (m >> 6) << 6; c0 >= 0 && !stop; c0 -= 64) {
    const uint32_t vv = c0 + lane <= m ? info[c0 + lane] : 0u;
    uint64_t cand = __ballot((vv >> 22) & 1u);
    while (cand) {
      const int l = 63 - __builtin_clzll(cand);  // descending entries
      cand &= ~(1ull << l);
      const uint32_t v = __builtin_amdgcn_readlane(vv, l);
      const int li = (int)(v & 0xFFFFu);
      if (is_picked(li)) continue;
      if (++taken > kCornerPerSeg) {
        stop = true;
        break;
      }
      if (lane == 0) {
        tlist[taken - 1] = li + S.wlo;
        atomicOr((unsigned long long*)&S.labpos.w[li >> 6], 1ull << (li & 63));
      }
      mark(li - (int)((v >> 19) & 7u), li + (int)((v >> 16) & 7u));
    }
  }
  const int nc = min(taken, kCornerPerSeg);
  // surf: k = sp .. ep (:245-276); the picked-surf labels collect in the lanes' window words
  uint64_t lv = 0ull;
  for (int c0 = 0; c0 <= m; c0 += 64) {
    const uint32_t vv = c0 + lane <= m ? info[c0 + lane] : 0u;
    uint64_t cand = __ballot((vv >> 23) & 1u);
    while (cand) {
      const int l = __builtin_ctzll(cand);  // ascending entries
      cand &= cand - 1ull;
      const uint32_t v = __builtin_amdgcn_readlane(vv, l);
      const int li = (int)(v & 0xFFFFu);
      if (is_picked(li)) continue;
      lv |= lane == (li >> 6) - w_lo ? 1ull << (li & 63) : 0ull;
      mark(li - (int)((v >> 19) & 7u), li + (int)((v >> 16) & 7u));
    }
  }
  if (lv) atomicOr((unsigned long long*)&S.labneg.w[myw], (unsigned long long)lv);
  if (myw < S.nw) S.picked.w[myw] = pv;
  wsync();
  for (int t = lane; t < nc; t += 64) corner_out[corner_cnt + t] = cloud_point(CL, a.c12, tlist[t]);
  corner_cnt += nc;
  wsync();
  return true;
}

// ---- phase 2: occlusion marks, column gaps, curvature, threshold bits (chunk c = 64 indices) ----
// range / col are staged per group of 4 chunks: window [256g - 8, 256g + 264) in region B (a
// window per wave); with one wave the next group's window is loaded into registers while this
// group is processed, with several the waves take the groups in turn.
constexpr int kWq = (kWin + 63) / 64;
struct WinRegs {
  float r[kWq];
  int c[kWq];
};

__device__ __forceinline__ void load_window(const FeatLds S, const Ring rg, int c, const int lane, WinRegs& v) {
  const int wb = 64 * c - 8;
#pragma unroll
  for (int q = 0; q < kWq; ++q) {
    const int t = 64 * q + lane, idx = wb + t;
    const bool in = t < kWin && idx >= 0 && idx < S.L;
    v.r[q] = in ? rg.R[S.wlo + idx] : 0.0f;
    v.c[q] = in ? rg.C[S.wlo + idx] : 0;
  }
}

__device__ __forceinline__ void store_window(float* rw, int16_t* cw, const int lane, const WinRegs& v) {
#pragma unroll
  for (int q = 0; q < kWq; ++q) {
    const int t = 64 * q + lane;
    if (t < kWin) {
      rw[t] = v.r[q];
      cw[t] = (int16_t)v.c[q];
    }
  }
}

__device__ __forceinline__ void flag_chunk(const FeatLds S, const FeatArgs& a, const Ring rg, const float* rw,
                                           const int16_t* cw, int c, const int lane) {
  const int n = rg.n;
  const int i = 64 * c + lane;
  const int j = S.wlo + i;
  const int wo = 64 * (c & ~3) - 8;  // window origin of this chunk's group
  // Branch-free: every window read is in bounds (t in [8, 264), margins of 8), values past the
  // ring are masked by the conditions; the arithmetic is the reference's, in its order.
  const int t = i - wo;
  const float rm5 = rw[t - 5], rm4 = rw[t - 4], rm3 = rw[t - 3], rm2 = rw[t - 2], rm1 = rw[t - 1], r0 = rw[t];
  const float rp1 = rw[t + 1], rp2 = rw[t + 2], rp3 = rw[t + 3], rp4 = rw[t + 4], rp5 = rw[t + 5];
  const int c0 = cw[t], c1 = cw[t + 1];
  const bool inL = i < S.L, has1 = i + 1 < S.L;
  const int columnDiff = abs(c1 - c0);
  const bool gp = !(inL & has1) | (columnDiff > 10);
  const bool occ = inL & has1 & (j >= 5) & (j < n - 6) & (i >= 1);  // markOccludedPoints (:140-175)
  const bool near = columnDiff < 10;
  const bool a1 = (double)(r0 - rp1) > 0.3;  // depth1 - depth2
  const bool fa = occ & near & a1;
  const bool fb = occ & near & !a1 & ((double)(rp1 - r0) > 0.3);
  const float diff1 = fabsf(rm1 - r0), diff2 = fabsf(rp1 - r0);
  const bool fc = occ & ((double)diff1 > 0.02 * (double)r0) & ((double)diff2 > 0.02 * (double)r0);
  const bool smooth_ok = inL & (j >= 5) & (j < n - 5) & (i >= 5) & (i + 5 < S.L);  // calculateSmoothness (:113-122)
  const float d = rm5 + rm4 + rm3 + rm2 + rm1 - r0 * 10.0f + rp1 + rp2 + rp3 + rp4 + rp5;
  const float curv = smooth_ok ? d * d : 0.0f;
  if (inL) S.gcurv[i] = curv;  // indices outside [5, n-5) keep the zero-initialised scratch value
  const uint64_t ba = __ballot(fa), bb = __ballot(fb), bc = __ballot(fc), bg = __ballot(gp);
  const uint64_t be = __ballot(i < S.L && curv > a.edge_thr);
  const uint64_t bs = __ballot(i < S.L && curv < a.surf_thr);
  if (lane == 0) {
    S.occa.w[c] = ba;
    S.occb.w[c] = bb;
    S.occc.w[c] = bc;
    S.gap.w[c] = bg;
    S.edgec.w[c] = be;
    S.surfc.w[c] = bs;
  }
}

template <int NWV>
__device__ __forceinline__ void flag_pass(const FeatLds S, const FeatArgs& a, const Ring rg, const int lane, const int wv) {
  float* rw = rb_at<float>(S, S.B.win(wv));
  int16_t* cw = (int16_t*)(rw + kWin);
  WinRegs v;
  if constexpr (NWV == 1) {
    load_window(S, rg, 0, lane, v);
    for (int c = 0; c < S.nw; ++c) {
      if ((c & 3) == 0) {
        wsync();
        store_window(rw, cw, lane, v);
        wsync();
        if (c + 4 < S.nw) load_window(S, rg, c + 4, lane, v);
      }
      flag_chunk(S, a, rg, rw, cw, c, lane);
    }
  } else {
    const int G = (S.nw + 3) >> 2;  // groups of 4 chunks, dealt round-robin; uniform trip count
    for (int g0 = 0; g0 < G; g0 += NWV) {
      const int g = g0 + wv;
      if (g < G) {
        load_window(S, rg, 4 * g, lane, v);
        store_window(rw, cw, lane, v);
      }
      __syncthreads();
      if (g < G)
        for (int c = 4 * g; c < min(4 * g + 4, S.nw); ++c) flag_chunk(S, a, rg, rw, cw, c, lane);
      __syncthreads();
    }
  }
  __syncthreads();
}

// cloudNeighborPicked: reset over [5, n-5) (:124) then the marks; indices < 5 keep stream state
template <int NT>
__device__ __forceinline__ void picked_init(const FeatLds S, const StreamState* st, const int tid) {
  for (int c = tid; c < S.nw; c += NT) {
    const uint64_t A = S.occa.w[c], An = c + 1 < S.nw ? S.occa.w[c + 1] : 0ull;
    const uint64_t B = S.occb.w[c], Bp = c > 0 ? S.occb.w[c - 1] : 0ull;
    uint64_t mk = S.occc.w[c] | A;
#pragma unroll
    for (int d = 1; d <= 5; ++d) mk |= (A >> d) | (An << (64 - d));
#pragma unroll
    for (int d = 1; d <= 6; ++d) mk |= (B << d) | (Bp >> (64 - d));
    if (c == 0 && S.wlo == 0)
      for (int k = 0; k < 5 && k < S.L; ++k)
        if (st->picked04[k]) mk |= 1ull << k;
    S.picked.w[c] = mk;
  }
  __syncthreads();
}

// ---- extractFeatures (:188-285): the segments ----
__device__ __forceinline__ int seg_first(const Ring rg, int j) { return (rg.s * (6 - j) + rg.e * j) / 6; }
__device__ __forceinline__ int seg_last(const Ring rg, int j) { return (rg.s * (5 - j) + rg.e * (j + 1)) / 6 - 1; }

__device__ __forceinline__ Seg make_seg(const FeatLds S, const FeatArgs& a, const Ring rg, int j, int lastj) {
  Seg g;
  g.j = j;
  g.sp = seg_first(rg, j);
  g.ep = seg_last(rg, j);
  g.m = g.ep - g.sp;
  g.li0 = g.sp - S.wlo;
  g.slen = min(g.ep - S.wlo + 7, S.L) - max(g.li0 - 6, 0);
  g.has_stale = !kSkipStale && (g.sp <= 4 && 4 < g.ep);
  g.seg_full = a.surf_full || (a.carry && g.sp <= 9);
  g.swin = a.compact ? a.surf_win : kSurfWindow;
  g.lastj = lastj;
  return g;
}

// The next non-empty segment's curvature window is loaded into registers during this segment's
// surf walk and written to LDS after it (windows up to 64 * KCQ entries; longer ones, the first
// segment and the segment after a stale-slot one are staged on the spot).
template <int KCQ>
struct CurvPf {
  float v[KCQ];
  int seg = -1;   // the segment whose window S.scurv already holds
  int next = -1;  // the segment whose window v holds, len entries
  int len = 0;
};

template <int KCQ>
__device__ __forceinline__ void prefetch_curv(const FeatLds S, const FeatArgs& a, const Ring rg, int j0, const int lane,
                                              CurvPf<KCQ>& pf) {
  pf.next = -1;
  for (int jj = j0; jj < 6; ++jj) {
    const int psp = seg_first(rg, jj), pep = seg_last(rg, jj);
    if (psp >= pep) continue;
    const int pb = max(psp - S.wlo - 6, 0), pl = min(pep - S.wlo + 7, S.L) - pb;
    if (pl > 64 * KCQ || pep - psp + 1 > a.segcap) return;
#pragma unroll
    for (int q = 0; q < KCQ; ++q) pf.v[q] = S.gcurv[pb + min(64 * q + lane, pl - 1)];  // clamped: no branch
    pf.next = jj;
    pf.len = pl;
    return;
  }
}

template <int KCQ>
__device__ __forceinline__ void prefetch_commit(const FeatLds S, const int lane, CurvPf<KCQ>& pf) {
  pf.seg = pf.next;
  if (pf.seg >= 0) {
#pragma unroll
    for (int q = 0; q < KCQ; ++q)
      if (64 * q + lane < pf.len) S.scurv[64 * q + lane] = pf.v[q];
  }
}

// Stage the segment's curvature window [sp-6, ep+7) in LDS (members +-5 plus ep), unless the
// previous segment's walk prefetched it.
template <int NT>
__device__ __forceinline__ void stage_segment(FeatLds& S, const Seg g, bool staged, const int tid) {
  S.sbase = max(g.li0 - 6, 0);
  if (!staged)
    for (int t = tid; t < g.slen; t += NT) S.scurv[t] = S.gcurv[S.sbase + t];
  __syncthreads();
}

// Corner candidates (!picked && edgec) of the window words from member 0's on, lane l the l-th
// (member_bits turns them into member words).
template <int WMAX>
__device__ __forceinline__ uint64_t cand_words(const FeatLds S, const Seg g, const int lane) {
  const int w = (g.li0 >> 6) + lane;
  return (lane <= WMAX && w < S.nw) ? ~S.picked.w[w] & S.edgec.w[w] : 0ull;
}

// The members [umin, m] that are not picked and have the flag (edgec / surfc) as the candidates
// of the member-indexed rounds.
template <int WMAX>
__device__ __forceinline__ void member_candidates(const FeatLds S, const Seg g, const Bits& flag, int umin, const int lane,
                                                  uint64_t (&und)[WMAX], uint64_t (&tak)[WMAX]) {
#pragma unroll
  for (int w = 0; w < WMAX; ++w) {
    const int u = 64 * w + lane;
    bool cand = false;
    if (u <= g.m && u >= umin) {
      const int li = g.sp + u - S.wlo;
      cand = !S.picked.get(li) && flag.get(li);
    }
    und[w] = __ballot(cand);
    tak[w] = 0ull;
  }
}

// Conflict masks of member u from curvature comparisons (the direct path): returns whether a
// conflicting neighbour has the same curvature (its order would be introsort's).
__device__ __forceinline__ bool cm_member(const FeatLds S, const Seg g, int u) {
  const int m = g.m;
  const int li = g.sp - S.wlo + u;
  const int f = reach_fwd(S, li), b = reach_bwd(S, li);
  float cv[11];
#pragma unroll
  for (int d = 0; d < 11; ++d) cv[d] = S.scurv[max(li + d - 5, 0) - S.sbase];
  const float vu = cv[5];
  // neighbour bits (bit 4+d forward, 5-d backward) as ranges: forward d <= min(f, m-u),
  // backward d <= min(b, u); ep (member m) outranks every neighbour
  const int lf = min(f, m - u), lb = min(b, u);
  const uint32_t nbf = ((1u << lf) - 1u) << 5, nbb = ((1u << lb) - 1u) << (5 - lb);
  const uint32_t epb = (m - u >= 1 && m - u <= 5) ? 1u << (4 + m - u) : 0u;
  uint32_t gt = 0, eq = 0;
#pragma unroll
  for (int d = 1; d <= 5; ++d) {
    gt |= (cv[5 + d] > vu ? 1u : 0u) << (4 + d);
    eq |= (!(cv[5 + d] < vu || cv[5 + d] > vu) ? 1u : 0u) << (4 + d);  // equal or NaN
    gt |= (cv[5 - d] > vu ? 1u : 0u) << (5 - d);
    eq |= (!(cv[5 - d] < vu || cv[5 - d] > vu) ? 1u : 0u) << (5 - d);
  }
  const uint32_t notep = u != m ? ~0u : 0u;
  const uint32_t nb = nbf | nbb;
  const uint32_t hc = ((gt | epb) & nbf) | (gt & nbb & notep);
  S.cm[u] = hc | (nb << 10) | ((uint32_t)f << 20) | ((uint32_t)b << 24);
  return ((eq & ~epb & nbf) | (eq & nbb & notep)) != 0u;
}

// Visit priority.  The greedy walks depend only on the relative priority of conflicting
// neighbours, and the corner cap / output order only on the order of the taken corners, so
// without ties among those no sort is needed: priorities come from curvature comparisons
// (corner walk: ep first, then descending; surf walk: the reverse).  The stale-slot segment
// and segments with a relevant tie (their order is introsort's) take the sorted path.
// cm_pass sets w.direct and, on the direct path, every member's conflict mask -- all waves.
// Batch jobs need cm only for the corner candidates and the surf window [m - swin + 1, m] (none
// for the surf walk of the ring's last segment): those members are listed in region B (cm_list,
// with the corner candidates in cand_list for the compact corner walk) and only they are
// computed; the rest follow in the rare case the surf window falls back to the whole walk
// (surf_generic's rest).
template <int WMAX, int NWV>
__device__ __forceinline__ void cm_pass(const FeatLds S, const Seg g, Walk& w, const int tid, const int lane, const int wv,
                                        Stamps& tm) {
  constexpr int NT = 64 * NWV;
  w.direct = !g.has_stale;
  w.nc_pre = -1;
  if (!w.direct) return;
  if constexpr (kSkipCm) {
    for (int u = tid; u <= g.m; u += NT) S.cm[u] = 0u;
    __syncthreads();
  } else {
    const int m = g.m;
    const bool sparse = !g.seg_full;
    const uint16_t* list = rb_at<uint16_t>(S, S.B.cm_list());
    bool tf = false;
    int nlist = m + 1;
    if (sparse) {
      if (wv == 0) {
        int cnt = 0, ncand = 0;
        const int wlo_u = g.j == g.lastj ? m + 1 : max(0, m - (g.swin - 1));
        const uint64_t cwv = cand_words<WMAX>(S, g, lane);
        for (int k = 0; 64 * k <= m; ++k) {
          const uint64_t cb = member_bits(cwv, g.li0 & 63, k, m);
          const int lo = wlo_u - 64 * k;  // the surf window's members of this chunk
          const int rem = m - 64 * k;
          uint64_t wb = lo <= 0 ? ~0ull : (lo >= 64 ? 0ull : ~0ull << lo);
          if (rem < 63) wb &= (2ull << rem) - 1ull;
          cnt = list_append(rb_at<uint16_t>(S, S.B.cm_list()), cnt, cb | wb, k, lane);
          ncand = list_append(rb_at<uint16_t>(S, S.B.cand_list()), ncand, cb, k, lane);
        }
        w.nc_pre = ncand;
        if (lane == 0) S.tmask[featlay::kTmaskWords - 1] = (uint64_t)cnt;
      }
      if constexpr (NWV == 1) wsync();
      else __syncthreads();
      nlist = (int)S.tmask[featlay::kTmaskWords - 1];
    }
    for (int k0 = 64 * wv; k0 < nlist; k0 += NT) {
      if (sparse) {
        const int k = k0 + lane;
        if (k < nlist) tf |= cm_member(S, g, list[k]);
      } else {
        const int u = k0 + lane;
        if (u <= m) tf |= cm_member(S, g, u);
      }
    }
    if constexpr (NWV == 1) {
      w.direct = !__any(tf);
      wsync();
    } else {
      __syncthreads();
      w.direct = !__syncthreads_or(tf);
    }
    tm.mark(10);
  }
}

// std::sort's result on a segment with equal curvatures (their order is introsort's), in S.seg:
// the partition phase on an LDS copy in region B (part_copy, whose other tenants are dead here,
// with the partition positions as u16 in cm: no global round trip per partition step), then the
// stable sort of the partitioned array.  NaNs: the serial emulation on lane 0.
template <int QP>
__device__ __forceinline__ void sort_tied(const FeatLds S, const Ring rg, const Seg g, bool nan, int kpow, const int lane) {
  const int m = g.m;
  SmoothEntry* A = nan ? S.seg : rb_at<SmoothEntry>(S, S.B.part_copy());
  for (int t = lane; t < m; t += 64) A[t] = entry_at(S, rg.st, g.sp + t);
  wsync();
  if (nan) {
    if (lane == 0) std_sort_emul(S.seg, m, S.sstack);
    wsync();
  } else {
    wave_introsort_partitions(A, m, S.sstack, (uint16_t*)S.cm, (uint16_t*)S.cm + S.B.segcap, lane);
    for (int t = lane; t < kpow; t += 64) S.keys[t] = t < m ? sort_key(A[t].v, t) : kPadKey;
    wsync();
    bitonic_sort_keys<QP>(S.keys, kpow, lane);  // stable sort of the partitioned array
    for (int k = lane; k < m; k += 64) S.seg[k] = A[S.keys[k] & 0xFFFFu];
    wsync();
  }
}

// The sorted path's conflict masks: members u in [0, m] (index sp+u) get their sorted position
// (sorder), corner visit rank (rankc) and cm from rank comparisons.
__device__ __forceinline__ void cm_from_ranks(const FeatLds S, const Seg g, bool tie, const int lane) {
  const int m = g.m, sp = g.sp;
  uint16_t* sorder = rb_at<uint16_t>(S, S.B.sorder());  // member index at each sorted position
  uint16_t* rankc = rb_at<uint16_t>(S, S.B.rankc());    // corner visit rank of each member
  for (int k = lane; k <= m; k += 64) {
    const int u = (k == m) ? m : (tie ? S.seg[k].ind - sp : (int)(S.keys[k] & 0xFFFFu));
    sorder[k] = (uint16_t)u;
    rankc[u] = (uint16_t)(k == m ? 0 : m - k);  // corner visit order: ep, then descending
  }
  wsync();
  for (int u = lane; u <= m; u += 64) {
    const int li = sp + u - S.wlo;
    const int f = reach_fwd(S, li), b = reach_bwd(S, li);
    const int ru = rankc[u];
    uint32_t nb = 0, hc = 0;
    int rn[10];
#pragma unroll
    for (int d = 1; d <= 5; ++d) {  // independent LDS reads, then the masks
      rn[4 + d] = (d <= f && u + d <= m) ? (int)rankc[u + d] : INT_MAX;
      rn[5 - d] = (d <= b && u - d >= 0) ? (int)rankc[u - d] : INT_MAX;
    }
#pragma unroll
    for (int d = 1; d <= 5; ++d) {
      if (d <= f && u + d <= m) nb |= 1u << (4 + d);
      if (d <= b && u - d >= 0) nb |= 1u << (5 - d);
      if (rn[4 + d] < ru) hc |= 1u << (4 + d);
      if (rn[5 - d] < ru) hc |= 1u << (5 - d);
    }
    S.cm[u] = hc | (nb << 10) | ((uint32_t)f << 20) | ((uint32_t)b << 24);
  }
  wsync();
}

// The sorted path: [sp, ep) by (curvature bits, position), std::sort's order.  The stale-slot
// segment gets its entries in S.seg (and hands the next scan its stale slot); the others their
// order, ranks and conflict masks.  Region B's candidate list does not survive it.
template <int QP>
__device__ __forceinline__ void sorted_order(const FeatLds S, const Ring rg, const Seg g, Walk& w, const int lane, Stamps& tm) {
  const int m = g.m, sp = g.sp;
  StreamState* st = rg.st;
  w.nc_pre = -1;
  int kpow = 1;
  while (kpow < m) kpow <<= 1;
  for (int t = lane; t < kpow; t += 64) S.keys[t] = t < m ? sort_key(entry_at(S, st, sp + t).v, t) : kPadKey;
  wsync();
  bitonic_sort_keys<QP>(S.keys, kpow, lane);
  bool tflag = false, nflag = false;
  for (int t = lane; t < m; t += 64) {
    const uint32_t vb = (uint32_t)(S.keys[t] >> 16);
    nflag |= vb > 0x7f800000u;  // NaN
    if (t + 1 < m) tflag |= (uint32_t)(S.keys[t + 1] >> 16) == vb;
  }
  const bool nan = __any(nflag);
  const bool tie = __any(tflag) || nan;
  tm.mark(2);
  if (tie) {
    sort_tied<QP>(S, rg, g, nan, kpow, lane);
  } else if (g.has_stale) {
    for (int k = lane; k < m; k += 64) S.seg[k] = entry_at(S, st, sp + (int)(S.keys[k] & 0xFFFFu));
    wsync();
  }
  if (g.has_stale) {
    if (lane == 0) {
      S.seg[m] = SmoothEntry{S.scurv[g.ep - S.wlo - S.sbase], g.ep};  // cloudSmoothness[ep] is never sorted (:203)
      st->smooth4_value = S.seg[4 - sp].v;            // the entry left at position 4 is the next
      st->smooth4_ind = S.seg[4 - sp].ind;            // scan's stale slot
    }
    wsync();
  } else {
    cm_from_ranks(S, g, tie, lane);
  }
}

// The stale-slot segment: the walk's entries in LDS (region B's stale_ent, free here).  cm is
// unused on this path: it holds the entries' walk info.
__device__ __forceinline__ void stale_segment(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, int& corner_cnt,
                                              const int lane) {
  SmoothEntry* ent = rb_at<SmoothEntry>(S, S.B.stale_ent());
  for (int k = lane; k <= g.m; k += 64) ent[k] = S.seg[k];
  wsync();
  if (!stale_walks_fast(S, g.slen, ent, a, g.m, rg.CL, rg.corner_out, corner_cnt, S.cm,
                        rb_at<int32_t>(S, S.B.stale_tlist()), lane)) {
    if (lane == 0) serial_walks(S, g.slen, ent, a, rg.job, g.m, rg.CL, rg.corner_out, corner_cnt);
    corner_cnt = __shfl(corner_cnt, 0);
    wsync();
  }
}

// -- corner walk --
// Both forms leave the taken corners (member order) in tlu / tlv on the direct path, and their
// member mask in S.tmask on the sorted one (whose cap scan walks the sorted order).
__device__ __forceinline__ void take_corner(const FeatLds S, const Seg g, int q, int u) {
  rb_at<uint16_t>(S, S.B.tlu())[q] = (uint16_t)u;
  rb_at<float>(S, S.B.tlv())[q] = member_curv(S, g, u);
}

// The compact rounds over nc <= 64 * NH listed candidates, list position q on lane q & 63.  The
// 10-bit mask of a candidate's higher-priority conflicting members becomes 11 bits over list
// positions: a conflicting candidate d <= 5 members away is one of the <= 5 next list entries.
template <int WMAX, int NH>
__device__ __forceinline__ void corner_compact_rounds(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, Walk& w,
                                                      int nc, const int lane) {
  const uint16_t* cl = rb_at<uint16_t>(S, S.B.cand_list());
  U128 cf[NH];
  int uu[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const int q = 64 * h + lane;
    uint32_t rel = 0u;
    int u = 0;
    if (q < nc) {
      u = cl[q];
      const uint32_t c10 = corner_cm(S, u);
      int un[10];
#pragma unroll
      for (int k = 1; k <= 5; ++k) {  // independent LDS reads, then the masks
        un[4 + k] = cl[min(q + k, nc - 1)];
        un[5 - k] = cl[max(q - k, 0)];
      }
#pragma unroll
      for (int k = 1; k <= 5; ++k) {
        const int df = min(un[4 + k] - u, 6), db = min(u - un[5 - k], 6);
        if (q + k < nc && df <= 5 && ((c10 >> (4 + df)) & 1u)) rel |= 1u << (5 + k);
        if (q - k >= 0 && db <= 5 && ((c10 >> (5 - min(db, 5))) & 1u)) rel |= 1u << (5 - k);
      }
    }
    uu[h] = u;
    cf[h] = place11(rel, q);
  }
  uint64_t und0 = nc >= 64 ? ~0ull : (1ull << nc) - 1ull;
  uint64_t und1 = NH > 1 ? (nc >= 128 ? ~0ull : (1ull << (nc - 64)) - 1ull) : 0ull;
  uint64_t tak0 = 0ull, tak1 = 0ull;
  if constexpr (!kSkipCorner) compact_rounds<NH>(lane, und0, und1, tak0, tak1, cf, 0ull, 4 * (nc + 2), a, rg.job);
  w.T = __popcll(tak0) + __popcll(tak1);
  if (!w.direct) {
    if (lane < WMAX) S.tmask[lane] = 0ull;
    wsync();
  }
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const uint64_t th = h == 0 ? tak0 : tak1;
    if ((th >> lane) & 1ull) {
      const int u = uu[h];
      if (w.direct) take_corner(S, g, (h == 0 ? 0 : __popcll(tak0)) + __popcll(th & lanes_below(lane)), u);
      else atomicOr((unsigned long long*)&S.tmask[u >> 6], 1ull << (u & 63));
    }
  }
  wsync();
}

// Compact form: the candidates are listed in member order (region B's cand_list; tlu takes its
// place afterwards).  More than 128 candidates: returns false, the member-indexed rounds run.
template <int WMAX>
__device__ __forceinline__ bool corner_compact(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, Walk& w,
                                               const int lane) {
  int nc = w.nc_pre;
  if (nc < 0) {
    nc = 0;
    const uint64_t cwv = cand_words<WMAX>(S, g, lane);
    for (int k = 0; 64 * k <= g.m; ++k)
      nc = list_append(rb_at<uint16_t>(S, S.B.cand_list()), nc, member_bits(cwv, g.li0 & 63, k, g.m), k, lane);
  }
  if (nc > 128) return false;
  w.T = 0;
  w.ccode = nc > 64 ? 1 : 0;
  if (nc == 0 && w.direct) return true;
  wsync();
  if (nc <= 64) corner_compact_rounds<WMAX, 1>(S, a, rg, g, w, nc, lane);
  else corner_compact_rounds<WMAX, 2>(S, a, rg, g, w, nc, lane);
  return true;
}

// Member-indexed form (more than 128 candidates, or FBR_FEAT_COMPACT=0).
template <int WMAX>
__device__ __forceinline__ void corner_generic(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, Walk& w,
                                               const int lane) {
  uint64_t und[WMAX], tak[WMAX];
  member_candidates<WMAX>(S, g, S.edgec, 0, lane, und, tak);
  if constexpr (!kSkipCorner) greedy_rounds(g.m, lane, und, tak, [&](int u) { return corner_cm(S, u); }, a, rg.job);
  w.T = 0;
  w.ccode = 2;
  if (w.direct) {
#pragma unroll
    for (int k = 0; k < WMAX; ++k) {
      if ((tak[k] >> lane) & 1ull) take_corner(S, g, w.T + __popcll(tak[k] & lanes_below(lane)), 64 * k + lane);
      w.T += __popcll(tak[k]);
    }
  }
  if (lane < WMAX) {
    uint64_t t = 0;
#pragma unroll
    for (int k = 0; k < WMAX; ++k)
      if (k == lane) t = tak[k];
    S.tmask[lane] = t;
  }
  wsync();
}

template <int WMAX>
__device__ __forceinline__ void corner_walk(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, Walk& w,
                                            const int lane) {
  if (!(a.compact && corner_compact<WMAX>(S, a, rg, g, w, lane))) corner_generic<WMAX>(S, a, rg, g, w, lane);
}

// Direct path: the visit order of the taken corners (ep first, then descending curvature) into
// region B's vis.  Returns whether two taken corners tie (their order is introsort's).
__device__ __forceinline__ bool corner_visit_order(const FeatLds S, const Seg g, const Walk& w, const int lane) {
  const uint16_t* tlu = rb_at<uint16_t>(S, S.B.tlu());
  const float* tlv = rb_at<float>(S, S.B.tlv());
  uint16_t* vis = rb_at<uint16_t>(S, S.B.vis());
  const int m = g.m;
  bool tf = false;
  for (int c = lane; c < w.T; c += 64) {
    const int u = tlu[c];
    const float vu = tlv[c];
    int rank = 0;
    for (int c2 = 0; c2 < w.T; ++c2) {
      const int u2 = tlu[c2];
      const float v2 = tlv[c2];
      if (u2 == m) rank += (u != m);
      else if (u != m && c2 != c) {
        if (v2 > vu) ++rank;
        else if (!(v2 < vu)) tf = true;
      }
    }
    vis[rank] = (uint16_t)u;
  }
  return __any(tf);
}

// The first kCornerPerSeg taken corners in visit order are kept (the walk breaks there).
__device__ __forceinline__ void corner_cap(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, const Walk& w,
                                           int& corner_cnt, const int lane) {
  const uint16_t* vis = rb_at<uint16_t>(S, S.B.vis());
  const uint16_t* sorder = rb_at<uint16_t>(S, S.B.sorder());
  const int m = g.m;
  const int R = w.direct ? w.T : m + 1;
  int taken = 0;
  for (int r0 = 0; r0 < R && taken < kCornerPerSeg; r0 += 64) {
    const int rr = r0 + lane;
    int u = -1;
    if (rr < R) u = w.direct ? (int)vis[rr] : (int)sorder[rr == 0 ? m : m - rr];
    const bool acc = u >= 0 && (w.direct || ((S.tmask[u >> 6] >> (u & 63)) & 1ull));  // vis holds taken ones only
    const uint64_t mk = __ballot(acc);
    const int pos = taken + __popcll(mk & lanes_below(lane));
    if (acc && pos < kCornerPerSeg) {
      rg.corner_out[corner_cnt + pos] = cloud_point(rg.CL, a.c12, g.sp + u);
      apply_pick(S, S.labpos, g, u);
    }
    taken += __popcll(mk);
  }
  corner_cnt += min(taken, kCornerPerSeg);
  wsync();
}

// -- surf walk: ascending, ep last -> higher priority = not higher corner priority --
// Batch jobs (a.surf_full == 0) need only the walk's picks within reach of ep (they suppress
// the next segment's first members); the last segment of a ring needs none.  The members of
// the window [ulo, m] are resolved with the candidates just left of it frozen (undecided);
// if a member within reach of ep stays undecided (its chain of higher-priority conflicts
// leaves the window), the whole walk runs.
//
// Member-indexed form.  window: resolve [ulo, m] first (FBR_FEAT_COMPACT=0); rest: the
// whole walk follows a window that cm was computed for only.  Returns the path record code.
template <int WMAX, int QP>
__device__ __forceinline__ int surf_generic(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, Walk& w, int ulo,
                                            bool window, bool rest, const int lane, Stamps& tm) {
  const int m = g.m;
  uint64_t und[WMAX], tak[WMAX];
  auto cmf = [&](int u) { return surf_cm(S, u); };
  int code = rest ? 2 : 3;
  bool whole = true;
  if constexpr (kSkipSurf) {
    member_candidates<WMAX>(S, g, S.surfc, 0, lane, und, tak);
  } else {
    if (window) {
      member_candidates<WMAX>(S, g, S.surfc, ulo - 5, lane, und, tak);
      uint64_t frz[WMAX];
#pragma unroll
      for (int k = 0; k < WMAX; ++k) frz[k] = und[k] & __ballot(64 * k + lane < ulo);
      greedy_rounds(m, lane, und, tak, cmf, a, rg.job, frz);
      bool open = false;  // every candidate within reach of ep decided?
#pragma unroll
      for (int k = 0; k < WMAX; ++k) open |= open_near_ep(64 * k + lane, m, und[k] & ~frz[k], lane);
      whole = __any(open);
      code = whole ? 2 : 1;
      rest = whole;
    }
    if (whole) {
      if (rest && w.direct) {  // cm was computed for the listed members only: all of them now
        bool tf2 = false;
        for (int u = lane; u <= m; u += 64) tf2 |= cm_member(S, g, u);
        wsync();
        if (__any(tf2)) sorted_order<QP>(S, rg, g, w, lane, tm);  // a relevant tie: introsort's order for the whole walk
      }
      member_candidates<WMAX>(S, g, S.surfc, 0, lane, und, tak);
      greedy_rounds(m, lane, und, tak, cmf, a, rg.job);
    }
  }
  tm.mark(6);
#pragma unroll
  for (int k = 0; k < WMAX; ++k) {
    const int u = 64 * k + lane;
    if (u <= m && ((tak[k] >> lane) & 1ull)) apply_pick(S, S.labneg, g, u);
  }
  return code;
}

// surf_cm's 10 member-offset bits as the 11 position bits of compact_rounds (bit 5 is the member).
__device__ __forceinline__ uint32_t surf_rel(const FeatLds S, int u) {
  const uint32_t s10 = surf_cm(S, u);
  return (s10 & 31u) | ((s10 >> 5) << 6);
}

// Compact form of the batch walk: the window and the <= 5 frozen candidates left of it,
// re-based at member ulo - 5, are at most swin + 5 <= 69 bits: lane l owns members base + l
// and (lanes 0..4) base + 64 + l, and the 10 member-offset bits of surf_cm are the position
// bits as they stand.  Returns false (nothing applied) when a member within reach of ep stays
// undecided.
__device__ __forceinline__ bool surf_compact(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, int ulo,
                                             const int lane, Stamps& tm) {
  const int m = g.m;
  const int base = max(0, ulo - 5);
  const bool two = m - base >= 64;
  const int u0 = base + lane, u1 = base + 64 + lane;
  const int lb = g.li0 + base, wb = (lb >> 6) + lane;
  const uint64_t swv = (lane < 3 && wb < S.nw) ? ~S.picked.w[wb] & S.surfc.w[wb] : 0ull;
  uint64_t und0 = member_bits(swv, lb & 63, 0, m - base);
  uint64_t und1 = two ? member_bits(swv, lb & 63, 1, m - base) : 0ull;
  const uint64_t frz0 = und0 & ((1ull << (ulo - base)) - 1ull);
  uint64_t tak0 = 0ull, tak1 = 0ull;
  if constexpr (!kSkipSurf) {
    const bool live0 = ((und0 & ~frz0) >> lane) & 1ull;
    if (!two) {
      U128 cf[1];
      cf[0] = place11(live0 ? surf_rel(S, u0) : 0u, lane);
      compact_rounds<1>(lane, und0, und1, tak0, tak1, cf, frz0, 4 * (m - base + 2), a, rg.job);
    } else {
      U128 cf[2];
      cf[0] = place11(live0 ? surf_rel(S, u0) : 0u, lane);
      cf[1] = place11(((und1 >> lane) & 1ull) ? surf_rel(S, u1) : 0u, 64 + lane);
      compact_rounds<2>(lane, und0, und1, tak0, tak1, cf, frz0, 4 * (m - base + 2), a, rg.job);
    }
    // every candidate within reach of ep decided?
    if (__any(open_near_ep(u0, m, und0 & ~frz0, lane) || open_near_ep(u1, m, und1, lane))) return false;
  }
  tm.mark(6);
  if ((tak0 >> lane) & 1ull) apply_pick(S, S.labneg, g, u0);
  if ((tak1 >> lane) & 1ull) apply_pick(S, S.labneg, g, u1);
  return true;
}

// Returns the path record code of the segment's surf walk.
template <int WMAX, int QP>
__device__ __forceinline__ int surf_walk(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, Walk& w, const int lane,
                                         Stamps& tm) {
  const bool bnd = !g.seg_full;
  const int ulo = bnd ? max(0, g.m - (g.swin - 1)) : 0;
  int scode = 0;
  if (bnd && g.j == g.lastj)  // the ring's last segment: no surf pick of it is observable
    tm.mark(6);
  else if (bnd && a.compact)
    scode = surf_compact(S, a, rg, g, ulo, lane, tm) ? 1 : surf_generic<WMAX, QP>(S, a, rg, g, w, ulo, false, ulo > 0, lane, tm);
  else
    scode = surf_generic<WMAX, QP>(S, a, rg, g, w, ulo, bnd && ulo > 0, false, lane, tm);
  return scode;
}

// A segment's walks: wave 0 alone (helper waves wait at the segment's closing barrier).  rec:
// FeatArgs::paths.  The surf candidates (label <= 0 in [sp, ep], :279-284) are selected by the
// per-ring VoxelGrid straight from the label mask (k_voxel_ring.hip, k_voxel_ring).
template <int WMAX, int QP, int NWV>
__device__ __forceinline__ void walk_segment(const FeatLds S, const FeatArgs& a, const Ring rg, const Seg g, Walk& w,
                                             CurvPf<WMAX>& pf, int& corner_cnt, uint32_t& rec, const int lane, Stamps& tm) {
  rec |= 1u << (24 + g.j);
  if (!w.direct) sorted_order<QP>(S, rg, g, w, lane, tm);
  tm.mark(3);
  if (g.has_stale) {
    stale_segment(S, a, rg, g, corner_cnt, lane);
    rec |= 15u << (4 * g.j);
  } else {
    corner_walk<WMAX>(S, a, rg, g, w, lane);
    tm.mark(4);
    if (w.direct) {
      if (corner_visit_order(S, g, w, lane)) {  // tied taken corners: their order is introsort's
        w.direct = false;
        wsync();
        sorted_order<QP>(S, rg, g, w, lane, tm);
        corner_walk<WMAX>(S, a, rg, g, w, lane);
      }
      wsync();
      tm.mark(11);
    }
    corner_cap(S, a, rg, g, w, corner_cnt, lane);
    tm.mark(5);
    if constexpr (NWV == 1) prefetch_curv(S, a, rg, g.j + 1, lane, pf);  // scurv is not read again in this segment
    const int scode = surf_walk<WMAX, QP>(S, a, rg, g, w, lane, tm);
    rec |= (uint32_t)(w.ccode | (scode << 2)) << (4 * g.j);
    prefetch_commit(S, lane, pf);
    wsync();
  }
  tm.mark(7);
  tm.mark(8);
}

template <int NT>
__device__ __forceinline__ void write_outputs(const FeatLds S, const FeatArgs& a, const Ring rg, int8_t* LB, int cb, int ca,
                                              const int tid) {
  const int n = rg.n;
  for (int k = max(cb, 0) + tid; k < ca; k += NT) {
    const int li = k - S.wlo;
    const int8_t lab = S.labpos.get(li) ? 1 : (S.labneg.get(li) ? -1 : 0);
    if (k >= 5 && k < n - 5) LB[k] = lab;      // cloudLabel reset range (:126)
    else if (k < 5 && (lab != 0 || a.fresh)) LB[k] = lab;  // stale slots keep earlier values
  }
  if (cb <= 0 && tid < 5 && tid < S.L) rg.st->picked04[tid] = S.picked.get(tid) ? 1 : 0;
}

// WMAX: 64-bit words of segment-member masks (members <= 64*WMAX); QP: bitonic pairs per lane
// (segment sort <= 128*QP keys).  <6,4> covers Horizon_SCAN <= 2048, <12,8> up to 4096.
// NWV: waves per ring.  NWV = 1 for large launches (every SIMD holds many ring waves, so one wave
// per ring hides its LDS latency behind the others).  With few rings per SIMD (single scans,
// small batches) a ring's critical path is one wave's latency chain, so NWV > 1 spreads the
// lane-parallel passes (flag_pass and picked_init, stage_segment and cm_pass of each segment,
// write_outputs) over NWV waves, while wave 0 alone runs walk_segment (ballot masks, greedy rounds,
// the sorted path) between workgroup barriers.
template <int WMAX, int QP, int NWV>
__global__ void __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(NWV > 1 ? 2 : 4)))
k_features(FeatArgs a) {
  constexpr int NT = 64 * NWV;
  Stamps tm;
  tm.start();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int H = a.H, W = a.W;
  // Ring 0 of every job first: its segment 0 holds the stale cloudSmoothness[4] slot and runs the
  // serial walk, the longest wave of the launch; dispatching those waves first hides them behind
  // the other rings instead of leaving the last jobs' ones in the tail.
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int job = b < a.B ? b : (b - a.B) / (H - 1);
  const int ring = b < a.B ? 0 : 1 + (b - a.B) % (H - 1);
  const int64_t HW = (int64_t)H * W;
  const int slot = job * H + ring;
  Ring rg;
  rg.job = job;
  rg.n = a.nvalid[job];
  rg.s = a.start_ring[slot];
  rg.e = a.end_ring[slot];
  const int cb = rg.s - 4, ca = rg.e + 6;  // this ring's points [cb, ca)
  if (ca <= cb) {
    if (tid == 0) a.corner_cnt[slot] = 0;
    return;
  }
  FeatLds S;
  S.wlo = max(rg.s - 12, 0);
  S.L = min(rg.e + 11, rg.n) - S.wlo;
  S.nw = (S.L + 63) >> 6;
  if (S.L > a.lcap) {
    if (tid == 0) atomicOr(&a.err[job], 1);
    return;
  }
  carve(S, a, smem, slot);
  rg.R = a.range + job * HW;
  rg.C = a.col + job * HW;
  rg.CL = a.cloud + job * HW;
  rg.st = a.stream + job;
  rg.corner_out = a.corner_slot + (int64_t)slot * kCornerPerRing;
  for (int w = tid; w < featlay::kBitArrays * a.nwcap; w += NT) S.gap.w[w] = 0ull;  // the nine arrays, gap first
  __syncthreads();
  tm.mark(0);
  flag_pass<NWV>(S, a, rg, lane, wv);
  picked_init<NT>(S, rg.st, tid);
  tm.mark(1);

  int corner_cnt = 0;
  CurvPf<WMAX> pf;    // 384 entries for W <= 2048
  int lastj = -1;     // the ring's last non-empty segment
  uint32_t rec = 0u;  // FeatArgs::paths
  for (int j = 0; j < 6; j++)
    if (seg_first(rg, j) < seg_last(rg, j)) lastj = j;
  for (int j = 0; j < 6; j++) {
    if (seg_first(rg, j) >= seg_last(rg, j)) continue;
    const Seg g = make_seg(S, a, rg, j, lastj);
    if (g.m + 1 > a.segcap || g.m > a.kseg) {
      if (tid == 0) atomicOr(&a.err[job], 2);
      return;
    }
    stage_segment<NT>(S, g, pf.seg == j, tid);
    Walk w;
    w.T = 0;
    w.ccode = 0;
    cm_pass<WMAX, NWV>(S, g, w, tid, lane, wv, tm);
    if (wv == 0) walk_segment<WMAX, QP, NWV>(S, a, rg, g, w, pf, corner_cnt, rec, lane, tm);
    if constexpr (NWV > 1) __syncthreads();
  }
  if constexpr (NWV > 1) __syncthreads();
  write_outputs<NT>(S, a, rg, a.label + job * HW, cb, ca, tid);
  if (tid == 0) a.corner_cnt[slot] = corner_cnt;
  if (tid == 0 && a.paths) a.paths[slot] = rec | (WMAX == 5 ? 1u : WMAX == 6 ? 2u : 3u) << 30;  // the instance
  tm.mark(9);
  if constexpr (kStamps) {
    if (tid == 0 && a.stamps)
      for (int i = 0; i < 12; ++i) a.stamps[(int64_t)slot * 12 + i] = tm.acc[i];
  }
}

size_t features_lds_bytes(const FeatArgs& a, int nwv) { return (size_t)featlay::lds_of(caps_of(a), nwv).total; }

size_t features_gslot_bytes(const FeatArgs& a) { return (size_t)featlay::slot_of(caps_of(a)).total; }

// Waves per ring: FBR_FEAT_WAVES (1, 2 or 4) or, by default, 4 while a launch has at most 2048
// rings (<= 2 rings per SIMD: single scans, small sub-batches), 1 above.
int feature_waves(int rings) {
  if (const int forced = knobs::feat_waves()) return forced;
  return rings <= 2048 ? 4 : 1;
}

void launch_features(hipStream_t s, const FeatArgs& a) {
  const int nwv = feature_waves(a.B * a.H);
  const dim3 grid(a.B * a.H);
  if (nwv == 1 && a.segcap <= 5 * 64 && a.kseg <= 4 * 128) {
    // Horizon_SCAN <= 1872 (C1 / C2): five mask words, twelve SGPRs of und / tak / frz less
    fbr_launch((k_features<5, 4, 1>), grid, dim3(64), features_lds_bytes(a, 1), s, a);
  } else if (a.segcap <= 6 * 64 && a.kseg <= 4 * 128) {
    if (nwv == 4)
      fbr_launch((k_features<6, 4, 4>), grid, dim3(256), features_lds_bytes(a, 4), s, a);
    else if (nwv == 2)
      fbr_launch((k_features<6, 4, 2>), grid, dim3(128), features_lds_bytes(a, 2), s, a);
    else
      fbr_launch((k_features<6, 4, 1>), grid, dim3(64), features_lds_bytes(a, 1), s, a);
  } else {
    if (nwv > 1)
      fbr_launch((k_features<12, 8, 4>), grid, dim3(256), features_lds_bytes(a, 4), s, a);
    else
      fbr_launch((k_features<12, 8, 1>), grid, dim3(64), features_lds_bytes(a, 1), s, a);
  }
}

}  // namespace fbr
