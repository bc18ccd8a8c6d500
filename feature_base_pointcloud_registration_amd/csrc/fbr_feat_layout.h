// fbr_feat_layout.h — where k_features keeps what: its capacities for a Horizon_SCAN of W, the
// carve-up of its dynamic LDS and of a ring's global scratch slot, and the tenants of LDS region B.
//
// The kernel (k_features.hip) fills its pointers from these offsets and the host sizes the launch
// and the scratch array from the same totals (features_lds_bytes, features_gslot_bytes, feat_caps),
// so the two cannot drift apart.  Free of HIP headers, as fbr_pace.h is: tests/native/
// feat_layout_check.cpp checks every offset on a CPU for every W.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FBR_FEAT_HD __host__ __device__
#else
#define FBR_FEAT_HD
#endif

namespace fbr {
namespace featlay {

constexpr int kWin = 256 + 16;            // phase-2 window: 4 chunks of 64 indices + 8 on each side
constexpr int kWinBytes = kWin * (4 + 2); // float range + int16 column: 1632 B per wave (16-B multiple)
constexpr int kBitArrays = 9;             // gap, picked, labpos, labneg, edgec, surfc, occa, occb, occc
constexpr int kTmaskWords = 16;           // taken-mask words (WMAX <= 12; word 15: the cm list length)
// The next four restate sizes of HIP-side types, so that this header stays free of HIP; a
// static_assert at the top of k_features.hip ties each to its original.
constexpr int kSortFrameBytes = 12, kSortStackFrames = 32;  // SortFrame[kSortStack] (fbr_sort.h)
constexpr int kEntryBytes = 8;            // SmoothEntry (fbr_sort.h)
constexpr int kCornersKept = 20;          // kCornerPerSeg (fbr_common.h)

struct Caps {
  int lcap;    // ring window length (points)
  int segcap;  // segment length (members, ep included)
  int kseg;    // segment sort capacity: next power of two >= segcap - 1
  int nwcap;   // 64-bit words per window bit array
};

FBR_FEAT_HD constexpr Caps caps_of(int W) {
  Caps c{W + 16, W / 6 + 8, 1, 0};
  while (c.kseg < c.segcap - 1) c.kseg <<= 1;
  c.nwcap = (c.lcap + 63) / 64 + 1;
  return c;
}

struct Span {
  int off, bytes;  // from the start of region B
  FBR_FEAT_HD constexpr int end() const { return off + bytes; }
};

// Region B: one LDS span with a tenant per phase of a segment's life.
//
//   tenant           bytes                    live                                   written by
//   win(wv)          kWinBytes per wave       flag pass                              flag_pass
//   cm_list          2 * segcap               cm pass of a batch segment             cm_pass
//   cand_list        2 * segcap  @ 4 segcap   cm pass .. compact corner walk         cm_pass / corner_compact
//   part_copy        8 * segcap               tie sort's partition phase             sort_tied
//   sorder, rankc    2 * segcap each          sorted path: sort's end .. corner cap  cm_from_ranks
//   tlv, tlu, vis    4, 2, 2 * segcap         direct path: corner walk .. corner cap corner walks, corner_visit_order
//   stale_ent, tlist 8 * segcap, 4 * 20       stale-slot segment's walks             stale_segment, stale_walks_fast
//
// Live together (must not overlap): the waves' windows; cm_list + cand_list; sorder + rankc +
// cand_list; tlv + tlu + vis; stale_ent + stale_tlist.  Everything else aliases by lifetime: the
// windows die with the flag pass; cm_list after the cm pass; part_copy is dead (and has overwritten
// cand_list, which the corner walk then lists again) before sorder / rankc are written; tlu takes
// cand_list's place once the compact walk has read its candidates into registers.
struct RegionB {
  int segcap;
  FBR_FEAT_HD constexpr Span win(int wv) const { return {wv * kWinBytes, kWinBytes}; }
  FBR_FEAT_HD constexpr Span cm_list() const { return {0, 2 * segcap}; }
  FBR_FEAT_HD constexpr Span cand_list() const { return {4 * segcap, 2 * segcap}; }
  FBR_FEAT_HD constexpr Span part_copy() const { return {0, kEntryBytes * segcap}; }
  FBR_FEAT_HD constexpr Span sorder() const { return {0, 2 * segcap}; }
  FBR_FEAT_HD constexpr Span rankc() const { return {2 * segcap, 2 * segcap}; }
  FBR_FEAT_HD constexpr Span tlv() const { return {0, 4 * segcap}; }
  FBR_FEAT_HD constexpr Span tlu() const { return {4 * segcap, 2 * segcap}; }
  FBR_FEAT_HD constexpr Span vis() const { return {6 * segcap, 2 * segcap}; }
  FBR_FEAT_HD constexpr Span stale_ent() const { return {0, kEntryBytes * segcap}; }
  FBR_FEAT_HD constexpr Span stale_tlist() const { return {kEntryBytes * segcap, 4 * kCornersKept}; }
  FBR_FEAT_HD constexpr int bytes(int nwv) const {
    // the longest tenant set of the walks is the stale one: every other tenant ends by 8 * segcap
    const int walks = stale_tlist().end(), wins = nwv * kWinBytes;
    return wins > walks ? wins : walks;
  }
};

// Dynamic LDS of one workgroup (one ring), byte offsets.
struct Lds {
  int scurv;  // float[segcap + 16], padded to a 16-B multiple: the bit words behind it are 64-bit
  int bits;   // uint64[kBitArrays][nwcap]
  int tmask;  // uint64[kTmaskWords]
  int sstack; // SortFrame[kSortStack]
  int cm;     // uint32[segcap]
  int rb;     // region B, 16-B aligned
  int total;
};

FBR_FEAT_HD constexpr Lds lds_of(const Caps& c, int nwv) {
  Lds l{};
  l.scurv = 0;
  l.bits = l.scurv + 4 * ((c.segcap + 19) & ~3);
  l.tmask = l.bits + 8 * kBitArrays * c.nwcap;
  l.sstack = l.tmask + 8 * kTmaskWords;
  l.cm = l.sstack + kSortFrameBytes * kSortStackFrames;
  const int end = l.cm + 4 * c.segcap;
  l.rb = (end + 15) & ~15;
  l.total = end + 16 + RegionB{c.segcap}.bytes(nwv);  // 16: the round-up's worst case, as ever
  return l;
}

// A ring's slot of FeatArgs::gscratch (the sorted path's buffers and the window's curvature).
struct Slot {
  int64_t keys;   // uint64[kseg] sort keys
  int64_t seg;    // SmoothEntry[segcap] the sorted entries
  int64_t tmp;    // SmoothEntry[segcap]
  int64_t spare;  // 2 x uint16[segcap], unused (sorder / rankc moved to region B): keeps gcurv in place
  int64_t gcurv;  // float[lcap], 16-B aligned
  int64_t total;  // 256-B multiple
};

FBR_FEAT_HD constexpr Slot slot_of(const Caps& c) {
  Slot s{};
  s.keys = 0;
  s.seg = s.keys + (int64_t)8 * c.kseg;
  s.tmp = s.seg + (int64_t)kEntryBytes * c.segcap;
  s.spare = s.tmp + (int64_t)kEntryBytes * c.segcap;
  const int64_t end = s.spare + (int64_t)2 * 2 * c.segcap;
  s.gcurv = (end + 15) & ~(int64_t)15;
  s.total = (end + 16 + (int64_t)4 * c.lcap + 255) & ~(int64_t)255;
  return s;
}

}  // namespace featlay
}  // namespace fbr
