// fbr_loop_plan.h — how a list of ICP pairs is cut into chunks and laid out in the pooled buffers
// of fbr_perform_loop_closures / fbr_icp_align_batch (fbr_loop.hip, k_icp.hip's batch kernels).
//
// Free of HIP headers, as fbr_pace.h is: tests/native/loop_plan_check.cpp checks it on a CPU.
//
// A chunk is a run of consecutive pairs that are in flight together.  Inside a chunk
//   * a pair's source-sized arrays (src, x, key, far_list) start at src_off and its target-sized
//     ones (the raw concatenation, the target) at tgt_off, in elements, both multiples of kAlign;
//   * its queries are cut into 256-query blocks from its own query 0: block b of the pair is entry
//     blk0 + b of the chunk's block table and owns row blk0 + b of the chunk's partial sums, so the
//     pair's sums run over its own rows in its own order, as in a single-pair call;
//   * a pair without source points has no block.
// The byte estimate of a pair is what the pools hold for it plus a nominal size of its search grid
// (the grid's cell array depends on the target's box, which is not known when the chunks are cut):
// the budget is a target for the pools' size, not a limit the allocator enforces.
//
// The namespace is hidden: nothing of it is exported from the library.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace fbr {
namespace loop_plan __attribute__((visibility("hidden"))) {

constexpr int64_t kAlign = 256;          // elements: a pair's first query is a block's first
constexpr int64_t kQueriesPerBlock = 256;
constexpr int64_t kPartialDoubles = 18;  // kIcpSums (fbr_kernels.h; fbr_loop.hip asserts the two agree)
constexpr int64_t kPairFixedBytes = 1024;  // two argument blocks, state, result, counts
constexpr int64_t kGridBytesPerPoint = 288;  // 2 x 16 B of points and a nominal 64 cells of 4 B
constexpr int64_t kMaxChunkBlocks = (int64_t)1 << 30;  // the block table's index is an int

struct PairSize {
  int64_t ns;  // source points
  int64_t nt;  // target points the pools must hold (loop closure: before the VoxelGrid)
};
struct PairSlot {
  int64_t src_off, tgt_off;  // elements into the source-sized / target-sized pools
  int64_t blk0, nblk;        // first entry of the block table (and partial row), blocks
};
struct BlockRef {  // a block table entry (an int2 on the device)
  int32_t pair, blk;
};
struct Chunk {
  int64_t first, count;          // pairs [first, first + count)
  int64_t src_total, tgt_total;  // elements of the source-sized / target-sized pools
  int64_t nblocks;
  int64_t bytes;                 // sum of pair_bytes
};

inline int64_t align_up(int64_t n) { return (std::max<int64_t>(n, 0) + kAlign - 1) / kAlign * kAlign; }
inline int64_t blocks_of(int64_t n) { return n > 0 ? (n + kQueriesPerBlock - 1) / kQueriesPerBlock : 0; }

// Device bytes a pair accounts for: src and x (16 B), key (8 B), far_list (4 B) per source slot, a
// partial row per block, raw and target (16 B each) per target slot, the nominal grid.
inline int64_t pair_bytes(const PairSize& z) {
  return 44 * align_up(z.ns) + 8 * kPartialDoubles * blocks_of(z.ns) + 32 * align_up(z.nt) +
         kGridBytesPerPoint * std::max<int64_t>(z.nt, 0) + kPairFixedBytes;
}

// The chunks of n pairs, in order.  chunk_pairs > 0: that many pairs each (the last one fewer);
// 0: as many as keep the chunk's bytes within `budget`, at least one.  Either way a chunk ends
// before its block table would pass kMaxChunkBlocks.
inline std::vector<Chunk> plan_chunks(const PairSize* sizes, int64_t n, int64_t chunk_pairs, int64_t budget) {
  std::vector<Chunk> out;
  Chunk c{0, 0, 0, 0, 0, 0};
  for (int64_t p = 0; p < n; ++p) {
    const int64_t b = pair_bytes(sizes[p]), nb = blocks_of(sizes[p].ns);
    const bool full = chunk_pairs > 0 ? c.count >= chunk_pairs : c.bytes + b > budget;
    if (c.count > 0 && (full || c.nblocks + nb > kMaxChunkBlocks)) {
      out.push_back(c);
      c = Chunk{p, 0, 0, 0, 0, 0};
    }
    c.count += 1;
    c.src_total += align_up(sizes[p].ns);
    c.tgt_total += align_up(sizes[p].nt);
    c.nblocks += nb;
    c.bytes += b;
  }
  if (c.count > 0) out.push_back(c);
  return out;
}

// The slots of a chunk's pairs (sizes points at the chunk's first pair) and its block table.
inline void layout_chunk(const PairSize* sizes, int64_t count, std::vector<PairSlot>* slots, std::vector<BlockRef>* table) {
  slots->clear();
  table->clear();
  int64_t so = 0, to = 0;
  for (int64_t p = 0; p < count; ++p) {
    PairSlot s;
    s.src_off = so;
    s.tgt_off = to;
    s.blk0 = (int64_t)table->size();
    s.nblk = blocks_of(sizes[p].ns);
    for (int64_t b = 0; b < s.nblk; ++b) table->push_back(BlockRef{(int32_t)p, (int32_t)b});
    so += align_up(sizes[p].ns);
    to += align_up(sizes[p].nt);
    slots->push_back(s);
  }
}

}  // namespace loop_plan
}  // namespace fbr
