// csrc/fbr_loop_plan.h alone, on a CPU under AddressSanitizer and UBSan (tests/test_loop_batch.py
// builds and runs it as its own program): the chunks and pool layout of fbr_perform_loop_closures
// and fbr_icp_align_batch for pair sizes {0, 1, 255, 256, 257, 3398} in mixtures.
//   * every block of a chunk's table maps to exactly one pair, and a pair's blocks are 0 .. nblk-1
//     in table order from blk0, nblk = ceil(ns / 256) (none for an empty source);
//   * offsets are multiples of 256 and the pairs' ranges are disjoint and inside the pool totals;
//   * a chunk never exceeds the byte budget unless it holds a single pair, and takes the next pair
//     whenever that pair would still fit (chunk_pairs = 0); with chunk_pairs = k every chunk but the
//     last holds exactly k pairs;
//   * the chunks cover all pairs in order, without gaps or overlap.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fbr_loop_plan.h"

namespace lp = fbr::loop_plan;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static void check_plan(const std::vector<lp::PairSize>& sizes, int64_t chunk_pairs, int64_t budget) {
  const int64_t n = (int64_t)sizes.size();
  const std::vector<lp::Chunk> chunks = lp::plan_chunks(sizes.data(), n, chunk_pairs, budget);
  int64_t next = 0;
  for (size_t ci = 0; ci < chunks.size(); ++ci) {
    const lp::Chunk& c = chunks[ci];
    CHECK(c.first == next && c.count >= 1);  // in order, no gap, no empty chunk
    next = c.first + c.count;
    CHECK(next <= n);
    if (next > n) return;
    int64_t bytes = 0;
    for (int64_t p = 0; p < c.count; ++p) bytes += lp::pair_bytes(sizes[c.first + p]);
    CHECK(bytes == c.bytes);
    if (chunk_pairs > 0) {
      CHECK(c.count <= chunk_pairs);
      if (ci + 1 < chunks.size()) CHECK(c.count == chunk_pairs);
    } else {
      CHECK(c.bytes <= budget || c.count == 1);
      if (next < n) CHECK(c.bytes + lp::pair_bytes(sizes[next]) > budget);  // the next pair did not fit
    }
    std::vector<lp::PairSlot> slots;
    std::vector<lp::BlockRef> table;
    lp::layout_chunk(sizes.data() + c.first, c.count, &slots, &table);
    CHECK((int64_t)slots.size() == c.count && (int64_t)table.size() == c.nblocks);
    std::vector<int> seen(table.size(), 0);
    int64_t src_end = 0, tgt_end = 0;
    for (int64_t p = 0; p < c.count; ++p) {
      const lp::PairSlot& s = slots[p];
      const lp::PairSize& z = sizes[c.first + p];
      CHECK(s.src_off % lp::kAlign == 0 && s.tgt_off % lp::kAlign == 0);
      CHECK(s.src_off >= src_end && s.tgt_off >= tgt_end);  // disjoint: each starts at or past the previous end
      src_end = s.src_off + z.ns;
      tgt_end = s.tgt_off + z.nt;
      CHECK(src_end <= c.src_total && tgt_end <= c.tgt_total);
      CHECK(s.nblk == (z.ns + 255) / 256 && (z.ns > 0 || s.nblk == 0));
      CHECK(s.blk0 >= 0 && s.blk0 + s.nblk <= (int64_t)table.size());
      for (int64_t b = 0; b < s.nblk && s.blk0 + b < (int64_t)table.size(); ++b) {
        const lp::BlockRef& e = table[(size_t)(s.blk0 + b)];
        CHECK(e.pair == p && e.blk == b);
        seen[(size_t)(s.blk0 + b)] += 1;
        // the block's queries lie inside the pair's range, and its partial row is its table index
        CHECK((int64_t)e.blk * 256 < z.ns);
      }
    }
    for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1);
  }
  CHECK(next == n);
  if (n == 0) CHECK(chunks.empty());
}

int main() {
  const int64_t kinds[] = {0, 1, 255, 256, 257, 3398};
  CHECK(lp::align_up(0) == 0 && lp::align_up(1) == 256 && lp::align_up(256) == 256 && lp::align_up(257) == 512);
  CHECK(lp::blocks_of(0) == 0 && lp::blocks_of(1) == 1 && lp::blocks_of(256) == 1 && lp::blocks_of(257) == 2 &&
        lp::blocks_of(3398) == 14);
  unsigned rng = 12345u;
  auto next = [&rng]() {
    rng = rng * 1664525u + 1013904223u;
    return rng >> 8;
  };
  int cases = 0;
  // every ordered pair and triple of the sizes, as sources against every size as target
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b)
      for (int t = 0; t < 6; ++t) {
        std::vector<lp::PairSize> two = {{kinds[a], kinds[t]}, {kinds[b], kinds[(t + 1) % 6]}};
        std::vector<lp::PairSize> three = two;
        three.push_back({kinds[(a + b) % 6], kinds[t]});
        for (int64_t chunk : {0, 1, 2, 3})
          for (int64_t budget : {(int64_t)1, (int64_t)4096, (int64_t)200000, (int64_t)1 << 28}) {
            check_plan(two, chunk, budget);
            check_plan(three, chunk, budget);
            cases += 2;
          }
      }
  // random mixtures of up to 40 pairs
  for (int rep = 0; rep < 300; ++rep) {
    std::vector<lp::PairSize> v(next() % 41);
    for (auto& z : v) z = lp::PairSize{kinds[next() % 6], kinds[next() % 6] * (int64_t)(1 + next() % 3)};
    const int64_t budget = (int64_t)1 << (10 + next() % 16);
    check_plan(v, 0, budget);
    check_plan(v, 1 + next() % 7, budget);
    cases += 2;
  }
  check_plan({}, 0, 1 << 20);
  // a budget that holds exactly two of three equal pairs
  {
    const lp::PairSize z{3398, 5146};
    const std::vector<lp::PairSize> v = {z, z, z};
    const auto ch = lp::plan_chunks(v.data(), 3, 0, 2 * lp::pair_bytes(z));
    CHECK(ch.size() == 2 && ch[0].count == 2 && ch[1].count == 1 && ch[0].nblocks == 28);
    CHECK(ch[0].src_total == 2 * 3584 && ch[0].tgt_total == 2 * 5376);
  }
  if (failures) {
    std::printf("loop_plan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("loop_plan_check: ok (%d plans)\n", cases);
  return 0;
}
