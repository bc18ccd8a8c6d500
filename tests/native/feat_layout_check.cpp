// feat_layout_check.cpp — csrc/fbr_feat_layout.h on a CPU: k_features' LDS, scratch-slot and region-B
// layout for every Horizon_SCAN W in 1 .. 4096 and 1, 2 or 4 waves per ring.
//
// Stand-alone; built with -fsanitize=address,undefined and run by tests/test_resources.py: it prints
// "feat_layout_check: ok" and exits 0, or names the first checks that failed and exits 1.
//
// The expected totals are the formulas k_features.hip and fbr_api.hip held before the layout header
// existed (features_lds_bytes, features_gslot_bytes, feat_caps), written out here on purpose.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <utility>
#include <vector>

#include "fbr_feat_layout.h"

using namespace fbr::featlay;

static int failures = 0;
#define CHECK(cond, ...)                                                              \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      if (failures++ < 20) {                                                          \
        std::printf("feat_layout_check: FAILED %s (line %d) ", #cond, __LINE__);      \
        std::printf(__VA_ARGS__);                                                     \
        std::printf("\n");                                                            \
      }                                                                               \
    }                                                                                 \
  } while (0)

static bool overlap(const Span& a, const Span& b) { return a.off < b.end() && b.off < a.end(); }

int main() {
  static_assert(caps_of(1800).segcap == 308 && caps_of(1800).kseg == 512, "constexpr layout");
  for (int W = 1; W <= 4096; ++W) {
    const Caps c = caps_of(W);
    // feat_caps / seg_cap as they were
    int kseg = 1;
    while (kseg < W / 6 + 8 - 1) kseg <<= 1;
    CHECK(c.lcap == W + 16 && c.segcap == W / 6 + 8 && c.kseg == kseg && c.nwcap == (W + 16 + 63) / 64 + 1, "W=%d", W);

    const Slot g = slot_of(c);
    {  // features_gslot_bytes as it was (sizeof(uint64_t) = sizeof(SmoothEntry) = 8)
      const size_t b = 8 * (size_t)c.kseg + 2 * 8 * (size_t)c.segcap + 2 * 2 * (size_t)c.segcap + 16 + 4 * (size_t)c.lcap;
      CHECK((size_t)g.total == ((b + 255) & ~(size_t)255), "W=%d", W);
    }
    CHECK(g.keys == 0 && g.seg == 8 * (int64_t)c.kseg && g.tmp == g.seg + 8 * (int64_t)c.segcap, "W=%d", W);
    CHECK(g.spare == g.tmp + 8 * (int64_t)c.segcap, "W=%d", W);
    CHECK(g.gcurv == ((g.spare + 4 * (int64_t)c.segcap + 15) & ~(int64_t)15), "W=%d", W);
    CHECK(g.keys % 8 == 0 && g.seg % 8 == 0 && g.tmp % 8 == 0 && g.gcurv % 16 == 0 && g.total % 256 == 0, "W=%d", W);
    CHECK(g.gcurv + 4 * (int64_t)c.lcap <= g.total, "W=%d", W);

    const RegionB rb{c.segcap};
    for (int nwv : {1, 2, 4}) {
      const Lds l = lds_of(c, nwv);
      {  // features_lds_bytes as it was (sizeof(SortFrame) = 12, kSortStack = 32, kCornerPerSeg = 20)
        const size_t region_b = std::max<size_t>((size_t)nwv * 1632, (size_t)8 * c.segcap + 4 * 20);
        const size_t want = (size_t)((c.segcap + 19) & ~3) * 4 + (size_t)9 * c.nwcap * 8 + 8 * 16 + 12 * 32 +
                            4 * (size_t)c.segcap + 16 + region_b;
        CHECK((size_t)l.total == want, "W=%d nwv=%d", W, nwv);
      }
      // the offsets the kernel carved by hand
      CHECK(l.scurv == 0 && l.bits == 4 * ((c.segcap + 19) & ~3) && l.tmask == l.bits + 72 * c.nwcap, "W=%d", W);
      CHECK(l.sstack == l.tmask + 128 && l.cm == l.sstack + 384 && l.rb == ((l.cm + 4 * c.segcap + 15) & ~15), "W=%d", W);
      CHECK(l.bits % 8 == 0 && l.tmask % 8 == 0 && l.rb % 16 == 0, "W=%d", W);
      CHECK(l.scurv + 4 * (c.segcap + 16) <= l.bits, "W=%d", W);
      const int rbytes = rb.bytes(nwv);
      CHECK(l.rb + rbytes <= l.total, "W=%d nwv=%d", W, nwv);

      // every tenant ends inside region B
      std::vector<std::pair<const char*, Span>> all = {
          {"cm_list", rb.cm_list()}, {"cand_list", rb.cand_list()}, {"part_copy", rb.part_copy()},
          {"sorder", rb.sorder()},   {"rankc", rb.rankc()},         {"tlv", rb.tlv()},
          {"tlu", rb.tlu()},         {"vis", rb.vis()},             {"stale_ent", rb.stale_ent()},
          {"stale_tlist", rb.stale_tlist()}};
      for (int wv = 0; wv < nwv; ++wv) all.push_back({"win", rb.win(wv)});
      for (const auto& t : all)
        CHECK(t.second.off >= 0 && t.second.bytes > 0 && t.second.end() <= rbytes, "%s W=%d nwv=%d", t.first, W, nwv);

      // tenants the header's table declares live together do not overlap
      const std::vector<std::vector<Span>> together = {
          {rb.cm_list(), rb.cand_list()},
          {rb.sorder(), rb.rankc(), rb.cand_list()},
          {rb.tlv(), rb.tlu(), rb.vis()},
          {rb.stale_ent(), rb.stale_tlist()}};
      for (size_t s = 0; s < together.size(); ++s)
        for (size_t i = 0; i < together[s].size(); ++i)
          for (size_t k = i + 1; k < together[s].size(); ++k)
            CHECK(!overlap(together[s][i], together[s][k]), "set %zu W=%d", s, W);
      for (int a = 0; a < nwv; ++a)
        for (int b = a + 1; b < nwv; ++b) CHECK(!overlap(rb.win(a), rb.win(b)), "win W=%d", W);

      // element alignment of the tenants: 16 B for the windows, 8 B for the entries, 4 B for floats
      CHECK(rb.win(nwv - 1).off % 16 == 0 && rb.part_copy().off % 8 == 0 && rb.stale_ent().off % 8 == 0, "W=%d", W);
      CHECK(rb.tlv().off % 4 == 0 && rb.stale_tlist().off % 4 == 0, "W=%d", W);
      CHECK(rb.cand_list().off % 2 == 0 && rb.rankc().off % 2 == 0 && rb.tlu().off % 2 == 0 && rb.vis().off % 2 == 0, "W=%d", W);
    }
  }
  if (failures) {
    std::printf("feat_layout_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("feat_layout_check: ok\n");
  return 0;
}
