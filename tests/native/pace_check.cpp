// pace_check.cpp — csrc/fbr_pace.h on a CPU: the flag words, the bounded-query flag wait and the
// run-ahead loop over a fake clock, and the Gauss-Newton launch plan against cases worked out by
// hand from the run driver's rules.
//
// A stand-alone program (tests/test_resources.py builds it with -fsanitize=address,undefined and
// runs it): it prints "pace_check: ok" and exits 0, or names the first check that failed and exits 1.
#include <cstdio>
#include <cstdlib>

#include "fbr_pace.h"

using namespace fbr::pace;

// the library's wait statistics, stood in for
static int64_t g_stat_last = -1;
static int g_stat_calls = 0;
void wait_stat(int64_t ns) {
  g_stat_last = ns;
  ++g_stat_calls;
}

namespace {

#define CHECK(x)                                                      \
  do {                                                                \
    if (!(x)) {                                                       \
      std::printf("pace_check: FAILED %s (line %d)\n", #x, __LINE__); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

// A clock that moves only when told to, or by `step` at each reading; it counts its readings.
struct FakeClock {
  using duration = std::chrono::nanoseconds;
  using rep = duration::rep;
  using period = duration::period;
  using time_point = std::chrono::time_point<FakeClock>;
  static constexpr bool is_steady = true;
  static int64_t t, step;
  static long reads;
  static time_point now() {
    ++reads;
    t += step;
    return time_point(duration(t));
  }
  static void reset(int64_t step_ns = 0) {
    t = 1000;
    step = step_ns;
    reads = 0;
  }
};
int64_t FakeClock::t = 0, FakeClock::step = 0;
long FakeClock::reads = 0;
using Wait = FlagWaitT<FakeClock>;

void check_words() {
  const unsigned long long g = 0xFFFFFFFFull;
  const unsigned long long c = pack_count(g, 0xFFFFFFFFu);
  CHECK(c == ~0ull && word_of(c, g) && word_count(c) == 0xFFFFFFFFu);
  CHECK(pack_count(7, 0) == 7ull << 32 && word_count(pack_count(7, 0)) == 0);
  // only the generation's low 32 bits are kept, and compared
  CHECK(pack_count(0x500000003ull, 9) == ((3ull << 32) | 9) && word_of(pack_count(0x500000003ull, 9), 0x500000003ull));
  CHECK(!word_of(pack_count(3, 9), 4) && !word_of(0, 1) && word_of(0, 0));
  const unsigned long long p = pack_progress(g, 0x7FFFFFFFu, 1);  // iterations have 31 bits
  CHECK(p == ~0ull && word_of(p, g) && word_iters(p) == 0x7FFFFFFF && word_stop(p));
  const unsigned long long q = pack_progress(g, 0x7FFFFFFFu, 0);
  CHECK(word_of(q, g) && word_iters(q) == 0x7FFFFFFF && !word_stop(q));
  CHECK(pack_progress(2, 5, 1) == ((2ull << 32) | 11) && word_iters(pack_progress(2, 5, 1)) == 5);
  static_assert(pack_count(1, 2) == 0x100000002ull && pack_progress(1, 2, 1) == 0x100000005ull, "constexpr");
}

void check_bound() {
  WaitBound b;
  CHECK(b.after() == kQueryMaxNs && kQueryMaxNs == 2000000 && kQueryMinNs == 500000);
  b.done(100000);
  CHECK(b.ema_ns == 100000.0 && b.after() == kQueryMinNs);  // 4 x 100 us is under the floor
  WaitBound b3;
  b3.done(300000);
  CHECK(b3.after() == 1200000);
  b3.done(1100000);  // 0.875 x 300 us + 0.125 x 1100 us = 400 us
  CHECK(b3.ema_ns == 0.875 * 300000.0 + 0.125 * 1100000.0 && b3.after() == 1600000);
  b3.done(10000000);
  CHECK(b3.after() == kQueryMaxNs);
}

// Polls until the first due query; returns the number of unanswered reads it took.
long polls_to_query(Wait& w, long limit) {
  for (long k = 1; k <= limit; ++k)
    if (w.query_due()) return k;
  return -1;
}

void check_flag_wait() {
  // the clock is read on every 1024th poll only: the 1023rd, 2047th, ... (phase 0), or the
  // 1024th, 2048th, ... (phase -1)
  for (long phase = 0; phase >= -1; --phase) {
    WaitBound b;
    FakeClock::reset();
    Wait w;
    w.begin(b, FakeClock::now(), phase);
    CHECK(w.next_query == kQueryMaxNs);
    const long reads0 = FakeClock::reads;
    for (long k = 1; k <= 5000; ++k) {
      CHECK(!w.query_due());  // the clock stands still: never due
      CHECK(FakeClock::reads - reads0 == (k + phase + 1) / 1024);
    }
  }
  // no query before bound.after(): empty bound 2 ms, after done(100 us) 500 us, after done(300 us) 1.2 ms
  const int64_t ema[3] = {0, 100000, 300000}, after[3] = {kQueryMaxNs, kQueryMinNs, 1200000};
  for (int c = 0; c < 3; ++c) {
    WaitBound b;
    if (ema[c]) b.done(ema[c]);
    FakeClock::reset();
    Wait w;
    w.begin(b, FakeClock::now());
    FakeClock::t += after[c];  // exactly the bound: not due yet (due once waited > next_query)
    CHECK(polls_to_query(w, 1023) == -1 && w.waited == after[c]);
    FakeClock::t += 1;
    CHECK(polls_to_query(w, 1024) == 1024 && w.waited == after[c] + 1);
    // the next one no earlier than waited + max(kQueryMinNs, previous next_query / 2)
    const int64_t gap = std::max<int64_t>(kQueryMinNs, after[c] / 2);
    CHECK(w.next_query == after[c] + 1 + gap);
    FakeClock::t += gap;
    CHECK(polls_to_query(w, 1024) == -1);
    FakeClock::t += 1;
    CHECK(polls_to_query(w, 1024) == 1024);
    CHECK(w.next_query == w.waited + std::max<int64_t>(kQueryMinNs, (after[c] + 1 + gap) / 2));
  }
  // a wait resumed across calls keeps its start and its poll count; finish feeds the bound (EMA by
  // 0.875 / 0.125) and the statistics, and leaves the state idle
  WaitBound b;
  b.done(200000);
  FakeClock::reset();
  Wait w;
  CHECK(w.polls == 0);
  w.begin(b, FakeClock::now());
  CHECK(!w.query_due() && w.polls == 1);
  FakeClock::t += 600000;
  const int calls = g_stat_calls;
  w.finish(b);
  CHECK(w.polls == 0 && w.waited == 600000 && g_stat_last == 600000 && g_stat_calls == calls + 1);
  CHECK(b.ema_ns == 0.875 * 200000.0 + 0.125 * 600000.0);
}

void check_run_ahead() {
  std::atomic<long long> polls{0};
  unsigned long long word = 0;
  const unsigned long long gen = 0xFFFFFFFFull;
  FakeClock::reset(1000);  // every reading moves the clock 1 us
  // nothing seen yet: iterations 0 .. lead go at once, one read each
  for (int it = 0; it <= 4; ++it) CHECK(!run_ahead<FakeClock>(&word, gen, it, 4, polls));
  CHECK(polls.load() == 5);
  // a word of another generation counts as nothing seen, stopped or not: iteration 5 waits, and
  // gives up after 2 ms with the word unchanged
  word = pack_progress(gen - 1, 100, 1);
  int64_t t0 = FakeClock::t;
  polls = 0;
  CHECK(!run_ahead<FakeClock>(&word, gen, 5, 4, polls));
  CHECK(FakeClock::t - t0 > 2000000 && FakeClock::t - t0 <= 2002000 && polls.load() == 2001);
  // this generation's: at most `lead` behind returns at once
  word = pack_progress(gen, 3, 0);
  polls = 0;
  CHECK(!run_ahead<FakeClock>(&word, gen, 7, 4, polls) && polls.load() == 1);
  t0 = FakeClock::t;
  CHECK(!run_ahead<FakeClock>(&word, gen, 8, 4, polls) && FakeClock::t - t0 > 2000000);  // 5 behind
  // stopped only with the generation and the low bit
  word = pack_progress(gen, 3, 1);
  polls = 0;
  CHECK(run_ahead<FakeClock>(&word, gen, 100, 4, polls) && polls.load() == 1);
  CHECK(run_ahead<FakeClock>(&word, gen, 0, 4, polls));
  word = pack_progress(gen, 96, 0);
  CHECK(!run_ahead<FakeClock>(&word, gen, 100, 4, polls));
  word = pack_progress(5, 96, 1);
  CHECK(!run_ahead<FakeClock>(&word, gen, 4, 4, polls));
}

struct Known {
  int value;
  mutable int calls = 0;
  int operator()() const {
    ++calls;
    return value;
  }
};

// the default knobs: tail divisor 8, one-item on, tail-one-item on, grid cap 16384, one-grid 32768
GnPlanIn plan_in(int B, bool stream, int active, int max_items, int items_hint, int hint_n, int hint_B) {
  GnPlanIn in{};
  in.tail_div = 8;
  in.grid_cap = 16384;
  in.one_grid = 32768;
  in.one_item = in.tail_one_item = true;
  in.B = B;
  in.stream_mode = stream;
  in.active = active;
  in.max_items = max_items;
  in.items_hint = items_hint;
  in.hint_n = hint_n;
  in.hint_B = hint_B;
  return in;
}

bool is(const GnPlan& p, bool fused, int grid, int mode, int rest) {
  return p.fused == fused && p.grid == grid && p.one_mode == mode && p.rest_grid == rest;
}

void check_gn_plan() {
  const Known none{-1};
  GnPlan p = gn_plan(plan_in(341, false, 341, 40000, 0, 0, 0), none);
  CHECK(is(p, false, 32768, 1, 0) && p.adopt < 0 && none.calls == 1);
  p = gn_plan(plan_in(341, false, 341, 40000, 0, 11000, 341), none);
  CHECK(is(p, false, 14006, 1, 64) && p.adopt < 0);
  p = gn_plan(plan_in(341, false, 341, 40000, 0, 11000, 340), none);  // a hint of another job count
  CHECK(is(p, false, 32768, 1, 0));
  for (int hint_B : {0, 341, 340}) {  // the known count wins over any hint
    p = gn_plan(plan_in(341, false, 341, 40000, 0, hint_B ? 11000 : 0, hint_B), Known{10950});
    CHECK(is(p, false, 10950, 2, 0) && p.adopt == 10950);
    p = gn_plan(plan_in(341, false, 341, 40000, 0, hint_B ? 11000 : 0, hint_B), Known{0});
    CHECK(is(p, false, 1, 2, 0) && p.adopt == 0);
  }
  CHECK(!gn_plan(plan_in(341, false, 43, 40000, 0, 0, 0), none).fused);  // 43 x 8 > 341
  p = gn_plan(plan_in(341, false, 42, 40000, 0, 0, 0), Known{10950});
  CHECK(is(p, true, 10950, 2, 0) && p.adopt == 10950);
  p = gn_plan(plan_in(341, false, 42, 40000, 0, 0, 0), none);
  CHECK(is(p, true, 32768, 1, 0));
  {
    GnPlanIn in = plan_in(341, false, 42, 40000, 0, 0, 0);  // tail-one-item off: a 1,024-workgroup loop
    in.tail_one_item = false;
    const Known k{10950};
    p = gn_plan(in, k);
    CHECK(is(p, true, 1024, 0, 0) && p.adopt < 0 && k.calls == 0);
    in.grid_cap = 512;
    CHECK(is(gn_plan(in, k), true, 512, 0, 0));
  }
  {
    GnPlanIn in = plan_in(341, false, 341, 40000, 0, 11000, 341);  // one-item off
    in.one_item = false;
    const Known k{10950};
    p = gn_plan(in, k);
    CHECK(is(p, false, 16384, 0, 0) && p.adopt < 0 && k.calls == 0);
    in.active = 42;
    CHECK(is(gn_plan(in, k), true, 1024, 0, 0) && k.calls == 0);
  }
  CHECK(is(gn_plan(plan_in(341, false, 341, 100, 0, 0, 0), none), false, 100, 1, 0));
  // single scans: the loop over the previous scan's grid until the count is known
  const Known single{-1};
  CHECK(is(gn_plan(plan_in(1, true, 1, 2000, 450, 0, 0), single), false, 900, 0, 0) && single.calls == 1);
  CHECK(is(gn_plan(plan_in(1, true, 1, 2000, 3, 0, 0), none), false, 16, 0, 0));
  p = gn_plan(plan_in(1, true, 1, 2000, 450, 0, 0), Known{430});
  CHECK(is(p, false, 430, 2, 0) && p.adopt == 430);
  CHECK(is(gn_plan(plan_in(1, true, 1, 2000, 0, 0, 0), none), false, 2000, 0, 0));
  // tail divisor 0: never fused
  for (int active : {341, 42, 1, 0}) {
    GnPlanIn in = plan_in(341, false, active, 40000, 0, 0, 0);
    in.tail_div = 0;
    CHECK(!gn_plan(in, none).fused);
  }
  CHECK(gn_plan(plan_in(341, false, 0, 40000, 0, 0, 0), none).fused);
}

}  // namespace

int main() {
  check_words();
  check_bound();
  check_flag_wait();
  check_run_ahead();
  check_gn_plan();
  std::printf("pace_check: ok\n");
  return 0;
}
