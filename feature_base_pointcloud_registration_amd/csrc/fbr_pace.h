// fbr_pace.h — how the host paces itself on words the device writes into host-mapped memory.
//
// Free of HIP headers, as fbr_own.h and fbr_knobs.h are: the word formats (which the kernels that
// write the words include too), the bounded-query flag wait, the run-ahead loop of ICP and the pose
// graph's PCG, and the launch shape of a Gauss-Newton iteration.  None of it calls HIP or reads the
// environment, and the waits take their clock as a template parameter, so tests/native/pace_check.cpp
// checks all of it on a CPU, without sleeping.
//
// The namespace is hidden: nothing of it is exported from the library.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>

#if defined(__HIPCC__)
#define FBR_PACE_HD __host__ __device__
#else
#define FBR_PACE_HD
#endif

// Every completed wait into the process-wide wait statistics (fbr_stages.hip; fbr_diag_wait_stats).
void wait_stat(int64_t ns);

namespace fbr {
namespace pace __attribute__((visibility("hidden"))) {

using u64 = unsigned long long;

// ---- the words ---------------------------------------------------------------------------------
// Both carry the low 32 bits of their run's generation on top, so a word a previous run left
// behind never reads as this run's.
// A count word, (gen << 32) | count: k_gn_solve's iter_flags (jobs still iterating) and items_flag.
// (count < 2^32 is the caller's: k_gn_solve widens its int count as it always did.)
FBR_PACE_HD constexpr u64 pack_count(u64 gen, u64 count) { return (gen << 32) | count; }
// A progress word, (gen << 32) | (iters << 1) | stop: k_icp_solve and the pose graph's pg_publish.
FBR_PACE_HD constexpr u64 pack_progress(u64 gen, uint32_t iters, unsigned stop) { return (gen << 32) | ((u64)iters << 1) | stop; }
FBR_PACE_HD constexpr bool word_of(u64 w, u64 gen) { return (w >> 32) == (gen & 0xFFFFFFFFull); }
FBR_PACE_HD constexpr uint32_t word_count(u64 w) { return (uint32_t)w; }
FBR_PACE_HD constexpr int word_iters(u64 w) { return (int)((w & 0xFFFFFFFFull) >> 1); }
FBR_PACE_HD constexpr bool word_stop(u64 w) { return (w & 1) != 0; }

template <typename TimePoint>
int64_t ns_since(TimePoint t0) {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(TimePoint::clock::now() - t0).count();
}

// ---- the flag wait -----------------------------------------------------------------------------
// A flag wait asks the runtime whether the stream drained (flags not visible although the work
// is done) only once it has lasted several times longer than the waits of its kind usually do:
// hipStreamQuery puts a marker into the stream, and a marker between two iterations' kernels cost
// ~5.7 us on the device (every launch enqueued after a wait had one).  The bound is 4x the
// smoothed duration of the completed waits of that kind (GN flags of batch runs, of single-scan
// runs, single-scan direct results), within [kQueryMinNs, kQueryMaxNs]; queries repeat at most
// every half bound.  (Round 5 used a fixed 2 ms, which a late-visible flag turned into a 2 ms scan.)
// The floor stays above the longest normal single-scan wait (0.44 ms measured, r06c): at 150 us
// about one wait per scan queried its stream, and each query is a marker before the next kernel.
constexpr int64_t kQueryMinNs = 500000, kQueryMaxNs = 2000000;
struct WaitBound {
  double ema_ns = 0.0;
  int64_t after() const {
    return ema_ns <= 0.0 ? kQueryMaxNs : std::min<int64_t>(kQueryMaxNs, std::max<int64_t>(kQueryMinNs, (int64_t)(4.0 * ema_ns)));
  }
  void done(int64_t ns) { ema_ns = ema_ns <= 0.0 ? (double)ns : 0.875 * ema_ns + 0.125 * (double)ns; }
};

// One wait's state.  The caller polls its word; after each unanswered read it asks query_due(),
// and on true queries its stream (hipStreamQuery, the counters and the fallback are the caller's).
template <typename Clock>
struct FlagWaitT {
  long polls = 0;                 // unanswered reads of the current wait (0: none under way)
  typename Clock::time_point t0;  // start of the current wait
  int64_t next_query = 0, waited = 0;  // ns into the wait: of the next stream query, at the last clock reading

  // phase: the value polls starts from.  The clock is read when (polls & 1023) reaches 1023: on
  // every 1024th read, the first of them the (1023 - phase)th.
  void begin(const WaitBound& b, typename Clock::time_point now, long phase = 0) {
    polls = phase;
    t0 = now;
    next_query = b.after();
  }
  bool query_due() {
    if ((++polls & 1023) != 1023) return false;
    waited = ns_since(t0);
    if (waited <= next_query) return false;
    next_query = waited + std::max<int64_t>(kQueryMinNs, next_query / 2);
    return true;
  }
  // The word arrived: the wait's duration into the bound of its kind and the statistics.
  void finish(WaitBound& b) {
    b.done(waited = ns_since(t0));
    wait_stat(waited);
    polls = 0;
  }
};
using FlagWait = FlagWaitT<std::chrono::steady_clock>;

// ---- running ahead -----------------------------------------------------------------------------
// Before the host enqueues iteration `it` of a loop whose kernels publish a progress word: return
// once the device has stopped (true: enqueue nothing more) or is at most `lead` iterations behind,
// or after 2 ms (enqueue anyway: iterations past the stop return at once).  A word of another
// generation counts as no iteration seen.  Every read counts into `polls`.
template <typename Clock = std::chrono::steady_clock>
bool run_ahead(const volatile u64* flag, u64 gen, int it, int lead, std::atomic<long long>& polls) {
  const auto t0 = Clock::now();
  for (;;) {
    const u64 w = *flag;
    polls.fetch_add(1, std::memory_order_relaxed);
    const bool mine = word_of(w, gen);
    if (mine && word_stop(w)) return true;
    if (it - (mine ? word_iters(w) : 0) <= lead) return false;
    if (Clock::now() - t0 > std::chrono::milliseconds(2)) return false;
  }
}

// ---- the launch shape of a Gauss-Newton iteration ----------------------------------------------
struct GnPlanIn {
  int tail_div, grid_cap, one_grid;  // knobs::gn_tail_div, gn_grid_cap, gn_one_grid
  bool one_item, tail_one_item;      // knobs::gn_one_item, gn_tail_one_item
  int B, active, max_items;  // the sub-batch's jobs, those iterating at the latest flag read, its work-item capacity
  bool stream_mode;          // a single-scan run
  int items_hint;            // single scans: the previous scan's work items (0: none)
  int hint_n, hint_B;        // batches: the last run's work items and its job count (fbr_ctx::gn_items_hint, _B)
};
struct GnPlan {
  bool fused = false;  // the batch tail: kNN and residual in one launch
  int grid = 1;
  int one_mode = 0, rest_grid = 0;  // GnArgs::one_item (0 loop, 1 one item per workgroup and a loop launch behind, 2 one
                                    // item per workgroup) and GnArgs::rest_grid
  int adopt = -1;      // >= 0: the count is known; (adopt, B) becomes the batch hint of the next run
};

// items_known(): the run's published work-item count or -1; called (once) only where the one-item
// modes can use it, since it reads host-mapped memory.
template <typename Known>
GnPlan gn_plan(const GnPlanIn& in, Known&& items_known) {
  GnPlan p;
  const bool tail = in.tail_div > 0 && (int64_t)in.active * in.tail_div <= in.B;
  // the batch tail also one item per workgroup (the grid then covers the items of the jobs that
  // stopped too, which return at once); FBR_GN_TAIL_ONE_ITEM=0: a 1,024-workgroup loop
  const bool tail_one = tail && !in.stream_mode && in.one_item && in.tail_one_item;
  p.fused = tail;
  p.grid = std::max(1, std::min(in.max_items, tail && !tail_one ? std::min(in.grid_cap, 1024) : in.grid_cap));
  if (in.stream_mode && in.items_hint > 0) p.grid = std::min(p.grid, std::max(16, 2 * in.items_hint));
  // one-item launches: one workgroup per item once the count is known (no loop launch), before
  // that a grid of gn_one_grid workgroups and the loop launch behind it
  // (single scans: once the count is known, iteration 2 on; before that the loop over the
  // previous scan's grid, so no second launch sits on their critical path)
  const int nk = in.one_item && (!tail || tail_one || in.stream_mode) ? items_known() : -1;
  const bool one = in.one_item && (!tail || tail_one) && (!in.stream_mode || nk >= 0);
  if (!one) return p;
  if (nk >= 0) {
    p.grid = std::max(1, nk);
    p.one_mode = 2;
    p.adopt = nk;  // the next run's first grids
  } else if (in.hint_n > 0 && in.hint_B == in.B) {
    // a previous run of this many jobs: its count + 25 % + 256, and a small loop launch behind
    p.grid = std::max(1, std::min(in.max_items, in.hint_n + in.hint_n / 4 + 256));
    p.one_mode = 1;
    p.rest_grid = 64;
  } else {
    p.grid = std::max(1, std::min(in.max_items, in.one_grid));
    p.one_mode = 1;
  }
  return p;
}

}  // namespace pace
}  // namespace fbr
