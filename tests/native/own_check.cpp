// own_check.cpp — the semantics of csrc/fbr_own.h's handles over a counting malloc / free policy.
//
// A stand-alone program (tests/test_resources.py builds it with -fsanitize=address,undefined and
// runs it): it prints "own_check: ok" and exits 0, or names the first check that failed and exits 1.
// The growable form is checked against its stated rule, ncap = max(need, 2 cap + 1024), the old
// block kept on every failure and released only after the copy step succeeded.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "fbr_own.h"

using namespace fbr::own;

namespace {

struct Heap {
  static long live, allocs, fail_at;  // fail_at: the allocation (counted from 1) that fails, 0 = none
  static std::map<void*, int> released;     // block -> times released
  static std::vector<std::pair<char, void*>> log;  // 'a' / 'r' in order
  static void reset(long fail = 0) {
    allocs = 0;
    fail_at = fail;
    released.clear();
    log.clear();
  }
  static void* alloc(size_t bytes) {
    if (++allocs == fail_at) return nullptr;
    void* p = std::malloc(bytes);
    if (!p) return nullptr;
    ++live;
    released[p] = 0;
    log.emplace_back('a', p);
    return p;
  }
  static void release(void* p) {
    --live;
    ++released[p];
    log.emplace_back('r', p);
    std::free(p);
  }
  static bool each_released_once() {
    for (const auto& kv : released)
      if (kv.second != 1) return false;
    return true;
  }
  static int times_released(void* p) { return released.count(p) ? released[p] : -1; }
};
long Heap::live = 0, Heap::allocs = 0, Heap::fail_at = 0;
std::map<void*, int> Heap::released;
std::vector<std::pair<char, void*>> Heap::log;

// a stream / event stand-in: a pointer-like raw handle with create and release
struct Tok {};
struct TokPolicy {
  static long live;
  static bool fail;
  static bool create(Tok** t, unsigned flags) {
    if (fail || flags == 99u) return false;
    *t = new Tok();
    ++live;
    return true;
  }
  static void release(Tok* t) {
    --live;
    delete t;
  }
};
long TokPolicy::live = 0;
bool TokPolicy::fail = false;

using Arr = Owned<int, Heap>;
using Grow = Growable<int, Heap>;
using Handle = Unique<Tok*, TokPolicy>;

static_assert(!std::is_copy_constructible<Arr>::value && !std::is_copy_assignable<Arr>::value, "Owned copies");
static_assert(!std::is_copy_constructible<Grow>::value && !std::is_copy_assignable<Grow>::value, "Growable copies");
static_assert(!std::is_copy_constructible<Handle>::value && !std::is_copy_assignable<Handle>::value, "Unique copies");
static_assert(std::is_move_constructible<Arr>::value && std::is_move_assignable<Arr>::value, "Owned moves");
static_assert(std::is_convertible<Arr, int*>::value && std::is_convertible<Grow, int*>::value, "converts to T*");
static_assert(std::is_convertible<Handle, Tok*>::value, "converts to the raw handle");

int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "own_check: line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

void alloc_and_destruct() {
  Heap::reset();
  {
    Arr a, z;
    CHECK(!a && a.get() == nullptr);
    CHECK(a.alloc(10) && a);
    int* raw = a;  // implicit conversion; the use sites index and offset through it
    raw[9] = 7;
    CHECK(a[9] == 7 && *(a + 9) == 7);
    CHECK(z.alloc(0) && z.get() != nullptr);  // a count of 0: one element
    z[0] = 1;
    CHECK(Heap::live == 2);
    a.reset();
    CHECK(!a && Heap::live == 1 && Heap::times_released(raw) == 1);
    a.reset();  // empty: nothing to release
    CHECK(Heap::times_released(raw) == 1);
    CHECK(a.alloc(3) && a.alloc(4));  // alloc over a held block releases it first
    CHECK(Heap::live == 2);
  }
  CHECK(Heap::live == 0 && Heap::each_released_once());
  Heap::reset(1);
  {
    Arr a;
    CHECK(!a.alloc(5) && !a);  // a failed allocation leaves the handle empty
  }
  CHECK(Heap::live == 0);
}

void moves() {
  Heap::reset();
  {
    Arr a;
    CHECK(a.alloc(4));
    int* pa = a;
    Arr b(std::move(a));
    CHECK(!a && b.get() == pa && Heap::live == 1);
    Arr c;
    CHECK(c.alloc(2));
    int* pc = c;
    c = std::move(b);  // onto a non-empty handle: its block goes, once
    CHECK(!b && c.get() == pa && Heap::times_released(pc) == 1 && Heap::times_released(pa) == 0);
    CHECK(Heap::live == 1);
    Arr& self = c;
    c = std::move(self);
    CHECK(c.get() == pa && Heap::times_released(pa) == 0);
    Grow g;
    CHECK(g.alloc(8) && g.cap() == 8);
    int* pg = g;
    Grow h(std::move(g));
    CHECK(!g && g.cap() == 0 && h.get() == pg && h.cap() == 8);
    Grow k;
    CHECK(k.alloc(1));
    k = std::move(h);
    CHECK(!h && h.cap() == 0 && k.get() == pg && k.cap() == 8);
  }
  CHECK(Heap::live == 0 && Heap::each_released_once());
  {
    Handle s, t;
    CHECK(s.create(0u) && s && TokPolicy::live == 1);
    Tok* raw = s;
    Handle u(std::move(s));
    CHECK(!s && u.get() == raw);
    CHECK(t.create(0u));
    t = std::move(u);
    CHECK(!u && t.get() == raw && TokPolicy::live == 1);
    CHECK(!t.create(99u) && !t && TokPolicy::live == 0);  // a failed create leaves it empty
  }
  CHECK(TokPolicy::live == 0);
}

const auto copy_ok = [](int* dst, const int* src, int64_t keep) {
  if (keep > 0) std::memcpy(dst, src, sizeof(int) * keep);
  return true;
};

// A handle of capacity `cap` (reached by exact allocation), first `keep` elements numbered.
void fill(Grow& g, int64_t cap, int64_t keep) {
  if (cap > 0) CHECK(g.alloc(cap) && g.cap() == cap);
  for (int64_t i = 0; i < keep; ++i) g[i] = (int)(1000 + i);
}
bool kept(const Grow& g, int64_t keep) {
  for (int64_t i = 0; i < keep; ++i)
    if (g[i] != (int)(1000 + i)) return false;
  return true;
}

void growable() {
  for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)1024, (int64_t)5000}) {
    for (int64_t need : {cap + 1, 10 * cap + 7}) {
      const int64_t want = std::max<int64_t>(need, 2 * cap + 1024);  // the rule
      const int64_t keep = cap / 2;
      {  // no growth when need <= cap
        Heap::reset();
        Grow g;
        fill(g, cap, keep);
        int* p = g;
        long calls = 0;
        CHECK(g.grow(cap, keep, [&](int*, const int*, int64_t) { return ++calls, true; }));
        CHECK(g.grow(cap / 2, keep, copy_ok));
        CHECK(g.get() == p && g.cap() == cap && calls == 0);
      }
      CHECK(Heap::live == 0 && Heap::each_released_once());
      {  // growth by the rule, keep elements survive, old block released after the new one exists
        Heap::reset();
        Grow g;
        fill(g, cap, keep);
        int* old = g;
        int* seen_dst = nullptr;
        int64_t seen_keep = -1;
        bool old_alive_in_copy = false;
        CHECK(g.grow(need, keep, [&](int* dst, const int* src, int64_t n) {
          seen_dst = dst;
          seen_keep = n;
          old_alive_in_copy = src == old && (!old || Heap::times_released(old) == 0);
          return copy_ok(dst, src, n);
        }));
        CHECK(g.cap() == want && g.get() == seen_dst && g.get() != nullptr && kept(g, keep));
        CHECK(seen_keep == (old ? keep : 0) && old_alive_in_copy);
        g[want - 1] = 5;  // the whole capacity is there (the sanitizer checks the bound)
        if (old) {
          CHECK(Heap::times_released(old) == 1);
          size_t ia = 0, ir = 0;
          for (size_t i = 0; i < Heap::log.size(); ++i) {
            if (Heap::log[i] == std::make_pair('a', (void*)g.get())) ia = i;
            if (Heap::log[i] == std::make_pair('r', (void*)old)) ir = i;
          }
          CHECK(ia < ir);
        }
        CHECK(Heap::live == 1);
      }
      CHECK(Heap::live == 0 && Heap::each_released_once());
      {  // the allocation fails: old pointer, capacity and contents intact, nothing leaked
        Heap::reset();
        Grow g;
        fill(g, cap, keep);
        int* old = g;
        Heap::fail_at = Heap::allocs + 1;
        long calls = 0;
        CHECK(!g.grow(need, keep, [&](int*, const int*, int64_t) { return ++calls, true; }));
        CHECK(calls == 0 && g.get() == old && g.cap() == cap && kept(g, keep));
        CHECK(Heap::live == (old ? 1 : 0) && (!old || Heap::times_released(old) == 0));
        CHECK(g.grow(need, keep, copy_ok) && g.cap() == want && kept(g, keep));  // and it can grow later
      }
      CHECK(Heap::live == 0 && Heap::each_released_once());
      {  // the copy step fails: the same, and the new block is released
        Heap::reset();
        Grow g;
        fill(g, cap, keep);
        int* old = g;
        int* fresh = nullptr;
        CHECK(!g.grow(need, keep, [&](int* dst, const int*, int64_t) {
          fresh = dst;
          return false;
        }));
        CHECK(fresh && Heap::times_released(fresh) == 1);
        CHECK(g.get() == old && g.cap() == cap && kept(g, keep));
        CHECK(Heap::live == (old ? 1 : 0) && (!old || Heap::times_released(old) == 0));
      }
      CHECK(Heap::live == 0 && Heap::each_released_once());
    }
  }
}

// The shape of a set-up that allocates in a chain and leaves at the first failure.
struct Five {
  Handle s;
  Arr a, b;
  Grow g;
  Owned<double, Heap> d;
  Arr e;
  bool init() {
    return s.create(0u) && a.alloc(3) && b.alloc(0) && g.alloc(7) && d.alloc(2) && e.alloc(1);
  }
};

void five_handles() {
  for (long k = 0; k <= 5; ++k) {
    Heap::reset(k);
    {
      Five f;
      CHECK(f.init() == (k == 0));
      if (k) {  // what ingest_init does after a failed ingest_setup: back to the empty state
        f = Five{};
        CHECK(!f.s && !f.a && !f.b && !f.g && !f.d && !f.e && Heap::live == 0 && TokPolicy::live == 0);
        Heap::fail_at = 0;
        CHECK(f.init());  // and the next call starts over
      }
    }
    CHECK(Heap::live == 0 && TokPolicy::live == 0 && Heap::each_released_once());
  }
}

void counters() {
  for (int k = 0; k < kLiveKinds; ++k) CHECK(live(k).load() == 0);
  live_add(kLiveEvent, 2);
  live_add(kLiveEvent, -1);
  CHECK(live(kLiveEvent).load() == 1 && live(kLiveDevice).load() == 0);
  live_add(kLiveEvent, -1);
}

}  // namespace

int main() {
  alloc_and_destruct();
  moves();
  growable();
  five_handles();
  counters();
  if (failures) {
    std::fprintf(stderr, "own_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::puts("own_check: ok");
  return 0;
}
