// fbr_own.h — owning handles for what the host units allocate: arrays, streams, events.
//
// Host-only and free of HIP headers, as fbr_knobs.h is: the handles take what they own from a
// policy (fbr_ctx.h holds the HIP ones; tests/native/own_check.cpp a counting malloc), so the
// semantics are checked on a CPU with sanitizers.
//
//   Unique<H, P>     one pointer-like raw handle H, released exactly once by P::release(H): in the
//                    destructor or in reset().  Move-only; a moved-from handle is empty.  Converts
//                    implicitly to H, so a use site reads as it would over the raw handle.
//                    create(args...) goes to P::create(&h, args...) (streams, events).
//   Owned<T, Mem>    an array of T from Mem::alloc(bytes) (null on failure) / Mem::release(p).
//   Growable<T, Mem> an Owned array with its capacity, grown by grow()'s rule.
//
// The namespace is hidden: nothing of it is exported from the library.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace fbr {
namespace own __attribute__((visibility("hidden"))) {

// Live resources of the process (fbr_diag_live_resources): the HIP policies count up on a
// successful allocation / create and down on a release.
enum { kLiveDevice = 0, kLivePinned = 1, kLiveStream = 2, kLiveEvent = 3, kLiveKinds = 4 };
inline std::atomic<long long>& live(int kind) {
  static std::atomic<long long> n[kLiveKinds];
  return n[kind];
}
inline void live_add(int kind, long long d) { live(kind).fetch_add(d, std::memory_order_relaxed); }

template <typename H, typename P>
class Unique {
 public:
  Unique() = default;
  Unique(const Unique&) = delete;
  Unique& operator=(const Unique&) = delete;
  Unique(Unique&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Unique& operator=(Unique&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  ~Unique() { reset(); }

  void reset() {
    if (h_) P::release(h_);
    h_ = nullptr;
  }
  // Releases what it held; true on success, empty after a failure.
  template <typename... A>
  bool create(A... args) {
    reset();
    if (!P::create(&h_, args...)) h_ = nullptr;
    return h_ != nullptr;
  }
  operator H() const { return h_; }
  H get() const { return h_; }

 protected:
  H h_ = nullptr;
};

template <typename Mem>
struct MemRelease {
  static void release(void* p) { Mem::release(p); }
};

template <typename T, typename Mem>
class Owned : public Unique<T*, MemRelease<Mem>> {
 public:
  // Releases what it held; true on success, empty after a failure.  A count of 0 allocates one element.
  bool alloc(size_t count) { return alloc_bytes(sizeof(T) * (count ? count : 1)); }
  bool alloc_bytes(size_t bytes) {
    this->reset();
    this->h_ = static_cast<T*>(Mem::alloc(bytes));
    return this->h_ != nullptr;
  }
  T* operator->() const { return this->h_; }
};

template <typename T, typename Mem>
class Growable {
 public:
  Growable() = default;
  Growable(Growable&& o) noexcept : p_(std::move(o.p_)), cap_(o.cap_) { o.cap_ = 0; }
  Growable& operator=(Growable&& o) noexcept {
    p_ = std::move(o.p_);
    cap_ = o.cap_;
    if (this != &o) o.cap_ = 0;
    return *this;
  }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  int64_t cap() const { return cap_; }
  void reset() {
    p_.reset();
    cap_ = 0;
  }
  // Exactly `count` elements in place of the old block, which is released first.
  bool alloc(int64_t count) {
    reset();
    if (!p_.alloc((size_t)count)) return false;
    cap_ = count;
    return true;
  }
  // Room for `need` elements, in a new block of max(need, 2 cap + 1024) when need > cap.
  // copy(dst, src, keep) moves the first `keep` elements over (keep is 0 without an old block) and
  // returns once they have arrived; only then is the old block released.  On a failed allocation or
  // copy the new block is released, the old block and capacity stay as they were, false is returned.
  template <typename Copy>
  bool grow(int64_t need, int64_t keep, Copy&& copy) {
    if (need <= cap_) return true;
    const int64_t ncap = std::max<int64_t>(need, cap_ * 2 + 1024);
    Owned<T, Mem> q;
    if (!q.alloc((size_t)ncap)) return false;
    if (!copy(q.get(), (const T*)p_.get(), p_ ? std::max<int64_t>(keep, 0) : 0)) return false;
    p_ = std::move(q);
    cap_ = ncap;
    return true;
  }

 private:
  Owned<T, Mem> p_;
  int64_t cap_ = 0;
};

}  // namespace own
}  // namespace fbr
