// fbr_scan.hip — the single-scan entry points (fbr_project*, fbr_extract_features, fbr_register*,
// fbr_process_scan / fbr_process_msg, fbr_reset_stream) and their upload path: pinned staging
// filled by a pool of host copy workers.
#include "fbr_ctx.h"

namespace {

int copy_stats(fbr_ctx* c, int B, fbr_reg_stats* stats) { return copy_results(c, B, stats, nullptr, true); }

// Host copy workers of the single-scan uploads, alive for the process (spawning threads per call
// cost ~30 us each).  run(fn) calls fn(p) on participants p = 0..kCopyWorkers (the caller is 0)
// and returns when all are done.  Idle workers spin briefly on the generation counter (back-to-back
// scans find them awake), then sleep on the condition variable.
class CopyPool {
 public:
  // + the caller: 4 host copies of a single-scan upload (7 workers and 256 KB chunks measured
  // slower: latency p50 0.72 -> 0.75 ms, profiles/r04z_latency_8_copiers.txt)
  static constexpr int kWorkers = 3;
  CopyPool() {
    for (int t = 1; t <= kWorkers; ++t) th_.emplace_back([this, t] { loop(t); });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_.store(true);
      gen_.fetch_add(1);
    }
    cv_.notify_all();
    for (auto& x : th_) x.join();
  }
  void run(const std::function<void(int)>& fn) {
    std::lock_guard<std::mutex> serial(run_mu_);  // one upload at a time (contexts may share it)
    // adaptive spin: 4x the smoothed interval between uploads, within [1 ms, spin_ns()]
    const int64_t now = std::chrono::duration_cast<std::chrono::nanoseconds>(
                            std::chrono::steady_clock::now().time_since_epoch()).count();
    if (last_run_ns_ > 0) {
      const double dt = (double)(now - last_run_ns_);
      ema_ns_ = ema_ns_ > 0.0 ? 0.8 * ema_ns_ + 0.2 * dt : dt;
      const int64_t cap = spin_ns();
      spin_cur_.store(std::min<int64_t>(cap, std::max<int64_t>(std::min<int64_t>(cap, 1000000), (int64_t)(4.0 * ema_ns_))));
    }
    last_run_ns_ = now;
    fn_ = &fn;
    pending_.store(kWorkers);
    {
      std::lock_guard<std::mutex> g(mu_);
      gen_.fetch_add(1);
    }
    cv_.notify_all();
    fn(0);
    while (pending_.load() != 0) __builtin_ia32_pause();
  }

 private:
  // The cap of the idle workers' spin after an upload (knobs::copy_spin_us says why they spin).
  static int64_t spin_ns() {
    return (int64_t)knobs::copy_spin_us() * 1000;
  }
  void loop(int id) {
    uint64_t seen = 0;
    while (true) {
      uint64_t g = gen_.load();
      const int64_t spin = spin_cur_.load();
      if (g == seen && spin > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; g == seen; ++k) {
          __builtin_ia32_pause();
          g = gen_.load();
          if ((k & 255) == 255 && ns_since(t0) > spin) break;
        }
      }
      if (g == seen) {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return gen_.load() != seen; });
        g = gen_.load();
      }
      seen = g;
      if (stop_.load()) return;
      (*fn_)(id);
      pending_.fetch_sub(1);
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_, run_mu_;
  std::condition_variable cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<int> pending_{0};
  const std::function<void(int)>* fn_ = nullptr;
  std::atomic<bool> stop_{false};
  std::atomic<int64_t> spin_cur_{spin_ns()};
  int64_t last_run_ns_ = 0;
  double ema_ns_ = 0.0;
};

CopyPool& copy_pool() {
  static CopyPool* pool = new CopyPool();  // never destroyed: workers may outlive static teardown
  return *pool;
}

// Host bytes -> pinned staging -> device, pipelined: the participants copy 512 KB chunks
// round-robin and each enqueues its chunk's DMA on `st` as soon as the chunk is staged, so the
// copy engine runs while the rest is still being copied (a 64x1800 scan is 2.6 MB).  The chunks
// are disjoint, so their order on the stream does not matter; the caller enqueues the consumer
// after this returns.
hipError_t pinned_upload_async(int dev, void* d_dst, void* h_stage, const void* src, size_t bytes, hipStream_t st) {
  constexpr size_t kChunk = 512 << 10;
  if (bytes <= kChunk) {
    std::memcpy(h_stage, src, bytes);
    return hipMemcpyAsync(d_dst, h_stage, bytes, hipMemcpyHostToDevice, st);
  }
  const size_t nchunk = (bytes + kChunk - 1) / kChunk;
  std::atomic<int> err{(int)hipSuccess};
  const std::function<void(int)> fn = [&](int p) {
    thread_local int cur_dev = -1;  // pool workers serve every context: the stream's device
    if (p > 0 && cur_dev != dev) {
      (void)hipSetDevice(dev);
      cur_dev = dev;
    }
    for (size_t k = (size_t)p; k < nchunk; k += CopyPool::kWorkers + 1) {
      const size_t b = k * kChunk, e = std::min(bytes, b + kChunk);
      std::memcpy((uint8_t*)h_stage + b, (const uint8_t*)src + b, e - b);
      const hipError_t r = hipMemcpyAsync((uint8_t*)d_dst + b, (uint8_t*)h_stage + b, e - b, hipMemcpyHostToDevice, st);
      if (r != hipSuccess) err.store((int)r);
    }
  };
  copy_pool().run(fn);
  return (hipError_t)err.load();
}

// A single scan into job slot `job` with no host synchronisation of its own: a copy from pageable
// memory returns once the runtime has staged the source, and the pinned staging buffer is only
// rewritten by the next call, after this call's results came back.
// A single-scan call at `stamp` registers (the mapping_process_interval gate, mapOptmization.h:279).
bool will_register(const fbr_ctx* c, double stamp) { return stamp - c->time_last >= c->P.mapping_process_interval; }

// The registration guess of a single-scan call, queued on the stream ahead of the scan's chunks
// (pinned, so the 24-B DMA runs while the host still copies the first chunk).
hipError_t queue_guess(fbr_ctx* c, const float* guess) {
  if (!guess) return hipSuccess;
  std::memcpy(c->h_guess, guess, sizeof(float) * 6);
  return hipMemcpyAsync(c->d_guess, c->h_guess, sizeof(float) * 6, hipMemcpyHostToDevice, c->stream);
}

int upload_scan(fbr_ctx* c, int job, const fbr_point_xyzirt* pts, int64_t n, const float* guess = nullptr) {
  if (n < 0 || n > c->NMAX) return FBR_ERR_CAPACITY;
  c->no_time_call = false;
  // staging free: a no-op after the previous call's result copy; after a direct result the stream
  // may still hold that call's no-op iterations, which read no staging buffer (the scan's DMA ran
  // before its projection), and this call's work is ordered after them
  if (c->tail_pending) c->tail_pending = false;
  else CK(fbr_sync(c->stream));
  CK(queue_guess(c, guess));
  if (n && knobs::pinned_upload()) {
    CK(pinned_upload_async(c->dev, c->d_pts + job * c->NMAX, c->h_scan, pts, sizeof(fbr_point_xyzirt) * n, c->stream));
  } else if (n) {
    CK(hipMemcpyAsync(c->d_pts + job * c->NMAX, pts, sizeof(fbr_point_xyzirt) * n, hipMemcpyHostToDevice, c->stream));
  }
  c->single_n = n;  // k_project takes it as an argument (no 8-B copy ahead of it on the stream)
  (void)job;
  return FBR_OK;
}

// The raw PointCloud2 goes to HBM as it is; k_unpack_msg writes job 0's scan buffer
// (cachePointCloud's fromROSMsg, imageProjection.cpp:253, on the device).
int upload_msg(fbr_ctx* c, const fbr_pointcloud2* msg, int32_t* msg_flags, const float* guess = nullptr) {
  MsgLayout L;
  int rc = resolve_msg(msg, &L);
  if (rc) return rc;
  if (L.n > c->NMAX) return FBR_ERR_CAPACITY;
  if (c->tail_pending) c->tail_pending = false;  // as upload_scan
  else CK(fbr_sync(c->stream));
  CK(queue_guess(c, guess));
  // nothing of the old message is kept: the old block goes first, the new one has the message's size
  if ((int64_t)L.bytes > c->d_msg.cap() && !c->d_msg.alloc((int64_t)L.bytes)) return alloc_failed();
  if ((int64_t)L.bytes > c->h_msg.cap() && !c->h_msg.alloc((int64_t)L.bytes)) return alloc_failed();
  if (L.bytes) {
    CK(pinned_upload_async(c->dev, c->d_msg, c->h_msg, msg->data, L.bytes, c->stream));
  }
  MsgDev D;
  D.n = L.n;
  D.width = L.width;
  D.row_step = L.row_step;
  D.point_step = L.point_step;
  for (int k = 0; k < kMsgFields; ++k) D.off[k] = L.off[k];
  TIMED(c, "unpack_msg", launch_unpack_msg(c->stream, c->d_msg, D, c->d_pts));
  c->single_n = L.n;
  if (msg_flags) *msg_flags = L.flags;
  c->no_time_call = (L.flags & FBR_MSG_NO_TIME) != 0;
  return FBR_OK;
}

int upload_cloud(fbr_ctx* c, float4* dst, int32_t* dcnt, const fbr_point_xyzi* src, int64_t n) {
  if (n < 0 || n > c->HW) return FBR_ERR_CAPACITY;
  if (n && !src) return FBR_ERR_INVALID_ARG;
  c->ring_box_valid = false;  // clouds from the host: the mapping DS takes their bounds from the points
  if (n) CK(hipMemcpyAsync(dst, src, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
  int32_t nn = (int32_t)n;
  CK(hipMemcpyAsync(dcnt, &nn, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  CK(fbr_sync(c->stream));
  return FBR_OK;
}

}  // namespace

extern "C" {

namespace {
// fbr_project after the scan is in job 0's buffer
int project_uploaded(fbr_ctx* c, int32_t* start_ring, int32_t* end_ring, int32_t* col_ind, float* range,
                     fbr_point_xyzi* cloud, int64_t* n_out);
// fbr_process_scan after the scan is in job 0's buffer
int process_uploaded(fbr_ctx* c, double stamp, float pose_inout[6], fbr_reg_stats* stats);
}  // namespace

int fbr_project(fbr_ctx* c, const fbr_point_xyzirt* points, int64_t n_in, int32_t* start_ring, int32_t* end_ring,
                int32_t* col_ind, float* range, fbr_point_xyzi* cloud, int64_t* n_out) {
  if (!c || (n_in && !points)) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  int rc = drop_staged_batch(c);
  if (rc) return rc;
  rc = upload_scan(c, 0, points, n_in);
  if (rc) return rc;
  return project_uploaded(c, start_ring, end_ring, col_ind, range, cloud, n_out);
}

int fbr_project_msg(fbr_ctx* c, const fbr_pointcloud2* msg, int32_t* start_ring, int32_t* end_ring, int32_t* col_ind,
                    float* range, fbr_point_xyzi* cloud, int64_t* n_out, int32_t* msg_flags) {
  if (!c || !msg) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  int rc = drop_staged_batch(c);
  if (rc) return rc;
  rc = upload_msg(c, msg, msg_flags);
  if (rc) return rc;
  return project_uploaded(c, start_ring, end_ring, col_ind, range, cloud, n_out);
}

namespace {
int project_uploaded(fbr_ctx* c, int32_t* start_ring, int32_t* end_ring, int32_t* col_ind, float* range,
                     fbr_point_xyzi* cloud, int64_t* n_out) {
  int rc = stage_project(c, single_sub(c));
  if (rc) return rc;
  int32_t n = 0;
  CK(hipMemcpyAsync(&n, c->d_nvalid, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  if (start_ring) CK(fbr_memcpy_sync(start_ring, c->d_start, sizeof(int32_t) * c->H, hipMemcpyDeviceToHost));
  if (end_ring) CK(fbr_memcpy_sync(end_ring, c->d_end, sizeof(int32_t) * c->H, hipMemcpyDeviceToHost));
  if (col_ind && n) CK(fbr_memcpy_sync(col_ind, c->d_col, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (range && n) CK(fbr_memcpy_sync(range, c->d_range, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (cloud && n) CK(fbr_memcpy_sync(cloud, c->d_cloud, sizeof(float4) * n, hipMemcpyDeviceToHost));
  if (n_out) *n_out = n;
  c->have_projection = true;
  return FBR_OK;
}
}  // namespace

int fbr_extract_features(fbr_ctx* c, int8_t* label, fbr_point_xyzi* corner, int64_t* n_corner, fbr_point_xyzi* surf,
                         int64_t* n_surf) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (!c->have_projection) return FBR_ERR_STATE;
  CK(enter(c));
  int rc = stage_features(c, single_sub(c), true, false, true);
  if (rc) return rc;
  rc = check_err(c, 1);
  if (rc) return rc;
  int32_t n = 0, nc = 0, ns = 0;
  CK(fbr_memcpy_sync(&n, c->d_nvalid, sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(&nc, c->d_ncorner, sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(&ns, c->d_nsurf, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (label && n) CK(fbr_memcpy_sync(label, c->d_label_stream, (size_t)n, hipMemcpyDeviceToHost));
  if (corner && nc) CK(fbr_memcpy_sync(corner, c->d_corner_all, sizeof(float4) * nc, hipMemcpyDeviceToHost));
  if (surf && ns) CK(fbr_memcpy_sync(surf, c->d_surf_all, sizeof(float4) * ns, hipMemcpyDeviceToHost));
  if (n_corner) *n_corner = nc;
  if (n_surf) *n_surf = ns;
  return FBR_OK;
}

int fbr_register_trace(fbr_ctx* c, const fbr_point_xyzi* corner, int64_t n_corner, const fbr_point_xyzi* surf,
                       int64_t n_surf, float pose_inout[6], fbr_reg_stats* stats, float* trace) {
  if (!c || !pose_inout) return FBR_ERR_INVALID_ARG;
  if (!c->has_map) return FBR_ERR_NO_MAP;
  CK(enter(c));
  int rc = drop_staged_batch(c);
  if (!rc) rc = upload_cloud(c, c->d_corner_all, c->d_ncorner, corner, n_corner);
  if (!rc) rc = upload_cloud(c, c->d_surf_all, c->d_nsurf, surf, n_surf);
  if (rc) return rc;
  CK(hipMemcpyAsync(c->d_guess, pose_inout, sizeof(float) * 6, hipMemcpyHostToDevice, c->stream));
  CK(hipMemsetAsync(c->d_nvalid, 0, sizeof(int32_t), c->stream));
  CK(hipMemsetAsync(c->d_err, 0, sizeof(int32_t), c->stream));  // no feature stage in this call
  rc = stage_register(c, single_sub(c), trace != nullptr);
  if (rc) return rc;
  CK(hipMemcpyAsync(pose_inout, c->d_pose_out, sizeof(float) * 6, hipMemcpyDeviceToHost, c->stream));
  if (trace)
    CK(hipMemcpyAsync(trace, c->d_trace, sizeof(float) * 6 * c->P.max_iterations, hipMemcpyDeviceToHost, c->stream));
  fbr_reg_stats st;
  rc = copy_stats(c, 1, &st);
  if (rc) return rc;
  c->stream_degenerate = st.degenerate;
  st.n_points = 0;
  st.n_corner = (int32_t)n_corner;
  st.n_surf = (int32_t)n_surf;
  if (stats) *stats = st;
  return FBR_OK;
}

int fbr_register(fbr_ctx* c, const fbr_point_xyzi* corner, int64_t n_corner, const fbr_point_xyzi* surf,
                 int64_t n_surf, float pose_inout[6], fbr_reg_stats* stats) {
  return fbr_register_trace(c, corner, n_corner, surf, n_surf, pose_inout, stats, nullptr);
}

int fbr_process_scan(fbr_ctx* c, const fbr_point_xyzirt* points, int64_t n_in, double stamp, float pose_inout[6],
                     fbr_reg_stats* stats) {
  if (!c || !pose_inout || (n_in && !points)) return FBR_ERR_INVALID_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  CK(enter(c, true));
  int rc = drop_staged_batch(c);
  if (rc) return rc;
  rc = upload_scan(c, 0, points, n_in, will_register(c, stamp) ? pose_inout : nullptr);
  if (rc) return rc;
  host_time(0, t0);
  rc = process_uploaded(c, stamp, pose_inout, stats);
  host_time(3, t0);
  return rc;
}

int fbr_process_msg(fbr_ctx* c, const fbr_pointcloud2* msg, double stamp, float pose_inout[6], fbr_reg_stats* stats,
                    int32_t* msg_flags) {
  if (!c || !msg || !pose_inout) return FBR_ERR_INVALID_ARG;
  CK(enter(c, true));
  int rc = drop_staged_batch(c);
  if (rc) return rc;
  rc = upload_msg(c, msg, msg_flags, will_register(c, stamp) ? pose_inout : nullptr);
  if (rc) return rc;
  return process_uploaded(c, stamp, pose_inout, stats);
}

namespace {
// The scan is already queued into job slot 0.  Everything up to the pose runs on the stream with
// no host round trip (the features' capacity error is checked with the results); one packed copy
// and one synchronisation return pose and stats.
int process_uploaded(fbr_ctx* c, double stamp, float pose_inout[6], fbr_reg_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  c->crop_join = false;
  const bool run = stamp - c->time_last >= c->P.mapping_process_interval;  // mapOptmization.h:279
  if (run && !c->has_map) return FBR_ERR_NO_MAP;
  int rc = FBR_OK;
  if (run) {
    // the guess went to the device ahead of the scan (queue_guess); the CropBox statistics, which
    // depend only on it, run on a side stream forked here, beside the front end, and copy_results
    // joins them
    CK(hipEventRecord(c->ev_fork, c->stream));
    CK(hipStreamWaitEvent(c->xstream[1], c->ev_fork, 0));
    rc = crop_stats(c, Sub{0, 1, 0, c->xstream[1], true});
    if (rc) return rc;
    CK(hipMemcpyAsync(c->h_crop, c->d_cropcnt, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, c->xstream[1]));
    c->crop_join = true;
  }
  rc = stage_project(c, single_sub(c));
  if (!rc) rc = stage_features(c, single_sub(c), true, true);
  if (rc) return rc;
  c->have_projection = true;
  fbr_reg_stats st;
  std::memset(&st, 0, sizeof(st));
  float pose[6];
  if (run) {
    c->crop_cached = true;
    c->direct_gen = knobs::direct_results() ? (c->direct_gen_seq = c->direct_gen_seq % 0x7fffffff + 1) : 0;
    rc = stage_register(c, single_sub(c), false);
    c->crop_cached = false;
    if (rc) {
      c->direct_gen = 0;
      return rc;
    }
  }
  host_time(1, t0);
  rc = copy_results(c, 1, &st, pose, run);
  c->direct_gen = 0;
  if (rc) return rc;  // capacity error: the pose stays the guess, the time gate is not consumed
  if (run) {
    c->time_last = stamp;
    for (int k = 0; k < 6; ++k) pose_inout[k] = pose[k];
    c->stream_degenerate = st.degenerate;
    c->items_hint = (st.n_corner_ds + 255) / 256 + (st.n_surf_ds + 255) / 256;  // 256-query items (k_gn_init)
  }
  if (stats) *stats = st;
  return FBR_OK;
}
}  // namespace

int fbr_reset_stream(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  CK(hipMemsetAsync(c->d_sstream, 0, sizeof(StreamState), c->stream));
  CK(hipMemsetAsync(c->d_label_stream, 0, c->HW, c->stream));
  CK(hipMemsetAsync(c->d_col, 0, sizeof(int32_t) * c->HW, c->stream));
  CK(hipMemsetAsync(c->d_range, 0, sizeof(float) * c->HW, c->stream));
  CK(fbr_sync(c->stream));
  c->time_last = -1.0;
  c->have_projection = false;
  c->stream_degenerate = 0;
  return FBR_OK;
}

}  // extern "C"
