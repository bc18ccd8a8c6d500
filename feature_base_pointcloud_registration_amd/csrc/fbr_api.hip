// fbr_api.hip — the extern "C" boundary (include/fbr.h): the context's life cycle, the profiling
// timers and the diagnostics.  The other entry points live with their subsystems (fbr_ctx.h lists
// the units).
#include "fbr_ctx.h"

namespace {

int64_t feat_slot_bytes(int W) {
  FeatArgs a{};
  feat_caps(W, a);
  return a.gslot_bytes;
}

int check_params(const fbr_params* p) {
  if (!p) return FBR_ERR_INVALID_ARG;
  if (p->n_scan <= 0 || p->horizon_scan <= 0 || p->horizon_scan > kMaxW) return FBR_ERR_UNSUPPORTED;
  if (p->max_points_per_scan <= 0 || p->max_batch <= 0 || p->max_iterations <= 0) return FBR_ERR_INVALID_ARG;
  if (!(p->odometry_surf_leaf_size > 0 && p->mapping_corner_leaf_size > 0 && p->mapping_surf_leaf_size > 0))
    return FBR_ERR_INVALID_ARG;
  return FBR_OK;
}

}  // namespace

namespace fbr {
namespace internal {

void timer_begin(fbr_ctx* c, hipStream_t st, const char* name, hipEvent_t* ev_end) {
  *ev_end = nullptr;
  if (!c->profiling) return;
  if (!c->profile_only.empty() && c->profile_only.count(name) == 0) return;
  KernelTimer& t = c->timers[name];
  std::pair<Event, Event> own;
  if (!t.pool.empty()) {
    own = std::move(t.pool.back());
    t.pool.pop_back();
  } else {
    (void)own.first.create(hipEventDefault);
    (void)own.second.create(hipEventDefault);
  }
  const std::pair<hipEvent_t, hipEvent_t> pr(own.first, own.second);
  t.pending.push_back(std::move(own));
  *ev_end = pr.second;
  // the launcher's kernels carry the events in their dispatches (fbr_launch, fbr_kernels.h)
  launch_timer() = LaunchTimer{pr.first, pr.second, 0};
}
void timer_end(hipStream_t st, hipEvent_t ev_end) {
  if (!ev_end) return;
  LaunchTimer& t = launch_timer();
  if (!t.launched) {  // nothing dispatched (empty input): a zero-length interval on the stream
    (void)hipEventRecord(t.start, st);
    (void)hipEventRecord(t.stop, st);
  }
  t = LaunchTimer{};
}

// LDS / scratch capacities of k_features for a Horizon_SCAN of W (fbr_feat_layout.h).
void feat_caps(int W, FeatArgs& a) {
  const featlay::Caps c = featlay::caps_of(W);
  a.lcap = c.lcap;
  a.segcap = c.segcap;
  a.kseg = c.kseg;
  a.nwcap = c.nwcap;
  a.gslot_bytes = (int64_t)features_gslot_bytes(a);
}

}  // namespace internal
}  // namespace fbr

// =============================================================================================
extern "C" {

void fbr_params_default(fbr_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_scan = 16;
  p->horizon_scan = 1800;
  p->edge_threshold = 1.0f;
  p->surf_threshold = 0.1f;
  p->edge_feature_min_valid_num = 10;
  p->surf_feature_min_valid_num = 100;
  p->odometry_surf_leaf_size = 0.4f;
  p->mapping_corner_leaf_size = 0.2f;
  p->mapping_surf_leaf_size = 0.4f;
  p->z_tollerance = 1000.0f;
  p->rotation_tollerance = 1000.0f;
  p->number_of_cores = 4;
  p->mapping_process_interval = 0.15;
  p->crop_half[0] = 30.0f;
  p->crop_half[1] = 30.0f;
  p->crop_half[2] = 10.0f;
  p->max_iterations = 30;
  p->max_points_per_scan = p->n_scan * p->horizon_scan;
  p->max_batch = 1;
}

const char* fbr_strerror(int s) {
  switch (s) {
    case FBR_OK: return "ok";
    case FBR_ERR_INVALID_ARG: return "invalid argument";
    case FBR_ERR_HIP: return "HIP runtime error";
    case FBR_ERR_NO_MAP: return "no map set (call fbr_set_map first)";
    case FBR_ERR_CAPACITY: return "input exceeds the context capacity";
    case FBR_ERR_UNSUPPORTED: return "configuration not supported by the device kernels";
    case FBR_ERR_NO_DEVICE: return "no HIP device available";
    case FBR_ERR_STATE: return "call order violated";
    case FBR_ERR_MSG: return "point cloud message rejected (not dense, or no ring field)";
    default: return "unknown status";
  }
}

int fbr_abi_version(void) { return FBR_ABI_VERSION; }

int fbr_device_count(int* count) {
  if (!count) return FBR_ERR_INVALID_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return FBR_OK;
}

int fbr_create(fbr_ctx** out, const fbr_params* p, int hip_device) {
  if (!out) return FBR_ERR_INVALID_ARG;
  *out = nullptr;
  int rc = check_params(p);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FBR_ERR_NO_DEVICE;
  if (hip_device < 0 || hip_device >= ndev) return FBR_ERR_INVALID_ARG;
  CK(hipSetDevice(hip_device));
  fbr_ctx* c = new fbr_ctx();
  c->P = *p;
  c->dev = hip_device;
  c->H = p->n_scan;
  c->W = p->horizon_scan;
  c->HW = (int64_t)c->H * c->W;
  c->Bcap = p->max_batch;
  c->NMAX = p->max_points_per_scan;
  const int nsub_env = knobs::nsub(kMaxSub);
  if (nsub_env) c->nsub_pref = nsub_env;
  // launch slots (fbr_params.pipeline_depth: 0 = the default 3)
  const int pipe = p->pipeline_depth <= 0 ? 3 : std::min(fbr_ctx::kMaxSlots, p->pipeline_depth);
  c->nslot = p->max_batch > 1 ? pipe : 1;
  // Pipelined, one sub-batch per launch is best at every batch size (the two launches in flight
  // overlap as the sub-batches did): B = 128 / 256 / 1024 give 91.8k / 96.7k / 97.4k scans/s
  // against 83.2k / 93.1k / 96.7k with 3 sub-batches (profiles/r04f_pipe_nsub_sweep.txt).  Three
  // slots (the default) against two: B = 128 / 256 96.8k / 100.1k vs 92.6k / 97.8k, B = 1024 equal
  // (profiles/r04n_mfma_pipe_cell_ab.txt).
  if (c->nslot > 1) c->nsub_pref = nsub_env ? std::min(c->nsub_pref, kMaxSub / c->nslot) : 1;
  c->Bwork = (int64_t)c->nslot * c->Bcap;
  const int64_t B = c->Bcap, Bw = c->Bwork, HW = c->HW, H = c->H;
  // streams of the sub-batches this context can use, per slot (each stream takes a hardware queue:
  // unused ones are not created, so they cannot share a queue with a busy one)
  const int nstreams = std::max(2, c->nslot * c->nsub_pref);
  bool sok = c->stream.create(hipStreamNonBlocking);
  for (int k = 0; k < nstreams && sok; ++k) {
    if (k > 0) sok = c->xstream[k].create(hipStreamNonBlocking);
    if (sok) sok = c->xev[k].create(hipEventDisableTiming);
  }
  sok = sok && c->ev_staged.create(hipEventDisableTiming) && c->ev_fork.create(hipEventDisableTiming) &&
        c->ev_ext.create(hipEventDisableTiming);
  if (!sok) {
    fbr_destroy(c);
    return FBR_ERR_HIP;
  }
  c->items_per_job = (int)(2 * ((HW + 255) / 256 + 1));
  c->max_items = (int)(Bw * c->items_per_job);
  c->vg_scratch_elems = kVgScratch * Bw * (HW + std::min<int64_t>(HW, (int64_t)kCornerPerRing * H));
  // inputs: B jobs; work arrays: Bw jobs (nslot launch slots)
  bool fail = dalloc(c->d_pts_own, B * c->NMAX) || dalloc(c->d_nin, B) || dalloc(c->d_guess, B * 6) ||
              dalloc(c->d_owner, Bw * HW) || dalloc(c->d_rowcnt, Bw * H) || dalloc(c->d_col, Bw * HW) ||
              dalloc(c->d_start, Bw * H) || dalloc(c->d_end, Bw * H) || dalloc(c->d_nvalid, Bw) ||
              dalloc(c->d_cloud, Bw * HW) || dalloc(c->d_range, Bw * HW) || dalloc(c->d_sstate, Bw) ||
              dalloc(c->d_sstream, 1) || dalloc(c->d_label, Bw * HW) || dalloc(c->d_label_stream, HW) ||
              dalloc(c->d_corner_slot, Bw * H * kCornerPerRing) || dalloc(c->d_corner_cnt, Bw * H) ||
              dalloc(c->d_surf_ring, Bw * HW) ||
              dalloc(c->d_surf_ring_cnt, Bw * H) || dalloc(c->d_ring_box, Bw * H * kRingBox) || dalloc(c->d_err, Bw) ||
              dalloc(c->d_corner_all, Bw * HW) ||
              dalloc(c->d_surf_all, Bw * HW) || dalloc(c->d_cornerDS, Bw * HW) || dalloc(c->d_surfDS, Bw * HW) ||
              dalloc(c->d_ncorner, Bw) || dalloc(c->d_nsurf, Bw) || dalloc(c->d_ncds, Bw) || dalloc(c->d_nsds, Bw) ||
              dalloc(c->d_vg_scratch, c->vg_scratch_elems) ||
              dalloc(c->d_gn, Bw) || dalloc(c->d_items, c->max_items) || dalloc(c->d_nitems, kMaxSub) ||
              dalloc(c->d_item_range, 2 * Bw) || dalloc(c->d_cropcnt, 2 * B) || dalloc(c->d_cropwork, 2 * Bw) ||
              dalloc(c->d_partial, (int64_t)c->max_items * 32) ||
              dalloc(c->d_nbr, (int64_t)c->max_items * 5 * 256) ||
              dalloc(c->d_fitc, (int64_t)c->max_items * 6 * 256) || dalloc(c->d_fits, (int64_t)c->max_items * 256) ||
              dalloc(c->d_nsame, (int64_t)c->max_items * 256) ||
              dalloc(c->d_iter_cnt, kMaxSub * 4 * std::max(1, p->max_iterations)) ||
              dalloc(c->d_feat_scratch, Bw * H * feat_slot_bytes(c->W)) ||
              c->iter_flags.alloc(kMaxSub * (std::max(1, p->max_iterations) + 1)) || dalloc(c->d_pose_out, Bw * 6) ||
              dalloc(c->d_stats, Bw) || dalloc(c->d_trace, Bw * p->max_iterations * 6 + 18) ||
              dalloc(c->d_desk_mode, B) || dalloc(c->d_rowmin, Bw * H) || dalloc(c->d_result, B) ||
              dalloc(c->d_choff, Bw * H * (c->W / 32 + 1)) ||
              dalloc(c->h_result, B) || dalloc(c->h_scan, c->NMAX) || dalloc(c->h_nin, 1) || dalloc(c->h_crop, 2) ||
              dalloc(c->h_guess, 6) || c->direct.alloc(1) || dalloc(c->d_direct_done, 1);
  if (fail) {
    fbr_destroy(c);
    return FBR_ERR_HIP;
  }
  c->d_pts = c->d_pts_own;
  c->knn_desc.assign((size_t)std::max(1, p->max_iterations), KnnLaunchDesc{});
  if (hipMemset(c->d_sstream, 0, sizeof(StreamState)) != hipSuccess ||
      hipMemset(c->d_label_stream, 0, HW) != hipSuccess || hipMemset(c->d_col, 0, sizeof(int32_t) * Bw * HW) != hipSuccess ||
      hipMemset(c->d_range, 0, sizeof(float) * Bw * HW) != hipSuccess ||
      hipMemset(c->d_desk_mode, 0, sizeof(int32_t) * B) != hipSuccess ||
      hipMemset(c->d_owner, 0x7F, sizeof(int32_t) * Bw * HW) != hipSuccess) {  // OwnerTag: refilled when the tags run out
    fbr_destroy(c);
    return FBR_ERR_HIP;
  }
  // index bits of the owner claims; tagged while at least 2^6 generations fit (scans up to 2^24 points)
  c->owner_ib = 1;
  while (((int64_t)1 << c->owner_ib) < c->NMAX) ++c->owner_ib;
  c->owner_tmax = (knobs::owner_tags() && c->owner_ib <= 24) ? ((uint32_t)kEmptyOwner >> c->owner_ib) - 1 : 0;
  if (const int cap = knobs::owner_tmax())  // tests: refill the images every few calls
    if (c->owner_tmax) c->owner_tmax = std::min<uint32_t>(c->owner_tmax, (uint32_t)cap);
  *out = c;
  return FBR_OK;
}

int fbr_destroy(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  (void)hipSetDevice(c->dev);
  // drain every stream; ~fbr_ctx then releases the buffers before the streams and events
  if (c->stream) (void)fbr_sync(c->stream);
  for (int k = 1; k < kMaxSub; ++k)
    if (c->xstream[k]) (void)fbr_sync(c->xstream[k]);
  if (c->ing.cstream) (void)fbr_sync(c->ing.cstream);
  if (c->ing.xstream) (void)fbr_sync(c->ing.xstream);
  delete c;
  return FBR_OK;
}

int fbr_debug_counters(long long* launches, long long* host_syncs, long long* flag_polls, int reset) {
  DebugCounters& d = debug_counters();
  if (launches) *launches = d.launches.load();
  if (host_syncs) *host_syncs = d.host_syncs.load();
  if (flag_polls) *flag_polls = d.flag_polls.load();
  if (reset) {
    d.launches = 0;
    d.host_syncs = 0;
    d.flag_polls = 0;
  }
  return FBR_OK;
}

// Diagnostic: host wall time (ns) of the single-scan calls since the last reset (DebugCounters).
extern "C" int fbr_diag_host_times(long long* out4, int reset) {
  DebugCounters& d = debug_counters();
  for (int k = 0; k < 4; ++k) {
    if (out4) out4[k] = d.host_ns[k].load();
    if (reset) d.host_ns[k] = 0;
  }
  return FBR_OK;
}

// Diagnostic: host waits on device results since the last reset: [0] fallbacks (a flag or a direct
// result not visible although its stream drained: the value is then read from device memory / the
// enqueued copy), [1] completed waits longer than 1 ms, [2] the longest wait (ns), [3] stream
// queries made by the waits.
extern "C" int fbr_diag_wait_stats(long long* out4, int reset) {
  DebugCounters& d = debug_counters();
  std::atomic<long long>* v[4] = {&d.flag_fallbacks, &d.waits_over_1ms, &d.wait_max_ns, &d.stream_queries};
  for (int k = 0; k < 4; ++k) {
    if (out4) out4[k] = v[k]->load();
    if (reset) *v[k] = 0;
  }
  return FBR_OK;
}

// Diagnostic: host wall time (ns) of fbr_batch_launch calls and the part of it spent waiting for
// the Gauss-Newton iteration flags, since the last reset.
extern "C" int fbr_diag_batch_times(long long* out2, int reset) {
  DebugCounters& d = debug_counters();
  for (int k = 0; k < 2; ++k) {
    if (out2) out2[k] = d.batch_ns[k].load();
    if (reset) d.batch_ns[k] = 0;
  }
  return FBR_OK;
}

// Diagnostic: what the process's contexts and communicators hold now: [0] device blocks, [1] pinned
// blocks, [2] streams, [3] events (fbr_own.h's handles; the kernels' per-device statics, the grids,
// the arena and the copy pool are not counted).  Back at its earlier value once they are destroyed.
extern "C" int fbr_diag_live_resources(long long out[4]) {
  if (!out) return FBR_ERR_INVALID_ARG;
  for (int k = 0; k < own::kLiveKinds; ++k) out[k] = own::live(k).load(std::memory_order_relaxed);
  return FBR_OK;
}

// Diagnostic: the per-ring surf filter kernel of this context's default-order launches: -1 by
// launch size (four waves per ring above 256 rings, else the 512-thread kernel), 0 the 512-thread
// kernel, 2 four waves per ring -- so a test can compare the two on the same scans.
extern "C" int fbr_diag_ring_filter(fbr_ctx* c, int kernel) {
  if (!c || (kernel != -1 && kernel != 0 && kernel != 2)) return FBR_ERR_INVALID_ARG;
  c->diag_ring_filter = kernel;
  return FBR_OK;
}

// Diagnostic (A/B and tests): force_wide 1 keeps the float4 projected cloud in the batch launches
// that would take the 12-B records (fbr_stages.hip, batch_cloud12), 0 restores the default, < 0
// leaves the switch as it is; *point_bytes (may be null) receives the record size of the last batch
// launch's cloud: 12, 16, or 0 before the first launch.
extern "C" int fbr_diag_batch_cloud(fbr_ctx* c, int force_wide, int32_t* point_bytes) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (force_wide >= 0) c->diag_wide_cloud = force_wide != 0;
  if (point_bytes) *point_bytes = c->last_cloud_bytes;
  return FBR_OK;
}

// Diagnostic (tests): the last kNN pass of the latest single-scan registration, decoded on the host
// from what the device keeps anyway: the down-sampled clouds, the work items, GnArgs::nbr and the
// transform k_gn_solve kept (GnArgs::knn_T).  The positions restate gn_knn_block's
// pointAssociateToMap in float; the library is built without contraction, so they are its bits.
extern "C" int fbr_diag_knn_last(fbr_ctx* c, int32_t* n_corner, int32_t* n_surf, float* queries, int32_t* nbr,
                                 int64_t cap, fbr_knn_desc* desc) {
  if (!c || cap < 0 || (cap && (!queries || !nbr))) return FBR_ERR_INVALID_ARG;
  if (!c->knn_last_valid) return FBR_ERR_STATE;
  CK(enter(c));
  CK(fbr_sync(c->stream));
  GnState g;
  int32_t ncs[2], range[2];
  CK(fbr_memcpy_sync(&g, c->d_gn, sizeof(g), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(&ncs[0], c->d_ncds, sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(&ncs[1], c->d_nsds, sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(range, c->d_item_range, sizeof(range), hipMemcpyDeviceToHost));
  if (n_corner) *n_corner = ncs[0];
  if (n_surf) *n_surf = ncs[1];
  const int pass = g.iter - 1;  // the job's last pass ran before its last solve
  if (desc) {
    *desc = fbr_knn_desc{};
    desc->iterations = g.iter;
    if (pass >= 0 && pass < (int)c->knn_desc.size()) {
      const KnnLaunchDesc& d = c->knn_desc[pass];
      desc->r = d.R; desc->rx = d.RX; desc->flat = d.flat; desc->sparse = d.sparse;
      desc->lpq = d.lpq; desc->fused = d.fused; desc->tiles = d.tiles;
    }
  }
  const int64_t n = (int64_t)ncs[0] + ncs[1];
  if (!cap) return FBR_OK;
  if (cap < n) return FBR_ERR_CAPACITY;
  float T[12];
  if (pass >= 0) CK(fbr_memcpy_sync(T, c->knn_T_slot(), sizeof(T), hipMemcpyDeviceToHost));
  else std::memcpy(T, g.T, sizeof(T));  // no pass ran (too few features): the guess's transform
  std::vector<float4> pts((size_t)std::max<int64_t>(n, 1));
  if (ncs[0]) CK(fbr_memcpy_sync(pts.data(), c->d_cornerDS, sizeof(float4) * ncs[0], hipMemcpyDeviceToHost));
  if (ncs[1]) CK(fbr_memcpy_sync(pts.data() + ncs[0], c->d_surfDS, sizeof(float4) * ncs[1], hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) {
    const float4 q = associate(T, pts[i]);
    queries[3 * i] = q.x;
    queries[3 * i + 1] = q.y;
    queries[3 * i + 2] = q.z;
  }
  for (int64_t i = 0; i < 5 * n; ++i) nbr[i] = -1;
  const int ni = range[1] - range[0];
  if (pass < 0 || ni <= 0) return FBR_OK;
  if (range[0] < 0 || range[1] > c->max_items) return FBR_ERR_STATE;
  std::vector<int4> items((size_t)ni);
  std::vector<int32_t> raw((size_t)ni * 5 * 256);
  CK(fbr_memcpy_sync(items.data(), c->d_items + range[0], sizeof(int4) * ni, hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(raw.data(), c->d_nbr + (int64_t)range[0] * 5 * 256, sizeof(int32_t) * raw.size(),
                     hipMemcpyDeviceToHost));
  for (int it = 0; it < ni; ++it) {
    const int4 item = items[it];  // {job, 0 corner / 1 surf, first query, queries}
    for (int slot = 0; slot < item.w && slot < 256; ++slot) {
      const int64_t q = (item.y == 0 ? 0 : ncs[0]) + item.z + slot;
      if (item.x != 0 || q < 0 || q >= n) return FBR_ERR_STATE;
      const int32_t* o = raw.data() + (size_t)it * 5 * 256 + slot;
      if (o[0] < 0) continue;
      for (int k = 0; k < 5; ++k) nbr[5 * q + k] = o[k * 256];
    }
  }
  return FBR_OK;
}

// Diagnostic (tests): the residual pass behind fbr_diag_knn_last's search, decoded the same way: the
// scan-frame point and the fit cache (GnArgs::fits / fitc / nsame) per query in that call's order, the job's work items with
// their normal-equation partials, and the transform and trig k_gn_solve kept before its step.
extern "C" int fbr_diag_gn_last(fbr_ctx* c, int32_t* n_corner, int32_t* n_surf, float* points, int8_t* fit_state,
                                float* fit, int8_t* nsame, int64_t cap, int32_t* n_items, int32_t* items,
                                double* partial, int64_t item_cap, float* T_trig) {
  if (!c || cap < 0 || item_cap < 0 || (cap && (!points || !fit_state || !fit || !nsame)) ||
      (item_cap && (!items || !partial)))
    return FBR_ERR_INVALID_ARG;
  if (!c->knn_last_valid) return FBR_ERR_STATE;
  CK(enter(c));
  CK(fbr_sync(c->stream));
  GnState g;
  int32_t ncs[2], range[2];
  CK(fbr_memcpy_sync(&g, c->d_gn, sizeof(g), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(&ncs[0], c->d_ncds, sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(&ncs[1], c->d_nsds, sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(range, c->d_item_range, sizeof(range), hipMemcpyDeviceToHost));
  const int pass = g.iter - 1;
  const int ni = pass >= 0 ? std::max(0, range[1] - range[0]) : 0;
  if (ni && (range[0] < 0 || range[1] > c->max_items)) return FBR_ERR_STATE;
  if (n_corner) *n_corner = ncs[0];
  if (n_surf) *n_surf = ncs[1];
  if (n_items) *n_items = ni;
  if (T_trig) {
    if (pass >= 0) {
      CK(fbr_memcpy_sync(T_trig, c->knn_T_slot(), sizeof(float) * 18, hipMemcpyDeviceToHost));
    } else {  // no pass ran: the guess's
      std::memcpy(T_trig, g.T, sizeof(g.T));
      std::memcpy(T_trig + 12, g.trig, sizeof(g.trig));
    }
  }
  const int64_t n = (int64_t)ncs[0] + ncs[1];
  if (!cap && !item_cap) return FBR_OK;
  if ((cap && cap < n) || (item_cap && item_cap < ni)) return FBR_ERR_CAPACITY;
  const bool fused = pass >= 0 && pass < (int)c->knn_desc.size() && c->knn_desc[pass].fused;
  if (cap) {
    std::vector<float4> pts((size_t)std::max<int64_t>(n, 1));
    if (ncs[0]) CK(fbr_memcpy_sync(pts.data(), c->d_cornerDS, sizeof(float4) * ncs[0], hipMemcpyDeviceToHost));
    if (ncs[1]) CK(fbr_memcpy_sync(pts.data() + ncs[0], c->d_surfDS, sizeof(float4) * ncs[1], hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
      points[3 * i] = pts[i].x;
      points[3 * i + 1] = pts[i].y;
      points[3 * i + 2] = pts[i].z;
      fit_state[i] = 0;
      nsame[i] = fused ? -1 : 0;
      for (int k = 0; k < 6; ++k) fit[6 * i + k] = 0.0f;
    }
  }
  if (!ni) return FBR_OK;
  std::vector<int4> its((size_t)ni);
  CK(fbr_memcpy_sync(its.data(), c->d_items + range[0], sizeof(int4) * ni, hipMemcpyDeviceToHost));
  if (item_cap) {
    std::memcpy(items, its.data(), sizeof(int4) * ni);
    CK(fbr_memcpy_sync(partial, c->d_partial + (int64_t)range[0] * 32, sizeof(double) * 32 * ni, hipMemcpyDeviceToHost));
  }
  if (!cap) return FBR_OK;
  std::vector<float> fc((size_t)ni * 6 * 256);
  std::vector<int8_t> fs((size_t)ni * 256), sm((size_t)ni * 256);
  CK(fbr_memcpy_sync(fc.data(), c->d_fitc + (int64_t)range[0] * 6 * 256, sizeof(float) * fc.size(), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(fs.data(), c->d_fits + (int64_t)range[0] * 256, fs.size(), hipMemcpyDeviceToHost));
  CK(fbr_memcpy_sync(sm.data(), c->d_nsame + (int64_t)range[0] * 256, sm.size(), hipMemcpyDeviceToHost));
  for (int it = 0; it < ni; ++it) {
    const int4 item = its[it];  // {job, 0 corner / 1 surf, first query, queries}
    for (int slot = 0; slot < item.w && slot < 256; ++slot) {
      const int64_t q = (item.y == 0 ? 0 : ncs[0]) + item.z + slot;
      if (item.x != 0 || q < 0 || q >= n) return FBR_ERR_STATE;
      fit_state[q] = fs[(size_t)it * 256 + slot];
      if (!fused) nsame[q] = sm[(size_t)it * 256 + slot];
      for (int k = 0; k < 6; ++k) fit[6 * q + k] = fc[((size_t)it * 6 + k) * 256 + slot];
    }
  }
  return FBR_OK;
}

// Diagnostic: batch job `job` of the following launches is treated as over the feature capacity
// (as if k_features had flagged it), so the tests can check how fbr_batch_results and the exported
// records report such a job (no valid scan reaches the capacity: a ring holds at most W points);
// job < 0 clears it.
extern "C" int fbr_diag_force_capacity_error(fbr_ctx* c, int job) {
  if (!c) return FBR_ERR_INVALID_ARG;
  c->diag_err_job = job < 0 ? -1 : job;
  return FBR_OK;
}

// Diagnostic: per-ring phase cycle sums of k_features (only filled by a -DFBR_FEAT_STAMPS build).
extern "C" int fbr_diag_feature_stamps(fbr_ctx* c, unsigned long long* out /* [max_batch*n_scan][12] */) {
  if (!c) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  const size_t n = (size_t)c->Bwork * c->H * 12;  // both launch slots (the first launch uses slot 0)
  if (!c->d_feat_stamps) {
    if (dalloc(c->d_feat_stamps, n)) return FBR_ERR_HIP;
    CK(hipMemset(c->d_feat_stamps, 0, sizeof(unsigned long long) * n));
    return FBR_OK;
  }
  if (out) CK(fbr_memcpy_sync(out, c->d_feat_stamps, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  return FBR_OK;
}

// Tests: which walk every segment of the k_features launches since the last call took
// (FeatArgs::paths).  The first call allocates the record; later calls copy it out ([every
// launch slot's jobs][n_scan] words, cap >= that many) and clear it.
extern "C" int fbr_diag_feature_paths(fbr_ctx* c, uint32_t* out, int64_t cap, int64_t* n_out) {
  if (!c) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  const size_t n = (size_t)c->Bwork * c->H;
  if (n_out) *n_out = (int64_t)n;
  if (!c->d_feat_paths) {
    if (dalloc(c->d_feat_paths, n)) return FBR_ERR_HIP;
    CK(hipMemset(c->d_feat_paths, 0, sizeof(uint32_t) * n));
    return FBR_OK;
  }
  if (!out) return FBR_OK;
  if (cap < (int64_t)n) return FBR_ERR_CAPACITY;
  CK(hipDeviceSynchronize());
  CK(fbr_memcpy_sync(out, c->d_feat_paths, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  CK(hipMemset(c->d_feat_paths, 0, sizeof(uint32_t) * n));
  return FBR_OK;
}

int fbr_set_profiling(fbr_ctx* c, int enable) {
  if (!c) return FBR_ERR_INVALID_ARG;
  c->profiling = enable != 0;
  return FBR_OK;
}

int fbr_set_profiling_kernels(fbr_ctx* c, const char* names) {
  if (!c) return FBR_ERR_INVALID_ARG;
  c->profile_only.clear();
  if (!names) return FBR_OK;
  std::string cur;
  for (const char* q = names;; ++q) {
    if (*q == ',' || *q == '\0') {
      if (!cur.empty()) c->profile_only.insert(cur);
      cur.clear();
      if (*q == '\0') break;
    } else {
      cur.push_back(*q);
    }
  }
  return FBR_OK;
}

int fbr_kernel_time(fbr_ctx* c, const char* kernel, double* total_ms, int64_t* launches) {
  if (!c || !kernel) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  auto itr = c->timers.find(kernel);
  if (itr == c->timers.end()) {
    if (total_ms) *total_ms = 0.0;
    if (launches) *launches = 0;
    return FBR_OK;
  }
  KernelTimer& t = itr->second;
  size_t done = 0;  // pairs read and moved to the pool; they leave `pending` on every path
  int rc = FBR_OK;
  for (; done < t.pending.size(); ++done) {
    std::pair<Event, Event>& pr = t.pending[done];
    float ms = 0.0f;
    if (!hip_ok(hipEventSynchronize(pr.second), "fbr_kernel_time") ||
        !hip_ok(hipEventElapsedTime(&ms, pr.first, pr.second), "fbr_kernel_time")) {
      rc = FBR_ERR_HIP;
      break;
    }
    t.total_ms += ms;
    t.launches += 1;
    t.pool.push_back(std::move(pr));
  }
  t.pending.erase(t.pending.begin(), t.pending.begin() + done);
  if (rc) return rc;
  if (total_ms) *total_ms = t.total_ms;
  if (launches) *launches = t.launches;
  return FBR_OK;
}

void* fbr_stream(fbr_ctx* c) { return c ? (void*)c->stream : nullptr; }

}  // extern "C"
