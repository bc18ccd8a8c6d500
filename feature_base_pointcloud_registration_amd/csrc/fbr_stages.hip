// fbr_stages.hip — the device pipeline's host side: the launch glue of each stage, the
// Gauss-Newton run driver (its flag wait and launch plan are fbr_pace.h's), and the copy of the results.
//
// One fbr_ctx = one HIP device + one stream + the HBM buffers for a batch of up to max_batch
// scans.  A batch runs entirely on the device:
//   memset owners -> k_project -> k_rowcount/k_compact        (imageProjection.cpp:583-670)
//   -> k_features (per ring) -> k_voxel_grid (per ring surf)  (featureExtraction.h:109-294)
//   -> k_concat -> k_voxel_grid x2 (downsampleCurrentScan)    (mapOptmization.h:981-993)
//   -> k_gn_init -> [k_gn_knn -> k_gn_residual -> k_gn_solve] x max_iter
//                                                             (mapOptmization.h:1403-1442)
//   -> k_gn_finalize                                          (transformUpdate, :1444-1479)
// with no host round trip between stages (converged jobs drop out on the device).
#include "fbr_ctx.h"

// Every completed wait into the process-wide wait statistics (fbr_diag_wait_stats).  (Global, not
// file-local: it is among the symbols the library's link exports, and that list is kept as it is.)
void wait_stat(int64_t ns) {
  DebugCounters& d = debug_counters();
  if (ns > 1000000) d.waits_over_1ms.fetch_add(1, std::memory_order_relaxed);
  long long m = d.wait_max_ns.load(std::memory_order_relaxed);
  while (ns > m && !d.wait_max_ns.compare_exchange_weak(m, ns, std::memory_order_relaxed)) {
  }
}

// ---------------------------------------------------------------------------------------------
// pipeline stages
// ---------------------------------------------------------------------------------------------
// Sub-batches (struct Sub, fbr_ctx.h) share the context's buffers without overlapping: the stages offset
// every per-job work array by j0 and every input array by in0.

namespace {

// The next owner generation of a projection call.  When the tags run out, every owner image is
// refilled once the device is idle (a call of the previous tag may still be running on another stream).
int next_owner_tag(fbr_ctx* c, OwnerTag* ot) {
  if (!c->owner_tmax) {
    *ot = OwnerTag{0u, 0x7FFFFFFFu, true};
    return FBR_OK;
  }
  if (c->owner_gen >= c->owner_tmax) {
    CK(hipDeviceSynchronize());
    CK(hipMemset(c->d_owner, 0x7F, sizeof(int32_t) * (int64_t)c->Bwork * c->HW));
    CK(hipDeviceSynchronize());
    c->owner_gen = 0;
  }
  const uint32_t g = ++c->owner_gen;
  *ot = OwnerTag{(((uint32_t)kEmptyOwner >> c->owner_ib) - g) << c->owner_ib, (1u << c->owner_ib) - 1u, false};
  return FBR_OK;
}

GnArgs gn_args(fbr_ctx* c, const Sub& sb, bool trace) {
  const int64_t j0 = sb.j0, HW = c->HW, ib = j0 * c->items_per_job;
  const int mi = std::max(1, c->P.max_iterations);
  GnArgs a{};
#ifdef FBR_KNN_STATS
  a.knn_stats = knn_stats_buffer();
#endif
  a.B = sb.B;
  a.max_iter = c->P.max_iterations;
  a.cornerDS = c->d_cornerDS + j0 * HW;
  a.capc = HW;
  a.ncds = c->d_ncds + j0;
  a.surfDS = c->d_surfDS + j0 * HW;
  a.caps = HW;
  a.nsds = c->d_nsds + j0;
  a.mc = c->grid_c.view();
  a.ms = c->grid_s.view();
  a.gn = c->d_gn + j0;
  a.guess = c->d_guess + (int64_t)sb.in0 * 6;
  a.items = c->d_items + ib;
  a.nitems = c->d_nitems + sb.k;
  a.item_range = c->d_item_range + j0 * 2;
  a.partial = c->d_partial + ib * 32;
  a.max_items = sb.B * c->items_per_job;
  a.edge_min = c->P.edge_feature_min_valid_num;
  a.surf_min = c->P.surf_feature_min_valid_num;
  for (int k = 0; k < 3; ++k) a.crop_half[k] = c->P.crop_half[k];
  a.rot_tol = c->P.rotation_tollerance;
  a.z_tol = c->P.z_tollerance;
  a.pose_out = c->d_pose_out + j0 * 6;
  a.stats = c->d_stats + j0;
  a.trace = trace ? c->d_trace + j0 * c->P.max_iterations * 6 : nullptr;
  a.nbr = c->d_nbr + ib * 5 * 256;
  a.fitc = c->d_fitc + ib * 6 * 256;
  a.fits = c->d_fits + ib * 256;
  a.nsame = c->d_nsame + ib * 256;
  a.fit_cache = knobs::fit_cache();
  a.iter_flags = c->iter_flags.dev() + (int64_t)sb.k * mi;
  a.items_flag = c->iter_flags.dev() + (int64_t)kMaxSub * mi + sb.k;  // after every sub-batch's iteration flags
  a.iter_cnt = c->d_iter_cnt + (int64_t)sb.k * 4 * mi;  // [2 * mi] solve, [mi] queued, [mi] blocks
  if (c->d_bin) {
    const int64_t slots = (int64_t)c->max_items * 256;
    a.fb_list = c->d_fb_list + ib * 256;
    a.bin_list = c->d_fb_list + slots + ib * 256;
    a.qblk = c->d_fb_list + 2 * slots + ib * 256;
    a.bin = c->d_bin + (int64_t)sb.k * 3 * c->bin_nb;
    a.nb_c = (int)c->bin_nb_c;
    a.nb_s = (int)(c->bin_nb - c->bin_nb_c);
  }
  a.desk_mode = c->desk_any ? c->d_desk_mode + sb.in0 : nullptr;
  a.desk = c->desk_any ? c->d_desk + sb.in0 : nullptr;
  a.nocrop = c->map_nocrop ? 1 : 0;
  a.deg_carry = sb.stream_mode ? c->stream_degenerate : 0;
  if (c->direct_gen && sb.stream_mode && sb.B == 1 && c->direct) {
    a.direct = c->direct.dev();
    a.direct_done = c->d_direct_done;
    a.direct_gen = c->direct_gen;
    a.nvalid = c->d_nvalid + j0;
    a.ncorner = c->d_ncorner + j0;
    a.nsurf = c->d_nsurf + j0;
    a.ferr = c->d_err + j0;
    a.cropcnt = c->d_cropcnt + (int64_t)sb.in0 * 2;
  }
  if (sb.stream_mode && sb.B == 1 && sb.j0 == 0) a.knn_T = c->knn_T_slot();  // fbr_diag_knn_last
  return a;
}

// The run's work-item count once iteration 0's solve has published it (GnArgs::items_flag), else -1.
int items_known(fbr_ctx* c, const GnRun& r, const GnSubRun& s) {
  if (!c->iter_flags) return -1;
  const int mi = std::max(1, c->P.max_iterations);
  const volatile unsigned long long* f = c->iter_flags.host() + (int64_t)kMaxSub * mi + s.sub.k;
  const unsigned long long v = *f;
  return word_of(v, r.gen) ? (int)word_count(v) : -1;
}

// The flag s.it needs, k_gn_solve's count of `lag` iterations before.  *ready: it is visible
// (block: wait for it); then s.active is that count, and s.live is cleared at 0.
int await_flag(fbr_ctx* c, const GnRun& r, GnSubRun& s, bool block, bool* ready) {
  const Sub& sb = s.sub;
  const int mi = std::max(1, c->P.max_iterations), i = s.it - r.lag;
  WaitBound& bound = c->wait_bound[sb.stream_mode ? kWaitScanFlag : kWaitBatchFlag];
  volatile unsigned long long* f = c->iter_flags.host() + (int64_t)sb.k * mi + i;
  unsigned long long v = *f;
  const auto tspin = std::chrono::steady_clock::now();
  if (s.wait.polls == 0) s.wait.begin(bound, tspin);
  while (!word_of(v, r.gen)) {
    if (s.wait.query_due()) {
      debug_counters().stream_queries.fetch_add(1, std::memory_order_relaxed);
      const hipError_t q = hipStreamQuery(sb.st);
      if (q != hipSuccess && q != hipErrorNotReady) return FBR_ERR_HIP;
      if (q == hipSuccess && !word_of(v = *f, r.gen)) {
        // the stream drained but the host-mapped flag is not visible: the solve's count is in
        // device memory (iter_cnt[2 i]), final once the stream is idle; read it and go on
        // watching (round 5 enqueued every remaining iteration here)
        int32_t cnt = 0;
        if (hipMemcpyAsync(&cnt, s.a.iter_cnt + 2 * i, sizeof(cnt), hipMemcpyDeviceToHost, sb.st) != hipSuccess ||
            fbr_sync(sb.st) != hipSuccess)
          return FBR_ERR_HIP;
        v = pack_count(r.gen, (uint32_t)cnt);
        debug_counters().flag_fallbacks.fetch_add(1, std::memory_order_relaxed);
        break;
      }
    }
    if (!block) break;
    v = *f;
  }
  *ready = word_of(v, r.gen);
  if (*ready) s.wait.finish(bound);  // the wait's duration, from its first poll
  if (block || *ready || !s.watch) debug_counters().batch_ns[1].fetch_add(ns_since(tspin), std::memory_order_relaxed);
  if (!*ready) return FBR_OK;  // not yet (non-blocking pass)
  debug_counters().flag_polls.fetch_add(1, std::memory_order_relaxed);
  s.active = (int)word_count(v);
  if (s.active == 0) s.live = false;
  return FBR_OK;
}

// Iteration s.it of a sub-batch in the plan's shape: kNN, residual (the batch tail: both in one
// launch), solve.  In one-item mode 1 the one-item launch and the loop launch behind it are timed
// apart (rocprof: k_gn_knn / k_gn_loop_*).
void enqueue_iteration(fbr_ctx* c, const GnRun& r, GnSubRun& s, const GnPlan& p) {
  const hipStream_t st = s.sub.st;
  const int it = s.it, part = p.one_mode == 1 ? 1 : 0;
  GnArgs a1 = s.a;
  a1.one_item = p.one_mode;
  a1.rest_grid = p.rest_grid;
  auto parts = [&](const char* name, auto launch) {
    a1.one_part = part;
    TIMED_ON(c, st, name, launch());
    if (!part) return;
    a1.one_part = 2;
    TIMED_ON(c, st, "gn_loop", launch());
  };
  parts("gn_knn", [&] { launch_gn_knn(st, a1, p.grid, it, p.fused); });
  if (!p.fused) parts("gn_residual", [&] { launch_gn_residual(st, a1, p.grid); });  // (whole runs fused: 4 % slower, r06b)
  if (c->knn_last_valid && it < (int)c->knn_desc.size()) c->knn_desc[it] = knn_launch_desc();  // fbr_diag_knn_last
  TIMED_ON(c, st, "gn_solve", launch_gn_solve(st, s.a, it, r.gen));
  s.it = it + 1;
}

// Enqueue the rest of a run, waiting for its flags.
int gn_run_finish(fbr_ctx* c, GnRun& r) {
  while (r.pending) {
    bool p = false;
    const int rc = gn_run_pass(c, r, true, &p);
    if (rc) return rc;
  }
  return FBR_OK;
}

// The Gauss-Newton iterations of sub-batches enqueued to the end (single-scan calls).
int register_iterate(fbr_ctx* c, const Sub* subs, int nsub, bool trace) {
  GnRun r;
  gn_run_start(c, r, subs, nsub, trace);
  return gn_run_finish(c, r);
}

// A single scan's direct result (GnArgs::direct): spin on its generation word; false when the
// stream drained without it (then the caller takes the enqueued path).
int wait_direct(fbr_ctx* c, bool* got) {
  volatile int32_t* gen = &c->direct.host()->pad;
  *got = false;
  WaitBound& bound = c->wait_bound[kWaitDirect];
  FlagWait w;
  w.begin(bound, std::chrono::steady_clock::now(), -1);  // phase -1: the clock is read on the 1024th poll, not the 1023rd
  while (*gen != c->direct_gen) {
    if (w.query_due()) {
      debug_counters().stream_queries.fetch_add(1, std::memory_order_relaxed);
      const hipError_t q = hipStreamQuery(c->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return FBR_ERR_HIP;
      if (q == hipSuccess && *gen != c->direct_gen) {  // the caller copies the enqueued results
        debug_counters().flag_fallbacks.fetch_add(1, std::memory_order_relaxed);
        wait_stat(w.waited);
        return FBR_OK;
      }
    }
    __builtin_ia32_pause();
  }
  w.finish(bound);
  std::atomic_thread_fence(std::memory_order_acquire);
  std::memcpy(c->h_result, (const void*)c->direct.host(), sizeof(JobResult));
  *got = true;
  return FBR_OK;
}

}  // namespace

namespace fbr {
namespace internal {

// The single-scan sub-batch: job slot 0 on the primary stream, stream mode (the state the
// reference's stage objects keep between scans is carried between calls).
Sub single_sub(fbr_ctx* c) { return Sub{0, 1, 0, c->stream, true}; }

// The per-ring surf filter's launch selection of a sub-batch (the fields launch_voxel_ring decides by).
static VgRing ring_filter_choice(fbr_ctx* c, const Sub& sb) {
  VgRing v{};
  v.B = sb.B;
  v.H = c->H;
  v.cap = c->W;
  v.dbg = knobs::vr_dbg();
  v.exact = c->P.exact_voxel_order ? 1 : 0;
  v.kernel = c->diag_ring_filter;
  return v;
}

// Whether the call's extraction reads the points' `time`: an IMU table or a field-timed motion on
// some job, and a cloud that has the field.  Such launches need the 24-B scans.
static bool reads_point_time(const fbr_ctx* c) { return (c->desk_any || c->mot_field_any) && !c->no_time_call; }

// Whether a sub-batch's projected cloud is Pt3 records (fbr_kernels.h).  Only where every reader of
// the launch takes them and the fourth word is the constant 0: 16-B scan records (so no deskew that reads a
// point's time, no intensity), not stream mode (fbr_project / fbr_extract_features hand the float4 cloud out), and
// the four-wave per-ring filter (the exact-order and 512-thread kernels read float4).  stage_project
// and stage_features of one launch both decide by this, from state that does not change between them.
static bool batch_cloud12(fbr_ctx* c, const Sub& sb) {
  if (sb.stream_mode || c->diag_wide_cloud) return false;
  if (reads_point_time(c) || !c->staged_pk) return false;  // (stage_project's pk)
  return vr_takes_four_waves(ring_filter_choice(c, sb));
}

int stage_project(fbr_ctx* c, const Sub& sb) {
  const int64_t j0 = sb.j0, i0 = sb.in0;
  DeskArgs desk{nullptr, nullptr, nullptr};
  const bool timed = reads_point_time(c);
  if (timed || c->mot_col_any) {  // deskewFlag == -1 without a "time" field (:296-297, :548)
    desk = DeskArgs{c->d_desk_mode + i0, c->d_desk ? c->d_desk + i0 : nullptr, c->d_rowmin + j0 * c->H};
    desk.motion = c->d_motion ? c->d_motion + i0 : nullptr;
    desk.no_time = c->no_time_call ? 1 : 0;
    desk.col_motion = timed ? 0 : 1;
  }
  // batch jobs read the 16-B device records when the staged batch has them and nothing reads a
  // point's time (no deskew, or column-timed motions only)
  const float4* pk = (!sb.stream_mode && !timed && c->staged_pk) ? c->staged_pk + i0 * c->NMAX : nullptr;
  if (!sb.stream_mode && !pk && !c->staged_24) return FBR_ERR_STATE;  // deskew tables set after a 16-B upload
  int32_t* owner = c->d_owner + j0 * c->HW;
  OwnerTag ot;
  const int trc = next_owner_tag(c, &ot);
  if (trc) return trc;
  const bool c12 = pk && batch_cloud12(c, sb);
  if (!sb.stream_mode) c->last_cloud_bytes = c12 ? (int)sizeof(Pt3) : (int)sizeof(float4);
  TIMED_ON(c, sb.st, "project", launch_project(sb.st, c->d_pts + i0 * c->NMAX, c->d_nin + i0, c->NMAX, sb.B, c->H,
                                               c->W, owner, c->d_err + j0, sb.stream_mode ? c->single_n : -1, pk, ot));
  TIMED_ON(c, sb.st, "extract",
           launch_extract(sb.st, c->d_pts + i0 * c->NMAX, c->NMAX, owner, sb.B, c->H, c->W, c->d_rowcnt + j0 * c->H,
                          c->d_choff + j0 * c->H * (c->W / 32 + 1),
                          c->d_cloud + j0 * c->HW, c->d_col + j0 * c->HW, c->d_range + j0 * c->HW,
                          c->d_start + j0 * c->H, c->d_end + j0 * c->H, c->d_nvalid + j0, desk, pk, ot, c12));
  return FBR_OK;
}

// err_clear: stage_project has just cleared the jobs' feature-capacity flags (k_project).
// labels_out: cloudLabel is an output of the call (fbr_extract_features), so every surf walk runs
// whole; otherwise only the picks that reach something observable are resolved (FeatArgs).
int stage_features(fbr_ctx* c, const Sub& sb, bool stream_mode, bool err_clear, bool labels_out) {
  const int64_t j0 = sb.j0, HW = c->HW, H = c->H;
  FeatArgs a{};
  a.B = sb.B;
  a.H = c->H;
  a.W = c->W;
  a.cloud = c->d_cloud + j0 * HW;
  a.c12 = !stream_mode && batch_cloud12(c, sb) ? 1 : 0;
  a.col = c->d_col + j0 * HW;
  a.range = c->d_range + j0 * HW;
  a.start_ring = c->d_start + j0 * H;
  a.end_ring = c->d_end + j0 * H;
  a.nvalid = c->d_nvalid + j0;
  a.edge_thr = c->P.edge_threshold;
  a.surf_thr = c->P.surf_threshold;
  if (stream_mode) {
    a.stream = c->d_sstream;
    a.label = c->d_label_stream;
  } else {
    CK(hipMemsetAsync(c->d_sstate + j0, 0, sizeof(StreamState) * sb.B, sb.st));
    a.stream = c->d_sstate + j0;
    a.label = c->d_label + j0 * HW;
  }
  a.corner_slot = c->d_corner_slot + j0 * H * kCornerPerRing;
  a.corner_cnt = c->d_corner_cnt + j0 * H;
  a.err = c->d_err + j0;
  a.surf_full = labels_out || !knobs::feat_surf_window() ? 1 : 0;
  a.carry = stream_mode ? 1 : 0;
  a.fresh = stream_mode ? 0 : 1;
  feat_caps(c->W, a);
  a.gscratch = c->d_feat_scratch + j0 * H * a.gslot_bytes;
  a.stamps = c->d_feat_stamps ? c->d_feat_stamps + j0 * H * 12 : nullptr;
  a.compact = knobs::feat_compact() ? 1 : 0;
  a.surf_win = knobs::feat_surf_win();
  a.paths = c->d_feat_paths ? c->d_feat_paths + j0 * H : nullptr;
  if (!err_clear) CK(hipMemsetAsync(c->d_err + j0, 0, sizeof(int32_t) * sb.B, sb.st));
  TIMED_ON(c, sb.st, "features", launch_features(sb.st, a));
  if (!stream_mode && c->diag_err_job >= sb.in0 && c->diag_err_job < sb.in0 + sb.B)
    CK(hipMemsetD32Async((hipDeviceptr_t)(c->d_err + j0 + (c->diag_err_job - sb.in0)), 1, 1, sb.st));
  VgRing v{};
  v.cloud = a.cloud;
  v.label = a.label;
  v.start_ring = a.start_ring;
  v.end_ring = a.end_ring;
  v.B = sb.B;
  v.H = c->H;
  v.HW = HW;
  v.cap = c->W;
  v.leaf = c->P.odometry_surf_leaf_size;
  v.out = c->d_surf_ring + j0 * HW;
  v.stride_out = c->W;
  v.cnt_out = c->d_surf_ring_cnt + j0 * H;
  v.dbg = knobs::vr_dbg();
  v.exact = c->P.exact_voxel_order ? 1 : 0;
  v.stamps = a.stamps;
  v.kernel = c->diag_ring_filter;
  v.c12 = a.c12;
  TIMED_ON(c, sb.st, "voxel_ring", launch_voxel_ring(sb.st, v));
  TIMED_ON(c, sb.st, "concat",
           launch_concat(sb.st, sb.B, c->H, c->W, a.corner_slot, a.corner_cnt, v.out, v.cnt_out,
                         c->d_corner_all + j0 * HW, HW, c->d_ncorner + j0, c->d_surf_all + j0 * HW, HW,
                         c->d_nsurf + j0, c->d_ring_box + j0 * H * kRingBox));
  c->ring_box_valid = true;
  return FBR_OK;
}

int crop_stats(fbr_ctx* c, const Sub& sb) {
  GnArgs a = gn_args(c, sb, false);
  int32_t* cnt = c->d_cropcnt + (int64_t)sb.in0 * 2;
  if (c->map_nocrop) {  // keyframe local map: laserCloud*FromMapDSNum = the whole DS map
    std::vector<int32_t> v(2 * sb.B);
    for (int j = 0; j < sb.B; ++j) {
      v[2 * j] = (int32_t)c->grid_c.g.n_points;
      v[2 * j + 1] = (int32_t)c->grid_s.g.n_points;
    }
    CK(hipMemcpyAsync(cnt, v.data(), sizeof(int32_t) * 2 * sb.B, hipMemcpyHostToDevice, sb.st));
    CK(fbr_sync(sb.st));
    return FBR_OK;
  }
  TIMED_ON(c, sb.st, "crop", launch_crop_count(sb.st, a, c->grid_c.pts, c->grid_c.g.n_points, c->grid_s.pts,
                                                c->grid_s.g.n_points, c->d_cropwork + (int64_t)sb.j0 * 2, cnt));
  return FBR_OK;
}

// downsampleCurrentScan (mapOptmization.h:981-993) + the Gauss-Newton set-up of a sub-batch.
int register_prepare(fbr_ctx* c, const Sub& sb, bool trace) {
  const int64_t j0 = sb.j0, HW = c->HW;
  // corner and surf filters in one launch; Morton voxel order (internal clouds: spatially compact
  // query order for the kNN waves)
  VgArgs v{};
  const int64_t ccap = std::min<int64_t>(HW, (int64_t)kCornerPerRing * c->H);
  v.s[0] = VgSet{c->d_surf_all + j0 * HW, HW, c->d_nsurf + j0, HW, c->d_surfDS + j0 * HW, HW, c->d_nsds + j0,
                 c->d_vg_scratch + j0 * kVgScratch * HW, c->P.mapping_surf_leaf_size, sb.B, 1, c->P.exact_voxel_order ? 1 : 0};
  v.s[1] = VgSet{c->d_corner_all + j0 * HW, HW, c->d_ncorner + j0, ccap, c->d_cornerDS + j0 * HW, HW, c->d_ncds + j0,
                 c->d_vg_scratch + c->Bwork * kVgScratch * HW + j0 * kVgScratch * ccap, c->P.mapping_corner_leaf_size,
                 sb.B, 1, c->P.exact_voxel_order ? 1 : 0};
  if (c->ring_box_valid) {  // the clouds' bounds from k_concat: the filter reads each cloud twice, not 3 times
    const float* rb = c->d_ring_box + j0 * c->H * kRingBox;
    for (int k = 0; k < 2; ++k) {
      v.s[k].box = rb + (k == 0 ? 6 : 0);  // set 0 = surf (box floats 6-11), set 1 = corner (0-5)
      v.s[k].box_n = c->H;
      v.s[k].box_stride = (int64_t)c->H * kRingBox;
    }
  }
  v.err = c->d_err + j0;  // a failed split look-back flags the job (FBR_REG_FEATURE_CAPACITY / error)
  TIMED_ON(c, sb.st, "voxel_scan", launch_voxel_grid(sb.st, v));
  GnArgs a = gn_args(c, sb, trace);
  if (trace) CK(hipMemsetAsync(a.trace, 0, sizeof(float) * sb.B * c->P.max_iterations * 6, sb.st));
  TIMED_ON(c, sb.st, "gn_init", launch_gn_init(sb.st, a));  // also zeroes a.iter_cnt
  // map-in-box statistics (from the kNN grid, every launch; the single-scan path runs them on a side
  // stream beside its front end, the keyframe map's are host constants set at staging)
  if (!c->crop_cached) {
    const int rc = crop_stats(c, sb);
    if (rc) return rc;
  }
  return FBR_OK;
}

void gn_run_start(fbr_ctx* c, GnRun& r, const Sub* subs, int nsub, bool trace) {
  r = GnRun{};
  r.pending = true;
  r.trace = trace;
  r.nsub = nsub;
  r.gen = ++c->gn_gen;
  r.lag = knobs::gn_lag();
  c->knn_last_valid = nsub == 1 && subs[0].stream_mode && subs[0].B == 1 && subs[0].j0 == 0;
  for (int k = 0; k < nsub; ++k) {
    r.s[k] = GnSubRun{subs[k], gn_args(c, subs[k], trace), /*live*/ true, /*watch*/ (bool)c->iter_flags, /*done*/ false,
                      /*active*/ subs[k].B};
  }
}

// One pass over the run's sub-batches: each enqueues its next iteration if the flag it needs is
// visible (block: wait for it).  A sub-batch whose jobs all stopped, or that reached
// max_iterations, gets its transformUpdate.  *progress: something was enqueued.
int gn_run_pass(fbr_ctx* c, GnRun& r, bool block, bool* progress) {
  bool all_done = true;
  for (int k = 0; k < r.nsub; ++k) {
    GnSubRun& s = r.s[k];
    if (s.done) continue;
    const Sub& sb = s.sub;
    if (s.live && s.it < c->P.max_iterations && s.watch && s.it >= r.lag) {
      bool ready = false;
      const int rc = await_flag(c, r, s, block, &ready);
      if (rc) return rc;
      if (!ready) {
        all_done = false;
        continue;
      }
    }
    if (!s.live || s.it >= c->P.max_iterations) {
      if (!s.a.direct) TIMED_ON(c, sb.st, "gn_finalize", launch_gn_finalize(sb.st, s.a));
      CK(hipEventRecord(c->xev[sb.k], sb.st));  // the sub-batch's last work (batch_quiesce joins it)
      s.done = true;
      *progress = true;
      continue;
    }
    all_done = false;
    const GnPlanIn in{knobs::gn_tail_div(), knobs::gn_grid_cap(), knobs::gn_one_grid(), knobs::gn_one_item(),
                      knobs::gn_tail_one_item(), sb.B, s.active, s.a.max_items, sb.stream_mode, c->items_hint,
                      c->gn_items_hint, c->gn_items_hint_B};
    const GnPlan p = gn_plan(in, [&] { return items_known(c, r, s); });
    if (p.adopt >= 0) {
      c->gn_items_hint = p.adopt;
      c->gn_items_hint_B = sb.B;
    }
    enqueue_iteration(c, r, s, p);
    *progress = true;
  }
  if (all_done) r.pending = false;
  return FBR_OK;
}

// Advance the batch launches in flight together (non-blocking passes; spin while neither can
// progress) until run[target] is fully enqueued (target -1: every run).
int advance_runs(fbr_ctx* c, int target) {
  auto busy = [&] {
    if (target >= 0) return c->run[target].pending;
    for (int q = 0; q < fbr_ctx::kMaxSlots; ++q)
      if (c->run[q].pending) return true;
    return false;
  };
  auto tw = std::chrono::steady_clock::now();
  bool waiting = false;
  while (busy()) {
    bool p = false;
    for (int s = 0; s < fbr_ctx::kMaxSlots; ++s)
      if (c->run[s].pending) {
        const int rc = gn_run_pass(c, c->run[s], false, &p);
        if (rc) return rc;
      }
    if (p && waiting) {
      debug_counters().batch_ns[1].fetch_add(ns_since(tw), std::memory_order_relaxed);
      waiting = false;
    } else if (!p && !waiting) {
      waiting = true;
      tw = std::chrono::steady_clock::now();
    }
    if (!p) __builtin_ia32_pause();
  }
  return FBR_OK;
}

// Every batch launch fully enqueued, and the primary stream ordered after all of them (on the
// device): the caller may then overwrite the inputs or use job slot 0 on the primary stream.
int batch_quiesce(fbr_ctx* c) {
  const int rc = advance_runs(c, -1);
  if (rc) return rc;
  for (int s = 0; s < fbr_ctx::kMaxSlots; ++s)
    for (int k = 0; k < c->run[s].nsub; ++k)
      if (c->run[s].s[k].sub.st != c->stream) CK(hipStreamWaitEvent(c->stream, c->xev[c->run[s].s[k].sub.k], 0));
  return FBR_OK;
}

// Registration of the clouds in d_corner_all / d_surf_all (counts d_ncorner / d_nsurf) from d_guess.
int stage_register(fbr_ctx* c, const Sub& sb, bool trace) {
  if (!c->has_map) return FBR_ERR_NO_MAP;
  int rc = register_prepare(c, sb, trace);
  if (!rc) rc = register_iterate(c, &sb, 1, trace);
  return rc;
}

// Per-job results of the last B jobs, packed on the device and returned by one copy (then one
// host synchronisation): poses (when poses_out), stats, and the features' capacity errors
// (FBR_ERR_UNSUPPORTED if any job has one).  with_reg = false: the registration was gated off.
int copy_results(fbr_ctx* c, int B, fbr_reg_stats* stats, float* poses_out, bool with_reg, int64_t w0, bool per_job) {
  const auto tw = std::chrono::steady_clock::now();
  bool direct = false;
  if (c->direct_gen && with_reg && B == 1 && w0 == 0 && !per_job) {
    const int rc = wait_direct(c, &direct);
    if (rc) return rc;
    // the stream may still run the no-op iterations enqueued ahead of the last flag (tail_pending)
    if (direct) c->tail_pending = true;
    else TIMED(c, "gn_finalize", launch_gn_finalize(c->stream, gn_args(c, single_sub(c), false)));
  }
  if (!direct) {
    launch_pack_results(c->stream, B, with_reg ? 1 : 0, c->d_pose_out + w0 * 6, c->d_stats + w0, c->d_nvalid + w0,
                        c->d_ncorner + w0, c->d_nsurf + w0, c->d_cropcnt, c->d_err + w0, per_job ? c->d_guess : nullptr,
                        c->d_result);
    CK(hipMemcpyAsync(c->h_result, c->d_result, sizeof(JobResult) * B, hipMemcpyDeviceToHost, c->stream));
    CK(fbr_sync(c->stream));
  }
  if (c->crop_join) {  // the single-scan CropBox statistics: their own copy on the side stream (no
    c->crop_join = false;  // cross-stream dependency on the device; that stream finished long ago)
    CK(fbr_sync(c->xstream[1]));
    c->h_result[0].st.n_corner_map = c->h_crop[0];
    c->h_result[0].st.n_surf_map = c->h_crop[1];
  }
  host_time(2, tw);
  // Single scans: a capacity error (features truncated) fails the call before anything is written
  // (pose_inout keeps the guess, as the reference leaves the pose on a failed scan).  Batches: the
  // failed jobs carry FBR_REG_FEATURE_CAPACITY and their guesses (k_pack_results), the rest their
  // results.
  if (!per_job)
    for (int j = 0; j < B; ++j)
      if (c->h_result[j].err) return FBR_ERR_UNSUPPORTED;
  if (with_reg) {
    c->last_iters.resize(B);
    c->last_q.resize(B);
    c->last_n.resize(B);
    c->last_m.resize(B);
  }
  for (int j = 0; j < B; ++j) {
    const JobResult& r = c->h_result[j];
    if (with_reg) {
      c->last_iters[j] = r.st.iterations;
      c->last_q[j] = r.st.n_corner_ds + r.st.n_surf_ds;
      c->last_n[j] = r.st.n_points;
      c->last_m[j] = r.st.n_corner_map + r.st.n_surf_map;
    }
    if (stats) stats[j] = r.st;
    if (poses_out && with_reg)
      for (int k = 0; k < 6; ++k) poses_out[6 * j + k] = r.pose[k];
  }
  return FBR_OK;
}

int check_err(fbr_ctx* c, int B) {
  std::vector<int32_t> e(B);
  CK(hipMemcpyAsync(e.data(), c->d_err, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
  CK(fbr_sync(c->stream));
  for (int j = 0; j < B; ++j)
    if (e[j]) return FBR_ERR_UNSUPPORTED;
  return FBR_OK;
}

}  // namespace internal
}  // namespace fbr
