// fbr_ctx.h — internal to the host units (fbr_*.hip): the context behind include/fbr.h's opaque
// fbr_ctx, the small helpers every unit uses, and the few functions that cross units.
//
//   fbr_api.hip     life cycle (fbr_create's allocations, the drain before ~fbr_ctx), profiling timers, diagnostics
//   fbr_stages.hip  per-stage launch glue, the Gauss-Newton run driver, results
//   fbr_scan.hip    single-scan entry points, their upload path and copy-worker pool
//   fbr_batch.hip   batch stage / launch / export state machine, the pinned-ring ingest
//   fbr_comm.hip    RCCL communicator and pose gather
//   fbr_map.hip     map VoxelGrid and kNN grids, keyframe store and local map, pose helpers
//   fbr_loop.hip    loop closure candidate search and ICP
//   fbr_sc.hip      scan-context place recognition: descriptor store, search, loop closure under drift
//   fbr_pg.hip      pose graph: the factor list, the Levenberg-Marquardt driver, correctPoses
//   fbr_gmap.hip    global map: build from the keyframe store, get, install, save
//   fbr_score.hip   pose scoring: a scan against the map at many poses, the lattice search
//   fbr_reg_info.hip  registration information: the normal matrix and covariance of poses and batch jobs
//
// and the headers free of HIP, each checked on a CPU by a program under tests/native:
//   fbr_knobs.h     the environment knobs
//   fbr_own.h       owning handles (HostWord below builds on them)
//   fbr_pace.h      device-paced host loops: the flag words, the flag wait, run_ahead, gn_plan
//   fbr_loop_plan.h chunks and pool layout of loop closure for many keyframe pairs
//
// Everything shared lives in fbr::internal, which is hidden: the library's link exports every
// default-visibility symbol, and none of this is part of its interface.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "fbr_common.h"
#include "fbr_imu.h"
#include "fbr_kernels.h"
#include "fbr_motion.h"
#include "fbr_knobs.h"
#include "fbr_msg.h"
#include "fbr_own.h"
#include "fbr_pace.h"

using namespace fbr;

#define CK(x)                                                                        \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      fprintf(stderr, "fbr: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return FBR_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)

namespace fbr {
namespace internal __attribute__((visibility("hidden"))) {

// Host wall time since t0 into DebugCounters::host_ns[k] (fbr_diag_host_times).
inline void host_time(int k, std::chrono::steady_clock::time_point t0) {
  debug_counters().host_ns[k].fetch_add((long long)pace::ns_since(t0), std::memory_order_relaxed);
}

// Blocking host synchronisations, counted (fbr_debug_counters).
inline hipError_t fbr_sync(hipStream_t s) {
  debug_counters().host_syncs.fetch_add(1, std::memory_order_relaxed);
  return hipStreamSynchronize(s);
}
inline hipError_t fbr_memcpy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  debug_counters().host_syncs.fetch_add(1, std::memory_order_relaxed);
  return hipMemcpy(dst, src, bytes, kind);
}

// ---- the HIP policies of fbr_own.h's handles; they keep the live-resource counts ----
inline bool hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) fprintf(stderr, "fbr: HIP error %s in %s\n", hipGetErrorString(e), what);
  return e == hipSuccess;
}
struct DeviceMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    own::live_add(own::kLiveDevice, 1);
    return p;
  }
  static void release(void* p) {
    (void)hipFree(p);
    own::live_add(own::kLiveDevice, -1);
  }
};
template <unsigned Flags>  // hipHostMallocDefault or hipHostMallocMapped
struct PinnedMem {
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, Flags) != hipSuccess) return nullptr;
    own::live_add(own::kLivePinned, 1);
    return p;
  }
  static void release(void* p) {
    (void)hipHostFree(p);
    own::live_add(own::kLivePinned, -1);
  }
};
struct StreamPolicy {
  static bool create(hipStream_t* s, unsigned flags) {
    if (!hip_ok(hipStreamCreateWithFlags(s, flags), "hipStreamCreateWithFlags")) return false;
    own::live_add(own::kLiveStream, 1);
    return true;
  }
  static void release(hipStream_t s) {
    (void)hipStreamDestroy(s);
    own::live_add(own::kLiveStream, -1);
  }
};
struct EventPolicy {
  static bool create(hipEvent_t* e, unsigned flags) {
    if (!hip_ok(hipEventCreateWithFlags(e, flags), "hipEventCreateWithFlags")) return false;
    own::live_add(own::kLiveEvent, 1);
    return true;
  }
  static void release(hipEvent_t e) {
    (void)hipEventDestroy(e);
    own::live_add(own::kLiveEvent, -1);
  }
};
template <typename T>
using Dev = own::Owned<T, DeviceMem>;
template <typename T>
using GrowDev = own::Growable<T, DeviceMem>;
template <typename T>
using Pinned = own::Owned<T, PinnedMem<hipHostMallocDefault>>;
template <typename T>
using GrowPinned = own::Growable<T, PinnedMem<hipHostMallocDefault>>;
template <typename T>
using Mapped = own::Owned<T, PinnedMem<hipHostMallocMapped>>;  // host-mapped: the device writes it
using Stream = own::Unique<hipStream_t, StreamPolicy>;
using Event = own::Unique<hipEvent_t, EventPolicy>;

// A handle's alloc() failed where that is an error (the memory policies themselves are quiet: a
// caller with a fallback stays silent): report the runtime's error.
inline int alloc_failed() {
  (void)hip_ok(hipPeekAtLastError(), "an allocation");
  return FBR_ERR_HIP;
}

// `count` elements (at least one) of device or pinned memory, by the handle's type.
template <typename T, typename Mem>
int dalloc(own::Owned<T, Mem>& p, size_t count) {
  return p.alloc(count) ? FBR_OK : alloc_failed();
}

// A host-mapped block the device writes and the host polls, zero-filled, with its device address.
template <typename T>
class HostWord {
 public:
  int alloc(size_t count) {
    if (!h_.alloc(count)) return alloc_failed();
    std::memset(h_.get(), 0, sizeof(T) * std::max<size_t>(count, 1));
    if (hip_ok(hipHostGetDevicePointer((void**)&d_, h_.get(), 0), "hipHostGetDevicePointer")) return FBR_OK;
    h_.reset();
    return FBR_ERR_HIP;
  }
  explicit operator bool() const { return h_ != nullptr; }
  T* host() const { return h_; }
  T* dev() const { return d_; }  // not owning: host()'s device address

 private:
  Mapped<T> h_;
  T* d_ = nullptr;
};

// Grow a device array to hold `need` elements (keeping `keep` of them): own::Growable's rule, with
// the copy on `st` and its sync as the step the old block has to outlive.
template <typename T>
int grow(GrowDev<T>& g, int64_t need, int64_t keep, hipStream_t st) {
  const bool ok = g.grow(need, keep, [st](T* dst, const T* src, int64_t n) {
    if (n > 0 && !hip_ok(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToDevice, st), "grow")) return false;
    return hip_ok(fbr_sync(st), "grow");
  });
  return ok ? FBR_OK : FBR_ERR_HIP;
}

// Timed launches' event pairs (timing enabled), reused through the pool.
struct KernelTimer {
  std::vector<std::pair<Event, Event>> pending;
  std::vector<std::pair<Event, Event>> pool;
  double total_ms = 0.0;
  int64_t launches = 0;
};

}  // namespace internal
}  // namespace fbr
using namespace fbr::internal;
using namespace fbr::pace;

constexpr int kMaxSub = 8;  // sub-batch streams per launch (FBR_NSUB); more than 3 pays only with
                             // GPU_MAX_HW_QUEUES above HIP's default of 4 (one hardware queue per stream)

// Host ingest of fbr_process_batch: the caller's (pageable) scans are packed into a ring of pinned
// staging chunks by host threads and copied to HBM on a copy stream, into the input slot the
// running device batch does not read; batch k+1's upload overlaps batch k's compute.
// Empty (no copy stream) until ingest_init has set all of it up; streams and events stand before
// the buffers, so they are destroyed after them.
struct __attribute__((visibility("hidden"))) Ingest {
  static constexpr int kChunks = 4;
  Stream cstream;
  Stream xstream;                    // k_expand_scans, off the copy stream (FBR_INGEST_XSTREAM=0: on it)
  Event copied_ev;                   // the copies of the current upload are done (on cstream)
  Event up_ev[2];                    // the upload of input slot s is complete (on xstream / cstream)
  Event chunk_ev[kChunks];           // the copies out of chunk k are complete
  bool chunk_used[kChunks] = {};
  int next_chunk = 0;
  Pinned<uint8_t> h_stage;           // kChunks x chunk_bytes
  int64_t chunk_bytes = 0;
  Dev<fbr_point_xyzirt> d_pts1;          // input slot 1's scan buffer
  fbr_point_xyzirt* d_pts_slot[2] = {};  // not owning: slot 0 = the context's d_pts_own, slot 1 = d_pts1
  int nthreads = 8;                  // packing threads per chunk
  double h2d_bytes = 0.0;            // bytes copied host -> device by the last fbr_process_batch
  // Compact records (no deskew tables set: `time` is never read): per scan the x, y, z planes
  // (f32) and the rings (u8 below 256 rings), 13 B per point instead of 24, expanded on the device
  // by k_expand_scans (the batch returns poses and statistics, which no point's intensity or time
  // reaches).
  Dev<uint8_t> d_stage[2];           // per input slot: [Bcap][ingest_region_bytes(NMAX)] (one per
                                     // slot, so slot s's expand overlaps slot s^1's copies)
  Dev<int64_t> d_nin;                // [2][2][Bcap] per input slot: the staged scans' point counts,
                                     // then their records' byte offsets in d_stage (copy stream)
  Pinned<int64_t> h_nin;             // [2][2][Bcap]
  bool compact_used = false;         // the last fbr_process_batch used compact records
  bool pk_slot[2] = {};              // input slot s holds 16-B device records (launch_expand_scans pk)
};

// A contiguous sub-batch of jobs driven on one stream.  j0 is the first job of the sub-batch's
// work buffers (every per-job intermediate array, and the Gauss-Newton work-item arrays at
// j0 * items_per_job); in0 the first job of its inputs (raw scans, counts, guesses, deskew tables,
// CropBox statistics).  A batch launch in work slot s has j0 = s * max_batch + in0, so two launches
// in flight never share intermediates.  k indexes the sub-batch's GN flags / counters.
struct Sub {
  int j0, B, k;  // first work job, job count, GN flag index (< kMaxSub)
  hipStream_t st;
  bool stream_mode = false;  // single-scan call (carries stream state) vs independent batch jobs
  int in0 = 0;               // first input job
};

// The Gauss-Newton iterations of one launch that the host has still to enqueue.  The host stays
// `lag` (gn_lag) iterations ahead of each sub-batch and stops once its k_gn_solve reports that no job is
// active (flags in host-mapped memory), so a launch's tail cannot be enqueued before the device
// has run most of it; two launches in flight are advanced together (fbr_batch_launch).
struct GnSubRun {
  Sub sub;
  GnArgs a;
  bool live = false, watch = false, done = false;
  int active = 0;  // jobs still iterating `lag` iterations ago (an upper bound now)
  int it = 0;      // next iteration to enqueue
  FlagWait wait;   // the wait for the flag that iteration needs (a non-blocking pass resumes it)
};
struct GnRun {
  bool pending = false;
  bool trace = false;
  int nsub = 0;
  unsigned long long gen = 0;
  int lag = 2;  // gn_lag: iterations enqueued ahead of the latest flag read
  GnSubRun s[kMaxSub];
};

// The kinds of flag wait, each with a bound of its own (fbr_pace.h WaitBound).
enum { kWaitBatchFlag = 0, kWaitScanFlag = 1, kWaitDirect = 2 };

// Members stand under the unit that owns them: the unit that gives them their meaning and, but for
// fbr_create's allocations, writes them.
//
// Ownership: every array, stream and event is an owning handle (fbr_own.h) and is released by
// ~fbr_ctx, whichever unit allocated it and whenever ("grown on demand", "allocated on first
// use"); a raw pointer member does not own and says so.  Members are destroyed in reverse order of
// declaration: the streams, the events, the ingest and the timers stand first, so they go after
// every buffer.  fbr_destroy drains the streams before it deletes the context.
struct __attribute__((visibility("hidden"))) fbr_ctx {
  fbr_params P;
  int dev = 0;
  int H = 0, W = 0, Bcap = 0;
  int64_t HW = 0, NMAX = 0;
  int items_per_job = 0;
  int max_items = 0;

  ~fbr_ctx() {
    free_grid(grid_c);
    free_grid(grid_s);
    free_grid(icp_grid);
    for (DevGrid& g : icp_grids) free_grid(g);
    arena_free(arena);
  }

  // ---- streams and events (fbr_api.hip creates them; every unit enqueues on them) ----
  Stream stream;            // primary stream (single-scan calls, batch sub-batch 0, export)
  Stream xstream[kMaxSub];  // extra streams of batch sub-batches 1.. (index 0 unused)
  Event xev[kMaxSub];       // fork / join events
  Event ev_staged;          // the staged inputs are on the device (recorded on stream)
  Event ev_fork;            // single-scan side-stream fork
  Event ev_ext;             // a caller's stream, waited on before an export (fbr_batch_export_ready)
  Ingest ing;               // fbr_process_batch host ingest (fbr_batch.hip; allocated on first use)
  std::map<std::string, KernelTimer> timers;  // profiling (fbr_api.hip)
  DevArena arena;           // scratch of the set-up paths (map VoxelGrid, grid builds)

  // ---- stage inputs and work arrays: projection, features, mapping DS (fbr_stages.hip) ----
  // inputs
  Dev<fbr_point_xyzirt> d_pts_own;    // [Bcap][NMAX] the context's scan buffer
  fbr_point_xyzirt* d_pts = nullptr;  // not owning: the scan buffer the stages read, d_pts_own but
                                      // for the ingest slot of a running fbr_process_batch
  Dev<int64_t> d_nin;
  Dev<float> d_guess;
  // projection
  // owner image generations (OwnerTag, fbr_kernels.h): owner_ib index bits, owner_tmax the last
  // generation before the image is refilled (0: untagged, reset by k_compact)
  int owner_ib = 0;
  uint32_t owner_gen = 0, owner_tmax = 0;
  Dev<int32_t> d_owner, d_rowcnt, d_col, d_start, d_end, d_nvalid;
  Dev<float4> d_cloud;
  Dev<float> d_range;
  // features
  Dev<StreamState> d_sstate;     // [Bcap] batch (zeroed per batch)
  Dev<StreamState> d_sstream;    // [1]   stream mode (persistent)
  Dev<int8_t> d_label;           // [Bcap][HW]
  Dev<int8_t> d_label_stream;    // [HW]   stream mode (persistent)
  Dev<float4> d_corner_slot;
  Dev<int32_t> d_corner_cnt;
  Dev<float4> d_surf_ring;
  Dev<int32_t> d_surf_ring_cnt;
  Dev<float> d_ring_box;        // [B][H][kRingBox]: k_concat's per-ring cloud bounds
  bool ring_box_valid = false;  // d_corner_all / d_surf_all came from k_concat (not upload_cloud)
  Dev<int32_t> d_err;
  Dev<float4> d_corner_all, d_surf_all, d_cornerDS, d_surfDS;
  Dev<int32_t> d_ncorner, d_nsurf, d_ncds, d_nsds;
  Dev<uint32_t> d_vg_scratch;
  int64_t vg_scratch_elems = 0;
  Dev<unsigned char> d_feat_scratch;  // k_features sorted-path slots [B*H][gslot_bytes]
  // IMU deskew (fbr_set_deskew, fbr_batch.hip, fills the tables)
  Dev<fbr_deskew_table> d_desk;  // [Bcap] tables (allocated on first use)
  Dev<int32_t> d_desk_mode;      // [Bcap] kDesk* bits per job
  Dev<int32_t> d_rowmin;         // [Bcap][H] minimum owner per row
  Dev<int32_t> d_choff;          // [Bcap][H][W / 32 + 1] compaction tile offsets
  bool desk_any = false;         // some job has an IMU mode (kDeskPoints | kDeskImu)
  bool no_time_call = false;     // the current call's PointCloud2 has no "time" field
  // Motion deskew (fbr_set_motion, fbr_batch.hip): d_desk_mode holds both setters' bits
  Dev<fbr_motion> d_motion;               // [Bcap] records (allocated on first use)
  std::vector<int32_t> imu_mode, mot_mode;  // [Bcap] each setter's bits (empty: none set yet)
  bool mot_field_any = false;    // some job's motion takes its time from the field (needs the 24-B scans)
  bool mot_col_any = false;      // some job's motion takes its time from the column

  // ---- Gauss-Newton work arrays, run driver state and results (fbr_stages.hip) ----
  Dev<GnState> d_gn;
  Dev<int4> d_items;
  Dev<int32_t> d_nitems, d_item_range, d_cropcnt;
  Dev<int32_t> d_cropwork;  // [Bwork][2]: a launch's CropBox counts while they accumulate
  Dev<double> d_partial;
  Dev<int32_t> d_nbr;
  Dev<float> d_fitc;     // [max_items][6][256] per-query fit cache (k_gn_residual)
  Dev<int8_t> d_fits;    // [max_items][256]
  Dev<int8_t> d_nsame;   // [max_items][256]
  // block-tile kNN (k_knn_tile.hip), allocated by build_map_grids when the map's grids take it:
  Dev<int32_t> d_fb_list;  // [3][max_items][256] queued / binned query slots, query blocks
  Dev<int32_t> d_bin;      // [kMaxSub][3][bin_nb] per-block counts, cursors, non-empty list
  int64_t bin_nb = 0, bin_nb_c = 0;
  HostWord<unsigned long long> iter_flags;  // written by k_gn_solve: [kMaxSub][max_iterations], then [kMaxSub] item counts
  unsigned long long gn_gen = 0;
  Dev<int32_t> d_iter_cnt;
  WaitBound wait_bound[3];            // kWaitBatchFlag / kWaitScanFlag / kWaitDirect
  int gn_items_hint = 0, gn_items_hint_B = 0;  // the last batch run's work items and its job count
  // Work items of the previous single scan: the next one's Gauss-Newton grids are sized from it
  // (2x, at least 16 workgroups) instead of from the capacity bound.  The kernels loop over the
  // items whatever the grid, so the hint only moves time: the C2 bound of ~900 items launched
  // ~870 workgroups (x 8 in the wide kNN mode) that found no item.
  int items_hint = 0;
  bool crop_cached = false;  // d_cropcnt holds the staged batch's CropBox statistics
  Dev<float> d_pose_out;
  Dev<fbr_reg_stats> d_stats;
  Dev<float> d_trace;  // [Bwork][max_iterations][6] traced poses, then knn_T_slot's 12 + 6 floats
  Dev<JobResult> d_result;     // [Bcap] packed per-job results
  Pinned<JobResult> h_result;  // [Bcap]
  std::vector<int32_t> last_iters, last_q, last_n, last_m;
  // fbr_diag_knn_last: the kernel every iteration's kNN pass of a single scan ran, and whether the
  // latest run was a single scan (job slot 0 then holds it); the pass's transform and trig
  // (GnArgs::knn_T, 12 + 6 floats: fbr_diag_gn_last reads both) are kept behind the traced poses
  // (knn_T_slot: no device block of its own)
  float* knn_T_slot() { return d_trace + Bwork * std::max(0, P.max_iterations) * 6; }
  std::vector<KnnLaunchDesc> knn_desc;  // [max_iterations]
  bool knn_last_valid = false;

  // ---- single-scan state (fbr_scan.hip) ----
  int64_t single_n = -1;  // the single-scan path's point count (k_project's argument, no copy)
  bool have_projection = false;
  double time_last = -1.0;
  int stream_degenerate = 0;  // mapOptimization::isDegenerate across single-scan registrations
  bool crop_join = false;    // single scan: copy_results takes the CropBox counts from h_crop (side stream)
  Pinned<int32_t> h_crop;          // [2]: the single-scan CropBox counts
  Pinned<float> h_guess;           // [6]: the single-scan guess (queue_guess)
  Pinned<fbr_point_xyzirt> h_scan;  // [NMAX] staging of single-scan uploads
  Pinned<int64_t> h_nin;           // scalar
  GrowDev<uint8_t> d_msg;          // raw PointCloud2 bytes of the last *_msg call (grown on demand)
  GrowPinned<uint8_t> h_msg;       // staging of raw PointCloud2 bytes (grown on demand)
  // fbr_process_scan's direct result (GnArgs::direct): the ending k_gn_solve packs the job's
  // result into `direct` (host-mapped); the host spins on its generation word instead of
  // enqueueing finalize + pack + copy and synchronising.  The no-op iterations the host had
  // enqueued ahead of the last flag may still be queued when the call returns (tail_pending):
  // the next single-scan call is ordered after them on the stream, every other entry point
  // synchronises the stream first (enter).
  HostWord<JobResult> direct;
  Dev<int32_t> d_direct_done;
  int32_t direct_gen = 0;     // generation of the current single-scan run (0: direct off)
  int32_t direct_gen_seq = 0;
  bool tail_pending = false;

  // ---- batch staging and launch slots (fbr_batch.hip) ----
  int nsub_pref = 3;                  // sub-batches per batch launch (FBR_NSUB overrides): 3 unpipelined (at
                                      // B = 128: 2 -> 76.1k, 3 -> 78.5k, 4 -> 46.7k scans/s), 1 pipelined
  // Batch launches rotate over nslot work slots (fbr_params.pipeline_depth, default 3; 1 when max_batch = 1): the
  // next launch's projection / features overlap the previous ones' Gauss-Newton tails.  Work arrays
  // hold Bwork = nslot * Bcap jobs; inputs hold Bcap.
  static constexpr int kMaxSlots = 3;
  int nslot = 1;
  int64_t Bwork = 0;
  GnRun run[kMaxSlots];
  int64_t launch_seq = 0;     // batch launches so far
  int last_slot = -1;         // slot of the latest launch (-1: none since the last stage)
  int64_t slot_launch[kMaxSlots] = {-1, -1, -1};  // launch number of each slot's latest launch
  bool batch_full_masks = false;            // fbr_batch_set_full_masks: launches compute whole masks
  bool slot_full_masks[kMaxSlots] = {};     // ... and which slots' latest launch did
  int64_t exported = -1;      // latest launch whose records fbr_batch_export_ready exported
  int64_t first_valid = 0;    // launches below this id belong to a dropped batch (fbr_batch_allgather)
  int staged_B = 0;
  std::vector<int64_t> staged_nin;
  // the staged batch's 16-B device records (fbr_kernels.h: x, y, z, ring bits), null = the 24-B
  // scans in d_pts; d_pk backs them for fbr_batch_stage (fbr_process_batch expands into its slots)
  Dev<float4> d_pk;
  const float4* staged_pk = nullptr;  // not owning: d_pk or an ingest slot's records
  bool staged_24 = false;  // d_pts holds the staged batch's 24-B scans (a deskewing launch needs them)

  // ---- map grids (fbr_map.hip) ----
  bool has_map = false;
  DevGrid grid_c, grid_s;  // kNN grids of the corner / surf maps (k_grid.hip)
  std::vector<fbr_point_xyzi> map_c_host, map_s_host;
  bool map_nocrop = false;  // the registration map is a keyframe local map

  // ---- keyframes (fbr_map.hip) ----
  // LIO-SAM keyframe store (fbr_keyframes_*) and the local map built from it
  std::vector<fbr_keypose> kf_poses;
  std::vector<int64_t> kf_c_off, kf_c_cnt, kf_s_off, kf_s_cnt;
  GrowDev<float4> d_kf_c, d_kf_s;  // lidar-frame keyframe clouds, appended
  int64_t kf_c_used = 0, kf_s_used = 0;
  GrowDev<float4> d_kraw_c, d_kraw_s;  // concatenated transformed clouds
  Dev<float4> d_kds_c, d_kds_s;        // their VoxelGrids (laserCloud*FromMapDS)
  int64_t kds_c_n = 0, kds_s_n = 0;
  GrowDev<KfSeg> d_kf_segs;

  // ---- loop closure / ICP scratch (fbr_loop.hip) ----
  // loop closure ICP (fbr_perform_loop_closure, fbr_icp_align): scratch of its own, grown on demand
  GrowDev<float4> d_icp_src, d_icp_x, d_icp_raw, d_icp_tgt;
  GrowDev<unsigned long long> d_icp_key;
  GrowDev<int32_t> d_icp_far;  // [n + 1]: the far-query list, then its count
  GrowDev<double> d_icp_partial;
  GrowDev<KfSeg> d_icp_segs;
  Dev<IcpState> d_icp_state;   // the state, then the fbr_icp_result record
  HostWord<unsigned long long> icp_flag;  // the progress word k_icp_solve writes (allocated on first use)
  unsigned long long icp_gen = 0;
  DevGrid icp_grid;            // the ICP's own grid over its target
  // many pairs per launch (fbr_perform_loop_closures, fbr_icp_align_batch): the pools of one chunk
  // (fbr_loop_plan.h), grown on demand; the progress word and its generation are the two above
  GrowDev<float4> d_lb_src, d_lb_x, d_lb_raw, d_lb_tgt;
  GrowDev<unsigned long long> d_lb_key;
  GrowDev<int32_t> d_lb_far;       // the pairs' far-query lists
  GrowDev<double> d_lb_partial;    // [blocks of the chunk][kIcpSums]
  GrowDev<KfSeg> d_lb_segs;
  GrowDev<uint8_t> d_lb_meta;      // argument blocks, block table, splits; control block, states, results, queue counts
  std::vector<DevGrid> icp_grids;  // one search grid per pair of the chunk (released by ~fbr_ctx)

  // ---- scan-context place recognition (fbr_sc.hip) ----
  // One descriptor per keyframe, in keyframe order, described on demand (fbr_sc_update) from the
  // keyframe pools above; fbr_keyframes_reset (fbr_map.hip) and a change of sc_P empty the store.
  fbr_sc_params sc_P{};           // the parameters the store was described with (sc_n > 0)
  int64_t sc_n = 0;               // keyframes described so far
  GrowDev<uint32_t> d_sc_desc;    // [keyframes][n_ring][n_sector] float bits, grown on demand
  GrowDev<double> d_sc_norm;      // [keyframes][n_sector] column norms
  GrowDev<ScSeg> d_sc_segs;       // a describe launch's segments
  GrowDev<ScRec> d_sc_rec;        // [keyframes] a search's per-candidate records
  GrowPinned<ScRec> h_sc_rec;     // the pinned result block: the records of the last search
  Dev<uint32_t> d_sc_q;           // the query slot: one descriptor of the largest shape
  Dev<double> d_sc_qn;            // ... and its column norms
  GrowDev<float4> d_sc_cloud;     // an uploaded query cloud, corner then surf

  // ---- pose graph (fbr_pg.hip) ----
  // The factors live on the host, like kf_poses, and are uploaded per optimise; fbr_keyframes_reset
  // (fbr_map.hip) empties them.  Every buffer is allocated on first use and grown on demand.
  std::vector<PgFactor> pg_factors;
  std::vector<double> pg_result;   // [pg_result_n][6] the last optimise's poses
  int64_t pg_result_n = -1;        // the store's size at that optimise (-1: no result)
  GrowDev<PgFactor> d_pg_fac;
  GrowDev<int32_t> d_pg_adj;       // the two adjacency lists: offsets, then entries
  GrowDev<double> d_pg_work;       // every double array of an optimise (fbr_pg.hip pg_prepare)
  Dev<PgState> d_pg_state;
  HostWord<unsigned long long> pg_flag;  // the progress word k_pg_decide writes (allocated on first use)
  unsigned long long pg_gen = 0;
  // marginal covariances (fbr_pg_marginals): valid for the result above while the factor count is
  // the one that optimise saw
  int64_t pg_result_nf = -1;
  GrowDev<double> d_pg_marg;       // every double array of a marginals call (fbr_pg.hip pg_marginals_run)
  GrowDev<int32_t> d_pg_loops;     // the loop factors' indices, in factor order
  GrowDev<int64_t> d_pg_nodes;     // the requested nodes, then the distinct ones in ascending order
  // robust loop factors and the direct solve (fbr_pg_params.robust / solver; kernels: k_posegraph.hip's
  // k_pg_robust, k_pg_direct.hip over k_pg_marginals.hip's launchers)
  int32_t pg_result_robust = 0;    // the last optimise's robust option: the marginals use it too
  double pg_result_scale = 0.0;
  std::vector<int32_t> pg_loop_index;        // fbr_pg_loop_weights: the loop factors' indices in add order,
  std::vector<double> pg_loop_chi2, pg_loop_w;  // their |r|^2 and weight at the result poses
  GrowDev<double> d_pg_direct;     // W, the chunk's right-hand sides per level, C and z of a direct solve

  // ---- global map (fbr_gmap.hip) ----
  // The clouds of the last fbr_global_map_build, until the next build, fbr_keyframes_reset or
  // fbr_destroy; the raw concatenations only when that build kept them.
  bool gm_built = false, gm_has_raw = false;
  Dev<float4> d_gm_c, d_gm_s, d_gm_raw_c, d_gm_raw_s;
  int64_t gm_c_n = 0, gm_s_n = 0, gm_raw_c_n = 0, gm_raw_s_n = 0;
  std::vector<fbr_keypose> gm_poses;  // the key poses that build used
  GrowDev<KfSeg> d_gm_segs;           // a build's entries, corner then surf
  // the map fbr_global_map_install put in place, in map-index order: fbr_get_map's source while
  // map_host_stale says that map_*_host have not been filled from it yet (fbr_map.hip)
  Dev<float4> d_inst_c, d_inst_s;
  int64_t inst_c_n = 0, inst_s_n = 0;
  bool map_host_stale = false;

  // ---- pose scoring (fbr_score.hip) ----
  // Scratch of fbr_score_poses / fbr_pose_search, grown on demand; but for the scan's clouds it is
  // sized by the poses of one launch (fbr_score_params.pose_chunk), not by the call's.
  GrowDev<float4> d_score_cloud;              // the scan's clouds, corner then surf
  GrowDev<float> d_score_T;                   // [chunk][kScorePose]
  GrowDev<ScorePartial> d_score_partial;      // [chunk][work items of a pose]
  GrowDev<fbr_pose_score> d_score_out;        // [chunk]
  GrowDev<unsigned long long> d_score_keys;   // [chunk][n_corner + n_surf], calls that ask for the keys

  // ---- registration information (fbr_reg_info.hip) ----
  // Scratch of fbr_reg_info_poses / fbr_batch_info, grown on demand and sized by the poses (jobs) of
  // one launch (fbr_info_params.pose_chunk); nothing else reads or writes it.
  GrowDev<float4> d_info_cloud;       // fbr_reg_info_poses: the clouds, corner then surf
  GrowDev<float> d_info_pose;         // [chunk][6]
  GrowDev<double> d_info_partial;     // [chunk][work items of a job][kInfoPartial]
  GrowDev<fbr_reg_info> d_info_out;   // [chunk]

  // ---- profiling (fbr_api.hip; the timers stand with the events above) ----
  bool profiling = false;
  std::set<std::string> profile_only;  // empty: time every kernel

  // ---- diagnostics (fbr_api.hip) ----
  int diag_err_job = -1;      // diagnostic (fbr_diag_force_capacity_error): batch job flagged over capacity
  int diag_ring_filter = -1;  // diagnostic (fbr_diag_ring_filter): per-ring surf filter kernel, -1 = by size
  bool diag_wide_cloud = false;  // diagnostic (fbr_diag_batch_cloud): batch launches keep the float4 cloud
  int last_cloud_bytes = 0;      // record size of the last batch launch's projected cloud (12 or 16; 0: none yet)
  Dev<unsigned long long> d_feat_stamps;  // diagnostic builds (FBR_FEAT_STAMPS) only
  Dev<uint32_t> d_feat_paths;             // tests (fbr_diag_feature_paths): FeatArgs::paths [Bwork][H]
};

namespace fbr {
namespace internal __attribute__((visibility("hidden"))) {

// A * B of two affine row-major 4x4 float matrices (Eigen::Affine3f product): entries
// ((a0 b0 + a1 b1) + a2 b2), the translation column + a3.
inline void affine_mul(const float* A, const float* B, float* G) {
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 4; ++q) {
      float s = (A[4 * r] * B[q] + A[4 * r + 1] * B[4 + q]) + A[4 * r + 2] * B[8 + q];
      if (q == 3) s = s + A[4 * r + 3];
      G[4 * r + q] = s;
    }
  G[12] = G[13] = G[14] = 0.0f;
  G[15] = 1.0f;
}

// Every public entry point: the context's device, and no single-scan tail left on the stream
// unless the call is a single scan itself (keep_tail: its work is ordered after the tail).
inline hipError_t enter(fbr_ctx* c, bool keep_tail = false) {
  hipError_t e = hipSetDevice(c->dev);
  if (e == hipSuccess && c->tail_pending && !keep_tail) {
    e = fbr_sync(c->stream);
    c->tail_pending = false;
  }
  return e;
}

// ---- functions that cross units, by the unit that defines them ----
// (A unit defines them in namespace fbr::internal; they are hidden by their declaration here.
// Everything else in a unit is file-local, in its anonymous namespace.)
// fbr_api.hip
void timer_begin(fbr_ctx* c, hipStream_t st, const char* name, hipEvent_t* ev_end);
void timer_end(hipStream_t st, hipEvent_t ev_end);
void feat_caps(int W, FeatArgs& a);
// fbr_stages.hip
Sub single_sub(fbr_ctx* c);
int stage_project(fbr_ctx* c, const Sub& sb);
int stage_features(fbr_ctx* c, const Sub& sb, bool stream_mode, bool err_clear = false, bool labels_out = false);
int crop_stats(fbr_ctx* c, const Sub& sb);
int register_prepare(fbr_ctx* c, const Sub& sb, bool trace);
int stage_register(fbr_ctx* c, const Sub& sb, bool trace);
void gn_run_start(fbr_ctx* c, GnRun& r, const Sub* subs, int nsub, bool trace);
int gn_run_pass(fbr_ctx* c, GnRun& r, bool block, bool* progress);
int advance_runs(fbr_ctx* c, int target);
int batch_quiesce(fbr_ctx* c);
int copy_results(fbr_ctx* c, int B, fbr_reg_stats* stats, float* poses_out, bool with_reg = true, int64_t w0 = 0,
                 bool per_job = false);
int check_err(fbr_ctx* c, int B);
// fbr_batch.hip
int drop_staged_batch(fbr_ctx* c);
// fbr_map.hip
int voxel_grid_dev(fbr_ctx* c, const float4* d_in, int64_t n, float leaf, float4* d_out, int64_t* n_out);
// fbr_set_map on clouds that are on the device already (fbr_global_map_install)
int set_map_device(fbr_ctx* c, const float4* d_corner, int64_t n_corner, const float4* d_surf, int64_t n_surf);
// fbr_gmap.hip
void gmap_drop(fbr_ctx* c);  // forgets the built global map (fbr_keyframes_reset)
// fbr_loop.hip
bool loop_params_ok(const fbr_loop_params* lp);
// performLoopClosure for a given candidate pair; latest_pose (null: the stored one) stands for the
// last keyframe's pose wherever performLoopClosure reads it
int loop_perform(fbr_ctx* c, const fbr_loop_params* lp, int32_t latest, int32_t closest, const float* latest_pose,
                 fbr_loop_result* out);

}  // namespace internal
}  // namespace fbr

// Kernel launch timed by its dispatches' own start / end timestamps (when profiling).
#define TIMED_ON(ctx, st, name, launch)   \
  do {                                    \
    hipEvent_t ev_;                       \
    timer_begin(ctx, st, name, &ev_);     \
    launch;                               \
    timer_end(st, ev_);                   \
  } while (0)
#define TIMED(ctx, name, launch) TIMED_ON(ctx, (ctx)->stream, name, launch)
