// fbr_knobs.h — every environment tuning knob of the library, one accessor each.
//
// Host-only and free of HIP headers: the launchers in the k_*.hip files, the host units
// (fbr_*.hip) and the CPU probe (tests/native/host_probe.cpp, tests/test_knobs.py) include it.
// The accessors stand in the order of the table in DESIGN.md §6 "Tuning knobs", which has one row
// per accessor; tests/test_knobs.py holds the two together and checks every parse.
//
// When a knob is read:
//   once per process   at its first use (a function-local static); every knob not named below
//   per fbr_create     FBR_NSUB, FBR_OWNER_TMAX
//   per map build      FBR_KNN_CELL, FBR_KNN_CELL_X
//   first ingest       FBR_STAGE_MB, FBR_STAGE_THREADS (a context's first fbr_process_batch)
// The per-call accessors say so at their definition; they hold no static.
//
// The namespace is hidden: the accessors and their statics are shared by the library's translation
// units and are not exported from it.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>

namespace fbr {
namespace knobs __attribute__((visibility("hidden"))) {

// ---- the parses ------------------------------------------------------------------------------
// A switch: any value atoi reads as non-zero is on (text reads as 0).
inline bool flag(const char* name, bool def) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) != 0 : def;
}
// An integer clamped to [lo, hi] when set; the default is returned as it is.
inline int clamped(const char* name, int def, int lo, int hi) {
  const char* e = std::getenv(name);
  return e ? std::min(hi, std::max(lo, std::atoi(e))) : def;
}
inline int64_t clamped64(const char* name, int64_t def, int64_t lo) {
  const char* e = std::getenv(name);
  return e ? std::max<int64_t>(lo, std::atoll(e)) : def;
}
// "0 = not forced": 0 when unset, else the value clamped to [lo, hi] with lo >= 1.
inline int forced(const char* name, int lo, int hi) { return clamped(name, 0, lo, hi); }

// ---- the knobs, in the order of DESIGN.md §6 -----------------------------------------------------

// Sub-batches (HIP streams) per batch launch, 1..max_sub; 0 = unset (3 unpipelined, 1 pipelined:
// fbr_create).  Read at each fbr_create.
inline int nsub(int max_sub) { return forced("FBR_NSUB", 1, max_sub); }

// FBR_KNN_TILE: 1 serves iterations >= 1 on dense 0.5 m x 0.125 m grids from the block tiles; 0
// (the default: the tiles measured slower than the grid search) keeps the grid
// search for every query.
inline bool knn_tile() {
  static const bool v = flag("FBR_KNN_TILE", false);
  return v;
}

// Diagnostic counters of the block tiles (FBR_KNN_TILE_STATS=1; k_knn_tile.hip allocates them).
inline bool knn_tile_stats() {
  static const bool v = flag("FBR_KNN_TILE_STATS", false);
  return v;
}

// Few segments (single-scan calls): P workgroups per segment of the mapping-DS VoxelGrid
// (FBR_VG_SPLIT = P, default 8: C2 latency -10 us against 4,
// profiles/r05w_latency_knob_sweep.txt; below 2: 1, off).
inline int vg_split() {
  static const int v = clamped("FBR_VG_SPLIT", 8, 1, 8);
  return v;
}

// FBR_INGEST_COMPACT=0: always ship the 24-B records.
inline bool ingest_compact() {
  static const bool v = flag("FBR_INGEST_COMPACT", true);
  return v;
}

// Idle copy workers spin after an upload for 4x the smoothed interval between uploads, at least
// 1 ms and at most FBR_COPY_SPIN_US (default 5000 us), so a pose-chained scan stream (one call
// every ~0.7-0.9 ms, the caller's own work included) finds them awake while a sensor-rate stream
// (a scan every 100 ms) holds the cores for at most 5 % of the time; then they sleep on the
// condition variable.  0 = never spin.  A fixed 1000 us spin let late calls find the workers
// asleep, and the futex wake-up put ms-scale outliers into the upload (p99 3.9 ms).
inline int copy_spin_us() {
  static const int v = clamped("FBR_COPY_SPIN_US", 5000, 0, INT_MAX);
  return v;
}

// Compaction tile size in cells (FBR_COMPACT_CELLS: 512, 1024 or 2048).  512 since round 5: 10 KB of
// LDS per workgroup, twice the tiles in flight per CU; once the other kernels had shrunk, C2 B = 1024
// 114.5-114.9k -> 115.7-115.8k and C3 +0.9 % interleaved (profiles/r05ar_compact_cells_ab.txt; it was
// even with 1024 in round 4).
inline int compact_cells() {
  static const int v = [] {
    const int c = clamped("FBR_COMPACT_CELLS", 512, INT_MIN, INT_MAX);
    return c >= 2048 ? 2048 : c >= 1024 ? 1024 : 512;
  }();
  return v;
}

// Workgroups of the per-iteration GN kernels (each loops over the work items; FBR_GN_GRID overrides).
// 16384 covers the ~11k items of a C2 launch of 341 jobs with one workgroup each (8192 left a second
// round of items to half the workgroups: flat gn_knn -4 % per step, r05q).
inline int gn_grid_cap() {
  static const int v = clamped("FBR_GN_GRID", 16384, 1, INT_MAX);
  return v;
}

// One work item per workgroup in the batch kNN / residual launches (GnArgs::one_item;
// FBR_GN_ONE_ITEM=0: grid-stride loops, for A/B).
inline bool gn_one_item() {
  static const bool v = flag("FBR_GN_ONE_ITEM", true);
  return v;
}

// The batch tail also one item per workgroup; FBR_GN_TAIL_ONE_ITEM=0: a 1,024-workgroup loop.
inline bool gn_tail_one_item() {
  static const bool v = flag("FBR_GN_TAIL_ONE_ITEM", true);
  return v;
}

// Workgroups of a one-item launch before the run's item count is known (FBR_GN_ONE_GRID; a C2
// launch of 1,024 jobs has ~25.6k items); the loop launch behind it takes any items past them.
inline int gn_one_grid() {
  static const int v = clamped("FBR_GN_ONE_GRID", 32768, 1, INT_MAX);
  return v;
}

// Batch scans as 16-B device records (fbr_kernels.h; FBR_PACKED_SCANS=0: the 24-B scans, for A/B).
inline bool packed_scans() {
  static const bool v = flag("FBR_PACKED_SCANS", true);
  return v;
}

// The greedy walks over compact bit words (FeatArgs::compact; FBR_FEAT_COMPACT=0: the
// member-indexed rounds everywhere, for A/B).
inline bool feat_compact() {
  static const bool v = flag("FBR_FEAT_COMPACT", true);
  return v;
}

// Members the compact batch surf window resolves left of a segment's end: 59 (one word with the
// frozen candidates; the measured best) or 64 (two words); FBR_FEAT_SURF_WIN overrides, for A/B.
inline int feat_surf_win() {
  static const int v = clamped("FBR_FEAT_SURF_WIN", 59, INT_MIN, INT_MAX) == 59 ? 59 : 64;
  return v;
}

// Batch jobs resolve the surf walk only within reach of each segment's end (FeatArgs::surf_full;
// FBR_FEAT_SURF_WINDOW=0: the whole walk, for A/B).
inline bool feat_surf_window() {
  static const bool v = flag("FBR_FEAT_SURF_WINDOW", true);
  return v;
}

// Generation-tagged owner images (fbr_kernels.h OwnerTag; FBR_OWNER_TAGS=0: untagged images reset
// by k_compact, for A/B).
inline bool owner_tags() {
  static const bool v = flag("FBR_OWNER_TAGS", true);
  return v;
}

// Tests: the last owner generation before the images are refilled, so they refill every few calls;
// 0 = unset (by the index bits, fbr_create).  Read at each fbr_create.
inline int owner_tmax() { return clamped("FBR_OWNER_TMAX", 0, 0, INT_MAX); }

// Tail mode: once at most 1/FBR_GN_TAIL of a sub-batch's jobs are still iterating (default 8),
// its iterations run fused (kNN + residual in one launch) on a smaller grid: the few remaining
// jobs' work is latency-bound, so one launch less per iteration and fewer idle workgroups
// matter more than the fused kernel's register cost (0 disables).
inline int gn_tail_div() {
  static const int v = clamped("FBR_GN_TAIL", 8, 0, INT_MAX);
  return v;
}

// Iterations the host enqueues ahead of a sub-batch's latest flag (FBR_GN_LAG, 1..8, default 2).
// Three for single scans (~40 us iterations, a ~5.7 us host gap before each from the third on)
// measured no better: C2 latency p50 0.719 / 0.746 ms against 0.716 / 0.716 with 2 (profiles/r04v_*).
inline int gn_lag() {
  static const int v = forced("FBR_GN_LAG", 1, 8);
  return v ? v : 2;
}

// Flat row queue (FBR_KNN_FLAT=0 disables): from iteration 1 on (warm-start bound), 1 m y/z cells
// (9 rows: the queue is 18 KB of LDS per workgroup), not in the fused tail launch.
inline bool knn_flat() {
  static const bool v = flag("FBR_KNN_FLAT", true);
  return v;
}

// kNN grid cell sizes as inverse cells (powers of two, so cell coordinates and edges are exact),
// chosen from the map density the mapping leaf implies (one point per leaf voxel at most): 1 m
// along y and z and 0.25 m along x for surf leaves >= 0.3 m (sparse_leaf; the 0.4 m default),
// 0.5 m / 0.125 m for denser maps (measured).  FBR_KNN_CELL / FBR_KNN_CELL_X
// override in metres, rounded to a power of two and clamped; both maps share them.  Read at each
// map build.
inline float cell_inv(const char* name, float def, float lo, float hi) {
  float inv = def;
  if (const char* e = std::getenv(name)) {
    const float cell = std::strtof(e, nullptr);
    if (cell > 0.0f) inv = std::min(hi, std::max(lo, std::exp2(-std::round(std::log2(cell)))));
  }
  return inv;
}
inline float knn_cell_inv(bool sparse_leaf) {
  return cell_inv("FBR_KNN_CELL", sparse_leaf ? 1.0f : 2.0f, 0.5f, 4.0f);  // 2 m .. 0.25 m
}
inline float knn_cell_x_inv(bool sparse_leaf) {
  return cell_inv("FBR_KNN_CELL_X", sparse_leaf ? 4.0f : 8.0f, 0.5f, 8.0f);  // 2 m .. 0.125 m
}

// Clouds at least this large take the device-wide VoxelGrid (below 32768 the one-workgroup kernel
// is faster; FBR_VG_LARGE_MIN overrides: tests use it to compare both kernels on the same input).
inline int64_t vg_large_min() {
  static const int64_t v = clamped64("FBR_VG_LARGE_MIN", 32768, 1);
  return v;
}

// Diagnostic phase cut of k_voxel_ring (VgRing::dbg; 0 = the full kernel).
inline int vr_dbg() {
  static const int v = clamped("FBR_VR_DBG", 0, INT_MIN, INT_MAX);
  return v;
}

// In-place LDS sort of the mapping-DS segments (FBR_VG_INPLACE=0: the global-scratch kernel).
inline bool vg_inplace() {
  static const bool v = flag("FBR_VG_INPLACE", true);
  return v;
}

// Size classes of a two-set mapping-DS launch (k_voxel.hip): 0 = one launch of the large instance
// for both sets, 1 = the small set's launch first (default), 2 = last; anything else is 1.
inline int vg_classes() {
  static const int v = [] {
    const int c = clamped("FBR_VG_CLASSES", 1, INT_MIN, INT_MAX);
    return c < 0 || c > 2 ? 1 : c;
  }();
  return v;
}

// GnArgs::fit_cache: reuse a query's line / plane while its neighbours do not change (the value
// goes to the kernel as it is).
inline int fit_cache() {
  static const int v = clamped("FBR_FIT_CACHE", 1, INT_MIN, INT_MAX);
  return v;
}

// Tests: every kNN grid as hashed chunks.
inline bool grid_sparse() {
  static const bool v = flag("FBR_GRID_SPARSE", false);
  return v;
}

// Lanes per query of the plain kNN pass: 8 or more gives 8, any other set value 1; 0 = unset
// (by the sub-batch's jobs, fbr_gn.h knn_lpq).
inline int knn_lpq() {
  static const int v = [] {
    const int f = forced("FBR_KNN_LPQ", 1, 8);
    return f == 8 ? 8 : f ? 1 : 0;
  }();
  return v;
}

// Waves per ring of k_features: 4 or more gives 4, 2 or 3 gives 2, 1 gives 1; anything else is
// 0 = not forced (by the launch's rings, k_features.hip feature_waves).
inline int feat_waves() {
  static const int v = [] {
    const int w = clamped("FBR_FEAT_WAVES", 0, INT_MIN, INT_MAX);
    return w >= 4 ? 4 : w >= 2 ? 2 : w == 1 ? 1 : 0;
  }();
  return v;
}

// Single scans take their result from the ending solve (FBR_DIRECT=0: finalize + pack + copy).
inline bool direct_results() {
  static const bool v = flag("FBR_DIRECT", true);
  return v;
}

// Single-scan uploads stage through our own pinned buffer with a threaded host copy (default;
// 1.00 vs 1.07 ms per pose-chained C2 scan) or hand the caller's pageable buffer to the runtime's
// staging copy (FBR_PINNED_UPLOAD=0).
inline bool pinned_upload() {
  static const bool v = flag("FBR_PINNED_UPLOAD", true);
  return v;
}

// fbr_process_batch staging: MB per pinned chunk (one H2D copy each; at least one scan), and the
// packing threads per chunk, 0 = unset (16, at most the host's hardware threads: the CPU share of
// a one-GPU box; 8 -> 16: ingest line +10-20 %, r06m/r06n).  Read at a context's first ingest.
inline int64_t stage_mb() { return clamped64("FBR_STAGE_MB", 64, 1); }
inline int stage_threads() { return forced("FBR_STAGE_THREADS", 1, INT_MAX); }

// FBR_INGEST_XSTREAM=0: k_expand_scans on the copy stream, one device stage (A/B).
inline bool ingest_xstream() {
  static const bool v = flag("FBR_INGEST_XSTREAM", true);
  return v;
}

// FBR_INGEST_NT=0: the packers use plain stores instead of streaming ones.
inline bool ingest_nt() {
  static const bool v = flag("FBR_INGEST_NT", true);
  return v;
}

// ---- knobs without an environment name ---------------------------------------------------------
// (not in the table of DESIGN.md §6, which lists what the environment sets)

// Device bytes the pairs of one chunk of fbr_perform_loop_closures / fbr_icp_align_batch may take
// when the caller leaves the chunk to the library (chunk_pairs = 0; fbr_loop_plan.h pair_bytes).
// 256 MiB: about 400 pairs of the loop fixture's size (3,400 source and 5,100 target points,
// ~0.6 MB each), whose ~4,000 query blocks fill the device several times over, and a small share
// of its memory.  The call's chunk_pairs overrides it per call, and no result depends on either
// (DESIGN.md §4.8), so it has no environment name.
inline int64_t loop_batch_bytes() { return (int64_t)256 << 20; }

}  // namespace knobs
}  // namespace fbr
