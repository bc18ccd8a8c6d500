// fbr_batch.hip — the batch entry points: the stage / launch / export state machine over the
// launch slots (fbr_batch_*, fbr_set_deskew), and fbr_process_batch with its ingest, a ring of
// pinned staging chunks packed by host threads and copied on a stream of its own.
#include "fbr_ctx.h"

namespace fbr {
namespace internal {

// Single-scan entry points reuse job slot 0 of the device buffers: a staged batch is dropped
// (fbr_batch_launch then reports FBR_ERR_STATE until the next fbr_batch_stage).
int drop_staged_batch(fbr_ctx* c) {
  const int rc = batch_quiesce(c);
  c->staged_B = 0;
  c->staged_pk = nullptr;
  c->staged_24 = false;
  c->crop_cached = false;
  c->last_slot = -1;
  // launch ids only grow: every launch made so far belongs to the dropped batch (or its slot was
  // overwritten by a single-scan call), so fbr_batch_export_ready must never hand one of them out
  c->exported = c->launch_seq - 1;
  c->first_valid = c->launch_seq;
  return rc;
}

}  // namespace internal
}  // namespace fbr

namespace {
// d_desk_mode = the IMU bits of fbr_set_deskew | the motion bits of fbr_set_motion
hipError_t upload_desk_modes(fbr_ctx* c) {
  std::vector<int32_t> mode(c->Bcap, 0);
  for (int j = 0; j < c->Bcap; ++j)
    mode[j] = (j < (int)c->imu_mode.size() ? c->imu_mode[j] : 0) | (j < (int)c->mot_mode.size() ? c->mot_mode[j] : 0);
  return fbr_memcpy_sync(c->d_desk_mode, mode.data(), sizeof(int32_t) * c->Bcap, hipMemcpyHostToDevice);
}
}  // namespace

extern "C" {

int fbr_batch_stage(fbr_ctx* c, const fbr_point_xyzirt* const* scans, const int64_t* n_in, int n_jobs,
                    const float* poses_in) {
  if (!c || !scans || !n_in || !poses_in || n_jobs <= 0) return FBR_ERR_INVALID_ARG;
  if (n_jobs > c->Bcap) return FBR_ERR_CAPACITY;
  // every job is validated before anything is copied: a rejected batch leaves the previous one's
  // buffers untouched, and nothing stays staged after a failure
  for (int j = 0; j < n_jobs; ++j) {
    if (n_in[j] < 0 || n_in[j] > c->NMAX) return FBR_ERR_CAPACITY;
    if (n_in[j] && !scans[j]) return FBR_ERR_INVALID_ARG;
  }
  CK(enter(c));
  int rc = drop_staged_batch(c);  // launches in flight read the inputs: they are enqueued first
  if (rc) return rc;
  c->no_time_call = false;
  auto q = [&](hipError_t e) {
    if (e != hipSuccess && !rc) rc = FBR_ERR_HIP;
  };
  // Without deskew tables the scans go over as 16-B device records (x, y, z, ring bits; packed by
  // host threads, as fbr_process_batch's compact records are); a deskewing batch keeps the 24-B
  // scans, whose time deskewPoint reads (IMU tables and field-timed motions; a column-timed motion
  // reads no time and keeps the records).
  const bool pk = knobs::packed_scans() && !c->desk_any && !c->mot_field_any;
  if (pk) {
    if (!c->d_pk && dalloc(c->d_pk, (int64_t)c->Bcap * c->NMAX)) return FBR_ERR_HIP;
    std::vector<float4> rec;
    for (int j0 = 0; j0 < n_jobs && !rc; j0 += 64) {  // 64 scans per host buffer (~118 MB for C2)
      const int j1 = std::min(n_jobs, j0 + 64);
      std::vector<int64_t> at(j1 - j0 + 1, 0);
      for (int j = j0; j < j1; ++j) at[j - j0 + 1] = at[j - j0] + n_in[j];
      rec.resize((size_t)at.back());
      const int nt = std::max(1, std::min(16, j1 - j0));
      auto pack = [&](int t) {
        for (int j = j0 + t; j < j1; j += nt) {
          const fbr_point_xyzirt* P = scans[j];
          float4* o = rec.data() + at[j - j0];
          for (int64_t i = 0; i < n_in[j]; ++i) {
            float4 v;
            v.x = P[i].x;
            v.y = P[i].y;
            v.z = P[i].z;
            const int32_t ring = P[i].ring;
            std::memcpy(&v.w, &ring, 4);
            o[i] = v;
          }
        }
      };
      std::vector<std::thread> th;
      for (int t = 1; t < nt; ++t) th.emplace_back(pack, t);
      pack(0);
      for (auto& x : th) x.join();
      for (int j = j0; j < j1 && !rc; ++j)
        if (n_in[j])
          q(hipMemcpyAsync(c->d_pk + j * c->NMAX, rec.data() + at[j - j0], sizeof(float4) * n_in[j],
                           hipMemcpyHostToDevice, c->stream));
      q(fbr_sync(c->stream));  // rec is refilled next round
    }
  } else {
    for (int j = 0; j < n_jobs && !rc; ++j)
      if (n_in[j])
        q(hipMemcpyAsync(c->d_pts + j * c->NMAX, scans[j], sizeof(fbr_point_xyzirt) * n_in[j],
                         hipMemcpyHostToDevice, c->stream));
  }
  if (!rc) q(hipMemcpyAsync(c->d_nin, n_in, sizeof(int64_t) * n_jobs, hipMemcpyHostToDevice, c->stream));
  if (!rc) q(hipMemcpyAsync(c->d_guess, poses_in, sizeof(float) * 6 * n_jobs, hipMemcpyHostToDevice, c->stream));
  if (!rc && c->has_map && c->map_nocrop) rc = crop_stats(c, Sub{0, n_jobs, 0, c->stream});
  if (!rc) q(hipEventRecord(c->ev_staged, c->stream));  // every launch's streams start after it
  // the caller's host buffers may be reused once this returns: drain the queued copies on every path
  q(fbr_sync(c->stream));
  if (rc) return rc;
  c->crop_cached = c->has_map && c->map_nocrop;
  c->staged_B = n_jobs;
  c->staged_pk = pk ? c->d_pk : nullptr;
  c->staged_24 = !pk;
  c->staged_nin.assign(n_in, n_in + n_jobs);
  return FBR_OK;
}

int fbr_set_deskew(fbr_ctx* c, const fbr_deskew_table* tables, int n_tables) {
  if (!c || n_tables < 0 || (n_tables > 0 && !tables)) return FBR_ERR_INVALID_ARG;
  if (n_tables > c->Bcap) return FBR_ERR_CAPACITY;
  CK(enter(c));
  std::vector<int32_t> mode(c->Bcap, 0);
  bool any = false;
  for (int j = 0; j < n_tables; ++j) {
    if (tables[j].imu_available && (tables[j].imu_pointer_cur < 1 || tables[j].imu_pointer_cur >= FBR_IMU_QUEUE))
      return FBR_ERR_INVALID_ARG;
    // deskewPoint and transformUpdate both key on cloudInfo.imuAvailable (:548, mapOptmization.h:1447)
    mode[j] = tables[j].imu_available ? (kDeskPoints | kDeskImu) : 0;
    any = any || mode[j] != 0;
  }
  if (any && !c->d_desk && dalloc(c->d_desk, c->Bcap)) return FBR_ERR_HIP;
  CK(fbr_sync(c->stream));
  if (any) CK(fbr_memcpy_sync(c->d_desk, tables, sizeof(fbr_deskew_table) * n_tables, hipMemcpyHostToDevice));
  c->imu_mode = mode;
  CK(upload_desk_modes(c));
  c->desk_any = any;
  return FBR_OK;
}

int fbr_set_motion(fbr_ctx* c, const fbr_motion* motions, int n) {
  if (!c || n < 0 || (n > 0 && !motions)) return FBR_ERR_INVALID_ARG;
  if (n > c->Bcap) return FBR_ERR_CAPACITY;
  CK(enter(c));
  std::vector<int32_t> mode(c->Bcap, 0);
  bool field = false, col = false;
  for (int j = 0; j < n; ++j) {
    const fbr_motion& m = motions[j];
    if (!m.flags) continue;  // the job is untouched, whatever else the record holds
    if (m.flags & ~(FBR_MOTION_POSITION | FBR_MOTION_ROTATION)) return FBR_ERR_INVALID_ARG;
    if (m.time_source != FBR_TIME_FIELD && m.time_source != FBR_TIME_COLUMN) return FBR_ERR_INVALID_ARG;
    if (m.time_source == FBR_TIME_COLUMN && m.column_direction != 1 && m.column_direction != -1)
      return FBR_ERR_INVALID_ARG;
    if (m.time_source == FBR_TIME_FIELD && !(m.scan_period > 0.0 && std::isfinite(m.scan_period)))
      return FBR_ERR_INVALID_ARG;
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(m.incre[k])) return FBR_ERR_INVALID_ARG;
    mode[j] = motion_mode_bits(m);
    (m.time_source == FBR_TIME_COLUMN ? col : field) = true;
  }
  if ((field || col) && !c->d_motion && dalloc(c->d_motion, c->Bcap)) return FBR_ERR_HIP;
  CK(fbr_sync(c->stream));
  if (field || col) CK(fbr_memcpy_sync(c->d_motion, motions, sizeof(fbr_motion) * n, hipMemcpyHostToDevice));
  c->mot_mode = mode;
  CK(upload_desk_modes(c));
  c->mot_field_any = field;
  c->mot_col_any = col;
  return FBR_OK;
}

int fbr_batch_launch(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (c->staged_B <= 0) return FBR_ERR_STATE;
  if (!c->has_map) return FBR_ERR_NO_MAP;
  // deskew tables set after the batch was staged as 16-B records (no time field): stage it again
  if ((c->desk_any || c->mot_field_any) && !c->no_time_call && !c->staged_24) return FBR_ERR_STATE;
  CK(enter(c));
  const auto t0 = std::chrono::steady_clock::now();
  // Sub-batches on separate streams: one sub-batch's low-occupancy phases (the features' ring-0
  // waves, the last Gauss-Newton iterations) overlap the others' work.  Consecutive launches take
  // alternate work slots with their own streams, and this call returns once the previous launch is
  // fully enqueued: this launch's projection and features run beside the previous one's GN tail.
  const int B = c->staged_B;
  const int slot = (int)(c->launch_seq % c->nslot);
  int rc = advance_runs(c, slot);  // (already enqueued by the previous call: launches n-2 < n-1)
  if (rc) return rc;
  const int nsub = std::max(1, std::min({c->nsub_pref, kMaxSub / c->nslot, B / 8}));
  Sub subs[kMaxSub];
  for (int k = 0; k < nsub; ++k) {
    const int j0 = (int)((int64_t)B * k / nsub), j1 = (int)((int64_t)B * (k + 1) / nsub);
    const int idx = slot * nsub + k;
    subs[k] = Sub{(int)((int64_t)slot * c->Bcap + j0), j1 - j0, idx, idx == 0 ? c->stream : c->xstream[idx], false, j0};
    CK(hipStreamWaitEvent(subs[k].st, c->ev_staged, 0));  // the staged inputs
  }
  for (int k = 0; k < nsub && !rc; ++k) {
    rc = stage_project(c, subs[k]);
    if (!rc && c->batch_full_masks)  // cloudLabel of a fresh FeatureExtraction: zeros outside the picks
      rc = hipMemsetAsync(c->d_label + (int64_t)subs[k].j0 * c->HW, 0, (size_t)subs[k].B * c->HW, subs[k].st) ? FBR_ERR_HIP
                                                                                                            : FBR_OK;
    if (!rc) rc = stage_features(c, subs[k], false, true, c->batch_full_masks);
    if (!rc) rc = register_prepare(c, subs[k], false);
  }
  if (rc) return rc;
  gn_run_start(c, c->run[slot], subs, nsub, false);
  c->last_slot = slot;
  c->slot_full_masks[slot] = c->batch_full_masks;
  c->slot_launch[slot] = c->launch_seq++;
  bool p = false;
  rc = gn_run_pass(c, c->run[slot], false, &p);  // the iterations that need no flag yet
  // return once launch n - (nslot - 1) is fully enqueued (its slot is launch_seq mod nslot now that
  // launch_seq = n + 1; nslot = 1: this launch itself)
  if (!rc) rc = advance_runs(c, (int)(c->launch_seq % c->nslot));
  debug_counters().batch_ns[0].fetch_add(ns_since(t0), std::memory_order_relaxed);
  return rc;
}

int fbr_batch_flush(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  return advance_runs(c, -1);
}

int fbr_batch_wait(fbr_ctx* c) {
  if (!c) return FBR_ERR_INVALID_ARG;
  CK(enter(c));
  const int rc = batch_quiesce(c);
  if (rc) return rc;
  CK(fbr_sync(c->stream));
  return FBR_OK;
}

int fbr_batch_results(fbr_ctx* c, float* poses_out, fbr_reg_stats* stats) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (c->staged_B <= 0 || c->last_slot < 0) return FBR_ERR_STATE;
  CK(enter(c));
  const int rc = batch_quiesce(c);
  if (rc) return rc;
  return copy_results(c, c->staged_B, stats, poses_out, true, (int64_t)c->last_slot * c->Bcap, true);
}

int fbr_batch_set_full_masks(fbr_ctx* c, int on) {
  if (!c) return FBR_ERR_INVALID_ARG;
  c->batch_full_masks = on != 0;
  return FBR_OK;
}

int fbr_batch_labels(fbr_ctx* c, int job, int8_t* label, int64_t cap, int64_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !label)) return FBR_ERR_INVALID_ARG;
  *n_out = 0;
  if (c->staged_B <= 0 || c->last_slot < 0) return FBR_ERR_STATE;
  if (job < 0 || job >= c->staged_B) return FBR_ERR_INVALID_ARG;
  if (!c->slot_full_masks[c->last_slot]) return FBR_ERR_STATE;  // window masks are incomplete
  CK(enter(c));
  const int rc = batch_quiesce(c);
  if (rc) return rc;
  const int64_t w = (int64_t)c->last_slot * c->Bcap + job;
  CK(fbr_sync(c->stream));
  for (const GnRun& r : c->run)
    for (int k = 0; k < r.nsub; ++k) CK(fbr_sync(r.s[k].sub.st));
  int32_t nv = 0;
  CK(hipMemcpy(&nv, c->d_nvalid + w, sizeof(int32_t), hipMemcpyDeviceToHost));
  *n_out = nv;
  if (nv > cap) return FBR_ERR_CAPACITY;
  if (nv > 0) CK(hipMemcpy(label, c->d_label + w * c->HW, (size_t)nv, hipMemcpyDeviceToHost));
  return FBR_OK;
}

int fbr_batch_export(fbr_ctx* c, void* device_dst) {
  if (!c || !device_dst) return FBR_ERR_INVALID_ARG;
  if (c->staged_B <= 0 || c->last_slot < 0) return FBR_ERR_STATE;
  CK(enter(c));
  const int rc = batch_quiesce(c);
  if (rc) return rc;
  const int64_t w0 = (int64_t)c->last_slot * c->Bcap;
  launch_export_records(c->stream, c->staged_B, c->d_pose_out + w0 * 6, c->d_stats + w0, c->d_err + w0, c->d_guess,
                        (float*)device_dst);
  CK(hipGetLastError());
  c->exported = c->slot_launch[c->last_slot];
  return FBR_OK;
}

int fbr_batch_export_ready(fbr_ctx* c, void* device_dst, void* wait_stream, void** export_stream, int64_t* launch_id) {
  if (!c || !device_dst || !export_stream || !launch_id) return FBR_ERR_INVALID_ARG;
  *export_stream = nullptr;
  *launch_id = -1;
  if (c->staged_B <= 0) return FBR_ERR_STATE;
  CK(enter(c));
  // the oldest launch not yet exported, if it is fully enqueued: launches are exported in order
  // (one call per fbr_batch_launch never falls behind: launch n returns with n-1 enqueued)
  int s = -1;
  for (int q = 0; q < c->nslot; ++q)
    if (c->slot_launch[q] > c->exported && c->run[q].nsub > 0 && (s < 0 || c->slot_launch[q] < c->slot_launch[s]))
      s = q;
  if (s < 0 || c->run[s].pending) return FBR_OK;
  const GnRun& r = c->run[s];
  hipStream_t st = r.s[0].sub.st;
  for (int k = 1; k < r.nsub; ++k) CK(hipStreamWaitEvent(st, c->xev[r.s[k].sub.k], 0));
  if (wait_stream) {  // the caller's previous reader of device_dst
    CK(hipEventRecord(c->ev_ext, (hipStream_t)wait_stream));
    CK(hipStreamWaitEvent(st, c->ev_ext, 0));
  }
  const int64_t w0 = (int64_t)s * c->Bcap;
  launch_export_records(st, c->staged_B, c->d_pose_out + w0 * 6, c->d_stats + w0, c->d_err + w0, c->d_guess,
                        (float*)device_dst);
  CK(hipGetLastError());
  c->exported = c->slot_launch[s];
  *export_stream = (void*)st;
  *launch_id = c->slot_launch[s];
  return FBR_OK;
}

int fbr_batch_bytes(fbr_ctx* c, double* bytes_total, double* bytes_gn) {
  if (!c) return FBR_ERR_INVALID_ARG;
  if (c->last_iters.empty()) return FBR_ERR_STATE;
  double tot = 0.0, gn = 0.0;
  for (size_t j = 0; j < c->last_iters.size(); ++j) {
    const double nin = j < c->staged_nin.size() ? (double)c->staged_nin[j] : 0.0;
    const double n = c->last_n[j], M = c->last_m[j], Q = c->last_q[j], I = c->last_iters[j];
    const double g = I * 96.0 * Q;  // query 16 B + 5 neighbours x 16 B per iteration
    tot += 22.0 * nin + 80.0 * n + 16.0 * M + 16.0 * Q + g;
    gn += g;
  }
  if (bytes_total) *bytes_total = tot;
  if (bytes_gn) *bytes_gn = gn;
  return FBR_OK;
}

namespace {

// Everything the ingest holds, or nothing: a set-up that fails part-way leaves `g` for the caller to
// empty, so the next call starts over instead of finding a copy stream over missing buffers.
// (static: this anonymous namespace stands inside extern "C", where the compiler exports its functions)
static bool ingest_setup(fbr_ctx* c, Ingest& g) {
  const int64_t mb = knobs::stage_mb();
  g.chunk_bytes = std::max<int64_t>(mb << 20, c->NMAX * (int64_t)sizeof(fbr_point_xyzirt));
  g.chunk_bytes = (g.chunk_bytes + 63) & ~(int64_t)63;  // 16-B aligned records for the streaming stores
  // 16 packing threads (the CPU share of a one-GPU box; 8 -> 16: ingest line +10-20 %, r06m/r06n)
  g.nthreads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (const int t = knobs::stage_threads()) g.nthreads = t;
  if (!g.cstream.create(hipStreamNonBlocking)) return false;
  if (knobs::ingest_xstream() && !(g.xstream.create(hipStreamNonBlocking) && g.copied_ev.create(hipEventDisableTiming)))
    return false;
  for (auto& e : g.up_ev)
    if (!e.create(hipEventDisableTiming)) return false;
  for (auto& e : g.chunk_ev)
    if (!e.create(hipEventDisableTiming)) return false;
  if (dalloc(g.h_stage, (size_t)g.chunk_bytes * Ingest::kChunks) || dalloc(g.d_pts1, (int64_t)c->Bcap * c->NMAX))
    return false;
  g.d_pts_slot[0] = c->d_pts_own;
  g.d_pts_slot[1] = g.d_pts1;
  for (int k = 0; k < (g.xstream ? 2 : 1); ++k)
    if (dalloc(g.d_stage[k], (int64_t)c->Bcap * ingest_region_bytes(c->NMAX))) return false;
  return !dalloc(g.d_nin, 4 * (int64_t)c->Bcap) && !dalloc(g.h_nin, 4 * (int64_t)c->Bcap);
}

int ingest_init(fbr_ctx* c) {
  if (c->ing.cstream) return FBR_OK;
  if (ingest_setup(c, c->ing)) return FBR_OK;
  c->ing = Ingest{};
  return FBR_ERR_HIP;
}

// One scan's compact record (fbr_kernels.h: ingest_plane / ingest_region_bytes) at the 16-B aligned
// `out`, in one pass over the caller's 24-B points.  Groups of 16 points go out as streaming stores
// (no read-for-ownership of the pinned chunk, and the caller's points are read once); a ring at or
// beyond H (projectPointCloud drops it, imageProjection.cpp:599) is stored as 255 when rb = 1.
void pack_compact(const fbr_point_xyzirt* src, int64_t n, int H, int rb, uint8_t* out) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  const int64_t m = ingest_plane(n);
  float* px = reinterpret_cast<float*>(out);
  float* py = px + m;
  float* pz = py + m;
  uint8_t* rr = out + 12 * m;
  auto ring8 = [&](const fbr_point_xyzirt& p) { return p.ring < H ? (uint8_t)p.ring : (uint8_t)255; };
  int64_t i = 0;
  if (knobs::ingest_nt())
    for (; i + 16 <= n; i += 16) {
      const fbr_point_xyzirt* s = src + i;
      for (int g = 0; g < 4; ++g) {
        const fbr_point_xyzirt* q = s + 4 * g;
        __builtin_nontemporal_store(f4{q[0].x, q[1].x, q[2].x, q[3].x}, reinterpret_cast<f4*>(px + i + 4 * g));
        __builtin_nontemporal_store(f4{q[0].y, q[1].y, q[2].y, q[3].y}, reinterpret_cast<f4*>(py + i + 4 * g));
        __builtin_nontemporal_store(f4{q[0].z, q[1].z, q[2].z, q[3].z}, reinterpret_cast<f4*>(pz + i + 4 * g));
      }
      if (rb == 1) {
        u4 w;
        for (int g = 0; g < 4; ++g)
          w[g] = (unsigned)ring8(s[4 * g]) | (unsigned)ring8(s[4 * g + 1]) << 8 |
                 (unsigned)ring8(s[4 * g + 2]) << 16 | (unsigned)ring8(s[4 * g + 3]) << 24;
        __builtin_nontemporal_store(w, reinterpret_cast<u4*>(rr + i));  // 12 m and i are multiples of 16
      } else {
        for (int k = 0; k < 16; ++k) reinterpret_cast<uint16_t*>(rr)[i + k] = s[k].ring;
      }
    }
  for (; i < n; ++i) {
    px[i] = src[i].x;
    py[i] = src[i].y;
    pz[i] = src[i].z;
    if (rb == 1)
      rr[i] = ring8(src[i]);
    else
      reinterpret_cast<uint16_t*>(rr)[i] = src[i].ring;
  }
}

// Upload B scans into input slot `slot`: pack them into free pinned chunks (host threads), queue
// one H2D copy per chunk (compact records) or per scan (24-B records) on the copy stream, expand the
// compact records into the slot's scan buffer, then record up_ev[slot].  Runs on a worker thread
// while the previous device batch computes.
int ingest_upload(fbr_ctx* c, int slot, const fbr_point_xyzirt* const* scans, const int64_t* n_in, int B) {
  CK(enter(c));
  Ingest& g = c->ing;
  fbr_point_xyzirt* dst = g.d_pts_slot[slot];
  // compact records unless a deskew table may read the per-point time (deskewPoint, :545-580)
  const bool compact = knobs::ingest_compact() && !c->desk_any && !c->mot_field_any;
  g.compact_used = compact;
  // compact records expand into 16-B device records (k_project / k_compact read those)
  const bool pk = compact && knobs::packed_scans();
  g.pk_slot[slot] = pk;
  // ring bytes per point: u8 for sensors of < 256 rings, where every out-of-range ring (>= H, which
  // projectPointCloud drops, imageProjection.cpp:599) is stored as 255, still out of range
  const int rb = c->H < 256 ? 1 : 2;
  auto host_bytes = [&](int64_t n) {
    return compact ? 12 * ingest_plane(n) + rb * n : n * (int64_t)sizeof(fbr_point_xyzirt);
  };
  // k_expand_scans' counts and record offsets (the slot's half of the pinned array)
  int64_t* h_nin = g.h_nin + 2 * (int64_t)slot * c->Bcap;
  int64_t* h_off = h_nin + c->Bcap;
  uint8_t* dstage = g.d_stage[g.xstream ? slot : 0];
  int64_t dpos = 0;  // dstage offset of the next chunk: the chunks land back to back
  std::vector<int64_t> off;
  for (int j = 0; j < B;) {
    const int k = g.next_chunk;
    g.next_chunk = (k + 1) % Ingest::kChunks;
    if (g.chunk_used[k]) CK(hipEventSynchronize(g.chunk_ev[k]));  // its previous copies are done
    uint8_t* base = g.h_stage + (int64_t)k * g.chunk_bytes;
    int j1 = j;
    int64_t used = 0;
    off.clear();
    while (j1 < B && used + host_bytes(n_in[j1]) <= g.chunk_bytes) {
      off.push_back(used);
      used += (host_bytes(n_in[j1]) + 15) & ~(int64_t)15;
      ++j1;
    }
    if (j1 == j) return FBR_ERR_CAPACITY;  // (chunk_bytes >= NMAX * 24: not reached)
    const int64_t end = off.back() + host_bytes(n_in[j1 - 1]);  // the chunk's bytes
    for (int jj = j; jj < j1; ++jj) {
      h_nin[jj] = n_in[jj];
      h_off[jj] = dpos + off[jj - j];
    }
    const int nt = std::max(1, std::min(g.nthreads, j1 - j));
    auto pack = [&](int t) {
      for (int jj = j + t; jj < j1; jj += nt) {
        const int64_t n = n_in[jj];
        if (!n) continue;
        if (!compact) {
          std::memcpy(base + off[jj - j], scans[jj], n * sizeof(fbr_point_xyzirt));
          continue;
        }
        pack_compact(scans[jj], n, c->H, rb, base + off[jj - j]);
      }
      if (knobs::ingest_nt()) __builtin_ia32_sfence();  // the streaming stores before the DMA reads them
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(pack, t);
    pack(0);
    for (auto& x : th) x.join();
    // compact records: the whole chunk in one copy (1.4 MB copies ran at 41 GB/s on the box, 64 MB
    // ones at 57: tools/h2d_probe.py); 24-B records straight into their scan slots
    if (compact)
      CK(hipMemcpyAsync(dstage + dpos, base, end, hipMemcpyHostToDevice, g.cstream));
    else
      for (int jj = j; jj < j1; ++jj)
        if (n_in[jj])
          CK(hipMemcpyAsync(dst + (int64_t)jj * c->NMAX, base + off[jj - j], n_in[jj] * sizeof(fbr_point_xyzirt),
                            hipMemcpyHostToDevice, g.cstream));
    CK(hipEventRecord(g.chunk_ev[k], g.cstream));
    dpos += (end + 15) & ~(int64_t)15;
    g.chunk_used[k] = true;
    for (int jj = j; jj < j1; ++jj) g.h2d_bytes += (double)(n_in[jj] ? host_bytes(n_in[jj]) : 0);
    j = j1;
  }
  if (compact) {  // stream order: after the copies
    int64_t* d_nin = g.d_nin + 2 * (int64_t)slot * c->Bcap;
    CK(hipMemcpyAsync(d_nin, h_nin, sizeof(int64_t) * 2 * c->Bcap, hipMemcpyHostToDevice, g.cstream));
    hipStream_t es = g.cstream;
    if (g.xstream) {  // the expand off the copy stream: the next upload's copies start at once
      CK(hipEventRecord(g.copied_ev, g.cstream));
      CK(hipStreamWaitEvent(g.xstream, g.copied_ev, 0));
      es = g.xstream;
    }
    launch_expand_scans(es, dstage, c->NMAX, B, d_nin, d_nin + c->Bcap, rb, dst, pk);
    CK(hipEventRecord(g.up_ev[slot], es));
    return FBR_OK;
  }
  CK(hipEventRecord(g.up_ev[slot], g.cstream));
  return FBR_OK;
}

// Stage device batch `slot` whose scans ingest_upload queued: job metadata on the primary stream,
// which then waits for the slot's upload.
int ingest_stage(fbr_ctx* c, int slot, const int64_t* n_in, int B, const float* poses_in) {
  const int rc0 = drop_staged_batch(c);
  if (rc0) return rc0;
  c->no_time_call = false;
  c->d_pts = c->ing.d_pts_slot[slot];
  // 16-B records live in the slot's scan buffer (16 <= 24 B per point at the same NMAX stride)
  c->staged_pk = c->ing.pk_slot[slot] ? reinterpret_cast<const float4*>(c->d_pts) : nullptr;
  CK(hipMemcpyAsync(c->d_nin, n_in, sizeof(int64_t) * B, hipMemcpyHostToDevice, c->stream));
  CK(hipMemcpyAsync(c->d_guess, poses_in, sizeof(float) * 6 * B, hipMemcpyHostToDevice, c->stream));
  CK(hipStreamWaitEvent(c->stream, c->ing.up_ev[slot], 0));
  if (c->has_map && c->map_nocrop) {
    const int rc = crop_stats(c, Sub{0, B, 0, c->stream});
    if (rc) return rc;
  }
  CK(hipEventRecord(c->ev_staged, c->stream));
  CK(fbr_sync(c->stream));  // n_in / poses_in are the caller's
  c->crop_cached = c->has_map && c->map_nocrop;
  c->staged_B = B;
  c->staged_24 = !c->staged_pk;
  c->staged_nin.assign(n_in, n_in + B);
  return FBR_OK;
}

}  // namespace

// Independent jobs in device batches of max_batch.  The scans go through pinned staging on a copy
// stream, double-buffered: batch k+1 is packed and copied while batch k computes.
int fbr_process_batch(fbr_ctx* c, const fbr_point_xyzirt* const* scans, const int64_t* n_in, int n_jobs,
                      float* poses_inout, fbr_reg_stats* stats) {
  if (!c || !scans || !n_in || !poses_inout || n_jobs < 0) return FBR_ERR_INVALID_ARG;
  for (int j = 0; j < n_jobs; ++j) {  // validated before anything is copied
    if (n_in[j] < 0 || n_in[j] > c->NMAX) return FBR_ERR_CAPACITY;
    if (n_in[j] && !scans[j]) return FBR_ERR_INVALID_ARG;
  }
  if (n_jobs == 0) return FBR_OK;
  if (!c->has_map) return FBR_ERR_NO_MAP;
  CK(enter(c));
  int rc = ingest_init(c);
  if (rc) return rc;
  c->ing.h2d_bytes = 0.0;
  const int nb = (n_jobs + c->Bcap - 1) / c->Bcap;
  auto first = [&](int b) { return b * c->Bcap; };
  auto count = [&](int b) { return std::min(c->Bcap, n_jobs - b * c->Bcap); };
  rc = ingest_upload(c, 0, scans, n_in, count(0));
  for (int b = 0; b < nb && !rc; ++b) {
    const int slot = b & 1, j0 = first(b), B = count(b);
    int up_rc = FBR_OK;
    std::thread up;
    if (b + 1 < nb)  // the other slot is free: batch b - 1 finished before its results were read
      up = std::thread([&, b] { up_rc = ingest_upload(c, slot ^ 1, scans + first(b + 1), n_in + first(b + 1), count(b + 1)); });
    rc = ingest_stage(c, slot, n_in + j0, B, poses_inout + 6 * j0);
    if (!rc) rc = fbr_batch_launch(c);
    if (!rc) rc = fbr_batch_wait(c);
    if (!rc) rc = fbr_batch_results(c, poses_inout + 6 * j0, stats ? stats + j0 : nullptr);
    if (up.joinable()) up.join();
    if (!rc) rc = up_rc;
  }
  (void)fbr_sync(c->ing.cstream);
  if (c->ing.xstream) (void)fbr_sync(c->ing.xstream);
  c->d_pts = c->ing.d_pts_slot[0];
  if (rc) (void)drop_staged_batch(c);
  return rc;
}

int fbr_ingest_bytes(fbr_ctx* c, double* h2d_bytes) {
  if (!c || !h2d_bytes) return FBR_ERR_INVALID_ARG;
  *h2d_bytes = c->ing.h2d_bytes;
  return FBR_OK;
}

}  // extern "C"
