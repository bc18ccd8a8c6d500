// fbr_comm.hip — the library's own RCCL communicator (fbr_comm_*) and fbr_batch_allgather.
//
// ---------------------------------------------------------------------------------------------
// RCCL pose gather.  librccl is opened on first use (dlopen, RTLD_LOCAL): a host
// that never builds a communicator does not need it, and a process that already holds RCCL (torch)
// shares the loaded copy through its soname.  Only the types come from the header.
// ---------------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "fbr_ctx.h"

namespace {
struct RcclApi {
  bool ok = false;
  ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
  ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*comm_abort)(ncclComm_t) = nullptr;
  ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*group_start)() = nullptr;
  ncclResult_t (*group_end)() = nullptr;
};
const RcclApi& rccl() {
  static const RcclApi api = [] {
    RcclApi a;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) return a;
    a.get_unique_id = (decltype(a.get_unique_id))dlsym(h, "ncclGetUniqueId");
    a.comm_init_rank = (decltype(a.comm_init_rank))dlsym(h, "ncclCommInitRank");
    a.comm_destroy = (decltype(a.comm_destroy))dlsym(h, "ncclCommDestroy");
    a.comm_abort = (decltype(a.comm_abort))dlsym(h, "ncclCommAbort");
    a.all_gather = (decltype(a.all_gather))dlsym(h, "ncclAllGather");
    a.group_start = (decltype(a.group_start))dlsym(h, "ncclGroupStart");
    a.group_end = (decltype(a.group_end))dlsym(h, "ncclGroupEnd");
    a.ok = a.get_unique_id && a.comm_init_rank && a.comm_destroy && a.comm_abort && a.all_gather && a.group_start &&
           a.group_end;
    return a;
  }();
  return api;
}
}  // namespace

struct __attribute__((visibility("hidden"))) fbr_comm {
  ncclComm_t nc = nullptr;
  int dev = 0, nranks = 0, rank = 0, max_jobs = 0;
  Dev<float> send;        // [max_jobs][8] this rank's padded records
  Event done;             // after the latest all-gather: the next one (on another launch's
  bool used = false;      // stream) reuses `send` and the caller's recv buffer
  Event ev_wait;          // the caller's reader of recv (fbr_batch_allgather's wait_stream)
  bool failed = false;    // a call returned an error: peers may be blocked, destroy aborts

  // Deleted on its own device, after `nc` has been ended (abort or destroy: fbr_comm_destroy,
  // fbr_comm_create_local's cleanup); the handles then release themselves.
  // this rank's send block and events; false on a failure (the caller deletes the communicator)
  bool init(int max_jobs_per_rank) {
    return dalloc(send, 8 * (size_t)max_jobs_per_rank) == FBR_OK && done.create(hipEventDisableTiming) &&
           ev_wait.create(hipEventDisableTiming);
  }
};

extern "C" {

int fbr_comm_unique_id(uint8_t id_out[FBR_COMM_ID_BYTES]) {
  static_assert(FBR_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  if (!id_out) return FBR_ERR_INVALID_ARG;
  if (!rccl().ok) return FBR_ERR_UNSUPPORTED;
  ncclUniqueId id;
  if (rccl().get_unique_id(&id) != ncclSuccess) return FBR_ERR_HIP;
  std::memcpy(id_out, id.internal, FBR_COMM_ID_BYTES);
  return FBR_OK;
}

int fbr_comm_create(fbr_comm** out, fbr_ctx* c, const uint8_t id[FBR_COMM_ID_BYTES], int nranks, int rank,
                    int max_jobs_per_rank) {
  if (!out || !c || !id || nranks < 1 || rank < 0 || rank >= nranks || max_jobs_per_rank < 1) return FBR_ERR_INVALID_ARG;
  *out = nullptr;
  // every batch this ctx can stage fits the rank's block: the collective never fails on capacity
  if (max_jobs_per_rank < c->Bcap) return FBR_ERR_CAPACITY;
  if (!rccl().ok) return FBR_ERR_UNSUPPORTED;
  CK(enter(c));
  fbr_comm* m = new fbr_comm();
  m->dev = c->dev;
  m->nranks = nranks;
  m->rank = rank;
  m->max_jobs = max_jobs_per_rank;
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, FBR_COMM_ID_BYTES);
  // comm_init_rank blocks until every rank has joined (bootstrap over the id's socket)
  if (!m->init(max_jobs_per_rank) || rccl().comm_init_rank(&m->nc, nranks, uid, rank) != ncclSuccess) {
    delete m;
    return FBR_ERR_HIP;
  }
  *out = m;
  return FBR_OK;
}

int fbr_comm_create_local(fbr_comm** out, fbr_ctx* const* ctxs, int n, int max_jobs_per_rank) {
  if (!out || !ctxs || n < 1 || max_jobs_per_rank < 1) return FBR_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return FBR_ERR_INVALID_ARG;
    for (int j = 0; j < i; ++j)
      if (ctxs[j]->dev == ctxs[i]->dev) return FBR_ERR_INVALID_ARG;  // one rank per device
    if (max_jobs_per_rank < ctxs[i]->Bcap) return FBR_ERR_CAPACITY;
  }
  if (!rccl().ok) return FBR_ERR_UNSUPPORTED;
  ncclUniqueId uid;
  if (rccl().get_unique_id(&uid) != ncclSuccess) return FBR_ERR_HIP;
  std::vector<fbr_comm*> m(n, nullptr);
  auto cleanup = [&] {
    for (fbr_comm* q : m) {
      if (!q) continue;
      (void)hipSetDevice(q->dev);
      if (q->nc) (void)rccl().comm_abort(q->nc);
      delete q;
    }
  };
  for (int i = 0; i < n; ++i) {
    if (enter(ctxs[i]) != hipSuccess) {
      cleanup();
      return FBR_ERR_HIP;
    }
    m[i] = new fbr_comm();
    m[i]->dev = ctxs[i]->dev;
    m[i]->nranks = n;
    m[i]->rank = i;
    m[i]->max_jobs = max_jobs_per_rank;
    if (!m[i]->init(max_jobs_per_rank)) {
      cleanup();
      return FBR_ERR_HIP;
    }
  }
  // every device's rank from this thread: the inits form one group (RCCL would otherwise wait in
  // the first init for ranks this thread has not started yet)
  bool ok = rccl().group_start() == ncclSuccess;
  for (int i = 0; ok && i < n; ++i) {
    ok = hipSetDevice(m[i]->dev) == hipSuccess && rccl().comm_init_rank(&m[i]->nc, n, uid, i) == ncclSuccess;
  }
  ok = (rccl().group_end() == ncclSuccess) && ok;
  if (!ok) {
    cleanup();
    return FBR_ERR_HIP;
  }
  for (int i = 0; i < n; ++i) out[i] = m[i];
  return FBR_OK;
}

int fbr_comm_destroy(fbr_comm* m) {
  if (!m) return FBR_ERR_INVALID_ARG;
  (void)hipSetDevice(m->dev);
  int rc = FBR_OK;
  // after a failed collective the peers may be inside an all-gather this rank never joined:
  // abort (tear down without the collective handshake) instead of destroying
  if (m->nc && (m->failed ? rccl().comm_abort(m->nc) : rccl().comm_destroy(m->nc)) != ncclSuccess) rc = FBR_ERR_HIP;
  delete m;
  return rc;
}

namespace {
int batch_allgather(fbr_ctx* c, fbr_comm* m, int64_t launch_id, void* recv, void* wait_stream, void** done_stream) {
  if (m->dev != c->dev) return FBR_ERR_INVALID_ARG;
  if (c->staged_B <= 0 || c->launch_seq == 0) return FBR_ERR_STATE;
  if (c->staged_B > m->max_jobs) return FBR_ERR_CAPACITY;  // unreachable: fbr_comm_create checks max_batch
  if (launch_id < 0) launch_id = c->launch_seq - 1;
  if (launch_id < c->first_valid || launch_id >= c->launch_seq) return FBR_ERR_STATE;
  int s = -1;
  for (int q = 0; q < c->nslot; ++q)
    if (c->slot_launch[q] == launch_id) s = q;
  if (s < 0) return FBR_ERR_STATE;  // its slot has been reused by a later launch
  CK(enter(c));
  int rc = advance_runs(c, s);  // the launch fully enqueued (the host follows its GN flags)
  if (rc) return rc;
  const GnRun& r = c->run[s];
  hipStream_t st = r.s[0].sub.st;
  for (int k = 1; k < r.nsub; ++k) CK(hipStreamWaitEvent(st, c->xev[r.s[k].sub.k], 0));
  if (m->used) CK(hipStreamWaitEvent(st, m->done, 0));  // the previous gather (maybe another stream)
  if (wait_stream) {  // the caller's reads of the previous result out of recv
    CK(hipEventRecord(m->ev_wait, (hipStream_t)wait_stream));
    CK(hipStreamWaitEvent(st, m->ev_wait, 0));
  }
  const int64_t w0 = (int64_t)s * c->Bcap;
  if (c->staged_B < m->max_jobs)  // padding records: zeros
    CK(hipMemsetAsync(m->send + 8 * (int64_t)c->staged_B, 0, sizeof(float) * 8 * (m->max_jobs - c->staged_B), st));
  launch_export_records(st, c->staged_B, c->d_pose_out + w0 * 6, c->d_stats + w0, c->d_err + w0, c->d_guess, m->send);
  CK(hipGetLastError());
  if (rccl().all_gather(m->send, recv, (size_t)8 * m->max_jobs, ncclFloat32, m->nc, st) != ncclSuccess) return FBR_ERR_HIP;
  CK(hipEventRecord(m->done, st));
  m->used = true;
  if (done_stream) *done_stream = (void*)st;
  else {
    CK(hipEventRecord(c->ev_ext, st));
    CK(hipStreamWaitEvent(c->stream, c->ev_ext, 0));
  }
  return FBR_OK;
}
}  // namespace

int fbr_batch_allgather(fbr_ctx* c, fbr_comm* m, int64_t launch_id, void* recv, void* wait_stream, void** done_stream) {
  if (!c || !m || !recv) return FBR_ERR_INVALID_ARG;
  if (done_stream) *done_stream = nullptr;
  const int rc = batch_allgather(c, m, launch_id, recv, wait_stream, done_stream);
  if (rc) m->failed = true;
  return rc;
}

}  // extern "C"
