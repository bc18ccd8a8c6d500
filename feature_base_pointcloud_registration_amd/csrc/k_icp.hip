// k_icp.hip — loop closure's ICP on the device (performLoopClosure, mapOptmization.h:689-711).
//
// PCL's IterativeClosestPoint with TransformationEstimationSVD and DefaultConvergenceCriteria, no
// rejectors, guess = identity, as include/fbr.h restates it.  One iteration is
//   k_icp_nn      one thread per source point: applies the previous iteration's transform to X
//                 (in place), then the exact nearest target point over a grid of the ICP's own:
//                 the query's cell, then Chebyshev shells of cells around it, until the shell's
//                 lower bound exceeds the best d2 found (or the distance gate), or every cell of the
//                 box has been seen.  Queries not finished after kIcpShells shells are queued.
//   k_icp_far     the queued queries against the whole target, 256 queries per workgroup, target
//                 tiles of 1024 points in LDS, the target split over gridDim.y workgroups.
//   k_icp_reduce  count, sum s, sum t, sum t s^T, sum d2 of the correspondences in double, one
//                 partial per workgroup.
//   k_icp_solve   one wave: partials summed in a fixed order, Umeyama (3x3 one-sided Jacobi SVD in
//                 double, fbr_icp_solve.h), final = T * final, the convergence rules, the host's
//                 stop word.
// A correspondence is the 64-bit key (d2 bits << 32) | target index: non-negative floats order as
// their bit patterns, so the smallest key is the smallest d2 and, among equal d2, the lowest
// index.  The grid kernel stores a finished query's key; the far kernel's target splits combine
// with a 64-bit integer atomicMin, whose result does not depend on arrival order.  No float or
// double atomics anywhere: two runs on the same input give the same bytes.
// Once the state's `stopped` word is set, the iteration kernels the host had already enqueued
// return at once.  The fitness pass (mode 1) runs the search on final * source without a gate.
// The k_icp_*_batch kernels advance many pairs in the same launches over the same bodies (below,
// "many pairs per launch"): a pair's bytes do not depend on which kernels ran it.
#include <math.h>

#include "fbr_common.h"
#include "fbr_icp_solve.h"
#include "fbr_kernels.h"
#include "fbr_pace.h"

namespace fbr {

namespace {

constexpr int kIcpShells = 3;       // shells searched on the grid before a query is queued
constexpr int kIcpTile = 1024;      // target points per LDS tile of k_icp_far
constexpr unsigned long long kIcpNone = ~0ull;

__device__ __forceinline__ void icp_consider(const float4 p, uint32_t id, float qx, float qy, float qz, float& best,
                                             uint32_t& bi) {
  const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
  const float d = (dx * dx + dy * dy) + dz * dz;  // flann::L2_Simple
  if (d < best || (d == best && id < bi)) {
    best = d;
    bi = id;
  }
}

// The bodies below are shared by the single-pair kernels (k_icp_*: the block in the pair is
// blockIdx.x) and the batch kernels (k_icp_*_batch: pair and block from the block table): one copy
// of the arithmetic, so a pair gets the same bytes either way.
__device__ __forceinline__ void icp_init_body(const IcpArgs& a) {
  IcpState* st = a.st;
  for (int k = 0; k < 12; ++k) st->T[k] = st->fin[k] = (k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f;
  st->prev_mse = DBL_MAX;
  st->stopped = st->converged = st->convergence = st->iterations = st->ncorr = 0;
  *a.far_cnt = 0;
}

__global__ void k_icp_init(IcpArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  icp_init_body(a);
}

__device__ __forceinline__ void icp_nn_body(const IcpArgs& a, int blk, int mode, int first) {
  const IcpState* st = a.st;
  if (mode == 0 && st->stopped) return;
  const int64_t i = (int64_t)blk * 256 + threadIdx.x;
  if (i >= a.n) return;
  float4 p = (mode || first) ? a.src[i] : a.x[i];
  if (mode) p = associate(st->fin, p);
  else if (!first) p = associate(st->T, p);
  a.x[i] = p;
  if (!map_point_finite(p)) {  // no correspondence
    a.key[i] = kIcpNone;
    return;
  }
  float best = INFINITY;
  uint32_t bi = 0xFFFFFFFFu;
  bool done = false;
  const GridDesc& g = a.grid.g;
  const float fx = floorf(p.x * g.inv_x), fy = floorf(p.y * g.inv_cell), fz = floorf(p.z * g.inv_cell);
  // (cell indices beyond 1e7 are not exact in float: such a query is far from every dense box)
  if (a.use_grid && fabsf(fx) < 1.0e7f && fabsf(fy) < 1.0e7f && fabsf(fz) < 1.0e7f) {
    const int qx = (int)fx - (int)g.origin[0], qy = (int)fy - (int)g.origin[1], qz = (int)fz - (int)g.origin[2];
    const int dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    // cells between the query's cell and the box / the farthest cell of the box (Chebyshev)
    const int r_out = max(max(max(-qx, qx - (dx - 1)), max(-qy, qy - (dy - 1))), max(max(-qz, qz - (dz - 1)), 0));
    const int r_all = max(max(max(qx, dx - 1 - qx), max(qy, dy - 1 - qy)), max(qz, dz - 1 - qz));
    const float cell = 1.0f / g.inv_cell;
    const float4* __restrict__ pts = a.grid.pts;
    const int32_t* __restrict__ cs = a.grid.cell_start;
    if (r_out <= kIcpShells) {
      for (int r = 0;; ++r) {
        if (r > r_all) {  // every cell of the box has been searched
          done = true;
          break;
        }
        if (r >= 1) {
          // a point of shell r or beyond is at least (r - 1) cells away along some axis; the 0.999
          // covers the rounding of the float d2 it is compared with
          const float lb = (float)(r - 1) * cell;
          const float lb2 = lb * lb * 0.999f;
          if (lb2 > best || (double)lb2 > a.gate2) {
            done = true;
            break;
          }
        }
        if (r > kIcpShells) break;
        const int z0 = max(qz - r, 0), z1 = min(qz + r, dz - 1), y0 = max(qy - r, 0), y1 = min(qy + r, dy - 1);
        for (int z = z0; z <= z1; ++z) {
          for (int y = y0; y <= y1; ++y) {
            const int64_t row = ((int64_t)z * dy + y) * dx;
            if (abs(z - qz) == r || abs(y - qy) == r) {  // a face of the shell: the whole x range
              const int xa = max(qx - r, 0), xb = min(qx + r, dx - 1);
              if (xa <= xb) {
                const int e = cs[row + xb + 1];
                for (int k = cs[row + xa]; k < e; ++k) {
                  const float4 t = pts[k];
                  icp_consider(t, __float_as_uint(t.w), p.x, p.y, p.z, best, bi);
                }
              }
            } else {  // inside: the two end cells (r > 0 here)
              for (int side = 0; side < 2; ++side) {
                const int x = side ? qx + r : qx - r;
                if (x < 0 || x >= dx) continue;
                const int e = cs[row + x + 1];
                for (int k = cs[row + x]; k < e; ++k) {
                  const float4 t = pts[k];
                  icp_consider(t, __float_as_uint(t.w), p.x, p.y, p.z, best, bi);
                }
              }
            }
          }
        }
      }
    }
  }
  if (done) {
    a.key[i] = bi == 0xFFFFFFFFu ? kIcpNone : ((unsigned long long)__float_as_uint(best) << 32) | bi;
  } else {
    a.key[i] = kIcpNone;
    const int slot = atomicAdd(a.far_cnt, 1);  // slot < n: one per query
    a.far_list[slot] = (int32_t)i;
  }
}

__global__ void __launch_bounds__(256) k_icp_nn(IcpArgs a, int mode, int first) { icp_nn_body(a, blockIdx.x, mode, first); }

// split / nsplit: this workgroup's part of the target's tiles (every member of the workgroup gets
// the same values: the returns below are the whole workgroup's)
__device__ __forceinline__ void icp_far_body(const IcpArgs& a, int blk, int split, int nsplit, int mode) {
  __shared__ float4 tile[kIcpTile];
  if (mode == 0 && a.st->stopped) return;
  const int cnt = *a.far_cnt;
  const int q0 = blk * 256;
  if (q0 >= cnt) return;  // (the whole workgroup)
  const int qi = q0 + (int)threadIdx.x < cnt ? a.far_list[q0 + threadIdx.x] : -1;
  const float4 q = qi >= 0 ? a.x[qi] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float best = INFINITY;
  uint32_t bi = 0xFFFFFFFFu;
  for (int64_t t0 = (int64_t)split * kIcpTile; t0 < a.nt; t0 += (int64_t)nsplit * kIcpTile) {
    __syncthreads();
    for (int k = threadIdx.x; k < kIcpTile; k += 256) {
      float4 t = make_float4(NAN, NAN, NAN, 0.0f);  // past the end / non-finite: never a candidate
      if (t0 + k < a.nt) {
        const float4 v = a.tgt[t0 + k];
        if (map_point_finite(v)) t = v;
      }
      tile[k] = t;
    }
    __syncthreads();
    const int m = (int)min((int64_t)kIcpTile, a.nt - t0);
    for (int k = 0; k < m; ++k) icp_consider(tile[k], (uint32_t)(t0 + k), q.x, q.y, q.z, best, bi);
  }
  if (qi >= 0 && bi != 0xFFFFFFFFu) atomicMin(&a.key[qi], ((unsigned long long)__float_as_uint(best) << 32) | bi);
}

__global__ void __launch_bounds__(256) k_icp_far(IcpArgs a, int mode) {
  icp_far_body(a, blockIdx.x, blockIdx.y, gridDim.y, mode);
}

// partial[b][0..16] = count, sum s (3), sum t (3), sum t_r s_c (9), sum d2 of block b's queries
__device__ __forceinline__ void icp_reduce_body(const IcpArgs& a, int blk, int mode) {
  __shared__ double sh[4][kIcpSums];
  if (mode == 0 && a.st->stopped) return;
  const int64_t i = (int64_t)blk * 256 + threadIdx.x;
  double v[17];
#pragma unroll
  for (int k = 0; k < 17; ++k) v[k] = 0.0;
  if (i < a.n) {
    const unsigned long long key = a.key[i];
    if (key != kIcpNone) {
      const float d2 = __uint_as_float((uint32_t)(key >> 32));
      if ((double)d2 <= a.gate2) {
        const float4 s = a.x[i];
        const float4 t = a.tgt[(uint32_t)key];
        const double sv[3] = {(double)s.x, (double)s.y, (double)s.z}, tv[3] = {(double)t.x, (double)t.y, (double)t.z};
        v[0] = 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          v[1 + r] = sv[r];
          v[4 + r] = tv[r];
#pragma unroll
          for (int c = 0; c < 3; ++c) v[7 + 3 * r + c] = tv[r] * sv[c];
        }
        v[16] = (double)d2;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 17; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 17; ++k) sh[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 17)
    a.partial[(int64_t)blk * kIcpSums + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

__global__ void __launch_bounds__(256) k_icp_reduce(IcpArgs a, int mode) { icp_reduce_body(a, blockIdx.x, mode); }

// The workgroup partials summed by one wave: lane l takes blocks l, l + 64, ... in order, then a
// butterfly (every lane ends with the same bits).
__device__ __forceinline__ void icp_sum_partials(const double* partial, int nblk, double* v) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 17; ++k) v[k] = 0.0;
  for (int b = lane; b < nblk; b += 64)
#pragma unroll
    for (int k = 0; k < 17; ++k) v[k] += partial[(int64_t)b * kIcpSums + k];
#pragma unroll
  for (int k = 0; k < 17; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
}

// One wave.  Returns -1 to every lane but the one that ran an iteration's solve (lane 0 of a pair
// that had not stopped), and to that one whether the pair stopped now (1) or goes on (0).
__device__ __forceinline__ int icp_solve_body(const IcpArgs& a, int nblk, int max_iter, double teps, double feps) {
  IcpState* st = a.st;
  const int was_stopped = st->stopped;
  if (threadIdx.x == 0) *a.far_cnt = 0;  // the next search's queue
  if (was_stopped) return -1;
  double v[17];
  icp_sum_partials(a.partial, nblk, v);
  if (threadIdx.x != 0) return -1;
  const double n = v[0];
  st->ncorr = (int32_t)n;
  int stop = 0;
  if (n < 3.0) {
    st->converged = 0;
    st->convergence = FBR_ICP_NO_CORRESPONDENCES;
    stop = 1;
  } else {
    float T[12];
    icp_umeyama(v, T);
    float F[12], G[12];
    for (int k = 0; k < 12; ++k) F[k] = st->fin[k];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) {
        float s = (T[4 * r] * F[c] + T[4 * r + 1] * F[4 + c]) + T[4 * r + 2] * F[8 + c];
        if (c == 3) s = s + T[4 * r + 3];
        G[4 * r + c] = s;
      }
    for (int k = 0; k < 12; ++k) {
      st->T[k] = T[k];
      st->fin[k] = G[k];
    }
    const int it = ++st->iterations;
    if (it >= max_iter) {
      st->converged = 1;
      st->convergence = FBR_ICP_ITERATIONS;
      stop = 1;
    } else {
      const double cosang = 0.5 * ((((double)T[0] + (double)T[5]) + (double)T[10]) - 1.0);
      const double t2 = ((double)T[3] * (double)T[3] + (double)T[7] * (double)T[7]) + (double)T[11] * (double)T[11];
      if (cosang >= 1.0 - teps && t2 <= teps) {
        st->converged = 1;
        st->convergence = FBR_ICP_TRANSFORM;
        stop = 1;
      } else {
        const double mse = v[16] / n, prev = st->prev_mse;
        if (fabs(mse - prev) < 1e-12) {
          st->converged = 1;
          st->convergence = FBR_ICP_ABS_MSE;
          stop = 1;
        } else if (fabs(mse - prev) / prev < feps) {
          st->converged = 1;
          st->convergence = FBR_ICP_REL_MSE;
          stop = 1;
        }
        st->prev_mse = mse;
      }
    }
  }
  st->stopped = stop;
  return stop;
}

// The host's progress word (fbr_pace.h), by one lane.
__device__ __forceinline__ void icp_publish(unsigned long long* flag, unsigned long long gen, uint32_t iters, unsigned stop) {
  __threadfence_system();
  __hip_atomic_store(flag, pace::pack_progress(gen, iters, stop), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(64)
k_icp_solve(IcpArgs a, int nblk, int max_iter, double teps, double feps, unsigned long long gen) {
  const int stop = icp_solve_body(a, nblk, max_iter, teps, feps);
  if (stop >= 0 && a.flag) icp_publish(a.flag, gen, (uint32_t)a.st->iterations, (unsigned)stop);
}

// After the fitness pass: getFitnessScore and the result record.
__device__ __forceinline__ void icp_finish_body(const IcpArgs& a, int nblk, fbr_icp_result* out) {
  double v[17];
  icp_sum_partials(a.partial, nblk, v);
  if (threadIdx.x != 0) return;
  *a.far_cnt = 0;
  const IcpState* st = a.st;
  out->converged = st->converged;
  out->convergence = st->convergence;
  out->iterations = st->iterations;
  out->n_correspondences = st->ncorr;
  out->fitness = v[0] > 0.0 ? v[16] / v[0] : DBL_MAX;
  for (int k = 0; k < 12; ++k) out->transform[k] = st->fin[k];
  out->transform[12] = out->transform[13] = out->transform[14] = 0.0f;
  out->transform[15] = 1.0f;
}

__global__ void __launch_bounds__(64) k_icp_finish(IcpArgs a, int nblk, fbr_icp_result* out) { icp_finish_body(a, nblk, out); }

// ---- many pairs per launch ------------------------------------------------------------------------
// args[pair] is that pair's IcpArgs over its own parts of the pools; table[workgroup] = {pair, block
// in the pair}, every pair's blocks counted from its own query 0 (fbr_loop_plan.h).  Workgroups
// of a stopped pair return at once, as the single-pair kernels do.
__device__ __forceinline__ int icp_pair_blocks(const IcpArgs& a) { return a.n > 0 ? (int)((a.n + 255) / 256) : 0; }

__global__ void __launch_bounds__(64) k_icp_init_batch(const IcpArgs* args, int npairs, IcpBatchCtl* ctl) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p == 0) {
    ctl->running = npairs;
    ctl->ticket = 0;
    ctl->launches = 0;
  }
  if (p < npairs) icp_init_body(args[p]);
}

__global__ void __launch_bounds__(256) k_icp_nn_batch(const IcpArgs* args, const int2* table, int mode, int first) {
  const int2 e = table[blockIdx.x];
  const IcpArgs a = args[e.x];
  icp_nn_body(a, e.y, mode, first);
}

// gridDim.y is the launch's largest target split; a pair's workgroups beyond its own return.  (The
// 64-bit atomicMin makes a pair's keys independent of how its target is split.)
__global__ void __launch_bounds__(256) k_icp_far_batch(const IcpArgs* args, const int2* table, const int32_t* nsplit, int mode) {
  const int2 e = table[blockIdx.x];
  const int ns = nsplit[e.x];
  if ((int)blockIdx.y >= ns) return;
  const IcpArgs a = args[e.x];
  icp_far_body(a, e.y, blockIdx.y, ns, mode);
}

__global__ void __launch_bounds__(256) k_icp_reduce_batch(const IcpArgs* args, const int2* table, int mode) {
  const int2 e = table[blockIdx.x];
  const IcpArgs a = args[e.x];
  icp_reduce_body(a, e.y, mode);
}

// One wave per pair.  A pair that stops leaves the count of running pairs; the workgroup that draws
// the launch's last ticket publishes (launches done, nobody running) to the host.  The state a
// solve writes is read by later launches only, so the ticket orders nothing but the count.
__global__ void __launch_bounds__(64)
k_icp_solve_batch(const IcpArgs* args, int npairs, IcpBatchCtl* ctl, int max_iter, double teps, double feps,
                  unsigned long long gen, unsigned long long* flag) {
  const IcpArgs a = args[blockIdx.x];
  const int stop = icp_solve_body(a, icp_pair_blocks(a), max_iter, teps, feps);
  if (threadIdx.x != 0) return;
  if (stop > 0) (void)__hip_atomic_fetch_add(&ctl->running, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  const int ticket = __hip_atomic_fetch_add(&ctl->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != npairs - 1) return;
  __threadfence();
  __hip_atomic_store(&ctl->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the next launch's
  const uint32_t done = ++ctl->launches;  // (the winner's alone; launches follow each other on the stream)
  const int running = __hip_atomic_load(&ctl->running, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (flag) icp_publish(flag, gen, done, running == 0 ? 1u : 0u);
}

__global__ void __launch_bounds__(64) k_icp_finish_batch(const IcpArgs* args, fbr_icp_result* out) {
  const IcpArgs a = args[blockIdx.x];
  icp_finish_body(a, icp_pair_blocks(a), out + blockIdx.x);
}

inline int icp_blocks(int64_t n) { return (int)std::max<int64_t>(1, (n + 255) / 256); }

}  // namespace

void launch_icp_init(hipStream_t s, const IcpArgs& a) { fbr_launch(k_icp_init, dim3(1), dim3(64), 0, s, a); }

void launch_icp_nn(hipStream_t s, const IcpArgs& a, int mode, int first) {
  if (a.n <= 0) return;
  fbr_launch(k_icp_nn, dim3(icp_blocks(a.n)), dim3(256), 0, s, a, mode, first);
}

void launch_icp_far(hipStream_t s, const IcpArgs& a, int mode) {
  if (a.n <= 0) return;
  fbr_launch(k_icp_far, dim3(icp_blocks(a.n), icp_far_split(a.nt)), dim3(256), 0, s, a, mode);
}

void launch_icp_solve(hipStream_t s, const IcpArgs& a, int max_iter, double teps, double feps, unsigned long long gen) {
  const int nblk = a.n > 0 ? icp_blocks(a.n) : 0;
  if (nblk) fbr_launch(k_icp_reduce, dim3(nblk), dim3(256), 0, s, a, 0);
  fbr_launch(k_icp_solve, dim3(1), dim3(64), 0, s, a, nblk, max_iter, teps, feps, gen);
}

void launch_icp_finish(hipStream_t s, const IcpArgs& a, fbr_icp_result* out) {
  const int nblk = a.n > 0 ? icp_blocks(a.n) : 0;
  if (nblk) fbr_launch(k_icp_reduce, dim3(nblk), dim3(256), 0, s, a, 1);
  fbr_launch(k_icp_finish, dim3(1), dim3(64), 0, s, a, nblk, out);
}

int icp_far_split(int64_t nt) { return (int)std::min<int64_t>(std::max<int64_t>((nt + kIcpTile - 1) / kIcpTile, 1), 32); }

void launch_icp_init_batch(hipStream_t s, const IcpBatch& b) {
  fbr_launch(k_icp_init_batch, dim3((b.npairs + 63) / 64), dim3(64), 0, s, b.args, b.npairs, b.ctl);
}

void launch_icp_nn_batch(hipStream_t s, const IcpBatch& b, int mode, int first) {
  if (b.nblocks <= 0) return;
  fbr_launch(k_icp_nn_batch, dim3(b.nblocks), dim3(256), 0, s, mode ? b.args_fit : b.args, b.table, mode, first);
}

void launch_icp_far_batch(hipStream_t s, const IcpBatch& b, int mode) {
  if (b.nblocks <= 0) return;
  fbr_launch(k_icp_far_batch, dim3(b.nblocks, b.max_split), dim3(256), 0, s, mode ? b.args_fit : b.args, b.table, b.nsplit, mode);
}

void launch_icp_solve_batch(hipStream_t s, const IcpBatch& b, int max_iter, double teps, double feps, unsigned long long gen) {
  if (b.nblocks > 0) fbr_launch(k_icp_reduce_batch, dim3(b.nblocks), dim3(256), 0, s, b.args, b.table, 0);
  fbr_launch(k_icp_solve_batch, dim3(b.npairs), dim3(64), 0, s, b.args, b.npairs, b.ctl, max_iter, teps, feps, gen, b.flag);
}

void launch_icp_finish_batch(hipStream_t s, const IcpBatch& b, fbr_icp_result* out) {
  if (b.nblocks > 0) fbr_launch(k_icp_reduce_batch, dim3(b.nblocks), dim3(256), 0, s, b.args_fit, b.table, 1);
  fbr_launch(k_icp_finish_batch, dim3(b.npairs), dim3(64), 0, s, b.args_fit, out);
}

}  // namespace fbr
