// k_selftest.hip — device numerics probe behind fbr_selftest_math (diagnostic entry point).
//
// The path's bit-exactness rests on a few device primitives matching the reference's host libm:
// correctly rounded f32 sqrt and division (SSE sqrtss / divss), glibc atan2f
// (imageProjection.cpp:605,618) and glibc sinf / cosf (pcl::getTransformation, LMOptimization
// mapOptmization.h:1259-1264).  tests/test_gpu_parity.py feeds random operands through this
// kernel and compares every output bit with the host.  Also here: the per-query functions of the
// Gauss-Newton residual pass, its workgroup reduction and the 6x6 solvers on caller-given inputs
// (fbr_selftest_gn_rows / _gn_reduce / _solve6, tests/test_gn_rows.py), the selftests of the introsort
// partition phase and of the wave-chunk radix sorts (fbr_vg_sort.h), and the bandwidth / VALU probes.
#include <algorithm>

#include "fbr_common.h"
#include "fbr_fdlibm.h"
#include "fbr_gn.h"
#include "fbr_sincosf.h"
#include "fbr_introsort.h"
#include "fbr_solvers.h"
#include "fbr_vg_sort.h"

namespace fbr {

constexpr int kSelftestMathOut = 6;

__global__ void k_selftest_math(int n, const float* a, const float* b, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = a[i], y = b[i];
  float* o = out + (int64_t)kSelftestMathOut * i;
  o[0] = sqrt_rn(x < 0.0f ? -x : x);
  o[1] = x / y;
  o[2] = fd_atan2f(x, y);
  o[3] = x * y + y * x - x;  // plain mul/add with contraction disabled
  o[4] = gl_sinf(x);
  o[5] = gl_cosf(x);
}

// One 64-lane workgroup per symmetric 6x6 matrix: the single-lane jacobi_eigen<6> (lane 0) and the
// wave-parallel jacobi_eigen_wave<6>; out = 2 x (6 eigenvalues + 36 eigenvector entries).
__global__ void __launch_bounds__(64) k_selftest_eigen6(const float* a, float* out) {
  __shared__ float A[36], V[36], W[6];
  __shared__ int R[6], C[6];
  const int m = blockIdx.x, lane = threadIdx.x;
  float* o = out + (int64_t)m * 84;
  if (lane == 0) {
    float Ar[36], Wr[6], Vr[36];
    for (int k = 0; k < 36; ++k) Ar[k] = a[(int64_t)m * 36 + k];
    jacobi_eigen<6>(Ar, Wr, Vr);
    for (int k = 0; k < 6; ++k) o[k] = Wr[k];
    for (int k = 0; k < 36; ++k) o[6 + k] = Vr[k];
  }
  if (lane < 36) A[lane] = a[(int64_t)m * 36 + lane];
  __syncthreads();
  jacobi_eigen_wave<6>(A, W, V, R, C);
  if (lane < 6) o[42 + lane] = W[lane];
  if (lane < 36) o[48 + lane] = V[lane];
}

// out[i] = 1 when eig_above_certified<6> certifies every eigenvalue of matrix i above `thr`.
__global__ void k_selftest_eig_cert(int n, const float* a, float thr, int32_t* out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) out[m] = eig_above_certified<6>(a + (int64_t)m * 36, thr) ? 1 : 0;
}

// One lane per case: fbr_gn.h's fits, residual coefficients and LMOptimization row on caller-given
// neighbours, query, scan point and trig (fbr_selftest_gn_rows; layouts in include/fbr.h).
constexpr int kGnRowsIn = 28, kGnRowsOut = 20;
__global__ void k_selftest_gn_rows(int n, const float* in, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* c = in + (int64_t)kGnRowsIn * i;
  float* o = out + (int64_t)kGnRowsOut * i;
  const bool corner = c[0] == 0.0f;
  Nbr5 nn;
  for (int j = 0; j < 5; ++j) { nn.x[j] = c[1 + 3 * j]; nn.y[j] = c[2 + 3 * j]; nn.z[j] = c[3 + 3 * j]; }
  const float x0 = c[16], y0 = c[17], z0 = c[18];
  const float4 p = make_float4(c[19], c[20], c[21], 0.0f);
  GnState g{};
  for (int k = 0; k < 6; ++k) g.trig[k] = c[22 + k];
  float fit[6] = {0, 0, 0, 0, 0, 0}, row[6] = {0, 0, 0, 0, 0, 0}, b = 0.0f;
  float4 coeff = make_float4(0, 0, 0, 0);
  const bool fit_ok = corner ? corner_fit(nn, fit) : surf_fit(nn, fit);
  bool ok = false;
  if (fit_ok) {
    corner ? corner_apply(fit, x0, y0, z0, coeff) : surf_apply(fit, x0, y0, z0, coeff);
    ok = res_apply_row(g, corner, fit, p, x0, y0, z0, row, b);
  }
  o[0] = fit_ok ? 1.0f : 0.0f;
  for (int k = 0; k < 6; ++k) o[1 + k] = fit_ok ? fit[k] : 0.0f;
  o[7] = ok ? 1.0f : 0.0f;
  o[8] = coeff.x; o[9] = coeff.y; o[10] = coeff.z; o[11] = coeff.w;
  for (int k = 0; k < 6; ++k) o[12 + k] = row[k];
  o[18] = b;
  o[19] = 0.0f;
}

// One 256-thread workgroup per set of rows: res_reduce as gn_residual_item calls it (a lane
// without an accepted row passes zeros).
__global__ void __launch_bounds__(kResThreads) k_selftest_gn_reduce(const float* rows, const int8_t* okf, double* out) {
  __shared__ double red[kResThreads / 64][28];
  const int tid = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * kResThreads + tid;
  float row[6] = {0, 0, 0, 0, 0, 0}, b = 0.0f;
  const bool ok = okf[q] != 0;
  if (ok) {
    for (int k = 0; k < 6; ++k) row[k] = rows[q * 7 + k];
    b = rows[q * 7 + 6];
  }
  res_reduce(red, tid, row, b, ok, out + (int64_t)blockIdx.x * kPartial);
}

// One lane per 6x6 system: qr_solve6 and lu_inv6.
__global__ void k_selftest_solve6(int n, const float* a, const float* b, float* x, float* inv, int32_t* ret) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float A[36], X[6], Bi[36];
  for (int k = 0; k < 36; ++k) A[k] = a[(int64_t)36 * i + k];
  for (int k = 0; k < 6; ++k) X[k] = b[(int64_t)6 * i + k];
  ret[2 * i + 1] = lu_inv6(A, Bi);
  ret[2 * i] = qr_solve6(A, X);
  for (int k = 0; k < 6; ++k) x[(int64_t)6 * i + k] = X[k];
  for (int k = 0; k < 36; ++k) inv[(int64_t)36 * i + k] = Bi[k];
}

// std::sort's partition phase (fbr_introsort.h) on one array: lds = 0 keeps everything in global
// memory (the device-wide VoxelGrid's variant), lds = 1 the keys / values / positions in LDS
// (n <= kIsortLdsCap, the per-segment kernels' variant), lds = 2 keys / values in LDS and the
// positions in global memory (the mapping-DS kernel's variant).  v[] ends as the permuted indices.
constexpr int kIsortLdsCap = 8192;
__global__ void __launch_bounds__(1024) k_selftest_isort(uint32_t* k, uint32_t* v, int32_t* posL, int32_t* posR,
                                                         int* fa, int* fb, int n, int lds) {
  __shared__ int sh[64];
  if (!lds) {
    is_partition_phase<1024>(k, v, posL, posR, n, fa, fb, sh);
    return;
  }
  __shared__ uint32_t lk[kIsortLdsCap];
  __shared__ uint16_t lv[kIsortLdsCap], lpl[kIsortLdsCap], lpr[kIsortLdsCap];
  __shared__ int lfa[3 * (kIsortLdsCap / 17 + 2)], lfb[3 * (kIsortLdsCap / 17 + 2)];
  for (int i = threadIdx.x; i < n; i += 1024) {
    lk[i] = k[i];
    lv[i] = (uint16_t)i;
  }
  is_partition_phase<1024>((FBR_IS_LDS uint32_t*)lk, (FBR_IS_LDS uint16_t*)lv, (FBR_IS_LDS uint16_t*)lpl,
                           (FBR_IS_LDS uint16_t*)lpr, n, (FBR_IS_LDS int*)lfa, (FBR_IS_LDS int*)lfb, sh);
  for (int i = threadIdx.x; i < n; i += 1024) {
    k[i] = lk[i];
    v[i] = lv[i];
  }
}

// lds = 2: keys / values in LDS up to the mapping-DS kernel's 1024 * 18 points, positions in
// global memory (k_voxel_grid_ip's variant).
constexpr int kIsortLdsCap2 = 1024 * 18;
__global__ void __launch_bounds__(1024) k_selftest_isort2(uint32_t* k, uint32_t* v, int32_t* posL, int32_t* posR,
                                                          int n) {
  __shared__ int sh[64];
  __shared__ uint32_t lk[kIsortLdsCap2];
  __shared__ uint16_t lv[kIsortLdsCap2];
  __shared__ int lfa[3 * (kIsortLdsCap2 / 17 + 2)], lfb[3 * (kIsortLdsCap2 / 17 + 2)];
  for (int i = threadIdx.x; i < n; i += 1024) {
    lk[i] = k[i];
    lv[i] = (uint16_t)i;
  }
  is_partition_phase<1024>((FBR_IS_LDS uint32_t*)lk, (FBR_IS_LDS uint16_t*)lv, posL, posR, n, (FBR_IS_LDS int*)lfa,
                           (FBR_IS_LDS int*)lfb, sh);
  for (int i = threadIdx.x; i < n; i += 1024) {
    k[i] = lk[i];
    v[i] = lv[i];
  }
}

// lds = 3: the per-ring filter's shape -- 512 threads, everything in LDS (n <= 4096, u16
// positions) -- with the whole-workgroup partition from 128 elements up (the ring kernel uses 512)
// so that the block partition and its parallel K count see many frames.
constexpr int kIsortLdsCap3 = 4096;
__global__ void __launch_bounds__(512) k_selftest_isort3(uint32_t* k, uint32_t* v, int n) {
  __shared__ int sh[64];
  __shared__ uint32_t lk[kIsortLdsCap3];
  __shared__ uint16_t lv[kIsortLdsCap3], lpl[kIsortLdsCap3], lpr[kIsortLdsCap3];
  __shared__ int lfa[3 * (kIsortLdsCap3 / 17 + 2)], lfb[3 * (kIsortLdsCap3 / 17 + 2)];
  for (int i = threadIdx.x; i < n; i += 512) {
    lk[i] = k[i];
    lv[i] = (uint16_t)i;
  }
  is_partition_phase<512, FBR_IS_LDS uint32_t*, FBR_IS_LDS uint16_t*, FBR_IS_LDS uint16_t*, FBR_IS_LDS int*, 128>(
      (FBR_IS_LDS uint32_t*)lk, (FBR_IS_LDS uint16_t*)lv, (FBR_IS_LDS uint16_t*)lpl, (FBR_IS_LDS uint16_t*)lpr, n,
      (FBR_IS_LDS int*)lfa, (FBR_IS_LDS int*)lfb, sh);
  for (int i = threadIdx.x; i < n; i += 512) {
    k[i] = lk[i];
    v[i] = lv[i];
  }
}

// ---- radix sort selftests (fbr_selftest_radix_sort): one workgroup sorts one array with the
// product's configurations of the wave-chunk sorts ----
// variant 0: vg_radix_sort<512, u16, 8, LDS> (per-ring filter), 1: vg_radix_sort<256, u16, 9, LDS>
// (per-segment LDS kernel), 2: vg_radix_sort<1024, u32, 9, global> (global-scratch kernel),
// 3: vg_radix_sort_inplace<1024, 18> (mapping DS), 4: the same with ballot-leader digit counts,
// 5: round 3's rejected form (ballot-leader counts + wave-uniform early exits),
// 6: vg_radix_sort_inplace<256, 16> (the small size class of the mapping DS).
// (3 .. 6 run k_selftest_radix_ip, which k_voxel.hip keeps: see there.)
template <int T, typename V, int MAXD, bool KV_LDS>
__global__ void __launch_bounds__(T) k_selftest_radix(uint32_t* keys, uint32_t* vals, uint32_t* scratch, int n, int nbits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = T / 64;
  uint32_t* hist = (uint32_t*)smem;
  uint32_t* wsum = hist + (NW + 1) * 512;
  unsigned char* q = (unsigned char*)(wsum + NW);
  q = smem + (((q - smem) + 15) & ~15);
  uint32_t* kb[2];
  V* vb[2];
  if constexpr (KV_LDS) {
    kb[0] = (uint32_t*)q;
    kb[1] = kb[0] + n;
    vb[0] = (V*)(kb[1] + n);
    vb[1] = vb[0] + n;
  } else {
    kb[0] = scratch;
    kb[1] = scratch + n;
    vb[0] = (V*)(scratch + 2 * n);
    vb[1] = (V*)(scratch + 3 * n);
  }
  for (int i = threadIdx.x; i < n; i += T) {
    kb[0][i] = keys[i];
    vb[0][i] = (V)i;
  }
  __syncthreads();
  const int cur = vg_radix_sort<T, V, MAXD, KV_LDS>(kb, vb, n, nbits, hist, wsum);
  for (int i = threadIdx.x; i < n; i += T) {
    keys[i] = kb[cur][i];
    vals[i] = (uint32_t)vb[cur][i];
  }
}

}  // namespace fbr

// Diagnostic entry point (tests/test_gpu_parity.py): sort n keys (low nbits significant) with one of
// the product's radix sort configurations; keys_inout gets the sorted keys, perm the source index of
// each sorted position.
extern "C" int fbr_selftest_radix_sort(int64_t n, int nbits, int variant, uint32_t* keys_inout, uint32_t* perm) {
  using namespace fbr;
  const int64_t lcap[7] = {4096, 4096, 1 << 20, 1024 * kVgIpKpl, 1024 * kVgIpKpl, 1024 * kVgIpKpl,
                           kVgIpSmallT * kVgIpSmallKpl};
  if (n < 0 || variant < 0 || variant > 6 || n > lcap[variant] || nbits < 1 || nbits > 32 || (n && (!keys_inout || !perm)))
    return FBR_ERR_INVALID_ARG;
  if (n == 0) return FBR_OK;
  uint32_t *dk = nullptr, *dv = nullptr, *ds = nullptr;
  int rc = FBR_OK;
  if (hipMalloc(&dk, 4 * n) != hipSuccess || hipMalloc(&dv, 4 * n) != hipSuccess || hipMalloc(&ds, 16 * n) != hipSuccess ||
      hipMemcpy(dk, keys_inout, 4 * n, hipMemcpyHostToDevice) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    const int nn = (int)n;
    auto hdr = [](int T) { return (((size_t)(T / 64 + 1) * 512 + T / 64) * 4 + 15) & ~(size_t)15; };
    switch (variant) {
      case 0:
        hipLaunchKernelGGL((k_selftest_radix<512, uint16_t, 8, true>), dim3(1), dim3(512), hdr(512) + (size_t)n * 12, 0,
                           dk, dv, ds, nn, nbits);
        break;
      case 1:
        hipLaunchKernelGGL((k_selftest_radix<256, uint16_t, 9, true>), dim3(1), dim3(256), hdr(256) + (size_t)n * 12, 0,
                           dk, dv, ds, nn, nbits);
        break;
      case 2:
        hipLaunchKernelGGL((k_selftest_radix<1024, uint32_t, 9, false>), dim3(1), dim3(1024), hdr(1024), 0, dk, dv, ds,
                           nn, nbits);
        break;
      default:  // 3 .. 6: the in-place sort, whose selftest kernel stands with its product callers
        launch_selftest_radix_ip(variant, dk, dv, nn, nbits);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpy(keys_inout, dk, 4 * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(perm, dv, 4 * n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = FBR_ERR_HIP;
  }
  for (void* q : {(void*)dk, (void*)dv, (void*)ds}) (void)hipFree(q);
  return rc;
}

extern "C" int fbr_selftest_voxel_order(int64_t n, const uint32_t* keys, int lds, uint32_t* perm) {
  if (n < 0 || n > (int64_t)INT32_MAX / 4 || (n && (!keys || !perm)) || (lds == 1 && n > fbr::kIsortLdsCap) ||
      (lds == 2 && n > fbr::kIsortLdsCap2) || (lds == 3 && n > fbr::kIsortLdsCap3) || lds < 0 || lds > 3)
    return FBR_ERR_INVALID_ARG;
  if (n == 0) return FBR_OK;
  std::vector<uint32_t> iv(n);
  for (int64_t i = 0; i < n; ++i) iv[i] = (uint32_t)i;
  uint32_t *dk = nullptr, *dv = nullptr;
  int32_t *pl = nullptr, *pr = nullptr;
  int *fa = nullptr, *fb = nullptr;
  const int64_t nf = n / 17 + 2;
  int rc = FBR_OK;
  if (hipMalloc(&dk, 4 * n) != hipSuccess || hipMalloc(&dv, 4 * n) != hipSuccess || hipMalloc(&pl, 4 * n) != hipSuccess ||
      hipMalloc(&pr, 4 * n) != hipSuccess || hipMalloc(&fa, 3 * sizeof(int) * nf) != hipSuccess ||
      hipMalloc(&fb, 3 * sizeof(int) * nf) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else if (hipMemcpy(dk, keys, 4 * n, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(dv, iv.data(), 4 * n, hipMemcpyHostToDevice) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    if (lds == 3) hipLaunchKernelGGL(fbr::k_selftest_isort3, dim3(1), dim3(512), 0, 0, dk, dv, (int)n);
    else if (lds == 2) hipLaunchKernelGGL(fbr::k_selftest_isort2, dim3(1), dim3(1024), 0, 0, dk, dv, pl, pr, (int)n);
    else hipLaunchKernelGGL(fbr::k_selftest_isort, dim3(1), dim3(1024), 0, 0, dk, dv, pl, pr, fa, fb, (int)n, lds);
    if (hipMemcpy(perm, dv, 4 * n, hipMemcpyDeviceToHost) != hipSuccess) rc = FBR_ERR_HIP;
  }
  for (void* q : {(void*)dk, (void*)dv, (void*)pl, (void*)pr, (void*)fa, (void*)fb}) (void)hipFree(q);
  return rc;
}

extern "C" int fbr_selftest_eig_certified(int n, const float* a, float thr, int32_t* out) {
  if (n <= 0 || !a || !out) return FBR_ERR_INVALID_ARG;
  float* da = nullptr;
  int32_t* dout = nullptr;
  int rc = FBR_OK;
  if (hipMalloc(&da, sizeof(float) * 36 * n) != hipSuccess || hipMalloc(&dout, sizeof(int32_t) * n) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else if (hipMemcpy(da, a, sizeof(float) * 36 * n, hipMemcpyHostToDevice) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    hipLaunchKernelGGL(fbr::k_selftest_eig_cert, dim3((n + 63) / 64), dim3(64), 0, 0, n, da, thr, dout);
    if (hipMemcpy(out, dout, sizeof(int32_t) * n, hipMemcpyDeviceToHost) != hipSuccess) rc = FBR_ERR_HIP;
  }
  (void)hipFree(da);
  (void)hipFree(dout);
  return rc;
}

extern "C" int fbr_selftest_math(int n, const float* a, const float* b, float* out) {
  if (n <= 0 || !a || !b || !out) return FBR_ERR_INVALID_ARG;
  float *da = nullptr, *db = nullptr, *dout = nullptr;
  int rc = FBR_OK;
  if (hipMalloc(&da, sizeof(float) * n) != hipSuccess || hipMalloc(&db, sizeof(float) * n) != hipSuccess ||
      hipMalloc(&dout, sizeof(float) * fbr::kSelftestMathOut * n) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else if (hipMemcpy(da, a, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(db, b, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    hipLaunchKernelGGL(fbr::k_selftest_math, dim3((n + 255) / 256), dim3(256), 0, 0, n, da, db, dout);
    if (hipMemcpy(out, dout, sizeof(float) * fbr::kSelftestMathOut * n, hipMemcpyDeviceToHost) != hipSuccess) rc = FBR_ERR_HIP;
  }
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}

extern "C" int fbr_selftest_eigen6(int n, const float* a, float* out) {
  if (n <= 0 || !a || !out) return FBR_ERR_INVALID_ARG;
  float *da = nullptr, *dout = nullptr;
  int rc = FBR_OK;
  if (hipMalloc(&da, sizeof(float) * 36 * n) != hipSuccess || hipMalloc(&dout, sizeof(float) * 84 * n) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else if (hipMemcpy(da, a, sizeof(float) * 36 * n, hipMemcpyHostToDevice) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    hipLaunchKernelGGL(fbr::k_selftest_eigen6, dim3(n), dim3(64), 0, 0, da, dout);
    if (hipMemcpy(out, dout, sizeof(float) * 84 * n, hipMemcpyDeviceToHost) != hipSuccess) rc = FBR_ERR_HIP;
  }
  (void)hipFree(da);
  (void)hipFree(dout);
  return rc;
}

extern "C" int fbr_selftest_gn_rows(int n, const float* in, float* out) {
  if (n <= 0 || !in || !out) return FBR_ERR_INVALID_ARG;
  float *din = nullptr, *dout = nullptr;
  const size_t bi = sizeof(float) * fbr::kGnRowsIn * n, bo = sizeof(float) * fbr::kGnRowsOut * n;
  int rc = FBR_OK;
  if (hipMalloc(&din, bi) != hipSuccess || hipMalloc(&dout, bo) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else if (hipMemcpy(din, in, bi, hipMemcpyHostToDevice) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    hipLaunchKernelGGL(fbr::k_selftest_gn_rows, dim3((n + 63) / 64), dim3(64), 0, 0, n, din, dout);
    if (hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost) != hipSuccess) rc = FBR_ERR_HIP;
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}

extern "C" int fbr_selftest_gn_reduce(int n_sets, const float* rows, const int8_t* ok, double* out) {
  if (n_sets <= 0 || !rows || !ok || !out) return FBR_ERR_INVALID_ARG;
  float* drows = nullptr;
  int8_t* dok = nullptr;
  double* dout = nullptr;
  const size_t nq = (size_t)n_sets * fbr::kResThreads, bo = sizeof(double) * fbr::kPartial * n_sets;
  int rc = FBR_OK;
  if (hipMalloc(&drows, sizeof(float) * 7 * nq) != hipSuccess || hipMalloc(&dok, nq) != hipSuccess ||
      hipMalloc(&dout, bo) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else if (hipMemcpy(drows, rows, sizeof(float) * 7 * nq, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(dok, ok, nq, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dout, 0, bo) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    hipLaunchKernelGGL(fbr::k_selftest_gn_reduce, dim3(n_sets), dim3(fbr::kResThreads), 0, 0, drows, dok, dout);
    if (hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost) != hipSuccess) rc = FBR_ERR_HIP;
  }
  (void)hipFree(drows);
  (void)hipFree(dok);
  (void)hipFree(dout);
  return rc;
}

extern "C" int fbr_selftest_solve6(int n, const float* a, const float* b, float* x, float* inv, int32_t* ret) {
  if (n <= 0 || !a || !b || !x || !inv || !ret) return FBR_ERR_INVALID_ARG;
  float *da = nullptr, *db = nullptr, *dx = nullptr, *di = nullptr;
  int32_t* dr = nullptr;
  const size_t b36 = sizeof(float) * 36 * n, b6 = sizeof(float) * 6 * n, br = sizeof(int32_t) * 2 * n;
  int rc = FBR_OK;
  if (hipMalloc(&da, b36) != hipSuccess || hipMalloc(&db, b6) != hipSuccess || hipMalloc(&dx, b6) != hipSuccess ||
      hipMalloc(&di, b36) != hipSuccess || hipMalloc(&dr, br) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else if (hipMemcpy(da, a, b36, hipMemcpyHostToDevice) != hipSuccess ||
             hipMemcpy(db, b, b6, hipMemcpyHostToDevice) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    hipLaunchKernelGGL(fbr::k_selftest_solve6, dim3((n + 63) / 64), dim3(64), 0, 0, n, da, db, dx, di, dr);
    if (hipMemcpy(x, dx, b6, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(inv, di, b36, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ret, dr, br, hipMemcpyDeviceToHost) != hipSuccess)
      rc = FBR_ERR_HIP;
  }
  for (void* q : {(void*)da, (void*)db, (void*)dx, (void*)di, (void*)dr}) (void)hipFree(q);
  return rc;
}

// STREAM-copy probe (measurement helper, BASELINE.md "report vs measured STREAM-copy bandwidth"):
// float4 copies of `bytes` per direction, timed with HIP events over `iters` launches.  Three
// shapes are timed and the best is reported: a grid-stride loop, one float4 per thread with one
// workgroup per 4 KiB, and U float4 per thread (all loads issued before the stores, non-temporal
// stores) with one workgroup per U * 4 KiB.
namespace fbr {
__global__ void __launch_bounds__(256) k_stream_copy(const float4* __restrict__ a, float4* __restrict__ b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) b[i] = a[i];
}
template <int U>
__global__ void __launch_bounds__(256) k_stream_copy_u(const float4* __restrict__ a, float4* __restrict__ b, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * 256 * U + threadIdx.x;
  float4 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + (int64_t)u * 256;
    v[u] = i < n ? a[i] : make_float4(0, 0, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + (int64_t)u * 256;
    if (i < n) {
      __builtin_nontemporal_store(v[u].x, &b[i].x);
      __builtin_nontemporal_store(v[u].y, &b[i].y);
      __builtin_nontemporal_store(v[u].z, &b[i].z);
      __builtin_nontemporal_store(v[u].w, &b[i].w);
    }
  }
}
}  // namespace fbr

extern "C" int fbr_stream_copy_bandwidth(int hip_device, int64_t bytes, int iters, double* gbps) {
  if (bytes < 16 || iters <= 0 || !gbps) return FBR_ERR_INVALID_ARG;
  if (hipSetDevice(hip_device) != hipSuccess) return FBR_ERR_NO_DEVICE;
  const int64_t n = bytes / 16;
  float4 *a = nullptr, *b = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = FBR_OK;
  if (hipMalloc(&a, sizeof(float4) * n) != hipSuccess || hipMalloc(&b, sizeof(float4) * n) != hipSuccess ||
      hipMemset(a, 0, sizeof(float4) * n) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
      hipEventCreate(&e1) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    *gbps = 0.0;
    for (int variant = 0; variant < 3 && !rc; ++variant) {
      auto launch = [&]() {
        if (variant == 0)  // grid stride: 8 XCDs x 32 CUs, several workgroups per CU
          hipLaunchKernelGGL(fbr::k_stream_copy, dim3(256 * 8 * 4), dim3(256), 0, 0, a, b, n);
        else if (variant == 1)
          hipLaunchKernelGGL(fbr::k_stream_copy_u<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, a, b, n);
        else
          hipLaunchKernelGGL(fbr::k_stream_copy_u<4>, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, 0, a, b, n);
      };
      launch();  // warm-up
      (void)hipEventRecord(e0, 0);
      for (int k = 0; k < iters; ++k) launch();
      (void)hipEventRecord(e1, 0);
      float ms = 0.0f;
      if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0.0f)
        rc = FBR_ERR_HIP;
      else
        *gbps = std::max(*gbps, 2.0 * 16.0 * (double)n * iters / (ms * 1e-3) / 1e9);  // read + write
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(a);
  (void)hipFree(b);
  return rc;
}

// VALU issue-rate probe (measurement helper for the VALU roofline, bench.py / tools/valu_calib.py):
// every lane runs 8 independent dependency chains of one VALU instruction for `iters` rounds, written
// as inline asm so the compiler can neither pack (SLP) nor drop them.  kind 0: v_fma_f32, 1:
// v_add_u32, 2: v_pk_fma_f32 (2 lanes of f32 per slot), 3: v_cmp_lt_u64, 4: v_cmp_lt_u32 (both
// into SGPR pairs: the compares of the kNN list insertion).  The grid is n_cu * waves_per_simd
// workgroups of 256 threads (4 waves: one per SIMD), so every SIMD holds waves_per_simd waves.
namespace fbr {
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int KIND>
__global__ void __launch_bounds__(256) k_valu_peak(float* out, int iters, float a, float b) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if constexpr (KIND == 0) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (float)(t + u);
    for (int i = 0; i < iters; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(x[u]) : "v"(a), "v"(b));
    }
    float s = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += x[u];
    out[t] = s;
  } else if constexpr (KIND == 1) {
    uint32_t x[8];
    const uint32_t ia = __float_as_uint(a);
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (uint32_t)(t + u);
    for (int i = 0; i < iters; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("v_add_u32 %0, %1, %0" : "+v"(x[u]) : "v"(ia));
    }
    uint32_t s = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += x[u];
    out[t] = (float)s;
  } else if constexpr (KIND == 3 || KIND == 4) {  // 64-bit / 32-bit unsigned compares into SGPR pairs
    uint64_t x[8], m[8];
    const uint64_t y = (uint64_t)__float_as_uint(a) << 20;
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = (uint64_t)(t + u) << 16;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if constexpr (KIND == 3) asm volatile("v_cmp_lt_u64_e64 %0, %1, %2" : "=s"(m[u]) : "v"(x[u]), "v"(y));
          else asm volatile("v_cmp_lt_u32_e64 %0, %1, %2" : "=s"(m[u]) : "v"((uint32_t)x[u]), "v"((uint32_t)y));
        }
    }
    uint64_t s = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) s ^= m[u];
    out[t] = (float)(s & 0xffff);
  } else {
    f32x2 x[8];
    f32x2 va = {a, a}, vb = {b, b};
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = f32x2{(float)(t + u), (float)(t - u)};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 8; ++u) asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(x[u]) : "v"(va), "v"(vb));
    }
    float s = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += x[u].x + x[u].y;
    out[t] = s;
  }
}
}  // namespace fbr

// Wave-level VALU instructions per second of the probe above (32 per lane per round, timed with HIP
// events over `reps` launches after one warm-up launch).
extern "C" int fbr_valu_peak(int hip_device, int waves_per_simd, int kind, int iters, int reps, double* ginst_per_s,
                             double* ms_per_launch) {
  if (waves_per_simd < 1 || waves_per_simd > 8 || kind < 0 || kind > 4 || iters <= 0 || reps <= 0 || !ginst_per_s)
    return FBR_ERR_INVALID_ARG;
  if (hipSetDevice(hip_device) != hipSuccess) return FBR_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, hip_device) != hipSuccess) return FBR_ERR_HIP;
  const int blocks = prop.multiProcessorCount * waves_per_simd;
  float* out = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = FBR_OK;
  if (hipMalloc(&out, sizeof(float) * 256 * blocks) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
      hipEventCreate(&e1) != hipSuccess) {
    rc = FBR_ERR_HIP;
  } else {
    auto launch = [&]() {
      if (kind == 0) hipLaunchKernelGGL(fbr::k_valu_peak<0>, dim3(blocks), dim3(256), 0, 0, out, iters, 1.0000001f, 0.5f);
      else if (kind == 1) hipLaunchKernelGGL(fbr::k_valu_peak<1>, dim3(blocks), dim3(256), 0, 0, out, iters, 1.0000001f, 0.5f);
      else if (kind == 2) hipLaunchKernelGGL(fbr::k_valu_peak<2>, dim3(blocks), dim3(256), 0, 0, out, iters, 1.0000001f, 0.5f);
      else if (kind == 3) hipLaunchKernelGGL(fbr::k_valu_peak<3>, dim3(blocks), dim3(256), 0, 0, out, iters, 1.0000001f, 0.5f);
      else hipLaunchKernelGGL(fbr::k_valu_peak<4>, dim3(blocks), dim3(256), 0, 0, out, iters, 1.0000001f, 0.5f);
    };
    launch();
    (void)hipEventRecord(e0, 0);
    for (int k = 0; k < reps; ++k) launch();
    (void)hipEventRecord(e1, 0);
    float ms = 0.0f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0.0f) {
      rc = FBR_ERR_HIP;
    } else {
      const double waves = 4.0 * blocks;
      *ginst_per_s = waves * 32.0 * iters * reps / (ms * 1e-3) / 1e9;
      if (ms_per_launch) *ms_per_launch = ms / reps;
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(out);
  return rc;
}
