// Z = Q^T B for a tall-skinny Q (m x n, m >> n <= 256) and a few right-hand sides: the expensive step of the least-squares solve on a
// CholeskyQR2 factorization (cap_cacqr_apply_qt / cap_cacqr_solve, csrc/cacqr.hip).  Not in the reference, which stops at Q and R.
//
// The product reads Q exactly once and is bound by HBM.  dgemm_tn_skinny_kernel (gemm.hip) has the same operand form - TN, both operands
// K-contiguous, Q's columns as the A operand of v_mfma_f64_16x16x4_f64 and B's columns as its B operand - but gives one wave 16 output
// rows and the WHOLE K range: 16 waves on the chip at n = 256.  Here the K range (the rows of Q) is what is split:
//
//   tall_tn_kernel         one workgroup per SLAB of rows, one wave per 16 columns of Q (n / 16 waves: 16 at n = 256).  Lane (lr, kg)
//                          feeds column 16 w + lr of Q and right-hand side lr at k = k0 + 2 kg, + 1 (the k permutation of the other
//                          kernels), sixteen 16-byte loads in flight per lane.  No LDS, no barrier: the waves of a workgroup are
//                          independent and all read the SAME piece of B - the first wave's miss fetches it from HBM, the other
//                          n / 16 - 1 waves find it in the CU's L1 / the XCD's L2.  Loads are the bound, so the MFMA chains are short
//                          (8 per accumulator) and sparse, and fresh accumulators every 64 k keep the rounding error of a slab
//                          independent of its height.  Every slab writes its n x 16 partial to the work buffer with plain vector stores.
//   tall_tn_reduce_kernel  Z = the sum of the slabs in a fixed order (16 interleaved groups, each ascending, combined through LDS in
//                          a fixed tree): no floating-point atomics, the same bits on every run.
//
// Slab height: one slab per CU (a CU holds one 16-wave workgroup of this kernel), at least 512 rows, a multiple of 64.  At m = 2^21 on
// 256 CUs: 256 slabs of 8192 rows, 8 MiB of partials (0.2 % of Q's bytes).
//
// Measured at 2^21 x 256 (profiles/r09_cacqr_solve.txt has the variants): 1.03 ms at 8 right-hand sides = 4.3 TB/s, where a linear read of
// Q's bytes takes 0.67 ms (6.4 TB/s) in the same run.  What was tried and is NOT here: non-temporal loads of Q (1.36 ms: a lane quartet
// covers 64 B of a column per load, the second half of every 128-byte line then misses instead of hitting the line in flight); two or
// four slabs per CU (+ 4 %); a rotated start row per wave (no gain); B staged once per workgroup through LDS (- 3 % at 8, - 14 % at 16
// right-hand sides, + 8 % at 1: not worth a second kernel and a barrier); two column groups per wave sharing the B registers (- 4 %).
// Where the rest goes: the loads alone (no B, no MFMA) take 0.83 ms on the plan's Q, whose columns are 2^24 bytes apart (0.71 ms with
// the leading dimension padded by 528); B re-read by every wave costs 0 ... 0.3 ms with nrhs; and a wave issuing fp64 MFMAs keeps the
// other waves of its SIMD from issuing loads.
#include <algorithm>

#include "common.h"

namespace {

constexpr int TT_RHS = 16;                 // right-hand sides per launch: the 16 columns of the MFMA's B operand
constexpr int TT_MAX_N = 256;              // 16 waves x 16 columns
constexpr int64_t TT_SLAB_MIN = 512;
constexpr int TT_SLABS_PER_CU = 1;
// More than this many right-hand sides go to the 128 x 128 tile kernel, which pads them to 128 and costs the same up to there, instead of
// ceil(nrhs / 16) passes over Q.  Measured at 2^21 x 256 (profiles/r09_cacqr_solve.txt): one tile product 4.56 - 4.60 ms for nrhs = 32 ... 64;
// two passes 2.42 ms, three 3.60 ms, four 4.80 ms - three passes still win, four do not.
constexpr int64_t TT_TILE_CROSSOVER = 48;

struct TallArgs { const double* Q; const double* B; double* P; int64_t ldq, ldb, m, slab; int n, nrhs; };

__global__ void __launch_bounds__(1024) tall_tn_kernel(const TallArgs g) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * g.slab;
  const int64_t rows = std::min<int64_t>(g.slab, g.m - r0);          // > 0: the grid is ceil(m / slab); a multiple of 8
  const bool bon = lr < g.nrhs;
  const double* __restrict__ pa = g.Q + (int64_t)(16 * wid + lr) * g.ldq + r0 + 2 * kg;
  const double* __restrict__ pb = g.B + (int64_t)(bon ? lr : 0) * g.ldb + r0 + 2 * kg;
  d4 sum = {0.0, 0.0, 0.0, 0.0};
  int64_t k0 = 0;
  for (; k0 + 64 <= rows; k0 += 64) {          // 8 x (8 k): sixteen 16-byte loads in flight per lane
    d2 a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; u++) a[u] = *reinterpret_cast<const d2*>(pa + k0 + 8 * u);
#pragma unroll
    for (int u = 0; u < 8; u++) b[u] = *reinterpret_cast<const d2*>(pb + k0 + 8 * u);     // lanes past nrhs re-read column 0 (same lines) ...
#pragma unroll
    for (int u = 0; u < 8; u++) b[u] = bon ? b[u] : (d2){0.0, 0.0};                          // ... and drop it: no branch around the loads
    d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 8; u++) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u].x, b[u].x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u].y, b[u].y, acc1, 0, 0, 0);
    }
    sum += acc0 + acc1;
  }
  if (k0 < rows) {                             // the last slab's ragged end, 8 k at a time
    d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (; k0 < rows; k0 += 8) {
      const d2 a = *reinterpret_cast<const d2*>(pa + k0);
      d2 b = *reinterpret_cast<const d2*>(pb + k0);
      b = bon ? b : (d2){0.0, 0.0};
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, acc1, 0, 0, 0);
    }
    sum += acc0 + acc1;
  }
  if (!bon) return;                            // D layout: row = kg + 4 r (column of Q), column = lr (right-hand side)
  double* P = g.P + ((int64_t)blockIdx.x * TT_RHS + lr) * g.n + 16 * wid + kg;
#pragma unroll
  for (int r = 0; r < 4; r++) P[4 * r] = sum[r];
}

// element e = row + n * rhs of Z sits at P[slab * 16 n + e]: 64 elements per workgroup, 16 groups of slabs
__global__ void __launch_bounds__(1024) tall_tn_reduce_kernel(const double* __restrict__ P, int nslab, int n, int nrhs, double* Z, int64_t ldz) {
  __shared__ double part[16][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const bool on = e < n * nrhs;
  const int64_t st = (int64_t)TT_RHS * n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (on) {
    const double* p = P + e;
    int z = grp;
    for (; z + 48 < nslab; z += 64) {
      s0 += p[z * st]; s1 += p[(z + 16) * st]; s2 += p[(z + 32) * st]; s3 += p[(z + 48) * st];
    }
    for (; z < nslab; z += 16) s0 += p[z * st];
  }
  part[grp][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (grp != 0 || !on) return;
  double t[8];
#pragma unroll
  for (int i = 0; i < 8; i++) t[i] = part[2 * i][lane] + part[2 * i + 1][lane];
  Z[e % n + (int64_t)(e / n) * ldz] = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

int64_t tall_slab(int64_t m) {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  else (void)hipGetLastError();
  if (cus <= 0) cus = 256;
  return std::max<int64_t>(TT_SLAB_MIN, cap_round_up(cap_ceil_div(std::max<int64_t>(m, 1), (int64_t)TT_SLABS_PER_CU * cus), 64));
}

bool tall_kernel_takes(int64_t m, int64_t n, const double* Q, int64_t ldq, const double* B, int64_t ldb) {
  return m >= 8 && m % 8 == 0 && n % 16 == 0 && n <= TT_MAX_N && !(ldq & 1) && !(ldb & 1) && !((uintptr_t)Q & 15) && !((uintptr_t)B & 15);
}

}  // namespace

extern "C" {

int64_t cap_dgemm_tall_tn_work_size(int64_t m, int64_t n, int64_t nrhs) {
  if (m <= 0 || n <= 0 || nrhs <= 0) return 0;
  return cap_ceil_div(m, tall_slab(m)) * TT_RHS * cap_round_up(n, 16);
}

int cap_dgemm_tall_tn(int64_t m, int64_t n, int64_t nrhs, const double* Q, int64_t ldq, const double* B, int64_t ldb, double* Z, int64_t ldz,
                      double* work, void* stream) {
  if (m < 0 || n < 0 || nrhs < 0) return CAP_ERR_ARG;
  if (n == 0 || nrhs == 0) return CAP_OK;
  if (!Z || ldz < n || (m > 0 && (!Q || !B || ldq < m || ldb < m))) return CAP_ERR_ARG;
  hipStream_t s = cap_stream(stream);
  if (m == 0) return cap_zero_rect(Z, ldz, n, nrhs, s);
  if (!tall_kernel_takes(m, n, Q, ldq, B, ldb) || nrhs > TT_TILE_CROSSOVER)
    return cap_gemm_launch(CAP_TRANS, CAP_NOTRANS, n, nrhs, m, 1.0, Q, ldq, B, ldb, 0.0, Z, ldz, 0, s, cap_plain_device_ptr(Z) ? 0 : CAP_TAG_NO_ATOMIC);
  if (!work) return CAP_ERR_ARG;
  const int64_t slab = tall_slab(m), nslab = cap_ceil_div(m, slab);
  for (int64_t c0 = 0; c0 < nrhs; c0 += TT_RHS) {          // the work buffer is reused in stream order
    const int cnt = (int)std::min<int64_t>(TT_RHS, nrhs - c0);
    TallArgs g{Q, B + c0 * ldb, work, ldq, ldb, m, slab, (int)n, cnt};
    cap_acc_r(Q, ldq, m, n); cap_acc_r(g.B, ldb, m, cnt); cap_acc_w(work, 0, nslab * TT_RHS * n, 1);
    hipLaunchKernelGGL(tall_tn_kernel, dim3((unsigned)nslab), dim3((unsigned)(4 * n)), 0, s, g);
    CAP_HIP(hipGetLastError());
    cap_acc_r(work, 0, nslab * TT_RHS * n, 1); cap_acc_w(Z + c0 * ldz, ldz, n, cnt);
    hipLaunchKernelGGL(tall_tn_reduce_kernel, dim3((unsigned)cap_ceil_div(n * cnt, 64)), dim3(1024), 0, s, work, (int)nslab, (int)n, cnt,
                       Z + c0 * ldz, ldz);
    CAP_HIP(hipGetLastError());
  }
  return CAP_OK;
}

}  // extern "C"
