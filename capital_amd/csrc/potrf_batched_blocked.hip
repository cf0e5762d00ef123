// Batched Cholesky factor and solve for SPD blocks of 65 .. 256 rows (cap_dpotrf_batched_blocked, cap_dpotrs_batched_blocked): the arguments,
// layout, info / logdet and argument rules of potrf_batched.hip, whose launches serve n <= 64 here too (same kernels, same bits).
//
// ONE WORKGROUP PER BLOCK, nothing between workgroups: 1-D grid, no atomics, no spin waits, no reads of another workgroup's data, no scratch.
// A block no longer fits a wave's registers and at n = 256 its triangle does not fit the LDS either: the block stays in its own memory (512 KB
// at most: L2) and a right-looking blocked factorization walks over diagonal blocks of NB = 64 rows - the size at which the diagonal step is
// the in-register column algorithm of potrf_batched.hip on one wave.  The factor is templated on NBLK = ceil(n / 64) = 2, 3, 4, which sizes the
// static LDS (50 / 82.5 / 115 KiB) and the workgroup: four waves at NBLK = 2, where LDS and registers (about 210 per lane) let two workgroups
// share a CU, eight waves at NBLK = 3, 4, where the LDS holds one workgroup and the second wave per SIMD overlaps the memory latency of the
// staging and of the trailing update.  The solve has four waves and 50.5 KiB.
//
// Factor, step k0 = 0, 64, ... (nb = min(64, n - k0) rows, m = n - k0 - 64 trailing columns):
//   A. all waves: upper triangle of the diagonal block -> the packed LDS image (consecutive lanes along a column), and, when m > 0, the 64 x m
//      row panel A12 -> LDS (element (j, c) at j LDP + c, LDP odd: conflict-free with lanes along j and with lanes along c; columns up to the
//      next multiple of 16 are zeros).
//   B. wave 0: lane c takes column c of the image into registers and runs the 64 fully unrolled steps - pivot a_jj read from lane j, correctly
//      rounded square root and division, row j of R to the image, a_ic -= r_ji r_jc with r_ji read from lane i (v_readlane: no LDS round trip
//      in the chain).  The first pivot that is not > 0 (NaN included) sets info and turns this row and every later one into NaN.
//   C. all waves: R11 image -> memory; wave w: lane l owns column 64 w + l of the panel, R12 = R11^-T A12 by substitution (divide, then
//      independent fused multiply-adds against LDS broadcasts of R11), result back to the panel in LDS.
//   D. all waves: panel -> memory, and A22 -= R12^T R12 on the fp64 16 x 16 x 4 MFMA: the 16 x 16 tiles that intersect the upper triangle are
//      dealt round-robin to the waves; a tile's C values come from the block's memory and go back there, both operands from the LDS panel
//      (K = 64: sixteen MFMAs per tile).  Elements below the diagonal or beyond n are neither loaded nor stored.
// NaN rows of a failed block spread by themselves: row j of R11 is NaN, so are the quotients by r_jj in R12, so is every trailing element.
// Every block sees the same instruction sequence on its own data: its bits depend on (n, its data) only; all global accesses are 8-byte ones,
// so there is one load path whatever the alignment.
//
// Solve, right-hand sides in passes of 16: the n x 16 slice of B lives in LDS (element (i, k) at 17 i + k, dead columns are zeros).  Per
// diagonal block, forward then backward: its triangle -> the LDS image, wave 0 lane k runs the column sweep of right-hand side k on registers
// (no lane talks to another one), then the off-diagonal update B2 -= R12^T Y1 / B1 -= R12 X2 runs on the MFMA with R read straight from
// memory (every element once) and Y from LDS.  An MFMA output column depends on its own input column only: a dead column never feeds a live one
// and a column's bits do not depend on which of the 16 places it takes.
#include "batched_blocked.h"   // the per-block bodies of the two kernels below: shared with potrf_vbatched.hip
#include "vbatch_plan.h"       // the family's host arithmetic: grid limit, dispatch, operand rule

namespace {

template <int NBLK>
__global__ __launch_bounds__(64 * bb_factor_waves(NBLK)) void potrf_batched_blocked_kernel(BbArgs g) {
  bb_factor_block<NBLK>(g.A + (int64_t)blockIdx.x * g.stride_a, g.lda, g.n, g.info, g.logdet, blockIdx.x);
}

__global__ __launch_bounds__(BB_THREADS) void potrs_batched_blocked_kernel(BbSolveArgs g) {
  bb_solve_block(g.R + (int64_t)blockIdx.x * g.stride_r, g.ldr, g.B + (int64_t)blockIdx.x * g.stride_b, g.ldb, g.nrhs, g.n, g.info, blockIdx.x);
}

}  // namespace

extern "C" {

int cap_dpotrf_batched_blocked(int uplo, int64_t n, double* A, int64_t lda, int64_t stride_a, int64_t batch, int* info, double* logdet,
                               void* stream) {
  if (n < 0 || batch < 0) return CAP_ERR_ARG;
  if (n > 0 && batch > 0 && !A) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, lda, stride_a, batch)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpotrf_batched
  if (n > BB_MAX) return CAP_ERR_UNSUPPORTED;
  if (n == 0 || batch == 0) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  if (n <= BB_SMALL) return cap_potrf_batched_launch(n, A, lda, stride_a, batch, info, logdet, s);
  if (vb_grid(batch, 1) < 0) return CAP_ERR_UNSUPPORTED;  // a workgroup per block
  BbArgs g;
  g.A = A; g.lda = lda; g.stride_a = stride_a; g.info = info; g.logdet = logdet; g.n = (int)n;
  if (cap_acc_on()) {
    cap_acc_rw(A, 0, (batch - 1) * stride_a + (n - 1) * lda + n, 1);
    if (info) cap_acc_w(info, 0, batch, 1, 0, 4);
    if (logdet) cap_acc_w(logdet, 0, batch, 1);
  }
  vb_with_int<2, 3, 4>((int)cap_ceil_div(n, BB_NB), [&](auto NBLK) {
    hipLaunchKernelGGL(potrf_batched_blocked_kernel<NBLK()>, dim3((unsigned)batch), dim3(64 * bb_factor_waves(NBLK())), 0, s, g);
  });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_dpotrs_batched_blocked(int uplo, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                               int64_t stride_b, int64_t batch, const int* info, void* stream) {
  if (n < 0 || batch < 0 || nrhs < 0) return CAP_ERR_ARG;
  if (n > 0 && batch > 0 && (!R || !B)) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, ldr, stride_r, batch) || !vb_operand_ok(n, nrhs, ldb, stride_b, batch)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (n > BB_MAX) return CAP_ERR_UNSUPPORTED;
  if (n == 0 || batch == 0 || nrhs == 0) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  if (n <= BB_SMALL) return cap_potrs_batched_launch(n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, s);
  if (vb_grid(batch, 1) < 0) return CAP_ERR_UNSUPPORTED;
  BbSolveArgs g;
  g.R = R; g.ldr = ldr; g.stride_r = stride_r; g.B = B; g.ldb = ldb; g.stride_b = stride_b; g.nrhs = nrhs; g.info = info; g.n = (int)n;
  if (cap_acc_on()) {
    cap_acc_r(R, 0, (batch - 1) * stride_r + (n - 1) * ldr + n, 1);
    cap_acc_rw(B, 0, (batch - 1) * stride_b + (nrhs - 1) * ldb + n, 1);
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
  }
  hipLaunchKernelGGL(potrs_batched_blocked_kernel, dim3((unsigned)batch), dim3(BB_THREADS), 0, s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

}  // extern "C"
