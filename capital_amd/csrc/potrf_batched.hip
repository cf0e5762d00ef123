// Batched Cholesky factor and solve for many small SPD blocks of one size (cap_dpotrf_batched, cap_dpotrs_batched): block i of the batch is
// the n x n column-major block at A + i stride_a, 1 <= n <= 64, A_i = R_i^T R_i with R_i upper, in place.
//
// ONE WAVEFRONT PER GROUP OF BLOCKS, nothing between wavefronts: a workgroup is a single wave of 64 lanes (its __syncthreads is the order of
// the wave's own LDS accesses, no wave ever waits for another one), the grid is 1-D, there are no atomics, no spin waits and no reads of another
// workgroup's data.  The kernels are templated on the padded size NP = 8 / 16 / 32 / 64 (the smallest one >= n); a wave carries G = 64 / NP
// blocks in lane groups of NP lanes, so that n = 8 fills the wave with eight blocks.
//
// Factor.  The upper triangle is read with consecutive lanes along a column (coalesced; the strictly lower triangle is never addressed) into
// an LDS image, lane c of a group then takes column c into registers a[0 .. NP) - every register index is a compile-time constant, the steps
// are fully unrolled, steps and row chunks at or beyond n are skipped by wave-uniform branches.  Step j:
//   d = a_jj, taken from lane j of the group by a lane shuffle;  r_jc = a_jc / sqrt(d) in lane c (r_jj = sqrt(d)), both correctly rounded;
//   row j of R goes to the LDS image;  a_ic -= r_ji r_jc for i > j with r_ji read back from that row (every lane of a group reads the same
//   address: an LDS broadcast).
// The image therefore ends up holding R and the store runs coalesced again.  The image holds the upper triangle only: row r and row
// NP - 1 - r share one line of NP + 2 doubles (PbImg::at), half the LDS of a square image - at NP = 64 that is what lets more than one wave
// live on a SIMD.  The first pivot that is not > 0 (NaN included) sets info and turns this row and every later one into NaN.
// Every block sees the same instruction sequence on its own data only: its bits depend on (n, its data) and on nothing else - there is one
// load path, whatever the alignment.
//
// Solve.  R's upper triangle goes to the same LDS image; lane k of a group owns right-hand side k0 + k of its block with the n entries in
// registers and runs R^T y = b, then R x = y, as column sweeps (divide, then n - j - 1 independent fused multiply-adds against LDS broadcasts
// of R) - no lane ever talks to another one, so a column's bits cannot depend on how many columns travel with it.  More than NP right-hand
// sides are further passes inside the launch.
#include <math.h>

#include <utility>

#include "common.h"
#include "batched_small.h"     // the image and the unrolled steps: shared with potrf_vbatched.hip
#include "vbatch_plan.h"       // the family's host arithmetic: padded size, grid limit, dispatch, operand rule

namespace {

template <int NP>
__global__ __launch_bounds__(64) void potrf_batched_kernel(PbArgs g) {
  constexpr int G = 64 / NP;
  using Img = PbImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  __shared__ double s_log[64];
  const int lane = threadIdx.x, grp = lane / NP, c = lane % NP, n = g.n;
  const int64_t blk = (int64_t)blockIdx.x * G + grp;
  const bool live = blk < g.batch;
  double* A = g.A + (live ? blk * g.stride_a : 0);
  double* s = s_img + grp * Img::SIZE;

  pb_load_upper<NP>(A, g.lda, n, c, live, s);
  __syncthreads();
  double a[NP];
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const double v = s[Img::at(i, c)];
    a[i] = (i <= c && c < n) ? v : 0.0;
  }
  __syncthreads();                       // the image is in registers: from here on it takes the rows of R

  int info = 0;
  bool bad = false;
  if constexpr (NP < 64) {
#pragma unroll
    for (int j = 0; j < NP; j++) pb_factor_step<NP>(a, s, c, n, j, info, bad);
  } else {
    pb_factor_steps<NP>(a, s, c, n, info, bad, std::make_integer_sequence<int, NP>{});
  }
  __syncthreads();

#pragma unroll 8
  for (int cc = 0; cc < n; cc++)
    if (live && c <= cc) A[c + (int64_t)cc * g.lda] = s[Img::at(c, cc)];
  if (g.info && live && c == 0) g.info[blk] = info;
  if (g.logdet) {                        // 2 sum_j log r_jj in ascending j: lane j takes the logarithm, lane 0 of the group adds them in order
    s_log[lane] = c < n ? log(s[Img::at(c, c)]) : 0.0;
    __syncthreads();
    if (live && c == 0) {
      double t = 0.0;
      for (int j = 0; j < n; j++) t += s_log[grp * NP + j];
      g.logdet[blk] = bad ? (double)NAN : 2.0 * t;
    }
  }
}

template <int NP>
__global__ __launch_bounds__(64) void potrs_batched_kernel(PbSolveArgs g) {
  constexpr int G = 64 / NP;
  using Img = PbImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  const int lane = threadIdx.x, grp = lane / NP, k = lane % NP, n = g.n;
  const int64_t blk = (int64_t)blockIdx.x * G + grp;
  const bool live = blk < g.batch;
  const double* s = s_img + grp * Img::SIZE;

  pb_load_upper<NP>(g.R + (live ? blk * g.stride_r : 0), g.ldr, n, k, live, s_img + grp * Img::SIZE);
  const bool bad = g.info && live && g.info[blk] != 0;
  __syncthreads();

  for (int64_t k0 = 0; k0 < g.nrhs; k0 += NP) {
    const bool on = live && k0 + k < g.nrhs;
    double* b = g.B + (on ? blk * g.stride_b + (k0 + k) * g.ldb : 0);
    double x[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
      x[i] = 0.0;
      if (i < n) { if (on) x[i] = b[i]; }
    }
    if constexpr (NP < 64) {
#pragma unroll
      for (int j = 0; j < NP; j++) pb_forward_step<NP>(x, s, n, j);
#pragma unroll
      for (int j = NP - 1; j >= 0; j--) pb_backward_step<NP>(x, s, n, j);
    } else {
      pb_solve_steps<NP>(x, s, n, std::make_integer_sequence<int, NP>{});
    }
#pragma unroll
    for (int i = 0; i < NP; i++) {
      if (i < n) { if (on) b[i] = bad ? (double)NAN : x[i]; }
    }
  }
}

}  // namespace

int cap_potrf_batched_launch(int64_t n, double* A, int64_t lda, int64_t stride_a, int64_t batch, int* info, double* logdet, hipStream_t s) {
  if (n <= 0 || batch <= 0) return CAP_OK;
  if (n > PB_MAX) return CAP_ERR_UNSUPPORTED;
  const int np = vb_padded(n);
  const int64_t nwg = vb_grid(batch, 64 / np);
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  PbArgs g;
  g.A = A; g.lda = lda; g.stride_a = stride_a; g.batch = batch; g.info = info; g.logdet = logdet; g.n = (int)n;
  if (cap_acc_on()) {
    cap_acc_rw(A, 0, (batch - 1) * stride_a + (n - 1) * lda + n, 1);
    if (info) cap_acc_w(info, 0, batch, 1, 0, 4);
    if (logdet) cap_acc_w(logdet, 0, batch, 1);
  }
  vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { hipLaunchKernelGGL(potrf_batched_kernel<NP()>, dim3((unsigned)nwg), dim3(64), 0, s, g); });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_potrs_batched_launch(int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb, int64_t stride_b,
                             int64_t batch, const int* info, hipStream_t s) {
  if (n <= 0 || batch <= 0 || nrhs <= 0) return CAP_OK;
  if (n > PB_MAX) return CAP_ERR_UNSUPPORTED;
  const int np = vb_padded(n);
  const int64_t nwg = vb_grid(batch, 64 / np);
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  PbSolveArgs g;
  g.R = R; g.ldr = ldr; g.stride_r = stride_r; g.B = B; g.ldb = ldb; g.stride_b = stride_b; g.batch = batch; g.nrhs = nrhs; g.info = info;
  g.n = (int)n;
  if (cap_acc_on()) {
    cap_acc_r(R, 0, (batch - 1) * stride_r + (n - 1) * ldr + n, 1);
    cap_acc_rw(B, 0, (batch - 1) * stride_b + (nrhs - 1) * ldb + n, 1);
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
  }
  vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { hipLaunchKernelGGL(potrs_batched_kernel<NP()>, dim3((unsigned)nwg), dim3(64), 0, s, g); });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

extern "C" {

int cap_dpotrf_batched(int uplo, int64_t n, double* A, int64_t lda, int64_t stride_a, int64_t batch, int* info, double* logdet, void* stream) {
  if (n < 0 || batch < 0) return CAP_ERR_ARG;
  if (n > 0 && batch > 0 && !A) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, lda, stride_a, batch)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpotrf
  if (n > PB_MAX) return CAP_ERR_UNSUPPORTED;
  return cap_potrf_batched_launch(n, A, lda, stride_a, batch, info, logdet, cap_stream(stream));
}

int cap_dpotrs_batched(int uplo, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                       int64_t stride_b, int64_t batch, const int* info, void* stream) {
  if (n < 0 || batch < 0 || nrhs < 0) return CAP_ERR_ARG;
  if (n > 0 && batch > 0 && (!R || !B)) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, ldr, stride_r, batch) || !vb_operand_ok(n, nrhs, ldb, stride_b, batch)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (n > PB_MAX) return CAP_ERR_UNSUPPORTED;
  return cap_potrs_batched_launch(n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, cap_stream(stream));
}

}  // extern "C"
