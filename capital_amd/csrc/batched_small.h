// The device side that potrf_batched.hip and potrf_vbatched.hip share: the packed LDS image of an upper triangle and the fully unrolled
// steps of the in-register factorization and of the two substitutions for blocks of up to 64 rows (one lane group of NP lanes per block).
// The algorithm and its layout are described at the head of potrf_batched.hip.
#pragma once
#include <math.h>

#include <utility>

#include "common.h"

namespace {

constexpr int PB_MAX = 64;            // largest block
constexpr int PB_CH = 8;              // rows per wave-uniform "is this chunk below n" branch

// the packed image of an upper triangle: element (r, c), r <= c < NP; rows r < NP / 2 start their line, row NP - 1 - r fills its rest
template <int NP>
struct PbImg {
  static constexpr int LD = NP + 2;
  static constexpr int SIZE = (NP / 2) * LD;
  static __device__ __forceinline__ constexpr int at(int r, int c) { return r < NP / 2 ? r * LD + (c - r) : (NP - 1 - r) * LD + c + 1; }
};

struct PbArgs {
  double* A; int64_t lda, stride_a, batch;
  int* info; double* logdet;
  int n;
};

struct PbSolveArgs {
  const double* R; int64_t ldr, stride_r;
  double* B; int64_t ldb, stride_b, batch, nrhs;
  const int* info;
  int n;
};

// upper triangle of the n x n block at M (leading dimension ld) -> image; lane r of the group walks along row r, so a column is contiguous
template <int NP>
__device__ __forceinline__ void pb_load_upper(const double* M, int64_t ld, int n, int r, bool live, double* s) {
#pragma unroll 8
  for (int c = 0; c < n; c++)
    if (live && r <= c) s[PbImg<NP>::at(r, c)] = M[r + (int64_t)c * ld];
}

// Step J of the factorization (J is a compile-time constant at every call once the callers are expanded: every index of a[] is static)
template <int NP>
__device__ __forceinline__ void pb_factor_step(double (&a)[NP], double* s, int c, int n, const int J, int& info, bool& bad) {
  using Img = PbImg<NP>;
  if (J >= n) return;
  const double d = __shfl(a[J], J, NP);
  const bool ok = d > 0.0;               // false for a NaN too
  if (!ok && !bad) info = J + 1;
  bad = bad || !ok;
  const double sq = __dsqrt_rn(d);
  double r = c == J ? sq : a[J] / sq;
  r = bad ? (double)NAN : r;
  if (c >= J) s[Img::at(J, c)] = r;
  __syncthreads();
#pragma unroll
  for (int i0 = ((J + 1) / PB_CH) * PB_CH; i0 < NP; i0 += PB_CH) {
    if (i0 < n) {
#pragma unroll
      for (int i = (i0 > J + 1 ? i0 : J + 1); i < i0 + PB_CH; i++) a[i] = fma(-s[Img::at(J, i)], r, a[i]);
    }
  }
}
// NP = 64: the 64 steps as a parameter pack - the unroller's size limit would leave them a loop, with the column in scratch.  (The smaller
// sizes keep the unrolled loop: the compiler's register coalescer crashed on the pack form of NP = 16.)
template <int NP, int... J>
__device__ __forceinline__ void pb_factor_steps(double (&a)[NP], double* s, int c, int n, int& info, bool& bad, std::integer_sequence<int, J...>) {
  (pb_factor_step<NP>(a, s, c, n, J, info, bad), ...);
}

// R^T y = b, step J: y_j = b_j / r_jj, then b_i -= r_ji y_j for i > j (row j of R: contiguous in the image)
template <int NP>
__device__ __forceinline__ void pb_forward_step(double (&x)[NP], const double* s, int n, const int J) {
  using Img = PbImg<NP>;
  if (J >= n) return;
  x[J] = x[J] / s[Img::at(J, J)];
#pragma unroll
  for (int i0 = ((J + 1) / PB_CH) * PB_CH; i0 < NP; i0 += PB_CH) {
    if (i0 < n) {
#pragma unroll
      for (int i = (i0 > J + 1 ? i0 : J + 1); i < i0 + PB_CH; i++) x[i] = fma(-s[Img::at(J, i)], x[J], x[i]);
    }
  }
}

// R x = y, step J (taken in descending order): x_j = y_j / r_jj, then y_i -= r_ij x_j for i < j (column j of R)
template <int NP>
__device__ __forceinline__ void pb_backward_step(double (&x)[NP], const double* s, int n, const int J) {
  using Img = PbImg<NP>;
  if (J >= n) return;
  x[J] = x[J] / s[Img::at(J, J)];
#pragma unroll
  for (int i = 0; i < J; i++) x[i] = fma(-s[Img::at(i, J)], x[J], x[i]);
}
template <int NP, int... J>
__device__ __forceinline__ void pb_solve_steps(double (&x)[NP], const double* s, int n, std::integer_sequence<int, J...>) {
  (pb_forward_step<NP>(x, s, n, J), ...);
  (pb_backward_step<NP>(x, s, n, NP - 1 - J), ...);
}

}  // namespace
