// Conditioning kernels of shifted CholeskyQR3 (Fukaya, Kannan, Nakatsukasa, Yamamoto, Yanagisawa, SIAM J. Sci. Comput. 42 (2020)): the
// elementwise work a shifted sweep of csrc/cacqr.hip does on the n x n Gram between the all-reduce and cap_rec_cholinv_full, and on the
// factor and its inverse behind it.  Everything heavy in a shifted sweep is the unshifted sweep's own code (gram256 / qrapply256 or the
// split-K TN GEMM + the streaming NN GEMM): these launches are latency sized (n^2 / 2 elements each, n a few hundred).
//
//   equilibrate:  d_j = sqrt(G_jj) (1 where G_jj is not a positive finite number: the failure then shows as info of a later sweep)
//                 G_ij <- G_ij / d_i / d_j for i < j,  G_ii <- 1 + s exactly,   s = 11 (m n + n (n + 1)) 2^-53 n
//                 (the paper's shift 11 (m n + n (n + 1)) u ||A||_2^2 with ||.||_2^2 bounded by the squared Frobenius norm, which is exactly n
//                 once the columns have unit norm: no norm reduction, and the value is a closed form of the shape - m the GLOBAL row count,
//                 read from device memory where the plan's communicator summed the ranks' m_local)
//   unscale:      R_k = R' D (column j times d_j),  R_k^-1 = D^-1 R'^-1 (row i divided by d_i)
//
// Step 1 is two launches: the thread that rewrites G_ii would race with the threads that read it as a scale, so the scales go to an n-vector
// of the plan first.  Only the upper triangle is touched: both Gram paths leave zeros below the diagonal, and so does the factorization.
#include <cmath>

#include "common.h"

namespace {

__device__ __forceinline__ double scqr_shift_of(double m_global, int n) {
  // integers and a power of two: exact below 2^53, whatever the order
  return 11.0 * (m_global * (double)n + (double)n * (double)(n + 1)) * 0x1p-53 * (double)n;
}

__global__ void scqr_rows_kernel(double* m_global, double m_local) { *m_global = m_local; }

__global__ void scqr_scales_kernel(const double* __restrict__ G, int64_t ldg, int n, const double* __restrict__ m_global,
                                   double* __restrict__ d, double* __restrict__ shift) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) *shift = scqr_shift_of(*m_global, n);
  if (j >= n) return;
  const double g = G[j + j * ldg];
  d[j] = (g > 0.0 && g < INFINITY) ? sqrt(g) : 1.0;                 // (NaN fails both comparisons)
}

__global__ void scqr_equilibrate_kernel(double* __restrict__ G, int64_t ldg, int n, const double* __restrict__ d,
                                        const double* __restrict__ shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i > j || j >= n) return;
  double* g = G + i + j * ldg;
  *g = (i == j) ? 1.0 + *shift : *g / d[i] / d[j];                   // two divisions: d_i d_j may leave the range where the quotient does not
}

__global__ void scqr_unscale_kernel(double* __restrict__ R, int64_t ldr, double* __restrict__ Ri, int64_t ldi, int n,
                                    const double* __restrict__ d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i > j || j >= n) return;
  R[i + j * ldr] *= d[j];
  Ri[i + j * ldi] /= d[i];
}

}  // namespace

// this rank's row count into the plan's device word (the caller sums it over the ranks)
int cap_scqr_set_rows(double* m_global, int64_t m_local, hipStream_t s) {
  cap_acc_w(m_global, 1, 1, 1);
  hipLaunchKernelGGL(scqr_rows_kernel, dim3(1), dim3(1), 0, s, m_global, (double)m_local);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_scqr_equilibrate(double* G, int64_t ldg, int64_t n, const double* m_global, double* d, double* shift, hipStream_t s) {
  if (n <= 0) return CAP_OK;
  if (n > 65535) return CAP_ERR_UNSUPPORTED;                          // one grid row per column
  const dim3 grid((unsigned)cap_ceil_div(n, 256), (unsigned)n), block(256);
  cap_acc_r(G, ldg, n, n, 1); cap_acc_r(m_global, 1, 1, 1); cap_acc_w(d, n, n, 1); cap_acc_w(shift, 1, 1, 1);
  hipLaunchKernelGGL(scqr_scales_kernel, dim3(grid.x), block, 0, s, (const double*)G, ldg, (int)n, m_global, d, shift);
  CAP_HIP(hipGetLastError());
  cap_acc_rw(G, ldg, n, n, 1); cap_acc_r(d, n, n, 1); cap_acc_r(shift, 1, 1, 1);
  hipLaunchKernelGGL(scqr_equilibrate_kernel, grid, block, 0, s, G, ldg, (int)n, (const double*)d, (const double*)shift);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_scqr_unscale(double* R, int64_t ldr, double* Ri, int64_t ldi, int64_t n, const double* d, hipStream_t s) {
  if (n <= 0) return CAP_OK;
  if (n > 65535) return CAP_ERR_UNSUPPORTED;
  cap_acc_rw(R, ldr, n, n, 1); cap_acc_rw(Ri, ldi, n, n, 1); cap_acc_r(d, n, n, 1);
  hipLaunchKernelGGL(scqr_unscale_kernel, dim3((unsigned)cap_ceil_div(n, 256), (unsigned)n), dim3(256), 0, s, R, ldr, Ri, ldi, (int)n, d);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}
