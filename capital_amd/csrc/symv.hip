// Symmetric matrix times a thin block, the upper triangle read once (cap_dsymm_thin), and the 1-norm of a symmetric matrix on top of it
// (cap_dlansy): Y = beta opB(B) + alpha op(A) opX(X) with A n x n symmetric, X / B / Y n x nrhs, op = |.| of every element when `absolute`.
//
// Two plain launches per chunk of at most 16 right-hand sides, nothing between workgroups inside a launch:
//   part    one workgroup per S x S super-block (I, J), I <= J, of the upper block triangle (S = 512).  It streams the super-block in
//           64 x 64 tiles through LDS (leading dimension 65: the row walk and the column walk both hit distinct banks) and uses every
//           element twice: the row part P = A_IJ X_J (S x nrhs) and the column part Q = A_IJ^T X_I (S x nrhs; in the diagonal super-block
//           only the strictly upper elements, so the diagonal counts once).  The next tile is in flight in registers while the current one
//           is multiplied.  Waves 0 / 1 sum the two halves of a tile's columns for P (registers, carried along a tile row), waves 2 / 3
//           the two halves of its rows for Q (added into an LDS copy of Q per tile).  P and Q go to the super-block's own slot of `work`.
//   reduce  one thread per element of Y: the column parts Q(0, K) .. Q(K, K), then the row parts P(K, K) .. P(K, nsb - 1) of its
//           block row K are added in that order, then alpha, beta and B.  For the norm the launch keeps max |.| per workgroup instead
//           (a NaN stays a NaN) and a third, one-workgroup launch folds those.
// No floating-point atomics and no order that depends on timing: two calls give the same bits.  Masked elements (the strictly lower
// triangle inside diagonal tiles, rows and columns >= n) are never loaded - their addresses are clamped into the upper triangle and the
// value replaced by 0 - so NaN there cannot reach Y.  The arithmetic is fp64 VALU FMAs: 2 nrhs flops per 8 bytes of A.
#include <algorithm>

#include "common.h"

namespace {

constexpr int SV_S = 512;             // super-block edge
constexpr int SV_T = 64;              // tile edge
constexpr int SV_LD = SV_T + 1;       // LDS leading dimension of the tile
constexpr int SV_THREADS = 256;
constexpr int SV_NR_MAX = 16;
constexpr int SV_TPS = SV_S / SV_T;   // tiles per super-block edge

struct SvArgs {
  const double* A; int64_t lda;
  const double* X; int64_t ldx;       // NULL: every entry is 1 (the norm)
  double* part;                       // slot (I, J) at (J (J + 1) / 2 + I) * 2 S NR: P then Q, element (row, r) at row + r S
  int n, nrhs, absolute;
};

template <int NR>
constexpr size_t sv_lds_bytes() { return sizeof(double) * (size_t)(SV_T * SV_LD + 2 * SV_T * NR + SV_S * NR + 2 * SV_T * NR); }

template <int NR>
__global__ void __launch_bounds__(SV_THREADS) symm_thin_part_kernel(const SvArgs a) {
  // item k of the upper block triangle, column by column: k = J (J + 1) / 2 + I, 0 <= I <= J (the root is corrected for its rounding)
  const int k = blockIdx.x;
  int J = (int)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
  while ((int64_t)J * (J + 1) / 2 > k) J--;
  while ((int64_t)(J + 1) * (J + 2) / 2 <= k) J++;
  const int I = k - (int)((int64_t)J * (J + 1) / 2);
  extern __shared__ __attribute__((aligned(16))) double sv_lds[];
  double* Mt = sv_lds;                      // tile, element (row, col) at col SV_LD + row
  double* XI = Mt + SV_T * SV_LD;           // rows of X that meet the tile's rows / columns: (s, r) at s NR + r
  double* XJ = XI + SV_T * NR;
  double* Qs = XJ + SV_T * NR;              // the column part: (row, r) at r S + row (lanes along rows: no bank conflicts)
  double* cP = Qs + SV_S * NR;              // second halves of the sums
  double* cQ = cP + SV_T * NR;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n = a.n, r0 = I * SV_S, c0 = J * SV_S;
  const bool dsb = I == J;
  const int nti = min(SV_TPS, (n - r0 + SV_T - 1) / SV_T), ntj = min(SV_TPS, (n - c0 + SV_T - 1) / SV_T);
  double* P = a.part + ((int64_t)J * (J + 1) / 2 + I) * (2 * SV_S * NR);
  double* Q = P + SV_S * NR;

  for (int e = t; e < SV_S * NR; e += SV_THREADS) Qs[e] = 0.0;

  // a tile into registers: thread (lane, wv) takes row `lane` of the columns wv, wv + 4, ... (512 contiguous bytes per wave load)
  double v[SV_T / 4];
  auto load = [&](int ti, int tj) {
    const bool dt = dsb && ti == tj;
    const int grow = r0 + ti * SV_T + lane;
#pragma unroll
    for (int q = 0; q < SV_T / 4; q++) {
      const int gcol = c0 + tj * SV_T + wv + 4 * q;
      const int gc = min(gcol, n - 1);
      int gr = min(grow, n - 1);
      if (dt) gr = min(gr, gc);                                      // the address stays in the upper triangle
      const double x = a.A[gr + (int64_t)gc * a.lda];
      const bool on = grow < n && gcol < n && (!dt || grow <= gcol);
      v[q] = on ? (a.absolute ? fabs(x) : x) : 0.0;
    }
  };

  int ti = 0, tj = 0;
  load(ti, tj);
  double pacc[NR];
  while (ti < nti) {
    const int tj0 = dsb ? ti : 0;
    const bool first = tj == tj0, last = tj == ntj - 1, dt = dsb && ti == tj;
#pragma unroll
    for (int q = 0; q < SV_T / 4; q++) Mt[(wv + 4 * q) * SV_LD + lane] = v[q];
    for (int e = t; e < SV_T * NR; e += SV_THREADS) {
      const int s = e & (SV_T - 1), r = e >> 6;
      const bool rok = r < a.nrhs;
      const int gj = c0 + tj * SV_T + s;
      double xj = 0.0;
      if (rok && gj < n) { xj = a.X ? a.X[gj + (int64_t)r * a.ldx] : 1.0; if (a.absolute) xj = fabs(xj); }
      XJ[s * NR + r] = xj;
      if (first) {
        const int gi = r0 + ti * SV_T + s;
        double xi = 0.0;
        if (rok && gi < n) { xi = a.X ? a.X[gi + (int64_t)r * a.ldx] : 1.0; if (a.absolute) xi = fabs(xi); }
        XI[s * NR + r] = xi;
      }
    }
    __syncthreads();
    // the next tile is requested before this one is multiplied
    int nti_ = ti, ntj_ = tj + 1;
    if (ntj_ >= ntj) { nti_ = ti + 1; ntj_ = dsb ? nti_ : 0; }
    if (nti_ < nti) load(nti_, ntj_);

    double acc[NR];
    if (wv < 2) {
      if (first) {
#pragma unroll
        for (int r = 0; r < NR; r++) pacc[r] = 0.0;
      }
      for (int ss = 0; ss < SV_T / 2; ss++) {
        const int s = wv * (SV_T / 2) + ss;
        const double m = Mt[s * SV_LD + lane];
#pragma unroll
        for (int r = 0; r < NR; r++) pacc[r] = fma(m, XJ[s * NR + r], pacc[r]);
      }
      if (wv == 1 && last) {
#pragma unroll
        for (int r = 0; r < NR; r++) cP[r * SV_T + lane] = pacc[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < NR; r++) acc[r] = 0.0;
      for (int ss = 0; ss < SV_T / 2; ss++) {
        const int s = (wv - 2) * (SV_T / 2) + ss;
        double m = Mt[lane * SV_LD + s];
        if (dt && s >= lane) m = 0.0;                                // the diagonal belongs to the row part
#pragma unroll
        for (int r = 0; r < NR; r++) acc[r] = fma(m, XI[s * NR + r], acc[r]);
      }
      if (wv == 3) {
#pragma unroll
        for (int r = 0; r < NR; r++) cQ[r * SV_T + lane] = acc[r];
      }
    }
    __syncthreads();
    if (wv == 0 && last) {
#pragma unroll
      for (int r = 0; r < NR; r++) P[ti * SV_T + lane + r * SV_S] = pacc[r] + cP[r * SV_T + lane];
    }
    if (wv == 2) {
#pragma unroll
      for (int r = 0; r < NR; r++) Qs[r * SV_S + tj * SV_T + lane] += acc[r] + cQ[r * SV_T + lane];
    }
    ti = nti_; tj = ntj_;
  }
  __syncthreads();
  for (int e = t; e < SV_S * NR; e += SV_THREADS) {
    Q[e] = Qs[e];
  }
}

struct SvRed {
  const double* part; int nr;         // nr: the NR the parts were written with
  const double* B; int64_t ldb;
  double* Y; int64_t ldy;
  double* wmax;                       // != NULL: no Y; max |.| of this workgroup's rows of column 0 goes to wmax[blockIdx.x]
  double alpha, beta;
  int n, nrhs, nsb, absolute;
};

// the larger of two values, a NaN wins
__device__ __forceinline__ double sv_nanmax(double a, double b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

__device__ __forceinline__ double sv_block_max(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = SV_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = sv_nanmax(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(SV_THREADS) symm_thin_reduce_kernel(const SvRed a) {
  __shared__ double sh[SV_THREADS];
  const int row = blockIdx.x * SV_THREADS + threadIdx.x, r = blockIdx.y;
  double res = 0.0;
  if (row < a.n) {
    if (a.alpha != 0.0) {
      const int K = row / SV_S, o = row % SV_S;
      const int64_t slot = 2 * (int64_t)SV_S * a.nr, off = o + (int64_t)r * SV_S;
      double v = 0.0;
      for (int I = 0; I <= K; I++) v += a.part[((int64_t)K * (K + 1) / 2 + I) * slot + (int64_t)SV_S * a.nr + off];
      for (int J = K; J < a.nsb; J++) v += a.part[((int64_t)J * (J + 1) / 2 + K) * slot + off];
      res = a.alpha * v;
    }
    if (a.beta != 0.0) {
      const double b = a.B[row + (int64_t)r * a.ldb];
      res += a.beta * (a.absolute ? fabs(b) : b);
    }
    if (!a.wmax) a.Y[row + (int64_t)r * a.ldy] = res;
  }
  if (a.wmax) {
    const double m = sv_block_max(row < a.n ? fabs(res) : 0.0, sh);
    if (threadIdx.x == 0) a.wmax[blockIdx.x] = m;
  }
}

__global__ void __launch_bounds__(SV_THREADS) symm_max_kernel(const double* wmax, int count, double* out) {
  __shared__ double sh[SV_THREADS];
  double m = 0.0;
  for (int i = threadIdx.x; i < count; i += SV_THREADS) m = sv_nanmax(m, wmax[i]);
  m = sv_block_max(m, sh);
  if (threadIdx.x == 0) *out = m;
}

int sv_nr(int64_t nrhs) { return nrhs <= 1 ? 1 : nrhs <= 2 ? 2 : nrhs <= 4 ? 4 : nrhs <= 8 ? 8 : 16; }

template <int NR>
int launch_part(const SvArgs& g, int nsb, hipStream_t s) {
  // the dynamic LDS limit is a property of the loaded kernel: set once per device and instantiation
  static bool attr_set[16] = {};
  int dev = 0;
  CAP_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 16 || !attr_set[dev]) {
    CAP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(symm_thin_part_kernel<NR>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sv_lds_bytes<NR>()));
    if (dev >= 0 && dev < 16) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(symm_thin_part_kernel<NR>, dim3((unsigned)((int64_t)nsb * (nsb + 1) / 2)), dim3(SV_THREADS), sv_lds_bytes<NR>(), s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int64_t sv_part_elems(int64_t n, int64_t nrhs) {
  const int64_t nsb = cap_ceil_div(n, SV_S);
  return nsb * (nsb + 1) / 2 * 2 * SV_S * sv_nr(std::min<int64_t>(nrhs, SV_NR_MAX));
}

// one chunk (nrhs <= 16); X == NULL: ones; wmax != NULL: the norm's epilogue instead of Y
int sv_chunk(int absolute, int64_t n, int64_t nrhs, double alpha, const double* A, int64_t lda, const double* X, int64_t ldx, double beta,
             const double* B, int64_t ldb, double* Y, int64_t ldy, double* work, double* wmax, hipStream_t s) {
  const int nsb = (int)cap_ceil_div(n, SV_S), nr = sv_nr(nrhs);
  if (alpha != 0.0) {
    SvArgs g{A, lda, X, ldx, work, (int)n, (int)nrhs, absolute};
    if (cap_acc_on()) {
      cap_acc_r(A, lda, n, n, 1);
      if (X) cap_acc_r(X, ldx, n, nrhs);
      cap_acc_w(work, 0, sv_part_elems(n, nrhs), 1);
    }
    if (nr == 1) CAP_TRY(launch_part<1>(g, nsb, s));
    else if (nr == 2) CAP_TRY(launch_part<2>(g, nsb, s));
    else if (nr == 4) CAP_TRY(launch_part<4>(g, nsb, s));
    else if (nr == 8) CAP_TRY(launch_part<8>(g, nsb, s));
    else CAP_TRY(launch_part<16>(g, nsb, s));
  }
  SvRed q{work, nr, B, ldb, Y, ldy, wmax, alpha, beta, (int)n, (int)nrhs, nsb, absolute};
  const int wgs = (int)cap_ceil_div(n, SV_THREADS);
  if (cap_acc_on()) {
    if (alpha != 0.0) cap_acc_r(work, 0, sv_part_elems(n, nrhs), 1);
    if (beta != 0.0) cap_acc_r(B, ldb, n, nrhs);
    if (wmax) cap_acc_w(wmax, 0, wgs, 1); else cap_acc_w(Y, ldy, n, nrhs);
  }
  hipLaunchKernelGGL(symm_thin_reduce_kernel, dim3((unsigned)wgs, (unsigned)nrhs), dim3(SV_THREADS), 0, s, q);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

bool sv_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  if (!a || !b || abytes <= 0 || bbytes <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

int64_t sv_span(int64_t ld, int64_t rows, int64_t cols) { return (rows <= 0 || cols <= 0) ? 0 : 8 * (ld * (cols - 1) + rows); }

}  // namespace

int64_t cap_dsymm_thin_work_size(int64_t n, int64_t nrhs) {
  if (n <= 0 || nrhs <= 0) return 0;
  return sv_part_elems(n, nrhs);
}

int cap_dsymm_thin(int uplo, int absolute, int64_t n, int64_t nrhs, double alpha, const double* A, int64_t lda, const double* X, int64_t ldx,
                   double beta, const double* B, int64_t ldb, double* Y, int64_t ldy, double* work, void* stream) {
  if (n < 0 || nrhs < 0 || absolute < 0 || absolute > 1 || alpha != alpha || beta != beta) return CAP_ERR_ARG;
  if (n > 0 && nrhs > 0) {
    if (!Y || ldy < n) return CAP_ERR_ARG;
    if (alpha != 0.0 && (!A || !X || !work || lda < n || ldx < n)) return CAP_ERR_ARG;
    if (beta != 0.0 && (!B || ldb < n)) return CAP_ERR_ARG;
    const int64_t ys = sv_span(ldy, n, nrhs);
    if (alpha != 0.0 && (sv_overlap(Y, ys, A, sv_span(lda, n, n)) || sv_overlap(Y, ys, X, sv_span(ldx, n, nrhs)) ||
                         sv_overlap(Y, ys, work, 8 * cap_dsymm_thin_work_size(n, nrhs))))
      return CAP_ERR_ARG;
  }
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpstrf
  if (n == 0 || nrhs == 0) return CAP_OK;
  if (n > ((int64_t)1 << 24)) return CAP_ERR_ARG;        // item and row indices are ints
  hipStream_t s = cap_stream(stream);
  for (int64_t c = 0; c < nrhs; c += SV_NR_MAX) {
    const int64_t nc = std::min<int64_t>(SV_NR_MAX, nrhs - c);
    CAP_TRY(sv_chunk(absolute, n, nc, alpha, A, lda, alpha != 0.0 ? X + c * ldx : nullptr, ldx, beta, beta != 0.0 ? B + c * ldb : nullptr, ldb,
                     Y + c * ldy, ldy, work, nullptr, s));
  }
  return CAP_OK;
}

// [parts of one column][one maximum per workgroup of the reduce launch]
int64_t cap_dlansy_work_size(int64_t n) {
  if (n <= 0) return 0;
  return sv_part_elems(n, 1) + cap_ceil_div(n, SV_THREADS);
}

int cap_dlansy(int norm, int uplo, int64_t n, const double* A, int64_t lda, double* out_dev, double* work, void* stream) {
  if (n < 0 || !out_dev || (n > 0 && (!A || !work || lda < n))) return CAP_ERR_ARG;
  if (norm != '1' && norm != 'O' && norm != 'o' && norm != 'I' && norm != 'i') return CAP_ERR_UNSUPPORTED;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  hipStream_t s = cap_stream(stream);
  if (n == 0) return cap_set_double(out_dev, 0.0, s);
  if (n > ((int64_t)1 << 24)) return CAP_ERR_ARG;        // as cap_dsymm_thin
  double* wmax = work + sv_part_elems(n, 1);
  // |A| times a column of ones that the kernel supplies itself, then the largest entry
  CAP_TRY(sv_chunk(1, n, 1, 1.0, A, lda, nullptr, 0, 0.0, nullptr, 0, nullptr, 0, work, wmax, s));
  const int wgs = (int)cap_ceil_div(n, SV_THREADS);
  if (cap_acc_on()) { cap_acc_r(wmax, 0, wgs, 1); cap_acc_w(out_dev, 0, 1, 1); }
  hipLaunchKernelGGL(symm_max_kernel, dim3(1), dim3(SV_THREADS), 0, s, wmax, wgs, out_dev);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}
