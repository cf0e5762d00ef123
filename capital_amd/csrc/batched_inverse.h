// The device side that potri_batched.hip and potrf_vbatched.hip share: the sweep and product steps of the inverse of a block of up to 64 rows
// in one lane group, and the inverse of ONE block of 65 .. 256 rows by one workgroup as a function of the block's address, leading dimension
// and size.  The algorithms are described at the head of potri_batched.hip.
#pragma once
#include <math.h>

#include <utility>

#include "common.h"

namespace {

constexpr int PI_MAX = 256;           // largest block
constexpr int PI_SMALL = 64;          // up to here: a wavefront per 64 / NP blocks
constexpr int PI_NB = 64;             // rows of a diagonal block
constexpr int PI_CH = 8;              // rows per wave-uniform "is this chunk below n" branch
constexpr int PI_SW = 16;             // rows of a sweep step between two scheduling barriers

// the packed image of an upper triangle (PbImg of potrf_batched.hip): element (r, c), r <= c < NP
template <int NP>
struct PiImg {
  static constexpr int LD = NP + 2;
  static constexpr int SIZE = (NP / 2) * LD;
  static __device__ __forceinline__ constexpr int at(int r, int c) { return r < NP / 2 ? r * LD + (c - r) : (NP - 1 - r) * LD + c + 1; }
};

struct PiArgs {
  double* A; int64_t ld, stride, batch;
  const int* info;
  int n, fill;
};

// R w = e_c, step J (taken in descending order) in the lanes c >= J: w_j /= r_jj, then w_i -= r_ij w_j for i < j (column j of R)
template <int NP, int J>
__device__ __forceinline__ void pi_sweep_step(double (&x)[NP], const double* s, int c, int n) {
  using Img = PiImg<NP>;
  if (J >= n) return;
  if (c >= J) {
    x[J] = x[J] / s[Img::at(J, J)];
#pragma unroll
    for (int i0 = 0; i0 < J; i0 += PI_SW) {
#pragma unroll
      for (int i = i0; i < (i0 + PI_SW < J ? i0 + PI_SW : J); i++) x[i] = fma(-s[Img::at(i, J)], x[J], x[i]);
      __builtin_amdgcn_sched_barrier(0);       // a chunk's LDS reads stay with its multiply-adds: a step never holds a whole column of R beside x
    }
  }
}
template <int NP, int... J>
__device__ __forceinline__ void pi_sweep_steps(double (&x)[NP], const double* s, int c, int n, std::integer_sequence<int, J...>) {
  (pi_sweep_step<NP, NP - 1 - J>(x, s, c, n), ...);
}

// column c of the inverse of the n x n triangle in the image -> x (zeros below row c, and everywhere in the lanes c >= n)
template <int NP>
__device__ __forceinline__ void pi_invert(double (&x)[NP], const double* s, int c, int n) {
#pragma unroll
  for (int i = 0; i < NP; i++) x[i] = i == c ? 1.0 : 0.0;
  pi_sweep_steps<NP>(x, s, c, n, std::make_integer_sequence<int, NP>{});
}

// x -> column c of the image, every column of it: zeros at and beyond n, so that the image holds no stale word afterwards
template <int NP>
__device__ __forceinline__ void pi_put_column(const double (&x)[NP], double* s, int c, int n) {
#pragma unroll
  for (int i = 0; i < NP; i++)
    if (i <= c) s[PiImg<NP>::at(i, c)] = c < n ? x[i] : 0.0;
}

// row I of C = W W^T: c_Ij = sum_{k >= j} w_Ik w_jk in lane j (w: row j of W, zeros in front of column j), ascending k; then row I of the
// image, which no lane needs any more, takes it
template <int NP>
__device__ __forceinline__ void pi_product_row(const double (&w)[NP], double* s, int j, int n, const int I) {
  using Img = PiImg<NP>;
  if (I >= n) return;
  double acc = 0.0;
#pragma unroll
  for (int k0 = (I / PI_CH) * PI_CH; k0 < NP; k0 += PI_CH) {
    if (k0 < n) {
#pragma unroll
      for (int k = (k0 > I ? k0 : I); k < k0 + PI_CH; k++) acc = fma(s[Img::at(I, k)], w[k], acc);
    }
  }
  __syncthreads();                       // (one wave: orders the reads of row I in front of its stores)
  if (j >= I) s[Img::at(I, j)] = acc;
}
template <int NP, int... I>
__device__ __forceinline__ void pi_product_rows(const double (&w)[NP], double* s, int j, int n, std::integer_sequence<int, I...>) {
  (pi_product_row<NP>(w, s, j, n, I), ...);
}

using BImg = PiImg<PI_NB>;

struct PiBlkArgs {
  double* A; int64_t ld, stride;
  const int* info;
  int n, potri, fill;
};

// orders one wave's LDS stores before its later LDS loads of other lanes' data (a wave's LDS instructions execute in order)
__device__ __forceinline__ void pi_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// An opaque zero (as in potrf_batched_blocked.hip): added to an LDS pointer it keeps the uniform LDS addresses of the unrolled steps "one
// VGPR + immediate offset" instead of one SGPR constant each.
__device__ __forceinline__ int pi_opaque_zero() { int z = 0; asm volatile("" : "+v"(z)); return z; }

// waves of the workgroup: four where the LDS lets two workgroups share a CU (NBLK = 2), eight where it holds one
constexpr int pi_waves(int nblk) { return nblk == 2 ? 4 : 8; }

// the triangular inverse (potri = 0) or the SPD inverse (potri = 1) of ONE block by the whole workgroup; info (may be null): a block with info[slot] != 0 gets NaN
template <int NBLK>
__device__ __forceinline__ void pi_blocked_block(double* A, const int64_t ld, const int n, const int* info, const int64_t slot, const int potri, const int fill) {
  constexpr int NW = pi_waves(NBLK);
  constexpr int PW = PI_NB * (NBLK - 1);      // rows of the tallest column panel = columns of the widest row panel
  constexpr int LDC = PI_NB + 1;              // column panel: element (r, c), r < PW, c < 64, at r LDC + c
  constexpr int LDP = PW + 1;                 // row panel: element (j, c), j < 64, c < PW, at j LDP + c
  __shared__ double s_img[BImg::SIZE];
  __shared__ double s_pan[PW * LDC];          // (>= 64 LDP)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, kg = lane >> 4;
  const int nd = (n + PI_NB - 1) / PI_NB;

  if (info && info[slot] != 0) {     // a failed block: NaN wherever the call writes (uniform over the workgroup)
    for (int c = wave; c < n; c += NW)
      for (int r = lane; r < n; r += 64)
        if (r <= c || fill) A[r + (int64_t)c * ld] = (double)NAN;
    return;
  }

  // ---- the triangular inverse, block column by block column
  for (int J = 0; J < nd; J++) {
    const int k0 = J * PI_NB, nb = n - k0 < PI_NB ? n - k0 : PI_NB, nct = (nb + 15) >> 4;
    double* D = A + k0 + (int64_t)k0 * ld;
    double* P = A + (int64_t)k0 * ld;

    for (int c = wave; c < nb; c += NW)
      if (lane <= c) s_img[BImg::at(lane, c)] = D[lane + (int64_t)c * ld];
    for (int c = wave; c < nct * 16; c += NW)
      for (int r = lane; r < k0; r += 64) s_pan[r * LDC + c] = c < nb ? P[r + (int64_t)c * ld] : 0.0;
    __syncthreads();

    if (wave == 0) {
      double x[PI_NB];
      const int c = lane + pi_opaque_zero();   // (opaque: the unit vectors are built here, not kept in registers across the steps)
      pi_invert<PI_NB>(x, s_img + pi_opaque_zero(), c, nb);
      pi_wave_sync();                          // every lane is through with R22: the image takes W22
      pi_put_column<PI_NB>(x, s_img, c, nb);
    }
    __syncthreads();

    for (int c = wave; c < nb; c += NW)
      if (lane <= c) D[lane + (int64_t)c * ld] = s_img[BImg::at(lane, c)];

    if (k0 > 0) {
      // Y = R12 W22 in place; MFMA A operand: lane -> R12[i0 + lr][kk + kg], B operand: W22[kk + kg][c0 + lr] (zero below the diagonal);
      // D: row i0 + kg + 4 r, column c0 + lr
      for (int st = wave; st < k0 / 16; st += NW) {
        const int i0 = st * 16;
        for (int ct = nct - 1; ct >= 0; ct--) {
          const int c0 = ct * 16, col = c0 + lr;
          const double* pa = s_pan + (i0 + lr) * LDC + kg;
          d4 acc = {0.0, 0.0, 0.0, 0.0};
          for (int kk = 0; kk < c0 + 16; kk += 4) {
            const int k = kk + kg;
            const double v = s_img[BImg::at(k < col ? k : col, col)];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], k <= col ? v : 0.0, acc, 0, 0, 0);
          }
          pi_wave_sync();                      // the strip's reads of these columns are done
#pragma unroll
          for (int r = 0; r < 4; r++) s_pan[(i0 + kg + 4 * r) * LDC + col] = acc[r];
          pi_wave_sync();
        }
      }
      __syncthreads();
      // W12 = -W11 Y; A operand: lane -> -W11[i0 + lr][kk + kg] from memory (zero below the diagonal, never loaded), B operand: Y[kk + kg][c0 + lr]
      const int ntile = (k0 / 16) * nct;
      for (int t = wave; t < ntile; t += NW) {
        const int i0 = (t / nct) * 16, c0 = (t % nct) * 16, row = i0 + lr, col = c0 + lr;
        const double* pa = A + row + (int64_t)kg * ld;
        const double* pb = s_pan + kg * LDC + col;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int kk = i0; kk < k0; kk += 4) {
          double a = 0.0;
          if (row <= kk + kg) a = -pa[(int64_t)kk * ld];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pb[kk * LDC], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (col < nb) P[(i0 + kg + 4 * r) + (int64_t)col * ld] = acc[r];
      }
    }
    __syncthreads();                           // the next step reads what other waves stored, and reuses the LDS
  }

  if (!potri) return;

  // ---- the triangular product W W^T, block row by block row
  for (int I = 0; I < nd; I++) {
    const int k0 = I * PI_NB, nb = n - k0 < PI_NB ? n - k0 : PI_NB, nct = (nb + 15) >> 4, nb4 = (nb + 3) & ~3;
    const int t0 = k0 + PI_NB, m = n > t0 ? n - t0 : 0, m4 = (m + 3) & ~3;
    const double* D = A + k0 + (int64_t)k0 * ld;

    for (int c = wave; c < nb; c += NW)
      if (lane <= c) s_img[BImg::at(lane, c)] = D[lane + (int64_t)c * ld];
    for (int c = wave; c < m4; c += NW) s_pan[lane * LDP + c] = c < m ? A[(k0 + lane) + (int64_t)(t0 + c) * ld] : 0.0;   // (m > 0: nb == 64)
    __syncthreads();

    const int nst = k0 / 16 + nct;
    for (int st = wave; st < nst; st += NW) {
      const int i0 = st * 16, row = i0 + lr;
      for (int ct = 0; ct < nct; ct++) {
        const int c0 = ct * 16, cl = c0 + lr, col = k0 + cl;
        if (i0 > k0 + c0 + 15) continue;       // wholly below the diagonal
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        // W[., I] W_II^T; A operand: lane -> W[i0 + lr][k0 + kk + kg], B operand: W_II[c0 + lr][kk + kg] (zero in front of the diagonal)
        const double* pa = A + row + (int64_t)(k0 + kg) * ld;
        for (int kk = c0; kk < nb4; kk += 4) {
          const int k = kk + kg;
          double a = 0.0;
          if (row <= k0 + k && k < nb) a = pa[(int64_t)kk * ld];
          const int kc = k < PI_NB - 1 ? k : PI_NB - 1;
          const double v = s_img[BImg::at(cl < kc ? cl : kc, kc)];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (cl <= k && k < nb) ? v : 0.0, acc, 0, 0, 0);
        }
        // W[., I + 1 ..] W[I, I + 1 ..]^T; A operand from memory, B operand: the row panel [c0 + lr][kk + kg]
        const double* qa = A + row + (int64_t)(t0 + kg) * ld;
        const double* qb = s_pan + cl * LDP + kg;
        for (int kk = 0; kk < m4; kk += 4) {
          double a = 0.0;
          if (kk + kg < m) a = qa[(int64_t)kk * ld];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, qb[kk], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int orow = i0 + kg + 4 * r;
          if (col < n && orow <= col) A[orow + (int64_t)col * ld] = acc[r];
        }
      }
    }
    __syncthreads();
  }

  if (fill) {                                // the strictly lower triangle: the mirror of the finished upper one
    for (int c = wave; c < n; c += NW)
      for (int r = lane; r < c; r += 64) A[c + (int64_t)r * ld] = A[r + (int64_t)c * ld];
  }
}

}  // namespace
