// The device side that potrf_batched_blocked.hip and potrf_vbatched.hip share: the factorization and the solve of ONE block of 65 .. 256
// rows by one workgroup, as functions of the block's address, leading dimension and size.  The algorithm is described at the head of
// potrf_batched_blocked.hip; the kernels there and in potrf_vbatched.hip differ in how a workgroup finds its block, and in nothing else.
// The solve is bb_forward_sweep followed by bb_backward_sweep; trsm_batched.hip runs one of the two alone.
#pragma once
#include <math.h>

#include <utility>

#include "common.h"

namespace {

constexpr int BB_MAX = 256;           // largest block
constexpr int BB_SMALL = 64;          // up to here: potrf_batched.hip's kernels
constexpr int BB_NB = 64;             // rows of a diagonal block
constexpr int BB_THREADS = 256;
constexpr int BB_WAVES = BB_THREADS / 64;
constexpr int BB_CH = 8;              // rows per wave-uniform "is this chunk below nb" branch
constexpr int BB_KP = 16;             // right-hand sides per pass of the solve
constexpr int BB_LDY = BB_KP + 1;

// the packed image of a 64 x 64 upper triangle (PbImg<64> of potrf_batched.hip): rows r < 32 start their line, row 63 - r fills its rest
struct BbImg {
  static constexpr int LD = BB_NB + 2;
  static constexpr int SIZE = (BB_NB / 2) * LD;
  static __device__ __forceinline__ constexpr int at(int r, int c) { return r < BB_NB / 2 ? r * LD + (c - r) : (BB_NB - 1 - r) * LD + c + 1; }
};

struct BbArgs {
  double* A; int64_t lda, stride_a;
  int* info; double* logdet;
  int n;
};

struct BbSolveArgs {
  const double* R; int64_t ldr, stride_r;
  double* B; int64_t ldb, stride_b, nrhs;
  const int* info;
  int n;
};

// orders one wave's LDS stores before its later LDS loads of other lanes' data (a wave's LDS instructions execute in order)
__device__ __forceinline__ void bb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double bb_readlane(double v, const int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// An opaque zero (as in leaf.hip): added to an LDS pointer it keeps the compiler from turning every uniform LDS address of the unrolled steps
// into its own constant in SGPRs; with it the accesses are "one VGPR + immediate offset".
__device__ __forceinline__ int bb_opaque_zero() { int z = 0; asm volatile("" : "+v"(z)); return z; }

// upper triangle of the nb x nb block at M -> image, by all waves; lane r walks along row r, so a column is contiguous
__device__ __forceinline__ void bb_load_upper(const double* M, int64_t ld, int nb, int lane, int wave, int waves, double* s) {
  for (int c = wave; c < nb; c += waves)
    if (lane <= c) s[BbImg::at(lane, c)] = M[lane + (int64_t)c * ld];
}

// step J of the diagonal block's factorization on one wave (J is a compile-time constant at every call: every index of a[] is static)
__device__ __forceinline__ void bb_factor_step(double (&a)[BB_NB], double* s, int c, int nb, int k0, const int J, int& info, bool& bad) {
  if (J >= nb) return;
  const double d = bb_readlane(a[J], J);
  const bool ok = d > 0.0;               // false for a NaN too
  if (!ok && !bad) info = k0 + J + 1;
  bad = bad || !ok;
  const double sq = __dsqrt_rn(d);
  double r = c == J ? sq : a[J] / sq;
  r = bad ? (double)NAN : r;
  if (c >= J) s[BbImg::at(J, c)] = r;      // row J of R11, for the panel solve and the store; the wave itself takes r_ji from lane i
#pragma unroll
  for (int i0 = ((J + 1) / BB_CH) * BB_CH; i0 < BB_NB; i0 += BB_CH) {
    if (i0 < nb) {
#pragma unroll
      for (int i = (i0 > J + 1 ? i0 : J + 1); i < i0 + BB_CH; i++) a[i] = fma(-bb_readlane(r, i), r, a[i]);
    }
  }
}
template <int... J>
__device__ __forceinline__ void bb_factor_steps(double (&a)[BB_NB], double* s, int c, int nb, int k0, int& info, bool& bad, std::integer_sequence<int, J...>) {
  (bb_factor_step(a, s, c, nb, k0, J, info, bad), ...);
}

// R11^T y = b, step J: y_j = b_j / r_jj, then b_i -= r_ji y_j for i > j (row j of R11: contiguous in the image)
__device__ __forceinline__ void bb_forward_step(double (&x)[BB_NB], const double* s, int nb, const int J) {
  if (J >= nb) return;
  x[J] = x[J] / s[BbImg::at(J, J)];
#pragma unroll
  for (int i0 = ((J + 1) / BB_CH) * BB_CH; i0 < BB_NB; i0 += BB_CH) {
    if (i0 < nb) {
#pragma unroll
      for (int i = (i0 > J + 1 ? i0 : J + 1); i < i0 + BB_CH; i++) x[i] = fma(-s[BbImg::at(J, i)], x[J], x[i]);
    }
  }
}
// R11 x = y, step J (taken in descending order): x_j = y_j / r_jj, then y_i -= r_ij x_j for i < j (column j of R11)
__device__ __forceinline__ void bb_backward_step(double (&x)[BB_NB], const double* s, int nb, const int J) {
  if (J >= nb) return;
  x[J] = x[J] / s[BbImg::at(J, J)];
#pragma unroll
  for (int i = 0; i < J; i++) x[i] = fma(-s[BbImg::at(i, J)], x[J], x[i]);
}
template <int... J>
__device__ __forceinline__ void bb_forward_steps(double (&x)[BB_NB], const double* s, int nb, std::integer_sequence<int, J...>) {
  (bb_forward_step(x, s, nb, J), ...);
}
template <int... J>
__device__ __forceinline__ void bb_backward_steps(double (&x)[BB_NB], const double* s, int nb, std::integer_sequence<int, J...>) {
  (bb_backward_step(x, s, nb, BB_NB - 1 - J), ...);
}

// waves of the factor's workgroup: four where the LDS lets two workgroups share a CU (NBLK = 2), eight where it holds one
constexpr int bb_factor_waves(int nblk) { return nblk == 2 ? 4 : 8; }

// the factorization of ONE block by the whole workgroup (the algorithm: potrf_batched_blocked.hip); info_out / logdet_out (either may be null): the block's words are those at index slot
template <int NBLK>
__device__ __forceinline__ void bb_factor_block(double* A, const int64_t lda, const int n, int* info_out, double* logdet_out, const int64_t slot) {
  constexpr int NW = bb_factor_waves(NBLK);
  constexpr int PW = BB_NB * (NBLK - 1);      // widest row panel
  constexpr int LDP = PW + 1;
  __shared__ double s_img[BbImg::SIZE];
  __shared__ double s_pan[BB_NB * LDP];
  __shared__ double s_log[BB_NB * NBLK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  int info = 0;                                // wave 0 carries them from one diagonal block to the next
  bool bad = false;

  for (int k0 = 0; k0 < n; k0 += BB_NB) {
    const int nb = n - k0 < BB_NB ? n - k0 : BB_NB;
    const int t0 = k0 + BB_NB, m = n - t0;     // m > 0: a full diagonal block with m columns to its right
    const int mpad = m > 0 ? (m + 15) & ~15 : 0;
    double* D = A + k0 + (int64_t)k0 * lda;
    double* P = A + k0 + (int64_t)t0 * lda;

    // A. diagonal block -> image, row panel -> LDS
    bb_load_upper(D, lda, nb, lane, wave, NW, s_img);
    for (int c = wave; c < mpad; c += NW) s_pan[lane * LDP + c] = c < m ? P[lane + (int64_t)c * lda] : 0.0;
    __syncthreads();

    // B. the diagonal block on wave 0
    if (wave == 0) {
      double a[BB_NB];
#pragma unroll
      for (int i = 0; i < BB_NB; i++) {
        const double v = s_img[BbImg::at(i, lane)];
        a[i] = (i <= lane && lane < nb) ? v : 0.0;
      }
      bb_wave_sync();                          // the image is in registers: from here on it takes the rows of R11
      bb_factor_steps(a, s_img + bb_opaque_zero(), lane, nb, k0, info, bad, std::make_integer_sequence<int, BB_NB>{});
      bb_wave_sync();
      if (lane < nb) s_log[k0 + lane] = log(s_img[BbImg::at(lane, lane)]);
    }
    __syncthreads();

    // C. R11 -> memory; R12 = R11^-T A12, a column per lane
    for (int c = wave; c < nb; c += NW)
      if (lane <= c) D[lane + (int64_t)c * lda] = s_img[BbImg::at(lane, c)];
    if (m <= 0) break;                         // the last diagonal block (uniform over the workgroup)
    if (wave * 64 < m) {
      const int c = wave * 64 + lane;
      const bool on = c < m;
      double x[BB_NB];
#pragma unroll
      for (int i = 0; i < BB_NB; i++) x[i] = on ? s_pan[i * LDP + c] : 0.0;
      bb_forward_steps(x, s_img + bb_opaque_zero(), nb, std::make_integer_sequence<int, BB_NB>{});   // nb == 64 here; as a run-time value it keeps a row's LDS reads inside its step
#pragma unroll
      for (int i = 0; i < BB_NB; i++)
        if (on) s_pan[i * LDP + c] = x[i];
    }
    __syncthreads();

    // D. R12 -> memory; A22 -= R12^T R12 on the tiles that intersect the upper triangle
    for (int c = wave; c < m; c += NW) P[lane + (int64_t)c * lda] = s_pan[lane * LDP + c];
    const int mt = mpad >> 4;
    int t = 0;
    for (int bj = 0; bj < mt; bj++) {
      for (int bi = 0; bi <= bj; bi++, t++) {
        if ((t & (NW - 1)) != wave) continue;
        // MFMA A operand: lane -> R12[kk + kg][bi 16 + lr] (negated), B operand: R12[kk + kg][bj 16 + lr]; D: row bi 16 + kg + 4 r, column bj 16 + lr
        const int col = bj * 16 + lr, row0 = bi * 16 + kg;
        double* cp = A + (t0 + row0) + (int64_t)(t0 + col) * lda;
        d4 acc;
        bool live[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          live[r] = col < m && row0 + 4 * r <= col;
          acc[r] = 0.0;
          if (live[r]) acc[r] = cp[4 * r];
        }
        const double* pa = s_pan + kg * LDP + bi * 16 + lr;
        const double* pb = s_pan + kg * LDP + col;
#pragma unroll
        for (int kk = 0; kk < BB_NB; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[kk * LDP], pb[kk * LDP], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (live[r]) cp[4 * r] = acc[r];
      }
    }
    __syncthreads();                           // the next step reads what other waves stored, and reuses the LDS
  }

  if (tid == 0) {
    if (info_out) info_out[slot] = info;
    if (logdet_out) {                            // 2 sum_j log r_jj in ascending j
      double t = 0.0;
      for (int j = 0; j < n; j++) t += s_log[j];
      logdet_out[slot] = bad ? (double)NAN : 2.0 * t;
    }
  }
}

// The two halves of the solve on the n x BB_KP slice s_y of right-hand sides (element (i, k) at i BB_LDY + k, rows n .. npad - 1 and dead
// columns zero) by a workgroup of BB_THREADS; s_img: the diagonal block's image.  Each starts with a barrier and ends without one.
__device__ __forceinline__ void bb_forward_sweep(const double* R, const int64_t ldr, const int n, double* s_img, double* s_y, const int lane, const int wave) {
  const int lr = lane & 15, kg = lane >> 4;
  const int nblk = (n + BB_NB - 1) / BB_NB;
  // R^T y = b over the diagonal blocks in ascending order
  for (int d = 0; d < nblk; d++) {
    const int k0 = d * BB_NB, nb = n - k0 < BB_NB ? n - k0 : BB_NB, t0 = k0 + BB_NB;
    __syncthreads();
    bb_load_upper(R + k0 + (int64_t)k0 * ldr, ldr, nb, lane, wave, BB_WAVES, s_img);
    __syncthreads();
    if (wave == 0) {
      double x[BB_NB];
#pragma unroll
      for (int i = 0; i < BB_NB; i++) x[i] = i < nb ? s_y[(k0 + i) * BB_LDY + lr] : 0.0;
      bb_forward_steps(x, s_img + bb_opaque_zero(), nb, std::make_integer_sequence<int, BB_NB>{});
#pragma unroll
      for (int i = 0; i < BB_NB; i++)
        if (i < nb && lane < BB_KP) s_y[(k0 + i) * BB_LDY + lr] = x[i];
    }
    __syncthreads();
    // B2 -= R12^T Y1: MFMA A operand lane -> R[k0 + kk + kg][t0 + bi 16 + lr] (negated), B operand Y[k0 + kk + kg][lr]; D: row kg + 4 r, column lr
    const int mt = t0 < n ? (n - t0 + 15) >> 4 : 0;
    for (int bi = wave; bi < mt; bi += BB_WAVES) {
      const int i0 = t0 + bi * 16;
      const bool ain = i0 + lr < n;
      const double* ra = R + (k0 + kg) + (int64_t)(i0 + lr) * ldr;
      double* y = s_y + (i0 + kg) * BB_LDY + lr;
      const double* yb = s_y + (k0 + kg) * BB_LDY + lr;
      d4 acc;
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = y[4 * r * BB_LDY];
#pragma unroll
      for (int kk = 0; kk < BB_NB; kk += 4) {
        double a = 0.0;
        if (ain) a = -ra[kk];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[kk * BB_LDY], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; r++)
        if (i0 + kg + 4 * r < n) y[4 * r * BB_LDY] = acc[r];      // rows at or beyond n stay zero
    }
  }
}
__device__ __forceinline__ void bb_backward_sweep(const double* R, const int64_t ldr, const int n, double* s_img, double* s_y, const int lane, const int wave) {
  const int lr = lane & 15, kg = lane >> 4;
  const int nblk = (n + BB_NB - 1) / BB_NB;
  // R x = y over the diagonal blocks in descending order
  for (int d = nblk - 1; d >= 0; d--) {
    const int k0 = d * BB_NB, nb = n - k0 < BB_NB ? n - k0 : BB_NB;
    __syncthreads();
    bb_load_upper(R + k0 + (int64_t)k0 * ldr, ldr, nb, lane, wave, BB_WAVES, s_img);
    __syncthreads();
    if (wave == 0) {
      double x[BB_NB];
#pragma unroll
      for (int i = 0; i < BB_NB; i++) x[i] = i < nb ? s_y[(k0 + i) * BB_LDY + lr] : 0.0;
      bb_backward_steps(x, s_img + bb_opaque_zero(), nb, std::make_integer_sequence<int, BB_NB>{});
#pragma unroll
      for (int i = 0; i < BB_NB; i++)
        if (i < nb && lane < BB_KP) s_y[(k0 + i) * BB_LDY + lr] = x[i];
    }
    __syncthreads();
    // B1 -= R12 X2: MFMA A operand lane -> R[bi 16 + lr][k0 + kk + kg] (negated; zero at or beyond column n), B operand X[k0 + kk + kg][lr]
    const int kend = (nb + 3) & ~3;
    for (int bi = wave; bi < k0 / 16; bi += BB_WAVES) {
      const double* ra = R + (bi * 16 + lr) + (int64_t)(k0 + kg) * ldr;
      double* y = s_y + (bi * 16 + kg) * BB_LDY + lr;
      const double* yb = s_y + (k0 + kg) * BB_LDY + lr;
      d4 acc;
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = y[4 * r * BB_LDY];
      for (int kk = 0; kk < kend; kk += 4) {
        double a = 0.0;
        if (k0 + kk + kg < n) a = -ra[(int64_t)kk * ldr];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[kk * BB_LDY], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) y[4 * r * BB_LDY] = acc[r];
    }
  }
}

// the solve of ONE block's right-hand sides by a workgroup of BB_THREADS; info (may be null): a block with info[slot] != 0 gets NaN
__device__ __forceinline__ void bb_solve_block(const double* R, const int64_t ldr, double* B, const int64_t ldb, const int64_t nrhs, const int n, const int* info, const int64_t slot) {
  __shared__ double s_img[BbImg::SIZE];
  __shared__ double s_y[BB_MAX * BB_LDY];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npad = (n + 15) & ~15;

  if (info && info[slot] != 0) {     // a failed block: NaN (uniform over the workgroup)
    for (int64_t k = wave; k < nrhs; k += BB_WAVES)
      for (int i = lane; i < n; i += 64) B[i + k * ldb] = (double)NAN;
    return;
  }

  for (int64_t p0 = 0; p0 < nrhs; p0 += BB_KP) {
    const int kc = nrhs - p0 < BB_KP ? (int)(nrhs - p0) : BB_KP;
    for (int k = wave; k < BB_KP; k += BB_WAVES)
      for (int i = lane; i < npad; i += 64) s_y[i * BB_LDY + k] = (k < kc && i < n) ? B[i + (p0 + k) * ldb] : 0.0;

    bb_forward_sweep(R, ldr, n, s_img, s_y, lane, wave);
    bb_backward_sweep(R, ldr, n, s_img, s_y, lane, wave);
    __syncthreads();
    for (int k = wave; k < kc; k += BB_WAVES)
      for (int i = lane; i < n; i += 64) B[i + (p0 + k) * ldb] = s_y[i * BB_LDY + k];
    __syncthreads();                           // the next pass refills the slice
  }
}

}  // namespace
