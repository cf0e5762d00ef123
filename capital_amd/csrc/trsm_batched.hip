// Batched triangular solves and products on the upper factors the batched Cholesky calls keep on the device (cap_dtrsm_batched,
// cap_dtrmm_batched and, on a cap_vbatch_plan, cap_dtrsm_vbatched, cap_dtrmm_vbatched): left side, upper triangle, non-unit diagonal,
// 1 <= n <= 256, in place on B with the layout of cap_dpotrs_batched[_blocked] / cap_dpotrs_vbatched.
//   trsm  CAP_TRANS: B_i <- R_i^-T B_i (the first half of potrs: whitening),  CAP_NOTRANS: B_i <- R_i^-1 B_i (its second half)
//   trmm  CAP_TRANS: B_i <- R_i^T B_i  (colouring),                           CAP_NOTRANS: B_i <- R_i B_i
// ONE launch per fixed-size call on a 1-D grid, one per occurring size class on a plan; no scratch, no allocation, no memset, no atomics, no
// helper stream, no host synchronisation, nothing between workgroups.
//
// n <= 64: potrs_batched_kernel's structure (potrf_batched.hip) - a wavefront per 64 / NP blocks, NP = 8 / 16 / 32 / 64, R's triangle in the
// PbImg LDS image, lane k of a group owns column k0 + k of its block in registers x[0 .. NP), more than NP columns are further passes.  Every
// register index is static; steps and row chunks at or beyond n are skipped by wave-uniform branches.  No lane talks to another one.
//   trsm runs pb_forward_step (TRANS) or pb_backward_step (NOTRANS) of batched_small.h alone, in potrs's order.
//   trmm runs column sweeps too, so that every product is an independent fused multiply-add against an LDS broadcast of R:
//     TRANS,   steps J = n - 1 .. 0:  x_i = fma(r_Ji, x_J, x_i) for i > J (row J of R), then x_J = r_JJ x_J.  Row i of R^T x is therefore
//              summed as  r_ii x_i, + r_(i-1)i x_(i-1), + ... + r_0i x_0  - from the diagonal outwards, one fma per term.
//     NOTRANS, steps J = 0 .. n - 1:  x_i = fma(r_iJ, x_J, x_i) for i < J (column J of R), then x_J = r_JJ x_J.  Row i of R x is summed as
//              r_ii x_i, + r_i(i+1) x_(i+1), + ... + r_i(n-1) x_(n-1).
//     x_J is still the input when step J reads it: the steps that change row J as an off-diagonal row come later in either order.
//
// 64 < n <= 256: bb_solve_block's structure (batched_blocked.h) - a workgroup of BB_THREADS per block, 16 columns per pass in the s_y LDS slice,
// the diagonal block of 64 rows on wave 0 (lane k: column k), the off-diagonal blocks on the fp64 16 x 16 x 4 MFMA.
//   trsm TRANS is bb_forward_sweep, NOTRANS bb_backward_sweep (batched_blocked.h): the two calls bb_solve_block itself makes.
//   trmm NOTRANS, diagonal blocks ascending: Y1 = R11 X1 by the steps above, then Y1 += R12 X2 on the MFMA with K ascending over the columns to
//     the right - rows that are not yet overwritten.  TRANS, descending: Y1 = R11^T X1, then Y1 += R01^T X0 with K ascending over the rows above.
//     A row's sum is: its diagonal block's terms in the order above, then the MFMA terms in ascending K, four per instruction.
//   An MFMA output column depends on its own input column only.
//
// sumsq (trsm only): the thread that owns a finished column - its lane on the wave path, lane k of wave 0 on the finished slice above 64 rows -
// computes q = 0; for r = 0 .. n - 1: q = fma(x_r, x_r, q) from the values that are stored to B: ONE recurrence on both paths, a function of the
// stored column alone.
//
// THE BIT CONTRACTS.  1. trsm(TRANS) followed by trsm(NOTRANS) leaves what cap_dpotrs_batched_blocked leaves: the same steps in the same order
// on the same values (above 64 rows the same two functions; a store and a load between the halves change no bit), NaN for failed blocks
// included.  2. On a plan every block gets the bits of the fixed-size entry on it alone: above 64 rows the same body on another address; up to 64 rows the group's own n is the n of every
// step (a lane mask: each lane executes its block's fixed-size sequence), the wave-uniform skip is on the wave's largest n.  3. A column's
// result and sumsq do not depend on the columns that travel with it.
// SHARED (vbatch_plan.h): the argument rules, the grid and the dispatch of the entry points, the walk over a plan's classes and the lane
// group's block lookup of tri_vbatched_kernel.
#include <utility>
#include <vector>

#include "batched_small.h"
#include "batched_blocked.h"
#include "capital_amd.h"
#include "vbatch_plan.h"

namespace {

constexpr int TB_MAX = 256;
enum { TB_SOLVE_T, TB_SOLVE_N, TB_MUL_T, TB_MUL_N };

struct TbArgs {
  const double* R; int64_t ldr, stride_r;      // fixed size
  double* B; int64_t ldb, stride_b, batch, nrhs;
  const int* info;
  double* sumsq; int64_t ldq;
  int n;
  const VbRec* rec;                            // plan: one class of one call
  const int64_t* list; int64_t count;
};

// R^T x, step J (taken in descending order): x_i += r_ji x_j for i > j (row j of R: contiguous in the image), then x_j = r_jj x_j
template <int NP>
__device__ __forceinline__ void tb_mul_t_step(double (&x)[NP], const double* s, int n, const int J) {
  using Img = PbImg<NP>;
  if (J >= n) return;
#pragma unroll
  for (int i0 = ((J + 1) / PB_CH) * PB_CH; i0 < NP; i0 += PB_CH) {
    if (i0 < n) {
#pragma unroll
      for (int i = (i0 > J + 1 ? i0 : J + 1); i < i0 + PB_CH; i++) x[i] = fma(s[Img::at(J, i)], x[J], x[i]);
    }
  }
  x[J] = s[Img::at(J, J)] * x[J];
}

// R x, step J (taken in ascending order): x_i += r_ij x_j for i < j (column j of R), then x_j = r_jj x_j
template <int NP>
__device__ __forceinline__ void tb_mul_n_step(double (&x)[NP], const double* s, int n, const int J) {
  using Img = PbImg<NP>;
  if (J >= n) return;
#pragma unroll
  for (int i = 0; i < J; i++) x[i] = fma(s[Img::at(i, J)], x[J], x[i]);
  x[J] = s[Img::at(J, J)] * x[J];
}

// the steps of one operation on one column; nmax: the wave-uniform skip (the fixed-size kernels pass n itself), n: the block's own size
template <int NP, int OP>
__device__ __forceinline__ void tb_step(double (&x)[NP], const double* s, int nmax, int n, const int J) {
  if (J >= nmax) return;
  if constexpr (OP == TB_SOLVE_T) pb_forward_step<NP>(x, s, n, J);
  else if constexpr (OP == TB_SOLVE_N) pb_backward_step<NP>(x, s, n, J);
  else if constexpr (OP == TB_MUL_T) tb_mul_t_step<NP>(x, s, n, J);
  else tb_mul_n_step<NP>(x, s, n, J);
}
constexpr bool tb_ascending(int op) { return op == TB_SOLVE_T || op == TB_MUL_N; }

// NP = 64 takes the parameter-pack form (see batched_small.h)
template <int NP, int OP, int... J>
__device__ __forceinline__ void tb_steps(double (&x)[NP], const double* s, int nmax, int n, std::integer_sequence<int, J...>) {
  if constexpr (tb_ascending(OP)) (tb_step<NP, OP>(x, s, nmax, n, J), ...);
  else (tb_step<NP, OP>(x, s, nmax, n, NP - 1 - J), ...);
}

template <int NP, int OP>
__device__ __forceinline__ void tb_run(double (&x)[NP], const double* s, int nmax, int n) {
  if constexpr (NP < 64) {
    if constexpr (tb_ascending(OP)) {
#pragma unroll
      for (int j = 0; j < NP; j++) tb_step<NP, OP>(x, s, nmax, n, j);
    } else {
#pragma unroll
      for (int j = NP - 1; j >= 0; j--) tb_step<NP, OP>(x, s, nmax, n, j);
    }
  } else {
    tb_steps<NP, OP>(x, s, nmax, n, std::make_integer_sequence<int, NP>{});
  }
}

// ------------------------------------------------------------------------------------------------ n <= 64: a wavefront per 64 / NP blocks
// the passes over the columns of one group's block: b0 = its B, live = it has a block, n = the block's size, nmax = the wave's largest n
// (the fixed-size kernel: n itself), q = its sumsq row or null
template <int NP, int OP>
__device__ __forceinline__ void tb_small_passes(const double* s, double* b0, int64_t ldb, int64_t nrhs, int k, bool live, int n, int nmax, bool bad, double* q) {
  for (int64_t k0 = 0; k0 < nrhs; k0 += NP) {
    const bool on = live && k0 + k < nrhs;
    double* b = b0 + (on ? (k0 + k) * ldb : 0);
    double x[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
      double t = 0.0;                        // a scalar temporary: assigning x[i] twice made the NP = 16 instances wait for every load in turn
      if (i < nmax) { if (on && i < n) t = b[i]; }
      x[i] = t;
    }
    tb_run<NP, OP>(x, s, nmax, n);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < NP; i++) {
      if (i < nmax) {
        if (on && i < n) {
          const double v = bad ? (double)NAN : x[i];
          b[i] = v;
          acc = fma(v, v, acc);
        }
      }
    }
    if constexpr (OP == TB_SOLVE_T || OP == TB_SOLVE_N) {
      if (q && on) q[k0 + k] = acc;
    }
  }
}

template <int NP, int OP>
__global__ __launch_bounds__(64) void tri_batched_kernel(TbArgs g) {
  constexpr int G = 64 / NP;
  using Img = PbImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  const int lane = threadIdx.x, grp = lane / NP, k = lane % NP, n = g.n;
  const int64_t blk = (int64_t)blockIdx.x * G + grp;
  const bool live = blk < g.batch;
  pb_load_upper<NP>(g.R + (live ? blk * g.stride_r : 0), g.ldr, n, k, live, s_img + grp * Img::SIZE);
  const bool bad = g.info && live && g.info[blk] != 0;
  __syncthreads();
  tb_small_passes<NP, OP>(s_img + grp * Img::SIZE, g.B + (live ? blk * g.stride_b : 0), g.ldb, g.nrhs, k, live, n, n, bad,
                          g.sumsq && live ? g.sumsq + blk * g.ldq : nullptr);
}

template <int NP, int OP>
__global__ __launch_bounds__(64) void tri_vbatched_kernel(TbArgs g) {
  constexpr int G = 64 / NP;
  using Img = PbImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  const int lane = threadIdx.x, grp = lane / NP, k = lane % NP;
  const VbGroup v = vb_group<NP>(g.rec, g.list, g.count);
  const int n = v.n, nmax = v.nmax;
  double* s = s_img + grp * Img::SIZE;
  vb_load_upper<Img>(g.R + v.off, v.ld, n, nmax, k, s);
  const bool bad = g.info && n > 0 && g.info[v.blk] != 0;
  __syncthreads();
  tb_small_passes<NP, OP>(s, g.B + v.row, g.ldb, g.nrhs, k, n > 0, n, nmax, bad, g.sumsq && n > 0 ? g.sumsq + v.blk * g.ldq : nullptr);
}

// ------------------------------------------------------------------------------------------------ 64 < n <= 256: a workgroup per block
template <int OP, int... J>
__device__ __forceinline__ void tb_diag_steps(double (&x)[BB_NB], const double* s, int nb, std::integer_sequence<int, J...>) {
  if constexpr (OP == TB_MUL_N) (tb_mul_n_step<BB_NB>(x, s, nb, J), ...);
  else (tb_mul_t_step<BB_NB>(x, s, nb, BB_NB - 1 - J), ...);
}

// one operation on ONE block's right-hand sides by a workgroup of BB_THREADS (bb_solve_block's frame); q: the block's sumsq row or null
template <int OP>
__device__ __forceinline__ void tb_blocked_block(const double* R, const int64_t ldr, double* B, const int64_t ldb, const int64_t nrhs, const int n, const int* info,
                                                 const int64_t slot, double* q) {
  static_assert(BbImg::SIZE == PbImg<BB_NB>::SIZE, "the product steps address the diagonal block's image as PbImg<64>");
  __shared__ double s_img[BbImg::SIZE];
  __shared__ double s_y[BB_MAX * BB_LDY];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  const int npad = (n + 15) & ~15;
  const int nblk = (n + BB_NB - 1) / BB_NB;

  if (info && info[slot] != 0) {     // a failed block: NaN (uniform over the workgroup)
    for (int64_t k = wave; k < nrhs; k += BB_WAVES)
      for (int i = lane; i < n; i += 64) B[i + k * ldb] = (double)NAN;
    if (q)
      for (int64_t k = tid; k < nrhs; k += BB_THREADS) q[k] = (double)NAN;
    return;
  }

  for (int64_t p0 = 0; p0 < nrhs; p0 += BB_KP) {
    const int kc = nrhs - p0 < BB_KP ? (int)(nrhs - p0) : BB_KP;
    for (int k = wave; k < BB_KP; k += BB_WAVES)
      for (int i = lane; i < npad; i += 64) s_y[i * BB_LDY + k] = (k < kc && i < n) ? B[i + (p0 + k) * ldb] : 0.0;

    if constexpr (OP == TB_SOLVE_T) {
      bb_forward_sweep(R, ldr, n, s_img, s_y, lane, wave);
    } else if constexpr (OP == TB_SOLVE_N) {
      bb_backward_sweep(R, ldr, n, s_img, s_y, lane, wave);
    } else {
      // products: NOTRANS ascending (Y1 = R11 X1, += R12 X2 from the rows below, not yet overwritten), TRANS descending (Y1 = R11^T X1,
      // += R01^T X0 from the rows above)
      for (int dd = 0; dd < nblk; dd++) {
        const int d = OP == TB_MUL_N ? dd : nblk - 1 - dd;
        const int k0 = d * BB_NB, nb = n - k0 < BB_NB ? n - k0 : BB_NB, t0 = k0 + BB_NB;
        __syncthreads();
        bb_load_upper(R + k0 + (int64_t)k0 * ldr, ldr, nb, lane, wave, BB_WAVES, s_img);
        __syncthreads();
        if (wave == 0) {
          double x[BB_NB];
#pragma unroll
          for (int i = 0; i < BB_NB; i++) x[i] = i < nb ? s_y[(k0 + i) * BB_LDY + lr] : 0.0;
          tb_diag_steps<OP>(x, s_img + bb_opaque_zero(), nb, std::make_integer_sequence<int, BB_NB>{});
#pragma unroll
          for (int i = 0; i < BB_NB; i++)
            if (i < nb && lane < BB_KP) s_y[(k0 + i) * BB_LDY + lr] = x[i];
        }
        __syncthreads();
        const int mt = (nb + 15) >> 4;           // 16-row tiles of this diagonal block's rows
        if constexpr (OP == TB_MUL_N) {
          // MFMA A operand lane -> R[k0 + bi 16 + lr][kk + kg] (zero at or beyond column n), B operand X[kk + kg][lr], kk = t0, t0 + 4, ...
          // (t0 < n only below a full diagonal block: every row k0 .. k0 + 63 is a row of R)
          if (t0 < n) {
            const int kend = (n + 3) & ~3;
            for (int bi = wave; bi < mt; bi += BB_WAVES) {
              const double* ra = R + (k0 + bi * 16 + lr) + (int64_t)kg * ldr;
              double* y = s_y + (k0 + bi * 16 + kg) * BB_LDY + lr;
              const double* yb = s_y + kg * BB_LDY + lr;
              d4 acc;
#pragma unroll
              for (int r = 0; r < 4; r++) acc[r] = y[4 * r * BB_LDY];
              for (int kk = t0; kk < kend; kk += 4) {
                double a = 0.0;
                if (kk + kg < n) a = ra[(int64_t)kk * ldr];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[kk * BB_LDY], acc, 0, 0, 0);   // rows n .. npad - 1 of the slice are zeros
              }
#pragma unroll
              for (int r = 0; r < 4; r++) y[4 * r * BB_LDY] = acc[r];
            }
          }
        } else {
          // MFMA A operand lane -> R[kk + kg][k0 + bi 16 + lr] (zero at or beyond column n), B operand X[kk + kg][lr], kk = 0, 4, ... < k0
          for (int bi = wave; bi < mt && k0 > 0; bi += BB_WAVES) {
            const int i0 = k0 + bi * 16;
            const bool ain = i0 + lr < n;
            const double* ra = R + kg + (int64_t)(i0 + lr) * ldr;
            double* y = s_y + (i0 + kg) * BB_LDY + lr;
            const double* yb = s_y + kg * BB_LDY + lr;
            d4 acc;
#pragma unroll
            for (int r = 0; r < 4; r++) acc[r] = y[4 * r * BB_LDY];
            for (int kk = 0; kk < k0; kk += 4) {
              double a = 0.0;
              if (ain) a = ra[kk];
              acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[kk * BB_LDY], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; r++)
              if (i0 + kg + 4 * r < n) y[4 * r * BB_LDY] = acc[r];    // rows at or beyond n stay zero
          }
        }
      }
    }
    __syncthreads();
    for (int k = wave; k < kc; k += BB_WAVES)
      for (int i = lane; i < n; i += 64) B[i + (p0 + k) * ldb] = s_y[i * BB_LDY + k];
    if constexpr (OP == TB_SOLVE_T || OP == TB_SOLVE_N) {
      if (q && tid < kc) {                       // the finished slice, one lane per column: the wave path's recurrence
        double acc = 0.0;
        for (int i = 0; i < n; i++) {
          const double v = s_y[i * BB_LDY + tid];
          acc = fma(v, v, acc);
        }
        q[p0 + tid] = acc;
      }
    }
    __syncthreads();                           // the next pass refills the slice
  }
}

template <int OP>
__global__ __launch_bounds__(BB_THREADS) void tri_batched_blocked_kernel(TbArgs g) {
  const int64_t blk = blockIdx.x;
  tb_blocked_block<OP>(g.R + blk * g.stride_r, g.ldr, g.B + blk * g.stride_b, g.ldb, g.nrhs, g.n, g.info, blk, g.sumsq ? g.sumsq + blk * g.ldq : nullptr);
}

template <int OP>
__global__ __launch_bounds__(BB_THREADS) void tri_vbatched_blocked_kernel(TbArgs g) {
  const int64_t blk = g.list[blockIdx.x];
  const VbRec r = g.rec[blk];
  tb_blocked_block<OP>(g.R + r.off, r.ld, g.B + r.row, g.ldb, g.nrhs, (int)r.n, g.info, blk, g.sumsq ? g.sumsq + blk * g.ldq : nullptr);
}

// ------------------------------------------------------------------------------------------------ host
constexpr int tb_op(int mul, int trans) { return mul ? (trans == CAP_TRANS ? TB_MUL_T : TB_MUL_N) : (trans == CAP_TRANS ? TB_SOLVE_T : TB_SOLVE_N); }

// f(OP) with the operation as a template argument
template <class F>
void tb_with_op(int op, F f) { vb_with_int<TB_SOLVE_T, TB_SOLVE_N, TB_MUL_T, TB_MUL_N>(op, f); }

int tb_fixed(int mul, int uplo, int trans, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
             int64_t stride_b, int64_t batch, const int* info, double* sumsq, int64_t ldq, hipStream_t s) {
  if ((trans != CAP_NOTRANS && trans != CAP_TRANS) || n < 0 || nrhs < 0 || batch < 0) return CAP_ERR_ARG;
  if (n > 0 && nrhs > 0 && batch > 0 && (!R || !B)) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, ldr, stride_r, batch) || !vb_operand_ok(n, nrhs, ldb, stride_b, batch)) return CAP_ERR_ARG;
  if (sumsq && ldq < nrhs) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpotrs_batched
  if (n > TB_MAX) return CAP_ERR_UNSUPPORTED;
  const int64_t nwg = vb_grid(batch, vb_per_group(vb_class(n)));
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  if (n == 0 || nrhs == 0 || batch == 0) return CAP_OK;
  if (cap_acc_on()) {
    for (int64_t i = 0; i < batch; i++) {
      cap_acc_r(R + i * stride_r, ldr, n, n, 1);
      cap_acc_rw(B + i * stride_b, ldb, n, nrhs);
    }
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
    if (sumsq) cap_acc_w(sumsq, ldq, nrhs, batch);
  }
  TbArgs g = {};
  g.R = R; g.ldr = ldr; g.stride_r = stride_r; g.B = B; g.ldb = ldb; g.stride_b = stride_b; g.batch = batch; g.nrhs = nrhs; g.info = info;
  g.sumsq = sumsq; g.ldq = ldq; g.n = (int)n;
  const dim3 grid((unsigned)nwg);
  tb_with_op(tb_op(mul, trans), [&](auto OP) {
    if (n <= BB_SMALL) {
      vb_with_int<8, 16, 32, 64>(vb_padded(n), [&](auto NP) { hipLaunchKernelGGL((tri_batched_kernel<NP(), OP()>), grid, dim3(64), 0, s, g); });
    } else {
      hipLaunchKernelGGL((tri_batched_blocked_kernel<OP()>), grid, dim3(BB_THREADS), 0, s, g);
    }
  });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int tb_plan(int mul, const cap_vbatch_plan* p, int uplo, int trans, int64_t nrhs, const double* R, double* B, int64_t ldb, const int* info,
            double* sumsq, int64_t ldq, hipStream_t s) {
  if (!p || (trans != CAP_NOTRANS && trans != CAP_TRANS) || nrhs < 0) return CAP_ERR_ARG;
  if (p->nonempty > 0 && nrhs > 0 && (!R || !B)) return CAP_ERR_ARG;
  if (ldb < p->rows) return CAP_ERR_ARG;
  if (sumsq && ldq < nrhs) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (p->nonempty == 0 || nrhs == 0) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  TbArgs g = {};
  g.R = R; g.B = B; g.ldb = ldb; g.nrhs = nrhs; g.info = info; g.sumsq = sumsq; g.ldq = ldq; g.rec = p->d_rec;
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    g.list = list;
    g.count = count;
    if (cap_acc_on()) {
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[(size_t)b];
        cap_acc_r(R + r.off, r.ld, r.n, r.n, 1);
        cap_acc_rw(B + r.row, ldb, r.n, nrhs);
        if (info) cap_acc_r(info + b, 0, 1, 1, 0, 4);
        if (sumsq) cap_acc_w(sumsq + b * ldq, 0, nrhs, 1);
      }
    }
    tb_with_op(tb_op(mul, trans), [&](auto OP) {
      if (cls < 4) {
        vb_with_int<8, 16, 32, 64>(8 << cls, [&](auto NP) { hipLaunchKernelGGL((tri_vbatched_kernel<NP(), OP()>), grid, dim3(64), 0, s, g); });
      } else {
        hipLaunchKernelGGL((tri_vbatched_blocked_kernel<OP()>), grid, dim3(BB_THREADS), 0, s, g);
      }
    });
  });
}

}  // namespace

extern "C" {

int cap_dtrsm_batched(int uplo, int trans, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                      int64_t stride_b, int64_t batch, const int* info, double* sumsq, int64_t ldq, void* stream) {
  return tb_fixed(0, uplo, trans, n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, sumsq, ldq, cap_stream(stream));
}

int cap_dtrmm_batched(int uplo, int trans, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                      int64_t stride_b, int64_t batch, const int* info, void* stream) {
  return tb_fixed(1, uplo, trans, n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, nullptr, 0, cap_stream(stream));
}

int cap_dtrsm_vbatched(const cap_vbatch_plan* p, int uplo, int trans, int64_t nrhs, const double* R, double* B, int64_t ldb, const int* info,
                       double* sumsq, int64_t ldq, void* stream) {
  return tb_plan(0, p, uplo, trans, nrhs, R, B, ldb, info, sumsq, ldq, cap_stream(stream));
}

int cap_dtrmm_vbatched(const cap_vbatch_plan* p, int uplo, int trans, int64_t nrhs, const double* R, double* B, int64_t ldb, const int* info,
                       void* stream) {
  return tb_plan(1, p, uplo, trans, nrhs, R, B, ldb, info, nullptr, 0, cap_stream(stream));
}

}  // extern "C"
