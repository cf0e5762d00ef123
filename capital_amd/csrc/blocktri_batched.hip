// Batched BLOCK-TRIDIAGONAL Cholesky factor and solve (cap_dpotrf_blocktri_batched, cap_dpotrs_blocktri_batched): `batch` independent
// chains, each a symmetric positive definite block-tridiagonal matrix of T diagonal blocks D_0 .. D_(T-1) of n x n, 1 <= n <= 64, coupled
// to their neighbours by B_i = A[block i, block i + 1] in the column-major n x n block E_i, i = 0 .. T - 2.  In place:
//   S_0 = D_0;   U_i = chol(S_i) (upper, in the upper triangle of D_i);   W_i = U_i^-T B_i (in E_i);   S_(i+1) = D_(i+1) - W_i^T W_i.
// A = R^T R with R block upper bidiagonal (U_i on the diagonal, W_i to its right); read row-major (torch) the same memory holds the block
// lower bidiagonal L = R^T: L_ii in the lower triangle of D[c, i], L_(i+1, i) in E[c, i].
// ONE launch per call on a 1-D grid; a workgroup is one wavefront that carries G = 64 / NP chains (NP = 8 / 16 / 32 / 64 >= n) in lane
// groups of NP lanes and walks their T positions in a loop.  No scratch, no allocation, no memset, no atomics, no mutex, no helper stream,
// nothing between workgroups (the __syncthreads are the order of the wavefront's own LDS accesses); 64-bit offsets.
//
// THE ARITHMETIC IS A COMPOSITION of what the family states, and that is the bit contract: a chain's D, E, info, logdet and solutions are,
// bit for bit, what the fixed-size entries give when the host drives the recurrence on the chain's blocks.
//   factor, position i ascending:   cap_dpotrf_batched on S_i (pb_factor_step, batched_small.h: the same function);
//                                   cap_dtrsm_batched(CAP_TRANS) with that factor and its info on the n columns of E_i (pb_forward_step);
//                                   cap_dsyrk_batched(CAP_TRANS, alpha = -1, beta = 1) into the upper triangle of D_(i+1): every element its
//                                   own chain on the fp64 16 x 16 x 4 MFMA from a ZERO accumulator, K ascending, four per instruction, rows at or
//                                   beyond n as +0.0, then t = alpha s, out = fma(beta, d, t), uncontracted.
//   solve, forward  i ascending:    cap_dtrsm_batched(CAP_TRANS) on segment i, then cap_dgemm_batched(CAP_TRANS, CAP_NOTRANS, alpha = -1, beta = 1)
//                                   b_(i+1) -= W_i^T y_i (the same MFMA chain and epilogue);
//          backward i descending:   cap_dgemm_batched(CAP_NOTRANS, CAP_NOTRANS, -1, 1)  y_i -= W_i x_(i+1), then cap_dtrsm_batched(CAP_NOTRANS).
//   info[c]: 0 or the 1-based row of the T n system of the first pivot that is not > 0 (i n + the row cap_dpotrf_batched reports for S_i);
//   logdet[c] = s after s = 0; s += ld_i, i ascending, ld_i what cap_dpotrf_batched returns for S_i (NaN for a failed one).
// A chain's bits therefore depend on (n, T, its data) alone - not on batch, the chain's index, leading dimensions, steps, strides,
// alignment, the chains that share its wavefront or the columns that travel with a column (the family's ELEMENT INDEPENDENCE:
// syrk_batched.hip, gemm_batched.hip).  After a failure at position i: D_i holds what cap_dpotrf_batched leaves, E_i .. E_(T-2) and the
// upper triangles of D_(i+1) .. D_(T-1) hold NaN (trsm's NaN for a failed factor, carried on by the products), the chain's solutions are
// NaN; no other chain is touched.
//
// HOW THE BLOCKS TRAVEL.  S_i lives in the PbImg LDS image of its lane group and never in global memory: the factor steps turn the image
// into U_i (stored to D_i once), lane c of the group runs the forward substitution on column c of E_i in registers against that image
// (stored to E_i once), the columns of W_i go to the wavefront's exchange area in LDS, the MFMA reads both operands from there, and the
// epilogue combines the product with D_(i+1) - read from global memory once, in the accumulator layout, BEFORE the factor steps of position
// i start, as is E_i - and writes S_(i+1) into the image.  D and E go once in and once out; the loads of the next position are in flight
// while this one is factored.  The solve keeps a right-hand-side column in the registers of its lane across the chain; the product with
// W_i takes the column through the exchange area to the MFMA and back, W_i comes straight from global memory as gemm_batched.hip reads it.
// More than NP right-hand sides are further passes inside the launch (each pass walks the chain again).
// A long chain is sequential in its wavefront: few long chains leave the chip idle (splitting a chain needs cyclic reduction, which
// changes the arithmetic: out of scope).
//
// EVERY ADDRESS AND PREDICATE is a function of blocktri_addr.h, swept lane by lane on the CPU (tests/test_blocktri_addr.py): position
// T - 1 has no coupling block and no successor, T = 1 has no E at all.
#include <math.h>

#include <utility>

#include "batched_small.h"
#include "blocktri_addr.h"
#include "capital_amd.h"
#include "common.h"
#include "vbatch_plan.h"

namespace {

struct BtArgs {
  double* D; double* E;
  BtGeo gd, ge;
  int* info; double* logdet;
};

struct BtSolveArgs {
  const double* D; const double* E;
  BtGeo gd, ge;
  double* B; int64_t ldb, stride_b, nrhs;
  const int* info;
  int half;
};

template <int NP>
constexpr bool bt_img_agrees() {
  using Img = PbImg<NP>;
  return Img::SIZE == bt_img_size(NP) && Img::LD == bt_img_ld(NP);
}

// the epilogue of syrk_batched.hip / gemm_batched.hip with alpha = -1, beta = 1, without contraction: t = alpha s; out = fma(beta, c, t)
__device__ __forceinline__ double bt_minus(const double c, const double s) {
#pragma clang fp contract(off)
  const double t = -1.0 * s;
  return __builtin_fma(1.0, c, t);
}

// NP = 64 takes the parameter-pack form of the steps (see batched_small.h)
template <int NP, int... J>
__device__ __forceinline__ void bt_forward_pack(double (&x)[NP], const double* s, int n, std::integer_sequence<int, J...>) {
  (pb_forward_step<NP>(x, s, n, J), ...);
}
template <int NP, int... J>
__device__ __forceinline__ void bt_backward_pack(double (&x)[NP], const double* s, int n, std::integer_sequence<int, J...>) {
  (pb_backward_step<NP>(x, s, n, NP - 1 - J), ...);
}
template <int NP>
__device__ __forceinline__ void bt_forward(double (&x)[NP], const double* s, int n) {
  if constexpr (NP < 64) {
#pragma unroll
    for (int j = 0; j < NP; j++) pb_forward_step<NP>(x, s, n, j);
  } else {
    bt_forward_pack<NP>(x, s, n, std::make_integer_sequence<int, NP>{});
  }
}
template <int NP>
__device__ __forceinline__ void bt_backward(double (&x)[NP], const double* s, int n) {
  if constexpr (NP < 64) {
#pragma unroll
    for (int j = NP - 1; j >= 0; j--) pb_backward_step<NP>(x, s, n, j);
  } else {
    bt_backward_pack<NP>(x, s, n, std::make_integer_sequence<int, NP>{});
  }
}

// the upper triangle of diagonal block `pos` -> the group's image (pb_load_upper's walk on the addresses of blocktri_addr.h)
template <int NP>
__device__ __forceinline__ void bt_load_tri(const double* D, const BtGeo& gd, const int64_t wg, const int lane, const int64_t pos, double* s) {
  const int r = bt_idx(NP, lane);
#pragma unroll 8
  for (int cc = 0; cc < gd.n; cc++) {
    const BtAt at = bt_tri_at(gd, wg, lane, pos, cc);
    if (at.on) s[bt_img_at(NP, r, cc)] = D[at.off];
  }
}

// column lane % NP of coupling block `pos` -> registers (+0.0 where the lane has none)
template <int NP>
__device__ __forceinline__ void bt_load_ecol(const double* E, const BtGeo& ge, const int64_t wg, const int lane, const int64_t pos, double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    double t = 0.0;
    if (i < ge.n) {
      const BtAt at = bt_ecol_at(ge, wg, lane, pos, i);
      if (at.on) t = E[at.off];
    }
    x[i] = t;
  }
}

// ------------------------------------------------------------------------------------------------ factor
template <int NP>
__global__ __launch_bounds__(64) void blocktri_potrf_kernel(BtArgs g) {
  constexpr int G = 64 / NP;
  constexpr bool EARLY = NP < 64;        // E_pos is requested in front of the factor steps where the registers allow it (D_(pos+1) always is)
  using Img = PbImg<NP>;
  static_assert(bt_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h");
  __shared__ double s_img[G * Img::SIZE];
  __shared__ double s_x[bt_x_size(NP)];
  __shared__ double s_log[64];
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane = threadIdx.x, c = bt_idx(NP, lane), n = gd.n;
  const int64_t wg = blockIdx.x, T = gd.T;
  const bool live = bt_live(gd, wg, lane);
  double* s = s_img + bt_img_base(NP, lane);

  bt_load_tri<NP>(g.D, gd, wg, lane, 0, s);
  __syncthreads();
  int cinfo = 0;
  double ldsum = 0.0;

  for (int64_t pos = 0; pos < T; pos++) {
    // what position pos + 1 needs from memory, requested before the steps of this one: column c of E_pos, D_(pos+1) in the accumulator layout
    double x[NP];
    if constexpr (EARLY) bt_load_ecol<NP>(g.E, ge, wg, lane, pos, x);
    double dn[4][4][4];
#pragma unroll
    for (int si = 0; si < 4; si++)
#pragma unroll
      for (int sj = 0; sj < 4; sj++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double t = 0.0;
          if (bt_tile(NP, si, sj, true)) {
            if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
              const BtAt at = bt_next_at(gd, wg, lane, pos, si, sj, r);
              if (at.on) t = g.D[at.off];
            }
          }
          dn[si][sj][r] = t;
        }

    double a[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
      const double v = s[Img::at(i, c)];
      a[i] = (i <= c && c < n) ? v : 0.0;
    }
    __syncthreads();                     // the image is in registers: from here on it takes the rows of U

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
    for (int cc = 0; cc < n; cc++) {
      const BtAt at = bt_tri_at(gd, wg, lane, pos, cc);
      if (at.on) g.D[at.off] = s[bt_img_at(NP, c, cc)];
    }
    if (info != 0 && cinfo == 0) cinfo = (int)(pos * n) + info;
    if (g.logdet) {                      // potrf_batched_kernel's: lane j takes the logarithm, lane 0 of the group adds them in ascending j
      s_log[bt_log_at(NP, lane, c)] = c < n ? log(s[Img::at(c, c)]) : 0.0;
      __syncthreads();
      if (c == 0) {
        double t = 0.0;
        for (int j = 0; j < n; j++) t += s_log[bt_log_at(NP, lane, j)];
        ldsum += bad ? (double)NAN : 2.0 * t;
      }
    }
    if (!bt_has_next(T, pos)) break;     // wave-uniform: the last position has no coupling block and no successor

    // W = U^-T B, column c in lane c; NaN behind a failed factor, as cap_dtrsm_batched with its info
    if constexpr (!EARLY) bt_load_ecol<NP>(g.E, ge, wg, lane, pos, x);
    bt_forward<NP>(x, s, n);
#pragma unroll
    for (int i = 0; i < NP; i++) {
      if (i < n) {
        const double v = bad ? (double)NAN : x[i];
        const BtAt at = bt_ecol_at(ge, wg, lane, pos, i);
        if (at.on) g.E[at.off] = v;
        s_x[bt_x_own(i, lane)] = at.on ? v : 0.0;
      }
    }
    __syncthreads();                     // the columns are in the exchange area; nobody reads the image any more

    // W^T W on the MFMA, syrk_batched.hip's tiles: wave row w is column w % NP of the W of chain w / NP
    d4 acc[4][4];
#pragma unroll
    for (int si = 0; si < 4; si++)
#pragma unroll
      for (int sj = 0; sj < 4; sj++) acc[si][sj] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int q0 = 0; q0 < n; q0 += 16) {
      double v[4][4];
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int sl = 0; sl < 4; sl++) {
          double t = 0.0;
          if (q0 + 4 * u < n && bt_slab_on(NP, sl, n)) {
            const BtAt at = bt_x_slab(n, lane, sl, q0 + 4 * u);
            if (at.on) t = s_x[at.off];
          }
          v[u][sl] = t;
        }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (q0 + 4 * u < n) {
#pragma unroll
          for (int si = 0; si < 4; si++)
#pragma unroll
            for (int sj = 0; sj < 4; sj++)
              if (bt_tile(NP, si, sj, true)) {
                if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n))
                  acc[si][sj] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u][sj], v[u][si], acc[si][sj], 0, 0, 0);
              }
        }
      }
    }
    // S_(pos+1) = D_(pos+1) - W^T W into the image
#pragma unroll
    for (int si = 0; si < 4; si++)
#pragma unroll
      for (int sj = 0; sj < 4; sj++)
        if (bt_tile(NP, si, sj, true)) {
          if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const BtAt at = bt_img_tile(n, NP, lane, si, sj, r);
              if (at.on) s_img[at.off] = bt_minus(dn[si][sj][r], acc[si][sj][r]);
            }
          }
        }
    __syncthreads();
  }

  const BtAt at = bt_scalar_at(gd, wg, lane);
  if (at.on) {
    g.info[at.off] = cinfo;
    if (g.logdet) g.logdet[at.off] = ldsum;
  }
  (void)live;
}

// ------------------------------------------------------------------------------------------------ solve
template <int NP>
__device__ __forceinline__ void bt_rhs_load(const BtSolveArgs& g, const BtGeo& gd, const int64_t wg, const int lane, const int64_t pass, const int64_t pos,
                                            double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    double t = 0.0;
    if (i < gd.n) {
      const BtAt at = bt_rhs_at(gd, g.ldb, g.stride_b, g.nrhs, wg, lane, pass, pos, i);
      if (at.on) t = g.B[at.off];
    }
    x[i] = t;
  }
}

template <int NP>
__device__ __forceinline__ void bt_rhs_store(const BtSolveArgs& g, const BtGeo& gd, const int64_t wg, const int lane, const int64_t pass, const int64_t pos,
                                             const bool bad, const double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    if (i < gd.n) {
      const BtAt at = bt_rhs_at(gd, g.ldb, g.stride_b, g.nrhs, wg, lane, pass, pos, i);
      if (at.on) g.B[at.off] = bad ? (double)NAN : x[i];
    }
  }
}

// x <- c - op(W_epos) x: the column of every lane through the exchange area to the MFMA and back; c is segment `tpos` of B.
// TRANS: op(W) = W^T (forward sweep), else W (backward sweep) - gemm_batched.hip's tiles: the slab of the columns is the MFMA's A operand
template <int NP, bool TRANS>
__device__ __forceinline__ void bt_couple(const BtSolveArgs& g, const BtGeo& gd, const BtGeo& ge, const int64_t wg, const int lane, const int64_t pass,
                                          const int64_t epos, const int64_t tpos, double* s_x, double (&x)[NP]) {
  const int n = gd.n;
  constexpr bool EARLY = NP < 64;        // the target segment is requested in front of the product where the registers allow it
  double cn[NP];
  if constexpr (EARLY) bt_rhs_load<NP>(g, gd, wg, lane, pass, tpos, cn);
#pragma unroll
  for (int i = 0; i < NP; i++)
    if (i < n) s_x[bt_x_own(i, lane)] = x[i];
  __syncthreads();

  bool onc[4];                           // wave-uniform: does column slab s hold a right-hand side of this pass
#pragma unroll
  for (int sl = 0; sl < 4; sl++) onc[sl] = pass * NP + (sl * 16) % NP < g.nrhs;
  d4 acc[4][4];
#pragma unroll
  for (int si = 0; si < 4; si++)
#pragma unroll
    for (int sj = 0; sj < 4; sj++) acc[si][sj] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int q0 = 0; q0 < n; q0 += 16) {
    double av[4][4], bv[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int sl = 0; sl < 4; sl++) {
        double ta = 0.0, tb = 0.0;
        if (q0 + 4 * u < n) {
          if (bt_slab_on(NP, sl, n)) {
            const BtAt at = bt_eslab_at(ge, wg, lane, epos, sl, q0 + 4 * u, TRANS);
            if (at.on) ta = g.E[at.off];
          }
          if (onc[sl]) {
            const BtAt at = bt_x_slab(n, lane, sl, q0 + 4 * u);
            if (at.on) tb = s_x[at.off];
          }
        }
        av[u][sl] = ta;
        bv[u][sl] = tb;
      }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (q0 + 4 * u < n) {
#pragma unroll
        for (int si = 0; si < 4; si++)
#pragma unroll
          for (int sj = 0; sj < 4; sj++)
            if (bt_tile(NP, si, sj, false)) {
              if (bt_slab_on(NP, si, n) && onc[sj]) acc[si][sj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[u][sj], av[u][si], acc[si][sj], 0, 0, 0);
            }
      }
    }
  }
  __syncthreads();                       // every lane has read the columns: the products take their place
#pragma unroll
  for (int si = 0; si < 4; si++)
#pragma unroll
    for (int sj = 0; sj < 4; sj++)
      if (bt_tile(NP, si, sj, false)) {
        if (bt_slab_on(NP, si, n) && onc[sj]) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const BtAt at = bt_x_tile(n, NP, lane, si, sj, r);
            if (at.on) s_x[at.off] = acc[si][sj][r];
          }
        }
      }
  __syncthreads();
  if constexpr (!EARLY) bt_rhs_load<NP>(g, gd, wg, lane, pass, tpos, cn);
#pragma unroll
  for (int i = 0; i < NP; i++)
    if (i < n) x[i] = bt_minus(cn[i], s_x[bt_x_own(i, lane)]);
}

template <int NP>
__global__ __launch_bounds__(64) void blocktri_potrs_kernel(BtSolveArgs g) {
  constexpr int G = 64 / NP;
  using Img = PbImg<NP>;
  static_assert(bt_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h");
  __shared__ double s_img[G * Img::SIZE];
  __shared__ double s_x[bt_x_size(NP)];
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane = threadIdx.x, n = gd.n;
  const int64_t wg = blockIdx.x, T = gd.T;
  double* s = s_img + bt_img_base(NP, lane);
  const BtAt ia = bt_info_at(gd, wg, lane);
  bool bad = false;
  if (g.info) { if (ia.on) bad = g.info[ia.off] != 0; }

  const int64_t passes = bt_rhs_passes(NP, g.nrhs);
  for (int64_t pass = 0; pass < passes; pass++) {
    double x[NP];
    if (g.half != 2) {                   // R^T y = b, positions ascending
      bt_rhs_load<NP>(g, gd, wg, lane, pass, 0, x);
      for (int64_t pos = 0; pos < T; pos++) {
        __syncthreads();                 // the image of the position before is read no more
        bt_load_tri<NP>(g.D, gd, wg, lane, pos, s);
        __syncthreads();
        bt_forward<NP>(x, s, n);
        bt_rhs_store<NP>(g, gd, wg, lane, pass, pos, bad, x);
        if (!bt_has_next(T, pos)) break;
        bt_couple<NP, true>(g, gd, ge, wg, lane, pass, pos, pos + 1, s_x, x);
      }
    }
    if (g.half != 1) {                   // R x = y, positions descending
      bt_rhs_load<NP>(g, gd, wg, lane, pass, T - 1, x);
      for (int64_t pos = T - 1; pos >= 0; pos--) {
        __syncthreads();
        bt_load_tri<NP>(g.D, gd, wg, lane, pos, s);
        __syncthreads();
        bt_backward<NP>(x, s, n);
        bt_rhs_store<NP>(g, gd, wg, lane, pass, pos, bad, x);
        if (pos == 0) break;
        bt_couple<NP, false>(g, gd, ge, wg, lane, pass, pos - 1, pos - 1, s_x, x);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// the rule of a chained operand: `batch` chains of `blocks` column-major n x n blocks, leading dimension ld, `step` apart, chains `stride`
// apart - no two blocks overlap (128-bit products, as vb_operand_ok)
static inline bool bt_operand_ok(int64_t n, int64_t blocks, int64_t ld, int64_t step, int64_t stride, int64_t batch) {
  if (blocks <= 0) return true;          // E with T <= 1: nothing is stored
  if (ld < n) return false;
  const __int128 blk = (__int128)ld * n;
  if (blocks > 1 && (__int128)step < blk) return false;
  if (batch > 1 && (__int128)stride < (blocks > 1 ? (__int128)step * blocks : blk)) return false;
  return true;
}

static void bt_geo(BtGeo& g, int64_t n, int64_t T, int64_t batch, int64_t ld, int64_t step, int64_t stride) {
  g.ld = ld; g.step = step; g.stride = stride; g.T = T; g.batch = batch; g.n = (int)n; g.NP = vb_padded(n);
}

// rules 5 - 8 of both entries; > 0: the workgroups, 0: refused (st holds the status)
static inline int64_t bt_limits(int uplo, int64_t n, int64_t T, int64_t batch, int& st) {
  st = CAP_ERR_UNSUPPORTED;
  if (uplo != CAP_UPPER) return 0;       // as the other batched entries
  if (n > BT_MAX) return 0;
  if ((__int128)T * n > (__int128)0x7fffffffLL) return 0;
  const int64_t nwg = vb_grid(batch, 64 / vb_padded(n));
  if (nwg < 0) return 0;
  st = CAP_OK;
  return nwg;
}

}  // namespace

extern "C" {

int cap_dpotrf_blocktri_batched(int uplo, int64_t n, int64_t T, double* D, int64_t ldd, int64_t step_d, int64_t stride_d, double* E, int64_t lde,
                                int64_t step_e, int64_t stride_e, int* info, double* logdet, int64_t batch, void* stream) {
  if (n < 0 || T < 0 || batch < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && T > 0 && batch > 0;
  if (work && (!D || !info || (!E && T > 1))) return CAP_ERR_ARG;
  if (!bt_operand_ok(n, T, ldd, step_d, stride_d, batch) || !bt_operand_ok(n, T - 1, lde, step_e, stride_e, batch)) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bt_limits(uplo, n, T, batch, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  BtArgs g = {};
  g.D = D; g.E = E; g.info = info; g.logdet = logdet;
  bt_geo(g.gd, n, T, batch, ldd, step_d, stride_d);
  bt_geo(g.ge, n, T, batch, lde, step_e, stride_e);
  if (cap_acc_on()) {
    for (int64_t c = 0; c < batch; c++)
      for (int64_t i = 0; i < T; i++) {
        cap_acc_rw(D + bt_block(g.gd, c, i), ldd, n, n, 1);
        if (bt_has_next(T, i)) cap_acc_rw(E + bt_block(g.ge, c, i), lde, n, n);
      }
    cap_acc_w(info, 0, batch, 1, 0, 4);
    if (logdet) cap_acc_w(logdet, 0, batch, 1);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { hipLaunchKernelGGL(blocktri_potrf_kernel<NP()>, dim3((unsigned)nwg), dim3(64), 0, s, g); });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_dpotrs_blocktri_batched(int uplo, int half, int64_t n, int64_t T, int64_t nrhs, const double* D, int64_t ldd, int64_t step_d, int64_t stride_d,
                                const double* E, int64_t lde, int64_t step_e, int64_t stride_e, double* B, int64_t ldb, int64_t stride_b,
                                const int* info, int64_t batch, void* stream) {
  if (n < 0 || T < 0 || nrhs < 0 || batch < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && T > 0 && nrhs > 0 && batch > 0;
  if (work && (!D || !B || (!E && T > 1))) return CAP_ERR_ARG;
  if (!bt_operand_ok(n, T, ldd, step_d, stride_d, batch) || !bt_operand_ok(n, T - 1, lde, step_e, stride_e, batch)) return CAP_ERR_ARG;
  if ((__int128)ldb < (__int128)T * n || (batch > 1 && (__int128)stride_b < (__int128)ldb * nrhs)) return CAP_ERR_ARG;
  if (half < 0 || half > 2) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bt_limits(uplo, n, T, batch, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  BtSolveArgs g = {};
  g.D = D; g.E = E; g.B = B; g.ldb = ldb; g.stride_b = stride_b; g.nrhs = nrhs; g.info = info; g.half = half;
  bt_geo(g.gd, n, T, batch, ldd, step_d, stride_d);
  bt_geo(g.ge, n, T, batch, lde, step_e, stride_e);
  if (cap_acc_on()) {
    for (int64_t c = 0; c < batch; c++) {
      for (int64_t i = 0; i < T; i++) {
        cap_acc_r(D + bt_block(g.gd, c, i), ldd, n, n, 1);
        if (bt_has_next(T, i)) cap_acc_r(E + bt_block(g.ge, c, i), lde, n, n);
      }
      cap_acc_rw(B + c * stride_b, ldb, T * n, nrhs);
    }
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { hipLaunchKernelGGL(blocktri_potrs_kernel<NP()>, dim3((unsigned)nwg), dim3(64), 0, s, g); });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

}  // extern "C"
