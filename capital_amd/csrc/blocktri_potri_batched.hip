// Batched BLOCK-TRIDIAGONAL SELECTED INVERSE (cap_dpotri_blocktri_batched): the marginal covariances of `batch` independent chains from the
// factors cap_dpotrf_blocktri_batched left - A = R^T R, R block upper bidiagonal with U_i (upper triangular, in the upper triangle of D_i)
// on its diagonal and W_i = R[i, i + 1] in E_i, T blocks of n x n, 1 <= n <= 64.  With Sigma = A^-1 and G_i = U_i^-1 W_i, positions DESCENDING:
//   P_i = U_i^-1 U_i^-T;   Sigma_(T-1,T-1) = P_(T-1);   C_i = Sigma_(i,i+1) = -G_i Sigma_(i+1,i+1);   Sigma_(i,i) = P_i - C_i G_i^T
// (R Sigma = R^-T is block lower triangular).  In place: the upper triangle of D_i <- that of Sigma_(i,i), E_i <- C_i; fill = 1 makes the
// strictly lower triangle of every D block the bit-identical mirror, copied and never computed.  Read row-major (torch) the same memory
// holds Sigma[block i, block i] in the lower triangle of D[c, i] and Sigma[block i + 1, block i] in E[c, i]: the block-tridiagonal part of
// the inverse.  A chain with info != 0 gets NaN wherever the call writes; a zero on a diagonal is not detected (as cap_dtrtri_batched).
// ONE launch per call on a 1-D grid; a workgroup is one wavefront that carries G = 64 / NP chains (NP = 8 / 16 / 32 / 64 >= n) in lane
// groups of NP lanes and walks their positions T - 1 .. 0 in a loop.  No scratch, no allocation, no memset, no atomics, no mutex, no helper
// stream, nothing between workgroups (the __syncthreads are the order of the wavefront's own LDS accesses); 64-bit offsets.
//
// THE ARITHMETIC IS A COMPOSITION of what the family states, and that is the bit contract: a chain's D and E are, bit for bit, what the
// fixed-size entries give when the host drives the recurrence on the chain's blocks, positions descending:
//   1. cap_dtrsm_batched(CAP_NOTRANS) with U_i and the chain's info on the n columns of E_i -> G_i (pb_backward_step, batched_small.h: the same
//      function; NaN for a failed chain);
//   2. cap_dpotri_batched(fill = 1) on U_i -> P_i (pi_invert, pi_product_rows, batched_inverse.h: the same functions);
//   3. cap_dgemm_batched(CAP_NOTRANS, CAP_NOTRANS, alpha = -1, beta = 0) of G_i and the MIRRORED Sigma_(i+1,i+1) -> C_i: every element its own
//      chain on the fp64 16 x 16 x 4 MFMA from a ZERO accumulator, K ascending, four per instruction, rows at or beyond n as +0.0, t = alpha s;
//   4. cap_dgemm_batched(CAP_NOTRANS, CAP_TRANS, alpha = -1, beta = 1) of C_i and G_i into P_i: out = fma(beta, p, t), uncontracted.  ONLY THE
//      UPPER TRIANGLE of that result is Sigma_(i,i) (the two triangles of the product differ in rounding); the operand of position i - 1 is
//      the mirror of that triangle.
// A chain's bits therefore depend on (n, T, its data) alone - not on batch, the chain's index, leading dimensions, steps, strides, the
// chains that share its wavefront or fill (the family's ELEMENT INDEPENDENCE: gemm_batched.hip).  A failed chain: G_i is NaN, the products
// carry it into every C_i, the store of D writes NaN; no other chain is touched.
//
// HOW THE BLOCKS TRAVEL.  D and E go once in and once out.  U_i goes to the PbImg LDS image of its lane group; lane c runs the backward
// substitution on column c of W_i in registers against it and writes its column of G_i into exchange area X1; the image then turns into
// P_i (inverse, then product, as potri_batched.hip).  Sigma_(i+1,i+1) lives in exchange area X2 as a FULL mirrored block and never travels
// through global memory: the first product reads G_i and it from LDS, C_i goes from the accumulators to E_i and takes the place of
// Sigma_(i+1,i+1) in X2 (its readers are done), the second product reads C_i and G_i, the epilogue combines it with P_i from the image, and
// the upper triangle of Sigma_(i,i) and its mirror replace C_i in X2, from where the lanes store D_i (row r of the mirrored block is
// column r: a coalesced store for either value of fill).  Both areas start as +0.0 and are only ever written at rows and columns below n.
// Where the registers allow it the blocks of position i - 1 are requested early: column c of E_(i-1) in front of the inverse and the
// products of position i (NP < 64), row r of U_(i-1) in front of the whole position (NP <= 32).
// LDS: the image + two exchange areas = 11.0 / 21.5 / 42.5 / 84.5 KiB at NP = 8 / 16 / 32 / 64, dynamic; NP = 64 lies above the 64 KiB a
// kernel gets by default and asks for its size with hipFuncSetAttribute (as symv.hip, potrs.hip): ONE wavefront per CU there (160 KiB
// hold one such workgroup), three at NP = 32 - a long sequential chain per wavefront is latency bound, and n = 64 is the weak corner as it
// is for the factor.  Few long chains leave the chip idle (cyclic reduction changes the arithmetic: out of scope).
//
// EVERY ADDRESS AND PREDICATE is a function of blocktri_addr.h, swept lane by lane on the CPU (tests/test_blocktri_potri_addr.py): position
// 0 has no predecessor, position T - 1 no coupling block, T = 1 no E at all.
#include <math.h>

#include <utility>

#include "batched_inverse.h"
#include "batched_small.h"
#include "blocktri_addr.h"
#include "capital_amd.h"
#include "common.h"
#include "vbatch_plan.h"

namespace {

struct BpArgs {
  double* D; double* E;
  BtGeo gd, ge;
  const int* info;
  int fill;
};

template <int NP>
constexpr bool bp_img_agrees() {
  return PbImg<NP>::SIZE == bt_img_size(NP) && PbImg<NP>::LD == bt_img_ld(NP) && PiImg<NP>::SIZE == bt_img_size(NP) && PiImg<NP>::LD == bt_img_ld(NP);
}

template <int NP>
constexpr int64_t bp_lds_bytes() { return 8 * ((int64_t)(64 / NP) * bt_img_size(NP) + 2 * bt_x_size(NP)); }

// the epilogues of gemm_batched.hip without contraction: t = alpha s with alpha = -1 (beta = 0: out = t), out = fma(beta, p, t) with beta = 1
__device__ __forceinline__ double bp_neg(const double s) {
#pragma clang fp contract(off)
  return -1.0 * s;
}
__device__ __forceinline__ double bp_minus(const double p, const double s) {
#pragma clang fp contract(off)
  const double t = -1.0 * s;
  return __builtin_fma(1.0, p, t);
}

// NP = 64 takes the parameter-pack form of the steps (see batched_small.h)
template <int NP, int... J>
__device__ __forceinline__ void bp_backward_pack(double (&x)[NP], const double* s, int n, std::integer_sequence<int, J...>) {
  (pb_backward_step<NP>(x, s, n, NP - 1 - J), ...);
}
template <int NP>
__device__ __forceinline__ void bp_backward(double (&x)[NP], const double* s, int n) {
  if constexpr (NP < 64) {
#pragma unroll
    for (int j = NP - 1; j >= 0; j--) pb_backward_step<NP>(x, s, n, j);
  } else {
    bp_backward_pack<NP>(x, s, n, std::make_integer_sequence<int, NP>{});
  }
}

// the upper triangle of diagonal block `pos` -> the group's image
template <int NP>
__device__ __forceinline__ void bp_load_tri(const double* D, const BtGeo& gd, const int64_t wg, const int lane, const int64_t pos, double* s) {
  const int r = bt_idx(NP, lane);
#pragma unroll 8
  for (int cc = 0; cc < gd.n; cc++) {
    const BtAt at = bt_tri_at(gd, wg, lane, pos, cc);
    if (at.on) s[bt_img_at(NP, r, cc)] = D[at.off];
  }
}

// column lane % NP of coupling block `pos` -> registers (+0.0 where the lane has none)
template <int NP>
__device__ __forceinline__ void bp_load_ecol(const double* E, const BtGeo& ge, const int64_t wg, const int lane, const int64_t pos, double (&x)[NP]) {
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

// acc += (the block at line k, word w of area `a`) (the block of area `b`): gemm_batched.hip's recurrence with both operands in LDS - lane l
// supplies a(row l % 16 of slab si, k) and b(k, column l % 16 of slab sj), k = q + l / 16
template <int NP, bool UPPER>
__device__ __forceinline__ void bp_product(const double* a, const double* b, const int n, const int lane, d4 (&acc)[4][4]) {
  for (int q0 = 0; q0 < n; q0 += 16) {
    double av[4][4], bv[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int sl = 0; sl < 4; sl++) {
        double ta = 0.0, tb = 0.0;
        if (q0 + 4 * u < n && bt_slab_on(NP, sl, n)) {
          const BtAt at = bt_x_slab(n, lane, sl, q0 + 4 * u);
          if (at.on) { ta = a[at.off]; tb = b[at.off]; }
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
            if (bt_tile(NP, si, sj, UPPER)) {
              if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n))
                acc[si][sj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[u][sj], av[u][si], acc[si][sj], 0, 0, 0);
            }
      }
    }
  }
}

__device__ __forceinline__ void bp_zero(d4 (&acc)[4][4]) {
#pragma unroll
  for (int si = 0; si < 4; si++)
#pragma unroll
    for (int sj = 0; sj < 4; sj++) acc[si][sj] = (d4){0.0, 0.0, 0.0, 0.0};
}

template <int NP>
__global__ __launch_bounds__(64) void blocktri_potri_kernel(BpArgs g) {
  constexpr int G = 64 / NP;
  constexpr bool EARLY = NP < 64;        // column c of W_(pos-1) is requested in front of the inverse and the products of position pos,
  constexpr bool EARLY_U = NP <= 32;     // row c of U_(pos-1) in front of the whole position - where the registers allow it
  using Img = PiImg<NP>;
  static_assert(bp_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h and batched_inverse.h");
  extern __shared__ __attribute__((aligned(16))) double bp_lds[];
  double* s_img = bp_lds;                          // G images: U_i, then P_i
  double* s_g = s_img + G * bt_img_size(NP);       // X1: G_i
  double* s_sig = s_g + bt_x_size(NP);             // X2: Sigma_(i+1,i+1) mirrored, then C_i, then Sigma_(i,i) mirrored
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane0 = threadIdx.x, n = gd.n;
  const int64_t wg = blockIdx.x, T = gd.T;
  const BtAt ia = bt_info_at(gd, wg, lane0);
  bool bad = false;
  if (g.info) { if (ia.on) bad = g.info[ia.off] != 0; }

  for (int j = 0; j < bt_x_clear_passes(NP); j++) {
    const BtAt at = bt_x_clear(NP, lane0, j);
    if (at.on) s_g[at.off] = 0.0;
  }
  bp_load_tri<NP>(g.D, gd, wg, lane0, bt_walk_pos(T, 0), s_img + bt_img_base(NP, lane0));
  __syncthreads();

  double xe[EARLY ? NP : 1];            // EARLY: column c of W_(pos-1), requested one position ahead (off at position -1: T = 1)
  if constexpr (EARLY) bp_load_ecol<NP>(g.E, ge, wg, lane0, bt_walk_pos(T, 0) - 1, xe);

  for (int64_t step = 0; step < T; step++) {
    const int64_t pos = bt_walk_pos(T, step);
    const bool first = step == 0;        // wave-uniform: position T - 1 has no coupling block, Sigma = P
    // The lane behind an opaque zero: every offset, LDS address and lane predicate of a position is formed at that position.  Without it
    // the compiler keeps them all in registers across the walk (the tile store of C alone has 64 offsets per lane) and NP = 64 spills.
    const int lane = lane0 + pi_opaque_zero(), c = bt_idx(NP, lane);
    double* s = s_img + bt_img_base(NP, lane);
    double un[EARLY_U ? NP : 1];
    if constexpr (EARLY_U) {             // row c of U_(pos-1), off at position -1
#pragma unroll
      for (int cc = 0; cc < NP; cc++) {
        double t = 0.0;
        if (cc < n) {
          const BtAt at = bt_tri_at(gd, wg, lane, pos - 1, cc);
          if (at.on) t = g.D[at.off];
        }
        un[cc] = t;
      }
    }

    if (!first) {                        // G = U^-1 W, column c in lane c; NaN for a failed chain, as cap_dtrsm_batched with its info
      double x[NP];
      if constexpr (EARLY) {
#pragma unroll
        for (int i = 0; i < NP; i++) x[i] = xe[i];
      } else {
        bp_load_ecol<NP>(g.E, ge, wg, lane, pos, x);
      }
      bp_backward<NP>(x, s, n);
#pragma unroll
      for (int i = 0; i < NP; i++)
        if (i < n && c < n) s_g[bt_xt_own(NP, i, lane)] = bad ? (double)NAN : x[i];
      if constexpr (EARLY) bp_load_ecol<NP>(g.E, ge, wg, lane, pos - 1, xe);     // off at position -1
    }
    __builtin_amdgcn_sched_barrier(0);   // the substitution and the inverse both only read the image: keep their columns apart in the registers

    // P = U^-1 U^-T in the image: the steps of potri_batched_kernel
    {
      double w[NP];
      pi_invert<NP>(w, s, c, n);
      __syncthreads();                   // every lane is through with U: the image takes its inverse
      pi_put_column<NP>(w, s, c, n);
    }
    __syncthreads();
    {
      double w[NP];
#pragma unroll
      for (int k = 0; k < NP; k++) {
        const double v = s[Img::at(c < k ? c : k, k)];
        w[k] = k >= c ? v : 0.0;
      }
      __syncthreads();
      if constexpr (NP < 64) {
#pragma unroll
        for (int i = 0; i < NP; i++) pi_product_row<NP>(w, s, c, n, i);
      } else {
        pi_product_rows<NP>(w, s, c, n, std::make_integer_sequence<int, NP>{});
      }
    }
    __syncthreads();                     // P is in the image, G in X1

    d4 acc[4][4];
    bp_zero(acc);
    if (!first) {
      bp_product<NP, false>(s_g, s_sig, n, lane, acc);       // G Sigma_(pos+1,pos+1)
      __syncthreads();                   // every lane has read Sigma_(pos+1,pos+1): C takes its place
#pragma unroll
      for (int si = 0; si < 4; si++)
#pragma unroll
        for (int sj = 0; sj < 4; sj++)
          if (bt_tile(NP, si, sj, false)) {
            if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
#pragma unroll
              for (int r = 0; r < 4; r++) {
                const double t = bp_neg(acc[si][sj][r]);
                const BtAt at = bt_etile_at(ge, wg, lane, pos, si, sj, r);
                if (at.on) g.E[at.off] = t;
                const BtAt xt = bt_xt_tile(n, NP, lane, si, sj, r);
                if (xt.on) s_sig[xt.off] = t;
              }
            }
          }
      __syncthreads();
      bp_zero(acc);
      bp_product<NP, true>(s_sig, s_g, n, lane, acc);        // C G^T, the upper tiles
    }
    // Sigma_(pos,pos) = P - C G^T, the upper triangle
#pragma unroll
    for (int si = 0; si < 4; si++)
#pragma unroll
      for (int sj = 0; sj < 4; sj++)
        if (bt_tile(NP, si, sj, true)) {
          if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const BtAt at = bt_img_tile(n, NP, lane, si, sj, r);
              if (at.on) {
                const double p = s_img[at.off];
                acc[si][sj][r] = first ? p : bp_minus(p, acc[si][sj][r]);
              }
            }
          }
        }
    __syncthreads();                     // every lane has read C: the mirrored Sigma_(pos,pos) takes its place
#pragma unroll
    for (int si = 0; si < 4; si++)
#pragma unroll
      for (int sj = 0; sj < 4; sj++)
        if (bt_tile(NP, si, sj, true)) {
          if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const BtAt up = bt_sig_tile(n, NP, lane, si, sj, r, false);
              if (up.on) s_sig[up.off] = acc[si][sj][r];
              const BtAt lo = bt_sig_tile(n, NP, lane, si, sj, r, true);
              if (lo.on) s_sig[lo.off] = acc[si][sj][r];
            }
          }
        }
    __syncthreads();
#pragma unroll 8
    for (int cc = 0; cc < n; cc++) {     // row c of the mirrored block is column c: the triangle, or the whole block with fill
      const BtAt at = bt_full_at(gd, wg, lane, pos, cc, g.fill);
      if (at.on) g.D[at.off] = bad ? (double)NAN : s_sig[bt_x_own(cc, lane)];
    }
    if (!bt_has_prev(pos)) break;        // wave-uniform: position 0 has no predecessor

    if constexpr (EARLY_U) {
#pragma unroll
      for (int cc = 0; cc < NP; cc++)
        if (c <= cc && cc < n) s[bt_img_at(NP, c, cc)] = un[cc];
    } else {
      bp_load_tri<NP>(g.D, gd, wg, lane, pos - 1, s);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ host
// the operand rule and the limits of blocktri_batched.hip (its rules 3 and 5 - 8), restated: that file's text stays as it is
static inline bool bp_operand_ok(int64_t n, int64_t blocks, int64_t ld, int64_t step, int64_t stride, int64_t batch) {
  if (blocks <= 0) return true;          // E with T <= 1: nothing is stored
  if (ld < n) return false;
  const __int128 blk = (__int128)ld * n;
  if (blocks > 1 && (__int128)step < blk) return false;
  if (batch > 1 && (__int128)stride < (blocks > 1 ? (__int128)step * blocks : blk)) return false;
  return true;
}

static void bp_geo(BtGeo& g, int64_t n, int64_t T, int64_t batch, int64_t ld, int64_t step, int64_t stride) {
  g.ld = ld; g.step = step; g.stride = stride; g.T = T; g.batch = batch; g.n = (int)n; g.NP = vb_padded(n);
}

template <int NP>
int bp_launch(const BpArgs& g, int64_t nwg, hipStream_t s) {
  constexpr int BYTES = (int)bp_lds_bytes<NP>();
  if constexpr (BYTES > 64 * 1024) {
    static bool attr_set[16] = {};
    int dev = 0;
    CAP_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16 || !attr_set[dev]) {
      CAP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(blocktri_potri_kernel<NP>), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES));
      if (dev >= 0 && dev < 16) attr_set[dev] = true;
    }
  }
  hipLaunchKernelGGL(blocktri_potri_kernel<NP>, dim3((unsigned)nwg), dim3(64), BYTES, s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

}  // namespace

extern "C" {

int cap_dpotri_blocktri_batched(int uplo, int fill, int64_t n, int64_t T, double* D, int64_t ldd, int64_t step_d, int64_t stride_d, double* E, int64_t lde,
                                int64_t step_e, int64_t stride_e, const int* info, int64_t batch, void* stream) {
  if (n < 0 || T < 0 || batch < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && T > 0 && batch > 0;
  if (work && (!D || (!E && T > 1))) return CAP_ERR_ARG;
  if (!bp_operand_ok(n, T, ldd, step_d, stride_d, batch) || !bp_operand_ok(n, T - 1, lde, step_e, stride_e, batch)) return CAP_ERR_ARG;
  if (fill != 0 && fill != 1) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;       // as the other batched entries
  if (n > BT_MAX) return CAP_ERR_UNSUPPORTED;
  if ((__int128)T * n > (__int128)0x7fffffffLL) return CAP_ERR_UNSUPPORTED;
  const int64_t nwg = vb_grid(batch, 64 / vb_padded(n));
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  if (!work) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  BpArgs g = {};
  g.D = D; g.E = E; g.info = info; g.fill = fill;
  bp_geo(g.gd, n, T, batch, ldd, step_d, stride_d);
  bp_geo(g.ge, n, T, batch, lde, step_e, stride_e);
  if (cap_acc_on()) {
    for (int64_t c = 0; c < batch; c++)
      for (int64_t i = 0; i < T; i++) {
        cap_acc_rw(D + bt_block(g.gd, c, i), ldd, n, n, fill ? 0 : 1);      // as cap_dpotri_batched notes its block
        if (bt_has_next(T, i)) cap_acc_rw(E + bt_block(g.ge, c, i), lde, n, n);
      }
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
  }
  int st = CAP_OK;
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bp_launch<NP()>(g, nwg, s); });
  return st;
}

}  // extern "C"
