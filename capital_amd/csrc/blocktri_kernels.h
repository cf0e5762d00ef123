// The block-tridiagonal family's ONE body per operation - factor, solve, selected inverse - and the host rules its entries share.
// blocktri_batched.hip, blocktri_potri_batched.hip (fixed size) and blocktri_vbatched.hip (ragged chains on a plan) hold the extern "C"
// entries and a __global__ wrapper per kernel; a wrapper names the LOOKUP and calls the body here.  The lookup answers "which chain does
// this lane group carry, and how many steps does the wavefront walk" and nothing else:
//   BtFixed  chain wg G + group of `batch` chains of T positions, by arithmetic (bt_chain_fixed); no table; the walk is the launch's T;
//   BtPlan   place wg G + group of the plan's list sorted by T descending -> the chain's record (bt_chain_plan); the G chains of the
//            wavefront sit in a 320-byte LDS table (lane 0 of every group writes its entry once), the walk is the largest T of the groups.
// Everything below the lookup is one text: step-indexed walks over the ADDRESSED chain of blocktri_addr.h, ONE activity rule (a chain is
// active while step < its T, ascending at position `step`, descending at its own T - 1 - step), every address and predicate a function
// of that header.  With all lengths equal this is the plain walk over T positions; a dead lane group is a chain of T = 0.
//
// WHO IS ALIVE AT A STEP.  All chains start at step 0 - descending walks at their own last position (right-hand side loaded, Sigma = P
// without a coupling term) - so there is no joining in the middle of a loop; the price is that a descending position is a lane value,
// which only address arithmetic sees.  A chain that has ended leaves stale numbers (possibly NaN) in its image, its columns and its
// exchange lines, and the steps and products still run over them for the neighbours' sake; SELECTION keeps them in: every store, every
// prefetch and the sums into info / logdet carry the activity predicate, an ended chain's E columns enter the exchange area as +0.0, and
// the areas' "rows at or beyond n are +0.0" holds for every group since n is the call's.  A chain's tiles exist only inside its own lane
// group (bt_tile, and the group test of every tile accessor), so no number of one chain meets a number of another: a chain's bits depend
// on (n, T, its data) alone, and the ragged entries give every chain what the fixed-size entry gives it alone.
//
// THE ARITHMETIC is the family's, statement by statement: pb_factor_step, pb_forward_step, pb_backward_step (batched_small.h), pi_invert,
// pi_put_column, pi_product_row (batched_inverse.h), the fp64 16 x 16 x 4 MFMA recurrence from a ZERO accumulator, K ascending, rows at
// or beyond n as +0.0, and the uncontracted epilogues t = alpha s, out = fma(beta, c, t).
#pragma once
#include <math.h>

#include <utility>

#include "batched_inverse.h"
#include "batched_small.h"
#include "blocktri_addr.h"
#include "capital_amd.h"
#include "common.h"
#include "vbatch_plan.h"

struct BtRec {                         // one chain of a plan, in batch order
  int64_t first, T, row;
};

namespace {

// a wave-uniform 64-bit value in scalar registers
__device__ __forceinline__ int64_t bt_uniform(const int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)(uint64_t)v), hi = __builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ------------------------------------------------------------------------------------------------ the two lookups
// own<NP>: the lane's own chain and the wavefront's steps (fills the table where there is one); of<NP>: the chain of a lane group
struct BtFixed {
  static constexpr bool TABLE = false;
  int64_t stride_b;                    // the solve's: chains of right-hand sides `stride_b` apart
  template <int NP>
  __device__ __forceinline__ BtChain own(const BtGeo& gd, const BtGeo& ge, int64_t*, int64_t& steps) const {
    steps = gd.T;
    BtChain ch = bt_chain_fixed(gd, ge, stride_b, blockIdx.x, bt_group(NP, threadIdx.x));
    if constexpr (NP == 64) {          // one group: the chain is the wave's (as BtPlan hands it over)
      ch.d = bt_uniform(ch.d); ch.e = bt_uniform(ch.e); ch.b = bt_uniform(ch.b); ch.T = bt_uniform(ch.T); ch.id = bt_uniform(ch.id);
    }
    return ch;
  }
  template <int NP>
  __device__ __forceinline__ BtChain of(const BtGeo& gd, const BtGeo& ge, const int64_t*, const int group) const {
    return bt_chain_fixed(gd, ge, stride_b, blockIdx.x, group);
  }
};

struct BtPlan {
  static constexpr bool TABLE = true;
  const BtRec* rec; const int64_t* order; int64_t count;
  template <int NP>
  __device__ __forceinline__ BtChain own(const BtGeo& gd, const BtGeo& ge, int64_t* tab, int64_t& steps) const {
    const int lane = threadIdx.x;
    const int64_t at = bt_chain(NP, blockIdx.x, lane);
    BtChain ch = bt_chain_plan(gd, ge, 0, 0, 0, 0);          // a group beyond the list
    if (at < count) {
      const int64_t id = order[at];
      const BtRec r = rec[id];
      ch = bt_chain_plan(gd, ge, r.first, r.T, r.row, id);
    }
    if (bt_idx(NP, lane) == 0) {
      const int grp = bt_group(NP, lane);
      tab[bt_tab_at(grp, 0)] = ch.d;
      tab[bt_tab_at(grp, 1)] = ch.e;
      tab[bt_tab_at(grp, 2)] = ch.b;
      tab[bt_tab_at(grp, 3)] = ch.T;
      tab[bt_tab_at(grp, 4)] = ch.id;
    }
    steps = vb_wave_max((int)ch.T);    // n T <= 2^31 - 1 (the entries refuse more)
    __syncthreads();
    if constexpr (NP == 64) {          // one group: the record is the wave's
      ch.d = bt_uniform(ch.d); ch.e = bt_uniform(ch.e); ch.b = bt_uniform(ch.b); ch.T = bt_uniform(ch.T); ch.id = bt_uniform(ch.id);
    }
    return ch;
  }
  template <int NP>
  __device__ __forceinline__ BtChain of(const BtGeo&, const BtGeo&, const int64_t* tab, const int group) const {
    BtChain ch;
    ch.d = tab[bt_tab_at(group, 0)];
    ch.e = tab[bt_tab_at(group, 1)];
    ch.b = tab[bt_tab_at(group, 2)];
    ch.T = tab[bt_tab_at(group, 3)];
    ch.id = tab[bt_tab_at(group, 4)];
    return ch;
  }
};

// the chain of the lane's wave row in slab s; NP = 64 has one group - the lane's own chain, in scalar registers
template <int NP, class L>
__device__ __forceinline__ BtChain bt_row_chain(const L& lk, const BtGeo& gd, const BtGeo& ge, const int64_t* tab, const BtChain& own, const int lane,
                                                const int s) {
  if constexpr (NP == 64) return own;
  else return lk.template of<NP>(gd, ge, tab, bt_row_group(NP, lane, s));
}

template <class L>
struct BtArgs {                        // factor and inverse
  double* D; double* E;
  BtGeo gd, ge;
  L lk;
  int* info; double* logdet;           // the inverse reads info and has no logdet
  int fill;
};

template <class L>
struct BtSolveArgs {
  const double* D; const double* E;
  BtGeo gd, ge;
  L lk;
  double* B; int64_t ldb, nrhs;
  const int* info;
  int half;
};

template <int NP>
constexpr bool bt_img_agrees() {
  return PbImg<NP>::SIZE == bt_img_size(NP) && PbImg<NP>::LD == bt_img_ld(NP) && PiImg<NP>::SIZE == bt_img_size(NP) && PiImg<NP>::LD == bt_img_ld(NP);
}

// ------------------------------------------------------------------------------------------------ device helpers
// the epilogues of syrk_batched.hip / gemm_batched.hip without contraction: t = alpha s with alpha = -1; out = t, or out = fma(beta, c, t) with beta = 1
__device__ __forceinline__ double bt_neg(const double s) {
#pragma clang fp contract(off)
  return -1.0 * s;
}
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

// the upper triangle of diagonal block `pos` of the lane's chain -> the group's image (pb_load_upper's walk on the addresses of blocktri_addr.h)
template <int NP>
__device__ __forceinline__ void bt_load_tri(const double* D, const BtGeo& gd, const BtChain& own, const int lane, const int64_t pos, double* s) {
  const int r = bt_idx(NP, lane);
#pragma unroll 8
  for (int cc = 0; cc < gd.n; cc++) {
    const BtAt at = bt_tri_at(gd, own, lane, pos, cc);
    if (at.on) s[bt_img_at(NP, r, cc)] = D[at.off];
  }
}

// column lane % NP of coupling block `pos` -> registers (+0.0 where the lane has none)
template <int NP>
__device__ __forceinline__ void bt_load_ecol(const double* E, const BtGeo& ge, const BtChain& own, const int lane, const int64_t pos, double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    double t = 0.0;
    if (i < ge.n) {
      const BtAt at = bt_ecol_at(ge, own, lane, pos, i);
      if (at.on) t = E[at.off];
    }
    x[i] = t;
  }
}

template <int NP, class L>
__device__ __forceinline__ void bt_rhs_load(const BtSolveArgs<L>& g, const BtGeo& gd, const BtChain& own, const int lane, const int64_t pass,
                                            const int64_t pos, double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    double t = 0.0;
    if (i < gd.n) {
      const BtAt at = bt_rhs_at(gd, own, g.ldb, g.nrhs, lane, pass, pos, i);
      if (at.on) t = g.B[at.off];
    }
    x[i] = t;
  }
}

template <int NP, class L>
__device__ __forceinline__ void bt_rhs_store(const BtSolveArgs<L>& g, const BtGeo& gd, const BtChain& own, const int lane, const int64_t pass,
                                             const int64_t pos, const bool bad, const double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    if (i < gd.n) {
      const BtAt at = bt_rhs_at(gd, own, g.ldb, g.nrhs, lane, pass, pos, i);
      if (at.on) g.B[at.off] = bad ? (double)NAN : x[i];
    }
  }
}

__device__ __forceinline__ void bt_zero(d4 (&acc)[4][4]) {
#pragma unroll
  for (int si = 0; si < 4; si++)
#pragma unroll
    for (int sj = 0; sj < 4; sj++) acc[si][sj] = (d4){0.0, 0.0, 0.0, 0.0};
}

// acc += (the block at line k, word w of area `a`) (the block of area `b`): gemm_batched.hip's recurrence with both operands in LDS - lane l
// supplies a(row l % 16 of slab si, k) and b(k, column l % 16 of slab sj), k = q + l / 16
template <int NP, bool UPPER>
__device__ __forceinline__ void bt_product(const double* a, const double* b, const int n, const int lane, d4 (&acc)[4][4]) {
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

// ------------------------------------------------------------------------------------------------ factor
// Position i ascending: S_i lives in the PbImg LDS image of its lane group and never in global memory.  The factor steps turn the image
// into U_i (stored to D_i once), lane c runs the forward substitution on column c of E_i in registers against it (W_i, stored to E_i
// once), the columns go to the exchange area, the MFMA reads both operands from there, and the epilogue combines W_i^T W_i with D_(i+1) -
// read from global memory once, in the accumulator layout, BEFORE the factor steps of position i start, as is E_i where the registers
// allow it (EARLY) - and writes S_(i+1) into the image.
template <int NP, class L>
__device__ __forceinline__ void bt_factor(const BtArgs<L>& g) {
  constexpr int G = 64 / NP;
  constexpr bool EARLY = NP < 64;
  using Img = PbImg<NP>;
  static_assert(bt_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h and batched_inverse.h");
  __shared__ double s_img[G * Img::SIZE];
  __shared__ double s_x[bt_x_size(NP)];
  __shared__ double s_log[64];
  __shared__ int64_t s_tab[L::TABLE ? bt_tab_size() : 1];
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane0 = threadIdx.x, n = gd.n;
  int64_t Tw;
  const BtChain own = g.lk.template own<NP>(gd, ge, s_tab, Tw);

  bt_load_tri<NP>(g.D, gd, own, lane0, 0, s_img + bt_img_base(NP, lane0));
  __syncthreads();
  int cinfo = 0;
  double ldsum = 0.0;

  for (int64_t pos = 0; pos < Tw; pos++) {
    // NP = 64 on a plan: the lane behind an opaque zero, as the inverse has it - the offsets of a position are formed at that position
    // instead of all being kept in registers across the walk, which spills there; the fixed-size walk fits without (and loses 4 % with it)
    const int lane = NP == 64 && L::TABLE ? lane0 + pi_opaque_zero() : lane0, c = bt_idx(NP, lane);
    double* s = s_img + bt_img_base(NP, lane);
    const bool active = bt_active(own, pos);
    // what position pos + 1 needs from memory, requested before the steps of this one: column c of E_pos, D_(pos+1) in the accumulator layout
    double x[NP];
    if constexpr (EARLY) bt_load_ecol<NP>(g.E, ge, own, lane, pos, x);
    double dn[4][4][4];
#pragma unroll
    for (int si = 0; si < 4; si++) {
      const BtChain chr = bt_row_chain<NP>(g.lk, gd, ge, s_tab, own, lane, si);
#pragma unroll
      for (int sj = 0; sj < 4; sj++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double t = 0.0;
          if (bt_tile(NP, si, sj, true)) {
            if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
              const BtAt at = bt_next_at(gd, chr, lane, pos, si, sj, r);
              if (at.on) t = g.D[at.off];
            }
          }
          dn[si][sj][r] = t;
        }
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
      const BtAt at = bt_tri_at(gd, own, lane, pos, cc);
      if (at.on) g.D[at.off] = s[bt_img_at(NP, c, cc)];
    }
    if (active && info != 0 && cinfo == 0) cinfo = (int)(pos * n) + info;
    if (g.logdet) {                      // potrf_batched_kernel's: lane j takes the logarithm, lane 0 of the group adds them in ascending j
      s_log[bt_log_at(NP, lane, c)] = c < n ? log(s[Img::at(c, c)]) : 0.0;
      __syncthreads();
      if (c == 0 && active) {            // an ended chain's image is stale: its sum stands
        double t = 0.0;
        for (int j = 0; j < n; j++) t += s_log[bt_log_at(NP, lane, j)];
        ldsum += bad ? (double)NAN : 2.0 * t;
      }
    }
    if (!bt_has_next(Tw, pos)) break;    // wave-uniform: no chain of the wave has a successor

    // W = U^-T B, column c in lane c; NaN behind a failed factor, as cap_dtrsm_batched with its info
    if constexpr (!EARLY) bt_load_ecol<NP>(g.E, ge, own, lane, pos, x);
    bt_forward<NP>(x, s, n);
#pragma unroll
    for (int i = 0; i < NP; i++) {
      if (i < n) {
        const double v = bad ? (double)NAN : x[i];
        const BtAt at = bt_ecol_at(ge, own, lane, pos, i);
        if (at.on) g.E[at.off] = v;
        s_x[bt_x_own(i, lane)] = at.on ? v : 0.0;
      }
    }
    __syncthreads();                     // the columns are in the exchange area; nobody reads the image any more

    // W^T W on the MFMA, syrk_batched.hip's tiles: wave row w is column w % NP of the W of group w / NP
    d4 acc[4][4];
    bt_zero(acc);
    bt_product<NP, true>(s_x, s_x, n, lane, acc);
    // S_(pos+1) = D_(pos+1) - W^T W into the image (an ended chain's image takes -(0) + 0: nobody reads it)
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

  const BtAt at = bt_scalar_at(NP, own, lane0);
  if (at.on) {
    g.info[at.off] = cinfo;
    if (g.logdet) g.logdet[at.off] = ldsum;
  }
}

// ------------------------------------------------------------------------------------------------ solve
// x <- c - op(W) x at a step: the column of every lane through the exchange area to the MFMA and back, W straight from global memory as
// gemm_batched.hip reads it (the slab of the columns is the MFMA's A operand).  DESC false - the forward sweep, op(W) = W^T; true - the
// backward sweep.  The coupling block and the target segment c are those of the ADDRESSED chain at this step (bt_couple_epos, bt_couple_tpos)
template <int NP, bool DESC, class L>
__device__ __forceinline__ void bt_couple(const BtSolveArgs<L>& g, const BtGeo& gd, const BtGeo& ge, const BtChain& own, const int64_t* s_tab,
                                          const int lane, const int64_t pass, const int64_t step, double* s_x, double (&x)[NP]) {
  const int n = gd.n;
  constexpr bool EARLY = NP < 64;        // the target segment is requested in front of the product where the registers allow it
  const int64_t tpos = bt_couple_tpos(own, step, DESC);
  double cn[NP];
  if constexpr (EARLY) bt_rhs_load<NP>(g, gd, own, lane, pass, tpos, cn);
#pragma unroll
  for (int i = 0; i < NP; i++)
    if (i < n) s_x[bt_x_own(i, lane)] = x[i];
  __syncthreads();

  bool onc[4];                           // wave-uniform: does column slab s hold a right-hand side of this pass
#pragma unroll
  for (int sl = 0; sl < 4; sl++) onc[sl] = pass * NP + (sl * 16) % NP < g.nrhs;
  int64_t ebase[4], eT[4];               // the chain of the lane's wave row in every slab
#pragma unroll
  for (int sl = 0; sl < 4; sl++) {
    const BtChain chr = bt_row_chain<NP>(g.lk, gd, ge, s_tab, own, lane, sl);
    ebase[sl] = chr.e; eT[sl] = chr.T;
  }
  d4 acc[4][4];
  bt_zero(acc);
  for (int q0 = 0; q0 < n; q0 += 16) {
    double av[4][4], bv[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int sl = 0; sl < 4; sl++) {
        double ta = 0.0, tb = 0.0;
        if (q0 + 4 * u < n) {
          if (bt_slab_on(NP, sl, n)) {
            BtChain chr;
            chr.d = 0; chr.e = ebase[sl]; chr.b = 0; chr.T = eT[sl]; chr.id = 0;
            const BtAt at = bt_eslab_at(ge, chr, lane, bt_couple_epos(chr, step, DESC), sl, q0 + 4 * u, !DESC);
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
  if constexpr (!EARLY) bt_rhs_load<NP>(g, gd, own, lane, pass, tpos, cn);
#pragma unroll
  for (int i = 0; i < NP; i++)
    if (i < n) x[i] = bt_minus(cn[i], s_x[bt_x_own(i, lane)]);
}

// one sweep of a pass: the substitution of every position against the image of U, the coupling product between two positions; the
// right-hand-side column stays in the registers of its lane across the chain
template <int NP, bool DESC, class L>
__device__ __forceinline__ void bt_sweep(const BtSolveArgs<L>& g, const BtGeo& gd, const BtGeo& ge, const BtChain& own, const int64_t* s_tab,
                                         const int lane0, const int64_t pass, const int64_t Tw, const bool bad, double* s, double* s_x) {
  double x[NP];
  bt_rhs_load<NP>(g, gd, own, lane0, pass, bt_pos(own, 0, DESC), x);
  for (int64_t step = 0; step < Tw; step++) {
    const int lane = lane0;
    const int64_t pos = bt_pos(own, step, DESC);
    __syncthreads();                     // the image of the step before is read no more
    bt_load_tri<NP>(g.D, gd, own, lane, pos, s);
    __syncthreads();
    if constexpr (DESC) bt_backward<NP>(x, s, gd.n);
    else bt_forward<NP>(x, s, gd.n);
    bt_rhs_store<NP>(g, gd, own, lane, pass, pos, bad, x);
    if (!bt_has_next(Tw, step)) break;
    bt_couple<NP, DESC>(g, gd, ge, own, s_tab, lane, pass, step, s_x, x);
  }
}

// More than NP right-hand sides are further passes inside the launch (each pass walks the chain again).
template <int NP, class L>
__device__ __forceinline__ void bt_solve(const BtSolveArgs<L>& g) {
  constexpr int G = 64 / NP;
  static_assert(bt_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h and batched_inverse.h");
  __shared__ double s_img[G * PbImg<NP>::SIZE];
  __shared__ double s_x[bt_x_size(NP)];
  __shared__ int64_t s_tab[L::TABLE ? bt_tab_size() : 1];
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane = threadIdx.x;
  int64_t Tw;
  const BtChain own = g.lk.template own<NP>(gd, ge, s_tab, Tw);
  double* s = s_img + bt_img_base(NP, lane);
  const BtAt ia = bt_info_at(own);
  bool bad = false;
  if (g.info) { if (ia.on) bad = g.info[ia.off] != 0; }

  const int64_t passes = bt_rhs_passes(NP, g.nrhs);
  for (int64_t pass = 0; pass < passes; pass++) {
    if (g.half != 2) bt_sweep<NP, false>(g, gd, ge, own, s_tab, lane, pass, Tw, bad, s, s_x);      // R^T y = b, positions ascending
    if (g.half != 1) bt_sweep<NP, true>(g, gd, ge, own, s_tab, lane, pass, Tw, bad, s, s_x);       // R x = y, every chain's own positions descending
  }
}

// ------------------------------------------------------------------------------------------------ selected inverse
// Positions descending.  U_i goes to the image of its lane group; lane c runs the backward substitution on column c of W_i in registers
// against it and writes its column of G_i = U_i^-1 W_i into exchange area X1; the image then turns into P_i = U_i^-1 U_i^-T (inverse, then
// product, as potri_batched.hip).  Sigma_(i+1,i+1) lives in exchange area X2 as a FULL mirrored block and never travels through global
// memory: the first product reads G_i and it from LDS, C_i = -G_i Sigma_(i+1,i+1) goes from the accumulators to E_i and takes the place of
// Sigma_(i+1,i+1) in X2, the second product reads C_i and G_i, the epilogue combines it with P_i from the image (ONLY THE UPPER TRIANGLE
// of P_i - C_i G_i^T is Sigma_(i,i): the two triangles of the product differ in rounding), and that triangle and its mirror replace C_i in
// X2, from where the lanes store D_i (row r of the mirrored block is column r: a coalesced store for either value of fill).  Both areas
// start as +0.0 and are only ever written at rows and columns below n.  Where the registers allow it the blocks of position i - 1 are
// requested early: column c of E_(i-1) in front of the inverse and the products of position i (EARLY), row r of U_(i-1) in front of the
// whole position (EARLY_U).
// LDS, dynamic: the image + two exchange areas (+ the table) = 11.0 / 21.5 / 42.5 / 84.5 KiB at NP = 8 / 16 / 32 / 64; NP = 64 lies above
// the 64 KiB a kernel gets by default (bt_launch asks for it): ONE wavefront per CU there - n = 64 is the weak corner, as for the factor.
template <int NP, class L>
constexpr int64_t bt_inv_lds_bytes() { return 8 * ((int64_t)(64 / NP) * bt_img_size(NP) + 2 * bt_x_size(NP) + (L::TABLE ? bt_tab_size() : 0)); }

template <int NP, class L>
__device__ __forceinline__ void bt_inverse(const BtArgs<L>& g) {
  constexpr int G = 64 / NP;
  constexpr bool EARLY = NP < 64;
  constexpr bool EARLY_U = NP <= 32;
  using Img = PiImg<NP>;
  static_assert(bt_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h and batched_inverse.h");
  extern __shared__ __attribute__((aligned(16))) double bt_lds[];
  double* s_img = bt_lds;                          // G images: U_i, then P_i
  double* s_g = s_img + G * bt_img_size(NP);       // X1: G_i
  double* s_sig = s_g + bt_x_size(NP);             // X2: Sigma_(i+1,i+1) mirrored, then C_i, then Sigma_(i,i) mirrored
  int64_t* s_tab = reinterpret_cast<int64_t*>(s_sig + bt_x_size(NP));      // (not there without a table, and not touched)
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane0 = threadIdx.x, n = gd.n;
  int64_t Tw;
  const BtChain own0 = g.lk.template own<NP>(gd, ge, s_tab, Tw);
  const BtAt ia = bt_info_at(own0);
  bool bad = false;
  if (g.info) { if (ia.on) bad = g.info[ia.off] != 0; }

  for (int j = 0; j < bt_x_clear_passes(NP); j++) {
    const BtAt at = bt_x_clear(NP, lane0, j);
    if (at.on) s_g[at.off] = 0.0;
  }
  bt_load_tri<NP>(g.D, gd, own0, lane0, bt_pos(own0, 0, true), s_img + bt_img_base(NP, lane0));
  __syncthreads();

  double xe[EARLY ? NP : 1];            // EARLY: column c of W_(pos-1), requested one position ahead (off at position -1)
  if constexpr (EARLY) bt_load_ecol<NP>(g.E, ge, own0, lane0, bt_pos(own0, 0, true) - 1, xe);

  for (int64_t step = 0; step < Tw; step++) {
    const bool first = step == 0;        // wave-uniform: every chain starts at its own last position, Sigma = P
    // The lane behind an opaque zero: every offset, LDS address, lane predicate and the chain itself are formed at the step.  Without it
    // the compiler keeps them all in registers across the walk (the tile store of C alone has 64 offsets per lane) and NP = 64 spills.
    const int lane = lane0 + pi_opaque_zero(), c = bt_idx(NP, lane);
    const BtChain own = g.lk.template of<NP>(gd, ge, s_tab, bt_group(NP, lane));
    const int64_t pos = bt_pos(own, step, true);
    double* s = s_img + bt_img_base(NP, lane);
    double un[EARLY_U ? NP : 1];
    if constexpr (EARLY_U) {             // row c of U_(pos-1), off at position -1
#pragma unroll
      for (int cc = 0; cc < NP; cc++) {
        double t = 0.0;
        if (cc < n) {
          const BtAt at = bt_tri_at(gd, own, lane, pos - 1, cc);
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
        bt_load_ecol<NP>(g.E, ge, own, lane, pos, x);
      }
      bt_backward<NP>(x, s, n);
#pragma unroll
      for (int i = 0; i < NP; i++)
        if (i < n && c < n) s_g[bt_xt_own(NP, i, lane)] = bad ? (double)NAN : x[i];
      if constexpr (EARLY) bt_load_ecol<NP>(g.E, ge, own, lane, pos - 1, xe);      // off at position -1
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
    bt_zero(acc);
    if (!first) {
      bt_product<NP, false>(s_g, s_sig, n, lane, acc);       // G Sigma_(pos+1,pos+1)
      __syncthreads();                   // every lane has read Sigma_(pos+1,pos+1): C takes its place
#pragma unroll
      for (int si = 0; si < 4; si++) {
        const BtChain chr = bt_row_chain<NP>(g.lk, gd, ge, s_tab, own, lane, si);
        const int64_t rpos = bt_pos(chr, step, true);
#pragma unroll
        for (int sj = 0; sj < 4; sj++)
          if (bt_tile(NP, si, sj, false)) {
            if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
#pragma unroll
              for (int r = 0; r < 4; r++) {
                const double t = bt_neg(acc[si][sj][r]);
                const BtAt at = bt_etile_at(ge, chr, lane, rpos, si, sj, r);
                if (at.on) g.E[at.off] = t;
                const BtAt xt = bt_xt_tile(n, NP, lane, si, sj, r);
                if (xt.on) s_sig[xt.off] = t;
              }
            }
          }
      }
      __syncthreads();
      bt_zero(acc);
      bt_product<NP, true>(s_sig, s_g, n, lane, acc);        // C G^T, the upper tiles
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
                acc[si][sj][r] = first ? p : bt_minus(p, acc[si][sj][r]);
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
      const BtAt at = bt_full_at(gd, own, lane, pos, cc, g.fill);
      if (at.on) g.D[at.off] = bad ? (double)NAN : s_sig[bt_x_own(cc, lane)];
    }
    if (!bt_has_next(Tw, step)) break;   // wave-uniform: no chain of the wave has a predecessor left

    if constexpr (EARLY_U) {
#pragma unroll
      for (int cc = 0; cc < NP; cc++)
        if (c <= cc && cc < n) s[bt_img_at(NP, c, cc)] = un[cc];
    } else {
      bt_load_tri<NP>(g.D, gd, own, lane, pos - 1, s);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ host
// the rule of a chained operand: `batch` chains of `blocks` column-major n x n blocks, leading dimension ld, `step` apart, chains `stride`
// apart - no two blocks overlap (128-bit products, as vb_operand_ok).  A plan's operand is ONE chain of its slots.
static inline bool bt_operand_ok(int64_t n, int64_t blocks, int64_t ld, int64_t step, int64_t stride, int64_t batch) {
  if (blocks <= 0) return true;          // E with T <= 1: nothing is stored
  if (ld < n) return false;
  const __int128 blk = (__int128)ld * n;
  if (blocks > 1 && (__int128)step < blk) return false;
  if (batch > 1 && (__int128)stride < (blocks > 1 ? (__int128)step * blocks : blk)) return false;
  return true;
}

static inline void bt_geo(BtGeo& g, int64_t n, int64_t T, int64_t batch, int64_t ld, int64_t step, int64_t stride) {
  g.ld = ld; g.step = step; g.stride = stride; g.T = T; g.batch = batch; g.n = (int)n; g.NP = vb_padded(n);
}

// rules 5 - 8 of every entry (T: the longest chain); > 0: the workgroups, 0: refused (st holds the status) or, with st == CAP_OK, nothing to do
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

// chain c of a fixed-size launch, for the host's notes
static inline BtChain bt_host_chain(const BtGeo& gd, const BtGeo& ge, int64_t stride_b, int64_t c) {
  const int G = 64 / gd.NP;
  return bt_chain_fixed(gd, ge, stride_b, c / G, (int)(c % G));
}

// the access notes of one chain's blocks: mode_d / mode_e are CAP_ACC_R or CAP_ACC_RW, tri = 1: the upper triangle of a D block only
static inline void bt_note_chain(const BtGeo& gd, const BtGeo& ge, const BtChain& ch, const double* D, const double* E, int mode_d, int tri, int mode_e) {
  for (int64_t i = 0; i < ch.T; i++) {
    cap_acc(mode_d, D + ch.d + i * gd.step, gd.ld, gd.n, gd.n, tri);
    if (bt_has_next(ch, i)) cap_acc(mode_e, E + ch.e + i * ge.step, ge.ld, ge.n, ge.n);
  }
}

// one launch of KERNEL with BYTES of dynamic LDS; more than the 64 KiB a kernel gets by default is asked for once per device (as
// symv.hip, potrs.hip)
template <auto KERNEL, int BYTES, class Args>
int bt_launch(const Args& g, int64_t nwg, hipStream_t s) {
  if constexpr (BYTES > 64 * 1024) {
    static bool attr_set[16] = {};
    int dev = 0;
    CAP_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16 || !attr_set[dev]) {
      CAP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES));
      if (dev >= 0 && dev < 16) attr_set[dev] = true;
    }
  }
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)nwg), dim3(64), BYTES, s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

}  // namespace
