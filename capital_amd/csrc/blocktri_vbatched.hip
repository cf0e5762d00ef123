// RAGGED block-tridiagonal chains (cap_blocktri_plan, cap_dpotrf_blocktri_vbatched, cap_dpotrs_blocktri_vbatched,
// cap_dpotri_blocktri_vbatched): the factor, the solve and the selected inverse of blocktri_batched.hip / blocktri_potri_batched.hip for a
// batch whose chains have DIFFERENT lengths T_c >= 0, one n <= 64 per call.  D and E are one sequence of n x n slots each; chain c owns
// slots first_c .. first_c + T_c - 1, slot first_c + i of E couples its positions i and i + 1 (the chain's last slot of E is never
// addressed), the right-hand sides are stacked as cap_dpotrs_vbatched stacks them.  ONE launch per call on a 1-D grid over the plan's list
// of the chains SORTED BY T DESCENDING (stable): a workgroup is one wavefront, its G = 64 / NP lane groups carry G neighbours of that list -
// chains of neighbouring lengths - and the longest chains start first.  No scratch, no allocation, no memset, no atomics, no helper
// stream, nothing between workgroups; 64-bit offsets.
//
// THE BIT CONTRACT: every chain gets, bit for bit, what the fixed-size entry writes for it alone (T = T_c, batch = 1) - D, E, solutions,
// info, logdet.  The arithmetic is the fixed-size kernels' statement by statement (pb_factor_step, pb_forward_step, pb_backward_step,
// pi_invert, pi_product_row, the MFMA recurrence from a zero accumulator with the uncontracted epilogues); a chain's tiles exist only
// inside its own lane group (bt_tile, and the group test of every tile accessor), so no number of one chain meets a number of another.
//
// WHO IS ALIVE AT A STEP.  The wavefront walks steps 0 .. Tw - 1, Tw the largest T of its groups (vb_wave_max).  Ascending walks (factor,
// forward sweep) are at position `step` of every chain.  Descending walks (backward sweep, inverse) are at position T_c - 1 - step of EVERY
// CHAIN'S OWN length: all chains start at step 0 at their own last position, as the fixed-size kernels start (right-hand side loaded,
// Sigma = P without a coupling term), and in both directions a chain is active while step < T_c.  Aligning the starts was chosen over a
// wave-uniform descending position because it leaves ONE activity rule for all five walks and no joining in the middle of a loop (no
// mid-walk load of a segment, no selection between P and P - C G^T at a lane-dependent step); the price is that a descending position is
// a lane value, which only address arithmetic sees.  A chain that has ended leaves stale numbers (possibly NaN) in its image, its columns
// and its exchange lines, and the steps and products still run over them for the neighbours' sake; SELECTION keeps them in: every store,
// every prefetch and the sums into info / logdet carry the activity predicate of blocktri_addr.h, an ended chain's E columns enter the
// exchange area as +0.0, and the areas' "rows at or beyond n are +0.0" holds for every group since n is the call's.
// The T, first slot and row base of all G groups sit in a 256-byte LDS table (lane 0 of every group writes its entry once): a lane that
// holds a tile element or supplies a slab asks about the chain of its WAVE ROW, not its own.
//
// EVERY ADDRESS AND PREDICATE is a function of blocktri_addr.h (its btv_ section), swept lane by lane on the CPU over ragged plans
// (tests/test_blocktri_ragged_addr.py).  The bodies repeat those of the fixed-size kernels instead of sharing templates with them: the
// fixed-size device text stays byte for byte what it was.
#include <math.h>

#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "batched_inverse.h"
#include "batched_small.h"
#include "blocktri_addr.h"
#include "capital_amd.h"
#include "common.h"
#include "vbatch_plan.h"

struct BtRec {                         // one chain, in batch order
  int64_t first, T, row;
};

struct cap_blocktri_plan {
  int64_t batch = 0, slots = 0, eslots = 0, rows = 0, tmax = 0;
  int64_t nonempty = 0;                // chains with T > 0
  std::vector<BtRec> rec;              // host copies: the access notes and cap_blocktri_plan_order read them
  std::vector<int64_t> order;          // the chains by T descending, stable
  int device = -1;                     // -1: made in a process without a device - a description only, no entry runs on it
  BtRec* d_rec = nullptr;
  int64_t* d_order = nullptr;
};

namespace {

struct BvArgs {                        // factor and inverse
  double* D; double* E;
  BtGeo gd, ge;
  const BtRec* rec; const int64_t* order; int64_t count;
  int* info; double* logdet;           // the inverse reads info and has no logdet
  int fill;
};

struct BvSolveArgs {
  const double* D; const double* E;
  BtGeo gd, ge;
  const BtRec* rec; const int64_t* order; int64_t count;
  double* B; int64_t ldb, nrhs;
  const int* info;
  int half;
};

template <int NP>
constexpr bool bv_img_agrees() {
  return PbImg<NP>::SIZE == bt_img_size(NP) && PbImg<NP>::LD == bt_img_ld(NP) && PiImg<NP>::SIZE == bt_img_size(NP) && PiImg<NP>::LD == bt_img_ld(NP);
}

// the epilogues of syrk_batched.hip / gemm_batched.hip without contraction: t = alpha s with alpha = -1; out = t, or out = fma(beta, c, t) with beta = 1
__device__ __forceinline__ double bv_neg(const double s) {
#pragma clang fp contract(off)
  return -1.0 * s;
}
__device__ __forceinline__ double bv_minus(const double c, const double s) {
#pragma clang fp contract(off)
  const double t = -1.0 * s;
  return __builtin_fma(1.0, c, t);
}

// NP = 64 takes the parameter-pack form of the steps (see batched_small.h)
template <int NP, int... J>
__device__ __forceinline__ void bv_forward_pack(double (&x)[NP], const double* s, int n, std::integer_sequence<int, J...>) {
  (pb_forward_step<NP>(x, s, n, J), ...);
}
template <int NP, int... J>
__device__ __forceinline__ void bv_backward_pack(double (&x)[NP], const double* s, int n, std::integer_sequence<int, J...>) {
  (pb_backward_step<NP>(x, s, n, NP - 1 - J), ...);
}
template <int NP>
__device__ __forceinline__ void bv_forward(double (&x)[NP], const double* s, int n) {
  if constexpr (NP < 64) {
#pragma unroll
    for (int j = 0; j < NP; j++) pb_forward_step<NP>(x, s, n, j);
  } else {
    bv_forward_pack<NP>(x, s, n, std::make_integer_sequence<int, NP>{});
  }
}
template <int NP>
__device__ __forceinline__ void bv_backward(double (&x)[NP], const double* s, int n) {
  if constexpr (NP < 64) {
#pragma unroll
    for (int j = NP - 1; j >= 0; j--) pb_backward_step<NP>(x, s, n, j);
  } else {
    bv_backward_pack<NP>(x, s, n, std::make_integer_sequence<int, NP>{});
  }
}

// ------------------------------------------------------------------------------------------------ the wavefront's chains
__device__ __forceinline__ BtChain bv_chain_of(const int64_t* tab, const int group) {
  BtChain ch;
  ch.first = tab[btv_tab_at(group, 0)];
  ch.T = tab[btv_tab_at(group, 1)];
  ch.row = tab[btv_tab_at(group, 2)];
  ch.id = tab[btv_tab_at(group, 3)];
  return ch;
}

// a wave-uniform 64-bit value in scalar registers
__device__ __forceinline__ int64_t bv_uniform(const int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)(uint64_t)v), hi = __builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the chain of the lane's wave row in slab s: from the table; NP = 64 has one group - the lane's own chain, in scalar registers
template <int NP>
__device__ __forceinline__ BtChain bv_row_chain(const int64_t* tab, const BtChain& own, const int lane, const int s) {
  if constexpr (NP == 64) return own;
  else return bv_chain_of(tab, btv_row_group(NP, lane, s));
}

// blockIdx.x -> sorted list -> record (as vb_group): the lane's own chain, the table of all groups in LDS and the wave's largest T.  A group
// beyond the list has T = 0.
template <int NP>
__device__ __forceinline__ BtChain bv_lookup(const BtRec* rec, const int64_t* order, const int64_t count, int64_t* tab, int& tw) {
  const int lane = threadIdx.x;
  const int64_t at = bt_chain(NP, blockIdx.x, lane);
  BtChain ch;
  ch.first = 0; ch.T = 0; ch.row = 0; ch.id = 0;
  if (at < count) {
    ch.id = order[at];
    const BtRec r = rec[ch.id];
    ch.first = r.first; ch.T = r.T; ch.row = r.row;
  }
  if (bt_idx(NP, lane) == 0) {
    const int grp = bt_group(NP, lane);
    tab[btv_tab_at(grp, 0)] = ch.first;
    tab[btv_tab_at(grp, 1)] = ch.T;
    tab[btv_tab_at(grp, 2)] = ch.row;
    tab[btv_tab_at(grp, 3)] = ch.id;
  }
  tw = vb_wave_max((int)ch.T);         // n T <= 2^31 - 1 (the entries refuse more)
  __syncthreads();
  if constexpr (NP == 64) {            // one group: the record is the wave's
    ch.first = bv_uniform(ch.first); ch.T = bv_uniform(ch.T); ch.row = bv_uniform(ch.row); ch.id = bv_uniform(ch.id);
  }
  return ch;
}

// the upper triangle of diagonal block `pos` of the lane's chain -> the group's image
template <int NP>
__device__ __forceinline__ void bv_load_tri(const double* D, const BtGeo& gd, const BtChain& own, const int lane, const int64_t pos, double* s) {
  const int r = bt_idx(NP, lane);
#pragma unroll 8
  for (int cc = 0; cc < gd.n; cc++) {
    const BtAt at = btv_tri_at(gd, own, lane, pos, cc);
    if (at.on) s[bt_img_at(NP, r, cc)] = D[at.off];
  }
}

// column lane % NP of coupling block `pos` -> registers (+0.0 where the lane has none)
template <int NP>
__device__ __forceinline__ void bv_load_ecol(const double* E, const BtGeo& ge, const BtChain& own, const int lane, const int64_t pos, double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    double t = 0.0;
    if (i < ge.n) {
      const BtAt at = btv_ecol_at(ge, own, lane, pos, i);
      if (at.on) t = E[at.off];
    }
    x[i] = t;
  }
}

// ------------------------------------------------------------------------------------------------ factor
template <int NP>
__global__ __launch_bounds__(64) void blocktri_vpotrf_kernel(BvArgs g) {
  constexpr int G = 64 / NP;
  constexpr bool EARLY = NP < 64;
  using Img = PbImg<NP>;
  static_assert(bv_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h");
  __shared__ double s_img[G * Img::SIZE];
  __shared__ double s_x[bt_x_size(NP)];
  __shared__ double s_log[64];
  __shared__ int64_t s_tab[btv_tab_size()];
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane0 = threadIdx.x, n = gd.n;
  int tw;
  const BtChain own = bv_lookup<NP>(g.rec, g.order, g.count, s_tab, tw);
  const int64_t Tw = tw;

  bv_load_tri<NP>(g.D, gd, own, lane0, 0, s_img + bt_img_base(NP, lane0));
  __syncthreads();
  int cinfo = 0;
  double ldsum = 0.0;

  for (int64_t pos = 0; pos < Tw; pos++) {
    // NP = 64: the lane behind an opaque zero, as the inverse kernel has it - the offsets of a position are formed at that position instead of
    // all being kept in registers across the walk, which together with the chain's record spills
    const int lane = NP == 64 ? lane0 + pi_opaque_zero() : lane0, c = bt_idx(NP, lane);
    double* s = s_img + bt_img_base(NP, lane);
    const bool active = btv_active(own, pos);
    double x[NP];
    if constexpr (EARLY) bv_load_ecol<NP>(g.E, ge, own, lane, pos, x);
    double dn[4][4][4];
#pragma unroll
    for (int si = 0; si < 4; si++) {
      const BtChain chr = bv_row_chain<NP>(s_tab, own, lane, si);
#pragma unroll
      for (int sj = 0; sj < 4; sj++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double t = 0.0;
          if (bt_tile(NP, si, sj, true)) {
            if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
              const BtAt at = btv_next_at(gd, chr, lane, pos, si, sj, r);
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
    __syncthreads();

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
      const BtAt at = btv_tri_at(gd, own, lane, pos, cc);
      if (at.on) g.D[at.off] = s[bt_img_at(NP, c, cc)];
    }
    if (active && info != 0 && cinfo == 0) cinfo = (int)(pos * n) + info;
    if (g.logdet) {
      s_log[bt_log_at(NP, lane, c)] = c < n ? log(s[Img::at(c, c)]) : 0.0;
      __syncthreads();
      if (c == 0 && active) {          // an ended chain's image is stale: its sum stands
        double t = 0.0;
        for (int j = 0; j < n; j++) t += s_log[bt_log_at(NP, lane, j)];
        ldsum += bad ? (double)NAN : 2.0 * t;
      }
    }
    if (!bt_has_next(Tw, pos)) break;    // wave-uniform: no chain of the wave has a successor

    if constexpr (!EARLY) bv_load_ecol<NP>(g.E, ge, own, lane, pos, x);
    bv_forward<NP>(x, s, n);
#pragma unroll
    for (int i = 0; i < NP; i++) {
      if (i < n) {
        const double v = bad ? (double)NAN : x[i];
        const BtAt at = btv_ecol_at(ge, own, lane, pos, i);
        if (at.on) g.E[at.off] = v;
        s_x[bt_x_own(i, lane)] = at.on ? v : 0.0;
      }
    }
    __syncthreads();

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
              if (at.on) s_img[at.off] = bv_minus(dn[si][sj][r], acc[si][sj][r]);
            }
          }
        }
    __syncthreads();
  }

  const BtAt at = btv_scalar_at(NP, own, lane0);
  if (at.on) {
    g.info[at.off] = cinfo;
    if (g.logdet) g.logdet[at.off] = ldsum;
  }
}

// ------------------------------------------------------------------------------------------------ solve
template <int NP>
__device__ __forceinline__ void bv_rhs_load(const BvSolveArgs& g, const BtGeo& gd, const BtChain& own, const int lane, const int64_t pass, const int64_t pos,
                                            double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    double t = 0.0;
    if (i < gd.n) {
      const BtAt at = btv_rhs_at(gd, own, g.ldb, g.nrhs, lane, pass, pos, i);
      if (at.on) t = g.B[at.off];
    }
    x[i] = t;
  }
}

template <int NP>
__device__ __forceinline__ void bv_rhs_store(const BvSolveArgs& g, const BtGeo& gd, const BtChain& own, const int lane, const int64_t pass, const int64_t pos,
                                             const bool bad, const double (&x)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; i++) {
    if (i < gd.n) {
      const BtAt at = btv_rhs_at(gd, own, g.ldb, g.nrhs, lane, pass, pos, i);
      if (at.on) g.B[at.off] = bad ? (double)NAN : x[i];
    }
  }
}

// x <- c - op(W) x at a step (bt_couple of blocktri_batched.hip): DESC false - the forward sweep, op(W) = W^T; true - the backward sweep.
// The coupling block and the target segment are those of the ADDRESSED chain at this step (btv_couple_epos, btv_couple_tpos)
template <int NP, bool DESC>
__device__ __forceinline__ void bv_couple(const BvSolveArgs& g, const BtGeo& gd, const BtGeo& ge, const BtChain& own, const int64_t* s_tab, const int lane,
                                          const int64_t pass, const int64_t step, double* s_x, double (&x)[NP]) {
  const int n = gd.n;
  constexpr bool EARLY = NP < 64;
  const int64_t tpos = btv_couple_tpos(own, step, DESC);
  double cn[NP];
  if constexpr (EARLY) bv_rhs_load<NP>(g, gd, own, lane, pass, tpos, cn);
#pragma unroll
  for (int i = 0; i < NP; i++)
    if (i < n) s_x[bt_x_own(i, lane)] = x[i];
  __syncthreads();

  bool onc[4];
#pragma unroll
  for (int sl = 0; sl < 4; sl++) onc[sl] = pass * NP + (sl * 16) % NP < g.nrhs;
  int64_t ebase[4], eT[4];               // the chain of the lane's wave row in every slab
#pragma unroll
  for (int sl = 0; sl < 4; sl++) {
    const BtChain chr = bv_row_chain<NP>(s_tab, own, lane, sl);
    ebase[sl] = chr.first; eT[sl] = chr.T;
  }
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
            BtChain chr;
            chr.first = ebase[sl]; chr.T = eT[sl]; chr.row = 0; chr.id = 0;
            const BtAt at = btv_eslab_at(ge, chr, lane, btv_couple_epos(chr, step, DESC), sl, q0 + 4 * u, !DESC);
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
  __syncthreads();
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
  if constexpr (!EARLY) bv_rhs_load<NP>(g, gd, own, lane, pass, tpos, cn);
#pragma unroll
  for (int i = 0; i < NP; i++)
    if (i < n) x[i] = bv_minus(cn[i], s_x[bt_x_own(i, lane)]);
}

template <int NP>
__global__ __launch_bounds__(64) void blocktri_vpotrs_kernel(BvSolveArgs g) {
  constexpr int G = 64 / NP;
  static_assert(bv_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h");
  __shared__ double s_img[G * PbImg<NP>::SIZE];
  __shared__ double s_x[bt_x_size(NP)];
  __shared__ int64_t s_tab[btv_tab_size()];
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane = threadIdx.x, n = gd.n;
  int tw;
  const BtChain own = bv_lookup<NP>(g.rec, g.order, g.count, s_tab, tw);
  const int64_t Tw = tw;
  double* s = s_img + bt_img_base(NP, lane);
  const BtAt ia = btv_info_at(own);
  bool bad = false;
  if (g.info) { if (ia.on) bad = g.info[ia.off] != 0; }

  const int64_t passes = bt_rhs_passes(NP, g.nrhs);
  for (int64_t pass = 0; pass < passes; pass++) {
    double x[NP];
    if (g.half != 2) {                   // R^T y = b, positions ascending
      bv_rhs_load<NP>(g, gd, own, lane, pass, btv_pos(own, 0, false), x);
      for (int64_t step = 0; step < Tw; step++) {
        const int64_t pos = btv_pos(own, step, false);
        __syncthreads();                 // the image of the step before is read no more
        bv_load_tri<NP>(g.D, gd, own, lane, pos, s);
        __syncthreads();
        bv_forward<NP>(x, s, n);
        bv_rhs_store<NP>(g, gd, own, lane, pass, pos, bad, x);
        if (!bt_has_next(Tw, step)) break;
        bv_couple<NP, false>(g, gd, ge, own, s_tab, lane, pass, step, s_x, x);
      }
    }
    if (g.half != 1) {                   // R x = y, every chain's own positions descending
      bv_rhs_load<NP>(g, gd, own, lane, pass, btv_pos(own, 0, true), x);
      for (int64_t step = 0; step < Tw; step++) {
        const int64_t pos = btv_pos(own, step, true);
        __syncthreads();
        bv_load_tri<NP>(g.D, gd, own, lane, pos, s);
        __syncthreads();
        bv_backward<NP>(x, s, n);
        bv_rhs_store<NP>(g, gd, own, lane, pass, pos, bad, x);
        if (!bt_has_next(Tw, step)) break;
        bv_couple<NP, true>(g, gd, ge, own, s_tab, lane, pass, step, s_x, x);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ selected inverse
template <int NP>
constexpr int64_t bv_inv_lds_bytes() { return 8 * ((int64_t)(64 / NP) * bt_img_size(NP) + 2 * bt_x_size(NP) + btv_tab_size()); }

template <int NP, bool UPPER>
__device__ __forceinline__ void bv_product(const double* a, const double* b, const int n, const int lane, d4 (&acc)[4][4]) {
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

__device__ __forceinline__ void bv_zero(d4 (&acc)[4][4]) {
#pragma unroll
  for (int si = 0; si < 4; si++)
#pragma unroll
    for (int sj = 0; sj < 4; sj++) acc[si][sj] = (d4){0.0, 0.0, 0.0, 0.0};
}

template <int NP>
__global__ __launch_bounds__(64) void blocktri_vpotri_kernel(BvArgs g) {
  constexpr int G = 64 / NP;
  constexpr bool EARLY = NP < 64;
  constexpr bool EARLY_U = NP <= 32;
  using Img = PiImg<NP>;
  static_assert(bv_img_agrees<NP>(), "blocktri_addr.h restates the image of batched_small.h and batched_inverse.h");
  extern __shared__ __attribute__((aligned(16))) double bv_lds[];
  double* s_img = bv_lds;                          // G images: U_i, then P_i
  double* s_g = s_img + G * bt_img_size(NP);       // X1: G_i
  double* s_sig = s_g + bt_x_size(NP);             // X2: Sigma_(i+1,i+1) mirrored, then C_i, then Sigma_(i,i) mirrored
  int64_t* s_tab = reinterpret_cast<int64_t*>(s_sig + bt_x_size(NP));
  BtGeo gd = g.gd, ge = g.ge;
  gd.NP = NP; ge.NP = NP;
  const int lane0 = threadIdx.x, n = gd.n;
  int tw;
  const BtChain own0 = bv_lookup<NP>(g.rec, g.order, g.count, s_tab, tw);
  const int64_t Tw = tw;
  const BtAt ia = btv_info_at(own0);
  bool bad = false;
  if (g.info) { if (ia.on) bad = g.info[ia.off] != 0; }

  for (int j = 0; j < bt_x_clear_passes(NP); j++) {
    const BtAt at = bt_x_clear(NP, lane0, j);
    if (at.on) s_g[at.off] = 0.0;
  }
  bv_load_tri<NP>(g.D, gd, own0, lane0, btv_pos(own0, 0, true), s_img + bt_img_base(NP, lane0));
  __syncthreads();

  double xe[EARLY ? NP : 1];
  if constexpr (EARLY) bv_load_ecol<NP>(g.E, ge, own0, lane0, btv_pos(own0, 0, true) - 1, xe);

  for (int64_t step = 0; step < Tw; step++) {
    const bool first = step == 0;        // wave-uniform: every chain starts at its own last position, Sigma = P
    // The lane behind an opaque zero (see blocktri_potri_batched.hip): offsets, LDS addresses, lane predicates and the chain's record are
    // formed at the step, not kept in registers across the walk
    const int lane = lane0 + pi_opaque_zero(), c = bt_idx(NP, lane);
    const BtChain own = bv_chain_of(s_tab, bt_group(NP, lane));
    const int64_t pos = btv_pos(own, step, true);
    double* s = s_img + bt_img_base(NP, lane);
    double un[EARLY_U ? NP : 1];
    if constexpr (EARLY_U) {
#pragma unroll
      for (int cc = 0; cc < NP; cc++) {
        double t = 0.0;
        if (cc < n) {
          const BtAt at = btv_tri_at(gd, own, lane, pos - 1, cc);
          if (at.on) t = g.D[at.off];
        }
        un[cc] = t;
      }
    }

    if (!first) {
      double x[NP];
      if constexpr (EARLY) {
#pragma unroll
        for (int i = 0; i < NP; i++) x[i] = xe[i];
      } else {
        bv_load_ecol<NP>(g.E, ge, own, lane, pos, x);
      }
      bv_backward<NP>(x, s, n);
#pragma unroll
      for (int i = 0; i < NP; i++)
        if (i < n && c < n) s_g[bt_xt_own(NP, i, lane)] = bad ? (double)NAN : x[i];
      if constexpr (EARLY) bv_load_ecol<NP>(g.E, ge, own, lane, pos - 1, xe);
    }
    __builtin_amdgcn_sched_barrier(0);

    {
      double w[NP];
      pi_invert<NP>(w, s, c, n);
      __syncthreads();
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
    __syncthreads();

    d4 acc[4][4];
    bv_zero(acc);
    if (!first) {
      bv_product<NP, false>(s_g, s_sig, n, lane, acc);
      __syncthreads();
#pragma unroll
      for (int si = 0; si < 4; si++) {
        const BtChain chr = bv_row_chain<NP>(s_tab, own, lane, si);
        const int64_t rpos = btv_pos(chr, step, true);
#pragma unroll
        for (int sj = 0; sj < 4; sj++)
          if (bt_tile(NP, si, sj, false)) {
            if (bt_slab_on(NP, si, n) && bt_slab_on(NP, sj, n)) {
#pragma unroll
              for (int r = 0; r < 4; r++) {
                const double t = bv_neg(acc[si][sj][r]);
                const BtAt at = btv_etile_at(ge, chr, lane, rpos, si, sj, r);
                if (at.on) g.E[at.off] = t;
                const BtAt xt = bt_xt_tile(n, NP, lane, si, sj, r);
                if (xt.on) s_sig[xt.off] = t;
              }
            }
          }
      }
      __syncthreads();
      bv_zero(acc);
      bv_product<NP, true>(s_sig, s_g, n, lane, acc);
    }
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
                acc[si][sj][r] = first ? p : bv_minus(p, acc[si][sj][r]);
              }
            }
          }
        }
    __syncthreads();
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
    for (int cc = 0; cc < n; cc++) {
      const BtAt at = btv_full_at(gd, own, lane, pos, cc, g.fill);
      if (at.on) g.D[at.off] = bad ? (double)NAN : s_sig[bt_x_own(cc, lane)];
    }
    if (!bt_has_next(Tw, step)) break;   // wave-uniform: no chain of the wave has a predecessor left

    if constexpr (EARLY_U) {
#pragma unroll
      for (int cc = 0; cc < NP; cc++)
        if (c <= cc && cc < n) s[bt_img_at(NP, c, cc)] = un[cc];
    } else {
      bv_load_tri<NP>(g.D, gd, own, lane, pos - 1, s);
    }
    __syncthreads();
  }
}

template <int NP>
int bv_inv_launch(const BvArgs& g, int64_t nwg, hipStream_t s) {
  constexpr int BYTES = (int)bv_inv_lds_bytes<NP>();
  if constexpr (BYTES > 64 * 1024) {
    static bool attr_set[16] = {};
    int dev = 0;
    CAP_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16 || !attr_set[dev]) {
      CAP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(blocktri_vpotri_kernel<NP>), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES));
      if (dev >= 0 && dev < 16) attr_set[dev] = true;
    }
  }
  hipLaunchKernelGGL(blocktri_vpotri_kernel<NP>, dim3((unsigned)nwg), dim3(64), BYTES, s, g);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

// ------------------------------------------------------------------------------------------------ host
static void bv_geo(BtGeo& g, int64_t n, int64_t ld, int64_t step) {
  g.ld = ld; g.step = step; g.stride = 0; g.T = 0; g.batch = 0; g.n = (int)n; g.NP = vb_padded(n);
}

// rule 3 of the entries for D and E: leading dimensions, and the step where the plan spans more than one slot (128-bit products)
static bool bv_operands_ok(const cap_blocktri_plan* p, int64_t n, int64_t ldd, int64_t step_d, int64_t lde, int64_t step_e) {
  if (ldd < n) return false;
  if (p->slots > 1 && (__int128)step_d < (__int128)ldd * n) return false;
  if (p->eslots > 0) {
    if (lde < n) return false;
    if (p->eslots > 1 && (__int128)step_e < (__int128)lde * n) return false;
  }
  return true;
}

// rules 5 - 8; > 0: the workgroups, 0 with st == CAP_OK: an empty plan
static int64_t bv_limits(const cap_blocktri_plan* p, int uplo, int64_t n, int& st) {
  st = CAP_ERR_UNSUPPORTED;
  if (uplo != CAP_UPPER) return 0;
  if (n > BT_MAX) return 0;
  if ((__int128)p->tmax * n > (__int128)0x7fffffffLL) return 0;
  const int64_t nwg = vb_grid(p->batch, 64 / vb_padded(n));
  if (nwg < 0) return 0;
  st = CAP_OK;
  return nwg;
}

// the access notes of the plan and of the chains' blocks: mode_d / mode_e are CAP_ACC_R or CAP_ACC_RW
static void bv_notes(const cap_blocktri_plan* p, const BtGeo& gd, const BtGeo& ge, const double* D, const double* E, int mode_d, int tri, int mode_e) {
  cap_acc_r(p->d_rec, 0, p->batch * (int64_t)(sizeof(BtRec) / 8), 1);
  cap_acc_r(p->d_order, 0, p->batch, 1);
  for (const BtRec& r : p->rec) {
    const BtChain ch = {r.first, r.T, r.row, 0};
    for (int64_t i = 0; i < r.T; i++) {
      cap_acc(mode_d, D + btv_block(gd, ch, i), gd.ld, gd.n, gd.n, tri);
      if (btv_has_next(ch, i)) cap_acc(mode_e, E + btv_block(ge, ch, i), ge.ld, ge.n, ge.n);
    }
  }
}

// info / logdet: only the entries of the chains that have a position
static void bv_note_scalars(const cap_blocktri_plan* p, const void* v, int mode, int elem) {
  for (int64_t c = 0; c < p->batch; c++)
    if (p->rec[(size_t)c].T > 0) cap_acc(mode, (const char*)v + c * elem, 0, 1, 1, 0, elem);
}

}  // namespace

extern "C" {

int cap_blocktri_plan_destroy(cap_blocktri_plan* p) {
  if (!p) return CAP_OK;
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->d_order) (void)hipFree(p->d_order);
  delete p;
  return CAP_OK;
}

int cap_blocktri_plan_create(int64_t batch, const int64_t* T, const int64_t* first, cap_blocktri_plan** out) {
  if (!out) return CAP_ERR_ARG;
  *out = nullptr;
  if (batch < 0 || (batch > 0 && !T)) return CAP_ERR_ARG;
  for (int64_t c = 0; c < batch; c++)
    if (T[c] < 0 || (first && first[c] < 0)) return CAP_ERR_ARG;
  cap_blocktri_plan* p = new (std::nothrow) cap_blocktri_plan;
  if (!p) return CAP_ERR_ALLOC;
  p->batch = batch;
  p->rec.resize((size_t)batch);
  __int128 row = 0;
  bool over = false;
  std::vector<std::pair<int64_t, int64_t>> win;      // (first slot, one past the last) of every non-empty chain
  for (int64_t c = 0; c < batch; c++) {
    BtRec& r = p->rec[(size_t)c];
    r.T = T[c];
    r.first = first ? first[c] : (int64_t)row;
    r.row = (int64_t)row;
    row += r.T;
    over = over || row > (__int128)INT64_MAX || (__int128)r.first + r.T > (__int128)INT64_MAX;
    if (over) break;
    if (r.T == 0) continue;
    win.emplace_back(r.first, r.first + r.T);
    p->nonempty++;
    p->slots = std::max(p->slots, r.first + r.T);
    if (r.T > 1) p->eslots = std::max(p->eslots, r.first + r.T - 1);
    p->tmax = std::max(p->tmax, r.T);
  }
  if (!over) {
    std::sort(win.begin(), win.end());
    for (size_t k = 1; k < win.size(); k++)
      if (win[k].first < win[k - 1].second) { delete p; return CAP_ERR_ARG; }      // two chains' slot ranges meet
  }
  if (over) { delete p; return CAP_ERR_ARG; }
  p->rows = (int64_t)row;
  p->order.resize((size_t)batch);
  for (int64_t c = 0; c < batch; c++) p->order[(size_t)c] = c;
  std::stable_sort(p->order.begin(), p->order.end(), [&](int64_t a, int64_t b) { return p->rec[(size_t)a].T > p->rec[(size_t)b].T; });
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); *out = p; return CAP_OK; }
  if (hipGetDevice(&p->device) != hipSuccess) { (void)hipGetLastError(); delete p; return CAP_ERR_HIP; }
  if (batch > 0) {
    if (hipMalloc((void**)&p->d_rec, sizeof(BtRec) * (size_t)batch) != hipSuccess ||
        hipMalloc((void**)&p->d_order, sizeof(int64_t) * (size_t)batch) != hipSuccess ||
        hipMemcpy(p->d_rec, p->rec.data(), sizeof(BtRec) * (size_t)batch, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_order, p->order.data(), sizeof(int64_t) * (size_t)batch, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      cap_blocktri_plan_destroy(p);
      return CAP_ERR_ALLOC;
    }
  }
  *out = p;
  return CAP_OK;
}

int64_t cap_blocktri_plan_info(const cap_blocktri_plan* p, int what) {
  if (!p) return -1;
  switch (what) {
    case CAP_BLOCKTRI_BATCH: return p->batch;
    case CAP_BLOCKTRI_SLOTS: return p->slots;
    case CAP_BLOCKTRI_ESLOTS: return p->eslots;
    case CAP_BLOCKTRI_ROWS: return p->rows;
    case CAP_BLOCKTRI_TMAX: return p->tmax;
    default: return -1;
  }
}

int cap_blocktri_plan_order(const cap_blocktri_plan* p, int64_t* chains, int64_t cap) {
  if (!p || cap < 0 || (cap > 0 && !chains)) return CAP_ERR_ARG;
  const int64_t m = std::min(cap, p->batch);
  for (int64_t k = 0; k < m; k++) chains[k] = p->order[(size_t)k];
  return CAP_OK;
}

int cap_dpotrf_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int64_t n, double* D, int64_t ldd, int64_t step_d, double* E, int64_t lde,
                                 int64_t step_e, int* info, double* logdet, void* stream) {
  if (!p || n < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && p->nonempty > 0;
  if (work && (!D || !info || (!E && p->eslots > 0))) return CAP_ERR_ARG;
  if (!bv_operands_ok(p, n, ldd, step_d, lde, step_e)) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bv_limits(p, uplo, n, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  BvArgs g = {};
  g.D = D; g.E = E; g.info = info; g.logdet = logdet;
  g.rec = p->d_rec; g.order = p->d_order; g.count = p->batch;
  bv_geo(g.gd, n, ldd, step_d);
  bv_geo(g.ge, n, lde, step_e);
  if (cap_acc_on()) {
    bv_notes(p, g.gd, g.ge, D, E, CAP_ACC_RW, 1, CAP_ACC_RW);
    bv_note_scalars(p, info, CAP_ACC_W, 4);
    if (logdet) bv_note_scalars(p, logdet, CAP_ACC_W, 8);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { hipLaunchKernelGGL(blocktri_vpotrf_kernel<NP()>, dim3((unsigned)nwg), dim3(64), 0, s, g); });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_dpotrs_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int half, int64_t n, int64_t nrhs, const double* D, int64_t ldd, int64_t step_d,
                                 const double* E, int64_t lde, int64_t step_e, double* B, int64_t ldb, const int* info, void* stream) {
  if (!p || n < 0 || nrhs < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && nrhs > 0 && p->nonempty > 0;
  if (work && (!D || !B || (!E && p->eslots > 0))) return CAP_ERR_ARG;
  if (!bv_operands_ok(p, n, ldd, step_d, lde, step_e) || (__int128)ldb < (__int128)p->rows * n) return CAP_ERR_ARG;
  if (half < 0 || half > 2) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bv_limits(p, uplo, n, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  BvSolveArgs g = {};
  g.D = D; g.E = E; g.B = B; g.ldb = ldb; g.nrhs = nrhs; g.info = info; g.half = half;
  g.rec = p->d_rec; g.order = p->d_order; g.count = p->batch;
  bv_geo(g.gd, n, ldd, step_d);
  bv_geo(g.ge, n, lde, step_e);
  if (cap_acc_on()) {
    bv_notes(p, g.gd, g.ge, D, E, CAP_ACC_R, 1, CAP_ACC_R);
    for (const BtRec& r : p->rec) cap_acc_rw(B + r.row * n, ldb, r.T * n, nrhs);
    if (info) bv_note_scalars(p, info, CAP_ACC_R, 4);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { hipLaunchKernelGGL(blocktri_vpotrs_kernel<NP()>, dim3((unsigned)nwg), dim3(64), 0, s, g); });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int cap_dpotri_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int fill, int64_t n, double* D, int64_t ldd, int64_t step_d, double* E, int64_t lde,
                                 int64_t step_e, const int* info, void* stream) {
  if (!p || n < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && p->nonempty > 0;
  if (work && (!D || (!E && p->eslots > 0))) return CAP_ERR_ARG;
  if (!bv_operands_ok(p, n, ldd, step_d, lde, step_e)) return CAP_ERR_ARG;
  if (fill != 0 && fill != 1) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bv_limits(p, uplo, n, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  BvArgs g = {};
  g.D = D; g.E = E; g.info = const_cast<int*>(info); g.fill = fill;
  g.rec = p->d_rec; g.order = p->d_order; g.count = p->batch;
  bv_geo(g.gd, n, ldd, step_d);
  bv_geo(g.ge, n, lde, step_e);
  if (cap_acc_on()) {
    bv_notes(p, g.gd, g.ge, D, E, CAP_ACC_RW, fill ? 0 : 1, CAP_ACC_RW);
    if (info) bv_note_scalars(p, info, CAP_ACC_R, 4);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bv_inv_launch<NP()>(g, nwg, s); });
  return st;
}

}  // extern "C"
