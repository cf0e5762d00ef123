// Batched symmetric rank-k products into the layout the batched Cholesky calls factor (cap_dsyrk_batched and, on a cap_vbatch_plan,
// cap_dsyrk_vbatched): the upper triangle of every column-major n x n block C_i <- beta C_i + alpha op(V_i) op(V_i)^T (+ shift[i] I),
// 0 <= n <= 256, any k >= 0 - Gram and normal-equation blocks, covariances, linear-kernel matrices, Schur complements C - W^T W.
//   CAP_NOTRANS: V_i is n x k column-major (ldv >= n), the V of cap_dcholupdate_batched.
//   CAP_TRANS:   V_i is k x n column-major (ldv >= k), the B / W of cap_dpotrs_batched and cap_dtrsm_batched; C = alpha V^T V + beta C.
// ONE launch per fixed-size call on a 1-D grid, one per occurring size class on a plan; no scratch, no allocation, no memset, no atomics, no
// helper stream, no host synchronisation, nothing between workgroups.  The loop over k is inside the launch.  A large k with few blocks
// leaves most of the chip idle: splitting k across workgroups would need atomics or scratch and is out of scope.
//
// THE ARITHMETIC, on both paths.  s_rc = sum_q v_rq v_cq on the fp64 16 x 16 x 4 MFMA from a ZERO accumulator, K ascending, four columns
// per instruction; rows >= n and columns >= k are supplied as +0.0 by the loader and never addressed.  Then, without contraction:
//   t = alpha * s;   out = (beta == 0) ? t : fma(beta, c_old, t);   on the diagonal with a shift: out = out + shift[i].
// beta == 0: C is not read (NaN and Inf there do not propagate).  alpha == 0 or k == 0: V is not addressed, s = +0.0.
// fill = 1: the value that was stored to (r, c) is stored to (c, r) as well - copied, never computed a second time; the strictly lower
// triangle is never read.
//
// THE TILES.  Lane l of a wavefront supplies row l % 16, column l / 16 of a 16 x 4 slab of op(V) (tools/mfma_f64_probe.hip); both MFMA
// operands come straight from global memory (NOTRANS: 128 contiguous bytes per 16 lanes; TRANS: the same elements, strided by ldv), a
// diagonal tile uses one register for both.  A tile is computed TRANSPOSED - the column slab is the A operand, the row slab the B operand - so
// that lane l holds, in accumulator register r, element (row l % 16, column l / 16 + 4 r) of the upper tile and 16 lanes store 128
// contiguous bytes of a column of C.  Products commute, so the bits are those of the tile computed the other way round.
// A wavefront always holds four slabs = 64 rows ("sb_macro"): n <= 64 - 64 / NP blocks of NP = 8 / 16 / 32 / 64 rows (two 8-row blocks share
// a tile; only the tiles of the upper triangle of a block are computed); 64 < n <= 256 - a workgroup of BB_THREADS per block, the macro tiles
// of the upper triangle - 64 x 64 on the diagonal, 64 rows x 32 columns off it - dealt round over the four waves (off-diagonal ones first),
// accumulators in registers, every macro tile reads its slabs of V itself (from L2 after the first time).  The 32-column pieces keep the
// kernel at two waves per SIMD, so that a second workgroup fills the gaps an uneven deal leaves (64 x 64 pieces: one wave per SIMD,
// 0.77 - 0.95 of torch.bmm's speed at n = 96 .. 192, profiles/r25_syrk_batched.txt).  Slabs at or beyond n are skipped by wave-uniform
// branches.
//
// THE BIT CONTRACTS.  1. PLAN = FIXED: every block of a plan call gets the bits of the fixed-size entry on it alone with batch = 1.
// 2. LAYOUT INDEPENDENCE: a block's bits are a function of (n, k, alpha, beta, shift, its data) only.  3. TRANS IS A LAYOUT: the same V in
// either layout gives the same bits.  4. ELEMENT INDEPENDENCE: c_rc is a function of rows r and c of V (and k, alpha, beta, c_old, shift)
// alone, the same on the wave path and on the workgroup path: every output element is its own chain from a zero accumulator, and the
// epilogue is elementwise.  1 - 3 hold by construction given 4; 4 rests on the MFMA computing every element of a tile alike.
// SHARED (vbatch_plan.h): the argument rules, the grid and the dispatch of the entry points, the walk over a plan's classes and the wave's
// largest n (vb_wave_max).  sb_block keeps its own lookup: one function serves the fixed-size and the plan kernels (PLAN) and returns the
// block as pointers into V and C, which vb_group does not know.
#include <vector>

#include "batched_blocked.h"
#include "capital_amd.h"
#include "vbatch_plan.h"

namespace {

constexpr int SB_MAX = 256;
constexpr int SB_U = 4;                          // k steps (of four columns) whose loads are issued together

struct SbArgs {
  const double* V; int64_t ldv, stride_v;        // stride_*: fixed size only
  double* C; int64_t ldc, stride_c;
  const double* shift;
  double alpha, beta;
  int64_t batch, k;                              // k: 0 when alpha == 0
  int n, fill;
  const VbRec* rec;                              // plan: one class of one call
  const int64_t* list; int64_t count;
};

struct SbBlk {                                   // one block as a lane sees it; n = 0: no block
  const double* v; double* c; int64_t ldc; double lam; int n;
};

template <bool TRANS, bool PLAN>
__device__ __forceinline__ SbBlk sb_block(const SbArgs& g, const int64_t at) {
  SbBlk b;
  b.v = g.V; b.c = g.C; b.ldc = 1; b.lam = 0.0; b.n = 0;
  if constexpr (PLAN) {
    if (at < g.count) {
      const int64_t blk = g.list[at];
      const VbRec r = g.rec[blk];
      b.n = (int)r.n; b.c = g.C + r.off; b.ldc = r.ld;
      b.v = g.V + (TRANS ? r.row * g.ldv : r.row);
      if (g.shift) b.lam = g.shift[blk];
    }
  } else {
    if (at < g.batch) {
      b.n = g.n; b.c = g.C + at * g.stride_c; b.ldc = g.ldc;
      b.v = g.V + at * g.stride_v;
      if (g.shift) b.lam = g.shift[at];
    }
  }
  return b;
}

// which tiles (row slab si, column slab sj) of the four slabs exist: on a diagonal macro tile those of the upper triangle of one block
template <int NP, bool DIAG>
constexpr bool sb_tile(int si, int sj) {
  return !DIAG || (si <= sj && (si * 16) / NP == (sj * 16) / NP);
}

template <int NP, bool DIAG, int NJ>
__device__ __forceinline__ void sb_mma(d4 (&acc)[4][NJ], const double (&a)[NJ], const double (&b)[4], const bool (&ona)[NJ], const bool (&onb)[4]) {
#pragma unroll
  for (int si = 0; si < 4; si++) {
#pragma unroll
    for (int sj = 0; sj < NJ; sj++) {
      if (sb_tile<NP, DIAG>(si, sj)) {
        if (onb[si] && ona[sj]) acc[si][sj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[sj], b[si], acc[si][sj], 0, 0, 0);
      }
    }
  }
}

// the epilogue of one element, without contraction: t = alpha s; out = beta == 0 ? t : fma(beta, c_old, t); diagonal: out + shift
__device__ __forceinline__ double sb_combine(const double alpha, const double beta, const double s, const double* c, const bool diag, const bool shifted,
                                              const double lam) {
#pragma clang fp contract(off)
  const double t = alpha * s;
  double out = t;
  if (beta != 0.0) out = __builtin_fma(beta, *c, t);
  if (diag && shifted) out = out + lam;
  return out;
}

// Four row slabs (rows I0 .. I0 + 63) against NJ column slabs (rows J0 .. J0 + 16 NJ - 1 of op(V)) by one wavefront; NJ = 4 on a diagonal.
// NP < 64: I0 = J0 = 0, DIAG, and wave row w = 16 s + lr is row w % NP of block w / NP of the wavefront's 64 / NP blocks - b[s] is that block as this lane sees it.  NP = 64:
// b[0 .. 3] are one block.  nmax: the largest n of the wavefront (wave-uniform).
template <int NP, bool TRANS, bool DIAG, int NJ>
__device__ __forceinline__ void sb_macro(const SbArgs& g, const SbBlk (&b)[4], const int I0, const int J0, const int nmax, const int lr, const int kg) {
  static_assert(DIAG || NP == 64, "off-diagonal macro tiles belong to the workgroup path");
  static_assert(!DIAG || NJ == 4, "a diagonal macro tile is square");
  const int64_t qs = TRANS ? 1 : g.ldv, rs = TRANS ? g.ldv : 1;     // strides of op(V) along k and along the rows
  const double* pa[NJ];
  const double* pb[4];
  bool oka[NJ], okb[4], ona[NJ], onb[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int w = s * 16 + lr;
    const int ri = I0 + (NP < 64 ? w % NP : w);
    okb[s] = ri < b[s].n;
    pb[s] = b[s].v + ri * rs + kg * qs;
    onb[s] = I0 + (s * 16) % NP < nmax;
  }
#pragma unroll
  for (int s = 0; s < NJ; s++) {
    const int w = s * 16 + lr;
    const int rj = J0 + (NP < 64 ? w % NP : w);
    oka[s] = rj < b[s].n;
    pa[s] = b[s].v + rj * rs + kg * qs;
    ona[s] = J0 + (s * 16) % NP < nmax;
  }
  d4 acc[4][NJ];
#pragma unroll
  for (int si = 0; si < 4; si++)
#pragma unroll
    for (int sj = 0; sj < NJ; sj++) acc[si][sj] = (d4){0.0, 0.0, 0.0, 0.0};

  const int64_t K = g.k;
  int64_t q = 0;
  for (; q + 4 * SB_U <= K; q += 4 * SB_U) {       // whole groups of steps: no column is beyond k
    double a[SB_U][NJ], bb[SB_U][4];
#pragma unroll
    for (int u = 0; u < SB_U; u++) {
#pragma unroll
      for (int s = 0; s < NJ; s++) {
        double t = 0.0;
        if (ona[s]) { if (oka[s]) t = pa[s][(q + 4 * u) * qs]; }
        a[u][s] = t;
      }
      if constexpr (!DIAG) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
          double v = 0.0;
          if (onb[s]) { if (okb[s]) v = pb[s][(q + 4 * u) * qs]; }
          bb[u][s] = v;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < SB_U; u++) {
      if constexpr (DIAG) sb_mma<NP, DIAG, NJ>(acc, a[u], a[u], ona, ona);
      else sb_mma<NP, DIAG, NJ>(acc, a[u], bb[u], ona, onb);
    }
  }
  for (; q < K; q += 4) {                          // the tail: columns at or beyond k are +0.0
    const bool in = q + kg < K;
    double a[NJ], bb[4];
#pragma unroll
    for (int s = 0; s < NJ; s++) {
      double t = 0.0;
      if (ona[s]) { if (oka[s] && in) t = pa[s][q * qs]; }
      a[s] = t;
    }
    if constexpr (!DIAG) {
#pragma unroll
      for (int s = 0; s < 4; s++) {
        double v = 0.0;
        if (onb[s]) { if (okb[s] && in) v = pb[s][q * qs]; }
        bb[s] = v;
      }
    }
    if constexpr (DIAG) sb_mma<NP, DIAG, NJ>(acc, a, a, ona, ona);
    else sb_mma<NP, DIAG, NJ>(acc, a, bb, ona, onb);
  }

  // lane (lr, kg), register r of tile (si, sj): wave row 16 si + lr, wave column 16 sj + kg + 4 r
  const bool shifted = g.shift != nullptr;
#pragma unroll
  for (int si = 0; si < 4; si++) {
#pragma unroll
    for (int sj = 0; sj < NJ; sj++) {
      if (sb_tile<NP, DIAG>(si, sj)) {
        if (onb[si] && ona[sj]) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int wi = si * 16 + lr, wj = sj * 16 + kg + 4 * r;
            const bool same = NP < 64 ? wi / NP == wj / NP : true;
            const int row = I0 + (NP < 64 ? wi % NP : wi), col = J0 + (NP < 64 ? wj % NP : wj);
            if (same && row <= col && col < b[si].n) {
              double* c = b[si].c + row + (int64_t)col * b[si].ldc;
              const double out = sb_combine(g.alpha, g.beta, acc[si][sj][r], c, row == col, shifted, b[si].lam);
              *c = out;
              if (g.fill && row != col) b[si].c[col + (int64_t)row * b[si].ldc] = out;
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ n <= 64: a wavefront per 64 / NP blocks
template <int NP, bool TRANS, bool PLAN>
__device__ __forceinline__ void sb_wave(const SbArgs& g) {
  constexpr int G = 64 / NP;
  const int lane = threadIdx.x, lr = lane & 15, kg = lane >> 4;
  SbBlk b[4];
  int m = 0;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    b[s] = sb_block<TRANS, PLAN>(g, (int64_t)blockIdx.x * G + (s * 16 + lr) / NP);
    m = b[s].n > m ? b[s].n : m;
  }
  int nmax = g.n;
  if constexpr (PLAN) nmax = vb_wave_max(m);
  sb_macro<NP, TRANS, true, 4>(g, b, 0, 0, nmax, lr, kg);
}

template <int NP, bool TRANS>
__global__ __launch_bounds__(64) void syrk_batched_kernel(SbArgs g) { sb_wave<NP, TRANS, false>(g); }

template <int NP, bool TRANS>
__global__ __launch_bounds__(64) void syrk_vbatched_kernel(SbArgs g) { sb_wave<NP, TRANS, true>(g); }

// ------------------------------------------------------------------------------------------------ 64 < n <= 256: a workgroup per block
template <bool TRANS, bool PLAN>
__device__ __forceinline__ void sb_group(const SbArgs& g) {
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const SbBlk b0 = sb_block<TRANS, PLAN>(g, (int64_t)blockIdx.x);
  const SbBlk b[4] = {b0, b0, b0, b0};
  const int n = __builtin_amdgcn_readfirstlane(b0.n);
  const int T = (n + 63) >> 6;
  int t = 0;
  for (int J0 = 64; J0 < n; J0 += 32)                 // off-diagonal: 64 rows x 32 columns each (eight tiles, two waves per SIMD)
    for (int I0 = 0; I0 < (J0 & ~63); I0 += 64)
      if ((t++ & (BB_WAVES - 1)) == wave) sb_macro<64, TRANS, false, 2>(g, b, I0, J0, n, lr, kg);
  for (int I = 0; I < T; I++)
    if ((t++ & (BB_WAVES - 1)) == wave) sb_macro<64, TRANS, true, 4>(g, b, I * 64, I * 64, n, lr, kg);
}

template <bool TRANS>
__global__ __launch_bounds__(BB_THREADS) void syrk_batched_blocked_kernel(SbArgs g) { sb_group<TRANS, false>(g); }

template <bool TRANS>
__global__ __launch_bounds__(BB_THREADS) void syrk_vbatched_blocked_kernel(SbArgs g) { sb_group<TRANS, true>(g); }

// ------------------------------------------------------------------------------------------------ host
static_assert((BB_WAVES & (BB_WAVES - 1)) == 0, "the macro tiles are dealt with a mask");

// f(NP, TRANS) with the group size and the layout of V as template arguments
template <class F>
void sb_with(int np, int trans, F f) {
  vb_with_int<8, 16, 32, 64>(np, [&](auto NP) {
    if (trans == CAP_TRANS) f(NP, std::true_type{});
    else f(NP, std::false_type{});
  });
}

int sb_fixed(int uplo, int trans, int64_t n, int64_t k, double alpha, const double* V, int64_t ldv, int64_t stride_v, double beta, double* C,
             int64_t ldc, int64_t stride_c, const double* shift, int fill, int64_t batch, hipStream_t s) {
  if ((trans != CAP_NOTRANS && trans != CAP_TRANS) || n < 0 || k < 0 || batch < 0 || (fill != 0 && fill != 1)) return CAP_ERR_ARG;
  if (!C && n > 0 && batch > 0) return CAP_ERR_ARG;
  if (!V && n > 0 && k > 0 && batch > 0 && alpha != 0.0) return CAP_ERR_ARG;
  const int64_t vrows = trans == CAP_TRANS ? k : n, vcols = trans == CAP_TRANS ? n : k;
  if (!vb_operand_ok(n, n, ldc, stride_c, batch) || !vb_operand_ok(vrows, vcols, ldv, stride_v, batch)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;      // as the other batched entries
  if (n > SB_MAX) return CAP_ERR_UNSUPPORTED;
  const int64_t nwg = vb_grid(batch, vb_per_group(vb_class(n)));
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  if (n == 0 || batch == 0) return CAP_OK;
  const int64_t keff = alpha == 0.0 ? 0 : k;
  if (cap_acc_on()) {
    for (int64_t i = 0; i < batch; i++) {
      if (keff > 0) cap_acc_r(V + i * stride_v, ldv, vrows, vcols);
      if (beta == 0.0) cap_acc_w(C + i * stride_c, ldc, n, n, fill ? 0 : 1);
      else cap_acc_rw(C + i * stride_c, ldc, n, n, fill ? 0 : 1);
    }
    if (shift) cap_acc_r(shift, 0, batch, 1);
  }
  SbArgs g = {};
  g.V = V; g.ldv = ldv; g.stride_v = stride_v; g.C = C; g.ldc = ldc; g.stride_c = stride_c; g.shift = shift; g.alpha = alpha; g.beta = beta;
  g.batch = batch; g.k = keff; g.n = (int)n; g.fill = fill;
  const dim3 grid((unsigned)nwg);
  sb_with(vb_padded(n), trans, [&](auto NP, auto TR) {
    if (n <= BB_SMALL) hipLaunchKernelGGL((syrk_batched_kernel<NP(), TR()>), grid, dim3(64), 0, s, g);
    else if (NP() == 64) hipLaunchKernelGGL((syrk_batched_blocked_kernel<TR()>), grid, dim3(BB_THREADS), 0, s, g);
  });
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int sb_plan(const cap_vbatch_plan* p, int uplo, int trans, int64_t k, double alpha, const double* V, int64_t ldv, double beta, double* C,
            const double* shift, int fill, hipStream_t s) {
  if (!p || (trans != CAP_NOTRANS && trans != CAP_TRANS) || k < 0 || (fill != 0 && fill != 1)) return CAP_ERR_ARG;
  if (p->nonempty > 0 && !C) return CAP_ERR_ARG;
  if (p->nonempty > 0 && k > 0 && alpha != 0.0 && !V) return CAP_ERR_ARG;
  if (ldv < (trans == CAP_TRANS ? k : p->rows)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (p->nonempty == 0) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  const int64_t keff = alpha == 0.0 ? 0 : k;
  SbArgs g = {};
  g.V = V; g.ldv = ldv; g.C = C; g.shift = shift; g.alpha = alpha; g.beta = beta; g.k = keff; g.fill = fill; g.rec = p->d_rec;
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    g.list = list;
    g.count = count;
    if (cap_acc_on()) {
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[(size_t)b];
        if (keff > 0) {
          if (trans == CAP_TRANS) cap_acc_r(V + r.row * ldv, ldv, k, r.n);
          else cap_acc_r(V + r.row, ldv, r.n, k);
        }
        if (beta == 0.0) cap_acc_w(C + r.off, r.ld, r.n, r.n, fill ? 0 : 1);
        else cap_acc_rw(C + r.off, r.ld, r.n, r.n, fill ? 0 : 1);
        if (shift) cap_acc_r(shift + b, 0, 1, 1);
      }
    }
    sb_with(cls < 4 ? 8 << cls : 64, trans, [&](auto NP, auto TR) {
      if (cls < 4) hipLaunchKernelGGL((syrk_vbatched_kernel<NP(), TR()>), grid, dim3(64), 0, s, g);
      else if (NP() == 64) hipLaunchKernelGGL((syrk_vbatched_blocked_kernel<TR()>), grid, dim3(BB_THREADS), 0, s, g);
    });
  });
}

}  // namespace

extern "C" {

int cap_dsyrk_batched(int uplo, int trans, int64_t n, int64_t k, double alpha, const double* V, int64_t ldv, int64_t stride_v, double beta,
                      double* C, int64_t ldc, int64_t stride_c, const double* shift, int fill, int64_t batch, void* stream) {
  return sb_fixed(uplo, trans, n, k, alpha, V, ldv, stride_v, beta, C, ldc, stride_c, shift, fill, batch, cap_stream(stream));
}

int cap_dsyrk_vbatched(const cap_vbatch_plan* p, int uplo, int trans, int64_t k, double alpha, const double* V, int64_t ldv, double beta,
                       double* C, const double* shift, int fill, void* stream) {
  return sb_plan(p, uplo, trans, k, alpha, V, ldv, beta, C, shift, fill, cap_stream(stream));
}

}  // extern "C"
