// Batched products with the SYMMETRIC block itself, from the one triangle the batched family keeps, and the diagnostics built on them
// (cap_dsymm_batched, cap_dlansy_batched, cap_dpocon_batched, cap_dpoerr_batched and, on a cap_vbatch_plan, their _vbatched forms):
//   Y_i <- beta B_i + alpha A_i X_i,   A_i symmetric n x n, only the UPPER triangle of the column-major block holds data (the triangle potrf
//   reads and syrk / potri write); X_i, B_i, Y_i n x nrhs column-major, the right-hand-side layout of potrs; 0 <= n <= 256, any nrhs >= 0.
// ONE launch per fixed-size call on a 1-D grid, one per occurring size class on a plan; the passes over nrhs (16 columns each) stay inside
// the launch.  No scratch, no allocation, no memset, no atomics, no mutex, no helper stream, no host synchronisation, nothing between
// workgroups; 64-bit offsets; kernel launches only.
//
// THE ARITHMETIC, the same on both paths.  s_ij = sum_k a_ik x_kj over the symmetrised row - a_ik is element (min(i, k), max(i, k)) of the
// triangle - on the fp64 16 x 16 x 4 MFMA from a ZERO accumulator, K ascending, four k per instruction; rows and columns at or beyond n are
// supplied as +0.0 and never addressed (a wavefront that carries blocks of several sizes runs the steps of its largest: the further
// products are +0.0 * +0.0 and leave every bit alone, the accumulator of a chain that starts at +0.0 is never -0.0).  Then, without
// contraction:   t = alpha * s;   out = (beta == 0) ? t : fma(beta, b, t).
// beta == 0 never reads B.  alpha == 0 never addresses A or X (s = +0.0).  absolute = 1 takes |.| of every element of A, X and B on load.
// The strictly lower triangle of A is never read, inside diagonal tiles too; rows n .. ld - 1, the gaps between blocks and everything behind
// the last block are never read or written.  Y may be EXACTLY B (same pointer, ld and stride: every element is read by the lane that then
// writes it) or disjoint from it; Y must not overlap A or X (refused); any other overlap of an output with an input is undefined.
//
// THE TILES.  A tile is 16 rows of Y by 16 right-hand sides, computed TRANSPOSED (tools/mfma_f64_probe.hip): the A operand of the MFMA is
// the slab of X (lane l supplies x(k0 + l / 16, c0 + l % 16)), the B operand the slab of the symmetrised block (lane l supplies
// a(row l % 16, k0 + l / 16): 16 lanes read 128 contiguous bytes where k >= row, a strided column piece where k < row), so that lane l
// holds, in accumulator register r, element (row l % 16, column c0 + l / 16 + 4 r) and 16 lanes store 128 contiguous bytes of a column of Y.
// n <= 64: a wavefront per 64 / NP blocks of NP = 8 / 16 / 32 / 64 rows, block after block (two 8-row blocks share a tile: each is multiplied
// with its own X while the rows of the other enter as +0.0, and every lane keeps the accumulator of its own block).  64 < n <= 256: a
// workgroup of BB_THREADS per block, wave w owns the 16-row slabs w, w + 4, w + 8, w + 12 and streams their whole symmetrised rows.
//
// THE FUSED MODES of the same pass, so that A is streamed once:
//   NORM     the column 1-norms: the absolute product with a column of ones the kernel supplies itself, then the maximum (cap_dlansy's
//            definition; by symmetry the 1-norm and the infinity norm).  A NaN in the triangle gives NaN.
//   RESID    r = b - A x (alpha = -1, beta = 1) and s = |A||x| + |b| (absolute, alpha = beta = 1) from the same loads, two accumulators;
//            per column berr_j = max_i of cap_dpoerr's guarded ratio (s_i > safe2 ? |r_i| / s_i : (|r_i| + safe1) / (s_i + safe1),
//            safe1 = (n + 1) safmin, safe2 = safe1 / eps, eps = 2^-53, safmin = 2^-1022) and w_i = |r_i| + t s_i with t = (n + 1) eps, one
//            rounded multiplication, then one rounded addition, no fma; w goes to `work`.
//   ROWMAX   max_i y_ij of the absolute product divided by max_i |x_ij| of the SOLUTION (x_j = 0: the numerator alone, as cap_dpoerr): ferr.
// The maxima propagate NaN and are order-independent (all candidates are >= +0.0).
//
// THE BIT CONTRACTS.  1. PLAN = FIXED: every block of a plan call gets the bits of the fixed-size entry on it alone with batch = 1 (Y, the
// norm, rcond, ferr, berr).  2. LAYOUT INDEPENDENCE: a block's bits are a function of (n, its data, alpha, beta, absolute) only - not of
// batch, index, any ld / stride or the alignment.  3. COLUMN INDEPENDENCE: a column of Y, and its ferr / berr, do not depend on the columns
// that travel with it or on the pass it falls in - every element of Y is its own chain over k from a zero accumulator and the epilogue is
// elementwise.  4. COMPOSITION: norm1 = max of symm(absolute) against ones; rcond = 1 / (anorm * norm1(potri(copy of R))); berr and ferr =
// the formulas above on symm's outputs - the fused modes run the very chains of the plain product.
// 1 - 3 rest on the MFMA computing every element of a tile alike, as in syrk_batched.hip.
// SHARED (vbatch_plan.h): the operand rule, the grid and the dispatch of the entry points, the walk over a plan's classes.
#include <vector>

#include "batched_blocked.h"
#include "capital_amd.h"
#include "vbatch_plan.h"

namespace {

constexpr int SY_MAX = 256;
constexpr int SY_PROD = 0, SY_NORM = 1, SY_RESID = 2, SY_ROWMAX = 3;
constexpr double SY_EPS = 0x1p-53;
constexpr double SY_SAFMIN = 0x1p-1022;

struct SyArgs {
  const double* A; int64_t lda, stride_a;        // stride_*: fixed size only
  const double* X; int64_t ldx, stride_x;
  const double* B; int64_t ldb, stride_b;
  double* Y; int64_t ldy, stride_y;              // RESID: w (may be null)
  const double* S; int64_t lds, stride_s;        // ROWMAX: the solution whose column maxima divide
  double* out; int64_t lde;                      // NORM: out[i]; RESID: berr, ROWMAX: ferr at i lde + j (may be null)
  const int* info;
  double alpha, beta;
  int64_t batch, nrhs;
  int n, absolute, kon;                          // kon = 0: alpha == 0, A and X are not addressed
  const VbRec* rec;                              // plan: one class of one call
  const int64_t* list; int64_t count;
};

struct SyBlk {                                   // one block, wave-uniform; n = 0: no block
  const double* a; int64_t lda;
  const double* x; const double* b; double* y; const double* s;
  int64_t idx; int n;
};

template <bool PLAN>
__device__ __forceinline__ SyBlk sy_block(const SyArgs& g, const int64_t at) {
  SyBlk b;
  b.a = g.A; b.lda = 1; b.x = g.X; b.b = g.B; b.y = g.Y; b.s = g.S; b.idx = 0; b.n = 0;
  if constexpr (PLAN) {
    if (at < g.count) {
      const int64_t blk = g.list[at];
      const VbRec r = g.rec[blk];
      b.n = (int)r.n; b.idx = blk; b.a = g.A + r.off; b.lda = r.ld;
      b.x = g.X + r.row; b.b = g.B + r.row; b.y = g.Y + r.row; b.s = g.S + r.row;
    }
  } else {
    if (at < g.batch) {
      b.n = g.n; b.idx = at; b.a = g.A + at * g.stride_a; b.lda = g.lda;
      b.x = g.X + at * g.stride_x; b.b = g.B + at * g.stride_b; b.y = g.Y + at * g.stride_y; b.s = g.S + at * g.stride_s;
    }
  }
  return b;
}

// the epilogue of one element, without contraction: t = alpha s; out = beta == 0 ? t : fma(beta, b, t)
__device__ __forceinline__ double sy_combine(const double alpha, const double beta, const double s, const double b) {
#pragma clang fp contract(off)
  const double t = alpha * s;
  double out = t;
  if (beta != 0.0) out = __builtin_fma(beta, b, t);
  return out;
}

// w = |r| + t s: one rounded multiplication, one rounded addition
__device__ __forceinline__ double sy_weight(const double r, const double t, const double s) {
#pragma clang fp contract(off)
  const double p = t * s;
  return r + p;
}

// the larger of two values that are >= +0.0 or NaN; a NaN stays
__device__ __forceinline__ double sy_max(const double a, const double b) {
  if (a != a || b != b) return __builtin_nan("");
  return a > b ? a : b;
}

// the maximum over the ROWS lanes that hold the rows of one block in a tile (lane bits 0 .. 3 are the row)
template <int ROWS>
__device__ __forceinline__ double sy_row_max(double v) {
#pragma unroll
  for (int o = 1; o < ROWS; o <<= 1) v = sy_max(v, __shfl_xor(v, o));
  return v;
}

// S slabs of 16 rows (slab s: rows row0 + s step .. + 15) against every right-hand side, 16 columns a pass, by one wavefront.
// H = 1: the slabs belong to block b0.  H = 2 (S = 1): rows 0 .. 7 of the slab are block b0, rows 8 .. 15 block b1, 8 rows each.
// kend: the k steps end here (wave-uniform, a multiple of 4, 0 with alpha == 0).  red: LDS of a workgroup (the maxima of its waves) or null.
template <int MODE, int S, int H>
__device__ __forceinline__ void sy_rows(const SyArgs& g, const SyBlk& b0, const SyBlk& b1, const int row0, const int step, const int kend, const int nlive,
                                        const int lr, const int kg, const int wave, double* red) {
  static_assert(H == 1 || S == 1, "two blocks share one slab only");
  constexpr int ROWS = H == 2 ? 8 : 16;
  const int mine = H == 2 ? lr >> 3 : 0;                 // which of the blocks this lane's row belongs to
  SyBlk me = b0;
  if constexpr (H == 2) {
    if (mine) me = b1;
  }
  const bool absolute = MODE == SY_NORM || MODE == SY_ROWMAX || (MODE == SY_PROD && g.absolute);
  const double alpha = MODE == SY_PROD ? g.alpha : 1.0, beta = MODE == SY_PROD ? g.beta : 0.0;
  int row[S];
  bool on[S], live[S];
#pragma unroll
  for (int s = 0; s < S; s++) {
    row[s] = row0 + s * step + (H == 2 ? (lr & 7) : lr);
    on[s] = row0 + s * step < nlive;                     // wave-uniform
    live[s] = row[s] < me.n;
  }
  const int64_t npass = MODE == SY_NORM ? 1 : (g.nrhs + 15) >> 4;
  for (int64_t pass = 0; pass < npass; pass++) {
    const int64_t c0 = pass << 4;
    d4 acc[H][S], acc2[H][S];                            // acc2: RESID only, |A||x|
#pragma unroll
    for (int s = 0; s < S; s++) {
#pragma unroll
      for (int h = 0; h < H; h++) {
        acc[h][s] = (d4){0.0, 0.0, 0.0, 0.0};
        acc2[h][s] = (d4){0.0, 0.0, 0.0, 0.0};
      }
    }
    const bool colx = c0 + lr < g.nrhs;                  // this lane's column of the X slab exists
    for (int k0 = 0; k0 < kend; k0 += 4) {
      const int k = k0 + kg;
      double xv[H];
#pragma unroll
      for (int h = 0; h < H; h++) {
        const SyBlk& bh = h == 0 ? b0 : b1;
        double v = 0.0;
        if constexpr (MODE == SY_NORM) {
          if (lr == 0 && k < bh.n) v = 1.0;
        } else {
          if (colx && k < bh.n) v = bh.x[k + (c0 + lr) * g.ldx];
        }
        xv[h] = absolute ? __builtin_fabs(v) : v;
      }
#pragma unroll
      for (int s = 0; s < S; s++) {
        if (on[s]) {
          double av = 0.0;
          if (live[s] && k < me.n) {
            const int lo = row[s] < k ? row[s] : k, hi = row[s] < k ? k : row[s];
            av = me.a[lo + (int64_t)hi * me.lda];
          }
          if (absolute) av = __builtin_fabs(av);
#pragma unroll
          for (int h = 0; h < H; h++) {
            const double ah = (H == 1 || mine == h) ? av : 0.0;
            acc[h][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[h], ah, acc[h][s], 0, 0, 0);
            if constexpr (MODE == SY_RESID)
              acc2[h][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(__builtin_fabs(xv[h]), __builtin_fabs(ah), acc2[h][s], 0, 0, 0);
          }
        }
      }
    }

    // lane (lr, kg), register r of slab s: row row[s], column c0 + kg + 4 r
    double top[4] = {0.0, 0.0, 0.0, 0.0}, xm[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < S; s++) {
      if (on[s]) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int64_t col = c0 + kg + 4 * r;
          const double sum = H == 2 ? (mine ? acc[H - 1][s][r] : acc[0][s][r]) : acc[0][s][r];
          if constexpr (MODE == SY_NORM) {
            if (live[s] && r == 0 && kg == 0) top[0] = sy_max(top[0], sy_combine(1.0, 0.0, sum, 0.0));
          } else if (live[s] && col < g.nrhs) {
            if constexpr (MODE == SY_PROD) {
              double bv = 0.0;
              if (beta != 0.0) { bv = me.b[row[s] + col * g.ldb]; if (absolute) bv = __builtin_fabs(bv); }
              me.y[row[s] + col * g.ldy] = sy_combine(alpha, beta, sum, bv);
            } else if constexpr (MODE == SY_RESID) {
              const double bv = me.b[row[s] + col * g.ldb];
              const double res = __builtin_fabs(sy_combine(-1.0, 1.0, sum, bv));
              const double sum2 = H == 2 ? (mine ? acc2[H - 1][s][r] : acc2[0][s][r]) : acc2[0][s][r];
              const double den = sy_combine(1.0, 1.0, sum2, __builtin_fabs(bv));
              const double nz = (double)(me.n + 1), safe1 = nz * SY_SAFMIN, safe2 = safe1 / SY_EPS;
              const double q = den > safe2 ? res / den : (res + safe1) / (den + safe1);
              top[r] = sy_max(top[r], q);
              if (g.Y) me.y[row[s] + col * g.ldy] = sy_weight(res, nz * SY_EPS, den);
            } else {
              top[r] = sy_max(top[r], sy_combine(1.0, 0.0, sum, 0.0));
              xm[r] = sy_max(xm[r], __builtin_fabs(me.s[row[s] + col * g.lds]));
            }
          }
        }
      }
    }
    if constexpr (MODE != SY_PROD) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (MODE == SY_NORM && r > 0) break;
        top[r] = sy_row_max<ROWS>(top[r]);
        if constexpr (MODE == SY_ROWMAX) xm[r] = sy_row_max<ROWS>(xm[r]);
      }
      if (red) {                                         // a workgroup: the maxima of its waves meet in LDS
        if (lr == 0) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            red[wave * 16 + kg + 4 * r] = top[r];
            red[(BB_WAVES + wave) * 16 + kg + 4 * r] = xm[r];
          }
        }
        __syncthreads();
        if (wave == 0 && lr == 0) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            top[r] = red[kg + 4 * r]; xm[r] = red[BB_WAVES * 16 + kg + 4 * r];
#pragma unroll
            for (int w = 1; w < BB_WAVES; w++) {
              top[r] = sy_max(top[r], red[w * 16 + kg + 4 * r]);
              xm[r] = sy_max(xm[r], red[(BB_WAVES + w) * 16 + kg + 4 * r]);
            }
          }
        }
      }
      if ((lr & (ROWS - 1)) == 0 && wave == 0 && me.n > 0 && g.out) {
        const bool bad = g.info && g.info[me.idx] != 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int64_t col = c0 + kg + 4 * r;
          if constexpr (MODE == SY_NORM) {
            if (r == 0 && kg == 0) g.out[me.idx] = top[0];
          } else if (col < g.nrhs) {
            double v = top[r];
            if constexpr (MODE == SY_ROWMAX) v = xm[r] == 0.0 ? v : v / xm[r];
            g.out[me.idx * g.lde + col] = bad ? __builtin_nan("") : v;
          }
        }
      }
      if (red) __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------------ n <= 64: a wavefront per 64 / NP blocks
template <int MODE, int NP, bool PLAN>
__device__ __forceinline__ void sy_wave(const SyArgs& g) {
  constexpr int G = 64 / NP;
  const int lane = threadIdx.x, lr = lane & 15, kg = lane >> 4;
  const int64_t at0 = (int64_t)blockIdx.x * G;
  if constexpr (NP == 8) {
#pragma unroll 1
    for (int j = 0; j < G; j += 2) {
      const SyBlk b0 = sy_block<PLAN>(g, at0 + j), b1 = sy_block<PLAN>(g, at0 + j + 1);
      const int m = b0.n > b1.n ? b0.n : b1.n;
      if (m > 0) sy_rows<MODE, 1, 2>(g, b0, b1, 0, 0, g.kon ? (m + 3) & ~3 : 0, m, lr, kg, 0, nullptr);
    }
  } else {
#pragma unroll 1
    for (int j = 0; j < G; j++) {
      const SyBlk b0 = sy_block<PLAN>(g, at0 + j);
      if (b0.n > 0) sy_rows<MODE, NP / 16, 1>(g, b0, b0, 0, 16, g.kon ? (b0.n + 3) & ~3 : 0, b0.n, lr, kg, 0, nullptr);
    }
  }
}

template <int MODE, int NP>
__global__ __launch_bounds__(64) void symm_batched_kernel(SyArgs g) { sy_wave<MODE, NP, false>(g); }

template <int MODE, int NP>
__global__ __launch_bounds__(64) void symm_vbatched_kernel(SyArgs g) { sy_wave<MODE, NP, true>(g); }

// ------------------------------------------------------------------------------------------------ 64 < n <= 256: a workgroup per block
template <int MODE, bool PLAN>
__device__ __forceinline__ void sy_group(const SyArgs& g) {
  __shared__ double red[2 * BB_WAVES * 16];
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const SyBlk b0 = sy_block<PLAN>(g, (int64_t)blockIdx.x);
  const int n = b0.n;
  sy_rows<MODE, 4, 1>(g, b0, b0, wave * 16, 16 * BB_WAVES, g.kon ? (n + 3) & ~3 : 0, n, lr, kg, wave, MODE == SY_PROD ? nullptr : red);
}

template <int MODE>
__global__ __launch_bounds__(BB_THREADS) void symm_batched_blocked_kernel(SyArgs g) { sy_group<MODE, false>(g); }

template <int MODE>
__global__ __launch_bounds__(BB_THREADS) void symm_vbatched_blocked_kernel(SyArgs g) { sy_group<MODE, true>(g); }

// ------------------------------------------------------------------------------------------------ the copy of the factors, the last step of rcond
struct SyCopyArgs {
  const double* R; int64_t ldr, stride_r;
  double* W; int64_t ldw, stride_w;
  int64_t batch; int n, per;
  const VbRec* rec; const int64_t* list; int64_t count;
};

// the upper triangles of a workgroup's `per` blocks -> work (fixed size: ld n, n n apart; plan: the plan's own offsets and ld)
template <bool PLAN>
__global__ __launch_bounds__(BB_THREADS) void symm_copy_upper_kernel(SyCopyArgs g) {
  for (int j = 0; j < g.per; j++) {
    const int64_t at = (int64_t)blockIdx.x * g.per + j;
    const double* src; double* dst; int64_t lds, ldd; int n = 0;
    if constexpr (PLAN) {
      if (at >= g.count) return;
      const VbRec r = g.rec[g.list[at]];
      n = (int)r.n; src = g.R + r.off; dst = g.W + r.off; lds = r.ld; ldd = r.ld;
    } else {
      if (at >= g.batch) return;
      n = g.n; src = g.R + at * g.stride_r; dst = g.W + at * g.stride_w; lds = g.ldr; ldd = g.ldw;
    }
    for (int e = threadIdx.x; e < n * n; e += BB_THREADS) {
      const int c = e / n, r = e - c * n;
      if (r <= c) dst[r + (int64_t)c * ldd] = src[r + (int64_t)c * lds];
    }
  }
}

struct SyRcArgs {
  const double* anorm; double* rcond; const int* info; const VbRec* rec; int64_t batch;
};

// rcond[i] holds |A_i^-1|_1 and becomes 1 / (anorm_i * it): one multiplication, one correctly rounded division
__global__ __launch_bounds__(BB_THREADS) void symm_rcond_kernel(SyRcArgs g) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * BB_THREADS + threadIdx.x;
  if (i >= g.batch) return;
  if (g.rec && g.rec[i].n == 0) return;
  const double an = g.anorm[i], ai = g.rcond[i];
  double v;
  if (g.info && g.info[i] != 0) v = __builtin_nan("");
  else if (an != an) v = __builtin_nan("");
  else if (an == 0.0) v = 0.0;
  else v = 1.0 / (an * ai);
  g.rcond[i] = v;
}

// ------------------------------------------------------------------------------------------------ host
static inline bool sy_norm_ok(int norm) { return norm == '1' || norm == 'O' || norm == 'o' || norm == 'I' || norm == 'i'; }

// [first, last) of `batch` blocks of rows x cols
struct SySpan { const double* lo; const double* hi; };
static inline SySpan sy_span(const double* p, int64_t rows, int64_t cols, int64_t ld, int64_t stride, int64_t batch) {
  if (!p || rows <= 0 || cols <= 0 || batch <= 0) return {nullptr, nullptr};
  const __int128 last = (__int128)(batch - 1) * stride + (__int128)(cols - 1) * ld + rows;
  return {p, p + vb_clip(last)};
}
static inline bool sy_overlap(SySpan a, SySpan b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }

template <int MODE>
void sy_launch_fixed(const SyArgs& g, int64_t n, dim3 grid, hipStream_t s) {
  vb_with_int<8, 16, 32, 64>(vb_padded(n), [&](auto NP) {
    if (n <= BB_SMALL) hipLaunchKernelGGL((symm_batched_kernel<MODE, NP()>), grid, dim3(64), 0, s, g);
    else if (NP() == 64) hipLaunchKernelGGL((symm_batched_blocked_kernel<MODE>), grid, dim3(BB_THREADS), 0, s, g);
  });
}

template <int MODE>
void sy_launch_plan(const SyArgs& g, int cls, dim3 grid, hipStream_t s) {
  vb_with_int<8, 16, 32, 64>(cls < 4 ? 8 << cls : 64, [&](auto NP) {
    if (cls < 4) hipLaunchKernelGGL((symm_vbatched_kernel<MODE, NP()>), grid, dim3(64), 0, s, g);
    else if (NP() == 64) hipLaunchKernelGGL((symm_vbatched_blocked_kernel<MODE>), grid, dim3(BB_THREADS), 0, s, g);
  });
}

// the access notes of one block in one mode
void sy_note(int mode, const SyArgs& g, const double* a, int64_t lda, int64_t n, const double* x, const double* b, double* y, const double* sol,
             int64_t idx) {
  const int64_t nrhs = g.nrhs;
  if (g.kon) cap_acc_r(a, lda, n, n, 1);
  if (mode == SY_NORM) { cap_acc_w(g.out + idx, 0, 1, 1); return; }
  if (g.kon) cap_acc_r(x, g.ldx, n, nrhs);
  if (mode == SY_PROD) {
    if (g.beta != 0.0 && b == y) cap_acc_rw(y, g.ldy, n, nrhs);
    else {
      if (g.beta != 0.0) cap_acc_r(b, g.ldb, n, nrhs);
      cap_acc_w(y, g.ldy, n, nrhs);
    }
    return;
  }
  if (mode == SY_RESID) {
    cap_acc_r(b, g.ldb, n, nrhs);
    if (g.Y) cap_acc_w(y, g.ldy, n, nrhs);
  } else {
    cap_acc_r(sol, g.lds, n, nrhs);
  }
  if (g.out) {
    cap_acc_w(g.out + idx * g.lde, 0, nrhs, 1);
    if (g.info) cap_acc_r(g.info + idx, 0, 1, 1, 0, 4);
  }
}

// one launch of a mode on the fixed-size layout; the arguments have been checked
template <int MODE>
int sy_run_fixed(const SyArgs& g, hipStream_t s) {
  const int64_t n = g.n, nwg = vb_grid(g.batch, vb_per_group(vb_class(n)));
  if (cap_acc_on())
    for (int64_t i = 0; i < g.batch; i++)
      sy_note(MODE, g, g.A + i * g.stride_a, g.lda, n, g.X + i * g.stride_x, g.B + i * g.stride_b, g.Y + i * g.stride_y, g.S + i * g.stride_s, i);
  sy_launch_fixed<MODE>(g, n, dim3((unsigned)nwg), s);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

// one launch per occurring class of a mode on a plan
template <int MODE>
int sy_run_plan(const cap_vbatch_plan* p, SyArgs g, hipStream_t s) {
  g.rec = p->d_rec;
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    g.list = list;
    g.count = count;
    if (cap_acc_on())
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[(size_t)b];
        sy_note(MODE, g, g.A + r.off, r.ld, r.n, g.X + r.row, g.B + r.row, g.Y + r.row, g.S + r.row, b);
      }
    sy_launch_plan<MODE>(g, cls, grid, s);
  });
}

int sy_copy_fixed(int64_t n, const double* R, int64_t ldr, int64_t stride_r, double* W, int64_t batch, hipStream_t s) {
  SyCopyArgs c = {};
  c.R = R; c.ldr = ldr; c.stride_r = stride_r; c.W = W; c.ldw = n; c.stride_w = n * n; c.batch = batch; c.n = (int)n;
  c.per = vb_per_group(vb_class(n));
  if (cap_acc_on())
    for (int64_t i = 0; i < batch; i++) {
      cap_acc_r(R + i * stride_r, ldr, n, n, 1);
      cap_acc_w(W + i * n * n, n, n, n, 1);
    }
  hipLaunchKernelGGL(symm_copy_upper_kernel<false>, dim3((unsigned)vb_grid(batch, c.per)), dim3(BB_THREADS), 0, s, c);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int sy_copy_plan(const cap_vbatch_plan* p, const double* R, double* W, hipStream_t s) {
  SyCopyArgs c = {};
  c.R = R; c.W = W; c.rec = p->d_rec;
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    c.list = list; c.count = count; c.per = vb_per_group(cls);
    if (cap_acc_on())
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[(size_t)b];
        cap_acc_r(R + r.off, r.ld, r.n, r.n, 1);
        cap_acc_w(W + r.off, r.ld, r.n, r.n, 1);
      }
    hipLaunchKernelGGL(symm_copy_upper_kernel<true>, grid, dim3(BB_THREADS), 0, s, c);
  });
}

int sy_rcond(const cap_vbatch_plan* p, int64_t batch, const double* anorm, const int* info, double* rcond, hipStream_t s) {
  SyRcArgs c = {anorm, rcond, info, p ? p->d_rec : nullptr, batch};
  if (cap_acc_on()) {
    if (p) cap_acc_r(p->d_rec, 0, batch * (int64_t)(sizeof(VbRec) / 8), 1);
    for (int64_t i = 0; i < batch; i++) {
      if (p && p->rec[(size_t)i].n == 0) continue;
      cap_acc_r(anorm + i, 0, 1, 1);
      cap_acc_rw(rcond + i, 0, 1, 1);
      if (info) cap_acc_r(info + i, 0, 1, 1, 0, 4);
    }
  }
  hipLaunchKernelGGL(symm_rcond_kernel, dim3((unsigned)cap_ceil_div(batch, BB_THREADS)), dim3(BB_THREADS), 0, s, c);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

// the rules every fixed-size entry shares behind its own: the limits and the empty call.  > 0: return that - 1
int sy_limits(int uplo, int64_t n, int64_t batch) {
  if (uplo != CAP_UPPER) return 1 + CAP_ERR_UNSUPPORTED;      // as the other batched entries
  if (n > SY_MAX) return 1 + CAP_ERR_UNSUPPORTED;
  if (vb_grid(batch, vb_per_group(vb_class(n))) < 0) return 1 + CAP_ERR_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

int cap_dsymm_batched(int uplo, int absolute, int64_t n, int64_t nrhs, double alpha, const double* A, int64_t lda, int64_t stride_a,
                      const double* X, int64_t ldx, int64_t stride_x, double beta, const double* B, int64_t ldb, int64_t stride_b, double* Y,
                      int64_t ldy, int64_t stride_y, int64_t batch, void* stream) {
  if ((absolute != 0 && absolute != 1) || n < 0 || nrhs < 0 || batch < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && nrhs > 0 && batch > 0;
  if (work && !Y) return CAP_ERR_ARG;
  if (work && alpha != 0.0 && (!A || !X)) return CAP_ERR_ARG;
  if (work && beta != 0.0 && !B) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, lda, stride_a, batch) || !vb_operand_ok(n, nrhs, ldx, stride_x, batch) || !vb_operand_ok(n, nrhs, ldy, stride_y, batch))
    return CAP_ERR_ARG;
  if (beta != 0.0 && !vb_operand_ok(n, nrhs, ldb, stride_b, batch)) return CAP_ERR_ARG;
  if (alpha != 0.0) {
    const SySpan y = sy_span(Y, n, nrhs, ldy, stride_y, batch);
    if (sy_overlap(y, sy_span(A, n, n, lda, stride_a, batch)) || sy_overlap(y, sy_span(X, n, nrhs, ldx, stride_x, batch))) return CAP_ERR_ARG;
  }
  if (const int st = sy_limits(uplo, n, batch)) return st - 1;
  if (!work) return CAP_OK;
  SyArgs g = {};
  g.A = A; g.lda = lda; g.stride_a = stride_a; g.X = X; g.ldx = ldx; g.stride_x = stride_x; g.B = B; g.ldb = ldb; g.stride_b = stride_b;
  g.Y = Y; g.ldy = ldy; g.stride_y = stride_y; g.alpha = alpha; g.beta = beta; g.batch = batch; g.nrhs = nrhs; g.n = (int)n;
  g.absolute = absolute; g.kon = alpha != 0.0;
  return sy_run_fixed<SY_PROD>(g, cap_stream(stream));
}

int cap_dsymm_vbatched(const cap_vbatch_plan* p, int uplo, int absolute, int64_t nrhs, double alpha, const double* A, const double* X,
                       int64_t ldx, double beta, const double* B, int64_t ldb, double* Y, int64_t ldy, void* stream) {
  if (!p || (absolute != 0 && absolute != 1) || nrhs < 0) return CAP_ERR_ARG;
  const bool work = p->nonempty > 0 && nrhs > 0;
  if (work && !Y) return CAP_ERR_ARG;
  if (work && alpha != 0.0 && (!A || !X)) return CAP_ERR_ARG;
  if (work && beta != 0.0 && !B) return CAP_ERR_ARG;
  if (ldx < p->rows || ldy < p->rows || (beta != 0.0 && ldb < p->rows)) return CAP_ERR_ARG;
  if (alpha != 0.0) {
    const SySpan y = sy_span(Y, p->rows, nrhs, ldy, 0, 1);
    if (sy_overlap(y, sy_span(A, p->total, 1, p->total, 0, 1)) || sy_overlap(y, sy_span(X, p->rows, nrhs, ldx, 0, 1))) return CAP_ERR_ARG;
  }
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  SyArgs g = {};
  g.A = A; g.X = X; g.ldx = ldx; g.B = B; g.ldb = ldb; g.Y = Y; g.ldy = ldy; g.alpha = alpha; g.beta = beta; g.nrhs = nrhs;
  g.absolute = absolute; g.kon = alpha != 0.0;
  return sy_run_plan<SY_PROD>(p, g, cap_stream(stream));
}

int cap_dlansy_batched(int norm, int uplo, int64_t n, const double* A, int64_t lda, int64_t stride_a, int64_t batch, double* out, void* stream) {
  if (n < 0 || batch < 0) return CAP_ERR_ARG;
  if (n > 0 && batch > 0 && (!A || !out)) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, lda, stride_a, batch)) return CAP_ERR_ARG;
  if (!sy_norm_ok(norm)) return CAP_ERR_UNSUPPORTED;           // as cap_dlansy
  if (const int st = sy_limits(uplo, n, batch)) return st - 1;
  if (n == 0 || batch == 0) return CAP_OK;
  SyArgs g = {};
  g.A = A; g.lda = lda; g.stride_a = stride_a; g.out = out; g.batch = batch; g.nrhs = 1; g.n = (int)n; g.absolute = 1; g.kon = 1;
  return sy_run_fixed<SY_NORM>(g, cap_stream(stream));
}

int cap_dlansy_vbatched(const cap_vbatch_plan* p, int norm, int uplo, const double* A, double* out, void* stream) {
  if (!p) return CAP_ERR_ARG;
  if (p->nonempty > 0 && (!A || !out)) return CAP_ERR_ARG;
  if (!sy_norm_ok(norm)) return CAP_ERR_UNSUPPORTED;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (p->nonempty == 0) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  SyArgs g = {};
  g.A = A; g.out = out; g.nrhs = 1; g.absolute = 1; g.kon = 1;
  return sy_run_plan<SY_NORM>(p, g, cap_stream(stream));
}

int64_t cap_dpocon_batched_work_size(int64_t n, int64_t batch) {
  if (n <= 0 || batch <= 0) return 0;
  return vb_mul_clip(vb_mul_clip(n, n), batch);
}

int64_t cap_dpocon_vbatched_work_size(const cap_vbatch_plan* p) { return p ? p->total : -1; }

int cap_dpocon_batched(int uplo, int64_t n, const double* R, int64_t ldr, int64_t stride_r, int64_t batch, const double* anorm, const int* info,
                       double* rcond, double* work, void* stream) {
  if (n < 0 || batch < 0) return CAP_ERR_ARG;
  if (n > 0 && batch > 0 && (!R || !anorm || !rcond || !work)) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, ldr, stride_r, batch)) return CAP_ERR_ARG;
  if (const int st = sy_limits(uplo, n, batch)) return st - 1;
  if (n == 0 || batch == 0) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  CAP_TRY(sy_copy_fixed(n, R, ldr, stride_r, work, batch, s));
  CAP_TRY(cap_dpotri_batched(CAP_UPPER, n, work, n, n * n, batch, info, 0, stream));
  SyArgs g = {};
  g.A = work; g.lda = n; g.stride_a = n * n; g.out = rcond; g.batch = batch; g.nrhs = 1; g.n = (int)n; g.absolute = 1; g.kon = 1;
  CAP_TRY(sy_run_fixed<SY_NORM>(g, s));
  return sy_rcond(nullptr, batch, anorm, info, rcond, s);
}

int cap_dpocon_vbatched(const cap_vbatch_plan* p, int uplo, const double* R, const double* anorm, const int* info, double* rcond, double* work,
                        void* stream) {
  if (!p) return CAP_ERR_ARG;
  if (p->nonempty > 0 && (!R || !anorm || !rcond || !work)) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (p->nonempty == 0) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  CAP_TRY(sy_copy_plan(p, R, work, s));
  CAP_TRY(cap_dpotri_vbatched(p, CAP_UPPER, work, info, 0, stream));
  SyArgs g = {};
  g.A = work; g.out = rcond; g.nrhs = 1; g.absolute = 1; g.kon = 1;
  CAP_TRY(sy_run_plan<SY_NORM>(p, g, s));
  return sy_rcond(p, p->batch, anorm, info, rcond, s);
}

int64_t cap_dpoerr_batched_work_size(int64_t n, int64_t nrhs, int64_t batch) {
  if (n <= 0 || nrhs <= 0 || batch <= 0) return 0;
  return vb_mul_clip(vb_mul_clip(n, vb_clip((__int128)n + nrhs)), batch);
}

int64_t cap_dpoerr_vbatched_work_size(const cap_vbatch_plan* p, int64_t nrhs) {
  if (!p || nrhs < 0) return -1;
  return vb_clip((__int128)p->total + (__int128)p->rows * nrhs);
}

int cap_dpoerr_batched(int uplo, int64_t n, int64_t nrhs, const double* A, int64_t lda, int64_t stride_a, const double* R, int64_t ldr,
                       int64_t stride_r, const double* B, int64_t ldb, int64_t stride_b, const double* X, int64_t ldx, int64_t stride_x,
                       int64_t batch, const int* info, double* ferr, double* berr, int64_t lde, double* work, void* stream) {
  if (n < 0 || nrhs < 0 || batch < 0) return CAP_ERR_ARG;
  const bool any = n > 0 && nrhs > 0 && batch > 0 && (ferr || berr);
  if (any && (!A || !B || !X)) return CAP_ERR_ARG;
  if (any && ferr && (!R || !work)) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, lda, stride_a, batch) || (ferr && !vb_operand_ok(n, n, ldr, stride_r, batch)) ||
      !vb_operand_ok(n, nrhs, ldb, stride_b, batch) || !vb_operand_ok(n, nrhs, ldx, stride_x, batch))
    return CAP_ERR_ARG;
  if ((ferr || berr) && lde < nrhs) return CAP_ERR_ARG;
  if (const int st = sy_limits(uplo, n, batch)) return st - 1;
  if (!any) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  double* w = ferr ? work + n * n * batch : nullptr;            // the weights behind the copy of the factors: n x nrhs a block, ld n
  SyArgs g = {};
  g.A = A; g.lda = lda; g.stride_a = stride_a; g.X = X; g.ldx = ldx; g.stride_x = stride_x; g.B = B; g.ldb = ldb; g.stride_b = stride_b;
  g.Y = w; g.ldy = n; g.stride_y = n * nrhs; g.out = berr; g.lde = lde; g.info = info; g.batch = batch; g.nrhs = nrhs; g.n = (int)n; g.kon = 1;
  CAP_TRY(sy_run_fixed<SY_RESID>(g, s));
  if (!ferr) return CAP_OK;
  CAP_TRY(sy_copy_fixed(n, R, ldr, stride_r, work, batch, s));
  CAP_TRY(cap_dpotri_batched(CAP_UPPER, n, work, n, n * n, batch, info, 0, stream));
  SyArgs f = {};
  f.A = work; f.lda = n; f.stride_a = n * n; f.X = w; f.ldx = n; f.stride_x = n * nrhs; f.S = X; f.lds = ldx; f.stride_s = stride_x;
  f.out = ferr; f.lde = lde; f.info = info; f.batch = batch; f.nrhs = nrhs; f.n = (int)n; f.absolute = 1; f.kon = 1;
  return sy_run_fixed<SY_ROWMAX>(f, s);
}

int cap_dpoerr_vbatched(const cap_vbatch_plan* p, int uplo, int64_t nrhs, const double* A, const double* R, const double* B, int64_t ldb,
                        const double* X, int64_t ldx, const int* info, double* ferr, double* berr, int64_t lde, double* work, void* stream) {
  if (!p || nrhs < 0) return CAP_ERR_ARG;
  const bool any = p->nonempty > 0 && nrhs > 0 && (ferr || berr);
  if (any && (!A || !B || !X)) return CAP_ERR_ARG;
  if (any && ferr && (!R || !work)) return CAP_ERR_ARG;
  if (ldb < p->rows || ldx < p->rows) return CAP_ERR_ARG;
  if ((ferr || berr) && lde < nrhs) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;
  if (!any) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  hipStream_t s = cap_stream(stream);
  const int64_t ldw = p->rows;
  double* w = ferr ? work + p->total : nullptr;                 // the stacked weights behind the copy of the factors, ld sum n_i
  SyArgs g = {};
  g.A = A; g.X = X; g.ldx = ldx; g.B = B; g.ldb = ldb; g.Y = w; g.ldy = ldw; g.out = berr; g.lde = lde; g.info = info; g.nrhs = nrhs; g.kon = 1;
  CAP_TRY(sy_run_plan<SY_RESID>(p, g, s));
  if (!ferr) return CAP_OK;
  CAP_TRY(sy_copy_plan(p, R, work, s));
  CAP_TRY(cap_dpotri_vbatched(p, CAP_UPPER, work, info, 0, stream));
  SyArgs f = {};
  f.A = work; f.X = w; f.ldx = ldw; f.S = X; f.lds = ldx; f.out = ferr; f.lde = lde; f.info = info; f.nrhs = nrhs; f.absolute = 1; f.kon = 1;
  return sy_run_plan<SY_ROWMAX>(p, f, s);
}

}  // extern "C"
