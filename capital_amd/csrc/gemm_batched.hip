// Batched general products on the block layouts of the batched family (cap_dgemm_batched and, on a cap_vbatch_plan,
// cap_dgemm_vbatched_inner / cap_dgemm_vbatched_combine): for every block the column-major m x n block
//   C_i <- beta C_i + alpha op(A_i) op(B_i),   0 <= m, n <= 256, any k >= 0, two DIFFERENT operands - BLAS dgemm per block.
//   fixed     op(A_i) m x k, op(B_i) k x n, both transposes are layouts: the loader strides, nothing is copied.
//   inner     G_i <- beta G_i + alpha X_i^T Y_i with X (sum n_i) x m and Y (sum n_i) x n STACKED as the right-hand sides of cap_dpotrs_vbatched:
//             the contraction runs over the n_i rows of block i (X^T y, W_1^T W_2, V_i^T x).  The output size does not depend on the block, so
//             this is ONE launch whatever the plan's classes; an empty block is an empty sum, G_i <- beta G_i.
//   combine   C_i <- beta C_i + alpha V_i Z_i on the n_i rows of block i of the stacked (sum n_i) x nrhs matrix C, V the stacked (sum n_i) x k
//             matrix of cap_dcholupdate_vbatched, Z_i k x nrhs: one launch per occurring size class.
// ONE launch per fixed-size call on a 1-D grid; no scratch, no allocation, no memset, no atomics, no mutex, no helper stream, no host
// synchronisation, nothing between workgroups; 64-bit offsets.  The loop over k is inside the launch and k is never split across
// workgroups: a large k with few blocks leaves most of the chip idle (that would need atomics or scratch and is out of scope).
//
// THE ARITHMETIC, the same on every path.  s_rc = sum_q a_rq b_qc on the fp64 16 x 16 x 4 MFMA from a ZERO accumulator, K ascending, four
// per instruction; rows >= m, columns >= n and k-positions >= k enter as +0.0 and are never addressed (a wavefront of `inner` that carries
// blocks of several n_i runs the steps of its largest: the further products are +0.0 * +0.0 and leave every bit alone, the accumulator of
// a chain that starts at +0.0 is never -0.0).  Then, without contraction:
//   t = alpha * s;   out = (beta == 0) ? t : fma(beta, c_old, t).
// beta == 0 never reads C (NaN and Inf there do not propagate).  alpha == 0 or k == 0 never addresses A or B (s = +0.0).
//
// THE TILES (gemm_batched_addr.h holds every address and predicate, tests/test_gemm_batched_addr.py sweeps them on the CPU).  A tile is
// computed TRANSPOSED, as in syrk_batched.hip and symm_batched.hip: the slab of op(B) is the A operand of the MFMA (lane l supplies
// b(q + l / 16, column l % 16)), the slab of op(A) the B operand (lane l supplies a(row l % 16, q + l / 16)), so that lane l holds, in
// accumulator register r, element (row l % 16, column l / 16 + 4 r) and 16 lanes store 128 contiguous bytes of a column of C.  Both
// operands come straight from global memory.  max(m, n) <= 64: a wavefront per 64 / NP blocks, NP = 8 / 16 / 32 / 64 the padded
// max(m, n) (combine: the padded n_i of the class, NP columns of C a pass).  Above: a workgroup of BB_THREADS per block, the pieces of 64
// rows x 32 columns dealt round the four waves (two waves per SIMD, as syrk found necessary); every piece reads its slabs itself (from L2
// after the first time).  Slabs at or beyond m / n are skipped by wave-uniform branches.
//
// THE BIT CONTRACTS.  1. PLAN = FIXED: block i of `inner` has the bits of cap_dgemm_batched(CAP_TRANS, CAP_NOTRANS, m, n, n_i, batch = 1)
// on its rows, block i of `combine` those of cap_dgemm_batched(CAP_NOTRANS, CAP_NOTRANS, n_i, nrhs, k, batch = 1).  2. LAYOUT
// INDEPENDENCE: a block's bits are a function of (m, n, k, alpha, beta, its data) only.  3. TRANS IS A LAYOUT.  4. ELEMENT INDEPENDENCE:
// c_rc is the m = n = 1 product of row r of op(A) and column c of op(B): every output element is its own chain from a zero accumulator
// and the epilogue is elementwise.  5. COMPOSITION: the recurrence is the one syrk_batched.hip and symm_batched.hip state (same MFMA
// operand order, same K order, same epilogue), so gemm(N, T) with B = A has syrk's bits in the upper triangle and gemm(N, N) with the
// symmetrised block symm's.  1 - 3 hold by construction given 4; 4 rests on the MFMA computing every element of a tile alike.
// SHARED (vbatch_plan.h): the size classes, the operand rule, the grid limit, the walk over a plan's classes, the wave's maximum.
#include <vector>

#include "batched_blocked.h"
#include "capital_amd.h"
#include "gemm_batched_addr.h"
#include "vbatch_plan.h"

namespace {

constexpr int GM_U = 4;                          // k steps (of four) whose loads are issued together
constexpr int GM_FIXED = 0, GM_INNER = 1, GM_COMBINE = 2;

struct GmArgs {
  const double* A; int64_t a_si, a_sq, stride_a;   // strides along the rows of op(A) and along k (gm_stride_i / gm_stride_q)
  const double* B; int64_t b_si, b_sq, stride_b;   // along the columns of op(B) and along k
  double* C; int64_t ldc, stride_c;
  double alpha, beta;
  int64_t batch, k;                              // k: 0 when alpha == 0
  int m, n, kon;                                 // kon = 0: alpha == 0, A and B are not addressed
  const VbRec* rec;                              // plan: the records (inner: null when every block is empty)
  const int64_t* list; int64_t count;            // combine: one class of one call
};

struct GmBlk {                                   // one block as a lane sees it; m = n = 0: no block
  const double* a; const double* b; double* c;
  int64_t k; int m, n;
};

template <int MODE>
__device__ __forceinline__ GmBlk gm_block(const GmArgs& g, const int64_t at) {
  GmBlk b;
  b.a = g.A; b.b = g.B; b.c = g.C; b.k = 0; b.m = 0; b.n = 0;
  if constexpr (MODE == GM_FIXED) {
    if (at < g.batch) {
      b.m = g.m; b.n = g.n; b.k = g.k;
      b.a = g.A + at * g.stride_a; b.b = g.B + at * g.stride_b; b.c = g.C + at * g.stride_c;
    }
  } else if constexpr (MODE == GM_INNER) {
    if (at < g.batch) {
      b.m = g.m; b.n = g.n; b.c = g.C + at * g.stride_c;
      if (g.rec && g.kon) {
        const VbRec r = g.rec[at];
        b.k = r.n; b.a = g.A + r.row; b.b = g.B + r.row;
      }
    }
  } else {
    if (at < g.count) {
      const int64_t blk = g.list[at];
      const VbRec r = g.rec[blk];
      b.m = (int)r.n; b.n = g.n; b.k = g.k;
      b.a = g.A + r.row; b.b = g.B + blk * g.stride_b; b.c = g.C + r.row;
    }
  }
  return b;
}

// the epilogue of one element, without contraction: t = alpha s; out = beta == 0 ? t : fma(beta, c_old, t)
__device__ __forceinline__ double gm_combine(const double alpha, const double beta, const double s, const double* c) {
#pragma clang fp contract(off)
  const double t = alpha * s;
  double out = t;
  if (beta != 0.0) out = __builtin_fma(beta, *c, t);
  return out;
}

// Four row slabs (rows I0 .. of op(A)) against NJ column slabs (columns J0 .. of op(B)) by one wavefront.  NP < 64: wave row / column
// w = 16 s + l % 16 is row / column base + w % NP of block w / NP of the wavefront's 64 / NP blocks - b[s] is that block as this lane sees
// it.  NP = 64: b[0 .. 3] are one block.  mmax, nmax, kmax: the largest of the wavefront (wave-uniform).
template <int NP, int NJ>
__device__ __forceinline__ void gm_macro(const GmArgs& g, const GmBlk (&b)[4], const int I0, const int J0, const int mmax, const int nmax, const int64_t kmax,
                                         const int lane) {
  static_assert(NJ <= 4, "b[] has four entries");
  bool ona[4], onb[NJ];
#pragma unroll
  for (int s = 0; s < 4; s++) ona[s] = gm_slab_on(NP, I0, s, mmax);
#pragma unroll
  for (int s = 0; s < NJ; s++) onb[s] = gm_slab_on(NP, J0, s, nmax);
  d4 acc[4][NJ];
#pragma unroll
  for (int si = 0; si < 4; si++)
#pragma unroll
    for (int sj = 0; sj < NJ; sj++) acc[si][sj] = (d4){0.0, 0.0, 0.0, 0.0};

  int64_t q = 0;
  for (; q + 4 * GM_U <= kmax; q += 4 * GM_U) {    // whole groups of steps
    double av[GM_U][4], bv[GM_U][NJ];
#pragma unroll
    for (int u = 0; u < GM_U; u++) {
#pragma unroll
      for (int s = 0; s < 4; s++) {
        double t = 0.0;
        if (ona[s]) {
          const GmAt at = gm_load_at(g.a_si, g.a_sq, b[s].m, b[s].k, NP, I0, s, lane, q + 4 * u);
          if (at.on) t = b[s].a[at.off];
        }
        av[u][s] = t;
      }
#pragma unroll
      for (int s = 0; s < NJ; s++) {
        double t = 0.0;
        if (onb[s]) {
          const GmAt at = gm_load_at(g.b_si, g.b_sq, b[s].n, b[s].k, NP, J0, s, lane, q + 4 * u);
          if (at.on) t = b[s].b[at.off];
        }
        bv[u][s] = t;
      }
    }
#pragma unroll
    for (int u = 0; u < GM_U; u++) {
#pragma unroll
      for (int si = 0; si < 4; si++) {
#pragma unroll
        for (int sj = 0; sj < NJ; sj++) {
          if (gm_tile(NP, si, sj)) {
            if (ona[si] && onb[sj]) acc[si][sj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[u][sj], av[u][si], acc[si][sj], 0, 0, 0);
          }
        }
      }
    }
  }
  for (; q < kmax; q += 4) {                       // the tail: positions at or beyond k are +0.0
    double av[4], bv[NJ];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      double t = 0.0;
      if (ona[s]) {
        const GmAt at = gm_load_at(g.a_si, g.a_sq, b[s].m, b[s].k, NP, I0, s, lane, q);
        if (at.on) t = b[s].a[at.off];
      }
      av[s] = t;
    }
#pragma unroll
    for (int s = 0; s < NJ; s++) {
      double t = 0.0;
      if (onb[s]) {
        const GmAt at = gm_load_at(g.b_si, g.b_sq, b[s].n, b[s].k, NP, J0, s, lane, q);
        if (at.on) t = b[s].b[at.off];
      }
      bv[s] = t;
    }
#pragma unroll
    for (int si = 0; si < 4; si++) {
#pragma unroll
      for (int sj = 0; sj < NJ; sj++) {
        if (gm_tile(NP, si, sj)) {
          if (ona[si] && onb[sj]) acc[si][sj] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv[sj], av[si], acc[si][sj], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int si = 0; si < 4; si++) {
#pragma unroll
    for (int sj = 0; sj < NJ; sj++) {
      if (gm_tile(NP, si, sj)) {
        if (ona[si] && onb[sj]) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const GmAt at = gm_store_at(b[si].m, b[si].n, g.ldc, NP, I0, J0, si, sj, lane, r);
            if (at.on) {
              double* c = b[si].c + at.off;
              *c = gm_combine(g.alpha, g.beta, acc[si][sj][r], c);
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ max(m, n) <= 64: a wavefront per 64 / NP blocks
template <int NP, int MODE>
__device__ __forceinline__ void gm_wave(const GmArgs& g) {
  constexpr int G = 64 / NP;
  const int lane = threadIdx.x, lr = lane & 15;
  GmBlk b[4];
  int mm = 0, kk = 0;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    b[s] = gm_block<MODE>(g, (int64_t)blockIdx.x * G + gm_sub(NP, s * 16 + lr));
    mm = b[s].m > mm ? b[s].m : mm;
    kk = (int)b[s].k > kk ? (int)b[s].k : kk;      // inner: n_i <= 256
  }
  int mmax = g.m;
  int64_t kmax = g.k;
  if constexpr (MODE == GM_INNER) kmax = vb_wave_max(kk);
  if constexpr (MODE == GM_COMBINE) mmax = vb_wave_max(mm);
  const int np = gm_wave_passes(NP, g.n);
  for (int pass = 0; pass < np; pass++) gm_macro<NP, 4>(g, b, 0, pass * NP, mmax, g.n, kmax, lane);
}

template <int NP, int MODE>
__global__ __launch_bounds__(64) void gemm_batched_kernel(GmArgs g) { gm_wave<NP, MODE>(g); }

// ------------------------------------------------------------------------------------------------ above: a workgroup per block
template <int MODE>
__device__ __forceinline__ void gm_group(const GmArgs& g) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const GmBlk b0 = gm_block<MODE>(g, (int64_t)blockIdx.x);
  const GmBlk b[4] = {b0, b0, b0, b0};
  const int m = __builtin_amdgcn_readfirstlane(b0.m), n = __builtin_amdgcn_readfirstlane(b0.n);
  const int nt = gm_group_tiles(m, n);
  for (int t = wave; t < nt; t += BB_WAVES) gm_macro<64, GM_GROUP_NJ>(g, b, gm_group_I0(t, m), gm_group_J0(t, m), m, n, b0.k, lane);
}

template <int MODE>
__global__ __launch_bounds__(BB_THREADS, 2) void gemm_batched_blocked_kernel(GmArgs g) { gm_group<MODE>(g); }

// ------------------------------------------------------------------------------------------------ host
static_assert(GM_ROWS == BB_SMALL && GM_MAX == BB_MAX, "the wave path ends where the other batched entries' does");

template <int MODE>
void gm_launch(const GmArgs& g, int np, bool group, dim3 grid, hipStream_t s) {
  if (group) {
    hipLaunchKernelGGL((gemm_batched_blocked_kernel<MODE>), grid, dim3(BB_THREADS), 0, s, g);
    return;
  }
  vb_with_int<8, 16, 32, 64>(np, [&](auto NP) { hipLaunchKernelGGL((gemm_batched_kernel<NP(), MODE>), grid, dim3(64), 0, s, g); });
}

// [first, last) of `batch` blocks of rows x cols (as symm_batched.hip's refusal of an output that overlaps an input)
struct GmSpan { const double* lo; const double* hi; };
static inline GmSpan gm_span(const double* p, int64_t rows, int64_t cols, int64_t ld, int64_t stride, int64_t batch) {
  if (!p || rows <= 0 || cols <= 0 || batch <= 0) return {nullptr, nullptr};
  const __int128 last = (__int128)(batch - 1) * stride + (__int128)(cols - 1) * ld + rows;
  return {p, p + vb_clip(last)};
}
static inline bool gm_overlap(GmSpan a, GmSpan b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }

static inline bool gm_trans_ok(int t) { return t == CAP_NOTRANS || t == CAP_TRANS; }

int gm_fixed(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha, const double* A, int64_t lda, int64_t stride_a, const double* B,
             int64_t ldb, int64_t stride_b, double beta, double* C, int64_t ldc, int64_t stride_c, int64_t batch, hipStream_t s) {
  if (!gm_trans_ok(transa) || !gm_trans_ok(transb) || m < 0 || n < 0 || k < 0 || batch < 0) return CAP_ERR_ARG;
  const bool work = m > 0 && n > 0 && batch > 0;
  if (!C && work) return CAP_ERR_ARG;
  if ((!A || !B) && work && k > 0 && alpha != 0.0) return CAP_ERR_ARG;
  const int64_t arows = transa == CAP_TRANS ? k : m, acols = transa == CAP_TRANS ? m : k;
  const int64_t brows = transb == CAP_TRANS ? n : k, bcols = transb == CAP_TRANS ? k : n;
  if (!vb_operand_ok(m, n, ldc, stride_c, batch) || !vb_operand_ok(arows, acols, lda, stride_a, batch) ||
      !vb_operand_ok(brows, bcols, ldb, stride_b, batch))
    return CAP_ERR_ARG;
  if (alpha != 0.0 && k > 0) {
    const GmSpan c = gm_span(C, m, n, ldc, stride_c, batch);
    if (gm_overlap(c, gm_span(A, arows, acols, lda, stride_a, batch)) || gm_overlap(c, gm_span(B, brows, bcols, ldb, stride_b, batch)))
      return CAP_ERR_ARG;
  }
  if (m > GM_MAX || n > GM_MAX) return CAP_ERR_UNSUPPORTED;
  const int64_t big = m > n ? m : n;
  const bool group = big > BB_SMALL;
  const int np = vb_padded(big);
  const int64_t nwg = vb_grid(batch, group ? 1 : 64 / np);
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  if (!work) return CAP_OK;
  const int64_t keff = alpha == 0.0 ? 0 : k;
  if (cap_acc_on()) {
    for (int64_t i = 0; i < batch; i++) {
      if (keff > 0) {
        cap_acc_r(A + i * stride_a, lda, arows, acols);
        cap_acc_r(B + i * stride_b, ldb, brows, bcols);
      }
      if (beta == 0.0) cap_acc_w(C + i * stride_c, ldc, m, n);
      else cap_acc_rw(C + i * stride_c, ldc, m, n);
    }
  }
  GmArgs g = {};
  g.A = A; g.a_si = gm_stride_i(transa == CAP_TRANS, lda); g.a_sq = gm_stride_q(transa == CAP_TRANS, lda); g.stride_a = stride_a;
  g.B = B; g.b_si = gm_stride_i(transb == CAP_NOTRANS, ldb); g.b_sq = gm_stride_q(transb == CAP_NOTRANS, ldb); g.stride_b = stride_b;
  g.C = C; g.ldc = ldc; g.stride_c = stride_c; g.alpha = alpha; g.beta = beta; g.batch = batch; g.k = keff; g.m = (int)m; g.n = (int)n;
  g.kon = keff > 0;
  gm_launch<GM_FIXED>(g, np, group, dim3((unsigned)nwg), s);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int gm_inner(const cap_vbatch_plan* p, int64_t m, int64_t n, double alpha, const double* X, int64_t ldx, const double* Y, int64_t ldy, double beta,
             double* G, int64_t ldg, int64_t stride_g, hipStream_t s) {
  if (!p || m < 0 || n < 0) return CAP_ERR_ARG;
  const bool work = p->batch > 0 && m > 0 && n > 0;
  if (work && !G) return CAP_ERR_ARG;
  if (work && p->rows > 0 && alpha != 0.0 && (!X || !Y)) return CAP_ERR_ARG;
  if (ldx < p->rows || ldy < p->rows) return CAP_ERR_ARG;
  if (!vb_operand_ok(m, n, ldg, stride_g, p->batch)) return CAP_ERR_ARG;
  if (m > GM_MAX || n > GM_MAX) return CAP_ERR_UNSUPPORTED;
  const int64_t big = m > n ? m : n;
  const bool group = big > BB_SMALL;
  const int np = vb_padded(big);
  const int64_t nwg = vb_grid(p->batch, group ? 1 : 64 / np);
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  const bool kon = alpha != 0.0 && p->rows > 0;
  if (cap_acc_on()) {
    if (kon) cap_acc_r(p->d_rec, 0, p->batch * (int64_t)(sizeof(VbRec) / 8), 1);
    for (int64_t i = 0; i < p->batch; i++) {
      const VbRec& r = p->rec[(size_t)i];
      if (kon && r.n > 0) {
        cap_acc_r(X + r.row, ldx, r.n, m);
        cap_acc_r(Y + r.row, ldy, r.n, n);
      }
      if (beta == 0.0) cap_acc_w(G + i * stride_g, ldg, m, n);
      else cap_acc_rw(G + i * stride_g, ldg, m, n);
    }
  }
  GmArgs g = {};
  g.A = X; g.a_si = gm_stride_i(true, ldx); g.a_sq = gm_stride_q(true, ldx);
  g.B = Y; g.b_si = gm_stride_i(true, ldy); g.b_sq = gm_stride_q(true, ldy);
  g.C = G; g.ldc = ldg; g.stride_c = stride_g; g.alpha = alpha; g.beta = beta; g.batch = p->batch; g.m = (int)m; g.n = (int)n;
  g.kon = kon; g.rec = kon ? p->d_rec : nullptr;
  gm_launch<GM_INNER>(g, np, group, dim3((unsigned)nwg), s);
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

int gm_combine_plan(const cap_vbatch_plan* p, int64_t nrhs, int64_t k, double alpha, const double* V, int64_t ldv, const double* Z, int64_t ldz,
                    int64_t stride_z, double beta, double* C, int64_t ldc, hipStream_t s) {
  if (!p || nrhs < 0 || k < 0) return CAP_ERR_ARG;
  const bool work = p->nonempty > 0 && nrhs > 0;
  if (work && !C) return CAP_ERR_ARG;
  if (work && k > 0 && alpha != 0.0 && (!V || !Z)) return CAP_ERR_ARG;
  if (ldv < p->rows || ldc < p->rows) return CAP_ERR_ARG;
  if (!vb_operand_ok(k, nrhs, ldz, stride_z, p->batch)) return CAP_ERR_ARG;
  if (nrhs > GM_MAX) return CAP_ERR_UNSUPPORTED;
  if (!work) return CAP_OK;
  if (p->device < 0) return CAP_ERR_HIP;
  const int64_t keff = alpha == 0.0 ? 0 : k;
  GmArgs g = {};
  g.A = V; g.a_si = gm_stride_i(false, ldv); g.a_sq = gm_stride_q(false, ldv);
  g.B = Z; g.b_si = gm_stride_i(true, ldz); g.b_sq = gm_stride_q(true, ldz); g.stride_b = stride_z;
  g.C = C; g.ldc = ldc; g.alpha = alpha; g.beta = beta; g.k = keff; g.n = (int)nrhs; g.kon = keff > 0; g.rec = p->d_rec;
  return vb_for_each_class(p, [&](int cls, const int64_t* list, int64_t count, const std::vector<int64_t>& blocks, dim3 grid) {
    g.list = list;
    g.count = count;
    if (cap_acc_on()) {
      for (int64_t b : blocks) {
        const VbRec& r = p->rec[(size_t)b];
        if (keff > 0) {
          cap_acc_r(V + r.row, ldv, r.n, k);
          cap_acc_r(Z + b * stride_z, ldz, k, nrhs);
        }
        if (beta == 0.0) cap_acc_w(C + r.row, ldc, r.n, nrhs);
        else cap_acc_rw(C + r.row, ldc, r.n, nrhs);
      }
    }
    gm_launch<GM_COMBINE>(g, cls < 4 ? 8 << cls : 64, cls >= 4, grid, s);
  });
}

}  // namespace

extern "C" {

int cap_dgemm_batched(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha, const double* A, int64_t lda, int64_t stride_a,
                      const double* B, int64_t ldb, int64_t stride_b, double beta, double* C, int64_t ldc, int64_t stride_c, int64_t batch,
                      void* stream) {
  return gm_fixed(transa, transb, m, n, k, alpha, A, lda, stride_a, B, ldb, stride_b, beta, C, ldc, stride_c, batch, cap_stream(stream));
}

int cap_dgemm_vbatched_inner(const cap_vbatch_plan* p, int64_t m, int64_t n, double alpha, const double* X, int64_t ldx, const double* Y,
                             int64_t ldy, double beta, double* G, int64_t ldg, int64_t stride_g, void* stream) {
  return gm_inner(p, m, n, alpha, X, ldx, Y, ldy, beta, G, ldg, stride_g, cap_stream(stream));
}

int cap_dgemm_vbatched_combine(const cap_vbatch_plan* p, int64_t nrhs, int64_t k, double alpha, const double* V, int64_t ldv, const double* Z,
                               int64_t ldz, int64_t stride_z, double beta, double* C, int64_t ldc, void* stream) {
  return gm_combine_plan(p, nrhs, k, alpha, V, ldv, Z, ldz, stride_z, beta, C, ldc, cap_stream(stream));
}

}  // extern "C"
