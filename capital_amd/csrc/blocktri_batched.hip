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
// THE BODIES (bt_factor, bt_solve) are blocktri_kernels.h's, shared with the ragged entries of blocktri_vbatched.hip; here the chain of a
// lane group is arithmetic (BtFixed).  HOW THE BLOCKS TRAVEL is told there: S_i lives in an LDS image and never in global memory, D and E
// go once in and once out, the solve keeps a right-hand-side column in the registers of its lane across the chain.  A long chain is sequential in its wavefront: few long chains leave the chip idle (splitting a chain needs cyclic
// reduction, which changes the arithmetic: out of scope).  EVERY ADDRESS AND PREDICATE is a function of blocktri_addr.h, swept lane by
// lane on the CPU (tests/test_blocktri_addr.py): position T - 1 has no coupling block and no successor, T = 1 has no E at all.
#include "blocktri_kernels.h"

namespace {

template <int NP>
__global__ __launch_bounds__(64) void blocktri_potrf_kernel(BtArgs<BtFixed> g) { bt_factor<NP>(g); }

template <int NP>
__global__ __launch_bounds__(64) void blocktri_potrs_kernel(BtSolveArgs<BtFixed> g) { bt_solve<NP>(g); }

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
  BtArgs<BtFixed> g = {};
  g.D = D; g.E = E; g.info = info; g.logdet = logdet;
  bt_geo(g.gd, n, T, batch, ldd, step_d, stride_d);
  bt_geo(g.ge, n, T, batch, lde, step_e, stride_e);
  if (cap_acc_on()) {
    for (int64_t c = 0; c < batch; c++) bt_note_chain(g.gd, g.ge, bt_host_chain(g.gd, g.ge, 0, c), D, E, CAP_ACC_RW, 1, CAP_ACC_RW);
    cap_acc_w(info, 0, batch, 1, 0, 4);
    if (logdet) cap_acc_w(logdet, 0, batch, 1);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bt_launch<blocktri_potrf_kernel<NP()>, 0>(g, nwg, s); });
  return st;
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
  BtSolveArgs<BtFixed> g = {};
  g.D = D; g.E = E; g.B = B; g.ldb = ldb; g.lk.stride_b = stride_b; g.nrhs = nrhs; g.info = info; g.half = half;
  bt_geo(g.gd, n, T, batch, ldd, step_d, stride_d);
  bt_geo(g.ge, n, T, batch, lde, step_e, stride_e);
  if (cap_acc_on()) {
    for (int64_t c = 0; c < batch; c++) {
      bt_note_chain(g.gd, g.ge, bt_host_chain(g.gd, g.ge, 0, c), D, E, CAP_ACC_R, 1, CAP_ACC_R);
      cap_acc_rw(B + c * stride_b, ldb, T * n, nrhs);
    }
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bt_launch<blocktri_potrs_kernel<NP()>, 0>(g, nwg, s); });
  return st;
}

}  // extern "C"
