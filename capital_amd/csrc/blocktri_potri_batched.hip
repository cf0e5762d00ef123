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
// THE BODY (bt_inverse) is blocktri_kernels.h's, shared with cap_dpotri_blocktri_vbatched; here the chain of a lane group is arithmetic
// (BtFixed).  HOW THE BLOCKS TRAVEL is told there: D and E go once in and once out, the image of U_i turns into P_i (pi_invert,
// pi_product_rows), Sigma_(i+1,i+1) never travels through global memory.  LDS: the image + two exchange areas = 11.0 / 21.5 / 42.5 /
// 84.5 KiB at NP = 8 / 16 / 32 / 64, dynamic; NP = 64 lies above the 64 KiB a kernel gets by default and asks for its size with
// hipFuncSetAttribute (bt_launch): ONE wavefront per CU there (160 KiB hold one such workgroup), three at NP = 32 - a long sequential chain per wavefront is latency bound, and n = 64 is the weak corner as it is for the factor.  Few long
// chains leave the chip idle (cyclic reduction changes the arithmetic: out of scope).  EVERY ADDRESS AND PREDICATE is a function of
// blocktri_addr.h, swept lane by lane on the CPU (tests/test_blocktri_potri_addr.py): position 0 has no predecessor, position T - 1 no
// coupling block, T = 1 no E at all.
#include "blocktri_kernels.h"

namespace {

template <int NP>
__global__ __launch_bounds__(64) void blocktri_potri_kernel(BtArgs<BtFixed> g) { bt_inverse<NP>(g); }

}  // namespace

extern "C" {

int cap_dpotri_blocktri_batched(int uplo, int fill, int64_t n, int64_t T, double* D, int64_t ldd, int64_t step_d, int64_t stride_d, double* E, int64_t lde,
                                int64_t step_e, int64_t stride_e, const int* info, int64_t batch, void* stream) {
  if (n < 0 || T < 0 || batch < 0) return CAP_ERR_ARG;
  const bool work = n > 0 && T > 0 && batch > 0;
  if (work && (!D || (!E && T > 1))) return CAP_ERR_ARG;
  if (!bt_operand_ok(n, T, ldd, step_d, stride_d, batch) || !bt_operand_ok(n, T - 1, lde, step_e, stride_e, batch)) return CAP_ERR_ARG;
  if (fill != 0 && fill != 1) return CAP_ERR_ARG;
  int st;
  const int64_t nwg = bt_limits(uplo, n, T, batch, st);
  if (st != CAP_OK) return st;
  if (!work) return CAP_OK;
  hipStream_t s = cap_stream(stream);
  BtArgs<BtFixed> g = {};
  g.D = D; g.E = E; g.info = const_cast<int*>(info); g.fill = fill;
  bt_geo(g.gd, n, T, batch, ldd, step_d, stride_d);
  bt_geo(g.ge, n, T, batch, lde, step_e, stride_e);
  if (cap_acc_on()) {                    // a D block as cap_dpotri_batched notes its block
    for (int64_t c = 0; c < batch; c++) bt_note_chain(g.gd, g.ge, bt_host_chain(g.gd, g.ge, 0, c), D, E, CAP_ACC_RW, fill ? 0 : 1, CAP_ACC_RW);
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
  }
  vb_with_int<8, 16, 32, 64>(g.gd.NP, [&](auto NP) { st = bt_launch<blocktri_potri_kernel<NP()>, (int)bt_inv_lds_bytes<NP(), BtFixed>()>(g, nwg, s); });
  return st;
}

}  // extern "C"
