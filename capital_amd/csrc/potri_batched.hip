// Batched triangular inverse and SPD inverse from the factor for many blocks of one size (cap_dtrtri_batched, cap_dpotri_batched): block i is
// the n x n column-major block at base + i stride, 1 <= n <= 256, upper, in place.  The third and fourth members of the family of
// potrf_batched.hip / potrf_batched_blocked.hip: same layout, ONE launch on a 1-D grid, no scratch, no atomics, nothing between workgroups.
// TRTRI: the upper triangle <- that of T^-1.  POTRI: the upper triangle (the factor R) <- that of R^-1 R^-T; fill = 1 mirrors it into the
// strictly lower triangle afterwards.  A block with info != 0 gets NaN wherever the call writes and its input is not interpreted.
//
// n <= 64: ONE WAVEFRONT PER 64 / NP BLOCKS (NP = 8 / 16 / 32 / 64, the smallest one >= n; lane groups of NP lanes; one wave per workgroup, so
// __syncthreads orders the wave's own LDS accesses).  16.5 KiB of LDS at NP = 64, 4 KiB and less below.
//   The upper triangle goes to the packed LDS image of potrf_batched.hip (row r and row NP - 1 - r share a line of NP + 2 doubles).
//   Inverse.  Lane c owns column c of W = R^-1 in registers and runs the backward sweep of R w = e_c: for j = c .. 0: w_j /= r_jj, then
//     w_i -= r_ij w_j for i < j with r_ij an LDS broadcast; steps j > c are masked off (the column does not depend on later columns), steps
//     at or beyond n skipped by wave-uniform branches.  No lane talks to another one.  W then replaces R in the image.
//   Product.  Lane j takes row j of W into registers and forms column j of C = W W^T: c_ij = sum_{k >= j} w_ik w_jk, added in ascending k
//     by fused multiply-adds, w_ik an LDS broadcast.  Row i of the image is dead once every lane has its c_ij (the lanes' own rows are in
//     registers), so row i of C takes its place: the store is the coalesced one of the factor.
// 64 < n <= 256: ONE WORKGROUP PER BLOCK, templated on NBLK = ceil(n / 64) = 2, 3, 4: four waves and 49 KiB of static LDS at NBLK = 2, eight
// waves and 81.5 / 114 KiB at NBLK = 3 / 4 (168 / 238 / 238 registers per lane).  The block stays in its own memory (L2); both stages run in place on the upper triangle over
// diagonal blocks of 64 rows, as LAPACK's blocked dtrtri and dlauum do.
//   TRTRI, block column J = 0, 1, ... (k0 = 64 J rows above the diagonal block):
//     the diagonal block -> the image, the k0 x 64 column panel R12 -> LDS; wave 0 inverts the diagonal block by the sweep above; W22 ->
//     memory;  Y = R12 W22 on the fp64 16 x 16 x 4 MFMA, in place in the LDS panel: a wave owns strips of 16 rows and takes the column tiles
//     in descending order (tile c reads columns <= c only);  W12 = -W11 Y with W11 (inverted by the earlier steps) read from memory - its
//     strictly lower elements never - and Y from LDS, straight to memory.
//   LAUUM, block row I = 0, 1, ... (the LAPACK order: step I writes block column I only and reads columns >= I, which later steps need
//   unchanged from column I + 1 on):
//     W_II -> the image, the row panel W[I, I + 1 ..] -> LDS;  C[0 .. I, I] = W[., I] W_II^T + W[., I + 1 ..] W[I, I + 1 ..]^T, the
//     left operands from memory, the right ones from LDS, everything on the MFMA (the 64 x 64 triangle products too: one code path).  A wave
//     owns strips of 16 rows and takes the column tiles in ascending order (tile c reads columns >= c only), tiles wholly below the diagonal are
//     skipped, elements below it neither loaded nor stored.
// Every block sees the same instruction sequence on its own data: its bits depend on (n, its data, fill) only.  All global accesses are
// 8-byte ones: one load path whatever the alignment.  Divisions are correctly rounded (no reciprocal estimates).
#include "batched_inverse.h"   // the steps for n <= 64 and the per-block body for n > 64: shared with potrf_vbatched.hip
#include "vbatch_plan.h"       // the family's host arithmetic: padded size, grid limit, dispatch, operand rule

namespace {

template <int NP, bool POTRI>
__global__ __launch_bounds__(64) void potri_batched_kernel(PiArgs g) {
  constexpr int G = 64 / NP;
  using Img = PiImg<NP>;
  __shared__ double s_img[G * Img::SIZE];
  const int lane = threadIdx.x, grp = lane / NP, c = lane % NP, n = g.n;
  const int64_t blk = (int64_t)blockIdx.x * G + grp;
  const bool live = blk < g.batch;
  const int64_t ld = g.ld;
  double* A = g.A + (live ? blk * g.stride : 0);
  double* s = s_img + grp * Img::SIZE;
  const bool bad = g.info && live && g.info[blk] != 0;

  // upper triangle -> image; lane r walks along row r, so a column is contiguous
#pragma unroll 8
  for (int cc = 0; cc < n; cc++)
    if (live && c <= cc) s[Img::at(c, cc)] = A[c + (int64_t)cc * ld];
  __syncthreads();

  {
    double x[NP];
    pi_invert<NP>(x, s, c, n);
    __syncthreads();                     // every lane is through with R: the image takes W
    pi_put_column<NP>(x, s, c, n);
  }
  __syncthreads();

  if constexpr (POTRI) {
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
    __syncthreads();
  }

  const bool fill = POTRI && g.fill;
#pragma unroll 8
  for (int cc = 0; cc < n; cc++) {
    if (live && c <= cc) {
      const double v = bad ? (double)NAN : s[Img::at(c, cc)];
      A[c + (int64_t)cc * ld] = v;
      if (fill && c < cc) A[cc + (int64_t)c * ld] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- 64 < n <= 256
template <int NBLK>
__global__ __launch_bounds__(64 * pi_waves(NBLK)) void potri_batched_blocked_kernel(PiBlkArgs g) {
  pi_blocked_block<NBLK>(g.A + (int64_t)blockIdx.x * g.stride, g.ld, g.n, g.info, blockIdx.x, g.potri, g.fill);
}

// the two entries: potri = 0 the triangular inverse, 1 the SPD inverse from the factor
int pi_run(int potri, int uplo, int64_t n, double* T, int64_t ld, int64_t stride, int64_t batch, const int* info, int fill, void* stream) {
  if (n < 0 || batch < 0) return CAP_ERR_ARG;
  if (n > 0 && batch > 0 && !T) return CAP_ERR_ARG;
  if (!vb_operand_ok(n, n, ld, stride, batch)) return CAP_ERR_ARG;
  if (fill != 0 && fill != 1) return CAP_ERR_ARG;
  if (uplo != CAP_UPPER) return CAP_ERR_UNSUPPORTED;    // as cap_dpotrf_batched
  if (n > PI_MAX) return CAP_ERR_UNSUPPORTED;
  const int64_t nwg = vb_grid(batch, vb_per_group(vb_class(n)));
  if (n > PI_SMALL && nwg < 0) return CAP_ERR_UNSUPPORTED;     // a workgroup per block: refused in front of the empty case
  if (n == 0 || batch == 0) return CAP_OK;
  if (nwg < 0) return CAP_ERR_UNSUPPORTED;
  hipStream_t s = cap_stream(stream);
  if (cap_acc_on()) {
    for (int64_t i = 0; i < batch; i++) cap_acc_rw(T + i * stride, ld, n, n, fill ? 0 : 1);
    if (info) cap_acc_r(info, 0, batch, 1, 0, 4);
  }
  const dim3 grid((unsigned)nwg);
  if (n <= PI_SMALL) {
    PiArgs g;
    g.A = T; g.ld = ld; g.stride = stride; g.batch = batch; g.info = info; g.n = (int)n; g.fill = fill;
    if (potri) vb_with_int<8, 16, 32, 64>(vb_padded(n), [&](auto NP) { hipLaunchKernelGGL((potri_batched_kernel<NP(), true>), grid, dim3(64), 0, s, g); });
    else vb_with_int<8, 16, 32, 64>(vb_padded(n), [&](auto NP) { hipLaunchKernelGGL((potri_batched_kernel<NP(), false>), grid, dim3(64), 0, s, g); });
  } else {
    PiBlkArgs g;
    g.A = T; g.ld = ld; g.stride = stride; g.info = info; g.n = (int)n; g.potri = potri; g.fill = fill;
    vb_with_int<2, 3, 4>((int)cap_ceil_div(n, PI_NB), [&](auto NBLK) {
      hipLaunchKernelGGL(potri_batched_blocked_kernel<NBLK()>, grid, dim3(64 * pi_waves(NBLK())), 0, s, g);
    });
  }
  CAP_HIP(hipGetLastError());
  return CAP_OK;
}

}  // namespace

extern "C" {

int cap_dtrtri_batched(int uplo, int64_t n, double* T, int64_t ldt, int64_t stride_t, int64_t batch, const int* info, void* stream) {
  return pi_run(0, uplo, n, T, ldt, stride_t, batch, info, 0, stream);
}

int cap_dpotri_batched(int uplo, int64_t n, double* R, int64_t ldr, int64_t stride_r, int64_t batch, const int* info, int fill, void* stream) {
  return pi_run(1, uplo, n, R, ldr, stride_r, batch, info, fill, stream);
}

}  // extern "C"
