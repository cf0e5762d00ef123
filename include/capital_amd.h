/* capital_amd.h - C ABI of the MI355X-native CAPITAL hot path (libcapital_amd.so).
 *
 * This is the drop-in boundary.  The reference (tbennun/capital) has no FFI: its seam is
 * C++ static-template call signatures.  Each entry point below names the reference
 * interface it replaces (file:line relative to the reference tree).  INTEGRATION.md shows
 * the reference-side binding a maintainer would add.
 *
 * Conventions
 *  - all matrices are COLUMN-MAJOR fp64 in DEVICE memory (HBM), caller owned;
 *  - dimensions / leading dimensions are int64_t (blas/interface.h:58-66 uses int64_t);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call is
 *    asynchronous on that stream unless stated otherwise.  "No host synchronisation" below is
 *    about the steady state, with two exceptions that hold for every entry: (1) the FIRST call
 *    of a process on a device that needs one of the small per-device word blocks (the give-up /
 *    injection counters of cap_dpotrs, cap_cholinv_solve, cap_dpocon, cap_dpoerr, cap_dcholupdate,
 *    cap_cholinv_update and of the diagonal-block chain) allocates and zeroes it and synchronises
 *    the device once; (2) scratch that a PLAN keeps is allocated by the first call that needs it
 *    and sized for that call - a later call on the same plan that needs MORE synchronises the
 *    device once, frees it and allocates the larger one (see cap_cholinv_solve);
 *  - every function returns a cap_status (0 = ok).  The reference has no error channel
 *    (LAPACKE info is dropped, lapack/interface.hpp:39,54); here POTRF's `info` is
 *    propagated through a device-resident int the caller can read back.
 *  - enums use the reference's own numeric values (blas/engine.h:23-52,
 *    lapack/engine.h:23-52) so ArgPacks map 1:1.
 */
#ifndef CAPITAL_AMD_H_
#define CAPITAL_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CAP_OK = 0,
  CAP_ERR_ARG = 1,        /* bad argument */
  CAP_ERR_HIP = 2,        /* a HIP runtime call failed */
  CAP_ERR_NOT_SPD = 3,    /* potrf met a non-positive pivot (info > 0) */
  CAP_ERR_UNSUPPORTED = 4,
  CAP_ERR_COMM = 5,       /* RCCL failure */
  CAP_ERR_ALLOC = 6
} cap_status;

/* blas/engine.h:23-52 */
enum { CAP_NOTRANS = 0, CAP_TRANS = 1 };
enum { CAP_LEFT = 0, CAP_RIGHT = 1 };
enum { CAP_LOWER = 0, CAP_UPPER = 1 };
enum { CAP_NONUNIT = 0, CAP_UNIT = 1 };

const char* cap_status_string(int status);
/* library / device info: fills name (<= len bytes), CU count, HBM bytes. */
int cap_device_info(char* name, int len, int* cus, int64_t* hbm_bytes);

/* ------------------------------------------------------------------------------------
 * Operator seam  (replaces blas::engine / lapack::engine, device pointers + status)
 * ---------------------------------------------------------------------------------- */

/* blas::engine::_gemm  - blas/interface.h:58-60, interface.hpp:43-59 (cblas_dgemm).
 * C[m x n] = alpha * op(A)[m x k] * op(B)[k x n] + beta * C.
 * n <= 8 with op(B) = B and m >= 1024 (a few right-hand sides against a big operand: refinement residuals, TRSM block steps)
 * runs on streaming kernels that read op(A) once; their transposed form sums in 64-k blocks with Kahan's correction.      */
int cap_dgemm(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
              const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
              double* C, int64_t ldc, void* stream);

/* blas::engine::_syrk  - blas/interface.h:65-66, interface.hpp:81-97 (cblas_dsyrk).
 * C[n x n](uplo triangle only) = alpha * op(A) op(A)^T + beta * C;
 * trans == CAP_TRANS: A is k x n and C = alpha*A^T*A + beta*C (the form cacqr.hpp:15 and
 * the trailing update cholinv.hpp:128-137 use).                                        */
int cap_dsyrk(int uplo, int trans, int64_t n, int64_t k, double alpha, const double* A,
              int64_t lda, double beta, double* C, int64_t ldc, void* stream);

/* blas::engine::_trmm  - blas/interface.h:62-63, interface.hpp:61-79 (cblas_dtrmm).
 * B[m x n] = alpha * op(T) * B (side = LEFT, T m x m) or alpha * B * op(T) (RIGHT, T n x n).
 * In place like the reference; `work` is device scratch of >= cap_dtrmm_work_size doubles
 * (the reference hides the same copy inside MKL).  uplo = UPPER, diag = NONUNIT only (all
 * upstream call sites); other values return CAP_ERR_UNSUPPORTED.               */
int cap_dtrmm(int side, int uplo, int trans, int diag, int64_t m, int64_t n, double alpha,
              const double* T, int64_t ldt, double* B, int64_t ldb, double* work, void* stream);
int64_t cap_dtrmm_work_size(int side, int64_t m, int64_t n);

/* Real triangular solve (not in the reference, which inverts then multiplies - SURVEY 2b;
 * trsm/diaginvert/diaginvert.hpp:7-10 is a static_assert stub).  Solves
 * op(T) X = alpha B (LEFT) or X op(T) = alpha B (RIGHT) in place; T upper, non-unit.  Done as a
 * blocked substitution: only the diagonal blocks (width <= 512) are inverted (recursive TRTRI), then
 * per block step one MFMA GEMM with the block inverse and one GEMM update of the remaining rows.
 * `work`: device scratch >= cap_dtrsm_work_size doubles.                                   */
int cap_dtrsm(int side, int uplo, int trans, int64_t m, int64_t n, double alpha, const double* T,
              int64_t ldt, double* B, int64_t ldb, double* work, void* stream);
int64_t cap_dtrsm_work_size(int side, int64_t m, int64_t n);

/* lapack::engine::_potrf - lapack/interface.h:49-50, interface.hpp:30-43 (LAPACKE_dpotrf).
 * In-place A = R^T R (uplo = UPPER; LOWER returns CAP_ERR_UNSUPPORTED - upstream removed
 * 'L' too, cholinv.hpp:9) of the n x n block; the other triangle is not referenced.  `info` (device int, may be NULL): 0 or 1-based index of the first
 * non-positive pivot.  `work`: device scratch >= cap_dpotrf_work_size(n) doubles.         */
int cap_dpotrf(int uplo, int64_t n, double* A, int64_t lda, int* info, double* work, void* stream);
int64_t cap_dpotrf_work_size(int64_t n);

/* lapack-style POTRS beside cap_dpotrf (not in the reference, whose trsm/diaginvert/diaginvert.hpp:7-10 is a stub):
 * A X = B with A = R^T R, R upper (the output of cap_dpotrf; the other triangle is not referenced), B (n x nrhs) overwritten by X.
 * uplo = LOWER -> CAP_ERR_UNSUPPORTED, as for cap_dpotrf.  `work`: device scratch >= cap_dpotrs_work_size(n, nrhs) doubles.
 * Same two pieces as cap_cholinv_solve, the inverses of R's diagonal blocks computed into `work` on every call.              */
int cap_dpotrs(int uplo, int64_t n, int64_t nrhs, const double* R, int64_t ldr, double* B, int64_t ldb,
               double* work, void* stream);
int64_t cap_dpotrs_work_size(int64_t n, int64_t nrhs);

/* lapack::engine::_trtri - lapack/interface.h:52-53, interface.hpp:45-58 (LAPACKE_dtrtri).
 * In-place inverse of the triangular n x n block (non-unit).  work >= cap_dtrtri_work_size. */
int cap_dtrtri(int uplo, int64_t n, double* A, int64_t lda, double* work, void* stream);
int64_t cap_dtrtri_work_size(int64_t n);

/* LAPACK dlauum, out of place (not in the reference): upper triangle of C = W W^T, W upper triangular non-unit.  The strictly lower
 * triangle of W is not referenced, the strictly lower triangle of C is not written.  W and C must not overlap (CAP_ERR_ARG).
 * uplo = LOWER -> CAP_ERR_UNSUPPORTED.  n^3 / 3 flops on the LDS-DMA MFMA kernel when ldw is even and W 16-byte aligned (any n); an
 * odd ldw or an unaligned W goes through a copy and the dense-K product (three times the flops).                               */
int cap_dlauum(int uplo, int64_t n, const double* W, int64_t ldw, double* C, int64_t ldc, void* stream);

/* LAPACK dpotri beside cap_dpotrf (= dtrtri + dlauum): A holds R (upper, from cap_dpotrf); on return its upper triangle holds that of
 * A^-1 = R^-1 R^-T.  The strictly lower triangle is neither read nor written.  uplo = LOWER -> CAP_ERR_UNSUPPORTED.
 * work >= cap_dpotri_work_size(n) doubles (an n x n inverse + TRTRI's own scratch).                                             */
int cap_dpotri(int uplo, int64_t n, double* A, int64_t lda, double* work, void* stream);
int64_t cap_dpotri_work_size(int64_t n);

/* Rank-k update (sign = +1) / downdate (sign = -1) of the factor beside cap_dpotrf (LINPACK's dchud / dchdd, MATLAB's cholupdate; not in
 * the reference): R holds the upper factor of A = R^T R; on return it holds that of A' = A + sign V V^T, V n x k (column-major, ld ldv,
 * k << n), in 2 k n^2 flops and one pass over the upper triangle per 16 columns of V instead of n^3 / 3.  In place; the strictly lower
 * triangle of R (also inside diagonal tiles) is neither read nor written, V is not written, rows >= n of R and V are not touched.
 * sign other than +1 / -1, negative n or k -> CAP_ERR_ARG; with n > 0 and k > 0: NULL R, V or work, ldr < n, ldv < n -> CAP_ERR_ARG;
 * then uplo = LOWER -> CAP_ERR_UNSUPPORTED; n == 0 or k == 0 -> CAP_OK, nothing touched.  Any ldr >= n, any 8-byte aligned pointers.
 * Asynchronous on `stream`, no host synchronisation.  `work`: device scratch >= cap_dcholupdate_work_size(n, k) doubles.
 * The sweep (csrc/cholupdate.hip) applies one reflection per row to (R_rr; V^T[:, r]): a Householder reflection for the update, a
 * hyperbolic one in its mixed form for the downdate.  k > 16 is taken as consecutive passes of at most 16 columns of V, each a complete
 * update of its own.  Each pass is one launch whose workgroups claim the diagonal and tile items of the 64-blocked sweep from a ticket
 * counter, followed by a recovery launch that finishes the pass on one workgroup if a workgroup gave up waiting (counted by
 * cap_update_fallbacks); fixed summation order: two calls give the same bits.
 * `info` (device int, may be NULL) is set to 0 at the start of the device work, then holds the 1-based row at which A - V V^T was found
 * not positive definite (first one wins); the sweep carries on with NaN.  After info != 0, R IS NOT A FACTOR OF ANYTHING - keep a copy
 * if a failing downdate must be survivable.
 * Accuracy: the update is backward stable.  The downdate's error grows as A' approaches singularity relative to A (that is inherent:
 * R' then depends ill-conditionedly on R and V): backward error |R'^T R' - A'|_F / |A'|_F about 5e-16 when cond(A') stays below 10,
 * 4e-12 (CPU model of the same sweep) when a downdate lowers the condition number from 1e5 to about 5.                               */
int cap_dcholupdate(int uplo, int sign, int64_t n, int64_t k, double* R, int64_t ldr, const double* V, int64_t ldv, int* info,
                    double* work, void* stream);
int64_t cap_dcholupdate_work_size(int64_t n, int64_t k);

/* Pivoted Cholesky factorization with a rank cap (LAPACK's dpstrf, out of place and truncated; not in the reference): for a symmetric
 * positive SEMIdefinite or numerically rank-deficient A (kernel / Gram / covariance matrices) it gives the numerical rank, a factor that
 * survives a zero pivot and the low-rank approximation A[piv][:, piv] ~ R^T R in O(n rank^2) work.  A is n x n column-major (ld lda);
 * only its upper triangle is read (the strictly lower one may hold anything), A is never written.
 * The steps keep d, the remaining diagonal (initially diag A).  Step j = 0, 1, ...: p = the unselected index of largest d (ties: the
 * lowest index).  A NaN among the unselected d: stop, info = 2.  d[p] <= tol_used, or j = n: stop, info = 0.  j = max_rank: stop,
 * info = 1 (the cap was hit with the remainder still above the tolerance).  Otherwise row j of the factor is
 * (A(p, c) - sum_{i<j} W[i, p] W[i, c]) / sqrt(d[p]) for the unselected c != p, sqrt(d[p]) itself at c = p and 0 at the columns
 * selected before; d[c] -= W[j, c]^2; p becomes selected.  tol < 0: tol_used = n eps max_i a_ii with eps = 2^-53 (LAPACK's default);
 * tol >= 0 is absolute, as in LAPACK.
 * Results, all device memory: *rank = the number of steps done; piv[n] (0-based) = the chosen pivots in order, then the unselected
 * indices in increasing order - always a permutation; R (max_rank x n, ld ldr >= max(max_rank, 1)), R[:, k] = W[:, piv[k]]: R[0:rank,
 * 0:rank] is upper triangular with a positive, non-increasing diagonal, rows rank .. max_rank - 1 are zero, rows >= max_rank (padding)
 * are not touched; *resid (may be NULL) = the sum of the unselected d in index order = trace(A - R^T R), the nuclear-norm error of the
 * approximation for a semidefinite A; *info (may be NULL) as above.  info = 2 is a result, not an error: the call returns CAP_OK.
 * Negative n, max_rank < 0 or > n, a NaN tol -> CAP_ERR_ARG; with n > 0: NULL A, piv, rank or work, lda < n -> CAP_ERR_ARG; with n > 0
 * and max_rank > 0: NULL R or ldr < max_rank -> CAP_ERR_ARG; then uplo = LOWER -> CAP_ERR_UNSUPPORTED; n == 0 -> CAP_OK, nothing
 * touched.  max_rank = 0 is legal: rank 0, the identity piv, resid = trace A, info = 0 if max_i a_ii <= tol_used, else 1.
 * Asynchronous on `stream`, no host synchronisation: one launch per possible step (max_rank of them - after the stopping decision the
 * remaining ones return at once) plus one in front and one behind (csrc/pstrf.hip).  Every summation order is fixed: two calls give
 * the same bits.  `work`: device scratch >= cap_dpstrf_work_size(n, max_rank) doubles (>= max_rank n: the factor in natural column
 * order; monotone in both arguments), any 8-byte aligned pointers.
 * Accuracy: on the selected rows |A - R^T R| <= gamma_{rank+2} |R|^T |R| componentwise (the Cholesky backward-error bound).            */
int cap_dpstrf(int uplo, int64_t n, int64_t max_rank, double tol, const double* A, int64_t lda, double* R, int64_t ldr, int64_t* piv,
               int64_t* rank, double* resid, int* info, double* work, void* stream);
int64_t cap_dpstrf_work_size(int64_t n, int64_t max_rank);

/* Batched Cholesky factor and solve for MANY SMALL SPD matrices of one size (potrf_batched / potrs_batched of the vendor libraries, strided
 * form; not in the reference): matrix i is the n x n column-major block at A + i * stride_a (leading dimension lda), i = 0 .. batch - 1,
 * 1 <= n <= 64 - n > 64 returns CAP_ERR_UNSUPPORTED (loop over cap_dpotrf for larger blocks).  fp64, upper factor, one GPU, ONE launch per
 * call (csrc/potrf_batched.hip: one wavefront per 64 / NP blocks, NP = 8, 16, 32 or 64 >= n; nothing between workgroups).  No `work`
 * argument, no allocation, no process-wide state (no mutex, no helper stream): asynchronous on `stream`, callable from several host threads.
 * cap_dpotrf_batched: the upper triangle of every block is replaced by R_i (A_i = R_i^T R_i).  The strictly lower triangles, rows n .. lda - 1
 * of every column, the gaps between blocks (stride_a > lda n) and everything behind the last block are neither read nor written.
 * info (batch device ints, may be NULL): info[i] = 0, or the 1-based index p of the first pivot that is not > 0 (a NaN pivot counts as not
 * > 0).  Such a block holds the rows 0 .. p - 2 of R computed so far and NaN in rows p - 1 .. n - 1 of its upper triangle; no other block is
 * affected.  logdet (batch device doubles, may be NULL): logdet[i] = 2 sum_j log r_jj, added in ascending j; NaN for a failed block.
 * Square roots and divisions are correctly rounded ones, no reciprocal estimates.
 * cap_dpotrs_batched: B_i (n x nrhs at B + i * stride_b, leading dimension ldb) <- the solution of R_i^T R_i X = B_i, any nrhs >= 0 (more
 * than NP right-hand sides are further passes inside the launch).  The strictly lower triangle of R is not referenced; only rows 0 .. n - 1
 * of the nrhs columns of each B_i are written.  info (what the factor call wrote, may be NULL): info[i] != 0 leaves X_i NaN, the convention
 * of cap_cholinv_solve.
 * A block's result bits depend on (n, its own data) alone - not on batch, its index, lda, the strides, the alignment, the number of
 * right-hand sides that travel with a column, or the run.
 * n < 0, batch < 0, nrhs < 0; a NULL A / R / B with n batch > 0; lda, ldr or ldb < n; with batch > 1: stride_a < lda n, stride_r < ldr n or
 * stride_b < ldb nrhs -> CAP_ERR_ARG; then uplo = LOWER -> CAP_ERR_UNSUPPORTED, as cap_dpotrf; then n > 64 -> CAP_ERR_UNSUPPORTED; n == 0,
 * batch == 0 or nrhs == 0 -> CAP_OK without a launch.  All decided before any device call.  Offsets are 64-bit.                            */
int cap_dpotrf_batched(int uplo, int64_t n, double* A, int64_t lda, int64_t stride_a, int64_t batch, int* info, double* logdet, void* stream);
int cap_dpotrs_batched(int uplo, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                       int64_t stride_b, int64_t batch, const int* info, void* stream);

/* The same two calls for blocks of up to 256 rows: 1 <= n <= 256, n > 256 returns CAP_ERR_UNSUPPORTED.  Arguments, layout, info / logdet,
 * the argument rules and their order are those of cap_dpotrf_batched / cap_dpotrs_batched (which keep refusing n > 64).  n <= 64 runs the
 * kernels of those calls: the same bits.  64 < n <= 256 (csrc/potrf_batched_blocked.hip): ONE launch, one workgroup of four waves per block on
 * a 1-D grid (batch beyond one grid dimension -> CAP_ERR_UNSUPPORTED), nothing between workgroups; a right-looking factorization over diagonal
 * blocks of 64 rows - the diagonal block in one wave's registers, the row panel by substitution with a column per lane, the trailing update
 * on the fp64 MFMA from LDS - and blocked substitutions with 16 right-hand sides per pass.  No `work`, no allocation, no memset, no mutex, no
 * helper stream, no host synchronisation.  What is never read or written, the NaN rows of a failed block, correctly rounded square roots and
 * divisions, and "a block's bits depend on (n, its own data) alone, a column's on (n, R, that column of B) alone": as above.               */
int cap_dpotrf_batched_blocked(int uplo, int64_t n, double* A, int64_t lda, int64_t stride_a, int64_t batch, int* info, double* logdet,
                               void* stream);
int cap_dpotrs_batched_blocked(int uplo, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                               int64_t stride_b, int64_t batch, const int* info, void* stream);

/* Batched triangular inverse and SPD inverse from the factor (csrc/potri_batched.hip): block i is the n x n column-major block at
 * T + i * stride_t (R + i * stride_r) with the given leading dimension, 1 <= n <= 256, fp64, upper, one GPU.  One entry per operation for
 * the whole range: n <= 64 runs one wavefront per 64 / NP blocks (NP = 8, 16, 32 or 64 >= n), 64 < n <= 256 one workgroup per block.
 * The contract is that of the batched entries above: ONE launch per call on a 1-D grid, no `work` argument, no allocation, no memset, no
 * atomics, no mutex, no helper stream, no host synchronisation; asynchronous on `stream`, callable from several host threads; 64-bit
 * offsets; divisions are correctly rounded, no reciprocal estimates; a block's bits depend on (n, its own data, fill) alone - not on its
 * position in the batch, the batch size, ld / stride or alignment (all global accesses are 8-byte ones: one load path).
 * cap_dtrtri_batched: the upper triangle of every block <- that of T_i^-1 (non-unit diagonal).  A zero on the diagonal is not detected: it
 * propagates as IEEE infinities and NaNs inside its own block only (cap_dtrtri has no info either).
 * cap_dpotri_batched: R holds the factors cap_dpotrf_batched[_blocked] left; the upper triangle of every block <- that of A_i^-1 =
 * R_i^-1 R_i^-T.  fill = 0: the upper triangle only; fill = 1: the strictly lower triangle becomes the bit-identical mirror of the upper one
 * (copied, never computed a second time), cap_cholinv_inverse's fill; any other fill -> CAP_ERR_ARG.
 * info (what the factor call wrote, may be NULL): a block with info[i] != 0 gets NaN in everything the call would have written for it (the
 * upper triangle, or the n x n window with fill = 1) and its input is not interpreted - the convention of cap_dpotrs_batched.
 * Never read: the strictly lower triangle of an input block, rows n .. ld - 1 of every column, the gaps between blocks, everything behind
 * the last block.  Never written: the same elements, except the strictly lower triangle under fill = 1.
 * Argument rules, in this order, all decided before any device call: n < 0, batch < 0, a NULL block pointer with n batch > 0, ld < n,
 * batch > 1 with stride < ld n, a bad fill -> CAP_ERR_ARG; uplo = LOWER -> CAP_ERR_UNSUPPORTED; n > 256 -> CAP_ERR_UNSUPPORTED (also for an
 * empty batch); 64 < n with a batch beyond one grid dimension -> CAP_ERR_UNSUPPORTED; n == 0 or batch == 0 -> CAP_OK without a launch.   */
int cap_dtrtri_batched(int uplo, int64_t n, double* T, int64_t ldt, int64_t stride_t, int64_t batch, const int* info, void* stream);
int cap_dpotri_batched(int uplo, int64_t n, double* R, int64_t ldr, int64_t stride_r, int64_t batch, const int* info, int fill, void* stream);

/* Variable-size batched Cholesky (potrf_vbatched of the vendor libraries; csrc/potrf_vbatched.hip): factor, solve and SPD inverse of a batch
 * of blocks of DIFFERENT sizes 0 <= n_i <= 256 - fp64, upper, column-major - described once by a PLAN.
 * cap_vbatch_plan_create: n, ld, offset are HOST arrays of `batch` entries; block i is the n_i x n_i block at A + offset[i] with leading
 * dimension ld[i].  ld == NULL: ld[i] = max(n_i, 1); offset == NULL: the blocks lie back to back in batch order (offset[i] = sum_{j<i}
 * ld[j] n_j).  Argument rules, in this order: NULL out, batch < 0, NULL n with batch > 0, some n_i < 0, ld[i] < n_i or offset[i] < 0, two
 * non-empty blocks whose windows [offset, offset + (n - 1) ld + n) meet (checked after sorting the windows by offset; a block inside
 * another one's padding counts) -> CAP_ERR_ARG; then some n_i > 256 -> CAP_ERR_UNSUPPORTED; then a size class with more blocks than one
 * grid dimension serves -> CAP_ERR_UNSUPPORTED.  n_i = 0 is legal: nothing of that block is touched, info[i] and logdet[i] are NOT
 * written (zero them once; the Python layer does).  batch = 0 is legal.
 * Create sorts the blocks into seven size classes - NP = 8, 16, 32, 64 >= n_i (a wavefront per 64 / NP blocks) and NBLK = ceil(n_i / 64) =
 * 2, 3, 4 (a workgroup per block) - each list stably sorted by n_i, builds the per-block records (offset, ld, row offset, n) and uploads
 * both to the CURRENT device with synchronous copies: create and destroy MAY SYNCHRONISE the device and allocate / free device memory; no
 * other call of this section does.  The plan is read-only afterwards: any number of calls, from several streams and host threads at once.
 * In a process without a device create still succeeds and the plan serves cap_vbatch_plan_info / _table; the three entries return
 * CAP_ERR_HIP for it unless there is nothing to launch.
 * cap_vbatch_plan_info(p, what): CAP_VBATCH_BATCH; _TOTAL = elements spanned (the largest offset + (n - 1) ld + n); _ROWS = sum n_i;
 * _NMAX = the largest n_i; _LAUNCHES = the number of non-empty classes = launches per call; _COUNT + c, c = 0 .. 6 = blocks of class c (in
 * the order above).  -1 for a NULL plan or an unknown `what`.  cap_vbatch_plan_table(p, c, blocks, cap): the first min(cap, count) block
 * indices of class c's list, a host copy; NULL plan, c outside 0 .. 6, cap < 0, NULL blocks with cap > 0 -> CAP_ERR_ARG.
 * The three entries, asynchronous on `stream`: ONE launch per non-empty class (seven at most), all on `stream`; no scratch, no allocation,
 * no memset, no atomics, no helper stream, no host synchronisation.  info (may be NULL) and logdet (may be NULL) have `batch` entries in
 * BATCH order; their conventions, the NaN rows of a failed block, what is never read or written, and `fill` are those of
 * cap_dpotrf_batched[_blocked] / cap_dpotrs_batched[_blocked] / cap_dpotri_batched.
 * cap_dpotrs_vbatched: B is the STACKED system, (sum n_i) x nrhs column-major with ldb >= sum n_i; block i owns rows row_off[i] ..
 * row_off[i] + n_i, row_off the prefix sum of n in batch order: the call applies the inverse of the block-diagonal matrix.  Any nrhs >= 0.
 * THE BIT CONTRACT: for every block i the three entries write, bit for bit, what cap_dpotrf_batched_blocked / cap_dpotrs_batched_blocked /
 * cap_dpotri_batched write on the same data with n = n_i and batch = 1 - info[i] and logdet[i] included - whichever blocks share its
 * wavefront, its class list or the batch, and whatever ld[i], offset[i] and the order of the batch.
 * Entry rules, in this order: NULL plan, nrhs < 0, a NULL A / R / B when something would be launched, ldb < sum n_i, fill other than 0 / 1
 * -> CAP_ERR_ARG; uplo = LOWER -> CAP_ERR_UNSUPPORTED; an empty plan, an all-zero-size plan or nrhs = 0 -> CAP_OK without a launch.          */
typedef struct cap_vbatch_plan cap_vbatch_plan;
enum { CAP_VBATCH_BATCH = 0, CAP_VBATCH_TOTAL = 1, CAP_VBATCH_ROWS = 2, CAP_VBATCH_NMAX = 3, CAP_VBATCH_LAUNCHES = 4, CAP_VBATCH_COUNT = 5 };
int cap_vbatch_plan_create(int64_t batch, const int64_t* n, const int64_t* ld, const int64_t* offset, cap_vbatch_plan** out);
int cap_vbatch_plan_destroy(cap_vbatch_plan* p);
int64_t cap_vbatch_plan_info(const cap_vbatch_plan* p, int what);
int cap_vbatch_plan_table(const cap_vbatch_plan* p, int cls, int64_t* blocks, int64_t cap);
int cap_dpotrf_vbatched(const cap_vbatch_plan* p, int uplo, double* A, int* info, double* logdet, void* stream);
int cap_dpotrs_vbatched(const cap_vbatch_plan* p, int uplo, int64_t nrhs, const double* R, double* B, int64_t ldb, const int* info,
                        void* stream);
int cap_dpotri_vbatched(const cap_vbatch_plan* p, int uplo, double* R, const int* info, int fill, void* stream);

/* Batched rank-k update / downdate of the factors (csrc/cholupdate_batched.hip; the vendor libraries have no such call): block i is the
 * n x n column-major block at R + i * stride_r (leading dimension ldr), 1 <= n <= 256, holding the upper factor
 * cap_dpotrf_batched[_blocked] left; on return it holds the upper factor of R_i^T R_i + sign V_i V_i^T, in place.  V_i is n x k
 * column-major at V + i * stride_v (leading dimension ldv) and is never written.  sign = +1 or -1, one value per call.  Any k >= 0: k > 16
 * is taken as consecutive passes of at most 16 columns inside the same launch, each a complete update, as in cap_dcholupdate.
 * info (batch device ints, may be NULL) is INPUT AND OUTPUT, the convention of cap_cholinv_update on a plan: a block with info[i] != 0 on
 * entry is not touched and its info[i] stays; otherwise info[i] stays 0 or becomes the 1-based row at which A_i - V_i V_i^T was found
 * not positive definite - the sweep carries on with NaN, as in the single-matrix call, and no other block is affected.  NULL: every block
 * is swept.  A block has one owner (a wavefront's lane group for n <= 64, a workgroup of four waves above) and its rows go in order: the
 * first failing row is written with a plain store.
 * The contract is that of the batched entries above: ONE launch per call on a 1-D grid, no `work` argument, no allocation, no memset, no
 * atomics, no mutex, no helper stream, no host synchronisation; asynchronous on `stream`, callable from several host threads; 64-bit
 * offsets.  Never read: the strictly lower triangle of R, rows n .. ld - 1 of every column of R and V, the gaps between blocks, everything
 * behind the last block.  Never written: the same, and all of V.
 * THE BIT CONTRACT: for every block with info[i] == 0 on entry, R_i and info[i] come out bit for bit as cap_dcholupdate (either driver)
 * writes them for that block alone with the same sign, k and data - whatever batch, its index, ldr, ldv, the strides, the alignment and
 * whichever blocks share its wavefront.  (Both run the row steps of csrc/chud_step.h: rho^2 = fma(sigma, w.w, r_rr^2), a correctly rounded
 * square root and three divisions per row, the dot products in four interleaved partial sums over NK = 1 / 2 / 4 / 8 / 16 >= the pass's
 * columns, zero padded.)
 * Argument rules, in this order, all decided before any device call: sign other than +1 / -1, n < 0, k < 0, batch < 0 -> CAP_ERR_ARG; with
 * n k batch > 0: NULL R or V, ldr < n, ldv < n, and with batch > 1 stride_r < ldr n or stride_v < ldv k -> CAP_ERR_ARG; uplo = LOWER ->
 * CAP_ERR_UNSUPPORTED; n > 256 -> CAP_ERR_UNSUPPORTED; 64 < n with a batch beyond one grid dimension -> CAP_ERR_UNSUPPORTED; n == 0,
 * k == 0 or batch == 0 -> CAP_OK without a launch, nothing touched.
 * cap_dcholupdate_vbatched: the same on a cap_vbatch_plan (sizes 0 <= n_i <= 256, per-block offset / ld for R).  V is the STACKED matrix,
 * (sum n_i) x k column-major with ldv >= sum n_i; block i owns rows row_off[i] .. row_off[i] + n_i, exactly as B in cap_dpotrs_vbatched.
 * One launch per non-empty size class (seven at most); every block gets, bit for bit, what cap_dcholupdate_batched gives for it with
 * batch = 1.  info has `batch` entries in batch order; entries of empty blocks are neither read nor written.  Entry rules, in this order:
 * NULL plan, bad sign, k < 0, NULL R / V when something would be launched, ldv < sum n_i -> CAP_ERR_ARG; uplo = LOWER ->
 * CAP_ERR_UNSUPPORTED; an empty or all-zero-size plan or k = 0 -> CAP_OK without a launch; a plan made without a device -> CAP_ERR_HIP
 * unless nothing would be launched.                                                                                                       */
int cap_dcholupdate_batched(int uplo, int sign, int64_t n, int64_t k, double* R, int64_t ldr, int64_t stride_r, const double* V, int64_t ldv,
                            int64_t stride_v, int64_t batch, int* info, void* stream);
int cap_dcholupdate_vbatched(const cap_vbatch_plan* p, int uplo, int sign, int64_t k, double* R, const double* V, int64_t ldv, int* info,
                             void* stream);

/* Batched triangular solves and products on the factors (csrc/trsm_batched.hip): one HALF of what cap_dpotrs_batched[_blocked] applies, and
 * the products that go with it.  Left side, upper triangle, non-unit diagonal, no alpha, fp64, one GPU, 1 <= n <= 256.  R, ldr, stride_r, B,
 * ldb, stride_b, batch and info are exactly those of cap_dpotrs_batched[_blocked]: block i is the n x n column-major block at
 * R + i * stride_r holding an upper triangle (what cap_dpotrf_batched[_blocked] left, or any other), B_i is n x nrhs at B + i * stride_b.
 *   cap_dtrsm_batched  trans = CAP_TRANS: B_i <- R_i^-T B_i (the whitened right-hand sides: with L = R^T, y = L^-1 b);
 *                      trans = CAP_NOTRANS: B_i <- R_i^-1 B_i.
 *   cap_dtrmm_batched  trans = CAP_TRANS: B_i <- R_i^T B_i (colouring: x = L z draws from N(0, A_i));  trans = CAP_NOTRANS: B_i <- R_i B_i.
 * Any nrhs >= 0: more right-hand sides than a pass holds (NP = 8, 16, 32 or 64 >= n for n <= 64, 16 above) are further passes inside the
 * launch.  The strictly lower triangle of R, rows n .. ld - 1 of every column of R and B, the gaps between blocks and columns and everything
 * behind the last block are never addressed.  A zero on the diagonal is not detected, as in cap_dtrtri_batched: it shows as IEEE infinities
 * and NaNs inside its own block.  info (may be NULL): a block with info[i] != 0 gets NaN in its B_i - and in its sumsq row - and its R is
 * not interpreted.
 * sumsq (cap_dtrsm_* only, may be NULL; ldq >= nrhs): sumsq[i * ldq + k] = the sum of the squares of column k of the RESULT of block i -
 * with trans = CAP_TRANS the squared Mahalanobis distance b^T A_i^-1 b.  It is computed inside the same launch from the values that are
 * stored to B, by the one thread that owns the column, as   q = 0;  for r = 0 .. n - 1: q = fma(x_r, x_r, q)   - the same recurrence on
 * the wavefront path (n <= 64) and on the workgroup path: the value is a function of the stored column alone.
 * The contract is that of the batched entries above: ONE launch per call on a 1-D grid (n <= 64: a wavefront per 64 / NP blocks; above: a
 * workgroup of four waves per block), no `work` argument, no allocation, no memset, no atomics, no mutex, no helper stream, no host
 * synchronisation, nothing between workgroups; asynchronous on `stream`, callable from several host threads; 64-bit offsets; correctly
 * rounded divisions.  The order of the additions of a product's row sum is fixed (it is written at the head of csrc/trsm_batched.hip): for
 * n <= 64 from the diagonal outwards, one fused multiply-add per term.
 * THE BIT CONTRACTS.
 *   1. HALVES = WHOLE: cap_dtrsm_batched(CAP_TRANS) followed by cap_dtrsm_batched(CAP_NOTRANS) on the same B leaves, bit for bit, what
 *      cap_dpotrs_batched_blocked leaves, for every n, layout, nrhs and batch - the NaN of failed blocks included.
 *   2. PLAN = FIXED: every block of a plan call gets the bits of the fixed-size entry on it alone with batch = 1, sumsq included,
 *      whichever blocks share its wavefront or its class.
 *   3. COLUMN INDEPENDENCE: a column's result and its sumsq do not depend on how many columns travel with it or on its position among them.
 * Argument rules, in this order, all decided before any device call: trans other than CAP_NOTRANS / CAP_TRANS, n < 0, nrhs < 0, batch < 0; a
 * NULL R or B with n nrhs batch > 0; ldr < n or ldb < n; with batch > 1: stride_r < ldr n or stride_b < ldb nrhs; sumsq given with ldq <
 * nrhs -> CAP_ERR_ARG; then uplo = LOWER -> CAP_ERR_UNSUPPORTED; then n > 256 -> CAP_ERR_UNSUPPORTED; then a grid beyond one dimension
 * (2^31 - 1 workgroups) -> CAP_ERR_UNSUPPORTED; then n == 0, nrhs == 0 or batch == 0 -> CAP_OK without a launch.
 * cap_dtrsm_vbatched / cap_dtrmm_vbatched: the same on a cap_vbatch_plan, with the layout of cap_dpotrs_vbatched - B is the STACKED
 * (sum n_i) x nrhs matrix with ldb >= sum n_i, block i owning rows row_off[i] .. row_off[i] + n_i.  One launch per non-empty size class
 * (seven at most).  info and sumsq are indexed by the BATCH index i; the words of empty blocks are neither read nor written.  Entry rules,
 * in this order: NULL plan, bad trans, nrhs < 0, a NULL R / B when something would be launched, ldb < sum n_i, sumsq given with ldq < nrhs
 * -> CAP_ERR_ARG; uplo = LOWER -> CAP_ERR_UNSUPPORTED; an empty or all-zero-size plan or nrhs = 0 -> CAP_OK without a launch; a plan made
 * without a device -> CAP_ERR_HIP unless nothing would be launched.                                                                       */
int cap_dtrsm_batched(int uplo, int trans, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                      int64_t stride_b, int64_t batch, const int* info, double* sumsq, int64_t ldq, void* stream);
int cap_dtrmm_batched(int uplo, int trans, int64_t n, int64_t nrhs, const double* R, int64_t ldr, int64_t stride_r, double* B, int64_t ldb,
                      int64_t stride_b, int64_t batch, const int* info, void* stream);
int cap_dtrsm_vbatched(const cap_vbatch_plan* p, int uplo, int trans, int64_t nrhs, const double* R, double* B, int64_t ldb, const int* info,
                       double* sumsq, int64_t ldq, void* stream);
int cap_dtrmm_vbatched(const cap_vbatch_plan* p, int uplo, int trans, int64_t nrhs, const double* R, double* B, int64_t ldb, const int* info,
                       void* stream);

/* Batched symmetric rank-k products INTO the layout the batched factor reads (csrc/syrk_batched.hip): the step before cap_dpotrf_batched.
 * For every block the upper triangle of the column-major n x n block C_i (at C + i * stride_c, leading dimension ldc) becomes
 *   beta C_i + alpha op(V_i) op(V_i)^T (+ shift[i] I),   0 <= n <= 256, any k >= 0 (the loop over k is inside the one launch), fp64, one GPU.
 *   trans = CAP_NOTRANS: V_i is n x k column-major at V + i * stride_v with ldv >= n - exactly the V of cap_dcholupdate_batched.
 *   trans = CAP_TRANS:   V_i is k x n column-major with ldv >= k and C = alpha V^T V + beta C - the B / W layout of cap_dpotrs_batched and
 *                        cap_dtrsm_batched, contraction over the rows: with W = R^-T B from cap_dtrsm_batched, alpha = -1, beta = 1 gives the
 *                        Schur complement C - B^T A^-1 B.
 * V is never written and must not overlap C.  shift: NULL, or `batch` device doubles; shift[i] is added to every diagonal element after
 * the alpha / beta combination, with one rounding (ridge and Levenberg-Marquardt terms).  fill: that of cap_dpotri_batched - 1 makes the
 * strictly lower triangle the bit-identical mirror, copied and never computed a second time; the lower triangle is never read.
 * The arithmetic, the same on both paths: s_rc = sum_q v_rq v_cq on the fp64 16 x 16 x 4 MFMA from a zero accumulator with K ascending,
 * four columns per instruction (rows >= n and columns >= k enter as +0.0 and are never addressed); t = alpha * s;
 * out = (beta == 0) ? t : fma(beta, c_old, t); on the diagonal, out = out + shift[i].  beta == 0: C is not read, NaN or Inf there do not
 * propagate.  alpha == 0 or k == 0: V is not addressed and C_i <- beta C_i (+ shift[i] I).
 * The contract is that of the batched entries above: ONE launch per call on a 1-D grid (n <= 64: a wavefront per 64 / NP blocks; above: a
 * workgroup of four waves per block), no `work` argument, no allocation, no memset, no atomics, no mutex, no helper stream, no host
 * synchronisation, nothing between workgroups; asynchronous on `stream`; 64-bit offsets.  The strictly lower triangle of C with fill = 0,
 * rows n .. ld - 1 of every column of C and V, the gaps between blocks and everything behind the last block are never addressed.  A large k
 * with few blocks leaves most of the chip idle: k is not split across workgroups (that would need atomics or scratch).
 * THE BIT CONTRACTS.
 *   1. PLAN = FIXED: every block of a plan call gets the bits of the fixed-size entry on it alone with batch = 1, whichever blocks share
 *      its wavefront or its class.
 *   2. LAYOUT INDEPENDENCE: a block's bits are a function of (n, k, alpha, beta, shift[i], its data) only - not of batch, index, ldc, ldv,
 *      the strides or the alignment.
 *   3. TRANS IS A LAYOUT: the same mathematical V handed over in either layout gives the same bits.
 *   4. ELEMENT INDEPENDENCE: c_rc is a function of rows r and c of V (and k, alpha, beta, c_old, shift[i]) alone: it equals element (0, 1) of
 *      the 2 x 2 block formed from those two rows, for r = c element (0, 0) of the 1 x 1 block - one recurrence on both paths.
 * Argument rules, in this order, all decided before any device call: trans other than CAP_NOTRANS / CAP_TRANS, n < 0, k < 0, batch < 0, fill
 * other than 0 / 1; a NULL C with n batch > 0; a NULL V with n k batch > 0 and alpha != 0; ldc < n; ldv < n (CAP_NOTRANS) or ldv < k
 * (CAP_TRANS); with batch > 1: stride_c < ldc n, stride_v < ldv k (CAP_NOTRANS) or ldv n (CAP_TRANS) -> CAP_ERR_ARG; then uplo = LOWER ->
 * CAP_ERR_UNSUPPORTED; then n > 256 -> CAP_ERR_UNSUPPORTED; then a grid beyond one dimension (2^31 - 1 workgroups) -> CAP_ERR_UNSUPPORTED;
 * then n == 0 or batch == 0 -> CAP_OK without a launch.
 * cap_dsyrk_vbatched: the same on a cap_vbatch_plan.  C is the flat tensor with the plan's offsets and leading dimensions.  CAP_NOTRANS: V
 * is the STACKED (sum n_i) x k matrix with ldv >= sum n_i, as in cap_dcholupdate_vbatched; CAP_TRANS: V is k x (sum n_i) with ldv >= k,
 * block i owning columns row_off[i] .. row_off[i] + n_i.  shift is indexed by the BATCH index i.  One launch per non-empty size class
 * (seven at most); the words of empty blocks are neither read nor written.  Entry rules, in this order: NULL plan, bad trans, k < 0, bad
 * fill, a NULL C / V when something would be launched (V: with k > 0 and alpha != 0), ldv < sum n_i (CAP_NOTRANS) or ldv < k (CAP_TRANS)
 * -> CAP_ERR_ARG; uplo = LOWER -> CAP_ERR_UNSUPPORTED; an empty or all-zero-size plan -> CAP_OK without a launch; a plan made without a
 * device -> CAP_ERR_HIP unless nothing would be launched.                                                                                */
int cap_dsyrk_batched(int uplo, int trans, int64_t n, int64_t k, double alpha, const double* V, int64_t ldv, int64_t stride_v, double beta,
                      double* C, int64_t ldc, int64_t stride_c, const double* shift, int fill, int64_t batch, void* stream);
int cap_dsyrk_vbatched(const cap_vbatch_plan* p, int uplo, int trans, int64_t k, double alpha, const double* V, int64_t ldv, double beta,
                       double* C, const double* shift, int fill, void* stream);

/* Batched products with the SYMMETRIC block itself and the diagnostics built on them (csrc/symm_batched.hip): what says how many digits of
 * cap_dpotrs_batched's and cap_dpotri_batched's answers mean anything.  For every block
 *   Y_i <- beta B_i + alpha A_i X_i,   0 <= n <= 256, any nrhs >= 0 (the passes over nrhs are inside the one launch), fp64, one GPU.
 * A_i is the symmetric n x n block at A + i * stride_a (leading dimension lda) of which only the UPPER triangle of the column-major block
 * holds data - the triangle cap_dpotrf_batched reads and cap_dsyrk_batched / cap_dpotri_batched write.  X_i, B_i, Y_i are n x nrhs
 * column-major, the right-hand-side layout of cap_dpotrs_batched.  absolute = 1 takes |.| of every element of A, X and B on load.
 * The arithmetic, the same on both paths: s_ij = sum_k a_ik x_kj over the symmetrised row (a_ik from (min, max) of the triangle) on the
 * fp64 16 x 16 x 4 MFMA from a zero accumulator with K ascending (rows and columns >= n enter as +0.0 and are never addressed);
 * t = alpha * s; out = (beta == 0) ? t : fma(beta, b, t), without contraction.  beta == 0 never reads B (it may be NULL); alpha == 0 never
 * addresses A or X (they may be NULL).  The strictly lower triangle of A is never read, inside diagonal tiles too; rows n .. ld - 1, the gaps
 * between blocks and everything behind the last block are never read or written.  Y is either EXACTLY B (the same pointer, ld and stride: in
 * place) or disjoint from it; Y must not overlap A or X (refused).  A Y that overlaps B in any other way is not detected and gives undefined
 * results.
 * The contract is that of the batched entries above: ONE launch per call on a 1-D grid (n <= 64: a wavefront per 64 / NP blocks; above: a
 * workgroup of four waves per block), one per occurring size class on a plan; no allocation, no memset, no atomics, no mutex, no helper
 * stream, no host synchronisation, nothing between workgroups; asynchronous on `stream`; 64-bit offsets.
 * cap_dlansy_batched: out[i] = |A_i|_1 = max_j sum_i |a_ij| (norm '1' / 'O' / 'I': by symmetry one number, as cap_dlansy) in ONE launch -
 * the absolute product with a column of ones the kernel supplies itself, then the maximum.  A NaN in the triangle gives NaN.  It is the
 * norm of the matrix BEFORE cap_dpotrf_batched overwrote it.
 * cap_dpocon_batched: EXACT reciprocal condition numbers, not LAPACK's estimate (for blocks this small the inverse is cheaper than the
 * estimator's dependent solves).  R holds the factors cap_dpotrf_batched[_blocked] left and is not written; anorm[i] is |A_i|_1 from
 * cap_dlansy_batched.  The upper triangles are copied into work (cap_dpocon_batched_work_size(n, batch) = n n batch doubles),
 * cap_dpotri_batched runs on the copy, the 1-norm pass runs on the result and rcond[i] = 1 / (anorm[i] * |A_i^-1|_1): one multiplication,
 * one correctly rounded division.  anorm[i] == 0 -> 0; NaN -> NaN; info[i] != 0 (info may be NULL) -> NaN.  FOUR launches, whatever batch.
 * cap_dpoerr_batched: the bounds of LAPACK's dporfs for the solutions X of A X = B (A: the matrix before the factorization, upper triangle;
 * R: its factors; none of A, R, B, X is written).  berr[i * lde + j] = max_r of the guarded ratio of cap_dpoerr,
 * |b - A x|_r / (|A||x| + |b|)_r (safe1 = (n + 1) safmin added to both where the denominator is <= safe2 = safe1 / eps; eps = 2^-53,
 * safmin = 2^-1022); ferr[i * lde + j] = | |A_i^-1| w_j |_inf / |x_j|_inf (x_j = 0: the numerator alone) with w = |r| + (n + 1) eps
 * (|A||x| + |b|) - one rounded multiplication, one rounded addition - and the COMPUTED inverse in place of an estimate of that norm.
 * Either of ferr / berr may be NULL; berr alone needs no inverse, no copy and no work: ONE launch.  With ferr: FOUR launches (residual and
 * weights; copy; cap_dpotri_batched on the copy; the absolute product with its row maxima), whatever batch and nrhs;
 * cap_dpoerr_batched_work_size(n, nrhs, batch) = n (n + nrhs) batch doubles.  A block with info[i] != 0 gets NaN.  The outputs and work of
 * cap_dlansy_batched, cap_dpocon_batched and cap_dpoerr_batched (out, rcond, ferr, berr, work) must be disjoint from one another and from
 * every input (A, R, B, X, anorm, info); that is not checked, an overlap gives undefined results.
 * THE BIT CONTRACTS.
 *   1. PLAN = FIXED: every block of a plan call gets the bits of the fixed-size entry on it alone with batch = 1 - Y, the norm, rcond,
 *      ferr and berr.
 *   2. LAYOUT INDEPENDENCE: a block's bits are a function of (n, its data, alpha, beta, absolute) only - not of batch, index, any ld /
 *      stride or the alignment.
 *   3. COLUMN INDEPENDENCE: a column of Y, and its ferr / berr, do not depend on the columns that travel with it or on the pass it is in.
 *   4. COMPOSITION: the norm equals the maximum of cap_dsymm_batched(absolute = 1) against ones; rcond equals 1 / (anorm * the norm of
 *      cap_dpotri_batched on a copy of R); berr and ferr equal their formulas evaluated on the outputs of cap_dsymm_batched (r: alpha = -1,
 *      beta = 1; |A||x| + |b|: absolute, alpha = beta = 1; |A^-1| w: absolute, alpha = 1, beta = 0), all bit for bit.
 * Argument rules, in this order, all decided before any device call.  cap_dsymm_batched: absolute other than 0 / 1, n < 0, nrhs < 0,
 * batch < 0; with n nrhs batch > 0: a NULL Y, a NULL A or X with alpha != 0, a NULL B with beta != 0; lda < n, ldx < n, ldy < n, with
 * batch > 1 stride_a < lda n, stride_x < ldx nrhs, stride_y < ldy nrhs; with beta != 0 the same for ldb / stride_b; with alpha != 0 a Y that
 * overlaps A or X -> CAP_ERR_ARG; then uplo = LOWER -> CAP_ERR_UNSUPPORTED; then n > 256 -> CAP_ERR_UNSUPPORTED; then a grid beyond one
 * dimension (2^31 - 1 workgroups) -> CAP_ERR_UNSUPPORTED; then n == 0, nrhs == 0 or batch == 0 -> CAP_OK without a launch.
 * cap_dlansy_batched: n < 0, batch < 0; a NULL A or out with n batch > 0; lda / stride_a -> CAP_ERR_ARG; an unknown norm ->
 * CAP_ERR_UNSUPPORTED; then LOWER, n > 256, the grid, the empty call as above.  cap_dpocon_batched: n < 0, batch < 0; a NULL R, anorm, rcond
 * or work with n batch > 0; ldr / stride_r -> CAP_ERR_ARG; then as above.  cap_dpoerr_batched: n < 0, nrhs < 0, batch < 0; with
 * n nrhs batch > 0 and ferr or berr given: a NULL A, B or X, with ferr a NULL R or work; lda / stride_a, with ferr ldr / stride_r, ldb /
 * stride_b, ldx / stride_x; with ferr or berr given lde < nrhs -> CAP_ERR_ARG; then as above (nothing to do: n, nrhs or batch 0, or both
 * outputs NULL).
 * The _vbatched forms: the same on a cap_vbatch_plan.  A, R are flat tensors with the plan's offsets and leading dimensions; X, B, Y are
 * the STACKED system of cap_dpotrs_vbatched ((sum n_i) x nrhs, ld >= sum n_i); out, anorm, info, rcond have `batch` entries in batch order,
 * ferr / berr batch x lde; the entries of empty blocks are neither read nor written.  Launches: cap_dsymm_vbatched and
 * cap_dlansy_vbatched ONE per occurring size class; cap_dpocon_vbatched THREE per class plus ONE (work: the plan's CAP_VBATCH_TOTAL
 * doubles = cap_dpocon_vbatched_work_size); cap_dpoerr_vbatched ONE per class for berr alone, FOUR per class with ferr (work: CAP_VBATCH_TOTAL
 * + (sum n_i) nrhs doubles = cap_dpoerr_vbatched_work_size).  Entry rules, in this order: a NULL plan, bad absolute, nrhs < 0; NULL pointers
 * when something would be launched (as above); a leading dimension of a stacked operand < sum n_i, lde < nrhs; a Y that overlaps A or X ->
 * CAP_ERR_ARG; an unknown norm, uplo = LOWER -> CAP_ERR_UNSUPPORTED; nothing to launch -> CAP_OK; a plan made without a device ->
 * CAP_ERR_HIP.                                                                                                                          */
int cap_dsymm_batched(int uplo, int absolute, int64_t n, int64_t nrhs, double alpha, const double* A, int64_t lda, int64_t stride_a,
                      const double* X, int64_t ldx, int64_t stride_x, double beta, const double* B, int64_t ldb, int64_t stride_b, double* Y,
                      int64_t ldy, int64_t stride_y, int64_t batch, void* stream);
int cap_dsymm_vbatched(const cap_vbatch_plan* p, int uplo, int absolute, int64_t nrhs, double alpha, const double* A, const double* X,
                       int64_t ldx, double beta, const double* B, int64_t ldb, double* Y, int64_t ldy, void* stream);
int cap_dlansy_batched(int norm, int uplo, int64_t n, const double* A, int64_t lda, int64_t stride_a, int64_t batch, double* out, void* stream);
int cap_dlansy_vbatched(const cap_vbatch_plan* p, int norm, int uplo, const double* A, double* out, void* stream);
int64_t cap_dpocon_batched_work_size(int64_t n, int64_t batch);
int64_t cap_dpocon_vbatched_work_size(const cap_vbatch_plan* p);
int cap_dpocon_batched(int uplo, int64_t n, const double* R, int64_t ldr, int64_t stride_r, int64_t batch, const double* anorm, const int* info,
                       double* rcond, double* work, void* stream);
int cap_dpocon_vbatched(const cap_vbatch_plan* p, int uplo, const double* R, const double* anorm, const int* info, double* rcond, double* work,
                        void* stream);
int64_t cap_dpoerr_batched_work_size(int64_t n, int64_t nrhs, int64_t batch);
int64_t cap_dpoerr_vbatched_work_size(const cap_vbatch_plan* p, int64_t nrhs);
int cap_dpoerr_batched(int uplo, int64_t n, int64_t nrhs, const double* A, int64_t lda, int64_t stride_a, const double* R, int64_t ldr,
                       int64_t stride_r, const double* B, int64_t ldb, int64_t stride_b, const double* X, int64_t ldx, int64_t stride_x,
                       int64_t batch, const int* info, double* ferr, double* berr, int64_t lde, double* work, void* stream);
int cap_dpoerr_vbatched(const cap_vbatch_plan* p, int uplo, int64_t nrhs, const double* A, const double* R, const double* B, int64_t ldb,
                        const double* X, int64_t ldx, const int* info, double* ferr, double* berr, int64_t lde, double* work, void* stream);

/* Batched GENERAL products on the block layouts of the batched family (csrc/gemm_batched.hip): the level-3 product with two different
 * operands - the right-hand side X^T y of the normal equations, B_1^T A^-1 B_2 = W_1^T W_2 from two cap_dtrsm_batched results, V_i^T x and
 * V_i z of low-rank-plus-block operators.  For every block the column-major m x n block C_i (at C + i * stride_c, leading dimension ldc)
 * becomes
 *   beta C_i + alpha op(A_i) op(B_i),   0 <= m, n <= 256, any k >= 0 (the loop over k is inside the one launch, k is never split across
 *   workgroups), fp64, one GPU - BLAS dgemm per block.
 *   op(A_i) is m x k: transa = CAP_NOTRANS: A_i is m x k column-major at A + i * stride_a with lda >= m; CAP_TRANS: k x m with lda >= k.
 *   op(B_i) is k x n: transb = CAP_NOTRANS: B_i is k x n with ldb >= k; CAP_TRANS: n x k with ldb >= n.
 * Both transposes are layouts: the loader strides, nothing is copied.  A and B are never written.  The whole m x n rectangle of every C_i
 * is written and nothing else: rows m .. ld - 1 of every column of C, A and B, the gaps between blocks and everything behind the last block
 * are never addressed.
 * The arithmetic, the same on every path: s_rc = sum_q a_rq b_qc on the fp64 16 x 16 x 4 MFMA from a ZERO accumulator with K ascending,
 * four per instruction (rows >= m, columns >= n and k-positions >= k enter as +0.0 and are never addressed); then, without contraction,
 *   t = alpha * s;   out = (beta == 0) ? t : fma(beta, c_old, t).
 * beta == 0 never reads C: NaN and Inf there do not propagate.  alpha == 0 or k == 0 never addresses A or B, and they may be NULL.
 * The contract is that of the batched entries above: ONE launch per fixed-size call on a 1-D grid (max(m, n) <= 64: a wavefront per 64 / NP
 * blocks, NP the padded max(m, n); above: a workgroup of four waves per block), no `work` argument, no allocation, no memset, no atomics,
 * no mutex, no helper stream, no host synchronisation, nothing between workgroups; asynchronous on `stream`; 64-bit offsets.  A large k
 * with few blocks leaves most of the chip idle.
 * cap_dgemm_vbatched_inner, on a cap_vbatch_plan: G_i (m x n at G + i * stride_g, leading dimension ldg, one output per block in BATCH
 * order) becomes beta G_i + alpha X_i^T Y_i.  X is the STACKED (sum n_i) x m matrix and Y the stacked (sum n_i) x n matrix of
 * cap_dpotrs_vbatched (ldx, ldy >= sum n_i); block i owns rows row_off[i] .. row_off[i] + n_i, the contraction length is n_i.  The output
 * size does not depend on the block, so this is ONE launch whatever the plan's classes.  An EMPTY block (n_i = 0) is an empty sum:
 * G_i <- beta G_i, that is alpha * (+0.0) for beta = 0 - deliberately unlike the other plan entries, which skip empty blocks: every G_i of
 * the batch is defined after the call.
 * cap_dgemm_vbatched_combine: C_i (n_i x nrhs, block i's rows of the stacked (sum n_i) x nrhs matrix C, ldc >= sum n_i) becomes
 * beta C_i + alpha V_i Z_i.  V is the stacked (sum n_i) x k matrix of cap_dcholupdate_vbatched / cap_dsyrk_vbatched(CAP_NOTRANS)
 * (ldv >= sum n_i), Z_i is k x nrhs column-major at Z + i * stride_z with ldz >= k, nrhs <= 256.  One launch per occurring size class, seven
 * at most; empty blocks are neither read nor written.  The k x (sum n_i) layout of V is not offered.
 * THE BIT CONTRACTS.
 *   1. PLAN = FIXED: block i of cap_dgemm_vbatched_inner has the bits of cap_dgemm_batched(CAP_TRANS, CAP_NOTRANS, m, n, n_i, ..., batch = 1)
 *      on its rows, block i of cap_dgemm_vbatched_combine those of cap_dgemm_batched(CAP_NOTRANS, CAP_NOTRANS, n_i, nrhs, k, ..., batch = 1),
 *      whichever blocks share its wavefront or its class.
 *   2. LAYOUT INDEPENDENCE: a block's bits are a function of (m, n, k, alpha, beta, its data) only - not of batch, index, any ld or
 *      stride, or the alignment.
 *   3. TRANS IS A LAYOUT: the same mathematical operands under any of the four (transa, transb) give the same bits.
 *   4. ELEMENT INDEPENDENCE: c_rc equals the m = n = 1 product of row r of op(A) and column c of op(B), on the wave path and the
 *      workgroup path alike: a column's bits do not depend on its company.
 *   5. COMPOSITION: with B = A, cap_dgemm_batched(CAP_NOTRANS, CAP_TRANS) gives in its upper triangle the bits of
 *      cap_dsyrk_batched(CAP_NOTRANS) with the same alpha, beta; with A the symmetrised full block, cap_dgemm_batched(CAP_NOTRANS,
 *      CAP_NOTRANS) gives the bits of cap_dsymm_batched.
 * Argument rules, in this order, all decided before any device call.  cap_dgemm_batched: a trans other than CAP_NOTRANS / CAP_TRANS; m, n,
 * k or batch < 0; a NULL C with m n batch > 0; a NULL A or B with m n k batch > 0 and alpha != 0; ldc < m; lda or ldb below the operand's
 * rows as stored; with batch > 1 a stride below ld x the stored columns; with alpha != 0 and k > 0 a C whose span overlaps A's or B's (as
 * cap_dsymm_batched refuses Y) -> CAP_ERR_ARG; then m > 256 or n > 256 -> CAP_ERR_UNSUPPORTED; then a grid beyond one dimension (2^31 - 1
 * workgroups) -> CAP_ERR_UNSUPPORTED; then m == 0, n == 0 or batch == 0 -> CAP_OK without a launch.
 * The plan entries: a NULL plan; negative m / n / nrhs / k; NULL pointers when something would be launched (inner: G with m n batch > 0, X
 * and Y with sum n_i > 0 and alpha != 0 besides; combine: C with nrhs > 0 and a non-empty block, V and Z with k > 0 and alpha != 0
 * besides); a stacked leading dimension < sum n_i; ldg < m; with batch > 1 stride_g < ldg n; ldz < k; with batch > 1 stride_z < ldz nrhs
 * -> CAP_ERR_ARG; then m, n or nrhs > 256 -> CAP_ERR_UNSUPPORTED; then nothing to launch -> CAP_OK; then a plan made without a device ->
 * CAP_ERR_HIP.                                                                                                                          */
int cap_dgemm_batched(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha, const double* A, int64_t lda, int64_t stride_a,
                      const double* B, int64_t ldb, int64_t stride_b, double beta, double* C, int64_t ldc, int64_t stride_c, int64_t batch,
                      void* stream);
int cap_dgemm_vbatched_inner(const cap_vbatch_plan* p, int64_t m, int64_t n, double alpha, const double* X, int64_t ldx, const double* Y,
                             int64_t ldy, double beta, double* G, int64_t ldg, int64_t stride_g, void* stream);
int cap_dgemm_vbatched_combine(const cap_vbatch_plan* p, int64_t nrhs, int64_t k, double alpha, const double* V, int64_t ldv, const double* Z,
                               int64_t ldz, int64_t stride_z, double beta, double* C, int64_t ldc, void* stream);

/* Batched BLOCK-TRIDIAGONAL Cholesky factor and solve (csrc/blocktri_batched.hip): the first operation of the batched family that links
 * blocks to each other - Kalman / RTS smoothers and state-space likelihoods, Gauss-Markov random fields, splines, line-implicit solvers.
 * `batch` independent chains; chain c is the symmetric positive definite block-tridiagonal matrix A_c of T n rows, 1 <= n <= 64, T >= 1,
 * with diagonal blocks D_(c,0) .. D_(c,T-1) and the coupling blocks A_c[block i, block i + 1] = B_(c,i), i = 0 .. T - 2, fp64, one GPU.
 * Block (c, i) of D is the column-major n x n block at D + c * stride_d + i * step_d with leading dimension ldd; only its UPPER triangle
 * is read and written.  E is addressed likewise (lde, step_e, stride_e) and holds T - 1 full n x n blocks per chain: E_(c,i) = B_(c,i).
 * cap_dpotrf_blocktri_batched, in place:
 *   S_0 = D_0;   U_i = chol(S_i), U_i^T U_i = S_i, upper, in the upper triangle of D_i;   W_i = U_i^-T B_i in E_i;
 *   S_(i+1) = D_(i+1) - W_i^T W_i.
 * A_c = R^T R with R block upper bidiagonal (U_i on its diagonal, W_i to the right of U_i).  Read ROW-major the same memory holds the
 * block lower bidiagonal L = R^T with A = L L^T: L_ii in the lower triangle of D[c][i], L_(i+1,i) in E[c][i].
 * info[c] (required) is 0 or the 1-based row of the T n system of the first pivot that is not > 0: i n + the row cap_dpotrf_batched
 * reports for S_i.  logdet may be NULL; logdet[c] = s after s = 0; s += ld_i for i ascending, ld_i what cap_dpotrf_batched returns for S_i
 * (NaN for a failed chain).
 * cap_dpotrs_blocktri_batched: B is the column-major (T n) x nrhs right-hand side of chain c at B + c * stride_b (ldb >= T n), any nrhs
 * (more than NP right-hand sides are further passes inside the launch).  half = 0: A x = b (both sweeps); 1: the forward sweep alone,
 * R^-T b (whitening, log-likelihood terms); 2: the backward sweep alone, R^-1 z (sampling a field with precision A).  info may be NULL;
 * a chain with info[c] != 0 gets NaN.  D and E are not written.
 * THE BIT CONTRACT IS A COMPOSITION: a chain's D, E, info, logdet and solutions are, bit for bit, what the fixed-size entries give when the
 * host drives the recurrence on that chain's blocks.  Factor, i ascending: cap_dpotrf_batched on block i; cap_dtrsm_batched(CAP_TRANS)
 * with that factor and its info on the n columns of E_i; cap_dsyrk_batched(CAP_TRANS, alpha = -1, beta = 1) of E_i into the upper triangle
 * of D_(i+1) (every element its own chain on the fp64 16 x 16 x 4 MFMA from a zero accumulator, K ascending, then t = alpha s,
 * fma(beta, d, t), uncontracted).  Forward sweep, i ascending: cap_dtrsm_batched(CAP_TRANS) on segment i, then cap_dgemm_batched(CAP_TRANS,
 * CAP_NOTRANS, alpha = -1, beta = 1) of E_i and segment i into segment i + 1.  Backward sweep, i descending: cap_dgemm_batched(CAP_NOTRANS,
 * CAP_NOTRANS, -1, 1) of E_i and segment i + 1 into segment i, then cap_dtrsm_batched(CAP_NOTRANS).  half = 1 followed by half = 2 has
 * the bits of half = 0.  CONSEQUENCES: a chain's bits depend on (n, T, its data) alone - not on batch, the chain's index, any leading
 * dimension, step or stride, the alignment, the chains that share its wavefront or the columns that travel with a column.  After a
 * failure at position i, D_i holds what cap_dpotrf_batched leaves, E_i .. E_(T-2) and the upper triangles of D_(i+1) .. D_(T-1) hold NaN,
 * the chain's solutions are NaN and no other chain is affected.
 * The contract is that of the batched entries above: ONE launch per call on a 1-D grid - a wavefront carries 64 / NP chains (NP = 8, 16,
 * 32 or 64 >= n) and walks their positions in a loop inside the kernel - no `work` argument, no scratch, no allocation, no memset, no
 * atomics, no mutex, no helper stream, nothing between workgroups; asynchronous on `stream`; 64-bit offsets.  A chain is sequential in
 * its wavefront: a few long chains leave most of the chip idle.  Position T - 1 addresses no coupling block and no successor, T = 1
 * addresses no E at all (E may then be NULL).  Pad rows, the strictly lower triangles of D, the gaps between blocks and chains and
 * everything behind the last block are never addressed.
 * Argument rules, in this order, all decided before any device call: 1. n, T, nrhs or batch < 0 -> CAP_ERR_ARG; 2. with n T batch (solve:
 * and nrhs) > 0 a NULL D, a NULL info (factor) or B (solve), a NULL E with T > 1 -> CAP_ERR_ARG; 3. ldd or lde (T > 1) < n, with more than
 * one block per chain a step < ld n, with batch > 1 a stride < step x the blocks of a chain (T for D, T - 1 for E; ld n where that is one
 * block), ldb < T n, with batch > 1 stride_b < ldb nrhs, all in 128-bit arithmetic -> CAP_ERR_ARG; 4. half outside 0 .. 2 -> CAP_ERR_ARG;
 * 5. uplo = CAP_LOWER -> CAP_ERR_UNSUPPORTED; 6. n > 64 -> CAP_ERR_UNSUPPORTED; 7. T n > 2^31 - 1 -> CAP_ERR_UNSUPPORTED; 8. a grid beyond
 * one dimension (2^31 - 1 workgroups) -> CAP_ERR_UNSUPPORTED; 9. nothing to do (n, T, batch or nrhs = 0) -> CAP_OK, nothing touched.        */
int cap_dpotrf_blocktri_batched(int uplo, int64_t n, int64_t T, double* D, int64_t ldd, int64_t step_d, int64_t stride_d, double* E, int64_t lde,
                                int64_t step_e, int64_t stride_e, int* info, double* logdet, int64_t batch, void* stream);
int cap_dpotrs_blocktri_batched(int uplo, int half, int64_t n, int64_t T, int64_t nrhs, const double* D, int64_t ldd, int64_t step_d,
                                int64_t stride_d, const double* E, int64_t lde, int64_t step_e, int64_t stride_e, double* B, int64_t ldb,
                                int64_t stride_b, const int* info, int64_t batch, void* stream);

/* Batched BLOCK-TRIDIAGONAL SELECTED INVERSE (csrc/blocktri_potri_batched.hip): the marginal covariances of the chains above from their
 * factors - the diagonal blocks Sigma_(i,i) and the lag-one blocks Sigma_(i,i+1) of Sigma = A_c^-1, the other half of every smoother and
 * Gauss-Markov field fit - without forming the (T n) x (T n) inverse.  D, E and their layout are what cap_dpotrf_blocktri_batched left:
 * U_i in the upper triangle of D_i, W_i = R[i, i + 1] in E_i.  With G_i = U_i^-1 W_i, positions DESCENDING, in place:
 *   P_i = U_i^-1 U_i^-T;   Sigma_(T-1,T-1) = P_(T-1);   C_i = Sigma_(i,i+1) = -G_i Sigma_(i+1,i+1);   Sigma_(i,i) = P_i - C_i G_i^T.
 * The upper triangle of D_i becomes that of Sigma_(i,i), E_i becomes C_i.  Read ROW-major the same memory holds Sigma[block i, block i] in
 * the lower triangle of D[c][i] and Sigma[block i + 1, block i] in E[c][i]: the block-tridiagonal part of the inverse.  fill = 1: the
 * strictly lower triangle of every D block becomes the bit-identical mirror, copied and never computed a second time; fill = 0: it is
 * never addressed.  info is read and may be NULL: a chain with info[c] != 0 gets NaN wherever the call writes and no other chain is
 * touched.  A zero on a diagonal is not detected (as cap_dtrtri_batched).  The factor is overwritten: clone it first if it is still needed.
 * THE BIT CONTRACT IS A COMPOSITION: a chain's D and E are, bit for bit, what the host-driven loop gives on the chain's blocks, positions
 * descending: 1. cap_dtrsm_batched(CAP_NOTRANS) with U_i and the chain's info on the n columns of E_i -> G_i; 2. cap_dpotri_batched(fill = 1)
 * on U_i -> P_i; 3. cap_dgemm_batched(CAP_NOTRANS, CAP_NOTRANS, alpha = -1, beta = 0) of G_i and the MIRRORED Sigma_(i+1,i+1) -> C_i (every
 * element its own chain on the fp64 16 x 16 x 4 MFMA from a zero accumulator, K ascending, rows at or beyond n as +0.0, t = alpha s);
 * 4. cap_dgemm_batched(CAP_NOTRANS, CAP_TRANS, alpha = -1, beta = 1) of C_i and G_i into P_i, out = fma(beta, p, t), uncontracted - ONLY THE
 * UPPER TRIANGLE of that result is Sigma_(i,i) (the two triangles of the product differ in rounding) and the operand of position i - 1 is
 * the mirror of that triangle.  CONSEQUENCES: a chain's bits depend on (n, T, its data) alone - not on batch, the chain's index, any
 * leading dimension, step or stride, the chains that share its wavefront or fill.
 * ONE launch per call on a 1-D grid - a wavefront carries 64 / NP chains and walks positions T - 1 .. 0 inside the kernel - no `work`
 * argument, no scratch, no allocation, no memset, no atomics, no helper stream, nothing between workgroups; asynchronous on `stream`;
 * 64-bit offsets.  Position 0 has no predecessor, position T - 1 no coupling block, T = 1 addresses no E at all (E may then be NULL).  Pad
 * rows, the gaps between blocks and chains and everything behind the last block are never addressed.
 * Argument rules, in this order, all decided before any device call: 1. n, T or batch < 0 -> CAP_ERR_ARG; 2. with n T batch > 0 a NULL D,
 * a NULL E with T > 1 -> CAP_ERR_ARG; 3. the layout rule of the factor (rule 3 above, without B), in 128-bit arithmetic -> CAP_ERR_ARG;
 * 4. fill outside 0 .. 1 -> CAP_ERR_ARG; 5. uplo = CAP_LOWER -> CAP_ERR_UNSUPPORTED; 6. n > 64 -> CAP_ERR_UNSUPPORTED; 7. T n > 2^31 - 1 ->
 * CAP_ERR_UNSUPPORTED; 8. a grid beyond one dimension -> CAP_ERR_UNSUPPORTED; 9. nothing to do (n, T or batch = 0) -> CAP_OK, nothing touched. */
int cap_dpotri_blocktri_batched(int uplo, int fill, int64_t n, int64_t T, double* D, int64_t ldd, int64_t step_d, int64_t stride_d, double* E,
                                int64_t lde, int64_t step_e, int64_t stride_e, const int* info, int64_t batch, void* stream);

/* RAGGED block-tridiagonal chains (csrc/blocktri_vbatched.hip): the three entries above for a batch whose chains have DIFFERENT lengths
 * T_c >= 0 - time series, smoothers and likelihoods come in ragged batches - on a plan over the lengths, as the other members of the
 * family have a _vbatched form on a cap_vbatch_plan.  ONE launch per call; every chain gets, bit for bit, what the fixed-size entry
 * writes for it alone (T = T_c, batch = 1): D, E, the solutions, info[c], logdet[c] - whichever chains share its wavefront or the batch,
 * whatever `first`, the batch order, the leading dimensions and the steps, with and without fill; half = 1 followed by half = 2 leaves the
 * bits of half = 0, and the composition contracts of the fixed-size entries carry over.
 * THE PLAN.  cap_blocktri_plan_create(batch, T, first, &p): T and first are HOST arrays of batch entries.  D is one sequence of n x n
 * SLOTS, step_d apart with leading dimension ldd (both given per call: the plan knows no n and serves any n <= 64, one n per call); chain
 * c owns slots first[c] .. first[c] + T[c] - 1; first = NULL: the chains lie back to back in batch order (the prefix sum of T).  E is
 * addressed with the SAME slot indices: slot first[c] + i holds the coupling between positions i and i + 1 of chain c, the last slot of
 * every chain, first[c] + T[c] - 1, is never addressed (D and E can be two tensors of one shape); E may be NULL when no chain has more
 * than one position.  T[c] = 0 is legal: nothing of that chain is touched, info[c] and logdet[c] are NOT written.
 * create: 1. NULL out, batch < 0, NULL T with batch > 0 -> CAP_ERR_ARG; 2. a T[c] < 0 or first[c] < 0 -> CAP_ERR_ARG; 3. two non-empty
 * chains whose slot ranges meet -> CAP_ERR_ARG; 4. sums beyond int64 -> CAP_ERR_ARG.  It sorts the chains STABLY BY T DESCENDING into one
 * list (cap_blocktri_plan_order copies up to cap entries of it to the host): the 64 / NP chains of a wavefront are neighbours of that
 * list, and the longest start first.  The records and the list are uploaded with synchronous copies: create and destroy MAY SYNCHRONISE,
 * no other function does.  In a process without a device create succeeds and the plan serves _info and _order only.  The plan is read-only
 * afterwards: usable from several streams and host threads at once, on the device that was current when it was made.
 * cap_blocktri_plan_info(p, what): CAP_BLOCKTRI_BATCH; _SLOTS = max(first + T) over the non-empty chains; _ESLOTS = the largest addressed
 * coupling slot + 1 (0: no chain has two positions); _ROWS = sum T; _TMAX = the longest chain; -1 for anything else or a NULL plan.
 * THE ENTRIES.  1 <= n <= 64; the grid is ceil(batch / (64 / NP)) wavefronts over the sorted list, each walking to the largest T of its
 * chains.  info and logdet have batch entries in BATCH order; info[c] is 0 or the 1-based row inside chain c's own T[c] n system of the
 * first pivot that is not > 0.  B is the STACKED system, (n ROWS) x nrhs column-major with ldb >= n ROWS: chain c owns rows n row[c] ..
 * n (row[c] + T[c]), row the prefix sum of T in batch order (as cap_dpotrs_vbatched stacks blocks).  half, fill, failure and NaN
 * conventions are those of the fixed-size entries.  No `work`, scratch, allocation, memset, atomics or helper stream; asynchronous on
 * `stream`; 64-bit offsets.  Pad rows, gaps between slots, slots no chain owns and every chain's last slot of E are never addressed.
 * Argument rules, in this order, all before any device call: 1. NULL plan, n < 0 or nrhs < 0 -> CAP_ERR_ARG; 2. with something to launch
 * a NULL D, a NULL info (factor) or B (solve), a NULL E while some chain has T > 1 -> CAP_ERR_ARG; 3. ldd < n; lde < n when E is used;
 * step < ld n when the plan spans more than one slot; ldb < n ROWS - in 128-bit arithmetic -> CAP_ERR_ARG; 4. half or fill out of range
 * -> CAP_ERR_ARG; 5. uplo = CAP_LOWER -> CAP_ERR_UNSUPPORTED; 6. n > 64 -> CAP_ERR_UNSUPPORTED; 7. n TMAX > 2^31 - 1 ->
 * CAP_ERR_UNSUPPORTED; 8. a grid beyond one dimension -> CAP_ERR_UNSUPPORTED; 9. nothing to do (n = 0, an empty or all-empty plan, nrhs
 * = 0) -> CAP_OK without a launch; 10. a plan made without a device -> CAP_ERR_HIP. */
typedef struct cap_blocktri_plan cap_blocktri_plan;
enum { CAP_BLOCKTRI_BATCH = 0, CAP_BLOCKTRI_SLOTS = 1, CAP_BLOCKTRI_ESLOTS = 2, CAP_BLOCKTRI_ROWS = 3, CAP_BLOCKTRI_TMAX = 4 };
int cap_blocktri_plan_create(int64_t batch, const int64_t* T, const int64_t* first, cap_blocktri_plan** out);
int cap_blocktri_plan_destroy(cap_blocktri_plan* p);
int64_t cap_blocktri_plan_info(const cap_blocktri_plan* p, int what);
int cap_blocktri_plan_order(const cap_blocktri_plan* p, int64_t* chains, int64_t cap);
int cap_dpotrf_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int64_t n, double* D, int64_t ldd, int64_t step_d, double* E, int64_t lde,
                                 int64_t step_e, int* info, double* logdet, void* stream);
int cap_dpotrs_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int half, int64_t n, int64_t nrhs, const double* D, int64_t ldd,
                                 int64_t step_d, const double* E, int64_t lde, int64_t step_e, double* B, int64_t ldb, const int* info, void* stream);
int cap_dpotri_blocktri_vbatched(const cap_blocktri_plan* p, int uplo, int fill, int64_t n, double* D, int64_t ldd, int64_t step_d, double* E,
                                 int64_t lde, int64_t step_e, const int* info, void* stream);

/* Batched PIVOTED Cholesky factorization for symmetric positive SEMIdefinite blocks of up to 64 rows (csrc/pstrf_batched.hip): cap_dpstrf
 * on every block of a batch in ONE launch - numerical rank, a factor that survives zero pivots, the trace error of the low-rank
 * approximation - where cap_dpotrf_batched turns a block into NaN at the first pivot that is not > 0.  For every block
 *   A_i[piv_i][:, piv_i] ~ R_i^T R_i,   1 <= n <= 64, 0 <= max_rank <= n, fp64, one GPU.
 * A_i is the n x n column-major block at A + i * stride_a (leading dimension lda); only its UPPER triangle is read (the strictly lower one
 * may hold anything) and A is never written.  R_i is max_rank x n column-major at R + i * stride_r with ldr >= max(max_rank, 1) and, for
 * batch > 1, stride_r >= ldr n.  R MUST NOT OVERLAP A: that is not checked, an overlap gives undefined results.  piv is batch x n int64,
 * block i at piv + i n, 0-based; rank (required) and info (may be NULL) are int32 per block; resid and logdet are doubles per block and may
 * be NULL.
 * The steps are those of cap_dpstrf, per block.  d = the remaining diagonal (initially diag A_i).  In front of step j = 0, 1, ...: p = the
 * unselected index of largest d (ties: the lowest index).  A NaN among the unselected d: stop, info = 2.  No unselected index, or
 * !(d[p] > tol_used): stop, info = 0.  j = max_rank: stop, info = 1.  tol_used = tol < 0 ? n 2^-53 max_i a_ii : tol, formed in front of step
 * 0.  Otherwise, THE STATED RECURRENCE: for each unselected c != p, t = A(p, c); t = fma(-W[i, p], W[i, c], t) for i = 0 .. j - 1 in
 * ascending order; r = t / sqrt(d[p]); W[j, c] = r; d[c] = fma(-r, r, d[c]); W[j, p] = sqrt(d[p]); W[j, c] = +0.0 for the columns chosen
 * earlier - the square root and the division correctly rounded.  (cap_dpstrf forms the same sums in another order: its bits differ.)
 * Results: rank[i] = the steps done; piv_i = the chosen pivots in order, then the unselected indices in increasing order - always a
 * permutation; R_i[:, k] = W[:, piv_i[k]] with rows rank .. max_rank - 1 equal to +0.0: the WHOLE max_rank x n rectangle of every block is
 * written, rows >= max_rank, padding and gaps are not touched; resid[i] = s after s = 0; s += d[c] over the unselected c in ascending
 * order = trace(A_i - R_i^T R_i); logdet[i] = 2 sum_{j < rank} log r_jj added in ascending j as cap_dpotrf_batched does - the
 * pseudo-log-determinant of a degenerate Gaussian - and NaN for info = 2; info[i] as above.  info = 2 is a result, not an error: the call
 * returns CAP_OK, rank = the steps done and the finished rows of R are intact.  max_rank = 0 is legal: rank 0, the identity piv, resid =
 * trace A_i, info 0 or 1.  NOTE: this info (0 / 1 / 2) is NOT the info of cap_dpotrf_batched that cap_dpotrs_batched, cap_dtrsm_batched and
 * cap_dtrmm_batched expect.
 * THE BIT CONTRACT: a block's bits - R, piv, rank, resid, logdet, info - depend on (n, max_rank, tol, its data) alone.  They do not depend
 * on batch, the block's index, lda / ldr, the strides, the alignment or the blocks that share its wave.  PLAN = FIXED: cap_dpstrf_vbatched
 * gives every block the bits of cap_dpstrf_batched on it alone with n = n_i, max_rank = min(max_rank, n_i) and batch = 1.
 * The contract is that of the batched entries above: ONE launch per call on a 1-D grid (a wavefront per 64 / NP blocks, NP = 8, 16, 32 or
 * 64 >= n), one per occurring size class on a plan; no work argument, no allocation, no memset, no atomics, no mutex, no helper stream, no
 * host synchronisation, nothing between workgroups; asynchronous on `stream`; 64-bit offsets.
 * Argument rules, in this order, all decided before any device call.  n < 0, batch < 0, max_rank < 0, max_rank > n, a NaN tol ->
 * CAP_ERR_ARG; with n batch > 0: a NULL A, piv or rank, with max_rank > 0 a NULL R; lda < n, with batch > 1 stride_a < lda n; with
 * max_rank > 0: ldr < max_rank, with batch > 1 stride_r < ldr n -> CAP_ERR_ARG; then uplo = LOWER -> CAP_ERR_UNSUPPORTED (as cap_dpstrf: in
 * front of the empty case); then n > 64 (use cap_dpstrf per block) -> CAP_ERR_UNSUPPORTED; then a grid beyond one dimension (2^31 - 1
 * workgroups) -> CAP_ERR_UNSUPPORTED, nothing written; then n == 0 or batch == 0 -> CAP_OK, nothing touched.
 * cap_dpstrf_vbatched: the same on a cap_vbatch_plan.  A and R are two flat tensors in the plan's own layout (offsets and leading
 * dimensions); R gets EVERY entry of every n_i x n_i block (rows >= rank are +0.0), padding and gaps are untouched; the cap of block i is
 * min(max_rank, n_i).  piv is the stacked vector of sum n_i block-local 0-based indices, block i at the prefix sum of n in batch order
 * (the rows of cap_dpotrs_vbatched's right-hand sides); rank, resid, logdet, info have `batch` entries in batch order, and the entries of
 * empty blocks are neither read nor written (capital_amd.batched hands out zeros for them).  ONE launch per occurring size class.  Entry
 * rules, in this order: a NULL plan, max_rank < 0, a NaN tol; with a non-empty plan a NULL A, piv or rank, with max_rank > 0 a NULL R ->
 * CAP_ERR_ARG; uplo = LOWER -> CAP_ERR_UNSUPPORTED; a plan whose largest block exceeds 64 -> CAP_ERR_UNSUPPORTED, nothing written; nothing
 * to launch -> CAP_OK; a plan made without a device -> CAP_ERR_HIP.  (With max_rank = 0 a NULL R is legal and nothing of R is written.)      */
int cap_dpstrf_batched(int uplo, int64_t n, int64_t max_rank, double tol, const double* A, int64_t lda, int64_t stride_a, double* R,
                       int64_t ldr, int64_t stride_r, int64_t* piv, int* rank, double* resid, double* logdet, int* info, int64_t batch,
                       void* stream);
int cap_dpstrf_vbatched(const cap_vbatch_plan* p, int uplo, int64_t max_rank, double tol, const double* A, double* R, int64_t* piv, int* rank,
                        double* resid, double* logdet, int* info, void* stream);

/* Y = beta opB(B) + alpha op(A) opX(X) for a SYMMETRIC n x n A of which only the upper triangle holds data, and a thin block: X, B, Y are
 * n x nrhs, column-major device memory (not in the reference; the product behind cap_dlansy and the residuals of cap_dpoerr).  absolute = 1
 * takes |.| of every element of A, X and B before use (|A||X| + |B|); absolute = 0 uses them as they are.
 * beta == 0 never reads B (it may be NULL; NaN in it cannot reach Y); alpha == 0 never reads A, X or work.  Y may be B (in place).  The
 * strictly lower triangle of A is never read, inside diagonal tiles too; rows >= n of A, X, B (padding) are never read, those of Y never
 * written.  Any lda / ldx / ldb / ldy >= n, any 8-byte aligned pointers, any nrhs >= 0: more than 16 columns are taken in chunks of 16,
 * one pass over the triangle each.
 * Negative n or nrhs, absolute other than 0 / 1, a NaN alpha or beta -> CAP_ERR_ARG; with n > 0 and nrhs > 0: NULL Y or ldy < n; with
 * alpha != 0: NULL A, X or work, lda < n, ldx < n; with beta != 0: NULL B or ldb < n; the address range of Y meeting that of A, X or work
 * (alpha != 0) -> CAP_ERR_ARG; then uplo = LOWER -> CAP_ERR_UNSUPPORTED; n == 0 or nrhs == 0 -> CAP_OK, nothing touched.
 * Asynchronous on `stream`, no host synchronisation.  csrc/symv.hip: one workgroup per 512 x 512 super-block of the upper block triangle
 * streams it once through LDS and uses every element for both A_IJ X_J and A_IJ^T X_I, the parts go to the super-block's own slot of
 * `work`, a second launch adds the parts of each block row in a fixed order and applies alpha, beta and B.  No floating-point atomics:
 * two calls give the same bits.  work >= cap_dsymm_thin_work_size(n, nrhs) doubles (0 for an empty problem, monotone in both arguments,
 * constant beyond 16 columns).                                                                                                        */
int cap_dsymm_thin(int uplo, int absolute, int64_t n, int64_t nrhs, double alpha, const double* A, int64_t lda, const double* X,
                   int64_t ldx, double beta, const double* B, int64_t ldb, double* Y, int64_t ldy, double* work, void* stream);
int64_t cap_dsymm_thin_work_size(int64_t n, int64_t nrhs);

/* LAPACK dlansy for the 1-norm: *out_dev (ONE device double) = max_j sum_i |a_ij| of the symmetric A, from its upper triangle alone
 * (the strictly lower one is never read).  norm = '1', 'O' or 'I' (equal for a symmetric matrix); any other norm -> CAP_ERR_UNSUPPORTED.
 * It is cap_dsymm_thin's absolute product with a column of ones that the kernel supplies itself, followed by a maximum.  A NaN in the
 * upper triangle gives NaN (as LAPACK).  Negative n, NULL out_dev; with n > 0: NULL A or work, lda < n -> CAP_ERR_ARG; then the norm and
 * uplo = LOWER -> CAP_ERR_UNSUPPORTED; n == 0 -> *out_dev = 0.  Asynchronous, deterministic.  work >= cap_dlansy_work_size(n) doubles.   */
int cap_dlansy(int norm, int uplo, int64_t n, const double* A, int64_t lda, double* out_dev, double* work, void* stream);
int64_t cap_dlansy_work_size(int64_t n);

/* LAPACK dpocon beside cap_dpotrf: *rcond_dev (ONE device double) = 1 / (anorm est), est = LAPACK's estimate of ||A^-1||_1 for A = R^T R,
 * R the upper factor (the other triangle is not referenced), *anorm_dev = ||A||_1 (cap_dlansy) in device memory.  est is a LOWER
 * bound of ||A^-1||_1, so rcond >= the true reciprocal condition number up to rounding: the estimate is optimistic, in practice by less than a
 * factor 3 (1.0 - 1.4 on the matrices of tests/test_gpu_pocon.py).
 * The estimator (csrc/pocon.hip) is dlacn2 exactly - start vector 1 / n, sign vectors, the stop at a repeated sign vector or an estimate
 * that did not grow, arg max with the lowest index winning ties, at most 5 iterations, the final alternating-sign vector with its
 * 2 |x|_1 / (3 n) floor - run on the device: its state lives in device memory, one step is one solve with R (the two substitutions of
 * cap_dpotrs, the inverses of R's diagonal blocks made ONCE per call) and a small kernel that takes the step's decision.  No host
 * synchronisation: the 11 solves dlacn2 can need are always enqueued, and the ones behind the last decision return at once (4 - 5 are
 * typical).  Fixed reduction orders: two calls give the same bits.  LAPACK's overflow rescaling (dlatrs' scale) is not reproduced.
 * n == 0 -> 1; *anorm_dev == 0 -> 0; NaN anorm -> NaN.  Negative n, NULL rcond_dev; with n > 0: NULL R, anorm_dev or work, ldr < n ->
 * CAP_ERR_ARG; then uplo = LOWER -> CAP_ERR_UNSUPPORTED.  work >= cap_dpocon_work_size(n) doubles.
 * cap_pocon_last_solves: DIAGNOSTIC - the number of solves the last estimate on the current device actually took, the largest over the
 * columns of its LAST chunk of 16 (cap_dpoerr with more columns reports the last chunk only); one word per device, written with a plain
 * store: estimates running at the same time on several streams overwrite each other's count (synchronises the device).                                                                                                  */
int cap_dpocon(int uplo, int64_t n, const double* R, int64_t ldr, const double* anorm_dev, double* rcond_dev, double* work, void* stream);
int64_t cap_dpocon_work_size(int64_t n);
int64_t cap_pocon_last_solves(void);

/* The bounds of LAPACK dporfs WITHOUT its refinement (an fp64 Cholesky solve already has a componentwise backward error of a few eps,
 * which refinement does not improve): X (n x nrhs) is a computed solution of A X = B, A symmetric with its upper triangle given (the
 * strictly lower one is never read), R its upper factor.  Per column j, device arrays of nrhs doubles, either may be NULL:
 *   berr[j] = max_i |B - A X|_i / (|A||X| + |B|)_i, the componentwise backward error, with LAPACK's guard: where the denominator is
 *             <= safe2 = safe1 / eps, safe1 = (n + 1) safmin is added to numerator and denominator;
 *   ferr[j] = est || |A^-1| (|r_j| + (n + 1) eps (|A||x_j| + |b_j|)) ||_inf / ||x_j||_inf, a bound of ||x_j - x*||_inf / ||x_j||_inf, by
 *             cap_dpocon's estimator on diag(w) A^-1, up to 16 columns in lock-step (x_j == 0: the numerator alone, as LAPACK).
 * eps = 2^-53, safmin = 2^-1022 (dlamch).  Cost: two passes over A's upper triangle per 16 columns (cap_dsymm_thin: the residual, then
 * the absolute product), and for ferr the estimator's solves with 16 columns each.  Nothing is written but ferr, berr and work.
 * Negative n or nrhs; with n > 0 and nrhs > 0: NULL A, R, B, X or work, lda / ldr / ldb / ldx < n -> CAP_ERR_ARG; then uplo = LOWER ->
 * CAP_ERR_UNSUPPORTED; nrhs == 0 -> CAP_OK; n == 0 -> both bounds 0.  Asynchronous, no host synchronisation, deterministic.
 * work >= cap_dpoerr_work_size(n, nrhs) doubles.                                                                                      */
int cap_dpoerr(int uplo, int64_t n, int64_t nrhs, const double* A, int64_t lda, const double* R, int64_t ldr, const double* B, int64_t ldb,
               const double* X, int64_t ldx, double* ferr_dev, double* berr_dev, double* work, void* stream);
int64_t cap_dpoerr_work_size(int64_t n, int64_t nrhs);

/* Z[n x nrhs] = Q^T B for a tall-skinny Q (m x n, m >> n) and a few right-hand sides B (m x nrhs), all column-major in device memory
 * (not in the reference: the expensive step of a least-squares solve on a QR factorization, cap_cacqr_solve below).  Z is overwritten,
 * its padding rows (ldz > n) are not touched; Z must not overlap Q, B or work.
 * n % 16 == 0, n <= 256, m % 8 == 0, even ldq / ldb, 16-byte aligned Q and B, nrhs <= 48: the streaming kernel of csrc/cqr_solve.hip - the
 * ROWS of Q are split into slabs over the whole chip, Q is read once per 16 right-hand sides, the slabs' partial sums go through `work` and
 * are added in a fixed order (no floating-point atomics: two calls give the same bits; accumulators restart every 64 rows).  Bound by HBM.
 * Every other shape (other n, a ragged m, odd leading dimensions, unaligned operands, more right-hand sides) is the same product
 * through the 128 x 128 tile kernels of cap_dgemm(CAP_TRANS, CAP_NOTRANS, n, nrhs, m): correct, and several times slower for a few
 * right-hand sides (they are padded to 128).  work >= cap_dgemm_tall_tn_work_size(m, n, nrhs) doubles.                               */
int64_t cap_dgemm_tall_tn_work_size(int64_t m, int64_t n, int64_t nrhs);
int cap_dgemm_tall_tn(int64_t m, int64_t n, int64_t nrhs, const double* Q, int64_t ldq, const double* B, int64_t ldb, double* Z,
                      int64_t ldz, double* work, void* stream);

/* The two streaming kernels of a CholeskyQR sweep at n = 256 columns (csrc/cqr_kernels.hip), on their own (not in the reference; the
 * plan calls of cap_cacqr_factor run exactly these launches).  Kernel-level entries: whatever the kernels cannot run is refused with
 * CAP_ERR_UNSUPPORTED before anything is launched or written - there is no other route behind them.  All operands column-major in
 * device memory.  max_wgs = 0: one workgroup per CU as the plans launch them; max_wgs > 0 caps the grid (a test gives one workgroup
 * several row tiles at a small m with it, whatever the device's CU count); max_wgs < 0 is refused.  Asynchronous, deterministic.
 *
 * cap_dgram256     G = Q^T Q for Q m x 256: the upper triangle of the 256 x 256 square of G is written, its strictly-lower part is
 *                  set to 0.0, rows >= 256 of G (ldg > 256) and Q are not touched.  min(CUs, m / 512, max_wgs) (at least one) workgroups
 *                  own one slab of rows each, their partial Grams go through `work` (one 256 x 256 slab per workgroup, every slab
 *                  written, also by a workgroup without rows) and are added in a fixed order: two calls give the same bits.
 *                  m > 0, m % 16 == 0, ldq >= m and even, Q 16-byte aligned, ldg >= 256 (odd allowed), 128 * ldq * 8 < 0xfffffff0
 *                  (ldq <= 4194302: the kernel's 32-bit byte offsets), non-NULL Q, G, work; work >= cap_dgram256_work_size(m)
 *                  doubles (the uncapped slab count; 0 for m <= 0).  G and work must not overlap Q or each other.
 * cap_dqrapply256  Qout = Qin * Ri for Qin, Qout m x 256 and Ri 256 x 256 with leading dimension 256, upper triangular with its
 *                  strictly-lower part ZERO inside the 16 x 16 diagonal blocks (read as stored); the 16 x 16 blocks below the block
 *                  diagonal are never read.  min(CUs, m / 128, max_wgs) persistent workgroups walk consecutive row tiles of 128
 *                  rows.  Rows >= m of Qout (ldout > m) are not touched.  In place (Qout == Qin, ldout == ldin) is allowed; any other
 *                  overlap is not.  m > 0, m % 128 == 0, ldin >= m and even, ldout >= m, Qin and Ri 16-byte aligned (Qout: 8),
 *                  ldin and ldout <= 35791385 (15 * ld * 8 + 1024 < 0xfffffff0: rows of a tile are addressed by 32-bit byte
 *                  offsets of up to 15 columns), non-NULL Qin, Ri, Qout.                                                            */
int64_t cap_dgram256_work_size(int64_t m);
int cap_dgram256(int64_t m, const double* Q, int64_t ldq, double* G, int64_t ldg, double* work, int64_t max_wgs, void* stream);
int cap_dqrapply256(int64_t m, const double* Qin, int64_t ldin, const double* Ri, double* Qout, int64_t ldout, int64_t max_wgs,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * Matrix descriptor helpers (replaces src/matrix/: generators, serialize, structure)
 * ---------------------------------------------------------------------------------- */

/* matrix<T,U,Structure> descriptor - matrix.h:9-97: global dims (X = columns, Y = rows, upstream's naming), process
 * grid, local element-cyclic dims ceil(global / grid) (matrix.hpp:8-11), one column-major HBM buffer and its ownership:
 * cap_desc_create allocates (zero-filled; matrix.hpp:5-50,141-155), cap_desc_create_view is the injection constructor
 * (matrix.hpp:52-74: the caller keeps ownership of `device_data`), destroy frees only what the descriptor owns
 * (matrix.hpp:157-169).  import / export move the local piece between HOST memory (column-major, ld_host) and HBM
 * through two pinned 64 MiB chunk buffers, overlapping the host-side copy of one chunk with the PCIe transfer of the
 * other; a host pointer that is already pinned is copied directly.  import is ordered on `stream`; export blocks
 * until the host buffer is complete.  cap_desc_get: 0 global cols, 1 global rows, 2 local cols, 3 local rows, 4 ld,
 * 5 owns, 6 grid x, 7 grid y, 8 local element count.                                                                  */
typedef struct cap_desc cap_desc;
int cap_desc_create(cap_desc** desc, int64_t global_cols, int64_t global_rows, int64_t grid_x, int64_t grid_y);
int cap_desc_create_view(cap_desc** desc, int64_t global_cols, int64_t global_rows, int64_t grid_x, int64_t grid_y,
                         double* device_data, int64_t ld);
/* BLOCK-CYCLIC kind (north_star's "2D block-cyclic matrix descriptor"; upstream has only the element-cyclic map, matrix.hpp:8-11): nb x nb
 * blocks, block (I, J) on process (I mod Pr, J mod Pc) as local block (I div Pr, J div Pc).  The descriptor is the piece of process
 * (pr, pc): the VALID local rows x columns, compact, column-major - what cap_dist2d_factor / cap_dist2d_get_R take, and with Pr = 1 the
 * block columns of a multi-rank cap_cholinv_plan / cap_dist_plan.  device_data = NULL: allocated, zero-filled and owned; otherwise the
 * injection constructor (matrix.hpp:52-74) with leading dimension ld.  An empty piece (more processes than blocks) is valid.       */
int cap_desc_create_bc(cap_desc** desc, int64_t global_cols, int64_t global_rows, int64_t nb, int Pr, int Pc, int pr, int pc,
                       double* device_data, int64_t ld);
/* element-cyclic descriptors do not store their grid position (upstream passes (x, y) to the generators again, matrix.h:65-68);
 * the GLOBAL import / export below need it.                                                                                      */
int cap_desc_set_position(cap_desc* desc, int64_t x, int64_t y);
int cap_desc_destroy(cap_desc* desc);
double* cap_desc_data(cap_desc* desc);
int64_t cap_desc_get(const cap_desc* desc, int field);
int cap_desc_import_host(cap_desc* desc, const double* host, int64_t ld_host, void* stream);
int cap_desc_export_host(cap_desc* desc, double* host, int64_t ld_host, void* stream);
/* The caller holds the GLOBAL matrix in host memory (column-major, ld_host >= global rows: upstream's matrix<> on one rank, or what
 * a host application hands to a distributed solver): import picks this process's blocks (block-cyclic kind) or elements
 * (element-cyclic kind with cap_desc_set_position) out of it, export writes them back to their global places and touches nothing
 * else - every rank exporting into its own zero-filled copy and summing the copies assembles the global result.  Through the same
 * two pinned 64 MiB buffers: host threads pack / unpack one range of local columns while the previous one is on the PCIe link.
 * cap_desc_get adds: 9 kind (0 element-cyclic, 1 block-cyclic), 10 nb, 11 my grid column (pc / x; -1 unknown), 12 my grid row.  */
int cap_desc_import_host_global(cap_desc* desc, const double* host_global, int64_t ld_host, void* stream);
int cap_desc_export_host_global(cap_desc* desc, double* host_global, int64_t ld_host, void* stream);

/* rect::_distribute_symmetric - structure.hpp:68-103.  Fills the local element-cyclic piece
 * (grid position x,y of a d x d grid) of the N x N SPD test matrix directly on the GPU:
 * A[gy,gx] = u(max + N*min) (+N on the diagonal), u = srand48/drand48 closed form.
 * local: ceil(N/d) x ceil(N/d) column-major with leading dimension ld; padding zero-filled. */
int cap_fill_symmetric(double* local, int64_t ld, int64_t n_global, int64_t x, int64_t y, int64_t d,
                       int diagonally_dominant, void* stream);
/* rect::_distribute_random - structure.hpp:105-129 (sequential drand48 stream per rank,
 * key = rank / c; jump-ahead LCG so every element is computed independently, bit-exact).   */
int cap_fill_random(double* local, int64_t ld, int64_t m_global, int64_t n_global, int64_t x, int64_t y,
                    int64_t dx, int64_t dy, int64_t key, void* stream);

/* serialize<S1,S2>::invoke - serialize.hpp:12-150: copy a window between rect / packed-upper
 * buffers.  src/dst are either column-major rect (packed = 0, leading dim ld) or packed upper
 * (packed = 1: column x at x(x+1)/2, structure.h:39; ld ignored).  Copies the n x n window's
 * upper triangle (tri_only = 1) or the full rows x cols window (tri_only = 0).
 * zero_lower = 1 additionally zero-fills the strictly lower part of a rect destination.     */
int cap_copy_window(const double* src, int src_packed, int64_t src_ld, int64_t src_row0, int64_t src_col0,
                    double* dst, int dst_packed, int64_t dst_ld, int64_t dst_row0, int64_t dst_col0,
                    int64_t rows, int64_t cols, int tri_only, int zero_lower, void* stream);

/* Element-cyclic layout of the reference (matrix.hpp:8-11; util::block_to_cyclic_* / cyclic_to_local,
 * util.hpp:56-230): piece (x, y) of a dx x dy grid holds global rows y, y+dy, ... and columns x, x+dx, ...
 * (ceil sizes, zero padded).  import scatters one piece into a dense m x n matrix, export extracts it - so a
 * caller holding upstream-style cyclic pieces can assemble / split the dense operand of the GPU plans.      */
int cap_cyclic_import(const double* piece, int64_t ldp, double* dense, int64_t ldd, int64_t m, int64_t n, int64_t x, int64_t y,
                      int64_t dx, int64_t dy, void* stream);
int cap_cyclic_export(const double* dense, int64_t ldd, double* piece, int64_t ldp, int64_t m, int64_t n, int64_t x, int64_t y,
                      int64_t dx, int64_t dy, void* stream);

/* util::remove_triangle - util.hpp:266-318: zero the entries of a local element-cyclic piece
 * that are globally strictly below (dir 'U') / above ('L') the diagonal.                   */
int cap_remove_triangle(double* local, int64_t ld, int64_t rows_local, int64_t cols_local, int64_t x, int64_t y,
                        int64_t d, int dir_upper, void* stream);

/* util::residual_local pieces (util.hpp:25-53) + the validators' GEMMs
 * (test/cholesky/validate.hpp:33-46): writes out[0] = sum_{upper}(R^T R - A)^2,
 * out[1] = sum_{upper} A^2 (device doubles) for single-rank (d = 1) matrices.
 * work >= n*n doubles.                                                                    */
int cap_cholesky_residual_terms(const double* A, int64_t lda, const double* R, int64_t ldr, int64_t n,
                                double* work, double* out2, void* stream);
/* sum of squares of (alpha*X + beta*Y) over an m x n window, optional identity subtraction:
 * out[0] = sum (X - (sub_identity ? I : 0))^2 ; used by qr residual / orthogonality
 * (test/qr/validate.hpp:24-31,46-51).                                                      */
int cap_sumsq(const double* X, int64_t ldx, int64_t m, int64_t n, int sub_identity, int upper_only,
              double* out1, void* stream);

/* ------------------------------------------------------------------------------------
 * Communicators (replaces the MPI_Comm handles of topo::square / topo::rect, util/topology.h:16-143)
 * RCCL over xGMI, one process per GPU.  The 128-byte unique id is produced on rank 0 by
 * cap_comm_unique_id and shipped to the other ranks by the host (torch.distributed / MPI).
 * A communicator made by cap_comm_create issues RCCL calls for every collective, also when
 * size == 1; cap_comm_create_self is the RCCL-free single-rank form.
 * ---------------------------------------------------------------------------------- */
typedef struct cap_comm cap_comm;
int cap_comm_unique_id(void* id128);
int cap_comm_create(cap_comm** comm, const void* id128, int rank, int size, void* stream);
int cap_comm_create_self(cap_comm** comm);           /* P = 1, no RCCL */
/* Host-staged communicator: the three collectives are provided by the caller (device pointers in,
 * 0 = success).  The callback must order itself behind `stream` (and only that stream) before it
 * touches the buffers.  Used by the tests to run the multi-rank schedules with several processes
 * sharing one GPU (gloo over host memory); the product uses cap_comm_create (RCCL).              */
typedef int (*cap_allgather_fn)(void* ctx, const double* send, double* recv, int64_t count_per_rank, void* stream);
typedef int (*cap_bcast_fn)(void* ctx, double* buf, int64_t count, int root, void* stream);
typedef int (*cap_allreduce_fn)(void* ctx, double* buf, int64_t count, void* stream);
int cap_comm_create_callbacks(cap_comm** comm, int rank, int size, cap_allgather_fn allgather, cap_bcast_fn bcast,
                              cap_allreduce_fn allreduce, void* ctx);
/* MPI_Comm_split (topology.h:28-39,84-126) -> ncclCommSplit: collective over `comm`; color < 0 joins no
 * group (*out = NULL).  MPI_Comm_dup (topology.h:54-59): an independent communicator over the same ranks. */
int cap_comm_split(cap_comm* comm, int color, int key, cap_comm** out);
int cap_comm_dup(cap_comm* comm, cap_comm** out);
int cap_comm_destroy(cap_comm* comm);
int cap_comm_rank(const cap_comm* comm);
int cap_comm_size(const cap_comm* comm);
int cap_comm_backend(const cap_comm* comm);          /* 0 self, 1 RCCL, 2 host-staged */
/* what RCCL itself reports for this communicator: rank count, this rank, bound device (bench.py prints it as n_ranks_seen) */
int cap_comm_query(const cap_comm* comm, int* nranks, int* rank, int* device);
/* MPI_Allreduce(IN_PLACE, SUM) summa.hpp:236 | MPI_Reduce(SUM) to root cacqr.hpp:98 | MPI_Bcast summa.hpp:185
 * | MPI_Allgather policy.h:176 | MPI_Barrier bench/cholesky/cholinv.cpp:47 (drains the stream).          */
int cap_comm_allreduce_sum(cap_comm* comm, double* buf, int64_t count, void* stream);
int cap_comm_reduce_sum(cap_comm* comm, double* buf, int64_t count, int root, void* stream);
int cap_comm_bcast(cap_comm* comm, double* buf, int64_t count, int root, void* stream);
int cap_comm_allgather(cap_comm* comm, const double* send, double* recv, int64_t count_per_rank, void* stream);
int cap_comm_barrier(cap_comm* comm, void* stream);
/* Personalised all-to-all (what upstream assembles from MPI_Allgather + util::block_to_cyclic_* / cyclic_to_local,
 * util.hpp:56-230): rank r receives the `sendcounts[r]` doubles every rank addressed to it.  counts / displacements are HOST
 * arrays of cap_comm_size int64 (in doubles); grouped ncclSend / ncclRecv, the self piece is a device copy.
 * cap_comm_exchange = MPI_Sendrecv_replace with one partner (util::transpose, util.hpp:232-247): swaps `count` doubles of
 * `buf` with rank `partner` (tmp: device scratch of `count` doubles; partner == own rank: no-op).                       */
int cap_comm_alltoallv(cap_comm* comm, const double* send, const int64_t* sendcounts, const int64_t* sdispls, double* recv,
                       const int64_t* recvcounts, const int64_t* rdispls, void* stream);
int cap_comm_exchange(cap_comm* comm, double* buf, double* tmp, int64_t count, int partner, void* stream);
/* host-staged communicators (tests): the caller's all-to-all; 0 = success.  The self piece is copied by the library. */
typedef int (*cap_alltoallv_fn)(void* ctx, const double* send, const int64_t* sendcounts, const int64_t* sdispls, double* recv,
                                const int64_t* recvcounts, const int64_t* rdispls, void* stream);
int cap_comm_set_alltoallv_callback(cap_comm* comm, cap_alltoallv_fn fn);

/* Grid bundles: topo::square (kind 0, d x d x c, topology.h:67-143) and topo::rect (kind 1, c x d x c,
 * topology.h:16-65) - the row / column / depth / slice (/ column_contig / column_alt / cube)
 * sub-communicators split off `world` exactly as upstream's constructors do, plus the grid coordinates.
 * Collective over `world` (which stays owned by the caller).  Square layouts 1-2 are rejected
 * (numerically wrong upstream).  cap_topo_coords is the pure rank -> (d, x, y, z) map.               */
typedef struct cap_topo cap_topo;
int cap_topo_coords(int kind, int rank, int size, int c, int* d, int* x, int* y, int* z);
int cap_topo_create(cap_topo** topo, int kind, cap_comm* world, int c, int layout, int num_chunks);
/* bundle over caller-built sub-communicators: comms[7] = row, column, depth, slice, column_contig,
 * column_alt, cube (NULL where the kind has none); not owned.                                        */
int cap_topo_create_from(cap_topo** topo, int kind, cap_comm* world, int c, int layout, int num_chunks,
                         cap_comm** comms, int ncomms);
int cap_topo_destroy(cap_topo* topo);
/* which: 0 world, 1 row, 2 column, 3 depth, 4 slice, 5 column_contig, 6 column_alt, 7 cube */
cap_comm* cap_topo_comm(cap_topo* topo, int which);
/* field: 0 rank, 1 size, 2 c, 3 d, 4 x, 5 y, 6 z, 7 layout, 8 num_chunks, 9 kind */
int cap_topo_get(const cap_topo* topo, int field);

/* Distributed redistribution between the reference's element-cyclic pieces and the block-cyclic layouts of the multi-GPU
 * plans (csrc/redist.hip) - how a caller holding upstream-style pieces on P ranks reaches cap_dist_* / cap_dist2d_* / cap_dmp_*
 * and gets R / R^-1 back the way construct_R / construct_Rinv return them (cholinv.hpp:30-46).
 *   cyclic side: rank = z + c x + c d y of topo::square's d x d x c grid (topology.h:75-83) holds piece (x, y): global rows
 *                y, y + d, ..., columns x, x + d, ... (ceil(n / d) each, zero padded; matrix.hpp:8-11), replicated over z;
 *   block-cyclic side: block (I, J) of nb x nb on process (I mod Pr, J mod Pc), rank = pr Pc + pc, local block (I div Pr,
 *                J div Pc), compact local array (valid rows x valid columns); Pr = 1: the block columns of cap_dist_*.
 * One all-to-all over `world` (cap_comm_alltoallv) + one gather / scatter launch per peer; the index sets are derived on both
 * sides from (n, nb, d, Pr, Pc).  cyclic_to_bc: destination t reads from layer z = t mod c (the replicas share the work);
 * bc_to_cyclic: every rank of every layer receives its piece.  Collective, asynchronous on `stream`.
 * cap_redist_get: 0 cyclic piece edge, 1 / 2 valid local rows / columns of my block-cyclic piece, 3 d, 4 c, 5 x, 6 y, 7 z,
 * 8 Pr, 9 Pc, 10 pr, 11 pc, 12 / 13 doubles sent in direction cyclic->bc / bc->cyclic, 14 / 15 doubles received.        */
typedef struct cap_redist_plan cap_redist_plan;
int cap_redist_plan_create(cap_redist_plan** plan, int64_t n, int64_t nb, cap_comm* world, int c, int Pr);
int cap_redist_plan_destroy(cap_redist_plan* plan);
int64_t cap_redist_get(const cap_redist_plan* plan, int which);
/* pure index helper (no GPU): doubles rank `from` sends to rank `to`; dir 0 = cyclic -> block-cyclic, 1 = the way back */
int64_t cap_redist_message_elems(int64_t n, int64_t nb, int P, int c, int Pr, int from, int to, int dir);
int cap_redistribute_cyclic_to_bc(cap_redist_plan* plan, const double* piece, int64_t ldp, double* bc_local, int64_t ldb, void* stream);
int cap_redistribute_bc_to_cyclic(cap_redist_plan* plan, const double* bc_local, int64_t ldb, double* piece, int64_t ldp, void* stream);

/* ------------------------------------------------------------------------------------
 * Algorithm seam (replaces src/alg/cholesky/cholinv, src/alg/qr/cacqr)
 * ---------------------------------------------------------------------------------- */

/* cholesky::cholinv<...>::info + factor - cholinv.h:16-53, cholinv.hpp:6-28.
 * A plan handle (like `info`: create once, factor many times; owns R, Rinv and workspace).
 * Knobs keep the reference's meaning:
 *   complete_inv: 1 = full R^-1; 0 = skip the root-level Rinv12 (cholinv.hpp:147);
 *                 -1 (extension) = do not build R^-1 at all: blocked right-looking Cholesky
 *                 with real DTRSM/DSYRK - the headline "fp64 Cholesky" path;
 *   split:        root partition is n >> split (cholinv.hpp:107);
 *   bc_mult_dim:  base-case size knob (cholinv.hpp:15-18) -> panel width of the GPU schedule;
 *   dir:          'U' only, as upstream (cholinv.hpp:9).
 * comm = NULL or a size-1 communicator: single-GPU plan, A is the whole n x n matrix.
 * comm of size P > 1: the multi-GPU schedule of cap_dist_* behind the same handle - A, get_R / get_Rinv and
 * the *_ptr accessors then refer to THIS RANK's block-cyclic columns (global block column J, width nb, on
 * rank J % P; cap_bc_num_local_cols columns, all n rows; option "nb" sets the width); complete_inv = 0 / 1
 * also build R^-1 there (cap_dist_get_Rinv).
 * Option "cyclic_c" = c (multi-GPU plans; c = depth of topo::square's d x d x c grid, comm size = c d d): the plan speaks the
 * REFERENCE's layout end to end - factor's A is this rank's element-cyclic piece (ceil(n/d) x ceil(n/d), matrix.hpp:8-11),
 * get_R / get_Rinv write this rank's piece of R / R^-1 (what construct_R / construct_Rinv return on every rank of every layer,
 * cholinv.hpp:30-46; zero below the GLOBAL diagonal, i.e. already util::remove_triangle'd) - through the distributed
 * redistribution of cap_redistribute_* (one all-to-all each way).  get "piece" = the piece edge.  With it the knobs mean what they
 * mean upstream ON THAT GRID: the base-case dimension starts at c d (cholinv.hpp:15-18: with complete_inv = 0 and bc_mult_dim = 0 the
 * 2 x 2 x 2 grid partitions the root and leaves its block of R^-1 empty where one process would invert the whole base case), and
 * the root partition is taken on the local dimension, (ceil(n / d) >> split) d rows (cholinv.hpp:107).                          */
typedef struct cap_cholinv_plan cap_cholinv_plan;
int cap_cholinv_plan_create(cap_cholinv_plan** plan, int64_t n, int complete_inv, int64_t split,
                            int64_t bc_mult_dim, char dir, cap_comm* comm);
int cap_cholinv_plan_destroy(cap_cholinv_plan* plan);
/* factor: A (n x n col-major, lda) is read-only (only its upper triangle is consumed,
 * cholinv.hpp:13).  Results stay resident in the plan.                                     */
int cap_cholinv_factor(cap_cholinv_plan* plan, const double* A, int64_t lda, void* stream);
/* construct_R / construct_Rinv - cholinv.hpp:30-46: copy the upper-triangular result into a
 * caller rect buffer (strictly lower part zero-filled).                                    */
int cap_cholinv_get_R(cap_cholinv_plan* plan, double* out, int64_t ld, void* stream);
int cap_cholinv_get_Rinv(cap_cholinv_plan* plan, double* out, int64_t ld, void* stream);
/* The same three calls on descriptors - cholinv::factor(const Matrix& A, info&, Topo&&) and construct_R / construct_Rinv returning a
 * matrix (cholinv.h:46-53).  The descriptor must describe exactly the piece the plan works on, else CAP_ERR_ARG: a single-GPU plan
 * takes a 1 x 1-grid descriptor of the whole matrix; a multi-rank plan takes the block-cyclic kind with Pr = 1, Pc = P, pc = my rank
 * and the plan's nb (cap_desc_create_bc), or - option "cyclic_c" - upstream's element-cyclic kind on the d x d grid.               */
int cap_cholinv_factor_desc(cap_cholinv_plan* plan, const cap_desc* A, void* stream);
int cap_cholinv_get_R_desc(cap_cholinv_plan* plan, cap_desc* R, void* stream);
int cap_cholinv_get_Rinv_desc(cap_cholinv_plan* plan, cap_desc* Rinv, void* stream);
/* device pointers to the resident factors (leading dimension returned through *ld).        */
double* cap_cholinv_R_ptr(cap_cholinv_plan* plan, int64_t* ld);
double* cap_cholinv_Rinv_ptr(cap_cholinv_plan* plan, int64_t* ld);
/* A X = B with the factor of the plan's LAST factor call (any complete_inv).  B, X: n x nrhs, column-major,
 * device memory; X == B (in place) is allowed.  Asynchronous on `stream`, no host synchronisation.
 * Multi-rank plans and the "cyclic_c" layout return CAP_ERR_UNSUPPORTED.  If the last factor reported
 * info != 0, X is filled with NaN (read the pivot with cap_cholinv_info).  A plan that was never factored: CAP_ERR_ARG.
 * The first solve after a factor call inverts R's diagonal blocks and keeps them.  nrhs <= 16: one launch per substitution
 * (forward R^T Y = B into plan scratch, backward R X = Y), workgroups claiming the blocks' diagonal steps and tile products from a
 * ticket counter, each launch followed by a recovery launch that redoes the substitution on one workgroup if a workgroup of it
 * gave up waiting (counted by cap_solve_fallbacks); option "solve_kernel" = 0 sends these to the blocked path that more
 * right-hand sides take (cap_dtrsm's substitution: MFMA GEMMs per block step).
 * PLAN SCRATCH AND THE ONE HOST SYNCHRONISATION IT CAN COST.  cap_cholinv_solve, _update, _rcond and _error_bounds keep their scratch and
 * the block inverses in the plan, allocated by the first call that needs them and sized for that call (no synchronisation).  A later call
 * that needs more - more right-hand sides, the other substitution path and its block width (nrhs > 16 or "solve_kernel" = 0 after the
 * one-launch path), cap_cholinv_error_bounds after cap_cholinv_rcond, a larger k - waits for the device (hipDeviceSynchronize: the old
 * buffer may still be in use), frees the buffer and allocates the larger one.  Buffers never shrink, so a given sequence of calls
 * synchronises at most on its first pass over a plan; a caller that cannot afford even that makes its largest call first.           */
int cap_cholinv_solve(cap_cholinv_plan* plan, const double* B, int64_t ldb, double* X, int64_t ldx,
                      int64_t nrhs, void* stream);
/* A^-1 of the plan's LAST factor call into out (n x n, column-major, device).  fill = 0: upper triangle only, the rest of out untouched;
 * fill = 1: both triangles (the lower one is a copy of the upper one).  Asynchronous on `stream`, no host synchronisation.  Same rules as
 * cap_cholinv_solve: any complete_inv; multi-rank plans and "cyclic_c" -> CAP_ERR_UNSUPPORTED; never factored -> CAP_ERR_ARG; last factor
 * info != 0 -> the n x n window (fill = 0: its upper triangle) is NaN.  complete_inv = 1: one triangular product (cap_dlauum's kernel)
 * from the resident R^-1.  complete_inv = 0 / -1: the first call after a factor call inverts a copy of R and keeps it until the next
 * factor call - n^2 more doubles of device memory (plus TRTRI's scratch), allocated on the first call (CAP_ERR_ALLOC if that fails).  */
int cap_cholinv_inverse(cap_cholinv_plan* plan, double* out, int64_t ld, int fill, void* stream);
/* log det A = 2 sum log R_ii of the last factor call, written to ONE double in device memory; asynchronous, deterministic (fixed
 * summation order: two calls give the same bits).  NaN if the last factor failed.  Same UNSUPPORTED / ARG rules.                 */
int cap_cholinv_logdet(cap_cholinv_plan* plan, double* logdet_dev, void* stream);
/* The plan's resident R of the LAST factor call becomes the factor of A + sign V V^T (cap_dcholupdate's sweep, V n x k device memory,
 * not written; sign = +1 / -1).  The next solve / inverse rebuild what they cache per factor; logdet reads the new R.  Asynchronous on
 * `stream`, no host synchronisation; scratch lives in the plan (allocated on first use).  Single-GPU plans with complete_inv = -1 only:
 * complete_inv = 0 / 1 hold a resident R^-1 that would go stale, multi-rank plans and "cyclic_c" -> CAP_ERR_UNSUPPORTED.  NULL plan,
 * never factored, sign other than +1 / -1, k < 0, NULL V or ldv < n (k > 0) -> CAP_ERR_ARG; k == 0 -> CAP_OK.  A failing downdate
 * writes its row into the plan's report: cap_cholinv_info returns it and solve / inverse / logdet give NaN, until the next factor call.
 * If that report is already nonzero when the update runs, R and the report are left alone (decided on the device).
 * Option "chud_kernel": 1 = one launch per pass of 16 columns (default), 0 = two launches per 64-row block step; identical bits.        */
int cap_cholinv_update(cap_cholinv_plan* plan, int sign, const double* V, int64_t ldv, int64_t k, void* stream);
/* cap_dpocon / cap_dpoerr on the plan's resident R of the LAST factor or update call (single-GPU plans, any complete_inv; multi-rank plans
 * and "cyclic_c" -> CAP_ERR_UNSUPPORTED; never factored -> CAP_ERR_ARG, as cap_cholinv_solve).  They share the block inverses that
 * cap_cholinv_solve keeps per factor - whichever runs first makes them - and keep their scratch in the plan (allocated on first use, sized
 * for the call: rcond alone needs about n^2 / 512 + 5 n doubles).  The plan keeps ONE set of block inverses, of the width of the one-launch
 * substitution (nrhs <= 16, option "solve_kernel" = 1, the default): a solve with more than 16 right-hand sides or with "solve_kernel" = 0
 * uses another width and replaces the set, so alternating such solves with rcond / error_bounds rebuilds it each time.
 * cap_cholinv_rcond: exactly one of A / anorm_dev is non-NULL (else CAP_ERR_ARG): the 1-norm is computed from A's upper triangle
 * (cap_dlansy, then bit for bit cap_dpocon's result), or taken as given.  cap_cholinv_error_bounds: A, B, X as for cap_dpoerr.
 * THE PLAN DOES NOT KEEP A: passing the matrix (or norm) that matches the resident factor - after cap_cholinv_update the updated
 * matrix - is the caller's business.  If the last factor or downdate reported info != 0: rcond = 0 (what LAPACK's dposvx reports for a
 * matrix that is not positive definite - `rcond < eps` stays a valid test, which NaN would not be) and ferr = berr = NaN, beside the
 * NaN of solve / inverse / logdet.  Asynchronous on `stream`, no host synchronisation.                                                 */
int cap_cholinv_rcond(cap_cholinv_plan* plan, const double* A, int64_t lda, const double* anorm_dev, double* rcond_dev, void* stream);
int cap_cholinv_error_bounds(cap_cholinv_plan* plan, const double* A, int64_t lda, const double* B, int64_t ldb, const double* X,
                             int64_t ldx, int64_t nrhs, double* ferr_dev, double* berr_dev, void* stream);
/* host-readable status of the last factor: 0, or 1-based index of the failing pivot.  A launch of the one-launch
 * diagonal-block chain (option "chain_coop") whose workgroups were never all resident gives up after ~3 s of polling, and the
 * recovery launch behind it restores that diagonal block and re-runs it on two workgroups (counted in option
 * "chain_fallbacks"); -64 is only left if that re-run could not complete either (a stream restricted to fewer than two CUs).
 * Synchronises the stream.                                                                 */
int cap_cholinv_info(cap_cholinv_plan* plan, void* stream, int64_t* info);
/* tuning knobs of the GPU schedule: "nb" (panel width), "leaf", "lookahead", "outer" (strip height = K of
 * the bulk updates), "tail" (columns left below which strips are nb wide), "depth2" (look-ahead depth 2),
 * "occ1_m" (columns left below which bulk updates run one workgroup per CU so the diagonal-block chain
 * always finds a slot; 0 = never), "inner_la" (column-split look-ahead, off), "reserve" (CU-masked chain
 * stream, off), "serial_m", "fastdiag", "profile", "use_sb" (strip buffers: the solved block rows of a strip are written
 * K-contiguously into a ring of three buffers every update reads from, R receives a copy off the panel stream; on),
 * complete_inv >= 0: "inv_fast" (blocked sweep + inverse tree instead of the plain recursion of cholinv.hpp:85-165; on),
 * "inv_overlap" (tree nodes are enqueued as their inputs become final; on), "inv_start_m" (columns left below which the
 * tree starts), "fuse_copy" (only the first strip's rows of A are copied into R, the updates of step 0 read their C input
 * from A; on, bit-identical), "reserve_m" (with "reserve": the CU masks only apply once at most reserve_m columns are left;
 * measured slower, off), "chain_coop" (PER PLAN since round 5: resident workgroups of the one-launch diagonal-block chain - the
 * whole 64-blocked factor phase of a diagonal block + the inverse levels up to 256 as one launch whose workgroups meet at a
 * counter in device memory, csrc/leaf.hip; process default 32 (CAP_CHAIN_COOP), clamped to what the device holds at once; 0 = one
 * launch per 64-column step, bit-identical; -1 = back to the process default), get only: "chain_fallbacks" (diagonal blocks of
 * this process that the recovery launch had to re-run on this device; synchronises).
 * Multi-GPU plans forward to cap_dist_set_option.                                                                         */
int cap_cholinv_set_option(cap_cholinv_plan* plan, const char* key, int64_t value);
int64_t cap_cholinv_get_option(cap_cholinv_plan* plan, const char* key);
/* Diagnostics of the one-launch diagonal-block chain (no counterpart upstream: its base case is one LAPACKE_dpotrf + dtrtri on the
 * host, policy.h:307-414).  cap_chain_fallbacks: diagonal blocks of this process that the recovery launch restored and re-ran on the
 * current device because a workgroup gave up waiting for its peers (synchronises the device).  cap_chain_inject_timeouts(count):
 * TEST HOOK - the next `count` chain launches on the current device give up at their first meeting, so the recovery path runs.   */
int64_t cap_chain_fallbacks(void);
int cap_chain_inject_timeouts(int count);
/* The same two diagnostics for the one-launch substitutions of cap_cholinv_solve / cap_dpotrs: substitutions of this process that the
 * recovery launch finished on the current device (synchronises the device); TEST HOOK - the next `count` one-launch substitutions on
 * the current device give up at their first wait.                                                                                  */
int64_t cap_solve_fallbacks(void);
int cap_solve_inject_timeouts(int count);
/* And for the one-launch passes of cap_dcholupdate / cap_cholinv_update: passes of this process that the recovery launch finished on the
 * current device (synchronises the device); TEST HOOK - the next `count` one-launch passes on the current device give up before their
 * first item (through the normal give-up path; the result is the same bits).                                                          */
int64_t cap_update_fallbacks(void);
int cap_update_inject_timeouts(int count);
/* Live measurement of the dominant kernel (trailing-update DSYRK) of the LAST factor call, enabled
 * with cap_cholinv_set_option(plan, "profile", 1): number of launches, their summed duration in ms
 * (HIP events recorded on the stream each launch went to) and summed algorithmic flops
 * (m(m+1)k per launch).  Synchronises on the recorded events.                               */
int cap_cholinv_profile(cap_cholinv_plan* plan, int64_t* launches, double* ms_total, double* flops_total);
/* the same launches of the LAST factor call one by one: up to cap entries of (ms, algorithmic flops); *count = launches */
int cap_cholinv_profile_launches(cap_cholinv_plan* plan, double* ms_out, double* flops_out, int64_t cap, int64_t* count);

/* Multi-GPU blocked Cholesky on a 1 x P block-column-cyclic matrix (the 2D block-cyclic descriptor with
 * Pr = 1): global block column J (width nb) lives on rank J % P as local block J / P; rows are not
 * distributed.  Per step: the owner factors + inverts the diagonal block, broadcasts
 * [R(k,k+1) | Dinv(k+1)], every rank solves its own part of block row k with one GEMM, the solved rows
 * are all-gathered and each rank applies the rank-nb update to its own columns (upper staircase only).
 * Replaces the MPI_Bcast / MPI_Allgather schedule of summa.hpp:163-253 + policy.h:160-305 with RCCL
 * over xGMI; one process per GPU.  Inputs/outputs are the LOCAL column blocks (n rows, ld >= n).     */
typedef struct cap_dist_plan cap_dist_plan;
/* nb: block width (multiple of 128; 0 = 512).  Any n: the plan pads to a multiple of nb with an identity tail. */
int cap_dist_plan_create(cap_dist_plan** plan, int64_t n, int64_t nb, cap_comm* comm);
int cap_dist_plan_destroy(cap_dist_plan* plan);
int64_t cap_dist_local_cols(const cap_dist_plan* plan);                 /* columns stored on this rank   */
int cap_dist_factor(cap_dist_plan* plan, const double* Alocal, int64_t lda, void* stream);
double* cap_dist_R_ptr(cap_dist_plan* plan, int64_t* ld);               /* local columns of R, ld = padded n; entries
                                                                           below the global diagonal are scratch */
int cap_dist_get_R(cap_dist_plan* plan, double* out, int64_t ld, void* stream);   /* construct_R: n x local_cols, zero below
                                                                                      the global diagonal              */
/* Options "complete_inv" = 0 / 1 (+ "split"): the factor call also leaves this rank's block columns of R^-1 - upstream's
 * R + R^-1 semantics on P > 1 (cholinv.hpp:85-165) - STREAMED with the sweep: as soon as block row k is solved, the owner of
 * block column k finishes that column of R^-1 (X[0:k+1, k] Dinv(k)), broadcasts it ((k+1) nb x nb doubles) and every rank
 * updates its own block columns J > k with its OWN piece of the solved row (X[0:k+1, J] -= X[0:k+1, k] R[k, J]) - one MFMA GEMM
 * per step on the plan's inverse stream, (n^3/3)/P flops per rank, half the bytes of an all-gather of R, no replicated R:
 * per-rank memory is the local columns of R and R^-1 plus two n x nb buffers (allocated when the option is set, so a failure is
 * reported before any collective).  "safe" = 1 runs the steps after the sweep on the one communicator.
 * complete_inv = 0 leaves Ri[0 : n >> split, n >> split : n] empty (cholinv.hpp:107,147).                              */
int cap_dist_get_Rinv(cap_dist_plan* plan, double* out, int64_t ld, void* stream);   /* construct_Rinv, same layout as get_R */
double* cap_dist_Rinv_ptr(cap_dist_plan* plan, int64_t* ld);
/* 0, or the smallest failing pivot (1-based) reported by any rank.  Collective; call it on the stream
 * cap_dist_factor ran on.                                                                              */
int cap_dist_info(cap_dist_plan* plan, void* stream, int64_t* info);
/* knobs: "strip" (block rows per bulk update, 1|2), "depth2" (split bulk updates), "occ1_m" (bulk updates of at most
 * occ1_m^2 rows x local columns run one workgroup per CU), "profile", "safe" (one communicator + one communication
 * stream), "ipc" (strip exchange as IPC peer copies; get "ipc_active" tells whether the peers could be mapped),
 * "complete_inv" / "split" (R^-1, see cap_dist_get_Rinv), "root_n1" (the root partition given explicitly instead of n >> split:
 * upstream cuts its LOCAL dimension, (ceil(n / d) >> split) d global rows on a d x d x c grid, cholinv.hpp:107 - a cholinv plan
 * with "cyclic_c" sets it, together with the grid's base-case rule cholinv.hpp:15-18; 0 = n >> split), "jitter_us" / "jitter_seed" (stress testing: random spin kernels in
 * front of every launch group); get only: "count_gemm" / "count_chain" / "count_copy" / "count_coll" = launches and
 * collectives of the last factor call on this rank.                                                                     */
int cap_dist_set_option(cap_dist_plan* plan, const char* key, int64_t value);
int64_t cap_dist_get_option(const cap_dist_plan* plan, const char* key);
int cap_dist_profile(cap_dist_plan* plan, int64_t* launches, double* ms_total, double* flops_total);
/* profile mode, per stream role: out6 = busy ms of the diagonal-block chains, block-row solves, HEAD updates (panel stream),
 * message broadcasts, strip exchanges (communication streams) and bulk updates (caller's stream) of the LAST factor call. */
int cap_dist_profile_streams(cap_dist_plan* plan, double* out6);
/* the bulk updates of the LAST factor call in profile mode, one by one: up to cap entries of (ms, algorithmic flops); *count = launches */
int cap_dist_profile_launches(cap_dist_plan* plan, double* ms_out, double* flops_out, int64_t cap, int64_t* count);
/* profile mode, complete_inv >= 0: out3 = busy ms of the streamed inverse's launch groups, ms of it left after the sweep's join
 * (what the overlap did not hide), ms of the whole factor call.                                                          */
int cap_dist_profile_inverse(cap_dist_plan* plan, double* out3);
/* Non-blocking progress of the factor call in flight (host watchdog of bench.py): out9 = leading complete events among
 * fact, msg, rowdone (per block row), solved, gather, head2, rest (per strip), then the block-row and strip counts.
 * Option "safe" = 1 runs the same schedule with ONE communicator and ONE communication stream (collectives in program order). */
int cap_dist_progress(cap_dist_plan* plan, int64_t* out9);
/* distribute_symmetric (structure.hpp:68-103) for this layout: fills the local block columns.            */
int cap_fill_symmetric_bc(double* local, int64_t ld, int64_t n, int64_t nb, int P, int p, int diagonally_dominant,
                          void* stream);
/* pure index helpers (no GPU): owner / local block / local column offset of global block column J    */
int cap_bc_owner(int64_t J, int P);
int64_t cap_bc_local_block(int64_t J, int P);
int64_t cap_bc_num_local_cols(int64_t n, int64_t nb, int P, int p);

/* The same factorization on a 2D Pr x Pc BLOCK-CYCLIC process grid (csrc/dist2d.hip): block (I, J) of nb x nb elements on
 * process (I % Pr, J % Pc) as local block (I / Pr, J / Pc), rank = pr * Pc + pc, local arrays column-major; Pr must divide
 * Pc (1 x P, 2 x 2, 2 x 4, 4 x 4).  Strips of two block rows like cap_dist_*: per block row the diagonal block on its owner,
 * [R(a,b) | Dinv] along the owner's process row, block-row solve there, the solved row down the process columns into a
 * K-contiguous strip buffer (B operand); per strip the pieces I = pr mod Pr re-broadcast along the process rows by the Pc / Pr
 * columns that hold them (A operand) and ONE K = 2 nb staircase MFMA update of the local blocks b < I <= J, look-ahead depth 2.
 * Replaces topo::square's row / column communicators + summa::distribute (topology.h:67-143, summa.hpp:163-221).
 * row / col: communicators of my process row (ordered by pc) / column (ordered by pr), or NULL to split them off `world`
 * (ncclCommSplit).  Alocal / get_R: the valid local piece (cap_bc2d_local_extent rows x columns, column-major).
 * cap_dist2d_get: 0 valid local rows, 1 valid local columns, 2 Pr, 3 Pc, 4 pr, 5 pc, 6 nb, 7 padded n, 8..11 = MFMA kernels,
 * diagonal-block chains, copy kernels, collectives issued by the last factor call on this rank; 12 = IPC moves active.    */
typedef struct cap_dist2d_plan cap_dist2d_plan;
int cap_dist2d_plan_create(cap_dist2d_plan** plan, int64_t n, int64_t nb, cap_comm* world, int Pr, cap_comm* row, cap_comm* col);
int cap_dist2d_plan_destroy(cap_dist2d_plan* plan);
int64_t cap_dist2d_get(const cap_dist2d_plan* plan, int which);
int cap_dist2d_factor(cap_dist2d_plan* plan, const double* Alocal, int64_t lda, void* stream);
double* cap_dist2d_R_ptr(cap_dist2d_plan* plan, int64_t* ld);
int cap_dist2d_get_R(cap_dist2d_plan* plan, double* out, int64_t ld, void* stream);
int cap_dist2d_info(cap_dist2d_plan* plan, void* stream, int64_t* info);
/* options: "strip" (block rows per K = strip nb update, 1 | 2; default 2 from 8 block rows on), "depth2" (bulk update split so that
 * the rows of strip t + 2 release the panel stream early; on), "occ1_m", "safe" (one communicator family, one communication stream),
 * "complete_inv" = 0 / 1 + "split": the factor call also leaves my piece of R^-1 (cap_dist2d_get_Rinv), streamed with the sweep as in
 * cap_dist_*: per block row Dinv(k) down the owner's process column, the finished block column of R^-1 along the process rows, one
 * local MFMA GEMM with my piece of the solved row - no replicated R.  "ipc" = 1: both operand moves (the solved row down the process
 * columns, the strip pieces along the process rows) as IPC peer copies on SDMA engines with two 8-byte all-reduces each as barriers,
 * like the 1 x P plan's strip exchange (cap_dist2d_get(plan, 12) tells whether the peers could be mapped).                  */
int cap_dist2d_set_option(cap_dist2d_plan* plan, const char* key, int64_t value);
/* descriptor forms: A / R / Rinv are block-cyclic descriptors (cap_desc_create_bc) of THIS plan's n, nb, Pr x Pc and position -
 * checked, CAP_ERR_ARG otherwise.  Host matrix -> pieces -> factor -> host R: cap_desc_import_host_global, cap_dist2d_factor_desc,
 * cap_dist2d_get_R_desc, cap_desc_export_host_global.                                                                            */
int cap_dist2d_factor_desc(cap_dist2d_plan* plan, const cap_desc* A, void* stream);
int cap_dist2d_get_R_desc(cap_dist2d_plan* plan, cap_desc* R, void* stream);
int cap_dist2d_get_Rinv_desc(cap_dist2d_plan* plan, cap_desc* Rinv, void* stream);
int cap_dist2d_get_Rinv(cap_dist2d_plan* plan, double* out, int64_t ld, void* stream);
double* cap_dist2d_Rinv_ptr(cap_dist2d_plan* plan, int64_t* ld);
int64_t cap_bc2d_local_extent(int64_t n, int64_t nb, int Pr, int Pc, int pr, int pc, int which);   /* which: 0 rows, 1 columns */
/* pure index helper of the update kernel's staircase enumeration: local row tiles (128 rows) of process row pr of Pr, from
 * local row block rlb0 on, whose global tile index relative to block J0 is <= X (nbT = nb / 128)                        */
int cap_bc2d_rows_le(int X, int nbT, int J0, int Pr, int pr, int rlb0);
int cap_fill_symmetric_bc2d(double* local, int64_t ld, int64_t n, int64_t nb, int Pr, int Pc, int pr, int pc,
                            int diagonally_dominant, void* stream);

/* matmult::summa::invoke, GEMM overload (summa.hpp:6-44, distribute :163-221, collect :223-253; driver
 * bench/matmult/summa_gemm.cpp:7-55): C = alpha A B + beta C on the d x d x c grid of a topo::square bundle, operands
 * are the element-cyclic local pieces (ceil(M/d) x ceil(K/d) etc., zero padded).  Layer z walks the inner process
 * indices z, z + c, ... (c == d: upstream's single step; c == 1: 2D SUMMA); row / column broadcasts run on their own
 * streams and communicators, B moves in `num_chunks` column chunks overlapped with the local MFMA GEMMs
 * (upstream's Ibcast pipelining, summa.hpp:195-215); partial products are summed over `depth` when c > 1.          */
typedef struct cap_summa_plan cap_summa_plan;
int cap_summa_plan_create(cap_summa_plan** plan, cap_topo* topo, int64_t m, int64_t n, int64_t k, int num_chunks);
int cap_summa_plan_destroy(cap_summa_plan* plan);
void cap_summa_local_dims(const cap_summa_plan* plan, int64_t* ml, int64_t* nl, int64_t* kl);
int cap_summa_dgemm(cap_summa_plan* plan, double alpha, const double* A_local, int64_t lda, const double* B_local,
                    int64_t ldb, double beta, double* C_local, int64_t ldc, void* stream);
/* util::transpose (util.hpp:232-247): MPI_Sendrecv_replace with the transpose partner (x, y, z) <-> (y, x, z) of topo::square.
 * `count` doubles of `buf` are swapped (the received piece is the partner's piece as stored, NOT transposed); tmp: device
 * scratch of `count` doubles.                                                                                            */
int cap_util_transpose(cap_topo* topo, double* buf, double* tmp, int64_t count, void* stream);
/* matmult::summa::invoke, TRMM overload (summa.hpp:46-83; call sites cholinv.hpp:114-120,148-154): in place
 * B <- alpha op(T) B (side LEFT, T m x m; plan created with (m, n, k = m)) or alpha B op(T) (RIGHT, T n x n; plan (m, n, k = n))
 * on element-cyclic pieces.  T_local = my piece of the globally upper-triangular T: rect storage (t_packed = 0, only its upper
 * triangle is referenced) or upstream's packed-upper storage (t_packed = 1: column x at x (x + 1) / 2, structure.h:39; the
 * packed image is what travels).  trans = CAP_TRANS: T_local must be the piece AFTER cap_util_transpose, exactly as upstream's
 * call site prepares it.  uplo = UPPER, diag = NONUNIT only (every upstream call site); local products run on the MFMA GEMM
 * with K ranges cut at the triangle.                                                                                     */
int cap_summa_dtrmm(cap_summa_plan* plan, int side, int uplo, int trans, int diag, double alpha, const double* T_local, int64_t ldt,
                    int t_packed, double* B_local, int64_t ldb, void* stream);
/* matmult::summa::invoke, SYRK overload (summa.hpp:85-161; call site cholinv.hpp:128-133): C <- alpha A^T A + beta C (trans =
 * CAP_TRANS, A k x n) or alpha A A^T + beta C (NoTrans, A n x k); plan created with (m = n, n = n, k).  Like upstream a GEMM of
 * A's piece with the transpose partner's piece (internal copy + cap_util_transpose, summa.hpp:91-92).  C_local: nl x nl rect
 * (c_packed = 0: the whole local square is written, as upstream does for a rect C) or packed upper (c_packed = 1).        */
int cap_summa_dsyrk(cap_summa_plan* plan, int uplo, int trans, double alpha, const double* A_local, int64_t lda, double beta,
                    double* C_local, int64_t ldc, int c_packed, void* stream);

/* qr::cacqr<...>::info + factor, 1D path - cacqr.h:18-49, cacqr.hpp:5-29,172-193,217-248.
 * A is the local row-cyclic piece (m_local x n, column-major); R (n x n) is replicated;
 * num_iter = 1 (CholeskyQR) or 2 (CholeskyQR2).  comm == NULL -> single rank.
 *
 * num_iter = 3 or 4 (not in the reference; cap_cacqr_plan_create accepts num_iter 1 ... 4, anything else is CAP_ERR_ARG): shifted CholeskyQR3
 * (Fukaya, Kannan, Nakatsukasa, Yamamoto, Yanagisawa, SIAM J. Sci. Comput. 2020) for matrices whose Gram matrix CholeskyQR2 cannot factor
 * (kappa(A) >~ 1e8).  The first num_iter - 2 sweeps are SHIFTED, the last two are CholeskyQR2 unchanged.  A shifted sweep is a sweep - same
 * Gram kernel, same all-reduce, same factorization, same Q R^-1 pass, on the caller's stream without a host synchronisation - with the Gram
 * equilibrated in between: d_j = sqrt(G_jj), G_ij <- G_ij / (d_i d_j), diagonal set to 1 + s, and R_k = R' D, R_k^-1 = D^-1 R'^-1 behind the
 * factorization; R = R_last ... R_1.  The shift is the closed form s = 11 (m n + n (n + 1)) 2^-53 n with m the GLOBAL row count (the plan sums
 * m_local over its communicator once, on its first factor call): no norm reduction, bit-reproducible, and unaffected by column scaling.
 * Supported region: one shifted sweep brings kappa down by about 1 / sqrt(s), CholeskyQR2 then needs kappa <~ 1e7 - 1e8.  The shift grows
 * with m, so the reach shrinks with the row count: measured at n = 256 (profiles/r10_scqr.txt; largest kappa of the tested decades that ended
 * with info == 0, residual < 1e-13, orthogonality < 1e-15)
 *     m = 2^13: num_iter 3 up to kappa = 1e12, num_iter 4 up to 1e15;  m = 2^16: 1e11 / 1e14;  m = 2^21: 1e11 / 1e13
 * (CholeskyQR2 alone: 1e8 at all three; the decade above each figure ended with info != 0).
 * An input beyond that region - a shift too small for it - surfaces as info != 0 from cap_cacqr_info (and NaN from cap_cacqr_solve), never
 * as a silently wrong Q: the last two sweeps are plain CholeskyQR2, whose Cholesky factorization meets a non-positive pivot.
 * A plan is driven from ONE stream: what it keeps between calls on the device (the summed row count of the shift, buffers known to be zero) is
 * ordered by that stream only; a caller that moves a plan to another stream orders the two streams itself (an event, a synchronisation).
 * cap_cacqr_factor, _Q_ptr, _R_ptr, _info, _apply_qt and _solve keep their contracts for every num_iter.                              */
typedef struct cap_cacqr_plan cap_cacqr_plan;
int cap_cacqr_plan_create(cap_cacqr_plan** plan, int64_t m_local, int64_t n, int num_iter, cap_comm* comm);
/* The 3D / tunable-grid path (cacqr.hpp:44-170: sweep_3d, sweep_tune, solve; invoke_3d :195-215) on a topo::rect
 * bundle (c x d x c; c == d is the 3D cube): A_local = ceil(M/d) x (N/c) element-cyclic piece (rows y mod d, columns
 * x mod c, replicated over the layers).  Row broadcast + Gram block + all-reduces over the process column, dense
 * Gram assembled on every rank, Cholesky factor and inverse computed redundantly per GPU, Q R^-1 as one term per
 * layer summed over `depth`.  Q_ptr is the local piece of Q, R_ptr the dense replicated R, cap_cacqr_R_piece the
 * c x c cyclic piece upstream keeps.  num_iter 1 or 2 only: a grid plan with num_iter 3 or 4 returns CAP_ERR_UNSUPPORTED (the
 * shifted sweeps are built for the 1D path).                                                                      */
int cap_cacqr_plan_create_grid(cap_cacqr_plan** plan, int64_t m_global, int64_t n_global, int num_iter, cap_topo* topo);
int64_t cap_cacqr_local_cols(const cap_cacqr_plan* plan);
int cap_cacqr_R_piece(cap_cacqr_plan* plan, double* out, int64_t ld, void* stream);
int cap_cacqr_plan_destroy(cap_cacqr_plan* plan);
int cap_cacqr_factor(cap_cacqr_plan* plan, const double* A, int64_t lda, void* stream);
double* cap_cacqr_Q_ptr(cap_cacqr_plan* plan, int64_t* ld);
double* cap_cacqr_R_ptr(cap_cacqr_plan* plan, int64_t* ld);
int cap_cacqr_info(cap_cacqr_plan* plan, void* stream, int64_t* info);
/* The shift s of the plan's last factor call into *shift_host; 0.0 for plans with num_iter <= 2 and before the first factor call.
 * Synchronises the stream.                                                                                                              */
int cap_cacqr_shift(cap_cacqr_plan* plan, double* shift_host, void* stream);
/* Least squares on the plan's LAST factor call (not in the reference, which stops at Q and R): B is the caller's local m_local x nrhs piece
 * of the right-hand sides, rows distributed like A's; Z, X: n x nrhs, replicated on every rank.  Column-major device memory, asynchronous
 * on `stream`, no host synchronisation; any nrhs >= 0, every num_iter.
 *   cap_cacqr_apply_qt  Z = Q^T B: cap_dgemm_tall_tn on the plan's Q, then the all-reduce of the n x nrhs block over the plan's
 *                       communicator (none for comm == NULL).
 *   cap_cacqr_solve     X = argmin ||A X - B||_F = R^-1 (Q^T B): the above into X, then the blocked substitution of cap_dtrsm on the
 *                       plan's final R; the inverses of R's diagonal blocks are computed by the first solve after a factor call and kept.
 * Plans of the 1D path only: a grid plan (cap_cacqr_plan_create_grid) returns CAP_ERR_UNSUPPORTED.  A plan that was never factored, or
 * a bad argument: CAP_ERR_ARG.  If the last factor reported info != 0, Z / X are filled with NaN and the call returns CAP_OK, as
 * cap_cholinv_solve does (read the pivot with cap_cacqr_info).  The first call allocates the slab buffer of the product (sized for 16
 * right-hand sides) and the solve's scratch inside the plan (CAP_ERR_ALLOC if that fails); cap_cacqr_plan_destroy frees them.          */
int cap_cacqr_apply_qt(cap_cacqr_plan* plan, const double* B, int64_t ldb, int64_t nrhs, double* Z, int64_t ldz, void* stream);
int cap_cacqr_solve(cap_cacqr_plan* plan, const double* B, int64_t ldb, int64_t nrhs, double* X, int64_t ldx, void* stream);

/* ------------------------------------------------------------------------------------
 * Mixed-precision Cholesky solve (BASELINE config 5; not in the reference, whose solve path is the
 * stub trsm/diaginvert/diaginvert.hpp:7-10): factor in low precision - every O(n^3) flop on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation and fp32 storage, the O(nb n^2) panel work in fp64 -
 * then solve A X = B to fp64 accuracy by iterative refinement (fp64 residual GEMM + blocked fp64
 * TRSMs with the promoted factor).  n must be a multiple of 128.  `A` is the same fp64 matrix in both
 * calls; solve needs it FULL symmetric.  The fp64 path (cap_cholinv_* + cap_dtrsm) is its oracle.
 * ---------------------------------------------------------------------------------- */
typedef struct cap_mpchol_plan cap_mpchol_plan;
int cap_mpchol_plan_create(cap_mpchol_plan** plan, int64_t n, int64_t nrhs_max);
int cap_mpchol_plan_destroy(cap_mpchol_plan* plan);
int cap_mpchol_factor(cap_mpchol_plan* plan, const double* A, int64_t lda, void* stream);
int cap_mpchol_info(cap_mpchol_plan* plan, void* stream, int64_t* info);
/* up to max_iter refinement sweeps until ||B - A X||_F / ||B||_F <= tol; *iters sweeps used, *relres the final value.
 * Synchronises the stream once per sweep.                                                                          */
int cap_mpchol_solve(cap_mpchol_plan* plan, const double* A, int64_t lda, const double* B, int64_t ldb, double* X,
                     int64_t ldx, int64_t nrhs, int max_iter, double tol, int* iters, double* relres, void* stream);
float* cap_mpchol_R32_ptr(cap_mpchol_plan* plan, int64_t* ld);          /* the fp32 factor (upper, n x n) */
/* Live measurement of the bf16 trailing updates (the dominant kernel, bf16_tn_kernel) of the LAST factor call, enabled with
 * cap_mpchol_set_option(plan, "profile", 1): launches, summed duration (ms, HIP events on the launch stream), summed
 * algorithmic flops (2 K per updated element) and bytes (fp32 C read + write, bf16 panel once).  Same protocol as
 * cap_cholinv_profile.  Other options: "strip" = panels (1024 rows each) contracted per bf16 update, 1 | 2 (default 2: K = 2048);
 * "split" = column-split schedule (near columns of every block-row solve / head update on the panel stream, the far ones on a
 * third stream; default 1, bit-identical to 0).                                                                           */
int cap_mpchol_set_option(cap_mpchol_plan* plan, const char* key, int64_t value);
/* The bf16 trailing update by itself (tests, tools/bf16_bench.py): C32[m x n] += alpha A^T B, A: k x m, B: k x n bf16, both
 * K-contiguous (lda / ldb in elements), fp32 atomics into C; tri = 1: square problem, elements with row <= col only.
 * variant 0 = the 128 x 128-tile kernel, 1 = the wave-specialised 256 x 128-tile kernel with the three-deep LDS ring and the tile
 * loop (m % 256 == n % 128 == k % 64 == 0, else CAP_ERR_UNSUPPORTED), -1 = the dispatcher the factorization uses (options
 * "update_kernel" 0 | 1, "update_tpw" = supertile steps per workgroup, "update_min_tiles" of cap_mpchol_set_option; process-wide).
 * tpw > 0 overrides the chunk length.                                                                                     */
int cap_bf16_update(int variant, int64_t m, int64_t n, int64_t k, float alpha, const void* A16, int64_t lda, const void* B16,
                    int64_t ldb, float* C, int64_t ldc, int tri, int tpw, void* stream);
int cap_mpchol_profile(cap_mpchol_plan* plan, int64_t* launches, double* ms_total, double* flops_total, double* bytes_total);

/* The same solve on P GPUs (BASELINE config 5: N = 131072 on 8 MI355X; csrc/dist_mixed.hip): the bf16-MFMA factorization on
 * the 1 x P block-column-cyclic layout of cap_dist_* - fp64 diagonal blocks and block-row solves, Dinv broadcast, the bf16
 * panel pieces all-gathered (a quarter of the fp64 schedule's bytes), staircase bf16 update of the local fp32 columns - and
 * fp64 iterative refinement with a distributed solve: forward / backward block substitution over the block columns (one
 * nb x nrhs broadcast / all-reduce per block) and the residual from each rank's own columns of the symmetric A.
 * n % 128 == 0; nb = block width = K of the bf16 update (power of two >= 128, 0 = 1024); Alocal = this rank's block columns
 * (n rows, cap_dmp_local_cols columns); B and X are n x nrhs and the same on every rank.                                */
typedef struct cap_dmp_plan cap_dmp_plan;
int cap_dmp_plan_create(cap_dmp_plan** plan, int64_t n, int64_t nb, int64_t nrhs_max, cap_comm* comm);
int cap_dmp_plan_destroy(cap_dmp_plan* plan);
int64_t cap_dmp_local_cols(const cap_dmp_plan* plan);
int cap_dmp_factor(cap_dmp_plan* plan, const double* Alocal, int64_t lda, void* stream);
int cap_dmp_info(cap_dmp_plan* plan, void* stream, int64_t* info);
int cap_dmp_solve(cap_dmp_plan* plan, const double* Alocal, int64_t lda, const double* B, int64_t ldb, double* X, int64_t ldx,
                  int64_t nrhs, int max_iter, double tol, int* iters, double* relres, void* stream);
float* cap_dmp_R32_ptr(cap_dmp_plan* plan, int64_t* ld);                /* my block columns of the fp32 factor, ld = padded n */

#ifdef __cplusplus
}
#endif
#endif /* CAPITAL_AMD_H_ */
