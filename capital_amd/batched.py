"""Many small SPD systems of one size on plain torch tensors: one launch factors (potrf), solves (potrs) or inverts (potri, trtri) the
whole batch.

The tensors are the memory the C ABI works on: fp64, on the device, n <= 256 (n <= 64: cap_dpotrf_batched / cap_dpotrs_batched,
csrc/potrf_batched.hip, a wavefront per block; 64 < n <= 256: cap_dpotrf_batched_blocked / cap_dpotrs_batched_blocked,
csrc/potrf_batched_blocked.hip, a workgroup per block; the inverses: cap_dtrtri_batched / cap_dpotri_batched, csrc/potri_batched.hip, one
entry each for the whole range).
Blocks of DIFFERENT sizes: VarBatch, a plan built once from host-side sizes (cap_vbatch_plan, csrc/potrf_vbatched.hip), whose potrf / potrs /
potri take one launch per size class that occurs.
update / downdate (and VarBatch.update / .downdate): the factors of A_i +- V_i V_i^T from those of A_i in place, one launch
(cap_dcholupdate_batched / cap_dcholupdate_vbatched, csrc/cholupdate_batched.hip).
trsm / trmm / mahalanobis (and the VarBatch forms): ONE half of the factor applied to B - R^-T B, R^-1 B, R^T B, R B - and the squared
Mahalanobis distances, one launch (cap_dtrsm_batched / cap_dtrmm_batched / cap_dtrsm_vbatched / cap_dtrmm_vbatched, csrc/trsm_batched.hip).
syrk / schur (and VarBatch.syrk): FORMING the blocks - alpha V^T V + beta C (+ shift I) into the triangle potrf reads, and the Schur
complement C - B A^-1 B^T from a factor, one launch per product (cap_dsyrk_batched / cap_dsyrk_vbatched, csrc/syrk_batched.hip).
symm / norm1 / rcond / error_bounds (and the VarBatch forms): how many digits of those answers mean anything - the product with the symmetric
block itself from the triangle potrf reads, its 1-norm, the EXACT reciprocal condition number and the forward / backward error bounds of
a solve, from the computed inverse (cap_dsymm_batched / cap_dlansy_batched / cap_dpocon_batched / cap_dpoerr_batched and their _vbatched
forms, csrc/symm_batched.hip).
pstrf / permute (and the VarBatch forms): the PIVOTED factorization for blocks that are semidefinite or numerically rank deficient, n <= 64 -
rank, a factor that survives zero pivots, the trace error and the pseudo-log-determinant, one launch (cap_dpstrf_batched /
cap_dpstrf_vbatched, csrc/pstrf_batched.hip) - and its permutation applied to right-hand sides.
gemm (and VarBatch.inner / VarBatch.combine): the GENERAL product with two different operands, m, n <= 256, any k - the right-hand side
X^T y of normal equations, cross terms W_1^T W_2 of two trsm results, V_i^T x and V_i z of low-rank-plus-block operators - one launch
(cap_dgemm_batched / cap_dgemm_vbatched_inner, one launch for any plan / cap_dgemm_vbatched_combine, one per size class,
csrc/gemm_batched.hip).
blocktri_potrf / blocktri_potrs: blocks LINKED to each other - many independent block-tridiagonal SPD chains (Kalman / RTS smoothers, Gauss-Markov
random fields, splines), T diagonal blocks of n <= 64 rows each, factored and solved in one launch per call with the chain walked
inside the kernel (cap_dpotrf_blocktri_batched / cap_dpotrs_blocktri_batched, csrc/blocktri_batched.hip).
blocktri_potri: the MARGINAL COVARIANCES of those chains from the factor - the diagonal blocks and the lag-one blocks of the inverse, the
smoother's other half - in one launch, without the (T n) x (T n) inverse (cap_dpotri_blocktri_batched, csrc/blocktri_potri_batched.hip).
VarChains: those three for chains of DIFFERENT lengths - a plan built once from host-side lengths (cap_blocktri_plan,
csrc/blocktri_vbatched.hip), one launch per call, every chain bit for bit what the fixed-length function gives for it alone.
There is no CPU path and no fallback: anything else raises CapitalError."""
import ctypes

import torch

from . import _lib, blas, lapack

_PACK_F = lapack.ArgPack_potrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_S = lapack.ArgPack_potrs_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_T = lapack.ArgPack_trtri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_I = lapack.ArgPack_potri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VF = lapack.ArgPack_potrf_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VS = lapack.ArgPack_potrs_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VI = lapack.ArgPack_potri_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_U = lapack.ArgPack_cholupdate_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VU = lapack.ArgPack_cholupdate_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_TS = lapack.ArgPack_trsm_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_TM = lapack.ArgPack_trmm_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VTS = lapack.ArgPack_trsm_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VTM = lapack.ArgPack_trmm_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_N = lapack.ArgPack_lansy_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper, '1')
_PACK_C = lapack.ArgPack_pocon_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_E = lapack.ArgPack_poerr_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VN = lapack.ArgPack_lansy_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper, '1')
_PACK_VC = lapack.ArgPack_pocon_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VE = lapack.ArgPack_poerr_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_P = lapack.ArgPack_pstrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_VP = lapack.ArgPack_pstrf_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_BF = lapack.ArgPack_potrf_blocktri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_BS = {h: lapack.ArgPack_potrs_blocktri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper, half=v)
            for h, v in ((None, 0), ("forward", 1), ("backward", 2))}
_PACK_BI = lapack.ArgPack_potri_blocktri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)


def _check(t, name, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.CapitalError("%s must be a device tensor - there is no CPU path" % name)
    if t.dtype != torch.float64:
        raise _lib.CapitalError("%s must be fp64, got %s" % (name, t.dtype))
    if t.dim() not in dims:
        raise _lib.CapitalError("%s must have %s dimensions, got shape %s" % (name, " or ".join(str(d) for d in dims), tuple(t.shape)))


def _blocks(A, name):
    """(batch, n, lda, stride) of a (batch, n, n) tensor whose A[i] is read as column-major memory with lda = stride(1)"""
    _check(A, name, (3,))
    batch, n, n2 = A.shape
    if n != n2:
        raise _lib.CapitalError("%s must be (batch, n, n), got shape %s" % (name, tuple(A.shape)))
    lda, stride = (A.stride(1), A.stride(0)) if n > 1 else (max(A.stride(1), 1), A.stride(0))
    if n > 1 and A.stride(2) != 1:
        raise _lib.CapitalError("%s must have stride(2) == 1, got strides %s" % (name, A.stride()))
    if lda < n or (batch > 1 and stride < lda * n):
        raise _lib.CapitalError("%s: blocks overlap (strides %s)" % (name, A.stride()))
    return batch, n, lda, max(stride, 0)


_COUNT = {"right-hand side": "nrhs", "column": "k"}     # what the docstrings call the number of columns of each kind


def _columns(R, X, name, noun, first="R"):
    """(batch, n, ldr, stride_r, X3, count, ldx, stride_x) of the factors R and of X - potrs's and trsm's B (noun "right-hand side") or
    update's V ("column"): (batch, count, n) or (batch, n), every column contiguous, no two overlapping, on R's device; first: what the
    messages call the block operand"""
    batch, n, ldr, stride_r = _blocks(R, first)
    _check(X, name, (2, 3))
    X3 = X.unsqueeze(1) if X.dim() == 2 else X
    if X3.shape[0] != batch or X3.shape[2] != n:
        raise _lib.CapitalError("%s must be (batch, %s, n) or (batch, n) with batch = %d, n = %d, got shape %s"
                                % (name, _COUNT[noun], batch, n, tuple(X.shape)))
    count = X3.shape[1]
    if n > 1 and X3.stride(2) != 1:
        raise _lib.CapitalError("every %s of %s must be contiguous, got strides %s" % (noun, name, X.stride()))
    ldx = X3.stride(1) if count > 1 else max(n, 1)
    stride_x = X3.stride(0)
    if ldx < n or (batch > 1 and stride_x < ldx * count):
        raise _lib.CapitalError("%s: %ss overlap (strides %s)" % (name, noun, X.stride()))
    if X.device != R.device:
        raise _lib.CapitalError("%s and %s live on different devices" % (first, name))
    return batch, n, ldr, stride_r, X3, count, ldx, max(stride_x, 0)


def potrf(A, logdet=False):
    """Cholesky factors of the batch, in place.  A: fp64 device tensor of shape (batch, n, n), n <= 256, with stride(2) == 1; stride(1) >= n and
    stride(0) >= n stride(1) are free.  Each A[i] is read as COLUMN-MAJOR memory with leading dimension stride(1) and its upper factor R
    (A = R^T R) replaces the upper triangle of that column-major block.  In torch's row-major reading of the same memory this means: the
    LOWER triangle of A[i] then holds L = torch.linalg.cholesky(A)[i] (L = R^T) and the upper triangle of A[i] is untouched - the input must
    be symmetric or hold its data in the lower triangle of torch's reading.
    Returns info (int32 device tensor, batch entries: 0, or the 1-based index of the first pivot that is not > 0 - that block holds NaN from
    that row of R on), or (info, logdet) with logdet=True: log det A[i] = 2 sum log r_jj as an fp64 device tensor, NaN for a failed block.
    Asynchronous on the current stream; nothing is read back."""
    batch, n, lda, stride = _blocks(A, "A")
    info, ld = lapack.engine._potrf_batched(A, n, lda, stride, batch, _PACK_F, want_logdet=bool(logdet))
    return (info, ld) if logdet else info


def potrs(R, B, info=None):
    """Solves A[i] X[i] = B[i] in place with the factors potrf left in R (same layout rules as potrf's A; what torch reads as the strictly
    upper triangle of R[i] is not referenced).  B: fp64 device tensor of shape (batch, nrhs, n) or (batch, n), every right-hand side
    contiguous (stride(-1) == 1); it is overwritten by the solutions.  info: what potrf returned, or None - a block with info != 0 gets NaN.
    Returns B.  Asynchronous on the current stream."""
    batch, n, ldr, stride_r, B3, nrhs, ldb, stride_b = _columns(R, B, "B", "right-hand side")
    lapack.engine._potrs_batched(R, B3, n, nrhs, ldr, stride_r, ldb, stride_b, batch, info, _PACK_S)
    return B


def _info(info, T):
    if info is not None and isinstance(info, torch.Tensor) and info.is_cuda and info.device != T.device:
        raise _lib.CapitalError("info lives on another device")
    return info


def trtri(T, info=None):
    """Triangular inverses of the batch, in place.  T: fp64 device tensor of shape (batch, n, n), n <= 256, under potrf's layout rules
    (stride(2) == 1, stride(1) >= n, stride(0) >= n stride(1)).  Each T[i] is read as COLUMN-MAJOR memory and the upper triangle of that
    column-major block is replaced by the upper triangle of its inverse (non-unit diagonal).  In torch's row-major reading of the same memory:
    the LOWER triangle of T[i] holds L (for instance what potrf left there) and afterwards L^-1 = torch.linalg.inv(L); what torch reads as
    the strictly upper triangle is neither read nor written.  A zero on the diagonal is not detected: it shows as infinities and NaNs inside
    its own block.  info: what potrf returned, or None - a block with info != 0 gets NaN in that triangle.
    Returns T.  Asynchronous on the current stream."""
    batch, n, ld, stride = _blocks(T, "T")
    lapack.engine._trtri_batched(T, n, ld, stride, batch, _info(info, T), _PACK_T)
    return T


def potri(R, info=None, symmetric=False):
    """Inverses of the SPD blocks from the factors potrf left in R, in place (same layout rules as potrf's A; n <= 256).  The upper triangle
    of each column-major block R[i] is replaced by that of A[i]^-1 = R^-1 R^-T.  In torch's row-major reading of the same memory: after
    potrf(A); potri(A) the LOWER triangle of A[i] holds that of torch.cholesky_inverse(L) with L = torch.linalg.cholesky(A)[i], and what
    torch reads as the strictly upper triangle is untouched.  With symmetric=True (the C ABI's fill = 1) A[i] holds the whole symmetric
    inverse: the other triangle is the bit-identical mirror, copied and never computed a second time.
    info: what potrf returned, or None - a block with info != 0 gets NaN wherever the call writes (the triangle, or the whole block with
    symmetric=True).  Returns R.  Asynchronous on the current stream."""
    batch, n, ld, stride = _blocks(R, "R")
    lapack.engine._potri_batched(R, n, ld, stride, batch, _info(info, R), _PACK_I, fill=bool(symmetric))
    return R


def _own_info(info, batch, R):
    """the info tensor of update / downdate: the caller's (checked), or a fresh zeroed one"""
    if info is None:
        return torch.zeros(max(batch, 1), dtype=torch.int32, device=R.device)[:batch]
    if (not isinstance(info, torch.Tensor) or not info.is_cuda or info.dtype != torch.int32 or info.numel() < batch
            or not info.is_contiguous()):
        raise _lib.CapitalError("info must be a contiguous int32 device tensor of batch entries")
    if info.device != R.device:
        raise _lib.CapitalError("info lives on another device")
    return info


def _cholupdate(R, V, info, sign):
    batch, n, ldr, stride_r, V3, k, ldv, stride_v = _columns(R, V, "V", "column")
    info = _own_info(info, batch, R)
    lapack.engine._cholupdate_batched(R, V3, n, k, ldr, stride_r, ldv, stride_v, batch, sign, info if batch > 0 else None, _PACK_U)
    return info


def update(R, V, info=None):
    """Rank-k update of the factors potrf left in R, in place: R[i] <- the factor of A[i] + V_i V_i^T (same layout rules as potrf's A,
    n <= 256).  V: fp64 device tensor of shape (batch, k, n) or (batch, n) with stride(-1) == 1: V[i, q] is column q of V_i, every column
    contiguous like the right-hand sides of potrs; V is not written.  Any k; more than 16 columns are further passes inside the one launch.
    In torch's row-major reading of the same memory the LOWER triangle of R[i] holds L = torch.linalg.cholesky(A)[i] and afterwards L' with
    L' L'^T = A[i] + V[i]^T V[i] (the sum of the outer products of the rows V[i, q]); what torch reads as the strictly upper triangle is
    neither read nor written.
    info: int32 device tensor of batch entries, read and written in place - a block with info != 0 (a failed potrf, an earlier failed
    downdate) is not touched - or None for a fresh zeroed one.  Returns info.  Every block gets, bit for bit, what cap_dcholupdate gives
    for it alone.  Asynchronous on the current stream; nothing is read back."""
    return _cholupdate(R, V, info, 1)


def downdate(R, V, info=None):
    """Rank-k downdate, in place: R[i] <- the factor of A[i] - V_i V_i^T; R, V, info and the layout as in update.  In torch's row-major
    reading the LOWER triangle of R[i] afterwards holds L' with L' L'^T = A[i] - V[i]^T V[i].  A block whose A[i] - V_i V_i^T is not positive
    definite gets the 1-based row at which that was found in info[i] and NaN from that row on; no other block is affected.
    Returns info.  Asynchronous on the current stream; nothing is read back."""
    return _cholupdate(R, V, info, -1)


def trsm(R, B, trans=True, info=None, sumsq=False):
    """ONE of the two substitutions of potrs, in place: B[i] <- R_i^-T B[i] (trans=True) or R_i^-1 B[i] (trans=False) with the upper
    factors potrf left in R (same layout rules as potrf's A, n <= 256; B as in potrs: (batch, nrhs, n) or (batch, n), stride(-1) == 1).
    In torch's row-major reading of the same memory the LOWER triangle of R[i] holds L = R^T = torch.linalg.cholesky(A)[i]:
    trsm(trans=True) is L^-1 b (whitening: the result has identity covariance when b ~ N(0, A_i)), trsm(trans=False) is L^-T b.
    trsm(trans=True) followed by trsm(trans=False) leaves the bits of potrs.  A zero on the diagonal is not detected.
    info: what potrf returned, or None - a block with info != 0 gets NaN.  sumsq=True: also returns q, a fresh fp64 tensor of shape
    (batch, nrhs) - (batch,) for a 2-D B - with the sums of squares of the result's columns, computed in the same launch by a fixed
    recurrence (q = fma(x_r, x_r, q) in ascending r).  Returns B, or (B, q).  Asynchronous on the current stream."""
    batch, n, ldr, stride_r, B3, nrhs, ldb, stride_b = _columns(R, B, "B", "right-hand side")
    q = torch.zeros((batch, nrhs), dtype=torch.float64, device=R.device) if sumsq else None
    lapack.engine._trsm_batched(R, B3, n, nrhs, ldr, stride_r, ldb, stride_b, batch, bool(trans), _info(info, R), _PACK_TS,
                                sumsq=q if batch * nrhs > 0 else None, ldq=nrhs)
    if not sumsq:
        return B
    return B, (q[:, 0] if B.dim() == 2 else q)


def trmm(R, B, trans=True, info=None):
    """The product with one half of the factor, in place: B[i] <- R_i^T B[i] (trans=True) or R_i B[i] (trans=False); R, B and info as in
    trsm.  In torch's row-major reading the LOWER triangle of R[i] holds L = R^T: trmm(trans=True) is L z (sampling: L z ~ N(0, A_i) for
    z ~ N(0, I)), trmm(trans=False) is L^T z.  It undoes trsm with the same trans up to rounding.  Returns B.  Asynchronous on the
    current stream."""
    batch, n, ldr, stride_r, B3, nrhs, ldb, stride_b = _columns(R, B, "B", "right-hand side")
    lapack.engine._trmm_batched(R, B3, n, nrhs, ldr, stride_r, ldb, stride_b, batch, bool(trans), _info(info, R), _PACK_TM)
    return B


def mahalanobis(R, B, info=None):
    """Squared Mahalanobis distances d^2 = b^T A_i^-1 b of the columns of B[i] from the factors potrf left in R: trsm(R, B, trans=True,
    sumsq=True).  B is left WHITENED (L^-1 b with L = R^T, what torch reads in the LOWER triangle of R[i]).  Returns q of shape
    (batch, nrhs), or (batch,) for a 2-D B; NaN for a block with info != 0.  With potrf's logdet the Gaussian log-density is
    -(d^2 + logdet + n log 2 pi) / 2.  Asynchronous on the current stream."""
    return trsm(R, B, trans=True, info=info, sumsq=True)[1]


def _span(t):
    """[first, last) byte addresses a tensor's elements lie in"""
    if t.numel() == 0:
        return 0, 0
    return t.data_ptr(), t.data_ptr() + 8 * (sum((d - 1) * abs(st) for d, st in zip(t.shape, t.stride())) + 1)


def _no_overlap(V, C):
    (a0, a1), (b0, b1) = _span(V), _span(C)
    if a0 < b1 and b0 < a1:
        raise _lib.CapitalError("V and C overlap")


def _syrk_pack(trans, alpha, beta):
    return blas.ArgPack_syrk(blas.Order.AblasColumnMajor, blas.UpLo.AblasUpper, blas.Transpose.AblasTrans if trans else blas.Transpose.AblasNoTrans,
                             alpha, beta)


def _shift(shift, batch, ref):
    """None, a number or a (batch,) fp64 device tensor -> None or the tensor"""
    if shift is None:
        return None
    if isinstance(shift, (int, float)):
        return torch.full((max(batch, 1),), float(shift), dtype=torch.float64, device=ref.device)
    _check(shift, "shift", (1,))
    if shift.shape[0] != batch or not shift.is_contiguous():
        raise _lib.CapitalError("shift must be a number or a contiguous (batch,) tensor with batch = %d, got shape %s" % (batch, tuple(shift.shape)))
    if shift.device != ref.device:
        raise _lib.CapitalError("shift lives on another device")
    return shift


def syrk(V, C=None, trans=False, alpha=1.0, beta=0.0, shift=None, symmetric=False):
    """Forms the blocks potrf factors, one launch: C[i] <- alpha V[i]^T V[i] + beta C[i] (+ shift[i] I) in torch's reading.
    trans=False: V is (batch, k, n) or (batch, n) with stride(-1) == 1, exactly update's V - C[i] is the Gram matrix of the k rows V[i, q]
    (their sum of outer products: normal equations, covariances).  trans=True: V is (batch, n, k) with stride(-1) == 1 and
    C[i] <- alpha V[i] V[i]^T + beta C[i] (linear-kernel matrices; the layout of potrs's and trsm's B).  Any k; n <= 256.  V is not written
    and must not overlap C.
    C: fp64 device tensor of shape (batch, n, n) under potrf's layout rules, or None (only with beta == 0) for a fresh zero-initialised one.
    The triangle that is written is the one potrf reads - the upper triangle of the column-major block, which is the LOWER triangle of C[i]
    in torch's row-major reading - so potrf(syrk(X)) works without a copy; what torch reads as the strictly upper triangle is neither read
    nor written, unless symmetric=True (the C ABI's fill = 1): then it becomes the bit-identical mirror.  beta == 0 does not read C (NaN there
    does not propagate).  shift: None, a number, or a (batch,) fp64 device tensor added to the diagonals (ridge terms).
    The summation order is fixed (csrc/syrk_batched.hip): every element is a function of its two rows of V alone, the same bits for any batch,
    layout or trans.  Returns C.  Asynchronous on the current stream."""
    _check(V, "V", (2, 3))
    V3 = V.unsqueeze(2 if trans else 1) if V.dim() == 2 else V
    batch = V3.shape[0]
    n, k = (V3.shape[1], V3.shape[2]) if trans else (V3.shape[2], V3.shape[1])
    inner, outer = (k, n) if trans else (n, k)               # V3 is (batch, outer, inner): `outer` contiguous runs of `inner` elements
    if inner > 1 and V3.stride(2) != 1:
        raise _lib.CapitalError("V must have stride(-1) == 1, got strides %s" % (V.stride(),))
    ldv = V3.stride(1) if outer > 1 else max(inner, 1)
    stride_v = V3.stride(0)
    if ldv < inner or (batch > 1 and stride_v < ldv * outer):
        raise _lib.CapitalError("V: columns overlap (strides %s)" % (V.stride(),))
    if C is None:
        if beta != 0:
            raise _lib.CapitalError("C=None needs beta == 0")
        C = torch.zeros((batch, n, n), dtype=torch.float64, device=V.device)
    cb, cn, ldc, stride_c = _blocks(C, "C")
    if cb != batch or cn != n:
        raise _lib.CapitalError("C must be (batch, n, n) with batch = %d, n = %d, got shape %s" % (batch, n, tuple(C.shape)))
    if C.device != V.device:
        raise _lib.CapitalError("V and C live on different devices")
    _no_overlap(V, C)
    blas.engine._syrk_batched(V3, C, n, k, ldv, max(stride_v, 0), ldc, stride_c, batch, _syrk_pack(trans, alpha, beta),
                              shift=_shift(shift, batch, V), fill=bool(symmetric))
    return C


def schur(R, B, C, info=None):
    """Schur complements (conditional covariances) from the factors potrf left in R, in place: C[i] <- C[i] - B[i] A_i^-1 B[i]^T for B of shape
    (batch, m, n) and C of shape (batch, m, m), m <= 256, n <= 256 - two launches: trsm(R, B, trans=True, info=info), then
    syrk(B, C, trans=True, alpha=-1, beta=1).  B is left WHITENED: row j of B[i] holds L^-1 b_j with L = R^T (what torch reads in the LOWER
    triangle of R[i]).  The triangle of C that is read and written is the one potrf reads (the LOWER triangle in torch's reading).  A block
    with info != 0 gets NaN in its B from trsm and through it NaN in that triangle of its C.  Returns C.  Asynchronous on the current
    stream."""
    trsm(R, B, trans=True, info=info)
    return syrk(B, C, trans=True, alpha=-1.0, beta=1.0)


def _chain_blocks(t, name, batch=None, blocks=None, n=None):
    """(batch, blocks, n, ld, step, stride) of a (batch, blocks, n, n) tensor whose t[c, i] is read as column-major memory with ld = stride(2)"""
    _check(t, name, (4,))
    b, k, r, c = t.shape
    if r != c or (batch is not None and (b, k, r) != (batch, blocks, n)):
        raise _lib.CapitalError("%s must be (batch, %s, n, n)%s, got shape %s"
                                % (name, "T" if batch is None else "T - 1", "" if batch is None else " = (%d, %d, %d, %d)" % (batch, blocks, n, n),
                                   tuple(t.shape)))
    if t.numel() == 0:
        return b, k, r, max(r, 1), max(r * r, 1), max(k * r * r, 1)
    if r > 1 and t.stride(3) != 1:
        raise _lib.CapitalError("%s must have stride(-1) == 1, got strides %s" % (name, t.stride()))
    ld = t.stride(2) if r > 1 else max(t.stride(2), 1)
    step, stride = t.stride(1), t.stride(0)
    if ld < r or (k > 1 and step < ld * r) or (b > 1 and stride < (step * k if k > 1 else ld * r)):
        raise _lib.CapitalError("%s: blocks overlap (strides %s)" % (name, t.stride()))
    return b, k, r, ld, max(step, 0), max(stride, 0)


def _chain(D, E):
    batch, T, n, ldd, step_d, stride_d = _chain_blocks(D, "D")
    if n > 64:
        raise _lib.CapitalError("block-tridiagonal Cholesky takes blocks of at most 64 rows, got n = %d" % n)
    if E is None:
        if T > 1:
            raise _lib.CapitalError("E may be None only when T == 1, got T = %d" % T)
        return batch, T, n, ldd, step_d, stride_d, n, n * n, n * n
    if T < 1:
        raise _lib.CapitalError("D must hold at least one block per chain")
    _, _, _, lde, step_e, stride_e = _chain_blocks(E, "E", batch, T - 1, n)
    if E.device != D.device:
        raise _lib.CapitalError("D and E live on different devices")
    (a0, a1), (b0, b1) = _span(D), _span(E)
    if a0 < b1 and b0 < a1:
        raise _lib.CapitalError("D and E overlap")
    return batch, T, n, ldd, step_d, stride_d, lde, step_e, stride_e


def blocktri_potrf(D, E, logdet=False):
    """Cholesky factors of a batch of block-tridiagonal SPD chains, in place, in ONE launch - the recurrence of a Kalman / RTS smoother, a
    Gauss-Markov random field or a spline system run inside the kernel instead of 3 launches per chain position.
    D: fp64 device tensor (batch, T, n, n), the diagonal blocks, n <= 64; E: (batch, T - 1, n, n), E[c, i] = A_c[block i + 1, block i] in
    torch's reading, or None when T == 1.  Both need stride(-1) == 1; stride(-2) >= n and the other strides are free as long as no two
    blocks overlap.  In torch's row-major reading the factor is L, block lower bidiagonal, with A = L L^T: L_ii replaces the LOWER triangle
    of D[c, i] (what torch reads as the strictly upper triangle is neither read nor written, exactly as in potrf) and L_(i+1, i) replaces
    E[c, i] - together they equal torch.linalg.cholesky of the assembled (T n) x (T n) matrix.
    Returns info (int32, batch entries: 0, or the 1-based row of the T n system of the first pivot that is not > 0 - from there on the
    chain holds NaN), or (info, logdet) with logdet=True: log det A_c, NaN for a failed chain.
    A chain's bits are those of the host-driven loop potrf(D[:, i]); trsm(D[:, i], E[:, i], info=.); syrk(E[:, i], D[:, i + 1], trans=True,
    alpha=-1, beta=1) and depend on (n, T, its data) alone.  Asynchronous on the current stream; nothing is read back."""
    batch, T, n, ldd, step_d, stride_d, lde, step_e, stride_e = _chain(D, E)
    info, ld = lapack.engine._potrf_blocktri_batched(D, E, n, T, ldd, step_d, stride_d, lde, step_e, stride_e, batch, _PACK_BF,
                                                     want_logdet=bool(logdet))
    return (info, ld) if logdet else info


def blocktri_potrs(D, E, B, info=None, half=None):
    """Solves A_c x = b in place with the factors blocktri_potrf left in D and E (same layout rules), in ONE launch.  B: fp64 device tensor
    (batch, nrhs, T n) or (batch, T n), every right-hand side contiguous (stride(-1) == 1), with potrs's rules; it is overwritten.
    half: None - both sweeps (the solution); "forward" - L^-1 b alone (whitening, the terms of a state-space log-likelihood); "backward" -
    L^-T z alone (a sample of the Gauss-Markov field with precision A from z ~ N(0, I)), L the block lower bidiagonal factor of torch's
    reading: L_ii in the lower triangle of D[c, i], L_(i+1, i) in E[c, i], L = torch.linalg.cholesky of the assembled matrix.  "forward"
    followed by "backward" leaves the bits of the full solve.  info: what blocktri_potrf returned, or None - a chain with info != 0 gets NaN.
    Returns B.  Asynchronous on the current stream."""
    if half not in _PACK_BS:
        raise _lib.CapitalError("half must be None, 'forward' or 'backward', got %r" % (half,))
    batch, T, n, ldd, step_d, stride_d, lde, step_e, stride_e = _chain(D, E)
    _check(B, "B", (2, 3))
    B3 = B.unsqueeze(1) if B.dim() == 2 else B
    if B3.shape[0] != batch or B3.shape[2] != T * n:
        raise _lib.CapitalError("B must be (batch, nrhs, T n) or (batch, T n) with batch = %d, T n = %d, got shape %s" % (batch, T * n, tuple(B.shape)))
    nrhs = B3.shape[1]
    if T * n > 1 and B3.stride(2) != 1:
        raise _lib.CapitalError("every right-hand side of B must be contiguous, got strides %s" % (B.stride(),))
    ldb = B3.stride(1) if nrhs > 1 else max(T * n, 1)
    stride_b = B3.stride(0)
    if ldb < T * n or (batch > 1 and stride_b < ldb * nrhs):
        raise _lib.CapitalError("B: right-hand sides overlap (strides %s)" % (B.stride(),))
    if B.device != D.device:
        raise _lib.CapitalError("D and B live on different devices")
    for t, name in ((D, "D"), (E, "E")):
        if t is not None:
            (a0, a1), (b0, b1) = _span(t), _span(B)
            if a0 < b1 and b0 < a1:
                raise _lib.CapitalError("%s and B overlap" % name)
    lapack.engine._potrs_blocktri_batched(D, E, B3, n, T, nrhs, ldd, step_d, stride_d, lde, step_e, stride_e, ldb, max(stride_b, 0), batch,
                                          _info(info, D), _PACK_BS[half])
    return B


def blocktri_potri(D, E, info=None, symmetric=False):
    """The marginal covariances of a batch of block-tridiagonal SPD chains from the factors blocktri_potrf left in D and E (same layout
    rules), in place, in ONE launch: the diagonal blocks and the lag-one blocks of Sigma = A_c^-1 - what a Kalman / RTS smoother or a
    Gauss-Markov field fit needs beside the mean - by a backward recurrence on the factor, without the (T n) x (T n) inverse.
    In torch's row-major reading afterwards: the LOWER triangle of D[c, i] holds Sigma[block i, block i] and E[c, i] holds
    Sigma[block i + 1, block i] (the convention by which E[c, i] = A[block i + 1, block i] on input) - together the block-tridiagonal part
    of torch.linalg.inv of the assembled matrix.  What torch reads as the strictly upper triangle of D[c, i] is neither read nor written,
    unless symmetric=True (the C ABI's fill = 1): then it becomes the bit-identical mirror, copied and never computed a second time.
    The factor is overwritten: clone D and E first if blocktri_potrs is still to be called.  A zero on a diagonal is not detected.
    info: what blocktri_potrf returned, or None - a chain with info != 0 gets NaN wherever the call writes, no other chain is touched.
    A chain's bits are those of the host-driven loop, i descending: trsm(D[:, i], E[:, i], trans=False, info=.); potri(D[:, i],
    symmetric=True); gemm with alpha=-1, beta=0 of the mirrored Sigma_(i+1,i+1) and that E[:, i]; gemm with alpha=-1, beta=1 into D[:, i], of
    which the lower triangle counts - and depend on (n, T, its data) alone.  Returns (D, E).  Asynchronous on the current stream."""
    batch, T, n, ldd, step_d, stride_d, lde, step_e, stride_e = _chain(D, E)
    lapack.engine._potri_blocktri_batched(D, E, n, T, ldd, step_d, stride_d, lde, step_e, stride_e, batch, _info(info, D), _PACK_BI,
                                          fill=bool(symmetric))
    return D, E


def _gemm_pack(transa, transb, alpha, beta):
    T = blas.Transpose
    return blas.ArgPack_gemm(blas.Order.AblasColumnMajor, T.AblasTrans if transa else T.AblasNoTrans, T.AblasTrans if transb else T.AblasNoTrans,
                             alpha, beta)


def _matrices(t, name):
    """(batch, rows, cols, ld, stride) of a (batch, rows, cols) tensor whose t[i] is row-major with a free stride(1) >= cols"""
    _check(t, name, (3,))
    batch, rows, cols = t.shape
    if t.numel() == 0:                                   # nothing to address: the strides of an empty tensor say nothing
        return batch, rows, cols, max(cols, 1), max(cols, 1) * rows
    if cols > 1 and t.stride(2) != 1:
        raise _lib.CapitalError("%s must have stride(-1) == 1, got strides %s" % (name, t.stride()))
    ld = t.stride(1) if rows > 1 else max(cols, 1)
    stride = t.stride(0)
    if ld < cols or (batch > 1 and stride < ld * rows):
        raise _lib.CapitalError("%s: blocks overlap (strides %s)" % (name, t.stride()))
    return batch, rows, cols, ld, max(stride, 0)


def _out_overlap(out, operands, alpha=1.0):
    for t, name in operands:
        (a0, a1), (b0, b1) = _span(t), _span(out)
        if alpha != 0 and a0 < b1 and b0 < a1:
            raise _lib.CapitalError("%s and the output overlap" % name)


def gemm(A, B, C=None, transa=False, transb=False, alpha=1.0, beta=0.0):
    """The general product of every pair of blocks, one launch, with torch.baddbmm's semantics:
    C[i] <- alpha op(A[i]) @ op(B[i]) + beta C[i], op(M) = M or (transa / transb) M^T - right-hand sides X^T y of normal equations, cross
    terms W_1^T W_2, V^T x and V z.  A, B, C: fp64 device tensors (batch, ., .) with stride(-1) == 1, a free stride(1) >= the last
    dimension and non-overlapping blocks; op(A[i]) is m x k, op(B[i]) k x n, C is (batch, m, n) with m, n <= 256, any k.  C=None needs
    beta == 0 and returns a fresh tensor.  beta == 0 does not read C (NaN there does not propagate).  A and B are not written; C must not
    overlap A or B.  A row-major product is the column-major product with the operands swapped: that is what is handed to
    cap_dgemm_batched, nothing is copied.  The summation order is fixed (csrc/gemm_batched.hip): every element is a function of its row of
    op(A) and its column of op(B) alone, the same bits for any batch, layout or transposes.  Returns C.  Asynchronous on the current
    stream."""
    ba, ar, ac, lda, stride_a = _matrices(A, "A")
    bb, br, bc, ldb, stride_b = _matrices(B, "B")
    m, k = (ac, ar) if transa else (ar, ac)
    kb, n = (bc, br) if transb else (br, bc)
    if bb != ba or kb != k:
        raise _lib.CapitalError("op(A) is (batch, m, k) and op(B) must be (batch, k, n) with batch = %d, k = %d, got shapes %s and %s"
                                % (ba, k, tuple(A.shape), tuple(B.shape)))
    if m > 256 or n > 256:
        raise _lib.CapitalError("gemm takes outputs of at most 256 rows and columns, got m = %d, n = %d" % (m, n))
    if B.device != A.device:
        raise _lib.CapitalError("A and B live on different devices")
    if C is None:
        if beta != 0:
            raise _lib.CapitalError("C=None needs beta == 0")
        C = torch.zeros((ba, m, n), dtype=torch.float64, device=A.device)
    cb, cm, cn, ldc, stride_c = _matrices(C, "C")
    if (cb, cm, cn) != (ba, m, n):
        raise _lib.CapitalError("C must be (batch, m, n) = (%d, %d, %d), got shape %s" % (ba, m, n, tuple(C.shape)))
    if C.device != A.device:
        raise _lib.CapitalError("A and C live on different devices")
    _out_overlap(C, ((A, "A"), (B, "B")))
    # row-major C = op(A) op(B)  <=>  column-major C^T = op(B)^T op(A)^T: the memory of B[i] is the first operand, with B's own flag
    blas.engine._gemm_batched(B, A, C, n, m, k, ldb, stride_b, lda, stride_a, ldc, stride_c, ba, _gemm_pack(transb, transa, alpha, beta))
    return C


def _symm_pack(alpha, beta, absolute):
    return blas.ArgPack_symm(blas.Order.AblasColumnMajor, blas.UpLo.AblasUpper, alpha, beta, absolute)


def _same_columns(ref, got, name):
    """the (batch, n, X3, nrhs, ldx, stride_x) part of _columns for a second operand, which must match the first in shape"""
    if got[0] != ref[0] or got[1] != ref[1] or got[5] != ref[5]:
        raise _lib.CapitalError("%s must have the shape of X" % name)
    return got[4], got[6], got[7]


def _vector(t, batch, name, ref):
    """a contiguous (batch,) fp64 device tensor on ref's device"""
    _check(t, name, (1,))
    if t.shape[0] != batch or not t.is_contiguous():
        raise _lib.CapitalError("%s must be a contiguous (batch,) tensor with batch = %d, got shape %s" % (name, batch, tuple(t.shape)))
    if t.device != ref.device:
        raise _lib.CapitalError("%s lives on another device" % name)
    return t


def symm(A, X, B=None, alpha=1.0, beta=0.0, absolute=False, out=None):
    """The product with the symmetric blocks themselves, one launch: out[i] <- beta B[i] + alpha A_i X[i] (per right-hand side: a block-diagonal
    matvec, residuals b - A x with alpha=-1, beta=1).  A: fp64 device tensor of shape (batch, n, n), n <= 256, under potrf's layout rules;
    only the triangle potrf reads is read - the upper triangle of the column-major block, which is the LOWER triangle of A[i] in torch's
    row-major reading - and the other one is never touched, so A may be what syrk or potri wrote.  It is the matrix itself, not its factor.
    X, B, out: (batch, nrhs, n) or (batch, n) with stride(-1) == 1, as potrs's B.  B=None needs beta == 0; beta == 0 does not read B (NaN
    there does not propagate).  out=None: a fresh tensor of X's shape; out may be B (in place), it must not overlap A or X.
    absolute=True takes |.| of every element of A, X and B on load (|A||x| + |b|).  The summation order is fixed
    (csrc/symm_batched.hip): the same bits for any batch, layout or set of columns that travel together.  Returns out.  Asynchronous on
    the current stream."""
    cx = _columns(A, X, "X", "right-hand side", first="A")
    batch, n, lda, stride_a, X3, nrhs, ldx, stride_x = cx
    if B is None:
        if beta != 0:
            raise _lib.CapitalError("B=None needs beta == 0")
        B3, ldb, stride_b = None, max(n, 1), 0
    else:
        B3, ldb, stride_b = _same_columns(cx, _columns(A, B, "B", "right-hand side", first="A"), "B")
    if out is None:
        out = torch.zeros_like(X, memory_format=torch.contiguous_format)
    Y3, ldy, stride_y = _same_columns(cx, _columns(A, out, "out", "right-hand side", first="A"), "out")
    if out.dim() != X.dim():
        raise _lib.CapitalError("out must have the shape of X")
    for t, name in ((A, "A"), (X, "X")):
        (a0, a1), (b0, b1) = _span(t), _span(out)
        if alpha != 0 and a0 < b1 and b0 < a1:
            raise _lib.CapitalError("%s and out overlap" % name)
    blas.engine._symm_batched(A, X3, B3, Y3, n, nrhs, lda, stride_a, ldx, stride_x, ldb, stride_b, ldy, stride_y, batch,
                              _symm_pack(alpha, beta, absolute))
    return out


def norm1(A):
    """The 1-norms |A_i|_1 = max_j sum_i |a_ij| of the symmetric blocks (equal to their infinity norms), one launch.  A as in symm: only
    the triangle potrf reads is read (the LOWER triangle of A[i] in torch's reading) - and it must hold the matrix BEFORE potrf overwrote
    it: take the norms first, or keep a copy.  Returns a fresh fp64 tensor of shape (batch,); a NaN in a block's triangle gives NaN.
    Asynchronous on the current stream."""
    batch, n, lda, stride = _blocks(A, "A")
    out = torch.zeros(max(batch, 1), dtype=torch.float64, device=A.device)
    lapack.engine._lansy_batched(A, n, lda, stride, batch, out, _PACK_N)
    return out[:batch]


def rcond(R, anorm, info=None):
    """EXACT reciprocal condition numbers 1 / (|A_i|_1 |A_i^-1|_1) from the factors potrf left in R (same layout rules as potrf's A,
    n <= 256; R is not written): the inverse of every block is computed into a work tensor (potri on a copy of the triangle potrf wrote,
    the LOWER one in torch's reading) and its 1-norm taken - four launches, whatever the batch; not LAPACK's estimate, which for blocks
    this small costs more and answers less.  anorm: what norm1 returned for the matrices before potrf, a (batch,) fp64 device tensor.
    info: what potrf returned, or None - a block with info != 0 gets NaN.  anorm == 0 gives 0, NaN gives NaN; for n == 0 the result is 0.
    Returns a fresh fp64 tensor of shape (batch,).  Asynchronous on the current stream; nothing is read back."""
    batch, n, ldr, stride_r = _blocks(R, "R")
    anorm = _vector(anorm, batch, "anorm", R)
    out = torch.zeros(max(batch, 1), dtype=torch.float64, device=R.device)
    lapack.engine._pocon_batched(R, n, ldr, stride_r, batch, anorm if batch > 0 else None, _info(info, R), out, _PACK_C)
    return out[:batch]


def error_bounds(A, R, B, X, info=None, ferr=True):
    """Error bounds of the solutions X of A_i x = b that potrs computed, as LAPACK's dporfs reports them: returns (ferr, berr), fresh fp64
    tensors of shape (batch, nrhs) - (batch,) for 2-D right-hand sides.  berr: the componentwise backward error max_r |b - A x|_r /
    (|A||x| + |b|)_r.  ferr: a bound on |x - x_true|_inf / |x|_inf, | |A^-1| (|r| + (n + 1) eps (|A||x| + |b|)) |_inf / |x|_inf with the
    COMPUTED inverse (potri on a copy of R) in place of an estimate of that norm.  A: the matrices BEFORE potrf overwrote them (keep a
    copy), R: the factors; of both only the triangle potrf reads is read (the LOWER one in torch's reading).  B, X: (batch, nrhs, n) or
    (batch, n) with stride(-1) == 1, the right-hand sides and the solutions.  Nothing but the results is written.  info: what potrf
    returned, or None - a block with info != 0 gets NaN.  ferr=False skips the inverse (one launch instead of four) and returns
    (None, berr).  Asynchronous on the current stream; nothing is read back."""
    cx = _columns(R, X, "X", "right-hand side")
    batch, n, ldr, stride_r, X3, nrhs, ldx, stride_x = cx
    B3, ldb, stride_b = _same_columns(cx, _columns(R, B, "B", "right-hand side"), "B")
    ab, an, lda, stride_a = _blocks(A, "A")
    if ab != batch or an != n or A.device != R.device:
        raise _lib.CapitalError("A must be (batch, n, n) like R and live on its device, got shape %s" % (tuple(A.shape),))
    lde = max(nrhs, 1)
    fe = torch.zeros((max(batch, 1), lde), dtype=torch.float64, device=R.device) if ferr else None
    be = torch.zeros((max(batch, 1), lde), dtype=torch.float64, device=R.device)
    lapack.engine._poerr_batched(A, R, B3, X3, n, nrhs, lda, stride_a, ldr, stride_r, ldb, stride_b, ldx, stride_x, batch, _info(info, R),
                                 fe, be, lde, _PACK_E)
    shape = lambda t: None if t is None else (t[:batch, 0] if X.dim() == 2 else t[:batch, :nrhs])
    return shape(fe), shape(be)


def _pstrf_args(max_rank, nmax, tol):
    """(max_rank, tol) of a pivoted call, checked; nmax: the largest block"""
    if nmax > lapack.BATCHED_SMALL_MAX:
        raise _lib.CapitalError("pstrf handles blocks of up to %d rows, got %d - use cholinv.factor_pivoted on each block"
                                % (lapack.BATCHED_SMALL_MAX, nmax))
    mr = nmax if max_rank is None else int(max_rank)
    if mr < 0 or (max_rank is not None and mr > nmax):
        raise _lib.CapitalError("max_rank must lie in 0 .. %d, got %s" % (nmax, max_rank))
    tol = float(tol)
    if tol != tol:
        raise _lib.CapitalError("tol is NaN")
    return mr, tol


def pstrf(A, max_rank=None, tol=-1.0, logdet=False):
    """PIVOTED Cholesky factors of a batch of symmetric positive SEMIdefinite blocks, one launch: for blocks that are rank deficient, where
    potrf gives info != 0 and NaN.  A: fp64 device tensor of shape (batch, n, n), n <= 64, under potrf's layout rules; only the triangle
    potrf reads is read (the LOWER triangle of A[i] in torch's reading) and A is not written.  At most max_rank steps per block (None: n);
    a block stops earlier at the first pivot <= tol (tol < 0: n 2^-53 max_i a_ii of that block, LAPACK's default; otherwise absolute).
    Returns (L, piv, rank, resid, info), plus logdet with logdet=True:
      L: a fresh (batch, n, max_rank) tensor whose torch reading is the dense lower-trapezoidal factor - L[i] @ L[i].T ~ A[i][piv[i]][:, piv[i]]
        with explicit zeros above the diagonal and in the columns >= rank[i].  With max_rank = n it is a valid R argument of trmm / trsm /
        potrs / potri / syrk(trans=True) (a block of rank < n has zeros on its diagonal: trmm and syrk are fine, the solves are not);
      piv: int64 (batch, n), the chosen pivots in order, then the unselected indices ascending - usable as a torch.gather index (permute);
      rank: int32 (batch,), the steps done; resid: fp64 (batch,), trace(A[i] - L L^T) of the permuted block, the sum of the remaining diagonal;
      info: int32 (batch,) with the meaning of cap_dpstrf - 0: stopped at a pivot <= tol (or after n steps), 1: max_rank steps done with
        the remainder above tol, 2: a NaN on the remaining diagonal (rank = the steps done, those columns of L are intact).  It is NOT the
        info that trsm, trmm or potrs expect: pass (info == 2).int() there if a guard is wanted;
      logdet: fp64 (batch,), 2 sum_{j < rank} log l_jj - the pseudo-log-determinant a degenerate Gaussian needs; NaN for info 2.
    A block's bits depend on (n, max_rank, tol, its data) alone.  n > 64 raises CapitalError: use cholinv.factor_pivoted per block.
    Asynchronous on the current stream; nothing is read back."""
    batch, n, lda, stride = _blocks(A, "A")
    mr, tol = _pstrf_args(max_rank, n, tol)
    L = torch.zeros((batch, n, mr), dtype=torch.float64, device=A.device)
    piv = torch.zeros((batch, n), dtype=torch.int64, device=A.device)
    rank, resid, info, ld = lapack.engine._pstrf_batched(A, L if L.numel() else None, piv, n, mr, lda, stride, max(mr, 1), n * mr, batch, tol,
                                                         _PACK_P, want_logdet=bool(logdet))
    return (L, piv, rank, resid, info, ld) if logdet else (L, piv, rank, resid, info)


def permute(B, piv, inverse=False):
    """The pivoting of pstrf applied to right-hand sides (torch only: a gather / scatter along the last dimension).  B: (batch, nrhs, n) or
    (batch, n); piv: what pstrf returned.  inverse=False: out[i, ..., k] = B[i, ..., piv[i, k]] - b in the pivoted order; inverse=True:
    out[i, ..., piv[i, k]] = B[i, ..., k] - back to the natural order.  So, for full-rank blocks,
    permute(potrs(L, permute(B, piv)), piv, inverse=True) solves A x = b, and permute(trmm(L, z), piv, inverse=True) samples N(0, A_i) for
    semidefinite ones.  Returns a fresh tensor."""
    if not isinstance(B, torch.Tensor) or not isinstance(piv, torch.Tensor) or B.dim() not in (2, 3) or piv.dim() != 2:
        raise _lib.CapitalError("B must be (batch, nrhs, n) or (batch, n) and piv (batch, n)")
    if piv.dtype != torch.int64 or piv.device != B.device or piv.shape[0] != B.shape[0] or piv.shape[1] != B.shape[-1]:
        raise _lib.CapitalError("piv must be an int64 (batch, n) tensor on B's device with B's batch and n, got shape %s for B of shape %s"
                                % (tuple(piv.shape), tuple(B.shape)))
    idx = piv if B.dim() == 2 else piv.unsqueeze(1).expand(B.shape)
    if inverse:
        return torch.empty_like(B, memory_format=torch.contiguous_format).scatter_(-1, idx, B)
    return torch.gather(B, -1, idx)


class VarBatch:
    """A batch of SPD blocks of DIFFERENT sizes 0 <= n_i <= 256 inside ONE flat fp64 device tensor: block i is the n_i x n_i column-major block
    at element offsets[i] with leading dimension ld[i].  sizes, ld, offsets: host sequences of ints; ld=None: ld[i] = max(n_i, 1);
    offsets=None: the blocks lie back to back in batch order.  The plan (cap_vbatch_plan) sorts the blocks once into the size classes of the
    fixed-size kernels and lives on the device that is current when it is made; building and freeing it may synchronise, no other method
    does.  It is reusable for any number of calls, from several streams at once.  Every block gets, bit for bit, what the fixed-size
    functions of this module give for it alone - whichever blocks travel with it.
    inner / combine work on the STACKED operands alone (no flat tensor): per-block products X_i^T Y_i of two stacked operands (one launch
    for any plan, empty blocks give beta out[i]) and per-block combinations V_i Z_i back into a stacked result.
    .offsets / .row_offsets: tuples in batch order (row_offsets: the prefix sum of the sizes - the rows of the stacked right-hand sides);
    .total: elements the blocks span (the least length of A); .rows: sum of the sizes; .launches: launches per call.
    Overlapping blocks, negative sizes, ld[i] < n_i or a size above 256 raise CapitalError."""

    def __init__(self, sizes, ld=None, offsets=None):
        self.sizes = tuple(int(x) for x in sizes)
        batch = len(self.sizes)
        for name, seq in (("ld", ld), ("offsets", offsets)):
            if seq is not None and len(seq) != batch:
                raise _lib.CapitalError("%s must have one entry per block (%d), got %d" % (name, batch, len(seq)))
        arr = lambda seq: (ctypes.c_int64 * max(batch, 1))(*[int(x) for x in seq]) if seq is not None else None
        L = _lib.lib()
        self._L, self._plan = L, ctypes.c_void_p()
        _lib.check(L.cap_vbatch_plan_create(batch, arr(self.sizes), arr(ld), arr(offsets), ctypes.byref(self._plan)), "VarBatch")
        self.batch = batch
        self.ld = tuple(int(x) for x in ld) if ld is not None else tuple(max(n, 1) for n in self.sizes)
        if offsets is not None:
            self.offsets = tuple(int(x) for x in offsets)
        else:
            self.offsets, at = [], 0
            for n, l in zip(self.sizes, self.ld):
                self.offsets.append(at)
                at += l * n
            self.offsets = tuple(self.offsets)
        rows, at = [], 0
        for n in self.sizes:
            rows.append(at)
            at += n
        self.row_offsets = tuple(rows)
        self.total = int(L.cap_vbatch_plan_info(self._plan, 1))
        self.rows = int(L.cap_vbatch_plan_info(self._plan, 2))
        self.launches = int(L.cap_vbatch_plan_info(self._plan, 4))
        self.device = torch.cuda.current_device() if torch.cuda.is_available() else None

    def __del__(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            self._L.cap_vbatch_plan_destroy(plan)

    def _flat(self, A, name):
        _check(A, name, (1,))
        if A.numel() < self.total or (A.numel() > 1 and A.stride(0) != 1):
            raise _lib.CapitalError("%s must be a contiguous 1-D tensor of at least %d elements, got shape %s, strides %s"
                                    % (name, self.total, tuple(A.shape), A.stride()))
        if A.device.index != self.device:
            raise _lib.CapitalError("%s lives on device %s, the plan on device %s" % (name, A.device.index, self.device))
        return A

    def potrf(self, A, logdet=False):
        """Cholesky factors of all blocks, in place.  A: 1-D fp64 device tensor of at least .total elements.  The upper triangle of every
        column-major block <- R_i (A_i = R_i^T R_i); in torch's row-major reading of the same memory (.block) the LOWER triangle then holds
        L = torch.linalg.cholesky(A_i).  Strictly lower triangles, padding rows and gaps are neither read nor written.
        Returns info (int32, batch order: 0, or the 1-based first pivot that is not > 0 - that block holds NaN from that row of R on; 0
        for an empty block), or (info, logdet) with logdet=True.  Asynchronous on the current stream."""
        info, ld = lapack.engine._potrf_vbatched(self._plan, self._flat(A, "A"), self.batch, _PACK_VF, want_logdet=bool(logdet))
        return (info, ld) if logdet else info

    def potrs(self, R, B, info=None):
        """Solves A_i x = b_i for all blocks in place with the factors potrf left in R.  B: fp64 device tensor of shape (rows,) or (nrhs, rows)
        with stride(-1) == 1 - every right-hand side is the stacked vector, block i owning entries row_offsets[i] .. row_offsets[i] + n_i: the
        call applies the inverse of the block-diagonal matrix.  info: what potrf returned, or None - a block with info != 0 gets NaN.
        Returns B.  Asynchronous on the current stream."""
        B2, nrhs, ldb = self._stacked(R, B, "B", "right-hand side")
        lapack.engine._potrs_vbatched(self._plan, R, B2, nrhs, ldb, self.batch, _info(info, R), _PACK_VS)
        return B

    def potri(self, R, info=None, symmetric=False):
        """Inverses of the SPD blocks from the factors potrf left in R, in place: the upper triangle of every column-major block <- that of
        A_i^-1; in torch's row-major reading (.block) the LOWER triangle holds that of torch.cholesky_inverse(L).  symmetric=True: the
        other triangle becomes the bit-identical mirror.  info: what potrf returned, or None - a block with info != 0 gets NaN wherever the
        call writes.  Returns R.  Asynchronous on the current stream."""
        lapack.engine._potri_vbatched(self._plan, self._flat(R, "R"), self.batch, _info(info, R), _PACK_VI, fill=bool(symmetric))
        return R

    def _cholupdate(self, R, V, info, sign):
        V2, k, ldv = self._stacked(R, V, "V", "column")
        info = _own_info(info, self.batch, R)
        lapack.engine._cholupdate_vbatched(self._plan, R, V2, k, ldv, self.batch, sign, info if self.batch > 0 else None, _PACK_VU)
        return info

    def update(self, R, V, info=None):
        """Rank-k update of the factors potrf left in R, in place: block i <- the factor of A_i + V_i V_i^T.  V: fp64 device tensor of shape
        (rows,) or (k, rows) with stride(-1) == 1 - every column of the stacked V, block i owning entries row_offsets[i] .. row_offsets[i] + n_i
        of it; V is not written.  In torch's row-major reading (.block) the LOWER triangle holds L and afterwards L' with L' L'^T = A_i + V_i V_i^T.
        info: int32 device tensor of batch entries in batch order, read and written in place - a block with info != 0 is not touched, the
        entries of empty blocks are neither read nor written - or None for a fresh zeroed one.  Returns info.  Every block gets the bits of
        the fixed-size update on it alone.  Asynchronous on the current stream."""
        return self._cholupdate(R, V, info, 1)

    def downdate(self, R, V, info=None):
        """Rank-k downdate, in place: block i <- the factor of A_i - V_i V_i^T; arguments as in update.  In torch's row-major reading (.block)
        the LOWER triangle afterwards holds L' with L' L'^T = A_i - V_i V_i^T.  A block whose matrix is not positive definite gets the 1-based
        row at which that was found in info[i] and NaN from that row on.  Returns info.  Asynchronous on the current stream."""
        return self._cholupdate(R, V, info, -1)

    def _stacked(self, R, X, name, noun, first="R"):
        """(X2, count, ldx) of the flat factors R and of the stacked X - potrs's and trsm's B (noun "right-hand side") or update's V
        ("column"): (rows,) or (count, rows), every column contiguous, no two overlapping, on R's device"""
        self._flat(R, first)
        _check(X, name, (1, 2))
        X2 = X.unsqueeze(0) if X.dim() == 1 else X
        if X2.shape[1] != self.rows:
            raise _lib.CapitalError("%s must be (rows,) or (%s, rows) with rows = %d, got shape %s" % (name, _COUNT[noun], self.rows, tuple(X.shape)))
        count = X2.shape[0]
        if self.rows > 1 and X2.stride(1) != 1:
            raise _lib.CapitalError("every %s of %s must be contiguous, got strides %s" % (noun, name, X.stride()))
        ldx = X2.stride(0) if count > 1 else max(self.rows, 1)
        if ldx < self.rows:
            raise _lib.CapitalError("%s: %ss overlap (strides %s)" % (name, noun, X.stride()))
        if X.device != R.device:
            raise _lib.CapitalError("%s and %s live on different devices" % (first, name))
        return X2, count, ldx

    def trsm(self, R, B, trans=True, info=None, sumsq=False):
        """ONE of the two substitutions of potrs on every block, in place: block i of the stacked B (as in potrs: (rows,) or (nrhs, rows))
        <- R_i^-T b (trans=True) or R_i^-1 b (trans=False).  In torch's row-major reading (.block) the LOWER triangle holds L = R^T:
        trans=True is L^-1 b (whitening), trans=False is L^-T b.  info: what potrf returned, or None - a block with info != 0 gets NaN.
        sumsq=True: also returns q, a fresh fp64 tensor of shape (batch, nrhs) - (batch,) for a 1-D B - in batch order with the sums of
        squares of every block's result columns (0 for an empty block).  Every block gets the bits of the fixed-size trsm on it alone.
        Returns B, or (B, q).  Asynchronous on the current stream."""
        B2, nrhs, ldb = self._stacked(R, B, "B", "right-hand side")
        q = torch.zeros((self.batch, nrhs), dtype=torch.float64, device=R.device) if sumsq else None
        lapack.engine._trsm_vbatched(self._plan, R, B2, nrhs, ldb, self.batch, bool(trans), _info(info, R), _PACK_VTS,
                                     sumsq=q if self.batch * nrhs > 0 else None, ldq=nrhs)
        if not sumsq:
            return B
        return B, (q[:, 0] if B.dim() == 1 else q)

    def trmm(self, R, B, trans=True, info=None):
        """The product with one half of every block's factor, in place: block i of the stacked B <- R_i^T b (trans=True) or R_i b
        (trans=False).  In torch's row-major reading (.block) the LOWER triangle holds L = R^T: trans=True is L z (sampling), trans=False
        is L^T z.  Returns B.  Asynchronous on the current stream."""
        B2, nrhs, ldb = self._stacked(R, B, "B", "right-hand side")
        lapack.engine._trmm_vbatched(self._plan, R, B2, nrhs, ldb, self.batch, bool(trans), _info(info, R), _PACK_VTM)
        return B

    def mahalanobis(self, R, B, info=None):
        """Squared Mahalanobis distances b_i^T A_i^-1 b_i of every block's piece of the stacked B: trsm(R, B, trans=True, sumsq=True).
        B is left WHITENED (L^-1 b with L = R^T, what torch reads in the LOWER triangle of .block).  Returns q of shape (batch, nrhs), or
        (batch,) for a 1-D B, in batch order; 0 for an empty block, NaN for a block with info != 0.  Asynchronous on the current stream."""
        return self.trsm(R, B, trans=True, info=info, sumsq=True)[1]

    def syrk(self, V, C=None, trans=False, alpha=1.0, beta=0.0, shift=None, symmetric=False):
        """Forms every block from its piece of the stacked V, one launch per size class: block i <- alpha V_i^T V_i + beta C_i (+ shift[i] I)
        in torch's reading (.block).  trans=False: V is (k, rows) or (rows,) with stride(-1) == 1, update's stacked V - block i owns entries
        row_offsets[i] .. row_offsets[i] + n_i of every row.  trans=True: V is (rows, k) with stride(-1) == 1, block i owning rows
        row_offsets[i] .. row_offsets[i] + n_i, and block i <- alpha V_i V_i^T + beta C_i.  C: the flat tensor of at least .total
        elements, or None (only with beta == 0) for a fresh zeroed one.  The triangle potrf reads is written (the LOWER one in torch's
        reading); symmetric=True mirrors it bit for bit.  shift: None, a number or a (batch,) fp64 device tensor in batch order.  Padding,
        gaps and empty blocks are neither read nor written.  Every block gets the bits of the fixed-size syrk on it alone.  Returns C.
        Asynchronous on the current stream."""
        _check(V, "V", (1, 2))
        if trans and V.dim() != 2:
            raise _lib.CapitalError("V must be (rows, k) with trans=True, got shape %s" % (tuple(V.shape),))
        V2 = V.unsqueeze(0) if V.dim() == 1 else V
        rows, k = (V2.shape[0], V2.shape[1]) if trans else (V2.shape[1], V2.shape[0])
        if rows != self.rows:
            raise _lib.CapitalError("V must be %s with rows = %d, got shape %s" % ("(rows, k)" if trans else "(rows,) or (k, rows)", self.rows, tuple(V.shape)))
        inner, outer = (k, rows) if trans else (rows, k)
        if inner > 1 and V2.stride(1) != 1:
            raise _lib.CapitalError("V must have stride(-1) == 1, got strides %s" % (V.stride(),))
        ldv = V2.stride(0) if outer > 1 else max(inner, 1)
        if ldv < inner:
            raise _lib.CapitalError("V: columns overlap (strides %s)" % (V.stride(),))
        if C is None:
            if beta != 0:
                raise _lib.CapitalError("C=None needs beta == 0")
            if self.device is None:
                raise _lib.CapitalError("there is no device - there is no CPU path")
            C = torch.zeros(max(self.total, 1), dtype=torch.float64, device=torch.device("cuda", self.device))[:self.total]
        self._flat(C, "C")
        if V.device != C.device:
            raise _lib.CapitalError("V and C live on different devices")
        _no_overlap(V, C)
        blas.engine._syrk_vbatched(self._plan, V2, C, k, ldv, self.batch, _syrk_pack(trans, alpha, beta), shift=_shift(shift, self.batch, C),
                                   fill=bool(symmetric))
        return C

    def _rows_of(self, X, name, count):
        """(X2, count, ldx) of a stacked operand (rows,) or (count, rows) with stride(-1) == 1 on the plan's device"""
        _check(X, name, (1, 2))
        X2 = X.unsqueeze(0) if X.dim() == 1 else X
        if X2.shape[1] != self.rows:
            raise _lib.CapitalError("%s must be (rows,) or (%s, rows) with rows = %d, got shape %s" % (name, count, self.rows, tuple(X.shape)))
        if self.rows > 1 and X2.stride(1) != 1:
            raise _lib.CapitalError("%s must have stride(-1) == 1, got strides %s" % (name, X.stride()))
        ldx = X2.stride(0) if X2.shape[0] > 1 else max(self.rows, 1)
        if ldx < self.rows:
            raise _lib.CapitalError("%s: rows overlap (strides %s)" % (name, X.stride()))
        if X.device.index != self.device:
            raise _lib.CapitalError("%s lives on device %s, the plan on device %s" % (name, X.device.index, self.device))
        return X2, X2.shape[0], ldx

    def inner(self, X, Y, out=None, alpha=1.0, beta=0.0):
        """The products of every block's rows of two stacked operands, ONE launch whatever the sizes:
        out[i, a, b] <- alpha sum_{r in block i} X[a, r] Y[b, r] + beta out[i, a, b] - X_i^T y_i of normal equations, W_1^T W_2 from two trsm
        results, V_i^T x.  X: (p, rows) or (rows,), Y: (q, rows) or (rows,), stacked as potrs takes B (stride(-1) == 1), p, q <= 256.  out:
        fp64 device tensor (batch, p, q) with stride(-1) == 1 and non-overlapping blocks, or None (only with beta == 0) for a fresh one, in
        which 1-D operands drop their axis.  An empty block is an empty sum and gives beta out[i] - unlike the other methods, which skip
        empty blocks.  beta == 0 does not read out.  Every block gets the bits of gemm on its rows alone.  Returns out.  Asynchronous on
        the current stream."""
        X2, p, ldx = self._rows_of(X, "X", "p")
        Y2, q, ldy = self._rows_of(Y, "Y", "q")
        if p > 256 or q > 256:
            raise _lib.CapitalError("inner takes at most 256 rows of X and of Y, got p = %d, q = %d" % (p, q))
        fresh = out is None
        if fresh:
            if beta != 0:
                raise _lib.CapitalError("out=None needs beta == 0")
            out = torch.zeros((self.batch, p, q), dtype=torch.float64, device=X.device)
        ob, op, oq, ldg, stride_g = _matrices(out, "out")
        if (ob, op, oq) != (self.batch, p, q):
            raise _lib.CapitalError("out must be (batch, p, q) = (%d, %d, %d), got shape %s" % (self.batch, p, q, tuple(out.shape)))
        if out.device != X.device:
            raise _lib.CapitalError("X and out live on different devices")
        _out_overlap(out, ((X, "X"), (Y, "Y")), alpha)
        # row-major out[i] (p x q) is the column-major q x p block Y_i^T X_i: Y is the first stacked operand
        blas.engine._gemm_vbatched_inner(self._plan, Y2, X2, out, q, p, ldy, ldx, ldg, stride_g, _gemm_pack(True, False, alpha, beta))
        if fresh:
            if Y.dim() == 1:
                out = out.squeeze(2)
            if X.dim() == 1:
                out = out.squeeze(1)
        return out

    def combine(self, Z, V, out=None, alpha=1.0, beta=0.0):
        """Combinations of every block's vectors, one launch per size class:
        out[b, row_offsets[i] + r] <- alpha sum_t Z[i, b, t] V[t, row_offsets[i] + r] + beta out[b, row_offsets[i] + r] - V_i z of low-rank
        terms.  V: (k, rows) or (rows,) with stride(-1) == 1, as update takes it; Z: (batch, q, k) with stride(-1) == 1 and non-overlapping
        blocks, q <= 256; out: (q, rows) with stride(-1) == 1, or None (only with beta == 0) for a fresh one.  Empty blocks are neither read
        nor written.  beta == 0 does not read out.  Every block gets the bits of gemm on it alone.  Returns out.  Asynchronous on the
        current stream."""
        V2, k, ldv = self._rows_of(V, "V", "k")
        zb, q, zk, ldz, stride_z = _matrices(Z, "Z")
        if zb != self.batch or zk != k:
            raise _lib.CapitalError("Z must be (batch, q, k) with batch = %d, k = %d, got shape %s" % (self.batch, k, tuple(Z.shape)))
        if q > 256:
            raise _lib.CapitalError("combine takes at most 256 rows of out, got q = %d" % q)
        if Z.device != V.device:
            raise _lib.CapitalError("V and Z live on different devices")
        if out is None:
            if beta != 0:
                raise _lib.CapitalError("out=None needs beta == 0")
            out = torch.zeros((q, self.rows), dtype=torch.float64, device=V.device)
        if out.dim() != 2 or out.shape[0] != q:
            raise _lib.CapitalError("out must be (q, rows) = (%d, %d), got shape %s" % (q, self.rows, tuple(out.shape)))
        O2, _, ldc = self._rows_of(out, "out", "q")
        _out_overlap(out, ((V, "V"), (Z, "Z")), alpha)
        blas.engine._gemm_vbatched_combine(self._plan, V2, Z, O2, q, k, ldv, max(ldz, k, 1), stride_z, ldc, _gemm_pack(False, False, alpha, beta))
        return out

    def symm(self, A, X, B=None, alpha=1.0, beta=0.0, absolute=False, out=None):
        """The product with every symmetric block itself, one launch per size class: block i of the stacked out <- beta b_i + alpha A_i x_i -
        the block-diagonal matvec.  A: the flat tensor; of every block only the triangle potrf reads is read (the LOWER one in torch's
        reading, .block).  X, B, out: (rows,) or (nrhs, rows) with stride(-1) == 1, as potrs's B.  B=None needs beta == 0; out=None: a fresh
        tensor; out may be B, it must not overlap A or X.  absolute=True: |.| of every element on load.  Every block gets the bits of the
        fixed-size symm on it alone.  Returns out.  Asynchronous on the current stream."""
        X2, nrhs, ldx = self._stacked(A, X, "X", "right-hand side", first="A")
        if B is None:
            if beta != 0:
                raise _lib.CapitalError("B=None needs beta == 0")
            B2, ldb = None, max(self.rows, 1)
        else:
            B2, nb, ldb = self._stacked(A, B, "B", "right-hand side", first="A")
            if nb != nrhs or B.dim() != X.dim():
                raise _lib.CapitalError("B must have the shape of X")
        if out is None:
            out = torch.zeros_like(X, memory_format=torch.contiguous_format)
        Y2, ny, ldy = self._stacked(A, out, "out", "right-hand side", first="A")
        if ny != nrhs or out.dim() != X.dim():
            raise _lib.CapitalError("out must have the shape of X")
        for t, name in ((A, "A"), (X, "X")):
            (a0, a1), (b0, b1) = _span(t), _span(out)
            if alpha != 0 and a0 < b1 and b0 < a1:
                raise _lib.CapitalError("%s and out overlap" % name)
        blas.engine._symm_vbatched(self._plan, A, X2, B2, Y2, nrhs, ldx, ldb, ldy, _symm_pack(alpha, beta, absolute))
        return out

    def norm1(self, A):
        """The 1-norms of all symmetric blocks of the flat tensor A, one launch per size class: a fresh fp64 tensor of batch entries in batch
        order, 0 for an empty block.  Only the triangle potrf reads is read (the LOWER one in torch's reading, .block), and it must hold the
        matrices BEFORE potrf overwrote them.  Asynchronous on the current stream."""
        self._flat(A, "A")
        out = torch.zeros(max(self.batch, 1), dtype=torch.float64, device=A.device)
        lapack.engine._lansy_vbatched(self._plan, A, self.batch, out, _PACK_VN)
        return out[:self.batch]

    def rcond(self, R, anorm, info=None):
        """EXACT reciprocal condition numbers of all blocks from the factors potrf left in the flat tensor R (not written; the triangle potrf
        wrote is read - the LOWER one in torch's reading), as rcond of this module: three launches per size class plus one.  anorm: what
        norm1 returned before potrf; info: what potrf returned, or None - a failed block gets NaN.  Returns a fresh fp64 tensor of batch
        entries in batch order, 0 for an empty block.  Every block gets the bits of the fixed-size rcond on it alone.  Asynchronous on the
        current stream."""
        self._flat(R, "R")
        anorm = _vector(anorm, self.batch, "anorm", R)
        out = torch.zeros(max(self.batch, 1), dtype=torch.float64, device=R.device)
        lapack.engine._pocon_vbatched(self._plan, R, self.batch, anorm if self.batch > 0 else None, _info(info, R), out, _PACK_VC)
        return out[:self.batch]

    def error_bounds(self, A, R, B, X, info=None, ferr=True):
        """(ferr, berr) of the stacked solutions X of A_i x = b_i, as error_bounds of this module: fresh fp64 tensors of shape (batch, nrhs) -
        (batch,) for 1-D right-hand sides - in batch order, 0 for an empty block.  A: the flat tensor of the matrices BEFORE potrf
        overwrote them, R: their factors; of both the triangle potrf reads is read (the LOWER one in torch's reading, .block).  B, X:
        (rows,) or (nrhs, rows) with stride(-1) == 1.  info: what potrf returned, or None - a failed block gets NaN.  ferr=False skips the
        inverses and returns (None, berr).  Every block gets the bits of the fixed-size error_bounds on it alone.  Asynchronous on the
        current stream."""
        self._flat(A, "A")
        X2, nrhs, ldx = self._stacked(R, X, "X", "right-hand side")
        B2, nb, ldb = self._stacked(R, B, "B", "right-hand side")
        if nb != nrhs or B.dim() != X.dim() or A.device != R.device:
            raise _lib.CapitalError("B must have the shape of X, and A must live on R's device")
        lde = max(nrhs, 1)
        fe = torch.zeros((max(self.batch, 1), lde), dtype=torch.float64, device=R.device) if ferr else None
        be = torch.zeros((max(self.batch, 1), lde), dtype=torch.float64, device=R.device)
        lapack.engine._poerr_vbatched(self._plan, A, R, B2, X2, nrhs, ldb, ldx, self.batch, _info(info, R), fe, be, lde, _PACK_VE)
        shape = lambda t: None if t is None else (t[:self.batch, 0] if X.dim() == 1 else t[:self.batch, :nrhs])
        return shape(fe), shape(be)

    def pstrf(self, A, max_rank=None, tol=-1.0, logdet=False):
        """PIVOTED Cholesky factors of all blocks (every n_i <= 64), one launch per size class, as pstrf of this module.  A: the flat
        tensor; of every block only the triangle potrf reads is read (the LOWER one in torch's reading, .block) and A is not written.  The
        cap of block i is min(max_rank, n_i) (None: no cap).  Returns (R, piv, rank, resid, info), plus logdet with logdet=True:
        R: a fresh flat tensor in the plan's layout - .block(R, i) reads as the n_i x n_i lower-triangular L_i with
        L_i L_i^T ~ A_i[piv_i][:, piv_i] and zero columns >= rank[i]; every entry of every block is written, padding and gaps are zero.
        piv: the stacked int64 (rows,) vector of block-local indices, block i at row_offsets[i] (VarBatch.permute applies it).
        rank, resid, info, logdet: (batch,) in batch order, 0 for an empty block.  info is 0 / 1 / 2 as for cap_dpstrf - NOT the info
        that trsm, trmm or potrs expect; pass (info == 2).int() there if a guard is wanted.  Every block gets the bits of the fixed-size
        pstrf on it alone.  A plan whose largest block exceeds 64 raises CapitalError: use cholinv.factor_pivoted per block.
        Asynchronous on the current stream; nothing is read back."""
        nmax = max(self.sizes, default=0)
        mr, tol = _pstrf_args(None if max_rank is None else min(max(int(max_rank), -1), nmax), nmax, tol)     # (a cap above n_i is n_i)
        self._flat(A, "A")
        R = torch.zeros(max(self.total, 1), dtype=torch.float64, device=A.device)[:self.total]
        piv = torch.zeros(max(self.rows, 1), dtype=torch.int64, device=A.device)[:self.rows]
        rank, resid, info, ld = lapack.engine._pstrf_vbatched(self._plan, A, R, piv, self.rows, nmax, mr, self.batch, tol, _PACK_VP,
                                                              want_logdet=bool(logdet))
        return (R, piv, rank, resid, info, ld) if logdet else (R, piv, rank, resid, info)

    def permute(self, B, piv, inverse=False):
        """The pivoting of VarBatch.pstrf applied to stacked vectors (torch only).  B: (rows,) or (nrhs, rows); piv: the stacked
        block-local indices pstrf returned.  inverse=False: entry row_offsets[i] + k of the result is entry row_offsets[i] + piv_i[k] of B;
        inverse=True undoes it.  Returns a fresh tensor."""
        if (not isinstance(B, torch.Tensor) or not isinstance(piv, torch.Tensor) or B.dim() not in (1, 2) or piv.dim() != 1
                or piv.dtype != torch.int64 or piv.shape[0] != self.rows or B.shape[-1] != self.rows or piv.device != B.device):
            raise _lib.CapitalError("B must be (rows,) or (nrhs, rows) and piv an int64 (rows,) tensor on its device, rows = %d" % self.rows)
        base = getattr(self, "_row_base", None)
        if base is None or base.device != B.device:
            host = [r for r, n in zip(self.row_offsets, self.sizes) for _ in range(n)]
            base = self._row_base = torch.tensor(host, dtype=torch.int64).to(B.device)
        idx = piv + base
        idx = idx if B.dim() == 1 else idx.unsqueeze(0).expand(B.shape)
        if inverse:
            return torch.empty_like(B, memory_format=torch.contiguous_format).scatter_(-1, idx, B)
        return torch.gather(B, -1, idx)

    def block(self, A, i):
        """The n_i x n_i view of block i of the flat tensor A in torch's row-major reading: block(A, i)[r, c] is element (c, r) of the
        column-major block, so after potrf torch sees L (lower triangular, L L^T = A_i) in the LOWER triangle of the view, as in potrf
        of this module."""
        n = self.sizes[i]
        return A.as_strided((n, n), (self.ld[i], 1), A.storage_offset() + self.offsets[i])

    def pack(self, blocks, device=None):
        """The flat fp64 device tensor (.total elements, zeros in padding and gaps) that holds blocks[i] (2-D, n_i x n_i, any dtype /
        device) as block i in torch's reading: pack(bl) followed by block(., i) gives bl[i] back."""
        if len(blocks) != self.batch:
            raise _lib.CapitalError("pack needs one matrix per block (%d), got %d" % (self.batch, len(blocks)))
        for i, b in enumerate(blocks):
            if not isinstance(b, torch.Tensor) or tuple(b.shape) != (self.sizes[i], self.sizes[i]):
                raise _lib.CapitalError("block %d must be a %d x %d tensor, got %s" % (i, self.sizes[i], self.sizes[i], tuple(getattr(b, "shape", ()))))
        if device is None and self.device is None:
            raise _lib.CapitalError("there is no device to pack to - there is no CPU path")
        A = torch.zeros(max(self.total, 1), dtype=torch.float64, device=torch.device("cuda", self.device if device is None else device))
        for i, b in enumerate(blocks):
            if self.sizes[i]:
                self.block(A, i).copy_(b)
        return A[:self.total]


class VarChains:
    """A batch of block-tridiagonal SPD chains of DIFFERENT lengths T_c >= 0 (ragged time series, smoothers, state-space likelihoods) in
    ONE pair of tensors: D is a sequence of n x n SLOTS, chain c owning slots first[c] .. first[c] + T_c - 1, and E is addressed with the
    SAME slot indices - E[first[c] + i] couples positions i and i + 1 of chain c, the last slot of every chain is never touched - so D and
    E can be two tensors of one shape.  lengths, first: host sequences of ints; first=None: the chains lie back to back in batch order.
    The plan (cap_blocktri_plan) knows no n: it serves any n <= 64, one n per call.  It sorts the chains once by length (descending,
    stable: .order) so that the chains of a wavefront have neighbouring lengths, and lives on the device that is current when it is made;
    building and freeing it may synchronise, no other method does.  It is reusable for any number of calls, from several streams at once.
    Every call is ONE launch, and every chain gets, BIT FOR BIT, what blocktri_potrf / blocktri_potrs / blocktri_potri give for it alone
    (a batch of one chain of T_c positions) - whichever chains travel with it, whatever first, the batch order and the strides.
    Never touched: slots no chain owns, every chain's last slot of E, pad rows and gaps, what torch reads as the strictly upper triangles of
    the D blocks (unless symmetric=True), and everything of a chain with T_c = 0 (its info and logdet are 0).
    .lengths / .first / .row_offsets: tuples in batch order (row_offsets: the prefix sum of the lengths - the block rows of the stacked
    right-hand sides); .slots: slots D must hold; .eslots: slots E must hold (0: E may be None); .rows: sum of the lengths; .tmax: the
    longest chain; .order: the plan's list; .batch.  Negative lengths or slots and overlapping chains raise CapitalError."""

    def __init__(self, lengths, first=None):
        self.lengths = tuple(int(x) for x in lengths)
        batch = len(self.lengths)
        if first is not None and len(first) != batch:
            raise _lib.CapitalError("first must have one entry per chain (%d), got %d" % (batch, len(first)))
        arr = lambda seq: (ctypes.c_int64 * max(batch, 1))(*[int(x) for x in seq]) if seq is not None else None
        L = _lib.lib()
        self._L, self._plan = L, ctypes.c_void_p()
        _lib.check(L.cap_blocktri_plan_create(batch, arr(self.lengths), arr(first), ctypes.byref(self._plan)), "VarChains")
        self.batch = batch
        rows, at = [], 0
        for t in self.lengths:
            rows.append(at)
            at += t
        self.row_offsets = tuple(rows)
        self.first = tuple(int(x) for x in first) if first is not None else self.row_offsets
        self.slots = int(L.cap_blocktri_plan_info(self._plan, 1))
        self.eslots = int(L.cap_blocktri_plan_info(self._plan, 2))
        self.rows = int(L.cap_blocktri_plan_info(self._plan, 3))
        self.tmax = int(L.cap_blocktri_plan_info(self._plan, 4))
        order = (ctypes.c_int64 * max(batch, 1))()
        _lib.check(L.cap_blocktri_plan_order(self._plan, order, batch), "VarChains")
        self.order = tuple(int(order[k]) for k in range(batch))
        self.device = torch.cuda.current_device() if torch.cuda.is_available() else None

    def __del__(self):
        plan, self._plan = getattr(self, "_plan", None), None
        if plan:
            self._L.cap_blocktri_plan_destroy(plan)

    def _slots_of(self, t, name, need, n=None):
        """(n, ld, step) of a (slots, n, n) tensor whose t[s] is read as column-major memory with ld = stride(1)"""
        _check(t, name, (3,))
        k, r, c = t.shape
        if r != c or k < need or (n is not None and r != n):
            raise _lib.CapitalError("%s must be (at least %d, n, n)%s, got shape %s" % (name, need, "" if n is None else " with n = %d" % n, tuple(t.shape)))
        if r > 64:
            raise _lib.CapitalError("block-tridiagonal Cholesky takes blocks of at most 64 rows, got n = %d" % r)
        if t.device.index != self.device:
            raise _lib.CapitalError("%s lives on device %s, the plan on device %s" % (name, t.device.index, self.device))
        if t.numel() == 0:
            return r, max(r, 1), max(r * r, 1)
        if r > 1 and t.stride(2) != 1:
            raise _lib.CapitalError("%s must have stride(-1) == 1, got strides %s" % (name, t.stride()))
        ld = t.stride(1) if r > 1 else max(t.stride(1), 1)
        step = t.stride(0)
        if ld < r or (k > 1 and step < ld * r):
            raise _lib.CapitalError("%s: blocks overlap (strides %s)" % (name, t.stride()))
        return r, ld, max(step, 0)

    def _pair(self, D, E):
        n, ldd, step_d = self._slots_of(D, "D", self.slots)
        if E is None:
            if self.eslots > 0:
                raise _lib.CapitalError("E may be None only when no chain has more than one position")
            return n, ldd, step_d, max(n, 1), max(n * n, 1)
        _, lde, step_e = self._slots_of(E, "E", self.eslots, n)
        (a0, a1), (b0, b1) = _span(D), _span(E)
        if a0 < b1 and b0 < a1:
            raise _lib.CapitalError("D and E overlap")
        return n, ldd, step_d, lde, step_e

    def potrf(self, D, E, logdet=False):
        """Cholesky factors of all chains, in place, in ONE launch.  D: fp64 device tensor (>= .slots, n, n), n <= 64; E: (>= .eslots, n, n)
        with E[first_c + i] = A_c[block i + 1, block i] in torch's reading, or None when .eslots == 0.  Both follow blocktri_potrf's
        reading and layout freedoms (stride(-1) == 1, stride(-2) >= n, stride(0) >= stride(-2) n): L_ii replaces the LOWER triangle of
        D[first_c + i], L_(i+1, i) replaces E[first_c + i].  Returns info (int32, batch order: 0, or the 1-based row inside chain c's own
        T_c n system of the first pivot that is not > 0 - from there on the chain holds NaN; 0 for an empty chain), or (info, logdet).
        Chain c's bits are those of blocktri_potrf on it alone.  Asynchronous on the current stream; nothing is read back."""
        n, ldd, step_d, lde, step_e = self._pair(D, E)
        info, ld = lapack.engine._potrf_blocktri_vbatched(self._plan, D, E, n, ldd, step_d, lde, step_e, self.batch, _PACK_BF,
                                                          want_logdet=bool(logdet))
        return (info, ld) if logdet else info

    def potrs(self, D, E, B, info=None, half=None):
        """Solves A_c x = b_c for all chains in place with the factors potrf left in D and E, in ONE launch.  B: fp64 device tensor of
        shape (rows n,) or (nrhs, rows n) with stride(-1) == 1 - every right-hand side is the stacked vector, chain c owning entries
        n row_offsets[c] .. n (row_offsets[c] + T_c).  half: None / "forward" / "backward" as in blocktri_potrs; "forward" followed by
        "backward" leaves the bits of the full solve.  info: what potrf returned, or None - a chain with info != 0 gets NaN.
        Chain c's bits are those of blocktri_potrs on it alone.  Returns B.  Asynchronous on the current stream."""
        if half not in _PACK_BS:
            raise _lib.CapitalError("half must be None, 'forward' or 'backward', got %r" % (half,))
        n, ldd, step_d, lde, step_e = self._pair(D, E)
        _check(B, "B", (1, 2))
        B2 = B.unsqueeze(0) if B.dim() == 1 else B
        total = self.rows * n
        if B2.shape[1] != total:
            raise _lib.CapitalError("B must be (rows n,) or (nrhs, rows n) with rows n = %d, got shape %s" % (total, tuple(B.shape)))
        nrhs = B2.shape[0]
        if total > 1 and B2.stride(1) != 1:
            raise _lib.CapitalError("every right-hand side of B must be contiguous, got strides %s" % (B.stride(),))
        ldb = B2.stride(0) if nrhs > 1 else max(total, 1)
        if ldb < total:
            raise _lib.CapitalError("B: right-hand sides overlap (strides %s)" % (B.stride(),))
        if B.device != D.device:
            raise _lib.CapitalError("D and B live on different devices")
        for t, name in ((D, "D"), (E, "E")):
            if t is not None:
                (a0, a1), (b0, b1) = _span(t), _span(B)
                if a0 < b1 and b0 < a1:
                    raise _lib.CapitalError("%s and B overlap" % name)
        lapack.engine._potrs_blocktri_vbatched(self._plan, D, E, B2, n, nrhs, ldd, step_d, lde, step_e, ldb, self.batch, _info(info, D), _PACK_BS[half])
        return B

    def potri(self, D, E, info=None, symmetric=False):
        """The marginal covariances of all chains from the factors potrf left in D and E, in place, in ONE launch: afterwards the LOWER
        triangle of D[first_c + i] holds Sigma_c[block i, block i] and E[first_c + i] holds Sigma_c[block i + 1, block i] in torch's
        reading; symmetric=True makes the other triangle of every owned D block the bit-identical mirror.  info: what potrf returned, or
        None - a chain with info != 0 gets NaN wherever the call writes.  Chain c's bits are those of blocktri_potri on it alone.
        Returns (D, E).  Asynchronous on the current stream."""
        n, ldd, step_d, lde, step_e = self._pair(D, E)
        lapack.engine._potri_blocktri_vbatched(self._plan, D, E, n, ldd, step_d, lde, step_e, self.batch, _info(info, D), _PACK_BI,
                                               fill=bool(symmetric))
        return D, E

    def chain(self, X, c):
        """The view X[first_c : first_c + T_c] of chain c's slots of D (for E: its last entry is the slot that is never touched)"""
        return X[self.first[c]:self.first[c] + self.lengths[c]]

    def pack(self, chains, device=None):
        """(D, E): two zero-filled fp64 device tensors of shape (max(slots, 1), n, n) that hold chains[c] = (D_c, E_c) - D_c (T_c, n, n) and
        E_c (T_c - 1, n, n) or None, any dtype / device - in chain c's slots: chain(D, c) gives D_c back, chain(E, c)[:-1] gives E_c."""
        if len(chains) != self.batch:
            raise _lib.CapitalError("pack needs one (D, E) pair per chain (%d), got %d" % (self.batch, len(chains)))
        if device is None and self.device is None:
            raise _lib.CapitalError("there is no device to pack to - there is no CPU path")
        n = None
        for c, (Dc, Ec) in enumerate(chains):
            T = self.lengths[c]
            if not isinstance(Dc, torch.Tensor) or Dc.dim() != 3 or Dc.shape[0] != T or Dc.shape[1] != Dc.shape[2] or (n is not None and Dc.shape[1] != n):
                raise _lib.CapitalError("chain %d: D must be a (%d, n, n) tensor, got %s" % (c, T, tuple(getattr(Dc, "shape", ()))))
            n = Dc.shape[1]
            if T > 1 and (not isinstance(Ec, torch.Tensor) or tuple(Ec.shape) != (T - 1, n, n)):
                raise _lib.CapitalError("chain %d: E must be a (%d, %d, %d) tensor, got %s" % (c, T - 1, n, n, tuple(getattr(Ec, "shape", ()))))
        n = n or 0
        dev = torch.device("cuda", self.device if device is None else device)
        D = torch.zeros((max(self.slots, 1), n, n), dtype=torch.float64, device=dev)
        E = torch.zeros((max(self.slots, 1), n, n), dtype=torch.float64, device=dev)
        for c, (Dc, Ec) in enumerate(chains):
            T = self.lengths[c]
            if T:
                self.chain(D, c).copy_(Dc)
            if T > 1:
                self.chain(E, c)[:-1].copy_(Ec)
        return D, E
