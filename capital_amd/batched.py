"""Many small SPD systems of one size on plain torch tensors: one launch factors (potrf), solves (potrs) or inverts (potri, trtri) the
whole batch.

The tensors are the memory the C ABI works on: fp64, on the device, n <= 256 (n <= 64: cap_dpotrf_batched / cap_dpotrs_batched,
csrc/potrf_batched.hip, a wavefront per block; 64 < n <= 256: cap_dpotrf_batched_blocked / cap_dpotrs_batched_blocked,
csrc/potrf_batched_blocked.hip, a workgroup per block; the inverses: cap_dtrtri_batched / cap_dpotri_batched, csrc/potri_batched.hip, one
entry each for the whole range).
There is no CPU path and no fallback: anything else raises CapitalError."""
import torch

from . import _lib, lapack

_PACK_F = lapack.ArgPack_potrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_S = lapack.ArgPack_potrs_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_T = lapack.ArgPack_trtri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
_PACK_I = lapack.ArgPack_potri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)


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
    batch, n, ldr, stride_r = _blocks(R, "R")
    _check(B, "B", (2, 3))
    B3 = B.unsqueeze(1) if B.dim() == 2 else B
    if B3.shape[0] != batch or B3.shape[2] != n:
        raise _lib.CapitalError("B must be (batch, nrhs, n) or (batch, n) with batch = %d, n = %d, got shape %s" % (batch, n, tuple(B.shape)))
    nrhs = B3.shape[1]
    if n > 1 and B3.stride(2) != 1:
        raise _lib.CapitalError("every right-hand side of B must be contiguous, got strides %s" % (B.stride(),))
    ldb = B3.stride(1) if nrhs > 1 else max(n, 1)
    stride_b = B3.stride(0)
    if ldb < n or (batch > 1 and stride_b < ldb * nrhs):
        raise _lib.CapitalError("B: right-hand sides overlap (strides %s)" % (B.stride(),))
    if B.device != R.device:
        raise _lib.CapitalError("R and B live on different devices")
    lapack.engine._potrs_batched(R, B3, n, nrhs, ldr, stride_r, ldb, max(stride_b, 0), batch, info, _PACK_S)
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
