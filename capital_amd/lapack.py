"""lapack::engine mirror (reference src/lapack/engine.h:23-102, src/lapack/interface.h:49-59).

_potrs (A X = B with the factor of _potrf), _potri (A^-1 from that factor), _cholupdate (that factor after A +- V V^T), _pstrf (the
pivoted factorization of a semidefinite A, LAPACK's dpstrf), _lansy (the 1-norm of a symmetric matrix), _pocon (the reciprocal condition
number from the factor, LAPACK's dpocon), _poerr (the error bounds of LAPACK's dporfs) and _potrf_batched / _potrs_batched / _trtri_batched /
_potri_batched (the factor, solve, triangular inverse and SPD inverse of many small blocks of one size in one launch) and _potrf_vbatched /
_potrs_vbatched / _potri_vbatched (the same for blocks of different sizes, described by a cap_vbatch_plan) and _cholupdate_batched /
_cholupdate_vbatched (the rank-k update / downdate of those factors) and _trsm_batched / _trmm_batched / _trsm_vbatched / _trmm_vbatched
(one triangular solve or product with those factors) and _lansy_batched / _pocon_batched / _poerr_batched with their _vbatched forms (the
1-norms, the exact reciprocal condition numbers and the solve error bounds of those blocks) and _pstrf_batched / _pstrf_vbatched (the
pivoted factorization of semidefinite blocks of up to 64 rows) have no counterpart upstream.
_potrf / _trtri run on the GPU (wavefront-cooperative in-LDS leaves + MFMA GEMM recursion).
Unlike upstream (which drops LAPACKE's return value, lapack/interface.hpp:39,54) _potrf
returns `info`.  _geqrf / _orgqr are never called by any upstream algorithm
and are out of scope."""
import enum

import torch

from . import _lib
from ._util import dptr, cur_stream, scratch


class Order(enum.IntEnum):
    AlapackRowMajor = 0x0
    AlapackColumnMajor = 0x1


class UpLo(enum.IntEnum):
    AlapackLower = 0x0
    AlapackUpper = 0x1


class Diag(enum.IntEnum):
    AlapackNonUnit = 0x0
    AlapackUnit = 0x1


class Method(enum.IntEnum):
    AlapackPotrf = 0x0
    AlapackTrtri = 0x1
    AlapackPotrs = 0x2          # extension: not in the reference's enum
    AlapackPotri = 0x3          # extension: not in the reference's enum
    AlapackCholupdate = 0x4     # extension: not in the reference's enum
    AlapackPstrf = 0x5          # extension: not in the reference's enum
    AlapackLansy = 0x6          # extension: not in the reference's enum
    AlapackPocon = 0x7          # extension: not in the reference's enum
    AlapackPoerr = 0x8          # extension: not in the reference's enum
    AlapackPotrfBatched = 0x9   # extension: not in the reference's enum
    AlapackPotrsBatched = 0xA   # extension: not in the reference's enum
    AlapackTrtriBatched = 0xB   # extension: not in the reference's enum
    AlapackPotriBatched = 0xC   # extension: not in the reference's enum
    AlapackPotrfVbatched = 0xD  # extension: not in the reference's enum
    AlapackPotrsVbatched = 0xE  # extension: not in the reference's enum
    AlapackPotriVbatched = 0xF  # extension: not in the reference's enum
    AlapackGeqrf = 0x10
    AlapackOrgqr = 0x11
    AlapackCholupdateBatched = 0x12    # extension: not in the reference's enum
    AlapackCholupdateVbatched = 0x13   # extension: not in the reference's enum
    AlapackTrsmBatched = 0x14          # extension: not in the reference's enum
    AlapackTrmmBatched = 0x15          # extension: not in the reference's enum
    AlapackTrsmVbatched = 0x16         # extension: not in the reference's enum
    AlapackTrmmVbatched = 0x17         # extension: not in the reference's enum
    AlapackLansyBatched = 0x18         # extension: not in the reference's enum
    AlapackPoconBatched = 0x19         # extension: not in the reference's enum
    AlapackPoerrBatched = 0x1A         # extension: not in the reference's enum
    AlapackLansyVbatched = 0x1B        # extension: not in the reference's enum
    AlapackPoconVbatched = 0x1C        # extension: not in the reference's enum
    AlapackPoerrVbatched = 0x1D        # extension: not in the reference's enum
    AlapackPstrfBatched = 0x1E         # extension: not in the reference's enum
    AlapackPstrfVbatched = 0x1F        # extension: not in the reference's enum
    AlapackPotrfBlocktriBatched = 0x20 # extension: not in the reference's enum
    AlapackPotrsBlocktriBatched = 0x21 # extension: not in the reference's enum
    AlapackPotriBlocktriBatched = 0x22 # extension: not in the reference's enum


class ArgPack_potrf:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotrf
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potrs:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotrs
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potri:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotri
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_cholupdate:
    def __init__(self, order, uplo):
        self.method = Method.AlapackCholupdate
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_pstrf:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPstrf
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_lansy:
    def __init__(self, order, uplo, norm='1'):
        self.method = Method.AlapackLansy
        self.order, self.uplo, self.norm = Order(order), UpLo(uplo), norm


class ArgPack_pocon:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPocon
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_poerr:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPoerr
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potrf_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotrfBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potrs_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotrsBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_trtri_batched:
    def __init__(self, order, uplo, diag=Diag.AlapackNonUnit):
        self.method = Method.AlapackTrtriBatched
        self.order, self.uplo, self.diag = Order(order), UpLo(uplo), Diag(diag)


class ArgPack_potri_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotriBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potrf_vbatched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotrfVbatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potrs_vbatched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotrsVbatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potri_vbatched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotriVbatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_cholupdate_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackCholupdateBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_cholupdate_vbatched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackCholupdateVbatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_trsm_batched:
    def __init__(self, order, uplo, diag=Diag.AlapackNonUnit):
        self.method = Method.AlapackTrsmBatched
        self.order, self.uplo, self.diag = Order(order), UpLo(uplo), Diag(diag)


class ArgPack_trmm_batched:
    def __init__(self, order, uplo, diag=Diag.AlapackNonUnit):
        self.method = Method.AlapackTrmmBatched
        self.order, self.uplo, self.diag = Order(order), UpLo(uplo), Diag(diag)


class ArgPack_trsm_vbatched:
    def __init__(self, order, uplo, diag=Diag.AlapackNonUnit):
        self.method = Method.AlapackTrsmVbatched
        self.order, self.uplo, self.diag = Order(order), UpLo(uplo), Diag(diag)


class ArgPack_trmm_vbatched:
    def __init__(self, order, uplo, diag=Diag.AlapackNonUnit):
        self.method = Method.AlapackTrmmVbatched
        self.order, self.uplo, self.diag = Order(order), UpLo(uplo), Diag(diag)


class ArgPack_lansy_batched:
    def __init__(self, order, uplo, norm='1'):
        self.method = Method.AlapackLansyBatched
        self.order, self.uplo, self.norm = Order(order), UpLo(uplo), norm


class ArgPack_pocon_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPoconBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_poerr_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPoerrBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_lansy_vbatched:
    def __init__(self, order, uplo, norm='1'):
        self.method = Method.AlapackLansyVbatched
        self.order, self.uplo, self.norm = Order(order), UpLo(uplo), norm


class ArgPack_pocon_vbatched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPoconVbatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_poerr_vbatched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPoerrVbatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_pstrf_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPstrfBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_pstrf_vbatched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPstrfVbatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potrf_blocktri_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotrfBlocktriBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


class ArgPack_potrs_blocktri_batched:
    def __init__(self, order, uplo, half=0):
        self.method = Method.AlapackPotrsBlocktriBatched
        self.order, self.uplo, self.half = Order(order), UpLo(uplo), int(half)      # half: 0 both sweeps, 1 forward only, 2 backward only


class ArgPack_potri_blocktri_batched:
    def __init__(self, order, uplo):
        self.method = Method.AlapackPotriBlocktriBatched
        self.order, self.uplo = Order(order), UpLo(uplo)


BATCHED_SMALL_MAX = 64      # cap_dpotrf_batched / cap_dpotrs_batched: a wavefront per block
BATCHED_MAX = 256           # cap_dpotrf_batched_blocked / cap_dpotrs_batched_blocked: a workgroup per block


def _batched_blocked(L, n):
    """the library, once n is known to be within the batched calls' limit"""
    if n > BATCHED_MAX:
        raise _lib.CapitalError("batched Cholesky: blocks of n = %d rows exceed the limit of %d rows per block" % (n, BATCHED_MAX))
    return L


class ArgPack_trtri:
    def __init__(self, order, uplo, diag):
        self.method = Method.AlapackTrtri
        self.order, self.uplo, self.diag = Order(order), UpLo(uplo), Diag(diag)


class engine:
    @staticmethod
    def _potrf(matrixA, n, lda, srcPackage, stream=None):
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        work = scratch(L.cap_dpotrf_work_size(n), matrixA)
        info = torch.zeros(1, dtype=torch.int32, device=work.device)
        st = L.cap_dpotrf(int(srcPackage.uplo), n, dptr(matrixA), lda, info.data_ptr(), dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrf")
        return int(info.item())

    @staticmethod
    def _potrs(matrixR, matrixB, n, nrhs, ldr, ldb, srcPackage, stream=None):
        """B (n x nrhs, ld ldb) <- A^-1 B with A = R^T R, R the upper factor _potrf left (ld ldr)."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        work = scratch(L.cap_dpotrs_work_size(n, nrhs), matrixB)
        st = L.cap_dpotrs(int(srcPackage.uplo), n, nrhs, dptr(matrixR), ldr, dptr(matrixB), ldb, dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrs")

    @staticmethod
    def _potri(matrixA, n, lda, srcPackage, stream=None):
        """The upper triangle of A (n x n, ld lda; the factor R _potrf left) <- that of A^-1 = R^-1 R^-T; the other triangle is untouched."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        work = scratch(L.cap_dpotri_work_size(n), matrixA)
        st = L.cap_dpotri(int(srcPackage.uplo), n, dptr(matrixA), lda, dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_potri")

    @staticmethod
    def _cholupdate(matrixR, matrixV, n, k, ldr, ldv, sign, srcPackage, stream=None):
        """The upper factor R (n x n, ld ldr; what _potrf left) <- the factor of R^T R + sign V V^T, V n x k (ld ldv, not written),
        sign = +1 / -1.  Returns info: 0, or the 1-based row at which a downdate found the matrix not positive definite (R is lost then)."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        work = scratch(L.cap_dcholupdate_work_size(n, k), matrixR)
        info = torch.zeros(1, dtype=torch.int32, device=work.device)
        st = L.cap_dcholupdate(int(srcPackage.uplo), int(sign), n, k, dptr(matrixR), ldr, dptr(matrixV), ldv, info.data_ptr(), dptr(work),
                               cur_stream(stream))
        _lib.check(st, "lapack::engine::_cholupdate")
        return int(info.item())

    @staticmethod
    def _pstrf(matrixA, matrixR, piv, n, max_rank, lda, ldr, tol, srcPackage, stream=None):
        """Pivoted Cholesky of the symmetric positive semidefinite A (n x n, ld lda; its upper triangle is read, nothing of it written) in at
        most max_rank steps: A[piv][:, piv] ~ R^T R with R max_rank x n (ld ldr) and piv an int64 device tensor of n entries (the pivots in
        order, then the unselected indices).  tol < 0: n eps max_i a_ii, otherwise absolute.  Returns (rank, info, resid) - info 0: stopped
        at a pivot <= tol, 1: max_rank steps done with the remainder above tol, 2: a NaN on the remaining diagonal; resid = trace(A - R^T R).
        Reading them back SYNCHRONISES the stream."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if not isinstance(piv, torch.Tensor) or not piv.is_cuda or piv.dtype != torch.int64 or piv.numel() < n or not piv.is_contiguous():
            raise _lib.CapitalError("piv must be a contiguous int64 device tensor of n entries")
        L = _lib.lib()
        work = scratch(L.cap_dpstrf_work_size(n, max_rank), matrixA)
        rank = torch.zeros(1, dtype=torch.int64, device=work.device)
        info = torch.zeros(1, dtype=torch.int32, device=work.device)
        resid = torch.zeros(1, dtype=torch.float64, device=work.device)
        st = L.cap_dpstrf(int(srcPackage.uplo), n, max_rank, float(tol), dptr(matrixA), lda, dptr(matrixR), ldr, piv.data_ptr(),
                          rank.data_ptr(), resid.data_ptr(), info.data_ptr(), dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_pstrf")
        return int(rank.item()), int(info.item()), float(resid.item())

    @staticmethod
    def _lansy(matrixA, n, lda, srcPackage, stream=None):
        """||A||_1 (srcPackage.norm = '1', 'O' or 'I': equal for a symmetric matrix) of the symmetric A (n x n, ld lda), read from its upper
        triangle alone, as a 1-element fp64 device tensor.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        work = scratch(max(L.cap_dlansy_work_size(n), 2), matrixA)
        out = torch.zeros(1, dtype=torch.float64, device=work.device)
        st = L.cap_dlansy(ord(srcPackage.norm), int(srcPackage.uplo), n, dptr(matrixA), lda, out.data_ptr(), dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_lansy")
        return out

    @staticmethod
    def _pocon(matrixR, n, ldr, anorm, srcPackage, stream=None):
        """Reciprocal condition number 1 / (anorm est ||A^-1||_1) of A = R^T R, R the upper factor _potrf left (n x n, ld ldr), anorm =
        ||A||_1 as a 1-element fp64 device tensor (_lansy).  Returns a 1-element fp64 device tensor.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        work = scratch(max(L.cap_dpocon_work_size(n), 2), matrixR)
        out = torch.zeros(1, dtype=torch.float64, device=work.device)
        st = L.cap_dpocon(int(srcPackage.uplo), n, dptr(matrixR), ldr, anorm.data_ptr(), out.data_ptr(), dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_pocon")
        return out

    @staticmethod
    def _poerr(matrixA, matrixR, matrixB, matrixX, n, nrhs, lda, ldr, ldb, ldx, srcPackage, stream=None):
        """(ferr, berr) of LAPACK's dporfs, without its refinement, for the computed solution X (n x nrhs, ld ldx) of A X = B: A symmetric
        (upper triangle read, ld lda), R its upper factor (ld ldr), B n x nrhs (ld ldb).  Two fp64 device tensors of nrhs entries.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        work = scratch(max(L.cap_dpoerr_work_size(n, nrhs), 2), matrixA)
        ferr = torch.zeros(max(nrhs, 1), dtype=torch.float64, device=work.device)
        berr = torch.zeros(max(nrhs, 1), dtype=torch.float64, device=work.device)
        st = L.cap_dpoerr(int(srcPackage.uplo), n, nrhs, dptr(matrixA), lda, dptr(matrixR), ldr, dptr(matrixB), ldb, dptr(matrixX), ldx,
                          ferr.data_ptr(), berr.data_ptr(), dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_poerr")
        return ferr[:nrhs], berr[:nrhs]

    @staticmethod
    def _potrf_batched(matrixA, n, lda, stride, batch, srcPackage, want_logdet=False, stream=None):
        """The n x n blocks (n <= 256, column-major, ld lda) at matrixA + i stride, i < batch, <- their upper factors, in one launch (n <= 64:
        cap_dpotrf_batched, a wavefront per block; 64 < n <= 256: cap_dpotrf_batched_blocked, a workgroup per block).  Returns
        (info, logdet): an int32 device tensor of batch entries (0, or the 1-based first pivot that is not > 0; such a block holds NaN from
        that row on) and, with want_logdet, an fp64 one with 2 sum log r_jj (NaN for a failed block), else None.  Nothing is read back:
        asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        fn = L.cap_dpotrf_batched if n <= BATCHED_SMALL_MAX else _batched_blocked(L, n).cap_dpotrf_batched_blocked
        a = dptr(matrixA)
        dev = matrixA.device if isinstance(matrixA, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        info = torch.zeros(max(batch, 1), dtype=torch.int32, device=dev)
        logdet = torch.zeros(max(batch, 1), dtype=torch.float64, device=dev) if want_logdet else None
        st = fn(int(srcPackage.uplo), n, a, lda, stride, batch, info.data_ptr(), logdet.data_ptr() if want_logdet else None, cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrf_batched")
        return info[:max(batch, 0)], (logdet[:max(batch, 0)] if want_logdet else None)

    @staticmethod
    def _potrs_batched(matrixR, matrixB, n, nrhs, ldr, stride_r, ldb, stride_b, batch, info, srcPackage, stream=None):
        """B_i (n x nrhs, ld ldb, at matrixB + i stride_b) <- A_i^-1 B_i with A_i = R_i^T R_i, R_i the upper factor _potrf_batched left at
        matrixR + i stride_r (ld ldr), n <= 256.  info: what _potrf_batched returned, or None; a block with info != 0 gets NaN.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if info is not None and (not isinstance(info, torch.Tensor) or not info.is_cuda or info.dtype != torch.int32
                                 or info.numel() < batch or not info.is_contiguous()):
            raise _lib.CapitalError("info must be a contiguous int32 device tensor of batch entries")
        L = _lib.lib()
        fn = L.cap_dpotrs_batched if n <= BATCHED_SMALL_MAX else _batched_blocked(L, n).cap_dpotrs_batched_blocked
        st = fn(int(srcPackage.uplo), n, nrhs, dptr(matrixR), ldr, stride_r, dptr(matrixB), ldb, stride_b, batch,
                info.data_ptr() if info is not None else None, cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrs_batched")

    @staticmethod
    def _potrf_blocktri_batched(matrixD, matrixE, n, T, ldd, step_d, stride_d, lde, step_e, stride_e, batch, srcPackage, want_logdet=False, stream=None):
        """`batch` block-tridiagonal SPD chains of T diagonal blocks of n x n, n <= 64, <- their block bidiagonal Cholesky factors, in place, in
        one launch (cap_dpotrf_blocktri_batched): block (c, i) of D is column-major with ld ldd at matrixD + c stride_d + i step_d, E likewise
        with T - 1 blocks per chain (matrixE may be None when T <= 1).  U_i replaces the upper triangle of D_i, W_i = U_i^-T A[i, i + 1]
        replaces E_i.  Returns (info, logdet): an int32 device tensor of batch entries (0, or the 1-based row of the T n system of the first
        pivot that is not > 0) and, with want_logdet, an fp64 one with log det A_c (NaN for a failed chain), else None.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if n > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("block-tridiagonal Cholesky: blocks of n = %d rows exceed the limit of %d rows per block" % (n, BATCHED_SMALL_MAX))
        L = _lib.lib()
        dev = matrixD.device if isinstance(matrixD, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        info = torch.zeros(max(batch, 1), dtype=torch.int32, device=dev)
        logdet = torch.zeros(max(batch, 1), dtype=torch.float64, device=dev) if want_logdet else None
        st = L.cap_dpotrf_blocktri_batched(int(srcPackage.uplo), n, T, dptr(matrixD), ldd, step_d, stride_d, dptr(matrixE), lde, step_e, stride_e,
                                           info.data_ptr(), logdet.data_ptr() if want_logdet else None, batch, cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrf_blocktri_batched")
        return info[:max(batch, 0)], (logdet[:max(batch, 0)] if want_logdet else None)

    @staticmethod
    def _potrs_blocktri_batched(matrixD, matrixE, matrixB, n, T, nrhs, ldd, step_d, stride_d, lde, step_e, stride_e, ldb, stride_b, batch, info,
                                srcPackage, stream=None):
        """B_c ((T n) x nrhs, ld ldb, at matrixB + c stride_b) <- A_c^-1 B_c with the factors _potrf_blocktri_batched left in matrixD and
        matrixE, n <= 64, in one launch (cap_dpotrs_blocktri_batched).  srcPackage.half = 1: the forward sweep alone (R^-T B), 2: the backward
        sweep alone (R^-1 B).  info: what _potrf_blocktri_batched returned, or None; a chain with info != 0 gets NaN.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if n > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("block-tridiagonal Cholesky: blocks of n = %d rows exceed the limit of %d rows per block" % (n, BATCHED_SMALL_MAX))
        L = _lib.lib()
        st = L.cap_dpotrs_blocktri_batched(int(srcPackage.uplo), int(srcPackage.half), n, T, nrhs, dptr(matrixD), ldd, step_d, stride_d, dptr(matrixE),
                                           lde, step_e, stride_e, dptr(matrixB), ldb, stride_b, engine._batched_info(info, batch), batch,
                                           cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrs_blocktri_batched")

    @staticmethod
    def _potri_blocktri_batched(matrixD, matrixE, n, T, ldd, step_d, stride_d, lde, step_e, stride_e, batch, info, srcPackage, fill=False, stream=None):
        """The factors _potrf_blocktri_batched left in matrixD and matrixE (same addressing, n <= 64) <- the block-tridiagonal part of the
        inverses of the chains, in place, in one launch (cap_dpotri_blocktri_batched): the upper triangle of D_i <- that of Sigma_(i,i), E_i <-
        Sigma_(i,i+1); fill: the strictly lower triangles of the D blocks become the mirror.  info: what _potrf_blocktri_batched returned,
        or None; a chain with info != 0 gets NaN wherever the call writes.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if n > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("block-tridiagonal inverse: blocks of n = %d rows exceed the limit of %d rows per block" % (n, BATCHED_SMALL_MAX))
        L = _lib.lib()
        st = L.cap_dpotri_blocktri_batched(int(srcPackage.uplo), 1 if fill else 0, n, T, dptr(matrixD), ldd, step_d, stride_d, dptr(matrixE), lde,
                                           step_e, stride_e, engine._batched_info(info, batch), batch, cur_stream(stream))
        _lib.check(st, "lapack::engine::_potri_blocktri_batched")

    @staticmethod
    def _potrf_blocktri_vbatched(plan, matrixD, matrixE, n, ldd, step_d, lde, step_e, batch, srcPackage, want_logdet=False, stream=None):
        """The chains of DIFFERENT lengths that `plan` (a cap_blocktri_plan handle) describes inside the slot sequences matrixD / matrixE
        (slot s is column-major with ld ldd at matrixD + s step_d, E likewise; n <= 64) <- their block bidiagonal Cholesky factors, in
        place, in one launch (cap_dpotrf_blocktri_vbatched).  Every chain gets the bits _potrf_blocktri_batched gives for it alone.
        Returns (info, logdet) in batch order as _potrf_blocktri_batched does, info[c] the row inside chain c's own system; the entries of
        empty chains are 0 (the kernel does not write them).  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if n > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("block-tridiagonal Cholesky: blocks of n = %d rows exceed the limit of %d rows per block" % (n, BATCHED_SMALL_MAX))
        L = _lib.lib()
        dev = matrixD.device if isinstance(matrixD, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        info = torch.zeros(max(batch, 1), dtype=torch.int32, device=dev)
        logdet = torch.zeros(max(batch, 1), dtype=torch.float64, device=dev) if want_logdet else None
        st = L.cap_dpotrf_blocktri_vbatched(plan, int(srcPackage.uplo), n, dptr(matrixD), ldd, step_d, dptr(matrixE), lde, step_e, info.data_ptr(),
                                            logdet.data_ptr() if want_logdet else None, cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrf_blocktri_vbatched")
        return info[:max(batch, 0)], (logdet[:max(batch, 0)] if want_logdet else None)

    @staticmethod
    def _potrs_blocktri_vbatched(plan, matrixD, matrixE, matrixB, n, nrhs, ldd, step_d, lde, step_e, ldb, batch, info, srcPackage, stream=None):
        """The stacked right-hand sides matrixB ((n sum T) x nrhs, column-major, ld ldb; chain c owns the rows behind n times the prefix sum
        of T) <- the solutions with the factors _potrf_blocktri_vbatched left, in one launch (cap_dpotrs_blocktri_vbatched); srcPackage.half
        as in _potrs_blocktri_batched.  info: what _potrf_blocktri_vbatched returned, or None; a chain with info != 0 gets NaN.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if n > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("block-tridiagonal Cholesky: blocks of n = %d rows exceed the limit of %d rows per block" % (n, BATCHED_SMALL_MAX))
        L = _lib.lib()
        st = L.cap_dpotrs_blocktri_vbatched(plan, int(srcPackage.uplo), int(srcPackage.half), n, nrhs, dptr(matrixD), ldd, step_d, dptr(matrixE), lde,
                                            step_e, dptr(matrixB), ldb, engine._batched_info(info, batch), cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrs_blocktri_vbatched")

    @staticmethod
    def _potri_blocktri_vbatched(plan, matrixD, matrixE, n, ldd, step_d, lde, step_e, batch, info, srcPackage, fill=False, stream=None):
        """The factors _potrf_blocktri_vbatched left <- the block-tridiagonal part of the inverses of the chains, in place, in one launch
        (cap_dpotri_blocktri_vbatched), as _potri_blocktri_batched does for every chain alone.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        if n > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("block-tridiagonal inverse: blocks of n = %d rows exceed the limit of %d rows per block" % (n, BATCHED_SMALL_MAX))
        L = _lib.lib()
        st = L.cap_dpotri_blocktri_vbatched(plan, int(srcPackage.uplo), 1 if fill else 0, n, dptr(matrixD), ldd, step_d, dptr(matrixE), lde, step_e,
                                            engine._batched_info(info, batch), cur_stream(stream))
        _lib.check(st, "lapack::engine::_potri_blocktri_vbatched")

    @staticmethod
    def _batched_info(info, batch):
        if info is not None and (not isinstance(info, torch.Tensor) or not info.is_cuda or info.dtype != torch.int32
                                 or info.numel() < batch or not info.is_contiguous()):
            raise _lib.CapitalError("info must be a contiguous int32 device tensor of batch entries")
        return info.data_ptr() if info is not None else None

    @staticmethod
    def _trtri_batched(matrixT, n, ldt, stride, batch, info, srcPackage, stream=None):
        """The upper triangles of the n x n blocks (n <= 256, column-major, ld ldt) at matrixT + i stride, i < batch, <- those of their inverses
        (non-unit diagonal), in place, in one launch (cap_dtrtri_batched: n <= 64 a wavefront per block, 64 < n <= 256 a workgroup per block).
        info: what _potrf_batched returned, or None; a block with info != 0 gets NaN in its upper triangle.  A zero on a diagonal is not
        detected.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor or getattr(srcPackage, "diag", Diag.AlapackNonUnit) != Diag.AlapackNonUnit:
            raise _lib.CapitalError("only AlapackColumnMajor / AlapackNonUnit is supported")
        _batched_blocked(None, n)
        L = _lib.lib()
        st = L.cap_dtrtri_batched(int(srcPackage.uplo), n, dptr(matrixT), ldt, stride, batch, engine._batched_info(info, batch), cur_stream(stream))
        _lib.check(st, "lapack::engine::_trtri_batched")

    @staticmethod
    def _potri_batched(matrixR, n, ldr, stride, batch, info, srcPackage, fill=False, stream=None):
        """The upper triangles of the n x n blocks (n <= 256, column-major, ld ldr) at matrixR + i stride, i < batch - the factors R_i
        _potrf_batched left - <- those of A_i^-1 = R_i^-1 R_i^-T, in place, in one launch (cap_dpotri_batched).  fill: the strictly lower
        triangles become the bit-identical mirrors of the upper ones.  info: what _potrf_batched returned, or None; a block with info != 0
        gets NaN wherever the call writes.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        _batched_blocked(None, n)
        L = _lib.lib()
        st = L.cap_dpotri_batched(int(srcPackage.uplo), n, dptr(matrixR), ldr, stride, batch, engine._batched_info(info, batch),
                                  1 if fill else 0, cur_stream(stream))
        _lib.check(st, "lapack::engine::_potri_batched")

    @staticmethod
    def _potrf_vbatched(plan, matrixA, batch, srcPackage, want_logdet=False, stream=None):
        """The blocks of different sizes (n_i <= 256) that `plan` (a cap_vbatch_plan handle) describes inside matrixA <- their upper factors:
        cap_dpotrf_vbatched, one launch per non-empty size class.  Returns (info, logdet) in batch order as _potrf_batched does; the entries of
        empty blocks are 0.  Nothing is read back: asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        dev = matrixA.device if isinstance(matrixA, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        info = torch.zeros(max(batch, 1), dtype=torch.int32, device=dev)
        logdet = torch.zeros(max(batch, 1), dtype=torch.float64, device=dev) if want_logdet else None
        st = L.cap_dpotrf_vbatched(plan, int(srcPackage.uplo), dptr(matrixA), info.data_ptr(), logdet.data_ptr() if want_logdet else None,
                                   cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrf_vbatched")
        return info[:max(batch, 0)], (logdet[:max(batch, 0)] if want_logdet else None)

    @staticmethod
    def _potrs_vbatched(plan, matrixR, matrixB, nrhs, ldb, batch, info, srcPackage, stream=None):
        """The stacked right-hand sides matrixB ((sum n_i) x nrhs, column-major, ld ldb; block i owns the rows behind the prefix sum of n) <-
        the solutions with the factors _potrf_vbatched left in matrixR, n_i <= 256: cap_dpotrs_vbatched.  info: what _potrf_vbatched
        returned, or None; a block with info != 0 gets NaN.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        st = L.cap_dpotrs_vbatched(plan, int(srcPackage.uplo), nrhs, dptr(matrixR), dptr(matrixB), ldb, engine._batched_info(info, batch),
                                   cur_stream(stream))
        _lib.check(st, "lapack::engine::_potrs_vbatched")

    @staticmethod
    def _potri_vbatched(plan, matrixR, batch, info, srcPackage, fill=False, stream=None):
        """The upper triangles of the factors _potrf_vbatched left in matrixR (n_i <= 256) <- those of the inverses A_i^-1: cap_dpotri_vbatched.
        fill: the strictly lower triangles become the bit-identical mirrors.  info: what _potrf_vbatched returned, or None; a block with
        info != 0 gets NaN wherever the call writes.  Asynchronous."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        st = L.cap_dpotri_vbatched(plan, int(srcPackage.uplo), dptr(matrixR), engine._batched_info(info, batch), 1 if fill else 0,
                                   cur_stream(stream))
        _lib.check(st, "lapack::engine::_potri_vbatched")

    @staticmethod
    def _cholupdate_batched(matrixR, matrixV, n, k, ldr, stride_r, ldv, stride_v, batch, sign, info, srcPackage, stream=None):
        """The upper factors R_i (n x n, n <= 256, column-major, ld ldr, at matrixR + i stride_r; what _potrf_batched left) <- the factors of
        R_i^T R_i + sign V_i V_i^T, V_i n x k (ld ldv, at matrixV + i stride_v, not written), sign = +1 / -1, in one launch
        (cap_dcholupdate_batched).  info: a contiguous int32 device tensor of batch entries, read AND written - a block with info != 0 on
        entry is not touched, a downdate that finds its matrix not positive definite leaves the 1-based row there - or None: every block is
        swept and nothing is reported.  Every block gets the bits of _cholupdate on it alone.  Asynchronous; nothing is read back."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        _batched_blocked(None, n)
        L = _lib.lib()
        st = L.cap_dcholupdate_batched(int(srcPackage.uplo), int(sign), n, k, dptr(matrixR), ldr, stride_r, dptr(matrixV), ldv, stride_v, batch,
                                       engine._batched_info(info, batch), cur_stream(stream))
        _lib.check(st, "lapack::engine::_cholupdate_batched")

    @staticmethod
    def _cholupdate_vbatched(plan, matrixR, matrixV, k, ldv, batch, sign, info, srcPackage, stream=None):
        """The factors _potrf_vbatched left in matrixR (n_i <= 256) <- those of R_i^T R_i + sign V_i V_i^T with the stacked matrixV
        ((sum n_i) x k, column-major, ld ldv; block i owns the rows behind the prefix sum of n): cap_dcholupdate_vbatched, one launch per
        non-empty size class.  info as in _cholupdate_batched, batch order; the entries of empty blocks are neither read nor written.
        Asynchronous; nothing is read back."""
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")
        L = _lib.lib()
        st = L.cap_dcholupdate_vbatched(plan, int(srcPackage.uplo), int(sign), k, dptr(matrixR), dptr(matrixV), ldv,
                                        engine._batched_info(info, batch), cur_stream(stream))
        _lib.check(st, "lapack::engine::_cholupdate_vbatched")

    @staticmethod
    def _tri_pack(srcPackage):
        if srcPackage.order != Order.AlapackColumnMajor or getattr(srcPackage, "diag", Diag.AlapackNonUnit) != Diag.AlapackNonUnit:
            raise _lib.CapitalError("only AlapackColumnMajor / AlapackNonUnit is supported")

    @staticmethod
    def _sumsq_ptr(sumsq, batch, nrhs, ldq):
        if sumsq is None:
            return None
        if (not isinstance(sumsq, torch.Tensor) or not sumsq.is_cuda or sumsq.dtype != torch.float64 or not sumsq.is_contiguous()
                or ldq < nrhs or sumsq.numel() < batch * ldq):
            raise _lib.CapitalError("sumsq must be a contiguous fp64 device tensor of batch x ldq entries with ldq >= nrhs")
        return sumsq.data_ptr()

    @staticmethod
    def _trsm_batched(matrixR, matrixB, n, nrhs, ldr, stride_r, ldb, stride_b, batch, trans, info, srcPackage, sumsq=None, ldq=0, stream=None):
        """B_i (n x nrhs, ld ldb, at matrixB + i stride_b) <- R_i^-T B_i (trans) or R_i^-1 B_i (not trans) with the upper triangles R_i at
        matrixR + i stride_r (ld ldr; what _potrf_batched left), n <= 256, in one launch (cap_dtrsm_batched).  info: what _potrf_batched
        returned, or None; a block with info != 0 gets NaN.  sumsq: None, or a contiguous fp64 device tensor of batch x ldq entries
        (ldq >= nrhs) that receives the sums of squares of the result's columns, computed in the same launch.  Asynchronous."""
        engine._tri_pack(srcPackage)
        _batched_blocked(None, n)
        q = engine._sumsq_ptr(sumsq, batch, nrhs, ldq)
        L = _lib.lib()
        st = L.cap_dtrsm_batched(int(srcPackage.uplo), 1 if trans else 0, n, nrhs, dptr(matrixR), ldr, stride_r, dptr(matrixB), ldb, stride_b,
                                 batch, engine._batched_info(info, batch), q, ldq, cur_stream(stream))
        _lib.check(st, "lapack::engine::_trsm_batched")

    @staticmethod
    def _trmm_batched(matrixR, matrixB, n, nrhs, ldr, stride_r, ldb, stride_b, batch, trans, info, srcPackage, stream=None):
        """B_i <- R_i^T B_i (trans) or R_i B_i (not trans); arguments and layout as in _trsm_batched, n <= 256, one launch
        (cap_dtrmm_batched).  A block with info != 0 gets NaN.  Asynchronous."""
        engine._tri_pack(srcPackage)
        _batched_blocked(None, n)
        L = _lib.lib()
        st = L.cap_dtrmm_batched(int(srcPackage.uplo), 1 if trans else 0, n, nrhs, dptr(matrixR), ldr, stride_r, dptr(matrixB), ldb, stride_b,
                                 batch, engine._batched_info(info, batch), cur_stream(stream))
        _lib.check(st, "lapack::engine::_trmm_batched")

    @staticmethod
    def _trsm_vbatched(plan, matrixR, matrixB, nrhs, ldb, batch, trans, info, srcPackage, sumsq=None, ldq=0, stream=None):
        """The stacked right-hand sides matrixB ((sum n_i) x nrhs, ld ldb) <- R_i^-T B_i (trans) or R_i^-1 B_i block by block with the
        factors _potrf_vbatched left in matrixR (n_i <= 256; a plan refuses larger blocks when it is made): cap_dtrsm_vbatched, one launch
        per non-empty size class.  info, sumsq (batch x ldq, batch order; rows of empty blocks are not written) as in _trsm_batched.
        Asynchronous."""
        engine._tri_pack(srcPackage)
        q = engine._sumsq_ptr(sumsq, batch, nrhs, ldq)
        L = _lib.lib()
        st = L.cap_dtrsm_vbatched(plan, int(srcPackage.uplo), 1 if trans else 0, nrhs, dptr(matrixR), dptr(matrixB), ldb,
                                  engine._batched_info(info, batch), q, ldq, cur_stream(stream))
        _lib.check(st, "lapack::engine::_trsm_vbatched")

    @staticmethod
    def _trmm_vbatched(plan, matrixR, matrixB, nrhs, ldb, batch, trans, info, srcPackage, stream=None):
        """The stacked matrixB <- R_i^T B_i (trans) or R_i B_i block by block (n_i <= 256; a plan refuses larger blocks when it is made):
        cap_dtrmm_vbatched, one launch per non-empty size class.  Asynchronous."""
        engine._tri_pack(srcPackage)
        L = _lib.lib()
        st = L.cap_dtrmm_vbatched(plan, int(srcPackage.uplo), 1 if trans else 0, nrhs, dptr(matrixR), dptr(matrixB), ldb,
                                  engine._batched_info(info, batch), cur_stream(stream))
        _lib.check(st, "lapack::engine::_trmm_vbatched")

    @staticmethod
    def _colmajor(srcPackage):
        if srcPackage.order != Order.AlapackColumnMajor:
            raise _lib.CapitalError("only AlapackColumnMajor is supported")

    @staticmethod
    def _out_ptr(t, count, name):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < count:
            raise _lib.CapitalError("%s must be a contiguous fp64 device tensor of at least %d entries" % (name, count))
        return t.data_ptr()

    @staticmethod
    def _lansy_batched(matrixA, n, lda, stride_a, batch, out, srcPackage, stream=None):
        """out[i] <- the 1-norm (norm '1' / 'O' / 'I' of the ArgPack: one number for a symmetric matrix) of the symmetric n x n blocks
        (n <= 256) whose upper triangles lie at matrixA + i stride_a (column-major, ld lda), in one launch (cap_dlansy_batched).  out: a
        contiguous fp64 device tensor of batch entries.  A NaN in a triangle gives NaN.  Asynchronous."""
        engine._colmajor(srcPackage)
        _batched_blocked(None, n)
        st = _lib.lib().cap_dlansy_batched(ord(str(srcPackage.norm)[0]), int(srcPackage.uplo), n, dptr(matrixA), lda, stride_a, batch,
                                           engine._out_ptr(out, batch, "out"), cur_stream(stream))
        _lib.check(st, "lapack::engine::_lansy_batched")

    @staticmethod
    def _lansy_vbatched(plan, matrixA, batch, out, srcPackage, stream=None):
        """The same for the blocks of a cap_vbatch_plan (n_i <= 256; a plan refuses larger blocks when it is made) inside the flat matrixA:
        cap_dlansy_vbatched, one launch per non-empty size class; out in batch order, the entries of empty blocks are not written.
        Asynchronous."""
        engine._colmajor(srcPackage)
        st = _lib.lib().cap_dlansy_vbatched(plan, ord(str(srcPackage.norm)[0]), int(srcPackage.uplo), dptr(matrixA),
                                            engine._out_ptr(out, batch, "out"), cur_stream(stream))
        _lib.check(st, "lapack::engine::_lansy_vbatched")

    @staticmethod
    def _pocon_batched(matrixR, n, ldr, stride_r, batch, anorm, info, rcond, srcPackage, stream=None):
        """rcond[i] <- 1 / (anorm[i] * |A_i^-1|_1) with the COMPUTED inverse of every block, from the factors _potrf_batched left at
        matrixR + i stride_r (n <= 256; not written): cap_dpocon_batched, four launches whatever the batch.  anorm, rcond: contiguous fp64
        device tensors of batch entries; info: what _potrf_batched returned, or None - a failed block gets NaN.  The work tensor is
        allocated here.  Asynchronous."""
        engine._colmajor(srcPackage)
        _batched_blocked(None, n)
        L = _lib.lib()
        work = scratch(L.cap_dpocon_batched_work_size(n, batch), rcond)
        st = L.cap_dpocon_batched(int(srcPackage.uplo), n, dptr(matrixR), ldr, stride_r, batch, engine._out_ptr(anorm, batch, "anorm"),
                                  engine._batched_info(info, batch), engine._out_ptr(rcond, batch, "rcond"), dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_pocon_batched")

    @staticmethod
    def _pocon_vbatched(plan, matrixR, batch, anorm, info, rcond, srcPackage, stream=None):
        """The same for the blocks of a cap_vbatch_plan (n_i <= 256; a plan refuses larger blocks when it is made): cap_dpocon_vbatched, three
        launches per non-empty size class plus one; the entries of empty blocks are not written.  Asynchronous."""
        engine._colmajor(srcPackage)
        L = _lib.lib()
        work = scratch(L.cap_dpocon_vbatched_work_size(plan), rcond)
        st = L.cap_dpocon_vbatched(plan, int(srcPackage.uplo), dptr(matrixR), engine._out_ptr(anorm, batch, "anorm"),
                                   engine._batched_info(info, batch), engine._out_ptr(rcond, batch, "rcond"), dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_pocon_vbatched")

    @staticmethod
    def _poerr_batched(matrixA, matrixR, matrixB, matrixX, n, nrhs, lda, stride_a, ldr, stride_r, ldb, stride_b, ldx, stride_x, batch, info,
                       ferr, berr, lde, srcPackage, stream=None):
        """The bounds of LAPACK's dporfs for the solutions X_i of A_i X = B_i, n <= 256: berr[i lde + j] the componentwise backward error,
        ferr[i lde + j] the forward error bound | |A_i^-1| w_j |_inf / |x_j|_inf with the COMPUTED inverse (cap_dpoerr_batched; one launch
        for berr alone, four with ferr).  matrixA: the blocks before the factorization (upper triangles), matrixR: their factors; nothing is
        written but ferr / berr (contiguous fp64 device tensors of batch x lde entries, either may be None).  A block with info != 0 gets
        NaN.  The work tensor is allocated here.  Asynchronous."""
        engine._colmajor(srcPackage)
        _batched_blocked(None, n)
        L = _lib.lib()
        work = scratch(L.cap_dpoerr_batched_work_size(n, nrhs, batch), matrixX) if ferr is not None else None
        st = L.cap_dpoerr_batched(int(srcPackage.uplo), n, nrhs, dptr(matrixA), lda, stride_a, dptr(matrixR), ldr, stride_r, dptr(matrixB), ldb,
                                  stride_b, dptr(matrixX), ldx, stride_x, batch, engine._batched_info(info, batch),
                                  engine._out_ptr(ferr, batch * lde, "ferr"), engine._out_ptr(berr, batch * lde, "berr"), lde, dptr(work),
                                  cur_stream(stream))
        _lib.check(st, "lapack::engine::_poerr_batched")

    @staticmethod
    def _poerr_vbatched(plan, matrixA, matrixR, matrixB, matrixX, nrhs, ldb, ldx, batch, info, ferr, berr, lde, srcPackage, stream=None):
        """The same for the blocks of a cap_vbatch_plan (n_i <= 256; a plan refuses larger blocks when it is made) with the stacked matrixB /
        matrixX of _potrs_vbatched: cap_dpoerr_vbatched, one launch per non-empty size class for berr alone, four with ferr; the rows of
        empty blocks are not written.  Asynchronous."""
        engine._colmajor(srcPackage)
        L = _lib.lib()
        work = scratch(L.cap_dpoerr_vbatched_work_size(plan, nrhs), matrixX) if ferr is not None else None
        st = L.cap_dpoerr_vbatched(plan, int(srcPackage.uplo), nrhs, dptr(matrixA), dptr(matrixR), dptr(matrixB), ldb, dptr(matrixX), ldx,
                                   engine._batched_info(info, batch), engine._out_ptr(ferr, batch * lde, "ferr"),
                                   engine._out_ptr(berr, batch * lde, "berr"), lde, dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_poerr_vbatched")

    @staticmethod
    def _pstrf_outputs(matrixA, matrixR, piv, count, batch, want_logdet):
        """the checks and the zeroed per-block result tensors the two pivoted entries share: (rank, resid, info, logdet)"""
        if not isinstance(matrixA, torch.Tensor) or not matrixA.is_cuda or matrixA.dtype != torch.float64:
            raise _lib.CapitalError("matrixA must be an fp64 device tensor - there is no CPU path")
        if matrixR is not None:
            if not isinstance(matrixR, torch.Tensor) or not matrixR.is_cuda or matrixR.dtype != torch.float64 or matrixR.device != matrixA.device:
                raise _lib.CapitalError("matrixR must be an fp64 device tensor on matrixA's device")
            if matrixA.numel() > 0 and matrixR.numel() > 0:
                span = lambda t: (t.data_ptr(), t.data_ptr() + 8 * (sum((d - 1) * abs(s) for d, s in zip(t.shape, t.stride())) + 1))
                (a0, a1), (r0, r1) = span(matrixA), span(matrixR)
                if a0 < r1 and r0 < a1:
                    raise _lib.CapitalError("matrixR overlaps matrixA")
        if (not isinstance(piv, torch.Tensor) or not piv.is_cuda or piv.dtype != torch.int64 or piv.numel() < count or not piv.is_contiguous()
                or piv.device != matrixA.device):
            raise _lib.CapitalError("piv must be a contiguous int64 device tensor of %d entries on matrixA's device" % count)
        dev = matrixA.device
        rank = torch.zeros(max(batch, 1), dtype=torch.int32, device=dev)
        info = torch.zeros(max(batch, 1), dtype=torch.int32, device=dev)
        resid = torch.zeros(max(batch, 1), dtype=torch.float64, device=dev)
        logdet = torch.zeros(max(batch, 1), dtype=torch.float64, device=dev) if want_logdet else None
        return rank, resid, info, logdet

    @staticmethod
    def _pstrf_batched(matrixA, matrixR, piv, n, max_rank, lda, stride_a, ldr, stride_r, batch, tol, srcPackage, want_logdet=False, stream=None):
        """Pivoted Cholesky of the symmetric positive semidefinite n x n blocks (n <= 64, column-major, ld lda; upper triangles read, nothing
        of them written) at matrixA + i stride_a, i < batch, in at most max_rank steps each, in one launch (cap_dpstrf_batched):
        A_i[piv_i][:, piv_i] ~ R_i^T R_i with R_i max_rank x n (ld ldr) at matrixR + i stride_r and piv a contiguous int64 device tensor of
        batch n entries.  tol < 0: n eps max_i a_ii per block, otherwise absolute.  matrixR must not overlap matrixA.  Returns
        (rank, resid, info, logdet): int32 / fp64 / int32 device tensors of batch entries and, with want_logdet, the fp64
        pseudo-log-determinants 2 sum_{j < rank} log r_jj (else None).  info is 0 / 1 / 2 as for _pstrf - stopped at a pivot <= tol, the
        cap was hit, a NaN on the remaining diagonal - NOT the info _potrs_batched, _trsm_batched or _trmm_batched expect.  Blocks above
        64 rows: cholinv.factor_pivoted, one block at a time.  Nothing is read back: asynchronous."""
        engine._colmajor(srcPackage)
        if n > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("the batched pivoted factorization handles blocks of up to %d rows, got n = %d - use "
                                    "cholinv.factor_pivoted on each block" % (BATCHED_SMALL_MAX, n))
        rank, resid, info, logdet = engine._pstrf_outputs(matrixA, matrixR, piv, batch * n, batch, want_logdet)
        st = _lib.lib().cap_dpstrf_batched(int(srcPackage.uplo), n, max_rank, float(tol), dptr(matrixA), lda, stride_a, dptr(matrixR), ldr,
                                           stride_r, piv.data_ptr(), rank.data_ptr(), resid.data_ptr(),
                                           logdet.data_ptr() if want_logdet else None, info.data_ptr(), batch, cur_stream(stream))
        _lib.check(st, "lapack::engine::_pstrf_batched")
        cut = lambda t: None if t is None else t[:max(batch, 0)]
        return cut(rank), cut(resid), cut(info), cut(logdet)

    @staticmethod
    def _pstrf_vbatched(plan, matrixA, matrixR, piv, rows, nmax, max_rank, batch, tol, srcPackage, want_logdet=False, stream=None):
        """The same for the blocks of a cap_vbatch_plan whose largest block has at most 64 rows (nmax: the plan's largest n; rows: sum n_i):
        cap_dpstrf_vbatched, one launch per non-empty size class.  matrixA, matrixR: two flat tensors in the plan's layout - matrixR gets
        every entry of every n_i x n_i block, the cap of block i is min(max_rank, n_i); piv: the stacked int64 vector of `rows` block-local
        indices.  Returns (rank, resid, info, logdet) in batch order as _pstrf_batched does; the entries of empty blocks are 0.  Blocks above
        64 rows: cholinv.factor_pivoted.  Asynchronous."""
        engine._colmajor(srcPackage)
        if nmax > BATCHED_SMALL_MAX:
            raise _lib.CapitalError("the batched pivoted factorization handles blocks of up to %d rows, the plan's largest has %d - use "
                                    "cholinv.factor_pivoted on each block" % (BATCHED_SMALL_MAX, nmax))
        rank, resid, info, logdet = engine._pstrf_outputs(matrixA, matrixR, piv, rows, batch, want_logdet)
        st = _lib.lib().cap_dpstrf_vbatched(plan, int(srcPackage.uplo), max_rank, float(tol), dptr(matrixA), dptr(matrixR), piv.data_ptr(),
                                            rank.data_ptr(), resid.data_ptr(), logdet.data_ptr() if want_logdet else None, info.data_ptr(),
                                            cur_stream(stream))
        _lib.check(st, "lapack::engine::_pstrf_vbatched")
        cut = lambda t: None if t is None else t[:max(batch, 0)]
        return cut(rank), cut(resid), cut(info), cut(logdet)

    @staticmethod
    def _trtri(matrixA, n, lda, srcPackage, stream=None):
        if srcPackage.order != Order.AlapackColumnMajor or srcPackage.diag != Diag.AlapackNonUnit:
            raise _lib.CapitalError("only AlapackColumnMajor / AlapackNonUnit is supported")
        L = _lib.lib()
        work = scratch(L.cap_dtrtri_work_size(n), matrixA)
        st = L.cap_dtrtri(int(srcPackage.uplo), n, dptr(matrixA), lda, dptr(work), cur_stream(stream))
        _lib.check(st, "lapack::engine::_trtri")
