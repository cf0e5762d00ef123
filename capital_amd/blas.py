"""blas::engine mirror (reference src/blas/engine.h:23-130, src/blas/interface.h:58-66).

Same enum names / values and ArgPack fields as upstream; the engine methods take DEVICE
buffers (torch tensors or raw device addresses) and run the hand-written MFMA kernels of
libcapital_amd.so.  No CPU path: missing library or non-device pointers fail loudly."""
import enum

import torch

from . import _lib
from ._util import dptr, cur_stream, scratch


class Order(enum.IntEnum):
    AblasRowMajor = 0x0
    AblasColumnMajor = 0x1


class Transpose(enum.IntEnum):
    AblasNoTrans = 0x0
    AblasTrans = 0x1


class Side(enum.IntEnum):
    AblasLeft = 0x0
    AblasRight = 0x1


class UpLo(enum.IntEnum):
    AblasLower = 0x0
    AblasUpper = 0x1


class Diag(enum.IntEnum):
    AblasNonUnit = 0x0
    AblasUnit = 0x1


class Method(enum.IntEnum):
    AblasGemm = 0x0
    AblasTrmm = 0x1
    AblasSyrk = 0x10
    AblasSymm = 0x11            # extension: not in the reference's enum


class ArgPack_gemm:
    def __init__(self, order, transposeA, transposeB, alpha, beta):
        self.method = Method.AblasGemm
        self.order, self.transposeA, self.transposeB = Order(order), Transpose(transposeA), Transpose(transposeB)
        self.alpha, self.beta = float(alpha), float(beta)


class ArgPack_trmm:
    def __init__(self, order, side, uplo, transposeA, diag, alpha):
        self.method = Method.AblasTrmm
        self.order, self.side, self.uplo = Order(order), Side(side), UpLo(uplo)
        self.transposeA, self.diag, self.alpha = Transpose(transposeA), Diag(diag), float(alpha)


class ArgPack_syrk:
    def __init__(self, order, uplo, transposeA, alpha, beta):
        self.method = Method.AblasSyrk
        self.order, self.uplo, self.transposeA = Order(order), UpLo(uplo), Transpose(transposeA)
        self.alpha, self.beta = float(alpha), float(beta)


class ArgPack_symm:
    def __init__(self, order, uplo, alpha, beta, absolute=False):
        self.method = Method.AblasSymm
        self.order, self.uplo = Order(order), UpLo(uplo)
        self.alpha, self.beta, self.absolute = float(alpha), float(beta), bool(absolute)


def _require_colmajor(order):
    if Order(order) != Order.AblasColumnMajor:
        raise _lib.CapitalError("only AblasColumnMajor is supported (every upstream call site uses it)")


class engine:
    """Static methods with upstream's signatures (blas/interface.h:58-66)."""

    @staticmethod
    def _gemm(matrixA, matrixB, matrixC, m, n, k, lda, ldb, ldc, srcPackage, stream=None):
        _require_colmajor(srcPackage.order)
        st = _lib.lib().cap_dgemm(int(srcPackage.transposeA), int(srcPackage.transposeB), m, n, k, srcPackage.alpha,
                                  dptr(matrixA), lda, dptr(matrixB), ldb, srcPackage.beta, dptr(matrixC), ldc,
                                  cur_stream(stream))
        _lib.check(st, "blas::engine::_gemm")

    @staticmethod
    def _trmm(matrixA, matrixB, m, n, lda, ldb, srcPackage, stream=None):
        _require_colmajor(srcPackage.order)
        L = _lib.lib()
        work = scratch(L.cap_dtrmm_work_size(int(srcPackage.side), m, n), matrixB)
        st = L.cap_dtrmm(int(srcPackage.side), int(srcPackage.uplo), int(srcPackage.transposeA), int(srcPackage.diag), m, n,
                         srcPackage.alpha, dptr(matrixA), lda, dptr(matrixB), ldb, dptr(work), cur_stream(stream))
        _lib.check(st, "blas::engine::_trmm")

    @staticmethod
    def _syrk(matrixA, matrixC, n, k, lda, ldc, srcPackage, stream=None):
        _require_colmajor(srcPackage.order)
        st = _lib.lib().cap_dsyrk(int(srcPackage.uplo), int(srcPackage.transposeA), n, k, srcPackage.alpha, dptr(matrixA), lda,
                                  srcPackage.beta, dptr(matrixC), ldc, cur_stream(stream))
        _lib.check(st, "blas::engine::_syrk")

    @staticmethod
    def _shift_ptr(shift, batch):
        if shift is None:
            return None
        if (not isinstance(shift, torch.Tensor) or not shift.is_cuda or shift.dtype != torch.float64 or not shift.is_contiguous()
                or shift.numel() < batch):
            raise _lib.CapitalError("shift must be a contiguous fp64 device tensor of batch entries")
        return shift.data_ptr()

    @staticmethod
    def _syrk_batched(matrixV, matrixC, n, k, ldv, stride_v, ldc, stride_c, batch, srcPackage, shift=None, fill=False, stream=None):
        """The upper triangle of every column-major n x n block C_i (matrixC + i stride_c, ld ldc) <- beta C_i + alpha op(V_i) op(V_i)^T
        (+ shift[i] I), n <= 256, any k, in one launch (cap_dsyrk_batched).  AblasNoTrans: V_i is n x k (ld ldv >= n) at matrixV + i stride_v;
        AblasTrans: V_i is k x n (ld ldv >= k) and C = alpha V^T V + beta C.  alpha, beta, uplo and transposeA come from the ArgPack_syrk.
        shift: None, or a contiguous fp64 device tensor of batch entries; fill: the strictly lower triangle becomes the bit-identical
        mirror.  beta == 0 does not read C.  Asynchronous."""
        _require_colmajor(srcPackage.order)
        if n > 256:
            raise _lib.CapitalError("_syrk_batched takes blocks of at most 256 rows, got n = %d" % n)
        st = _lib.lib().cap_dsyrk_batched(int(srcPackage.uplo), int(srcPackage.transposeA), n, k, srcPackage.alpha, dptr(matrixV), ldv, stride_v,
                                          srcPackage.beta, dptr(matrixC), ldc, stride_c, engine._shift_ptr(shift, batch), 1 if fill else 0, batch,
                                          cur_stream(stream))
        _lib.check(st, "blas::engine::_syrk_batched")

    @staticmethod
    def _syrk_vbatched(plan, matrixV, matrixC, k, ldv, batch, srcPackage, shift=None, fill=False, stream=None):
        """The same for the blocks of a cap_vbatch_plan (n_i <= 256; a plan refuses larger blocks when it is made): matrixC is the flat tensor
        of the plan, matrixV the stacked (sum n_i) x k matrix (AblasNoTrans, ldv >= sum n_i) or the k x (sum n_i) one (AblasTrans,
        ldv >= k); shift in batch order.  cap_dsyrk_vbatched, one launch per non-empty size class.  Asynchronous."""
        _require_colmajor(srcPackage.order)
        st = _lib.lib().cap_dsyrk_vbatched(plan, int(srcPackage.uplo), int(srcPackage.transposeA), k, srcPackage.alpha, dptr(matrixV), ldv,
                                           srcPackage.beta, dptr(matrixC), engine._shift_ptr(shift, batch), 1 if fill else 0, cur_stream(stream))
        _lib.check(st, "blas::engine::_syrk_vbatched")

    @staticmethod
    def _gemm_batched(matrixA, matrixB, matrixC, m, n, k, lda, stride_a, ldb, stride_b, ldc, stride_c, batch, srcPackage, stream=None):
        """Every column-major m x n block C_i (matrixC + i stride_c, ld ldc) <- beta C_i + alpha op(A_i) op(B_i), m, n <= 256, any k, in one
        launch (cap_dgemm_batched).  op(A_i) is m x k: AblasNoTrans - A_i is m x k (ld lda >= m) at matrixA + i stride_a, AblasTrans - k x m
        (lda >= k); op(B_i) is k x n likewise.  alpha, beta and the two transposes come from the ArgPack_gemm.  beta == 0 does not read C;
        alpha == 0 or k == 0 does not read A or B (they may be None).  C must not overlap A or B.  Asynchronous."""
        _require_colmajor(srcPackage.order)
        if m > 256 or n > 256:
            raise _lib.CapitalError("_gemm_batched takes blocks of at most 256 rows and columns, got m = %d, n = %d" % (m, n))
        st = _lib.lib().cap_dgemm_batched(int(srcPackage.transposeA), int(srcPackage.transposeB), m, n, k, srcPackage.alpha, dptr(matrixA), lda,
                                          stride_a, dptr(matrixB), ldb, stride_b, srcPackage.beta, dptr(matrixC), ldc, stride_c, batch,
                                          cur_stream(stream))
        _lib.check(st, "blas::engine::_gemm_batched")

    @staticmethod
    def _gemm_vbatched_inner(plan, matrixX, matrixY, matrixG, m, n, ldx, ldy, ldg, stride_g, srcPackage, stream=None):
        """On a cap_vbatch_plan: G_i (m x n at matrixG + i stride_g, ld ldg, batch order) <- beta G_i + alpha X_i^T Y_i, m, n <= 256, with
        the stacked (sum n_i) x m matrixX and (sum n_i) x n matrixY of _potrs_vbatched: the contraction runs over the n_i rows of block i.
        cap_dgemm_vbatched_inner, ONE launch whatever the size classes; an empty block gives beta G_i.  The transposes of the ArgPack_gemm
        must be (AblasTrans, AblasNoTrans).  Asynchronous."""
        _require_colmajor(srcPackage.order)
        if (srcPackage.transposeA, srcPackage.transposeB) != (Transpose.AblasTrans, Transpose.AblasNoTrans):
            raise _lib.CapitalError("_gemm_vbatched_inner computes X^T Y: the ArgPack_gemm must say (AblasTrans, AblasNoTrans)")
        if m > 256 or n > 256:
            raise _lib.CapitalError("_gemm_vbatched_inner takes outputs of at most 256 rows and columns, got m = %d, n = %d" % (m, n))
        st = _lib.lib().cap_dgemm_vbatched_inner(plan, m, n, srcPackage.alpha, dptr(matrixX), ldx, dptr(matrixY), ldy, srcPackage.beta,
                                                 dptr(matrixG), ldg, stride_g, cur_stream(stream))
        _lib.check(st, "blas::engine::_gemm_vbatched_inner")

    @staticmethod
    def _gemm_vbatched_combine(plan, matrixV, matrixZ, matrixC, nrhs, k, ldv, ldz, stride_z, ldc, srcPackage, stream=None):
        """On a cap_vbatch_plan: block i's rows of the stacked (sum n_i) x nrhs matrixC (ld ldc) <- beta C_i + alpha V_i Z_i, nrhs <= 256, any
        k, with the stacked (sum n_i) x k matrixV of _cholupdate_vbatched and Z_i k x nrhs (ld ldz >= k) at matrixZ + i stride_z.
        cap_dgemm_vbatched_combine, one launch per non-empty size class.  The transposes of the ArgPack_gemm must be (AblasNoTrans,
        AblasNoTrans).  Asynchronous."""
        _require_colmajor(srcPackage.order)
        if (srcPackage.transposeA, srcPackage.transposeB) != (Transpose.AblasNoTrans, Transpose.AblasNoTrans):
            raise _lib.CapitalError("_gemm_vbatched_combine computes V Z: the ArgPack_gemm must say (AblasNoTrans, AblasNoTrans)")
        if nrhs > 256:
            raise _lib.CapitalError("_gemm_vbatched_combine takes at most 256 columns, got nrhs = %d" % nrhs)
        st = _lib.lib().cap_dgemm_vbatched_combine(plan, nrhs, k, srcPackage.alpha, dptr(matrixV), ldv, dptr(matrixZ), ldz, stride_z,
                                                   srcPackage.beta, dptr(matrixC), ldc, cur_stream(stream))
        _lib.check(st, "blas::engine::_gemm_vbatched_combine")

    @staticmethod
    def _symm_batched(matrixA, matrixX, matrixB, matrixY, n, nrhs, lda, stride_a, ldx, stride_x, ldb, stride_b, ldy, stride_y, batch, srcPackage,
                      stream=None):
        """Y_i (n x nrhs, ld ldy, at matrixY + i stride_y) <- beta B_i + alpha A_i X_i with the SYMMETRIC n x n blocks A_i of which only the
        upper triangle of the column-major block at matrixA + i stride_a (ld lda) is read, n <= 256, any nrhs, in one launch
        (cap_dsymm_batched).  alpha, beta, uplo and absolute (|.| of every element of A, X and B on load) come from the ArgPack_symm.
        beta == 0 does not read B (matrixB may be None); matrixY may be matrixB, it must not overlap A or X.  Asynchronous."""
        _require_colmajor(srcPackage.order)
        if n > 256:
            raise _lib.CapitalError("_symm_batched takes blocks of at most 256 rows, got n = %d" % n)
        st = _lib.lib().cap_dsymm_batched(int(srcPackage.uplo), 1 if srcPackage.absolute else 0, n, nrhs, srcPackage.alpha, dptr(matrixA), lda,
                                          stride_a, dptr(matrixX), ldx, stride_x, srcPackage.beta, dptr(matrixB), ldb, stride_b, dptr(matrixY),
                                          ldy, stride_y, batch, cur_stream(stream))
        _lib.check(st, "blas::engine::_symm_batched")

    @staticmethod
    def _symm_vbatched(plan, matrixA, matrixX, matrixB, matrixY, nrhs, ldx, ldb, ldy, srcPackage, stream=None):
        """The same for the blocks of a cap_vbatch_plan (n_i <= 256; a plan refuses larger blocks when it is made): matrixA is the flat tensor
        of the plan, matrixX / matrixB / matrixY the stacked (sum n_i) x nrhs systems of _potrs_vbatched.  cap_dsymm_vbatched, one launch
        per non-empty size class.  Asynchronous."""
        _require_colmajor(srcPackage.order)
        st = _lib.lib().cap_dsymm_vbatched(plan, int(srcPackage.uplo), 1 if srcPackage.absolute else 0, nrhs, srcPackage.alpha, dptr(matrixA),
                                           dptr(matrixX), ldx, srcPackage.beta, dptr(matrixB), ldb, dptr(matrixY), ldy, cur_stream(stream))
        _lib.check(st, "blas::engine::_symm_vbatched")

    @staticmethod
    def _trsm(matrixA, matrixB, m, n, lda, ldb, srcPackage, stream=None):
        """Real triangular solve (upstream stubs it: trsm/diaginvert/diaginvert.hpp:7-10). Takes an ArgPack_trmm."""
        _require_colmajor(srcPackage.order)
        L = _lib.lib()
        work = scratch(L.cap_dtrsm_work_size(int(srcPackage.side), m, n), matrixB)
        st = L.cap_dtrsm(int(srcPackage.side), int(srcPackage.uplo), int(srcPackage.transposeA), m, n, srcPackage.alpha,
                         dptr(matrixA), lda, dptr(matrixB), ldb, dptr(work), cur_stream(stream))
        _lib.check(st, "blas::engine::_trsm")
