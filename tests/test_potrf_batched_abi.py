"""CPU-only: argument handling of the batched factor and solve (cap_dpotrf_batched, cap_dpotrs_batched) - every case here is decided
before the library touches a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, UNSUPPORTED = 0, 1, 4


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


A = C.c_void_p(1 << 20)                  # never dereferenced: every call below returns before any device work
B = C.c_void_p(1 << 30)
INFO, LOGDET = C.c_void_p(1 << 31), C.c_void_p(1 << 32)


def test_factor_arguments_are_checked_first(L):
    n, batch = 10, 5

    def call(uplo=UPPER, n=n, A=A, lda=n, stride=n * n, batch=batch, info=INFO, logdet=LOGDET):
        return L.cap_dpotrf_batched(uplo, n, A, lda, stride, batch, info, logdet, None)

    assert call(n=-1) == ARG
    assert call(batch=-1) == ARG
    assert call(A=None) == ARG
    assert call(lda=n - 1, stride=n * n) == ARG
    assert call(stride=n * n - 1) == ARG
    assert call(lda=n + 2, stride=(n + 2) * n - 1) == ARG
    assert call(stride=-1) == ARG
    assert call(n=65, lda=65, stride=65 * 65) == UNSUPPORTED
    assert call(n=65, lda=64, stride=65 * 65) == ARG               # the argument rules come first
    assert call(n=1 << 20, lda=1 << 20, stride=1 << 40) == UNSUPPORTED
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, n=0, lda=0, stride=0) == UNSUPPORTED   # as cap_dpstrf: LOWER is refused before the empty case
    assert call(uplo=LOWER, lda=n - 1) == ARG
    assert call(uplo=LOWER, A=None) == ARG
    # degenerate sizes: nothing is launched, whatever the pointers
    assert call(n=0, A=None, lda=0, stride=0, info=None, logdet=None) == OK
    assert call(n=0) == OK
    assert call(batch=0, A=None, info=None, logdet=None) == OK
    assert call(batch=0, stride=0) == OK
    assert call(n=0, batch=0, A=None, lda=0, stride=0) == OK
    assert call(n=65, lda=65, stride=0, batch=0) == UNSUPPORTED    # n > 64 is refused for an empty batch too
    # a single block needs no stride; a NULL pointer with nothing to address is fine
    assert call(batch=0, A=None, stride=-5) == OK


def test_solve_arguments_are_checked_first(L):
    n, nrhs, batch = 10, 3, 5

    def call(uplo=UPPER, n=n, nrhs=nrhs, R=A, ldr=n, stride_r=n * n, B=B, ldb=n, stride_b=n * nrhs, batch=batch, info=INFO):
        return L.cap_dpotrs_batched(uplo, n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, None)

    assert call(n=-1) == ARG
    assert call(batch=-1) == ARG
    assert call(nrhs=-1) == ARG
    assert call(R=None) == ARG
    assert call(B=None) == ARG
    assert call(ldr=n - 1) == ARG
    assert call(ldb=n - 1) == ARG
    assert call(stride_r=n * n - 1) == ARG
    assert call(stride_b=n * nrhs - 1) == ARG
    assert call(ldb=n + 1, stride_b=(n + 1) * nrhs - 1) == ARG
    assert call(n=65, ldr=65, stride_r=65 * 65, ldb=65, stride_b=65 * nrhs) == UNSUPPORTED
    assert call(n=65, ldr=65, stride_r=65 * 65, ldb=64, stride_b=65 * nrhs) == ARG
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, nrhs=0, stride_b=0) == UNSUPPORTED
    assert call(uplo=LOWER, ldr=n - 1) == ARG
    assert call(n=0, R=None, ldr=0, stride_r=0, B=None, ldb=0, stride_b=0, info=None) == OK
    assert call(batch=0, R=None, B=None, info=None) == OK
    assert call(nrhs=0, stride_b=0) == OK
    assert call(nrhs=0, stride_b=0, info=None) == OK


def test_single_block_needs_no_stride(L):
    """batch = 1: the strides are not used and not checked - decided before any device call, so only the status of the refusals around it is
    observable without a device: batch = 2 with the same strides is refused"""
    n, nrhs = 4, 2
    assert L.cap_dpotrf_batched(UPPER, n, A, n, 0, 2, None, None, None) == ARG
    assert L.cap_dpotrs_batched(UPPER, n, nrhs, A, n, 0, B, n, n * nrhs, 2, None, None) == ARG
    assert L.cap_dpotrs_batched(UPPER, n, nrhs, A, n, n * n, B, n, 0, 2, None, None) == ARG
    assert L.cap_dpotrf_batched(LOWER, n, A, n, 0, 1, None, None, None) == UNSUPPORTED      # passes the argument rules with stride 0 ...
    assert L.cap_dpotrf_batched(LOWER, n, A, n, 0, 2, None, None, None) == ARG              # ... which two blocks do not


def test_the_stride_rule_does_not_wrap(L):
    """ld * columns beyond int64 (2^60 * 16 = 2^64 wraps to 0): the stride rule compares with the clipped product, so two blocks at stride 0
    are refused like any other overlap - decided before any device work"""
    big = 1 << 60
    assert L.cap_dpotrf_batched(UPPER, 16, A, big, 0, 2, None, None, None) == ARG
    assert L.cap_dpotrs_batched(UPPER, 16, 16, A, big, 0, B, 16, 16 * 16, 2, None, None) == ARG
    assert L.cap_dpotrs_batched(UPPER, 16, 16, A, 16, 16 * 16, B, big, 0, 2, None, None) == ARG


def test_python_layer_names():
    from capital_amd import batched, lapack
    assert lapack.Method.AlapackPotrfBatched == 0x9 and lapack.Method.AlapackPotrsBatched == 0xA
    pf = lapack.ArgPack_potrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    ps = lapack.ArgPack_potrs_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    assert pf.method == lapack.Method.AlapackPotrfBatched and ps.method == lapack.Method.AlapackPotrsBatched
    assert pf.uplo == lapack.UpLo.AlapackUpper
    assert callable(lapack.engine._potrf_batched) and callable(lapack.engine._potrs_batched)
    assert callable(batched.potrf) and callable(batched.potrs)


def test_cpu_tensors_are_refused():
    import torch
    from capital_amd import _lib, batched
    a = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    with pytest.raises(_lib.CapitalError):
        batched.potrf(a)
    with pytest.raises(_lib.CapitalError):
        batched.potrs(a, torch.ones(3, 4, dtype=torch.float64))
