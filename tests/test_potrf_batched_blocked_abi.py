"""CPU-only: argument handling of the batched factor and solve for blocks of up to 256 rows (cap_dpotrf_batched_blocked,
cap_dpotrs_batched_blocked) - the table of tests/test_potrf_batched_abi.py for the two new symbols, with the size limit at 256.  Every case
here is decided before the library touches a device."""
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
        return L.cap_dpotrf_batched_blocked(uplo, n, A, lda, stride, batch, info, logdet, None)

    assert call(n=-1) == ARG
    assert call(batch=-1) == ARG
    assert call(A=None) == ARG
    assert call(lda=n - 1, stride=n * n) == ARG
    assert call(stride=n * n - 1) == ARG
    assert call(lda=n + 2, stride=(n + 2) * n - 1) == ARG
    assert call(stride=-1) == ARG
    assert call(n=257, lda=257, stride=257 * 257) == UNSUPPORTED
    assert call(n=257, lda=256, stride=257 * 257) == ARG             # the argument rules come first
    assert call(n=1 << 20, lda=1 << 20, stride=1 << 40) == UNSUPPORTED
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, n=0, lda=0, stride=0) == UNSUPPORTED     # LOWER is refused before the empty case
    assert call(uplo=LOWER, lda=n - 1) == ARG
    assert call(uplo=LOWER, A=None) == ARG
    assert call(uplo=LOWER, n=65, lda=65, stride=65 * 65) == UNSUPPORTED
    # degenerate sizes: nothing is launched, whatever the pointers
    assert call(n=0, A=None, lda=0, stride=0, info=None, logdet=None) == OK
    assert call(n=0) == OK
    assert call(batch=0, A=None, info=None, logdet=None) == OK
    assert call(batch=0, stride=0) == OK
    assert call(n=0, batch=0, A=None, lda=0, stride=0) == OK
    assert call(n=257, lda=257, stride=0, batch=0) == UNSUPPORTED    # n > 256 is refused for an empty batch too
    assert call(batch=0, A=None, stride=-5) == OK
    # 65 and 256 pass every rule: with an empty batch they end as OK without a launch, and their own refusals are the argument rules
    for big in (65, 256):
        assert call(n=big, lda=big, stride=big * big, batch=0) == OK
        assert call(n=big, lda=big, stride=big * big, batch=0, A=None) == OK
        assert call(n=big, lda=big - 1, stride=big * big) == ARG
        assert call(n=big, lda=big, stride=big * big - 1) == ARG
        assert call(n=big, lda=big, stride=big * big, A=None) == ARG


def test_solve_arguments_are_checked_first(L):
    n, nrhs, batch = 10, 3, 5

    def call(uplo=UPPER, n=n, nrhs=nrhs, R=A, ldr=n, stride_r=n * n, B=B, ldb=n, stride_b=n * nrhs, batch=batch, info=INFO):
        return L.cap_dpotrs_batched_blocked(uplo, n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, None)

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
    assert call(n=257, ldr=257, stride_r=257 * 257, ldb=257, stride_b=257 * nrhs) == UNSUPPORTED
    assert call(n=257, ldr=257, stride_r=257 * 257, ldb=256, stride_b=257 * nrhs) == ARG
    assert call(n=257, ldr=257, stride_r=0, ldb=257, stride_b=0, batch=0) == UNSUPPORTED
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, nrhs=0, stride_b=0) == UNSUPPORTED
    assert call(uplo=LOWER, ldr=n - 1) == ARG
    assert call(n=0, R=None, ldr=0, stride_r=0, B=None, ldb=0, stride_b=0, info=None) == OK
    assert call(batch=0, R=None, B=None, info=None) == OK
    assert call(nrhs=0, stride_b=0) == OK
    assert call(nrhs=0, stride_b=0, info=None) == OK
    for big in (65, 256):
        kw = dict(n=big, ldr=big, stride_r=big * big, ldb=big, stride_b=big * nrhs)
        assert call(**dict(kw, batch=0)) == OK
        assert call(**dict(kw, nrhs=0, stride_b=0)) == OK
        assert call(**dict(kw, ldb=big - 1)) == ARG
        assert call(**dict(kw, stride_r=big * big - 1)) == ARG
        assert call(**dict(kw, B=None)) == ARG
        assert call(**dict(kw, uplo=LOWER)) == UNSUPPORTED


def test_single_block_needs_no_stride(L):
    """batch = 1: the strides are not used and not checked; batch = 2 with the same strides is refused"""
    n, nrhs = 100, 2
    assert L.cap_dpotrf_batched_blocked(UPPER, n, A, n, 0, 2, None, None, None) == ARG
    assert L.cap_dpotrs_batched_blocked(UPPER, n, nrhs, A, n, 0, B, n, n * nrhs, 2, None, None) == ARG
    assert L.cap_dpotrs_batched_blocked(UPPER, n, nrhs, A, n, n * n, B, n, 0, 2, None, None) == ARG
    assert L.cap_dpotrf_batched_blocked(LOWER, n, A, n, 0, 1, None, None, None) == UNSUPPORTED      # passes the argument rules with stride 0 ...
    assert L.cap_dpotrf_batched_blocked(LOWER, n, A, n, 0, 2, None, None, None) == ARG              # ... which two blocks do not


def test_the_stride_rule_does_not_wrap(L):
    """ld * columns beyond int64 (2^60 * 16 = 2^64 wraps to 0): the stride rule compares with the clipped product, so two blocks at stride 0
    are refused like any other overlap - decided before any device work"""
    big = 1 << 60
    assert L.cap_dpotrf_batched_blocked(UPPER, 16, A, big, 0, 2, None, None, None) == ARG
    assert L.cap_dpotrs_batched_blocked(UPPER, 16, 16, A, big, 0, B, 16, 16 * 16, 2, None, None) == ARG
    assert L.cap_dpotrs_batched_blocked(UPPER, 16, 16, A, 16, 16 * 16, B, big, 0, 2, None, None) == ARG


def test_the_existing_entries_keep_their_limit(L):
    assert L.cap_dpotrf_batched(UPPER, 65, A, 65, 65 * 65, 5, INFO, LOGDET, None) == UNSUPPORTED
    assert L.cap_dpotrs_batched(UPPER, 65, 3, A, 65, 65 * 65, B, 65, 65 * 3, 5, INFO, None) == UNSUPPORTED


def test_python_layer_names():
    from capital_amd import _lib, batched, lapack
    assert lapack.BATCHED_SMALL_MAX == 64 and lapack.BATCHED_MAX == 256
    assert callable(lapack.engine._potrf_batched) and callable(lapack.engine._potrs_batched)
    assert callable(batched.potrf) and callable(batched.potrs)
    assert "256" in batched.potrf.__doc__ and "256" in lapack.engine._potrf_batched.__doc__
    with pytest.raises(_lib.CapitalError, match="256"):
        lapack._batched_blocked(None, 257)


def test_cpu_tensors_are_refused():
    import torch
    from capital_amd import _lib, batched
    a = torch.eye(100, dtype=torch.float64).repeat(3, 1, 1)
    with pytest.raises(_lib.CapitalError):
        batched.potrf(a)
    with pytest.raises(_lib.CapitalError):
        batched.potrs(a, torch.ones(3, 100, dtype=torch.float64))
