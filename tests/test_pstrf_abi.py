"""CPU-only: argument handling of the pivoted Cholesky entry points (cap_dpstrf, cap_dpstrf_work_size) - every case here is decided
before the library touches a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, UNSUPPORTED = 0, 1, 4
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


def test_work_size(L):
    for n, r in ((0, 0), (-1, 0), (0, 5)):
        assert L.cap_dpstrf_work_size(n, r) == 0
    ns = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 1001, 4096, 16384, 65536)
    for n in ns:
        ranks = sorted({0, 1, 2, 3, 16, 17, 64, n // 2, n - 1, n} & set(range(n + 1)))
        sizes = [L.cap_dpstrf_work_size(n, r) for r in ranks]
        assert sizes == sorted(sizes) and sizes[0] > 0, "not monotone in max_rank at n = %d" % n       # max_rank = 0 still needs the diagonal
        for r, s in zip(ranks, sizes):
            assert s >= r * n                                                                            # the factor in natural column order
    for r in (0, 1, 2, 17, 63):
        sizes = [L.cap_dpstrf_work_size(n, r) for n in ns if n >= r]
        assert sizes == sorted(sizes), "not monotone in n at max_rank = %d" % r


def test_arguments_are_checked_first(L):
    A = C.c_void_p(1 << 20)              # never dereferenced: every call below returns before any device work
    R = C.c_void_p(1 << 30)
    piv, rank, resid, info = C.c_void_p(1 << 31), C.c_void_p(1 << 32), C.c_void_p(1 << 33), C.c_void_p(1 << 34)
    wrk = C.c_void_p(1 << 35)
    n, r = 10, 3

    def call(uplo=UPPER, n=n, r=r, tol=-1.0, A=A, lda=n, R=R, ldr=r, piv=piv, rank=rank, resid=resid, info=info, wrk=wrk):
        return L.cap_dpstrf(uplo, n, r, tol, A, lda, R, ldr, piv, rank, resid, info, wrk, None)

    assert call(n=-1) == ARG
    assert call(r=-1) == ARG
    assert call(r=n + 1, ldr=n + 1) == ARG
    assert call(tol=NAN) == ARG
    assert call(n=0, r=0, tol=NAN) == ARG
    assert call(A=None) == ARG
    assert call(piv=None) == ARG
    assert call(rank=None) == ARG
    assert call(wrk=None) == ARG
    assert call(lda=n - 1) == ARG
    assert call(R=None) == ARG
    assert call(ldr=r - 1) == ARG
    assert call(r=0, R=None, ldr=0, A=None) == ARG               # max_rank = 0 still reads A ...
    assert call(r=0, R=None, ldr=0, wrk=None) == ARG             # ... and still needs its scratch
    # LOWER is refused after the argument rules and before the empty case
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, r=0, R=None, ldr=0) == UNSUPPORTED
    assert call(uplo=LOWER, lda=n - 1) == ARG
    assert call(uplo=LOWER, R=None) == ARG
    assert call(uplo=LOWER, tol=NAN) == ARG
    assert call(uplo=LOWER, n=0, r=0, A=None, lda=0, R=None, ldr=0, piv=None, rank=None, resid=None, info=None, wrk=None) == UNSUPPORTED
    # n = 0: nothing is touched, whatever the pointers
    assert call(n=0, r=0, A=None, lda=0, R=None, ldr=0, piv=None, rank=None, resid=None, info=None, wrk=None) == OK
    assert call(n=0, r=0) == OK
    assert call(n=0, r=1) == ARG                                  # max_rank > n


def test_python_layer_names():
    from capital_amd import cholinv, lapack
    assert lapack.Method.AlapackPstrf == 0x5
    pack = lapack.ArgPack_pstrf(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    assert pack.method == lapack.Method.AlapackPstrf and pack.uplo == lapack.UpLo.AlapackUpper
    assert callable(lapack.engine._pstrf) and callable(cholinv.factor_pivoted)
