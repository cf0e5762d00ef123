"""CPU-only: argument handling of the condition-estimate and error-bound entry points (cap_dsymm_thin, cap_dlansy, cap_dpocon, cap_dpoerr,
cap_cholinv_rcond, cap_cholinv_error_bounds and their work sizes) - every case here is decided before the library touches a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, UNSUPPORTED = 0, 1, 4
NAN = float("nan")
P = lambda k: C.c_void_p(1 << k)         # never dereferenced: every call below returns before any device work


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


def test_work_sizes(L):
    ns = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1000, 1025, 4096, 16384, 65536)
    for n in (0, -1):
        assert L.cap_dlansy_work_size(n) == 0 and L.cap_dpocon_work_size(n) == 0
        assert L.cap_dsymm_thin_work_size(n, 3) == 0 and L.cap_dpoerr_work_size(n, 3) == 0
    for f in (L.cap_dsymm_thin_work_size, L.cap_dpoerr_work_size):
        assert f(10, 0) == 0 and f(10, -1) == 0
        for r in (1, 2, 3, 4, 5, 8, 15, 16, 17, 33):
            sizes = [f(n, r) for n in ns]
            assert sizes == sorted(sizes) and sizes[0] > 0, "not monotone in n at nrhs = %d" % r
        for n in ns:
            sizes = [f(n, r) for r in (1, 2, 3, 4, 5, 8, 15, 16, 17, 33)]
            assert sizes == sorted(sizes), "not monotone in nrhs at n = %d" % n
    for f in (L.cap_dlansy_work_size, L.cap_dpocon_work_size):
        sizes = [f(n) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] > 0
    # one slot of row and column parts per super-block of the upper block triangle
    assert L.cap_dsymm_thin_work_size(1025, 16) >= 6 * 2 * 512 * 16


def test_symm_thin_arguments(L):
    n, r = 10, 3
    A, X, B, Y, W = P(20), P(30), P(31), P(32), P(35)

    def call(uplo=UPPER, ab=0, n=n, r=r, alpha=1.0, A=A, lda=n, X=X, ldx=n, beta=1.0, B=B, ldb=n, Y=Y, ldy=n, W=W):
        return L.cap_dsymm_thin(uplo, ab, n, r, alpha, A, lda, X, ldx, beta, B, ldb, Y, ldy, W, None)

    assert call(n=-1) == ARG and call(r=-1) == ARG
    assert call(ab=2) == ARG and call(ab=-1) == ARG
    assert call(alpha=NAN) == ARG and call(beta=NAN) == ARG
    for kw in (dict(A=None), dict(X=None), dict(B=None), dict(Y=None), dict(W=None), dict(lda=n - 1), dict(ldx=n - 1), dict(ldb=n - 1),
               dict(ldy=n - 1)):
        assert call(**kw) == ARG, kw
    # Y must not overlap A, X or work; Y may be B
    assert call(Y=A) == ARG and call(Y=X) == ARG and call(Y=W) == ARG
    assert call(Y=C.c_void_p((1 << 20) + 8 * (n * n - 1))) == ARG           # the last element of A
    assert call(uplo=LOWER, Y=B) == UNSUPPORTED                              # (in place passes the argument rules)
    # LOWER is refused after the argument rules and before the empty case
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, lda=n - 1) == ARG
    assert call(uplo=LOWER, n=0, lda=0, ldx=0, ldb=0, ldy=0) == UNSUPPORTED
    assert call(uplo=LOWER, r=0) == UNSUPPORTED
    # empty problems: nothing is touched, whatever the pointers
    assert call(n=0, A=None, X=None, B=None, Y=None, W=None, lda=0, ldx=0, ldb=0, ldy=0) == OK
    assert call(r=0, A=None, X=None, B=None, Y=None, W=None) == OK
    # beta == 0 does not need B; alpha == 0 needs neither A, X nor work - still LOWER is refused
    assert call(uplo=LOWER, beta=0.0, B=None, ldb=0) == UNSUPPORTED
    assert call(uplo=LOWER, alpha=0.0, A=None, X=None, W=None, lda=0, ldx=0) == UNSUPPORTED
    assert call(uplo=LOWER, alpha=0.0, Y=None) == ARG


def test_lansy_arguments(L):
    n = 10
    A, out, W = P(20), P(30), P(35)

    def call(norm=b'1', uplo=UPPER, n=n, A=A, lda=n, out=out, W=W):
        return L.cap_dlansy(ord(norm), uplo, n, A, lda, out, W, None)

    assert call(n=-1) == ARG and call(A=None) == ARG and call(out=None) == ARG and call(W=None) == ARG and call(lda=n - 1) == ARG
    assert call(n=0, out=None) == ARG
    for norm in (b'F', b'M', b'2', b'E'):
        assert call(norm=norm) == UNSUPPORTED
        assert call(norm=norm, lda=n - 1) == ARG
    for norm in (b'1', b'O', b'I'):
        assert call(norm=norm, uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, n=0, A=None, W=None, lda=0) == UNSUPPORTED
    assert call(uplo=LOWER, A=None) == ARG


def test_pocon_arguments(L):
    n = 10
    R, an, rc, W = P(20), P(30), P(31), P(35)

    def call(uplo=UPPER, n=n, R=R, ldr=n, an=an, rc=rc, W=W):
        return L.cap_dpocon(uplo, n, R, ldr, an, rc, W, None)

    assert call(n=-1) == ARG
    for kw in (dict(R=None), dict(an=None), dict(rc=None), dict(W=None), dict(ldr=n - 1), dict(n=0, rc=None)):
        assert call(**kw) == ARG, kw
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, ldr=n - 1) == ARG
    assert call(uplo=LOWER, n=0, R=None, an=None, W=None, ldr=0) == UNSUPPORTED


def test_poerr_arguments(L):
    n, r = 10, 3
    A, R, B, X, fe, be, W = P(20), P(28), P(30), P(31), P(32), P(33), P(35)

    def call(uplo=UPPER, n=n, r=r, A=A, lda=n, R=R, ldr=n, B=B, ldb=n, X=X, ldx=n, fe=fe, be=be, W=W):
        return L.cap_dpoerr(uplo, n, r, A, lda, R, ldr, B, ldb, X, ldx, fe, be, W, None)

    assert call(n=-1) == ARG and call(r=-1) == ARG
    for kw in (dict(A=None), dict(R=None), dict(B=None), dict(X=None), dict(W=None), dict(lda=n - 1), dict(ldr=n - 1), dict(ldb=n - 1),
               dict(ldx=n - 1)):
        assert call(**kw) == ARG, kw
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER, fe=None, be=None) == UNSUPPORTED
    assert call(uplo=LOWER, ldb=n - 1) == ARG
    assert call(uplo=LOWER, r=0) == UNSUPPORTED
    assert call(uplo=LOWER, n=0, lda=0, ldr=0, ldb=0, ldx=0) == UNSUPPORTED
    assert call(r=0, A=None, R=None, B=None, X=None, W=None) == OK
    assert call(fe=None, be=None) == OK                                      # nothing asked for


def test_plan_arguments(L):
    # without a device there is no plan: a NULL plan is refused first (the A / anorm rules on a live plan are in tests/test_gpu_pocon.py)
    A, an, rc = P(20), P(30), P(31)
    assert L.cap_cholinv_rcond(None, A, 10, None, rc, None) == ARG
    assert L.cap_cholinv_rcond(None, None, 0, None, rc, None) == ARG
    assert L.cap_cholinv_rcond(None, A, 10, an, rc, None) == ARG
    assert L.cap_cholinv_error_bounds(None, A, 10, A, 10, A, 10, 1, rc, rc, None) == ARG


def test_python_layer_names():
    from capital_amd import cholinv, lapack
    assert (lapack.Method.AlapackLansy, lapack.Method.AlapackPocon, lapack.Method.AlapackPoerr) == (0x6, 0x7, 0x8)
    col, up = lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper
    assert lapack.ArgPack_lansy(col, up).method == lapack.Method.AlapackLansy and lapack.ArgPack_lansy(col, up).norm == '1'
    assert lapack.ArgPack_pocon(col, up).method == lapack.Method.AlapackPocon
    assert lapack.ArgPack_poerr(col, up).method == lapack.Method.AlapackPoerr
    for f in (lapack.engine._lansy, lapack.engine._pocon, lapack.engine._poerr, cholinv.norm1, cholinv.rcond, cholinv.error_bounds):
        assert callable(f)
