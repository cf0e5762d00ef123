"""-m gpu: the SPD inverse and log-determinant from the Cholesky factor - the triangular product cap_dlauum (C = W W^T, bit for bit on
integer matrices), cap_cholinv_inverse / cap_cholinv_logdet on the plan's last factor, cap_dpotri beside cap_dpotrf, the failure cases and
the Python layer.  (Helpers as in tests/test_gpu_cholinv_solve.py.)"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNSUPPORTED = 4
SENTINEL = -7.5            # no integer: an element the exact-product test left unwritten cannot pass for a result


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _spd(n, seed):
    """Well-conditioned SPD test matrix G G^T / n + I on the GPU (symmetric: its buffer is column-major as well)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    G = torch.rand(n, n, dtype=torch.float64, device=DEV, generator=g) * 2 - 1
    return G @ G.T / n + torch.eye(n, dtype=torch.float64, device=DEV)


@functools.lru_cache(maxsize=4)
def _spd_and_inverse(n, seed):
    """(A on the GPU, A as NumPy, np.linalg.inv(A)): the same matrix serves several cases"""
    A = _spd(n, seed)
    a = A.cpu().numpy()
    return A, a, np.linalg.inv(a)


class Plan:
    def __init__(self, n, ci):
        self.n, self.h = n, C.c_void_p()
        assert _L().cap_cholinv_plan_create(C.byref(self.h), n, ci, 1, -2, b"U", None) == 0

    def factor(self, A):
        assert _L().cap_cholinv_factor(self.h, A.data_ptr(), A.shape[0], _stream()) == 0

    def inverse(self, Xbuf, fill):
        return _L().cap_cholinv_inverse(self.h, Xbuf.data_ptr(), Xbuf.shape[1], fill, _stream())

    def logdet(self):
        out = torch.zeros(1, dtype=torch.float64, device=DEV)
        assert _L().cap_cholinv_logdet(self.h, out.data_ptr(), _stream()) == 0
        return out.item()

    def diag_R(self):
        R = torch.empty(self.n, self.n, dtype=torch.float64, device=DEV)
        assert _L().cap_cholinv_get_R(self.h, R.data_ptr(), self.n, _stream()) == 0
        return torch.diagonal(R).cpu().numpy().copy()

    def info(self):
        v = C.c_int64(0)
        _L().cap_cholinv_info(self.h, _stream(), C.byref(v))
        return v.value

    def __del__(self):
        _L().cap_cholinv_plan_destroy(self.h)


def _out(n, ld):
    """n x n column-major output buffer with leading dimension ld, pre-filled with the sentinel: (buffer[col, row], view[row, col])"""
    buf = torch.full((n, ld), SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[:, :n].t()


def _untouched_outside_upper(buf, n):
    """strictly lower triangle of the window (buffer[col, row] with row > col) and the padding rows still hold the sentinel"""
    keep = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), diagonal=1)    # buffer indices (col, row): row > col is ABOVE the buffer's diagonal
    return bool(torch.all(buf[:, :n][keep] == SENTINEL)) and bool(torch.all(buf[:, n:] == SENTINEL))


# ---- 1. the kernel, bit for bit ---------------------------------------------------------------------------------------------------------------
LAUUM_SIZES = (1, 16, 100, 127, 128, 129, 256, 1000, 1152, 2048, 4096, 4224)
LAUUM_CASES = [(n, pw, pc) for n in LAUUM_SIZES for (pw, pc) in ((0, 0), (2, 6))] + [(100, 3, 1), (1152, 3, 1)]


@pytest.mark.parametrize("n,padw,padc", LAUUM_CASES)
def test_lauum_is_exact_on_integer_matrices(n, padw, padc):
    """W upper triangular with entries from {-3 ... 3} (diagonal non-zero) and NaN in every strictly-lower element: every product and partial
    sum of W W^T is an integer below 9 n < 2^53, so any summation order and any FMA contraction is exact - a mismatch is a wrong K range, a
    wrong tile map or a read below the diagonal, never rounding.  (9 tiles: neither a multiple nor a divisor of the 8 XCDs; 33 tiles: one
    more than four rounds of tile columns; padw = 3: odd leading dimension, the copy route.)"""
    ldw, ldc = n + padw, n + padc
    rng = np.random.default_rng(1000 + n)
    w = np.triu(rng.integers(-3, 4, size=(n, n)))
    d = rng.integers(1, 4, size=n) * rng.choice([-1, 1], size=n)
    w[np.arange(n), np.arange(n)] = d
    wt = torch.from_numpy(w.astype(np.float64)).to(DEV)                        # [row, col], exact zeros below the diagonal
    # the reference product: fp64 on integers below 2^53 is exact whatever the order; checked against the int64 product where that is cheap
    ref = wt @ wt.T
    if n <= 256:
        assert np.array_equal(ref.cpu().numpy().astype(np.int64), w.astype(np.int64) @ w.astype(np.int64).T)
    Wbuf = torch.full((n, ldw), float("nan"), dtype=torch.float64, device=DEV)   # [col, row]
    up = torch.tril(torch.ones(n, n, dtype=torch.bool, device=DEV))              # buffer (col, row) with row <= col
    Wbuf[:, :n][up] = wt.T[up]
    assert bool(torch.isnan(Wbuf[:, :n][~up]).all()) or n == 1
    Cbuf, Cv = _out(n, ldc)
    assert _L().cap_dlauum(1, n, Wbuf.data_ptr(), ldw, Cbuf.data_ptr(), ldc, _stream()) == 0
    torch.cuda.synchronize()
    iu = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV))              # view (row, col) with row <= col
    bad = (Cv != ref) & iu
    assert not bool(bad.any()), "upper triangle differs at %s" % (torch.nonzero(bad)[:5].tolist(),)
    assert _untouched_outside_upper(Cbuf, n), "written below the diagonal of C or into the padding rows"


# ---- 2. inverse accuracy ----------------------------------------------------------------------------------------------------------------------
# (n, complete_inv, fill, ld)
INV_CASES = ([(n, ci, fill, n + (5 if fill == 0 else 0)) for n in (100, 1000, 4096) for ci in (1, 0, -1) for fill in (0, 1)]
             + [(1, 1, 1, 1), (1, -1, 0, 4), (1, 0, 1, 1), (1000, -1, 1, 1005), (777, 1, 1, 780)])


@pytest.mark.parametrize("n,ci,fill,ld", INV_CASES)
def test_inverse_accuracy(n, ci, fill, ld):
    A, a, ainv = _spd_and_inverse(n, 1 + n)
    p = Plan(n, ci)
    p.factor(A)
    Xbuf, X = _out(n, ld)
    assert p.inverse(Xbuf, fill) == 0
    torch.cuda.synchronize()
    assert p.info() == 0
    x = X.cpu().numpy()
    if fill:
        assert np.array_equal(x, x.T), "fill = 1: X is not bit-for-bit symmetric"
        assert bool(torch.all(Xbuf[:, n:] == SENTINEL)), "written into the padding rows"
    else:
        assert _untouched_outside_upper(Xbuf, n), "fill = 0: written outside the upper triangle"
        x = np.triu(x) + np.triu(x, 1).T
    err = np.linalg.norm(x - ainv) / np.linalg.norm(ainv)
    print("n=%d ci=%d fill=%d ld=%d: |X - inv(A)|_F / |inv(A)|_F = %.3e" % (n, ci, fill, ld, err))
    assert err <= 1e-12, err


@pytest.mark.parametrize("ci", [1, -1])
def test_inverse_residual_16384(ci):
    n = 16384
    A = _spd(n, 5)
    p = Plan(n, ci)
    p.factor(A)
    Xbuf, X = _out(n, n)
    assert p.inverse(Xbuf, 1) == 0
    torch.cuda.synchronize()
    assert p.info() == 0
    na, nx = torch.linalg.norm(A).item(), torch.linalg.norm(X).item()
    E = A @ X
    E.diagonal().sub_(1.0)
    res = torch.linalg.norm(E).item() / (na * nx)
    print("n=%d ci=%d: |A X - I|_F / (|A|_F |X|_F) = %.3e" % (n, ci, res))
    assert res <= 1e-15, res


# ---- 3. routes agree and repeat ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4096])
def test_routes_agree_and_calls_repeat(n):
    A = _spd(n, 3)
    outs = {}
    for ci in (1, -1):
        p = Plan(n, ci)
        p.factor(A)
        X1, _ = _out(n, n)
        X2, _ = _out(n, n)
        assert p.inverse(X1, 1) == 0 and p.inverse(X2, 1) == 0
        torch.cuda.synchronize()
        assert torch.equal(X1, X2), "two calls on one plan differ (complete_inv = %d)" % ci
        outs[ci] = X1
    diff = (torch.linalg.norm(outs[1] - outs[-1]) / torch.linalg.norm(outs[1])).item()
    print("n=%d: routes differ by %.3e" % (n, diff))
    assert diff <= 1e-13, diff


# ---- 4. stale cache ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [-1, 0])
def test_a_new_factor_call_makes_the_cached_inverse_stale(ci):
    n = 1500
    A1, A2 = _spd(n, 21), _spd(n, 22) + 3 * torch.eye(n, dtype=torch.float64, device=DEV)
    p = Plan(n, ci)
    Xbuf, X = _out(n, n)
    p.factor(A1)
    assert p.inverse(Xbuf, 1) == 0
    p.factor(A2)
    assert p.inverse(Xbuf, 1) == 0
    torch.cuda.synchronize()
    ref = np.linalg.inv(A2.cpu().numpy())
    err = np.linalg.norm(X.cpu().numpy() - ref) / np.linalg.norm(ref)
    assert err <= 1e-12, err


# ---- 5. failure cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,fill", [(-1, 1), (-1, 0), (1, 1), (0, 0)])
def test_not_spd_gives_nan_and_no_error(ci, fill):
    n = 300
    A = torch.eye(n, dtype=torch.float64, device=DEV) * 2
    A[150, 150] = -1.0
    p = Plan(n, ci)
    p.factor(A)
    Xbuf, X = _out(n, n + 2)
    assert p.inverse(Xbuf, fill) == 0
    ld = p.logdet()
    torch.cuda.synchronize()
    if fill:
        assert bool(torch.isnan(X).all())
        assert bool(torch.all(Xbuf[:, n:] == SENTINEL))
    else:
        iu = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV))
        assert bool(torch.isnan(X[iu]).all())
        assert _untouched_outside_upper(Xbuf, n)
    assert math.isnan(ld)
    assert p.info() != 0


def _noop_comm(size):
    from capital_amd import _lib
    AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    BC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)
    AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    cbs = (AG(lambda *a: 0), BC(lambda *a: 0), AR(lambda *a: 0))
    h = C.c_void_p()
    _lib.check(_lib.lib().cap_comm_create_callbacks(C.byref(h), 0, size, *[C.cast(c, C.c_void_p) for c in cbs], None), "comm")
    return h, cbs


def test_unsupported_plans_bad_arguments_and_lower_uplo():
    L = _L()
    n = 512
    Xbuf, _ = _out(n, n)
    ld = torch.zeros(1, dtype=torch.float64, device=DEV)
    comm, cbs = _noop_comm(4)
    try:
        h = C.c_void_p()
        assert L.cap_cholinv_plan_create(C.byref(h), n, -1, 1, -2, b"U", comm) == 0
        assert L.cap_cholinv_inverse(h, Xbuf.data_ptr(), n, 1, _stream()) == UNSUPPORTED
        assert L.cap_cholinv_logdet(h, ld.data_ptr(), _stream()) == UNSUPPORTED
        assert L.cap_cholinv_set_option(h, b"cyclic_c", 1) == 0 and L.cap_cholinv_get_option(h, b"cyclic_c") == 1
        assert L.cap_cholinv_inverse(h, Xbuf.data_ptr(), n, 1, _stream()) == UNSUPPORTED
        assert L.cap_cholinv_logdet(h, ld.data_ptr(), _stream()) == UNSUPPORTED
        L.cap_cholinv_plan_destroy(h)
    finally:
        L.cap_comm_destroy(comm)
    p = Plan(n, -1)
    assert p.inverse(Xbuf, 1) == 1 and L.cap_cholinv_logdet(p.h, ld.data_ptr(), _stream()) == 1      # never factored
    p.factor(_spd(n, 2))
    assert p.inverse(Xbuf, 2) == 1 and p.inverse(Xbuf, -1) == 1                                        # fill outside {0, 1}
    assert L.cap_cholinv_inverse(p.h, Xbuf.data_ptr(), n - 1, 1, _stream()) == 1
    assert L.cap_cholinv_inverse(p.h, None, n, 1, _stream()) == 1 and L.cap_cholinv_logdet(p.h, None, _stream()) == 1
    torch.cuda.synchronize()
    assert bool(torch.all(Xbuf == SENTINEL)), "a refused call wrote its output"
    R = torch.eye(n, dtype=torch.float64, device=DEV)
    work = torch.empty(L.cap_dpotri_work_size(n), dtype=torch.float64, device=DEV)
    assert L.cap_dpotri(0, n, R.data_ptr(), n, work.data_ptr(), _stream()) == UNSUPPORTED
    assert L.cap_dlauum(0, n, R.data_ptr(), n, Xbuf.data_ptr(), n, _stream()) == UNSUPPORTED


# ---- 6. cap_dpotri after cap_dpotrf on a padded window ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [777, 2048])
def test_dpotri_after_dpotrf_on_a_padded_window(n):
    L = _L()
    lda = n + 7
    A, a, ainv = _spd_and_inverse(n, 30 + n)
    buf = torch.full((n + 1, lda), 5.0, dtype=torch.float64, device=DEV)    # an extra column: the window sits inside a bigger buffer
    buf[:n, :n] = A
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    w1 = torch.empty(L.cap_dpotrf_work_size(n), dtype=torch.float64, device=DEV)
    assert L.cap_dpotrf(1, n, buf.data_ptr(), lda, info.data_ptr(), w1.data_ptr(), _stream()) == 0
    low = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), diagonal=1)    # buffer (col, row) with row > col: strictly lower part
    buf[:n, :n][low] = float("nan")
    w2 = torch.empty(L.cap_dpotri_work_size(n), dtype=torch.float64, device=DEV)
    assert L.cap_dpotri(1, n, buf.data_ptr(), lda, w2.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    assert bool(torch.isnan(buf[:n, :n][low]).all()), "strictly lower part of the window written"
    assert bool(torch.all(buf[:, n:] == 5.0)) and bool(torch.all(buf[n, :] == 5.0)), "written outside the window"
    x = buf[:n, :n].t().cpu().numpy()
    x = np.triu(x) + np.triu(x, 1).T
    err = np.linalg.norm(x - ainv) / np.linalg.norm(ainv)
    assert err <= 1e-12, err


# ---- 7. log-determinant -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 100, 1000, 4096])
def test_logdet(n):
    """Against the factor's own diagonal: 2 ulp for the device log plus a summation tree of depth log2 n.  Against NumPy's slogdet of A: the
    factor's backward error, 16 n kappa(A) 2^-53."""
    A = _spd(n, 1 + n)
    a = A.cpu().numpy()
    p = Plan(n, -1)
    p.factor(A)
    v1, v2 = p.logdet(), p.logdet()
    torch.cuda.synchronize()
    assert p.info() == 0
    assert v1 == v2, "two calls differ"
    logd = np.log(p.diag_R())
    S = float(np.sum(np.abs(logd)))
    e1 = abs(v1 - 2.0 * math.fsum(logd))
    ev = np.linalg.eigvalsh(a)
    kappa = float(ev[-1] / ev[0])
    e2 = abs(v1 - np.linalg.slogdet(a)[1])
    print("n=%d: logdet = %.17g, against the diagonal %.3e (bound %.3e), against slogdet %.3e (bound %.3e)"
          % (n, v1, e1, 2 * (4 + math.log2(n)) * 2.0 ** -52 * S, e2, 16 * n * kappa * 2.0 ** -53))
    assert e1 <= 2 * (4 + math.log2(n)) * 2.0 ** -52 * S
    assert e2 <= 16 * n * kappa * 2.0 ** -53


# ---- 8. Python --------------------------------------------------------------------------------------------------------------------------------
def test_python_interfaces():
    from capital_amd import cholinv, lapack
    from capital_amd.matrix import matrix
    n = 600
    a = _spd(n, 41).cpu().numpy()
    ref = np.linalg.inv(a)
    A = matrix(n, n, 1, 1); A.from_numpy(a)
    for ci in (-1, 1):
        pack = cholinv.info(ci, 1, -2, 'U')
        cholinv.factor(A, pack, None)
        X = cholinv.inverse(pack).to_numpy()
        assert np.array_equal(X, X.T)
        assert np.linalg.norm(X - ref) / np.linalg.norm(ref) <= 1e-12
        out = matrix(n, n, 1, 1); out.from_numpy(np.full((n, n), SENTINEL))
        assert cholinv.inverse(pack, out, fill=False) is out
        U = out.to_numpy()
        assert np.all(np.tril(U, -1) == np.tril(np.full((n, n), SENTINEL), -1))
        assert np.linalg.norm(np.triu(U) - np.triu(ref)) / np.linalg.norm(np.triu(ref)) <= 1e-12
        ld = cholinv.logdet(pack)
        assert isinstance(ld, float) and abs(ld - np.linalg.slogdet(a)[1]) <= 16 * n * np.linalg.cond(a) * 2.0 ** -53
    R = torch.from_numpy(a.T.copy()).to(DEV)
    up = lapack.UpLo.AlapackUpper
    assert lapack.engine._potrf(R, n, n, lapack.ArgPack_potrf(lapack.Order.AlapackColumnMajor, up)) == 0
    lapack.engine._potri(R, n, n, lapack.ArgPack_potri(lapack.Order.AlapackColumnMajor, up))
    x = R.t().cpu().numpy()
    assert np.linalg.norm(np.triu(x) - np.triu(ref)) / np.linalg.norm(np.triu(ref)) <= 1e-12
