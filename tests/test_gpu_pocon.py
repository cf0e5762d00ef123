"""-m gpu: the reciprocal condition number - cap_dpocon against LAPACK's dpocon ON THE SAME FACTOR AND NORM (the GPU's R copied back), the
true value from an explicit inverse, the edge cases, and cap_cholinv_rcond / cholinv.rcond on the plan.  The matrices are the two
families of tests/poerr_model.py, on which LAPACK's decision path does not hang on the last bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl
import torch

from tests import poerr_model as pm
from tests.gpu_util import NanWork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, 1, 4
NAN = float("nan")


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


_FACTORS = {}


def _factor(family, n, kappa):
    """(A, R from cap_dpotrf on the GPU as a host array, the device buffer of R with leading dimension n + 1 and NaN padding)"""
    key = (family, n, kappa)
    if key not in _FACTORS:
        L = _L()
        A = pm.lap(n) if family == "lap" else pm.rand_spd(n, kappa)
        ld = n + 1
        buf = torch.full((n, ld), NAN, dtype=torch.float64, device=DEV)
        buf[:, :n] = _dev(A)                                                       # symmetric: column-major as well
        info = torch.zeros(1, dtype=torch.int32, device=DEV)
        w = torch.empty(max(int(L.cap_dpotrf_work_size(n)), 2), dtype=torch.float64, device=DEV)
        assert L.cap_dpotrf(1, n, buf.data_ptr(), ld, info.data_ptr(), w.data_ptr(), _stream()) == OK
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        R = np.triu(buf[:, :n].t().cpu().numpy())
        low = np.tril_indices(n, -1)
        v = buf[:, :n].t().clone(); v[low[0], low[1]] = NAN                        # the strictly lower triangle must not be used
        buf[:, :n] = v.t()
        _FACTORS[key] = (A, R, buf, ld)
    return _FACTORS[key]


def _pocon(n, Rbuf, ld, anorm):
    L = _L()
    an = torch.full((1,), anorm, dtype=torch.float64, device=DEV)
    out = torch.full((3,), -5.0, dtype=torch.float64, device=DEV)
    w = NanWork(L.cap_dpocon_work_size(n))                           # all NaN, exactly the stated size, a sentinel behind it
    assert L.cap_dpocon(1, n, Rbuf.data_ptr() if Rbuf is not None else None, ld, an.data_ptr(), out.data_ptr() + 8, w.data_ptr(), _stream()) == OK
    w.check("cap_dpocon(n = %d)" % n)
    o = out.cpu().numpy()
    assert o[0] == -5.0 and o[2] == -5.0
    return o[1]


def _cases():
    for n in pm.NS:
        yield "lap", n, None
        for k in (1e1, 1e4, 1e8, 1e12):
            yield "rand", n, k


@pytest.mark.parametrize("family,n,kappa", list(_cases()))
def test_dpocon_against_lapack_and_the_true_value(family, n, kappa):
    A, R, Rbuf, ld = _factor(family, n, kappa)
    anorm = np.abs(A).sum(0).max()
    got = _pocon(n, Rbuf, ld, anorm)
    true = 1.0 / (anorm * np.abs(np.linalg.inv(A)).sum(0).max())
    ref, info = sl.lapack.dpocon(R, anorm, uplo="U")
    assert info == 0
    print("%s n=%d kappa=%s: gpu %.17g lapack %.17g rel %.2e true %.6g solves %d"
          % (family, n, kappa, got, ref, abs(got - ref) / ref, true, _L().cap_pocon_last_solves()))
    assert 1 <= _L().cap_pocon_last_solves() <= 11
    if family == "lap" or kappa <= 1e4:
        # same R, same norm: the two differ only through the rounding of the solves, n kappa eps
        assert abs(got - ref) <= 1e-8 * ref
    if family == "lap" or kappa <= 1e8:
        assert true <= got * (1 + 1e-3) and got <= 2 * true
    if family == "rand" and kappa == 1e12:
        assert 0.5 * true <= got <= 2 * true


def test_edge_cases_and_repeatability():
    # n = 1: kappa = 1 by definition; exact where the arithmetic is (r and 1 / r powers of two) - LAPACK's own dpocon returns
    # 1.0000000000000002 for A = [[2]], through the rounding of 1 / sqrt(2)
    for a in (1.0, 4.0, 0.25):
        buf = torch.full((1, 2), NAN, dtype=torch.float64, device=DEV); buf[0, 0] = np.sqrt(a)
        assert _pocon(1, buf, 2, a) == 1.0
    A, R, Rbuf, ld = _factor("rand", 300, 1e4)
    assert _pocon(300, Rbuf, ld, 0.0) == 0.0
    assert np.isnan(_pocon(300, Rbuf, ld, NAN))
    anorm = np.abs(A).sum(0).max()
    r1, r2 = _pocon(300, Rbuf, ld, anorm), _pocon(300, Rbuf, ld, anorm)
    assert r1 == r2 and r1 > 0
    assert _pocon(0, None, 0, 1.0) == 1.0
    L = _L()
    assert L.cap_dpocon(0, 300, Rbuf.data_ptr(), ld, Rbuf.data_ptr(), Rbuf.data_ptr(), Rbuf.data_ptr(), _stream()) == UNSUPPORTED


class Plan:
    def __init__(self, n, ci=-1, comm=None):
        self.n, self.h = n, C.c_void_p()
        assert _L().cap_cholinv_plan_create(C.byref(self.h), n, ci, 1, -2, b"U", comm) == 0

    def factor(self, A):
        assert _L().cap_cholinv_factor(self.h, A.data_ptr(), A.shape[0], _stream()) == 0

    def rcond(self, A=None, anorm=None, ld=0):
        out = torch.full((1,), -5.0, dtype=torch.float64, device=DEV)
        st = _L().cap_cholinv_rcond(self.h, A.data_ptr() if A is not None else None, ld, anorm.data_ptr() if anorm is not None else None,
                                    out.data_ptr(), _stream())
        torch.cuda.synchronize()
        return st, out.item()

    def get(self, key):
        return _L().cap_cholinv_get_option(self.h, key.encode())

    def info(self):
        v = C.c_int64(0)
        _L().cap_cholinv_info(self.h, _stream(), C.byref(v))
        return v.value

    def __del__(self):
        _L().cap_cholinv_plan_destroy(self.h)


@pytest.mark.parametrize("ci", [-1, 0, 1])
def test_plan_rcond_is_lansy_then_pocon(ci):
    L = _L()
    n = 1000
    a = pm.rand_spd(n, 1e4)
    A = _dev(a)
    up = A.clone(); low = np.tril_indices(n, -1); up[low[1], low[0]] = NAN         # (column-major buffer: [col, row]) upper triangle only
    p = Plan(n, ci)
    st, _ = p.rcond(A=A, ld=n)
    assert st == ARG, "no factor yet"
    p.factor(A)
    st, got = p.rcond(A=up, ld=n)
    assert st == OK
    # the pieces by hand on the plan's R
    ldr = C.c_int64(0)
    Rp = L.cap_cholinv_R_ptr(p.h, C.byref(ldr))
    an = torch.zeros(1, dtype=torch.float64, device=DEV); rc = torch.zeros(1, dtype=torch.float64, device=DEV)
    w1, w2 = NanWork(L.cap_dlansy_work_size(n)), NanWork(L.cap_dpocon_work_size(n))
    assert L.cap_dlansy(ord('1'), 1, n, up.data_ptr(), n, an.data_ptr(), w1.data_ptr(), _stream()) == OK
    assert L.cap_dpocon(1, n, Rp, ldr.value, an.data_ptr(), rc.data_ptr(), w2.data_ptr(), _stream()) == OK
    w1.check("cap_dlansy"), w2.check("cap_dpocon")
    assert an.item() == np.abs(a).sum(0).max() or abs(an.item() - np.abs(a).sum(0).max()) <= 1e-13 * an.item()
    assert got == rc.item(), "bit for bit"
    st, got2 = p.rcond(anorm=an)
    assert st == OK and got2 == got
    # exactly one of A / anorm
    assert p.rcond()[0] == ARG and p.rcond(A=up, anorm=an, ld=n)[0] == ARG and p.rcond(A=up, ld=n - 1)[0] == ARG


def test_plan_shares_the_block_inverses_with_solve():
    L = _L()
    n = 700
    A = _dev(pm.rand_spd(n, 1e2))
    p = Plan(n)
    p.factor(A)
    B = torch.ones((2, n), dtype=torch.float64, device=DEV); X = torch.empty_like(B)
    assert L.cap_cholinv_solve(p.h, B.data_ptr(), n, X.data_ptr(), n, 2, _stream()) == OK
    assert p.get("solve_prepares") == 1
    assert p.rcond(A=A, ld=n)[0] == OK and p.get("solve_prepares") == 1, "rcond after solve rebuilt the inverses"
    p.factor(A)
    assert p.rcond(A=A, ld=n)[0] == OK and p.get("solve_prepares") == 2
    assert L.cap_cholinv_solve(p.h, B.data_ptr(), n, X.data_ptr(), n, 2, _stream()) == OK
    assert p.get("solve_prepares") == 2, "solve after rcond rebuilt the inverses"


def test_plan_follows_an_update_and_reports_a_failed_factor():
    from capital_amd import cholinv
    from capital_amd.matrix import matrix
    n = 300
    a = pm.rand_spd(n, 1e4)
    rng = np.random.default_rng(2)
    v = rng.standard_normal((n, 2)) * 0.1
    A = matrix(n, n, 1, 1); A.from_numpy(a)
    pack = cholinv.info(-1, 1, -2, 'U')
    cholinv.factor(A, pack, None)
    V = matrix(2, n, 1, 1); V.from_numpy(v)
    cholinv.update(V, pack)
    a2 = a + v @ v.T
    A2 = matrix(n, n, 1, 1); A2.from_numpy(a2)
    got = cholinv.rcond(A2, pack)
    R = np.triu(cholinv.construct_R(pack).to_numpy())
    anorm = np.abs(a2).sum(0).max()
    ref, _ = sl.lapack.dpocon(R, anorm, uplo="U")
    assert abs(got - ref) <= 1e-8 * ref
    # the Python entry point takes the matrix, a float or a device scalar
    assert abs(cholinv.rcond(float(anorm), pack) - ref) <= 1e-8 * ref
    n1 = cholinv.norm1(A2)
    assert n1.is_cuda and n1.numel() == 1 and abs(n1.item() - anorm) <= 1e-13 * anorm
    assert cholinv.rcond(n1, pack) == got
    # a matrix that is not positive definite: 0.0, and the pivot report says why
    bad = a.copy(); bad[n // 2, n // 2] = -1.0
    Ab = matrix(n, n, 1, 1); Ab.from_numpy(bad)
    cholinv.factor(Ab, pack, None)
    assert cholinv.rcond(Ab, pack) == 0.0
    assert pack.last_info() != 0


def _noop_comm(size):
    from capital_amd import _lib
    AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    BC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)
    AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    cbs = (AG(lambda *a: 0), BC(lambda *a: 0), AR(lambda *a: 0))
    h = C.c_void_p()
    _lib.check(_lib.lib().cap_comm_create_callbacks(C.byref(h), 0, size, *[C.cast(c, C.c_void_p) for c in cbs], None), "comm")
    return h, cbs


def test_a_multi_rank_plan_is_refused():
    L = _L()
    n = 512
    buf = torch.ones((n, n), dtype=torch.float64, device=DEV)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    comm, cbs = _noop_comm(4)
    try:
        h = C.c_void_p()
        assert L.cap_cholinv_plan_create(C.byref(h), n, -1, 1, -2, b"U", comm) == 0
        assert L.cap_cholinv_rcond(h, buf.data_ptr(), n, None, out.data_ptr(), _stream()) == UNSUPPORTED
        assert L.cap_cholinv_error_bounds(h, buf.data_ptr(), n, buf.data_ptr(), n, buf.data_ptr(), n, 2, out.data_ptr(), out.data_ptr() + 16,
                                          _stream()) == UNSUPPORTED
        L.cap_cholinv_plan_destroy(h)
    finally:
        L.cap_comm_destroy(comm)
