"""-m gpu: the error bounds of a computed solution - cap_cholinv_error_bounds / cap_dpoerr / cholinv.error_bounds.  berr against the same
quotient formed on the host in long double, ferr against the exact quantity it estimates (|| |A^-1| w ||_inf / ||x||_inf, from an explicit
inverse) and against the actual error of the solution."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import poerr_model as pm
from tests.gpu_util import NanWork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK = 0
NAN = float("nan")
EPS = pm.EPS


def _rhs(A, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.standard_normal(n), A @ np.ones(n), rng.standard_normal(n) * np.logspace(0, -8, n)], axis=1)


_SOLVED = {}


def _solved(n, kappa, nrhs=3):
    """(A, B, X from cholinv.solve, the pack, device matrices) - factored and solved once per case, then only read"""
    from capital_amd import cholinv
    from capital_amd.matrix import matrix
    key = (n, kappa, nrhs)
    if key not in _SOLVED:
        a = pm.rand_spd(n, kappa)
        b = _rhs(a, n, n)
        if nrhs > 3:
            b = np.concatenate([b] + [_rhs(a, n, n + k) for k in range(1, (nrhs + 2) // 3)], axis=1)[:, :nrhs]
        A = matrix(n, n, 1, 1); A.from_numpy(a)
        B = matrix(nrhs, n, 1, 1); B.from_numpy(b)
        pack = cholinv.info(-1, 1, -2, 'U')
        cholinv.factor(A, pack, None)
        X = cholinv.solve(B, pack)
        _SOLVED[key] = (a, b, X.to_numpy(), pack, A, B, X)
    return _SOLVED[key]


def _berr_ld(a, b, x):
    return pm.berr(a, b, x, dtype=np.longdouble).astype(np.float64)


def _refine(a, b, x):
    """x* from six refinement steps with long double residuals"""
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    xs = x.astype(np.longdouble)
    c = np.linalg.cholesky(a)
    import scipy.linalg as sl
    for _ in range(6):
        r = (bl - al @ xs).astype(np.float64)
        xs = xs + sl.cho_solve((c, True), r).astype(np.longdouble)
    return xs


CASES = [(n, k) for n in (129, 300, 1000) for k in (1e2, 1e6, 1e10)]


@pytest.mark.parametrize("n,kappa", CASES)
def test_bounds_of_a_solve(n, kappa):
    from capital_amd import cholinv
    a, b, x, pack, A, B, X = _solved(n, kappa)
    ferr, berr = cholinv.error_bounds(A, B, X, pack)
    assert ferr.is_cuda and berr.is_cuda and ferr.numel() == 3 and berr.numel() == 3
    ferr, berr = ferr.cpu().numpy(), berr.cpu().numpy()
    bl = _berr_ld(a, b, x)
    print("n=%d kappa=%g berr %s (long double %s) ferr %s" % (n, kappa, berr, bl, ferr))
    # the rounding of an fp64 residual of n + 1 terms relative to its own denominator, and of the quotient
    assert (np.abs(berr - bl) <= (n + 2) * EPS).all(), np.abs(berr - bl) / EPS
    ainv = np.abs(np.linalg.inv(a))
    E = (ainv @ pm.ferr_weights(a, b, x)).max(axis=0) / np.abs(x).max(axis=0)
    print("   ferr / E %s" % (ferr / E))
    assert (0.5 * E <= ferr).all()
    assert (ferr <= E * ((1 + 1e-6) if kappa <= 1e6 else 1.01)).all()
    xs = _refine(a, b, x)
    actual = (np.abs(x - xs).max(axis=0) / np.abs(x).max(axis=0)).astype(np.float64)
    print("   actual error %s" % actual)
    assert (ferr >= actual).all()


@pytest.mark.parametrize("n,kappa", CASES)
def test_berr_of_a_perturbed_solution(n, kappa):
    from capital_amd import cholinv
    from capital_amd.matrix import matrix
    a, b, x, pack, A, B, X = _solved(n, kappa)
    xp = x * (1 + 1e-8 * np.random.default_rng(7).standard_normal(x.shape))
    Xp = matrix(3, n, 1, 1); Xp.from_numpy(xp)
    _, berr = cholinv.error_bounds(A, B, Xp, pack)
    berr = berr.cpu().numpy()
    bl = _berr_ld(a, b, xp)
    print("perturbed: berr %s long double %s" % (berr, bl))
    assert (bl > 1e-11).all()
    assert (np.abs(berr - bl) <= (n + 2) * EPS).all()


def test_chunks_of_sixteen_columns_a_zero_column_and_null_outputs():
    from capital_amd import _lib
    L = _lib.lib()
    n, nrhs = 129, 17
    a, b, x, pack, A, B, X = _solved(n, 1e2, nrhs)
    b = b.copy(); x = x.copy()
    b[:, 4] = 0.0; x[:, 4] = 0.0                                      # one all-zero column of B and X
    ld = n + 3
    st = torch.cuda.current_stream().cuda_stream

    def dev(m):
        buf = torch.full((m.shape[1], ld), NAN, dtype=torch.float64, device=DEV)
        buf[:, :n] = torch.from_numpy(np.ascontiguousarray(m.T)).to(DEV)
        return buf
    au = np.triu(a); au[np.tril_indices(n, -1)] = NAN                 # the strictly lower triangle is never read
    Ad, Bd, Xd = dev(au), dev(b), dev(x)
    ferr = torch.full((nrhs + 2,), -5.0, dtype=torch.float64, device=DEV)
    berr = torch.full((nrhs + 2,), -5.0, dtype=torch.float64, device=DEV)
    args = (pack._plan, Ad.data_ptr(), ld, Bd.data_ptr(), ld, Xd.data_ptr(), ld, nrhs)
    assert L.cap_cholinv_error_bounds(*args, ferr.data_ptr() + 8, berr.data_ptr() + 8, st) == OK
    f, e = ferr.cpu().numpy(), berr.cpu().numpy()
    assert f[0] == -5.0 and f[-1] == -5.0 and e[0] == -5.0 and e[-1] == -5.0
    f, e = f[1:-1], e[1:-1]
    bl = _berr_ld(a, b, x)
    assert (np.abs(e - bl) <= (n + 2) * EPS).all()
    R = np.triu(np.linalg.cholesky(a).T)
    fm = pm.ferr(a, R, b, x)
    print("zero column: berr %r ferr %r model %r %r" % (e[4], f[4], bl[4], fm[4]))
    assert e[4] == bl[4] == 1.0                                       # the guard: safe1 / safe1
    assert f[4] > 0 and abs(f[4] - fm[4]) <= 1e-6 * fm[4]             # x = 0: the bare estimate, as the model
    keep = np.arange(nrhs) != 4                                       # every chunk, against the quantity the estimator bounds from below
    E = (np.abs(np.linalg.inv(a)) @ pm.ferr_weights(a, b, x)).max(axis=0)[keep] / np.abs(x).max(axis=0)[keep]
    assert (0.5 * E <= f[keep]).all() and (f[keep] <= E * (1 + 1e-6)).all()
    # either output may be NULL
    f2 = torch.full((nrhs,), -5.0, dtype=torch.float64, device=DEV); e2 = torch.full((nrhs,), -5.0, dtype=torch.float64, device=DEV)
    assert L.cap_cholinv_error_bounds(*args, f2.data_ptr(), None, st) == OK
    assert L.cap_cholinv_error_bounds(*args, None, e2.data_ptr(), st) == OK
    assert np.array_equal(f2.cpu().numpy(), f) and np.array_equal(e2.cpu().numpy(), e)
    # the same through cap_dpoerr on the plan's factor
    ldr = C.c_int64(0)
    Rp = L.cap_cholinv_R_ptr(pack._plan, C.byref(ldr))
    w = NanWork(L.cap_dpoerr_work_size(n, nrhs))                      # all NaN, exactly the stated size, a sentinel behind it
    f3 = torch.empty(nrhs, dtype=torch.float64, device=DEV); e3 = torch.empty(nrhs, dtype=torch.float64, device=DEV)
    assert L.cap_dpoerr(1, n, nrhs, Ad.data_ptr(), ld, Rp, ldr.value, Bd.data_ptr(), ld, Xd.data_ptr(), ld, f3.data_ptr(), e3.data_ptr(),
                        w.data_ptr(), st) == OK
    w.check("cap_dpoerr")
    assert np.array_equal(f3.cpu().numpy(), f) and np.array_equal(e3.cpu().numpy(), e)
    for m, m0 in ((Ad, au), (Bd, b), (Xd, x)):
        assert np.array_equal(m[:, :n].cpu().numpy(), m0.T, equal_nan=True) and torch.isnan(m[:, n:]).all(), "an input was written"


def test_a_failed_factor_gives_nan():
    from capital_amd import cholinv
    from capital_amd.matrix import matrix
    n = 200
    a = pm.rand_spd(n, 1e2); a[n // 2, n // 2] = -1.0
    A = matrix(n, n, 1, 1); A.from_numpy(a)
    B = matrix(2, n, 1, 1); B.from_numpy(np.ones((n, 2)))
    pack = cholinv.info(-1, 1, -2, 'U')
    cholinv.factor(A, pack, None)
    ferr, berr = cholinv.error_bounds(A, B, B, pack)
    assert torch.isnan(ferr).all() and torch.isnan(berr).all()
    assert pack.last_info() != 0


def test_lapack_engine_entry_points():
    """lapack.engine._lansy / _pocon / _poerr on the plan's factor against cholinv.norm1 / rcond / error_bounds: the same kernels on the
    same operands, so the same bits"""
    from capital_amd import cholinv, lapack
    n = 300
    a, b, x, pack, A, B, X = _solved(n, 1e6)
    col, up = lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper
    an = lapack.engine._lansy(A.data(), n, A.ld(), lapack.ArgPack_lansy(col, up))
    assert an.is_cuda and an.numel() == 1 and an.item() == cholinv.norm1(A).item()
    for norm in ('O', 'I'):
        assert lapack.engine._lansy(A.data(), n, A.ld(), lapack.ArgPack_lansy(col, up, norm)).item() == an.item()
    R = cholinv.construct_R(pack)
    rc = lapack.engine._pocon(R.data(), n, R.ld(), an, lapack.ArgPack_pocon(col, up))
    assert rc.is_cuda and rc.numel() == 1 and rc.item() == cholinv.rcond(A, pack)
    ferr, berr = lapack.engine._poerr(A.data(), R.data(), B.data(), X.data(), n, 3, A.ld(), R.ld(), B.ld(), X.ld(), lapack.ArgPack_poerr(col, up))
    f0, b0 = cholinv.error_bounds(A, B, X, pack)
    assert ferr.numel() == 3 and berr.numel() == 3
    assert torch.equal(ferr, f0) and torch.equal(berr, b0)
