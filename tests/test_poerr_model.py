"""CPU-only: the NumPy model of the condition estimator (tests/poerr_model.py) against LAPACK's own dpocon, on the two families of test
matrices the GPU tests use - rand(n, kappa) and the tridiagonal lap(n), on which LAPACK's decision path is stable."""
import numpy as np
import pytest
import scipy.linalg as sl

from tests import poerr_model as pm

KAPPAS = (1e1, 1e4, 1e8, 1e12)


def _cases():
    for n in pm.NS:
        yield "lap", n, None
        for k in KAPPAS:
            yield "rand", n, k


@pytest.mark.parametrize("family,n,kappa", list(_cases()))
def test_model_matches_lapack_dpocon(family, n, kappa):
    A = pm.lap(n) if family == "lap" else pm.rand_spd(n, kappa)
    R = np.linalg.cholesky(A).T
    anorm = np.abs(A).sum(0).max()
    ref, info = sl.lapack.dpocon(R, anorm, uplo="U")
    assert info == 0
    got = pm.rcond(R, anorm)
    print("%s n=%d kappa=%s: model %.17g lapack %.17g rel %.2e" % (family, n, kappa, got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-12 * ref
    est, solves = pm.inv_norm_est(R)
    assert solves <= 11
    if family == "lap" or kappa <= 1e8:
        true = np.abs(np.linalg.inv(A)).sum(0).max()
        assert est <= true * (1 + 1e-6)


def test_edge_cases():
    R = np.eye(3)
    assert pm.rcond(np.zeros((0, 0)), 1.0) == 1.0
    assert pm.rcond(R, 0.0) == 0.0
    assert np.isnan(pm.rcond(R, float("nan")))
    assert pm.rcond(np.array([[2.0]]), 4.0) == 1.0


def test_bounds_of_a_zero_column_and_an_exact_solution():
    n = 40
    A = pm.rand_spd(n, 1e3)
    R = np.linalg.cholesky(A).T
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 2)); X[:, 1] = 0.0
    B = A @ X
    be = pm.berr(A, B, X)
    fe = pm.ferr(A, R, B, X)
    assert be[0] <= 4 * (n + 1) * pm.EPS and fe[0] > 0
    # x = 0, b = 0: the guard keeps the quotient finite - safe1 / safe1 - and ferr is the bare estimate of a tiny w
    assert be[1] == 1.0 and 0 < fe[1] < 1e-280
