"""The row sweep of the Cholesky update / downdate (tests/cholupdate_model.py) checked on its own, without a GPU, against
np.linalg.cholesky(A +- V V^T).  Inputs with cond(A') < 10; the model's own errors there are <= 6.4e-16 backward (update), 5.2e-16
(round-trip downdate) and 3.8e-16 elementwise, so the gates (1e-14 / 1e-13) leave a 15-fold margin for another summation order."""
import numpy as np
import pytest

from tests import cholupdate_model as cm

CASES = [(1, 1), (2, 5), (63, 5), (64, 16), (65, 1), (128, 16), (129, 17), (300, 1), (517, 40), (1100, 16)]


@pytest.mark.parametrize("n,k", CASES)
def test_update_matches_cholesky_and_downdate_returns(n, k):
    A, V = cm.spd(n, 10 + n), cm.thin(n, k, 100 + n)
    A1 = A + V @ V.T
    assert np.linalg.cond(A1) < 10
    R = np.linalg.cholesky(A).T
    R1, i1 = cm.sweep(R, V, +1.0)
    ref = np.linalg.cholesky(A1).T
    e_b, e_e = cm.backward_error(R1, A1), cm.element_error(R1, ref)
    R2, i2 = cm.sweep(R1, V, -1.0)
    d_b, d_e = cm.backward_error(R2, A), cm.element_error(R2, R)
    print("n=%d k=%d: update backward %.2e elementwise %.2e | downdate backward %.2e elementwise %.2e" % (n, k, e_b, e_e, d_b, d_e))
    assert i1 == 0 and i2 == 0
    assert np.array_equal(np.tril(R1, -1), np.zeros((n, n)))
    assert e_b <= cm.BACKWARD_GATE and d_b <= cm.BACKWARD_GATE
    assert e_e <= cm.ELEMENT_GATE and d_e <= cm.ELEMENT_GATE


def test_passes_of_16_are_consecutive_updates():
    n, k = 100, 40
    A, V = cm.spd(n, 3), cm.thin(n, k, 4)
    R = np.linalg.cholesky(A).T
    whole, _ = cm.sweep(R, V, +1.0)
    step = R
    for k0 in range(0, k, cm.PASS):
        step, info = cm.sweep(step, V[:, k0:k0 + cm.PASS], +1.0)
        assert info == 0
    assert np.array_equal(whole, step)


@pytest.mark.parametrize("r0", [0, 127, 128, 299])
def test_failing_downdate_reports_its_row(r0):
    """V = 1.5 x (row r0 of R)^T: rows above r0 see w_r = 0 and keep their bits, row r0 has rho^2 = R_rr^2 (1 - 2.25) < 0"""
    n = 300
    R = np.linalg.cholesky(cm.spd(n, 9)).T
    V = 1.5 * R[r0, :].reshape(n, 1)
    Rf, info = cm.sweep(R, V, -1.0)
    assert info == r0 + 1
    assert np.array_equal(Rf[:r0], R[:r0])
    assert np.isnan(Rf[r0, r0])


def test_lower_triangle_is_ignored():
    n = 70
    A, V = cm.spd(n, 5), cm.thin(n, 3, 6)
    R = np.linalg.cholesky(A).T
    Rn = R + np.tril(np.full((n, n), np.nan), -1)
    R1, _ = cm.sweep(R, V, +1.0)
    R2, _ = cm.sweep(Rn, V, +1.0)
    assert np.array_equal(np.triu(R1), np.triu(R2)) and np.isnan(np.tril(R2, -1)[np.tril_indices(n, -1)]).all()
