"""CPU-only: the premises of tests/symm_batched_cases.py, checked in NumPy for every row the GPU tests use - so that a GPU failure is the
kernel's, never the operands'.  1. every exact row: partial sums in any order stay below 2^53 (integer data, dyadic coefficients) and two
different summation orders of NumPy agree with the reference bit for bit; 2. the row list reaches every n, every nrhs on both paths,
beta == 0 and != 0, absolute and plain, in place; 3. the bound formulas agree with tests/poerr_model.py where the two state the same thing;
4. the integer SPD systems: B = A x* exactly, and NumPy's own solve satisfies the inequality the GPU test asserts; 5. the norms of the exact
factor families sum exactly."""
import numpy as np
import pytest

from tests import poerr_model as PM
from tests import potri_batched_cases as P
from tests import symm_batched_cases as SC


def test_every_exact_row_has_one_answer_whatever_the_summation_order():
    for row in SC.exact_rows():
        n, nrhs, batch, absolute, (alpha, beta), la, lx, inplace = row
        for i in range(min(batch, 7)):
            A, X, B = SC.operands(n, nrhs, i)
            assert np.array_equal(A, A.T) and SC.premise(A, X, B, alpha, beta) < SC.LIMIT
            want = SC.expected(A, X, B, alpha, beta, absolute)
            Aa, Xa, Ba = (np.abs(m) for m in (A, X, B)) if absolute else (A, X, B)
            back = alpha * (Aa[:, ::-1] @ Xa[::-1, :])                           # K descending
            rows = np.zeros((n, nrhs))
            for k in range(n):                                                   # one rank-1 term at a time, K ascending
                rows += np.outer(Aa[:, k], Xa[k, :])
            for other in (back, alpha * rows):
                got = other if beta == 0.0 else beta * Ba + other
                assert np.array_equal(got, want), SC.row_id(row)


def test_the_rows_reach_every_path():
    rows = SC.exact_rows()
    assert {r[0] for r in rows} == set(SC.WAVE_N) | set(SC.GROUP_N)
    for lo, hi in ((1, 64), (65, 256)):
        part = [r for r in rows if lo <= r[0] <= hi]
        assert {r[1] for r in part} == set(SC.NRHS)
        assert {r[3] for r in part} == {0, 1} and {r[4][1] == 0.0 for r in part} == {True, False} and any(r[7] for r in part)
        assert {r[5] for r in part} == set(SC.LAYOUTS)
    assert {r[2] for r in rows if r[0] <= 64} == set(SC.WAVE_BATCHES) and {r[2] for r in rows if r[0] > 64} == set(SC.GROUP_BATCHES)
    assert len({SC.row_id(r) for r in rows}) == len(rows)


@pytest.mark.parametrize("n", (1, 7, 64, 130))
def test_the_bound_formulas_agree_with_the_single_matrix_model(n):
    rng = np.random.default_rng([12, n])
    A = PM.rand_spd(n, 1e3, seed=1)
    X = rng.standard_normal((n, 4))
    X[:, 1] = 0.0
    B = A @ X * (1 + 1e-12 * rng.standard_normal((n, 4)))
    B[:, 1] = 0.0                                                                # a column under the guard: r = s = 0
    r, s = B - A @ X, np.abs(A) @ np.abs(X) + np.abs(B)
    assert np.array_equal(SC.berr(r, s, n), PM.berr(A, B, X))
    assert SC.berr(r, s, n)[1] == 1.0                                            # (0 + safe1) / (0 + safe1), as LAPACK
    safe1, safe2 = SC.safe(n)
    assert (safe1, safe2) == PM.safe(n) and SC.EPS == PM.EPS and SC.SAFMIN == PM.SAFMIN
    w = SC.weights(r, s, n)
    assert np.array_equal(w[:, [0, 2, 3]], PM.ferr_weights(A, B, X)[:, [0, 2, 3]])       # above the guard the two are the same numbers
    assert np.array_equal(SC.ferr(w, X)[1], w[:, 1].max())                       # x_j = 0: the numerator alone
    bad = np.array(w)
    bad[n // 2, 0] = np.nan
    assert np.isnan(SC.ferr(bad, X)[0]) and np.isnan(SC.nanmax(bad, 0)[0]) and not np.isnan(SC.nanmax(bad, 0)[2])
    assert SC.norm1(A) == np.abs(A).sum(axis=0).max() and SC.norm1(np.zeros((0, 0))) == 0.0


@pytest.mark.parametrize("n,count", ((7, 4), (8, 3), (16, 3), (33, 4), (64, 3), (65, 3), (129, 2), (256, 2)))
def test_integer_spd_systems_are_exact_and_solvable_within_the_bound(n, count):
    for i in range(count):
        A, xs, B = SC.spd_system(n, 3, i)
        assert np.array_equal(A, A.T) and np.array_equal(A, np.round(A)) and np.array_equal(xs, np.round(xs))
        assert np.abs(A).sum(axis=1).max() * np.abs(xs).max() * 2 < SC.LIMIT and np.array_equal(B, A @ xs)
        assert np.linalg.eigvalsh(A).min() >= 1.0 - 1e-9                         # M M^T + I
        assert np.abs(xs).max(axis=0).min() > 0


def test_the_norms_of_the_exact_factor_families_sum_exactly():
    for k, n in enumerate((1, 2, 7, 8, 9, 16, 17, 33, 63, 64, 65, 96, 129, 200, 255, 256)):
        fam = P.FAMILIES[k % 3]
        T, Ti, C = P.batch(fam, n, False, 2)
        for i in range(2):
            assert SC.sums_exact(SC.sym(C[i])) and SC.sums_exact(T[i].T @ T[i])
            assert np.array_equal(SC.sym(C[i]), Ti[i] @ Ti[i].T)
    assert not SC.sums_exact(np.array([[1.0, 2.0 ** -60], [2.0 ** -60, 2.0 ** 60]]))
