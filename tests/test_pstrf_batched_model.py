"""CPU-only: the premises of the batched pivoted Cholesky tests.  The Fraction model (tests/pstrf_batched_model.py - the stated recurrence
of cap_dpstrf_batched, which the kernel is held to bit for bit) passes pstrf_model.check_properties on the fixtures the GPU tests use,
picks the pivots, rank and info of the NumPy model and of SciPy's dpstrf on them with the stated pivot gap, and reproduces the exact
families exactly."""
import numpy as np
import pytest

from tests import pstrf_batched_cases as PC
from tests import pstrf_batched_model as bm
from tests import pstrf_model as pm


@pytest.mark.parametrize("kind,args", PC.FIXTURES + PC.MORE)
def test_model_agrees_with_the_numpy_model_and_lapack(kind, args):
    from scipy.linalg import lapack
    A = PC.matrix(kind, args)
    n = A.shape[0]
    R, piv, rank, resid, info = bm.pstrf(A)
    Rm, pivm, rankm, residm, infom, trace = pm.pstrf(A)
    assert (rank, info) == (rankm, infom) and np.array_equal(piv, pivm)
    c, lp, lrank, linfo = lapack.dpstrf(A)                   # LAPACK: info 1 = rank deficient; its tail of piv is in swap order
    assert lrank == rank and np.array_equal(lp[:rank] - 1, piv[:rank]) and linfo == (1 if rank < n else 0)
    gap = min(((b - s) / b for b, s in trace["picks"]), default=np.inf)
    print("%s%s: rank %d, smallest relative pivot gap %.3g" % (kind, args, rank, gap))
    if kind == "rbf":
        assert gap == 0.0                                    # exact ties: the tie-break fixture
    else:
        assert gap >= PC.MIN_GAP
    assert np.abs(R - Rm).max() <= 1e-8 * np.abs(Rm).max()
    assert bm.tol_used(A) == pm.default_tol(A)


@pytest.mark.parametrize("kind,args", PC.FIXTURES + PC.MORE)
def test_model_has_the_properties(kind, args):
    A = PC.matrix(kind, args)
    if kind == "graded":                                     # the pivots fall into the noise of the largest entry: an absolute tolerance, as test_gpu_pstrf.py
        k = 3
        tol = pm.tol_between(bm.picks(A), k)
        R, piv, rank, resid, info = bm.pstrf(A, None, tol)
        assert (rank, info) == (k, 0)
        pm.check_properties(A, R, piv, rank, info, tol)
        return
    n = A.shape[0]
    for mr in (n, n // 2):
        R, piv, rank, resid, info = bm.pstrf(A, mr)
        pm.check_properties(A, R, piv, rank, info, pm.default_tol(A))
        mine = pm.remaining_diagonal(A, R, piv, rank).sum()
        assert abs(resid - mine) <= 2 * pm.gamma(n) * np.trace(A)


@pytest.mark.parametrize("n", PC.SIZES)
def test_model_reproduces_the_exact_families(n):
    for which in PC.FAMILY:
        A = PC.exact_matrix(n, which)
        for mr in PC.caps(n):
            got = bm.pstrf(A, mr)
            if which == "squares" or n <= PC.EXACT_KNOWN_MAX:
                R, piv, rank, resid, info = PC.known_answer(n, which, mr)
                assert got[2] == mr and got[4] == (0 if mr == n else 1), (which, mr)
                assert PC.same(got[0], R) and np.array_equal(got[1], piv) and got[3] == resid, (which, mr)
            else:                            # 2^(2n) is beyond 53 bits: an ordinary matrix whose small pivots lie below n eps max_i a_ii
                assert got[2] <= mr and got[4] in (0, 1), (which, mr)
                pm.check_properties(A, got[0], got[1], got[2], got[4], pm.default_tol(A))


def test_model_stopping_rules_and_nan():
    n = 9
    assert bm.pstrf(np.zeros((n, n)))[2:] == (0, 0.0, 0)
    R, piv, rank, resid, info = bm.pstrf(-np.eye(n), None, 0.0)
    assert (rank, info, resid) == (0, 0, -float(n)) and np.array_equal(piv, np.arange(n))
    R, piv, rank, resid, info = bm.pstrf(np.diag([-1.0, 0.0, -3.0]))                 # default tolerance: 3 eps max = 0
    assert (rank, info, resid) == (0, 0, -4.0)
    R, piv, rank, resid, info = bm.pstrf(2.0 * np.eye(n))
    assert np.array_equal(piv, np.arange(n)) and (rank, info, resid) == (n, 0, 0.0) and PC.same(R, np.sqrt(2.0) * np.eye(n))
    A = pm.dominant(n, 3).copy()
    order = bm.pstrf(A)[1]
    A[min(order[2], order[5]), max(order[2], order[5])] = np.nan                     # read when the third pivot is taken
    R, piv, rank, resid, info = bm.pstrf(A)
    assert (rank, info) == (3, 2) and np.array_equal(piv[:3], order[:3]) and np.isnan(resid) and np.isnan(bm.logdet(R, rank, info))
    A = pm.dominant(n, 3).copy()
    A[4, 4] = np.nan
    assert bm.pstrf(A)[2::2] == (0, 2)
    A, Tk, perm = PC.semidefinite_integer(12, 5, 2)
    R, piv, rank, resid, info = bm.pstrf(A)
    assert (rank, info, resid) == (5, 0, 0.0) and np.array_equal(piv[:5], perm[:5]) and PC.same(R[:5][:, np.argsort(piv)], Tk[:, np.argsort(perm)])
