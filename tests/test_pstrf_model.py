"""CPU-only: the NumPy model of the pivoted Cholesky factorization (tests/pstrf_model.py) on every fixture matrix of tests/test_gpu_pstrf.py.
The model's own output has to pass the property checks the kernel is held to, and the premises of the GPU tests - detected ranks, pivot
gaps far above the rounding level, a clear stopping decision - have to hold, so that those tests ask something a correct kernel can meet."""
import numpy as np
import pytest

from tests import pstrf_model as pm

GRAM = [(300, 40), (513, 64), (1030, 17), (63, 9), (64, 9), (129, 12)]
DOMINANT = [65, 200]
SEEDS = (1, 2, 3)


def _premises(A, rank, trace):
    """what makes `piv`, `rank` and `info` of a correct kernel equal to the model's: every pivot wins by more than the rounding errors of
    two different summation orders can move a remaining diagonal entry, and the stopping decision is as clear"""
    md = np.diag(A).max()
    g = pm.gamma(rank + 2)
    assert pm.min_gap(trace) >= 64 * g * md
    tol = pm.default_tol(A)
    if trace["picks"]:
        assert trace["picks"][-1][0] >= tol + 64 * g * md
    if trace["stop"] is not None:
        assert trace["stop"] + 4 * g * md <= tol


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,k", GRAM)
def test_gram_matrices(n, k, seed):
    A = pm.gram(n, k, seed)
    R, piv, rank, resid, info, trace = pm.pstrf(A)
    assert (rank, info) == (k, 0)
    _premises(A, rank, trace)
    assert trace["picks"][-1][0] >= 1e7 * pm.default_tol(A)
    ratio = pm.check_properties(A, R, piv, rank, info, pm.default_tol(A))
    print("gram %d x %d seed %d: backward error %.3f of the bound" % (n, k, seed, ratio))
    assert abs(resid - pm.remaining_diagonal(A, R, piv, rank).sum()) <= 2 * pm.gamma(n) * np.trace(A)
    # the capped form gives the same leading rows
    R2, piv2, rank2, resid2, info2, _ = pm.pstrf(A, k // 2)
    assert (rank2, info2) == (k // 2, 1) and np.array_equal(piv2[:rank2], piv[:rank2]) and resid2 > resid
    assert np.array_equal(R2[:, np.argsort(piv2)], R[:k // 2][:, np.argsort(piv)])
    pm.check_properties(A, R2, piv2, rank2, info2, pm.default_tol(A))


@pytest.mark.parametrize("n,seed", [(n, s) for n in DOMINANT for s in SEEDS] + [(1100, 3)])
def test_full_rank_matrices(n, seed):
    A = pm.dominant(n, seed)
    R, piv, rank, resid, info, trace = pm.pstrf(A)
    assert (rank, info, resid) == (n, 0, 0.0)
    _premises(A, rank, trace)
    rows = None if n <= 600 else pm.sample_rows(rank)
    ratio = pm.check_properties(A, R, piv, rank, info, pm.default_tol(A), rows)
    print("dominant %d seed %d: backward error %.3f of the bound" % (n, seed, ratio))
    assert np.allclose(R.T @ R, A[np.ix_(piv, piv)], rtol=0, atol=1e-12)


@pytest.mark.parametrize("seed", SEEDS)
def test_rbf_kernel_matrix(seed):
    A = pm.rbf(400, seed)
    R, piv, rank, resid, info, trace = pm.pstrf(A)
    assert info == 0 and 10 < rank < 100
    ratio = pm.check_properties(A, R, piv, rank, info, pm.default_tol(A))
    print("rbf seed %d: rank %d, backward error %.3f of the bound, trace of the remainder %.2e" % (seed, rank, ratio, resid))
    assert 0 <= resid <= 400 * pm.default_tol(A)


def test_exact_cases():
    for n in (1, 2, 63, 64, 65, 130):
        A = pm.squares(n)
        want = np.argsort(-np.diag(A), kind="stable")
        for mr in sorted({0, 1, n // 2, n}):
            R, piv, rank, resid, info, _ = pm.pstrf(A, mr)
            assert rank == mr and info == (0 if mr == n else 1)
            assert np.array_equal(piv[:mr], want[:mr]) and np.array_equal(piv[mr:], np.sort(want[mr:]))
            assert np.array_equal(R[:, :mr], np.diag(np.sqrt(np.diag(A)[want[:mr]]))) and np.all(R[:, mr:] == 0)
            assert resid == np.diag(A)[want[mr:]].sum()
    R, piv, rank, resid, info, _ = pm.pstrf(2.0 * np.eye(130))
    assert np.array_equal(piv, np.arange(130)) and rank == 130 and info == 0 and np.array_equal(R, np.sqrt(2.0) * np.eye(130))
    for n in (2, 7, 12):
        for flip in (0, 1, 2):
            A, T, perm = pm.exact_integer(n, flip)
            assert np.argmax(np.diag(A)) == (0, n - 1, perm[0])[flip]
            for mr in (n, n // 2):
                R, piv, rank, resid, info, _ = pm.pstrf(A, mr)
                assert rank == mr and np.array_equal(piv[:mr], perm[:mr])
                assert np.array_equal(R[:, np.argsort(piv)], T[:mr][:, np.argsort(perm)])        # both in natural column order


def test_stopping_rules():
    A = pm.graded(80, 6, 1)
    picks = [b for b, _ in pm.pstrf(A)[5]["picks"]]
    assert len(picks) == 6
    tol = pm.tol_between(picks, 3)
    R, piv, rank, resid, info, _ = pm.pstrf(A, None, tol)
    assert (rank, info) == (3, 0)
    pm.check_properties(A, R, piv, rank, info, tol)
    Z = np.zeros((70, 70))
    R, piv, rank, resid, info, _ = pm.pstrf(Z)
    assert (rank, info, resid) == (0, 0, 0.0) and np.array_equal(piv, np.arange(70)) and np.all(R == 0)
    R, piv, rank, resid, info, _ = pm.pstrf(pm.dominant(65, 1), 0)
    assert (rank, info) == (0, 1) and np.array_equal(piv, np.arange(65)) and R.shape == (0, 65)
    assert abs(resid - np.trace(pm.dominant(65, 1))) <= 65 * pm.EPS * resid


def test_nan_is_reported():
    A = pm.dominant(65, 1).copy()
    A[3, 40] = np.nan                                   # upper triangle: read when 3 or 40 becomes the pivot
    R, piv, rank, resid, info, _ = pm.pstrf(A)
    assert info == 2 and 0 < rank < 65
    assert 3 in piv[:rank] or 40 in piv[:rank]
    B = pm.dominant(65, 1).copy()
    B[40, 3] = np.nan                                   # strictly lower triangle: never read
    assert pm.pstrf(B)[4] == 0
    B[7, 7] = np.nan
    assert pm.pstrf(B)[2:5:2] == (0, 2)
