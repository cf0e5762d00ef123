"""No GPU: the operands of tests/potri_batched_cases.py are what they claim to be.
 * the exactness premise holds for every block of every row the GPU test uses (block() asserts it; here every row is built);
 * at n <= 40 the references T^-1 and triu(T^-1 T^-T) are recomputed with fractions.Fraction, and so is the chain's A = T^T T;
 * LAPACK on the CPU (scipy's dtrtri / dpotri) stays inside the two componentwise bounds of the random-block test on the very blocks that
   test uses - the bounds are ones a correct implementation meets."""
from fractions import Fraction

import numpy as np
import pytest

from tests import potri_batched_cases as P

ROWS = P.exact_rows()


def test_rows_cover_every_size_family_and_path():
    seen = {(r[0], r[1]) for r in ROWS}
    for n in P.SMALL_N + P.LARGE_N:
        for fam in P.FAMILIES:
            assert (n, fam) in seen
    assert {r[2] for r in ROWS if r[0] <= 64} >= set(P.SMALL_BATCHES) and {r[2] for r in ROWS if r[0] > 64} >= set(P.LARGE_BATCHES)
    assert {r[3] for r in ROWS} == set(P.LAYOUTS)
    odd = {r[0] for r in ROWS if (r[0] + r[3][0]) % 2 == 1}
    assert {8, 16, 32, 64} <= {8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64 for n in odd if n <= 64}     # every NP
    assert {2, 3, 4} <= {(n + 63) // 64 for n in odd if n > 64}                                                        # every NBLK


@pytest.mark.parametrize("signed", (True, False))
def test_premise_of_every_row(signed):
    for n, fam, batch, _ in ROWS:
        M, Mi, C = P.batch(fam, n, signed, min(batch, 9) if n > 64 else batch)
        assert M.shape == Mi.shape == C.shape
        assert not np.any(np.tril(M, -1)) and not np.any(np.tril(C, -1))
        if batch > 1:
            assert n == 1 or not np.array_equal(M[0], M[1]) or fam != "F1" or n < 4      # the blocks of a batch differ
        if not signed:
            assert np.all(np.diagonal(M, axis1=1, axis2=2) > 0)


def _frac(a):
    return [[Fraction(float(v)) for v in row] for row in a]


def _matmul(a, b):
    n, m, p = len(a), len(b), len(b[0])
    return [[sum((a[i][k] * b[k][j] for k in range(m) if a[i][k] and b[k][j]), Fraction(0)) for j in range(p)] for i in range(n)]


@pytest.mark.parametrize("fam", P.FAMILIES)
@pytest.mark.parametrize("n", [n for n in P.SMALL_N if n <= 40])
def test_references_in_exact_arithmetic(fam, n):
    for signed in (True, False):
        for idx in (0, 1, 4):
            M, Mi, C = P.block(fam, n, signed, idx)
            fm, fi = _frac(M), _frac(Mi)
            eye = [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]
            assert _matmul(fm, fi) == eye and _matmul(fi, fm) == eye
            fit = [list(r) for r in zip(*fi)]
            prod = _matmul(fi, fit)
            for i in range(n):
                for j in range(n):
                    assert Fraction(float(C[i, j])) == (prod[i][j] if i <= j else 0)
            if not signed:                  # the chain's input, formed in float64, is the exact T^T T
                fmt = [list(r) for r in zip(*fm)]
                assert _frac(M.T @ M) == _matmul(fmt, fm)


@pytest.mark.parametrize("kappa", P.KAPPAS)
@pytest.mark.parametrize("n", P.RANDOM_N)
def test_lapack_meets_the_componentwise_bounds(n, kappa):
    from scipy.linalg import lapack
    for A in P.random_spd(n, kappa, 2):
        R = np.linalg.cholesky(A).T
        W, info = lapack.dtrtri(np.asfortranarray(R), lower=0, unitdiag=0)
        assert info == 0
        X, info = lapack.dpotri(np.asfortranarray(R), lower=0)
        assert info == 0
        fw, fx = P.check_random(R, np.triu(W), np.triu(X))          # asserts both bounds
        print("n = %d kappa = %g: LAPACK uses %.3f / %.3f of the bounds" % (n, kappa, fw, fx))
