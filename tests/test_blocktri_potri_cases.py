"""CPU-only: the table and the exact family of the batched block-tridiagonal selected inverse tests (tests/blocktri_potri_cases.py).  The
table covers what it says it covers; every exact row's premise - no sum the kernel or the host-driven composition forms can round, in
any order - is PROVED in exact integer arithmetic while the row is built (exact_chain raises otherwise); the closed forms are the
block-tridiagonal part of the inverse of the assembled matrix, checked in exact rational arithmetic on the small rows and against a
longdouble inverse on the others; and the two evaluations of the recurrence the accuracy test compares agree with that inverse."""
from fractions import Fraction

import numpy as np
import pytest

from tests import blocktri_cases as BC
from tests import blocktri_potri_cases as IC


def _inverse(A):
    """Gauss-Jordan on Fractions"""
    N = len(A)
    M = [list(r) + [Fraction(int(a == b)) for b in range(N)] for a, r in enumerate(A)]
    for a in range(N):
        p = next(r for r in range(a, N) if M[r][a] != 0)
        M[a], M[p] = M[p], M[a]
        M[a] = [v / M[a][a] for v in M[a]]
        for r in range(N):
            if r != a and M[r][a] != 0:
                M[r] = [v - M[r][a] * w for v, w in zip(M[r], M[a])]
    return [r[N:] for r in M]


def test_the_table_covers_every_class_edge_chain_length_layout_and_fill():
    rows = IC.rows()
    assert {r[0] for r in rows} == set(BC.NS) == {1, 3, 8, 9, 16, 17, 32, 33, 63, 64}
    assert {r[1] for r in rows} == {1, 2, 3, 5, 257} and {r[4] for r in rows} == set(BC.LAYOUTS)
    for n in BC.NS:
        assert {r[3] for r in rows if r[0] == n} == {0, 1} and {r[1] for r in rows if r[0] == n} >= {1, 2, 3, 5}
    for T in BC.TS:
        assert {r[3] for r in rows if r[1] == T} == {0, 1}
    for NP in (8, 16, 32, 64):
        G = 64 // NP
        assert {r[2] for r in rows if BC.padded(r[0]) == NP} >= {1, 2 * G + 1}
    assert any(r[2] % (64 // BC.padded(r[0])) for r in rows if BC.padded(r[0]) < 64)       # a ragged last wavefront
    assert max(r[0] * r[1] for r in rows) <= 2056
    ex = IC.exact_rows()
    assert {(r[0], r[1]) for r, fam in ex if fam == "F2"} == {(n, T) for n in BC.NS for T in BC.TS}
    for fam in ("F1", "F2i"):
        assert {(r[0], r[1]) for r, f in ex if f == fam} >= {(n, T) for n in BC.NS for T in (2, 3)}
    assert {r[0] for r, f in ex if f != "F2" and r[1] == 1} == set(BC.NS)
    assert all(r[1] != 257 for r, _ in ex)


@pytest.mark.parametrize("row,fam", IC.exact_rows(), ids=lambda v: IC.row_id(v) if isinstance(v, tuple) else v)
def test_exact_rows_cannot_round_and_are_the_inverse(row, fam):
    n, T, batch, _, _ = row
    U, W, Sd, Sc, worst = IC.exact_chain(row, fam)                      # raises where a bound reaches 2^53
    assert worst < 53
    assert np.all(np.triu(U) == U) and np.all(np.diagonal(U, axis1=-2, axis2=-1) > 0)
    if T > 1:                                                           # W: one entry of +-{1/2, 1, 2} per row and column
        assert np.all((np.abs(W) > 0).sum(axis=-1) == 1) and np.all((np.abs(W) > 0).sum(axis=-2) == 1)
        assert set(np.unique(np.abs(W))) <= {0.0, 0.5, 1.0, 2.0}
    assert np.array_equal(Sd, np.swapaxes(Sd, -1, -2))
    R = BC.dense_factor(U, W)
    for c in range(batch):
        S = np.zeros((T * n, T * n))                                    # the band of Sigma from the closed forms
        for i in range(T):
            S[i * n:(i + 1) * n, i * n:(i + 1) * n] = Sd[c, i]
            if i + 1 < T:
                S[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = Sc[c, i]
                S[(i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] = Sc[c, i].T
        band = np.abs(np.arange(T * n)[:, None] // n - np.arange(T * n)[None, :] // n) <= 1
        if T * n <= 24 and c == 0:
            N = T * n                                                   # exactly: the inverse of R^T R in rational arithmetic
            Rf = [[Fraction(float(v)) for v in r] for r in R[c]]
            A = [[sum(Rf[k][a] * Rf[k][b] for k in range(N)) for b in range(N)] for a in range(N)]
            X = _inverse(A)
            assert all(Fraction(float(S[a, b])) == X[a][b] for a in range(N) for b in range(N) if band[a, b]), "closed forms"
        else:
            Rl = R[c].astype(np.longdouble)                             # Sigma = R^-1 R^-T, R^-1 by substitution in longdouble
            V = np.eye(T * n, dtype=np.longdouble)
            for j in range(T * n - 1, -1, -1):
                V[j] = (V[j] - Rl[j, j + 1:] @ V[j + 1:]) / Rl[j, j]
            X = V @ V.T
            err = np.max(np.abs(X - S)[band]) / np.max(np.abs(S))
            assert err < 1e-10, err


@pytest.mark.parametrize("row", [r for r in IC.random_rows() if r[0] in (3, 9, 17, 33) and r[1] in (2, 3, 5)], ids=IC.row_id)
def test_both_evaluations_of_the_recurrence_agree_with_the_inverse(row):
    """the yardsticks of the accuracy test: reference() in longdouble and in fp64 against a dense inverse of a random chain"""
    n, T, batch, _, _ = row
    D, Bc, _ = BC.random_chain((n, T, batch, 1, row[4]))
    A = BC.dense(D, Bc)[0]
    L = np.linalg.cholesky(A)
    R = L.T
    U = np.stack([np.triu(R[i * n:(i + 1) * n, i * n:(i + 1) * n]) for i in range(T)])
    W = np.stack([R[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] for i in range(T - 1)])
    X = np.linalg.inv(R.T @ R)
    for dtype, tol in ((np.longdouble, 1e-12), (np.float64, 1e-12)):
        Sd, Sc = IC.reference(U, W, dtype)
        for i in range(T):
            assert np.max(np.abs(Sd[i] - X[i * n:(i + 1) * n, i * n:(i + 1) * n])) <= tol * np.max(np.abs(X))
            if i + 1 < T:
                assert np.max(np.abs(Sc[i] - X[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n])) <= tol * np.max(np.abs(X))
