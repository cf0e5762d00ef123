"""CPU-only: the premise of tests/test_gpu_blocktri_batched.py's EXACT test, for every exact row of tests/blocktri_cases.py.  The
recurrence of csrc/blocktri_batched.hip - factor step by step, forward substitution on the coupling block, successor update, both sweeps
of the solve - is replayed in exact arithmetic and every number it forms must be exactly representable in fp64: then no operation of the
kernel rounds, whatever the order of its sums, the factor is R itself and the solution X itself.
The exact family scales by 2^k with k >= 0, so every intermediate is an INTEGER: the replay of all rows and all chains runs on int64
arrays (every value held below 2^53 in magnitude, every division checked to leave no remainder, and for the products on the MFMA - whose
order of the four terms of an instruction is the hardware's - the sum of the MAGNITUDES of the terms held below 2^53 as well, which bounds
every partial sum of every order).  The first chain of every row of up to 9 rows per block is replayed in fractions.Fraction as well,
with no assumption on integrality: every intermediate must convert to a float and back without change."""
from fractions import Fraction
from math import isqrt

import numpy as np
import pytest

from tests import blocktri_cases as BC

LIMIT = 2 ** 53
ROWS = BC.exact_rows()
IDS = ["n%d-T%d-b%d-k%d-%s" % r for r in ROWS]


def test_the_table_covers_what_the_kernels_distinguish():
    rows = BC.rows()
    assert len(rows) == len(set(rows))
    for NP in (8, 16, 32, 64):
        mine = [r for r in rows if BC.padded(r[0]) == NP]
        G = 64 // NP
        assert {r[0] for r in mine} >= {NP, NP // 2 + 1 if NP > 8 else 1}              # the upper edge and one above the class below
        assert {r[1] for r in mine} >= {1, 2, 3, 5}
        assert {1, 2 * G + 1} <= {r[2] for r in mine} and G in {r[2] for r in mine}     # a lone chain, a full wavefront, a ragged last one
    assert {r[3] for r in rows} >= {1, 3, 16, 17} and {BC.padded(r[0]) for r in rows if r[3] == 17} == {8, 16, 32, 64}
    assert any(r[3] > 64 for r in rows) and any(r[1] == 257 for r in rows) and {r[4] for r in rows} == set(BC.LAYOUTS)
    for r in rows:
        ldd, step_d, stride_d, lde, step_e, stride_e, ldb, stride_b = BC.layout(r)
        n, T, batch, nrhs, _ = r
        assert ldd >= n and step_d >= ldd * n and stride_d >= step_d * T and stride_e >= step_e * max(T - 1, 1) and ldb >= T * n and stride_b >= ldb * nrhs


class Exact:
    """the arithmetic of one replay: int64 arrays (batched) or object arrays of Fractions"""

    def __init__(self, frac):
        self.frac = frac

    def arr(self, a):
        if not self.frac:
            return np.array(a, dtype=np.int64)
        out = np.empty(np.shape(a), dtype=object)
        flat = out.reshape(-1)
        for i, v in enumerate(np.asarray(a).reshape(-1)):
            flat[i] = Fraction(int(v))
        return out

    def fits(self, a):
        if not self.frac:
            assert (np.abs(a) < LIMIT).all()
        else:
            for v in np.asarray(a, dtype=object).reshape(-1):
                assert Fraction(float(v)) == v
        return a

    def sqrt(self, d):
        if not self.frac:
            assert (d > 0).all()
            r = np.rint(np.sqrt(d.astype(np.float64))).astype(np.int64)
            assert (r * r == d).all()
            return r
        out = np.empty_like(d)
        for i, v in enumerate(d.reshape(-1)):
            assert v > 0 and v.denominator == 1
            r = isqrt(v.numerator)
            assert r * r == v.numerator
            out.reshape(-1)[i] = Fraction(r)
        return out

    def div(self, a, d):
        if self.frac:
            return self.fits(a / d)
        assert (a % d == 0).all()
        return a // d

    def dot(self, a, b):
        """a @ b with the sum of the magnitudes of the terms of every element below 2^53: no partial sum of any order can round"""
        if self.frac:
            assert all(v < LIMIT for v in (np.abs(a) @ np.abs(b)).reshape(-1))
        else:                                # magnitudes far below 2^53: their float sums are exact or overestimate by a few ulps
            assert (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64) < LIMIT / 2).all()
        return self.fits(a @ b)


def replay(ex, D, Bc, rhs):
    """-> U, W, X of the chains, every intermediate checked; arrays are [chain, position, row, col], column-major reading"""
    batch, T, n, _ = D.shape
    D, Bc, rhs = ex.arr(D), ex.arr(Bc), ex.arr(rhs)
    U, W = np.zeros_like(D), np.zeros_like(Bc)
    S = D[:, 0].copy()
    for i in range(T):
        for j in range(n):                                   # pb_factor_step
            r = ex.sqrt(S[:, j, j])
            row = ex.div(S[:, j, j:], r[:, None])
            row[:, 0] = r
            U[:, i, j, j:] = row
            S[:, j + 1:, j + 1:] = ex.fits(S[:, j + 1:, j + 1:] - row[:, 1:, None] * row[:, None, 1:])
        if i + 1 < T:
            B = Bc[:, i].copy()
            for j in range(n):                               # pb_forward_step on every column
                B[:, j] = ex.div(B[:, j], U[:, i, j, j, None])
                B[:, j + 1:] = ex.fits(B[:, j + 1:] - U[:, i, j, j + 1:, None] * B[:, j, None, :])
            W[:, i] = B
            S = ex.fits(D[:, i + 1] - ex.dot(np.swapaxes(B, -1, -2), B))
    x = rhs.copy()
    seg = lambda i: x[:, i * n:(i + 1) * n]
    for i in range(T):                                       # R^T y = b
        for j in range(n):
            seg(i)[:, j] = ex.div(seg(i)[:, j], U[:, i, j, j, None])
            seg(i)[:, j + 1:] = ex.fits(seg(i)[:, j + 1:] - U[:, i, j, j + 1:, None] * seg(i)[:, j, None, :])
        if i + 1 < T:
            seg(i + 1)[...] = ex.fits(seg(i + 1) - ex.dot(np.swapaxes(W[:, i], -1, -2), seg(i)))
    y = x.copy()
    for i in range(T - 1, -1, -1):                           # R x = y
        if i + 1 < T:
            seg(i)[...] = ex.fits(seg(i) - ex.dot(W[:, i], seg(i + 1)))
        for j in range(n - 1, -1, -1):                       # pb_backward_step
            seg(i)[:, j] = ex.div(seg(i)[:, j], U[:, i, j, j, None])
            seg(i)[:, :j] = ex.fits(seg(i)[:, :j] - U[:, i, :j, j, None] * seg(i)[:, j, None, :])
    return U, W, y, x


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_every_intermediate_of_an_exact_row_is_an_integer_below_2_to_53(row):
    D, Bc, X, rhs, Uf, W, logdet = BC.exact_chain(row)
    assert (np.abs(D) < LIMIT).all() and (np.abs(rhs) < LIMIT).all() and np.isfinite(logdet).all()
    assert np.array_equal(np.swapaxes(D, -1, -2), D) and (np.diagonal(Uf, axis1=-2, axis2=-1) > 0).all()
    U2, W2, Y2, X2 = replay(Exact(False), D, Bc, rhs)
    assert np.array_equal(U2, Uf) and np.array_equal(W2, W) and np.array_equal(X2, X)
    assert np.array_equal(Y2, BC.dense_factor(Uf, W) @ X)          # the forward half alone: R X
    if row[0] * row[1] <= 320:                                     # the assembled system itself: A = R^T R (the long chain: block by block above)
        R = BC.dense_factor(Uf, W)
        assert np.array_equal(np.swapaxes(R, -1, -2) @ R, BC.dense(D, Bc))


@pytest.mark.parametrize("row", [r for r in ROWS if r[0] <= 9 and r[1] <= 5], ids=lambda r: "n%d-T%d-b%d-k%d-%s" % r)
def test_the_first_chain_in_fractions(row):
    D, Bc, X, rhs, Uf, W, _ = BC.exact_chain(row)
    U2, W2, Y2, X2 = replay(Exact(True), D[:1], Bc[:1], rhs[:1, :, :min(row[3], 3)])
    assert (U2 == Uf[:1]).all() and (W2 == W[:1]).all() and (X2 == X[:1, :, :min(row[3], 3)]).all()
