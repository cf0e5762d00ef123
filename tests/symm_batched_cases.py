"""Operands and NumPy references for the batched symmetric products and the diagnostics built on them (cap_dsymm_batched,
cap_dlansy_batched, cap_dpocon_batched, cap_dpoerr_batched and their _vbatched forms), shared by tests/test_symm_batched_cases.py (no GPU)
and tests/test_gpu_symm_*.py (-m gpu).  NumPy only, nothing of torch or the GPU is imported here.

EXACT OPERANDS.  A symmetric with integer entries in [-4, 4], X and B integers in [-4, 4], alpha and beta dyadic: every product is an
integer, every partial sum in ANY order is an integer bounded by (|A||X|)_ij, and the result has at most three fraction bits - premise()
returns the bound times 2^3 times the largest |alpha|, |beta|, which must stay below 2^53.  Then every summation order gives the same bits
and NumPy's own product is the reference, bit for bit.

THE BOUNDS.  berr / weights / ferr restate the header's formulas on given r = b - A x and s = |A||x| + |b|, in float64 with the same
guard (safe1 = (n + 1) safmin, safe2 = safe1 / eps, eps = 2^-53, safmin = 2^-1022) and the same roundings (w = |r| + fl(t s))."""
import functools

import numpy as np

from tests import potri_batched_cases as P

EPS = 2.0 ** -53
SAFMIN = 2.0 ** -1022
LIMIT = 2.0 ** 53
WAVE_N = (1, 2, 7, 8, 9, 16, 17, 33, 63, 64)
WAVE_BATCHES = (1, 3, 65, 257)
GROUP_N = (65, 96, 129, 200, 255, 256)
GROUP_BATCHES = (1, 5, 33)
NRHS = (0, 1, 3, 16, 17, 33)
LAYOUTS = P.LAYOUTS
COEFFS = ((1.0, 0.0), (-1.0, 1.0), (2.0, -0.5), (0.25, 0.0), (-0.5, 4.0), (1.0, 1.0))


@functools.lru_cache(maxsize=600)
def operands(n, nrhs, idx):
    """(A symmetric n x n, X, B n x nrhs) of block idx: small integers, read-only"""
    rng = np.random.default_rng([4401, n, nrhs, idx])
    U = np.triu(rng.integers(-4, 5, size=(n, n))).astype(np.float64)
    A = U + np.triu(U, 1).T
    X = rng.integers(-4, 5, size=(n, nrhs)).astype(np.float64)
    B = rng.integers(-4, 5, size=(n, nrhs)).astype(np.float64)
    for a in (A, X, B):
        a.setflags(write=False)
    return A, X, B


def premise(A, X, B, alpha, beta):
    """the bound on every partial sum and result, times 2^3 fraction bits: must be < 2^53"""
    s = np.abs(A) @ np.abs(X)
    top = max(float(s.max()) if s.size else 0.0, float(np.abs(B).max()) if B.size else 0.0, 1.0)
    return top * 8 * max(abs(alpha), abs(beta), 1.0) * 2


def expected(A, X, B, alpha, beta, absolute):
    if absolute:
        A, X, B = np.abs(A), np.abs(X), np.abs(B)
    t = alpha * (A @ X)
    return t if beta == 0.0 else beta * B + t


def exact_rows():
    """(n, nrhs, batch, absolute, (alpha, beta), layout of A, layout of X / B / Y, in place) - every n with three nrhs, the batch sizes,
    coefficients and layouts dealt round; every nrhs occurs on both paths; in place only with beta != 0"""
    rows, q = [], 0
    for sizes, batches in ((WAVE_N, WAVE_BATCHES), (GROUP_N, GROUP_BATCHES)):
        for k, n in enumerate(sizes):
            for j in range(3):
                nrhs = NRHS[(k + 2 * j) % len(NRHS)]
                co = COEFFS[q % len(COEFFS)]
                rows.append((n, nrhs, batches[(k + j) % len(batches)], (q // 2) % 2, co, LAYOUTS[q % 4], LAYOUTS[(q + 1 + j) % 4],
                             bool(co[1] != 0.0 and q % 2 == 1)))
                q += 1
    return rows


def row_id(r):
    return "n%d-nrhs%d-b%d-abs%d-a%g-b%g-A+%d+%d-X+%d+%d%s" % (r[0], r[1], r[2], r[3], r[4][0], r[4][1], r[5][0], r[5][1], r[6][0], r[6][1],
                                                              "-inplace" if r[7] else "")


# --------------------------------------------------------------------------------------------------------------------- the bounds
def safe(n):
    safe1 = (n + 1) * SAFMIN
    return safe1, safe1 / EPS


def berr(r, s, n):
    """max over the rows of the guarded ratio, per column; NaN propagates"""
    safe1, safe2 = safe(n)
    r = np.abs(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(s > safe2, r / np.where(s > safe2, s, 1.0), (r + safe1) / (s + safe1))
    return nanmax(q, 0)


def weights(r, s, n):
    """w = |r| + fl((n + 1) eps * s)"""
    return np.abs(r) + ((n + 1) * EPS) * s


def ferr(y, x):
    """max_i y_ij / max_i |x_ij|, the numerator alone for x_j = 0"""
    top, xm = nanmax(y, 0), nanmax(np.abs(x), 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(xm == 0.0, top, top / np.where(xm == 0.0, 1.0, xm))


def nanmax(a, axis):
    """the maximum that keeps a NaN"""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    m = np.fmax.reduce(a, axis=axis)
    return np.where(np.isnan(a).any(axis=axis), np.nan, m)


def norm1(A):
    return float(nanmax(np.abs(A).sum(axis=0), 0)) if A.shape[0] else 0.0


def sums_exact(a):
    """every column sum of |a| is exact in any order: the entries are multiples of one 2^-f and the largest sum is below 2^53 2^-f"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    for f in range(0, 80):
        q = a * 2.0 ** f
        if np.array_equal(q, np.round(q)):
            return bool(q.sum(axis=0).max() < LIMIT)
    return False


def sym(U):
    """the symmetric matrix whose upper triangle is that of U"""
    U = np.triu(U)
    return U + np.triu(U, 1).T


# --------------------------------------------------------------------------------------------------------------------- integer SPD systems
@functools.lru_cache(maxsize=200)
def spd_system(n, nrhs, idx):
    """(A, xstar, B): A = M M^T + I with a sparse integer M, xstar integer, B = A xstar exact - the first seed for which NumPy's own
    Cholesky solve satisfies |X - xstar|_inf / |X|_inf <= ferr with the reference formulas in every column (so that the inequality the GPU
    test asserts without a tolerance is known to be satisfiable for this block)"""
    for seed in range(50):
        rng = np.random.default_rng([9103, n, nrhs, idx, seed])
        M = rng.integers(-1, 2, size=(n, n)) * (rng.random((n, n)) < min(1.0, 6.0 / n))
        A = (M @ M.T + np.eye(n, dtype=np.int64)).astype(np.float64)
        xs = rng.integers(-8, 9, size=(n, nrhs)).astype(np.float64)
        xs[0, :] += (np.abs(xs).max(axis=0) == 0)               # no zero column here
        B = A @ xs
        assert np.abs(A).sum(axis=1).max() * 16 < LIMIT
        L = np.linalg.cholesky(A)
        X = np.linalg.solve(L.T, np.linalg.solve(L, B))
        r = B - A @ X
        s = np.abs(A) @ np.abs(X) + np.abs(B)
        fe = ferr(np.abs(np.linalg.inv(A)) @ weights(r, s, n), X)
        if np.all(np.abs(X - xs).max(axis=0) / np.abs(X).max(axis=0) <= fe):
            for a in (A, xs, B):
                a.setflags(write=False)
            return A, xs, B
    raise AssertionError("no integer SPD system found for n = %d" % n)
