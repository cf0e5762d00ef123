"""Exact operands for the batched triangular solves and products (cap_dtrsm_batched, cap_dtrmm_batched and their plan forms), shared by
tests/test_trsm_batched_cases.py (no GPU) and tests/test_gpu_trsm_batched.py / test_gpu_trsm_vbatched.py (-m gpu).  NumPy only, nothing of
torch or the GPU is imported here.

T and T^-1 are potri_batched_cases.block (closed forms, power-of-two diagonals, positive diagonal), X has entries in {-2, -1, 0, 1, 2}:
  trsm: the right-hand side is B = T^T X (trans) or T X, formed exactly; the expected result is X, and sumsq the integer column sums of X^2;
  trmm: the input is X; the expected result is T^T X or T X.
THE EXACTNESS PREMISE (premise(), asserted per row by tests/test_trsm_batched_cases.py): with f the fraction bits of T,
(|T|^T |X|).max(), (|T| |X|).max() and (|T^-1| |T| |X|).max(), each times 2^f, stay below 2^53.  Every value either operation forms is a
partial sum, in some order, of terms t_ij x_j (the products) or of b_i - sum t_ij x_j over a subset of j with B itself such a sum (the
substitutions; the quotients are the integers x_j): a multiple of 2^-f bounded by the first two figures, hence a float64.  The third covers
a route that passes through T^-1.  A row that fails the premise is a bad row and gets replaced; the premise is not loosened."""
import functools

import numpy as np

from tests import potri_batched_cases as P

WAVE_N = (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64)
GROUP_N = (65, 80, 127, 128, 129, 191, 192, 193, 255, 256)
NRHS = (1, 3, 16, 17, 40)
BATCHES = (1, 3, 65, 257)
LAYOUTS = P.LAYOUTS                     # (ld - n, stride - ld n); the same pair pads B: (ldb - n, stride_b - ldb nrhs)
LIMIT = 2.0 ** 53
DISTINCT = 5                            # different blocks per (family, n); a batch repeats them round


def fraction_bits(M):
    """the least f with M 2^f integer"""
    for f in range(0, 60):
        if np.array_equal(np.round(M * 2.0 ** f), M * 2.0 ** f):
            return f
    raise AssertionError("not a dyadic matrix")


def premise(T, Ti, X):
    f = 2.0 ** fraction_bits(T)
    aT, aX = np.abs(T), np.abs(X)
    return {"|T|^T|X| x 2^f": (aT.T @ aX).max() * f, "|T||X| x 2^f": (aT @ aX).max() * f, "|Tinv||T||X| x 2^f": (np.abs(Ti) @ (aT @ aX)).max() * f}


def exact_rows():
    """(n, fam, batch, nrhs, (dl, ds)): every n with every family; batch, nrhs and layout dealt round as potri_batched_cases.exact_rows does
    (the large batches go to the wave path and to a few small workgroup blocks only: a test stays within seconds)"""
    rows = []
    for sizes in (WAVE_N, GROUP_N):
        for k, n in enumerate(sizes):
            for f, fam in enumerate(P.FAMILIES):
                b = BATCHES[(k + 3 * f) % len(BATCHES)]
                if n > 80 and b > 3:
                    b = 3 if b == 65 else 1
                rows.append((n, fam, b, NRHS[(k + 2 * f) % len(NRHS)], LAYOUTS[(k + f) % 4]))
    return rows


def row_id(r):
    return "n%d-%s-b%d-k%d-ld+%d-st+%d" % (r[0], r[1], r[2], r[3], r[4][0], r[4][1])


@functools.lru_cache(maxsize=None)
def operands(fam, n, nrhs, idx):
    """(T, Tinv, X, T^T X, T X) of block idx, read-only; the products are exact under the premise"""
    T, Ti, _ = P.block(fam, n, False, idx % DISTINCT)
    X = np.random.default_rng([41, n, nrhs, idx]).integers(-2, 3, size=(n, nrhs)).astype(np.float64)
    out = (T, Ti, X, T.T @ X, T @ X)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def sumsq_model(col):
    """q = 0; for r: q = fma(x_r, x_r, q) with one correctly rounded conversion per step (fractions: exact, then float())"""
    from fractions import Fraction
    q = 0.0
    for v in col:
        v = float(v)
        if not np.isfinite(v) or not np.isfinite(q):
            return float("nan") if np.isnan(v) or np.isnan(q) else float("inf")
        q = float(Fraction(v) * Fraction(v) + Fraction(q))
    return q
