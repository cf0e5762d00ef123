"""Fixtures of the batched pivoted Cholesky tests (cap_dpstrf_batched / cap_dpstrf_vbatched), shared by tests/test_pstrf_batched_model.py
(no GPU: the premises) and tests/test_gpu_pstrf_*batched*.py.  NumPy only.

FIXTURES: the matrices of tests/pstrf_model.py at which the Fraction model (tests/pstrf_batched_model.py), the NumPy model and SciPy's
dpstrf choose the same pivots, rank and info, with a smallest relative pivot gap >= 5e-4 - except rbf(64, 5), which has exact ties and is
kept for that reason: it is the tie-break test.  graded(...) falls by a few hundred per step down into the rounding noise of its largest
entry, so pstrf_model.check_properties is asked of it at an absolute tolerance between two pivots (tol_between), as the single-matrix
tests do, and of every other fixture at the default tolerance.

EXACT FAMILIES: squares(n) and exact_integer(n, flip).  Every operation of exact_integer is exact while 2^(2n) + n fits into 53 bits;
known_answer() therefore covers n <= EXACT_KNOWN_MAX, above that the blocks are ordinary matrices that are held to the model alone."""
import numpy as np

from tests import pstrf_model as pm

FIXTURES = (("dominant", (33, 1)), ("dominant", (64, 2)), ("gram", (64, 20, 3)), ("gram", (17, 5, 4)), ("gram", (9, 9, 8)),
            ("graded", (32, 8, 6)), ("rbf", (64, 5)))
MORE = (("dominant", (9, 11)), ("gram", (33, 12, 12)), ("graded", (17, 6, 13)))
MIN_GAP = 5e-4
SIZES = (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64)
EXACT_KNOWN_MAX = 17
FAMILY = ("squares", "flip0", "flip1", "flip2")


def matrix(kind, args):
    return getattr(pm, kind)(*args)


def padded(n):
    return next(p for p in (8, 16, 32, 64) if p >= n)


def batches(n):
    g = 64 // padded(n)
    return sorted({b for b in (1, g - 1, g, g + 1, 2 * g + 1) if b >= 1})


def caps(n):
    return sorted({0, 1, n // 2, n})


def exact_matrix(n, which):
    return pm.squares(n) if which == "squares" else pm.exact_integer(n, int(which[-1]))[0]


def known_answer(n, which, mr):
    """(R, piv, rank, resid, info) of an exact block at the default tolerance, from its construction (n <= EXACT_KNOWN_MAX for flip*)"""
    if which == "squares":
        dg = np.diag(pm.squares(n))
        order = np.argsort(-dg, kind="stable")
        R = np.zeros((mr, n))
        R[np.arange(mr), np.arange(mr)] = np.sqrt(dg[order[:mr]])
        rest = np.sort(order[mr:])
        return R, np.concatenate([order[:mr], rest]).astype(np.int64), mr, float(dg[rest].sum()), 0 if mr == n else 1
    assert n <= EXACT_KNOWN_MAX
    _, T, perm = pm.exact_integer(n, int(which[-1]))
    pos = np.argsort(perm)                       # column c of A is column pos[c] of T
    rest = np.sort(perm[mr:])
    piv = np.concatenate([perm[:mr], rest]).astype(np.int64)
    R = T[:mr][:, pos[piv]]
    resid = 0.0
    for c in rest:
        resid += float((T[mr:, pos[c]] ** 2).sum())
    return R, piv, mr, resid, 0 if mr == n else 1


def semidefinite_integer(n, k, flip):
    """(A, T_k, perm): A = P^T (T_k^T T_k) P with T_k the first k rows of exact_integer's T - rank k, every operation exact, the remaining
    diagonal exactly zero behind step k"""
    _, T, perm = pm.exact_integer(n, flip)
    Tk = T[:k]
    inv = np.argsort(perm)
    A = (Tk.T @ Tk)[np.ix_(inv, inv)]
    return A, Tk, perm


def same(got, want):
    """bit for bit through positive_zero, NaNs at the same places (their payloads are not compared)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    g, w = np.where(np.isnan(got), 0.0, got) + 0.0, np.where(np.isnan(want), 0.0, want) + 0.0      # (-0.0 + 0.0 is +0.0)
    return bool(np.array_equal(np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64)))


def plan_matrix(n, i):
    """the block of n rows at position i of a size list: full rank, rank n // 3 + 1 and numerically low rank in turn"""
    if n == 0:
        return None
    kind = i % 3
    return pm.dominant(n, 40 + i) if kind == 0 else pm.gram(n, n // 3 + 1, 40 + i) if kind == 1 else pm.rbf(n, 40 + i)
