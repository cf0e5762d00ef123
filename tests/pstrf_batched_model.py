"""Pure-Python restatement of the batched pivoted Cholesky factorization (cap_dpstrf_batched / cap_dpstrf_vbatched,
csrc/pstrf_batched.hip) in the arithmetic the kernel is held to BIT FOR BIT - the stated recurrence of include/capital_amd.h:
    t = A(p, c);  t = fma(-w_i[p], w_i[c], t) for i = 0 .. j - 1 ascending;  r = t / sqrt(d_p);  w_j[c] = r;  d_c = fma(-r, r, d_c)
with the decisions of tests/pstrf_model.py (the larger d wins, ties to the lowest index; NaN -> info 2; !(d_p > tol_used) -> info 0; the
cap -> info 1).  fma(a, b, c) is float(Fraction(a) Fraction(b) + Fraction(c)): float(Fraction) is correctly rounded, and this Python has
no math.fma.  A full-rank n = 64 block takes about half a second, so the uncapped run of a (matrix, tol) is cached with the remaining
diagonal behind every step: a capped run is a prefix of it."""
import functools
import math
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53


def fma(a, b, c):
    if a == 0.0 or b == 0.0 or not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c                     # a zero product is exact; NaN / infinity: no rounding is involved
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@functools.lru_cache(maxsize=None)
def _run(key, n, tol):
    """the run without a cap: (W rows, order, d behind every step [d_0 = diag A, d_1, ...], info at its stop, largest d in front of each step)"""
    A = np.frombuffer(key, dtype=np.float64).reshape(n, n)
    a = lambda p, c: float(A[min(p, c), max(p, c)])          # the upper triangle only
    d = [float(A[c, c]) for c in range(n)]
    sel = [-1] * n
    W, order, hist, best = [], [], [list(d)], []
    tol_used, info, j = 0.0, 0, 0
    while True:
        un = [c for c in range(n) if sel[c] < 0]
        nan = any(d[c] != d[c] for c in un)
        v, p = -math.inf, -1
        for c in un:
            if d[c] == d[c] and (p < 0 or d[c] > v):         # ascending c: a tie keeps the lowest index
                v, p = d[c], c
        if j == 0:
            tol_used = float(n) * EPS * v if tol < 0 else float(tol)
        best.append(v)
        if nan:
            info = 2
            break
        if p < 0 or not (v > tol_used):
            info = 0
            break
        root = math.sqrt(v)                  # correctly rounded
        row = [0.0] * n
        for c in un:
            if c == p:
                continue
            t = a(p, c)
            for i in range(j):
                t = fma(-W[i][p], W[i][c], t)
            r = t / root
            row[c] = r
            d[c] = fma(-r, r, d[c])
        row[p] = root
        W.append(row)
        sel[p] = j
        order.append(p)
        hist.append(list(d))
        j += 1
    return W, order, hist, info, best, tol_used


def pstrf(A, max_rank=None, tol=-1.0):
    """(R, piv, rank, resid, info): R = W[:, piv] (max_rank x n, rows >= rank +0.0), piv the chosen pivots in order then the unselected
    indices ascending, resid the sum of the unselected remaining diagonal in index order"""
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    max_rank = n if max_rank is None else int(max_rank)
    assert A.shape == (n, n) and 0 <= max_rank <= n and not math.isnan(tol)
    W, order, hist, info, best, tol_used = _run(A.tobytes(), n, float(tol))
    rank = len(order)
    if max_rank < rank:                      # the decision in front of step max_rank found a pivot above the tolerance: the cap
        rank, info = max_rank, 1
    order, d = order[:rank], hist[rank]
    rest = [c for c in range(n) if c not in set(order)]
    piv = np.array(order + rest, dtype=np.int64)
    resid = 0.0
    for c in rest:
        resid += d[c]
    R = np.zeros((max_rank, n))
    if rank:
        R[:rank] = np.array(W[:rank])[:, piv]
    return R, piv, rank, resid, info


def picks(A, tol=-1.0):
    """the largest remaining diagonal in front of every step of the uncapped run (the last one is that of the stopping decision)"""
    A = np.ascontiguousarray(A, dtype=np.float64)
    return list(_run(A.tobytes(), A.shape[0], float(tol))[4])


def tol_used(A, tol=-1.0):
    A = np.ascontiguousarray(A, dtype=np.float64)
    return _run(A.tobytes(), A.shape[0], float(tol))[5]


def logdet(R, rank, info):
    """2 sum_{j < rank} log r_jj in ascending j (libm's log: the kernel's may differ in the last bits - the tests allow 4 spacings)"""
    if info == 2:
        return math.nan
    t = 0.0
    for j in range(rank):
        t += math.log(float(R[j, j]))
    return 2.0 * t
