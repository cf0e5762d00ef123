"""NumPy restatement of the pivoted Cholesky factorization (cap_dpstrf, csrc/pstrf.hip; LAPACK's dpstrf with a rank cap): the semantics
the kernel is held to, the fixture matrices of the tests, and the property checks both the model (tests/test_pstrf_model.py, no GPU) and
the kernel (tests/test_gpu_pstrf.py) have to pass."""
import functools

import numpy as np

EPS = 2.0 ** -53        # LAPACK's dlamch('Epsilon') = the unit roundoff of fp64: the eps of the default tolerance and of gamma_k


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def default_tol(A):
    n = A.shape[0]
    return n * EPS * np.diag(A).max() if n else 0.0


def pstrf(A, max_rank=None, tol=-1.0):
    """(R, piv, rank, resid, info, trace) of the left-looking pivoted Cholesky factorization of the symmetric A (only its upper triangle
    is read).  R: max_rank x n with A[piv][:, piv] ~ R^T R; piv: the chosen pivots in order, then the unselected indices in increasing
    order; resid: the sum of the remaining diagonal in index order; info 0: stopped at a pivot <= tol (or after n steps), 1: max_rank
    steps done with the remainder above tol, 2: a NaN on the remaining diagonal.  tol < 0: n eps max_i a_ii.
    trace: {"picks": per chosen pivot the (best, second-best) remaining diagonal (second = -inf when only one is left), "stop": the
    largest remaining diagonal at the stopping decision (None after n steps or a NaN)}."""
    n = A.shape[0]
    max_rank = n if max_rank is None else int(max_rank)
    assert 0 <= max_rank <= n and not np.isnan(tol)
    d = np.diag(A).astype(np.float64).copy()
    sel = np.zeros(n, dtype=bool)
    W = np.zeros((max_rank, n))
    order, trace = [], {"picks": [], "stop": None}
    tol_used = float(tol) if tol >= 0 else default_tol(A)
    info = 0
    j = 0
    while True:
        un = np.flatnonzero(~sel)
        if np.isnan(d[un]).any():
            info = 2
            break
        if j == n:
            break
        p = un[np.argmax(d[un])]            # argmax returns the first maximum: ties go to the lowest index
        if d[p] <= tol_used or j == max_rank:
            info = 0 if d[p] <= tol_used else 1
            trace["stop"] = d[p]
            break
        rest = d[un[un != p]]
        trace["picks"].append((d[p], rest.max() if rest.size else -np.inf))
        root = np.sqrt(d[p])
        cols = un[un != p]
        a_row = np.where(cols >= p, A[p, cols], A[cols, p])
        r = np.zeros(n)
        r[cols] = (a_row - W[:j, cols].T @ W[:j, p]) / root
        r[p] = root
        W[j] = r
        d[cols] -= r[cols] * r[cols]
        sel[p] = True
        order.append(p)
        j += 1
    rest = np.flatnonzero(~sel)
    piv = np.array(order + list(rest), dtype=np.int64)
    resid = 0.0
    for c in rest:
        resid += d[c]
    R = W[:, piv]
    return R, piv, j, resid, info, trace


# ---- fixtures (computed once, never written) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram(n, k, seed):
    """G G^T with a Gaussian G (n x k): rank k"""
    G = np.random.default_rng(seed).standard_normal((n, k))
    A = G @ G.T
    A = (A + A.T) / 2
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def dominant(n, seed):
    """G G^T / 2n + diag(shuffled linspace(1, 3)): full rank, well separated pivots"""
    g = np.random.default_rng(seed)
    G = g.standard_normal((n, n))
    A = G @ G.T / (2 * n)
    A = (A + A.T) / 2 + np.diag(g.permutation(np.linspace(1.0, 3.0, n)))
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def rbf(n, seed):
    """exp(-(x_i - x_j)^2 / 0.02) on n sorted uniform points: numerically low rank, pivots that tie"""
    x = np.sort(np.random.default_rng(seed).random(n))
    A = np.exp(-(x[:, None] - x[None, :]) ** 2 / 0.02)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def graded(n, k, seed):
    """G D^2 G^T with a Gaussian G (n x k) and D = diag(10^(-1.25 i)): the pivots fall by a few hundred per step (the absolute-tol tests)"""
    G = np.random.default_rng(seed).standard_normal((n, k)) * 10.0 ** (-1.25 * np.arange(k))
    A = G @ G.T
    A = (A + A.T) / 2
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def squares(n, seed=5):
    """the diagonal matrix of the squares of 1 .. n in shuffled order"""
    A = np.diag(np.random.default_rng(seed + n).permutation(np.arange(1.0, n + 1)) ** 2)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def exact_integer(n, flip):
    """A = P^T (T^T T) P with T upper triangular, diagonal 2^(n-j) and entries -1 / 0 / 1 above it: every operation of the factorization is
    exact (integers, divisions by powers of two), the pivots come in the order of T's columns.  flip = 0: P = identity (the largest diagonal
    at index 0, every A(p, c) read as A[p, c]); 1: the reversal (largest at n - 1, every A(p, c) read as A[c, p]); 2: a shuffle (both)."""
    g = np.random.default_rng(7 + n)
    T = np.triu(g.integers(-1, 2, (n, n)).astype(np.float64), 1) + np.diag(2.0 ** np.arange(n, 0, -1))
    perm = [np.arange(n), np.arange(n)[::-1], g.permutation(n)][flip]
    inv = np.argsort(perm)
    A = (T.T @ T)[np.ix_(inv, inv)]          # A[perm][:, perm] = T^T T
    A.setflags(write=False)
    return A, T, perm.astype(np.int64)


# ---- property checks --------------------------------------------------------------------------------------------------------------------------
def check_properties(A, R, piv, rank, info, tol_used, rows=None):
    """Every property the issue asks of a factorization, in exact-enough arithmetic (long double products); returns the largest ratio
    |A - R^T R| / (gamma_{rank+2} |R|^T |R|) over the selected rows.  rows: check the backward error on these pivoted rows only (large n)."""
    n = A.shape[0]
    assert sorted(piv.tolist()) == list(range(n)), "piv is not a permutation"
    assert np.all(np.diff(piv[rank:]) > 0), "the tail of piv is not increasing"
    assert np.all(R[rank:] == 0), "rows >= rank are not zero"
    head = R[:rank, :rank]
    assert np.all(np.tril(head, -1) == 0), "R[:rank, :rank] is not upper triangular"
    dg = np.diag(head)
    assert np.all(dg > 0) and np.all(np.diff(dg) <= 0), "the diagonal is not positive and non-increasing"
    Asym = np.triu(A) + np.triu(A, 1).T                      # only the upper triangle counts
    Ap = Asym[np.ix_(piv, piv)]
    g = gamma(rank + 2)
    sel_rows = np.arange(rank) if rows is None else np.asarray([r for r in rows if r < rank], dtype=np.int64)
    Rl = R[:rank].astype(np.longdouble)
    E = np.abs(Ap[sel_rows].astype(np.longdouble) - Rl[:, sel_rows].T @ Rl)
    B = np.abs(Rl[:, sel_rows]).T @ np.abs(Rl)
    ratio = 0.0
    if sel_rows.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(B > 0, E / (g * B), np.where(E == 0, 0.0, np.inf))
        ratio = float(q.max())
        assert ratio <= 1.0, "backward error %.3g times the bound" % ratio
    if rank < n:
        a = np.diag(Ap)[rank:].astype(np.longdouble)
        rem = a - (Rl[:, rank:] ** 2).sum(axis=0)
        assert np.all(rem >= -2 * g * a), "remaining diagonal below -2 gamma a_cc: %s" % float((rem / a).min())
        if info == 0:
            assert np.all(rem <= tol_used + 2 * g * a), "remaining diagonal above tol: %s" % float((rem - tol_used - 2 * g * a).max())
    return ratio


def remaining_diagonal(A, R, piv, rank):
    """the fp64 remaining diagonal d_c = a_cc - sum_i R[i, c]^2 of the unselected columns, in index (= tail) order"""
    a = np.diag(A)[piv[rank:]]
    return a - (R[:rank, rank:] ** 2).sum(axis=0)


def min_gap(trace):
    """smallest best minus second-best remaining diagonal over the chosen pivots"""
    return min((b - s for b, s in trace["picks"]), default=np.inf)


def sample_rows(rank, count=48, seed=11):
    """pivoted rows on which a large case checks the backward error: the first and last eight and `count` random ones"""
    g = np.random.default_rng(seed)
    rows = set(range(min(8, rank))) | set(range(max(rank - 8, 0), rank)) | set(g.integers(0, max(rank, 1), count).tolist())
    return sorted(r for r in rows if r < rank)


def tol_between(picks, k):
    """the geometric mean of the model's pivots k - 1 and k: an absolute tolerance a factor of 10 or more from both, at which the
    factorization has to stop after exactly k steps"""
    tol = float(np.sqrt(picks[k - 1] * picks[k]))
    assert picks[k - 1] >= 10 * tol and tol >= 10 * picks[k]
    return tol
