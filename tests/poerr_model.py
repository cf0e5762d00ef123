"""NumPy restatement of what cap_dpocon / cap_dpoerr compute (LAPACK's dpocon and the bounds of dporfs), and the test matrices.

`lacn2(apply, apply_t, n)` is LAPACK's dlacn2 with its reverse communication turned into two callbacks: the start vector 1 / n, the sign
vector (x > 0 -> 1, else -1), the stop at a repeated sign vector or an estimate that did not grow, idamax with the lowest index winning
ties, ITMAX = 5, the final alternating-sign vector with its 2 |x|_1 / (3 n) floor.  It returns (est, number of operator applications).
With a list as `trace` it also appends, per operator application and in order, (stage, j, est): the stage in which the result of that
application is judged (1 the start vector, 2 / 4 a sign vector, 3 a unit vector, 5 the alternating-sign vector: the stage numbers of
csrc/pocon.hip) and the index and the estimate as they stand after that judgement.  The results do not depend on `trace`."""
import numpy as np

EPS = 2.0 ** -53                       # dlamch('Epsilon')
SAFMIN = 2.2250738585072014e-308       # dlamch('Safe minimum')
ITMAX = 5


def _sign(x):
    return np.where(x > 0.0, 1.0, -1.0)


def _idamax(x):
    return int(np.argmax(np.abs(x)))    # the first of equals, as idamax


def lacn2(apply, apply_t, n, trace=None):
    note = (lambda *a: None) if trace is None else (lambda stage, j, est: trace.append((stage, int(j), float(est))))
    solves = 1
    x = apply(np.full(n, 1.0 / n))
    if n == 1:
        note(1, 0, abs(x[0]))
        return abs(x[0]), solves
    est = np.abs(x).sum()
    note(1, 0, est)
    isgn = _sign(x)
    x = apply_t(isgn.copy()); solves += 1
    j = _idamax(x)
    note(2, j, est)
    it = 2
    while True:
        e = np.zeros(n); e[j] = 1.0
        x = apply(e); solves += 1
        estold, est = est, np.abs(x).sum()
        note(3, j, est)
        if np.array_equal(_sign(x), isgn) or est <= estold:
            break
        isgn = _sign(x)
        x = apply_t(isgn.copy()); solves += 1
        jlast, j = j, _idamax(x)
        note(4, j, est)
        if x[jlast] != abs(x[j]) and it < ITMAX:
            it += 1
            continue
        break
    i = np.arange(n, dtype=np.float64)
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + i / (n - 1))
    x = apply(alt); solves += 1
    temp = 2.0 * (np.abs(x).sum() / (3 * n))
    if temp > est:
        est = temp
    note(5, j, est)
    return est, solves


def _solver(R):
    import scipy.linalg as sl
    return lambda v: sl.solve_triangular(R, sl.solve_triangular(R, v, trans='T', lower=False), lower=False)


def inv_norm_est(R):
    """(est ||A^-1||_1, solves) for A = R^T R, R upper triangular"""
    s = _solver(R)
    return lacn2(s, s, R.shape[0])


def rcond(R, anorm):
    n = R.shape[0]
    if n == 0:
        return 1.0
    if anorm != anorm:
        return anorm
    if anorm == 0.0:
        return 0.0
    est, _ = inv_norm_est(R)
    return 0.0 if est == 0.0 else (1.0 / est) / anorm


def safe(n):
    safe1 = (n + 1) * SAFMIN
    return safe1, safe1 / EPS


def berr(A, B, X, dtype=np.float64):
    """componentwise backward error per column, LAPACK's guarded quotient, formed in `dtype`"""
    A, B, X = (np.asarray(m, dtype=dtype) for m in (A, B, X))
    n = A.shape[0]
    safe1, safe2 = safe(n)
    r = np.abs(B - A @ X)
    d = np.abs(A) @ np.abs(X) + np.abs(B)
    q = np.where(d > safe2, r / np.where(d > safe2, d, 1), (r + safe1) / (d + safe1))
    return q.max(axis=0)


def ferr_weights(A, B, X):
    """w = |r| + (n + 1) eps (|A||x| + |b|) (+ safe1 under the guard), n x nrhs"""
    n = A.shape[0]
    safe1, safe2 = safe(n)
    r = np.abs(B - A @ X)
    d = np.abs(A) @ np.abs(X) + np.abs(B)
    return r + (n + 1) * EPS * d + np.where(d > safe2, 0.0, safe1)


def ferr(A, R, B, X):
    """the forward error bound per column: lacn2 on diag(w) A^-1 / A^-1 diag(w), over max |x| (left alone when x = 0)"""
    s = _solver(R)
    W = ferr_weights(A, B, X)
    out = np.zeros(X.shape[1])
    for j in range(X.shape[1]):
        w = W[:, j]
        est, _ = lacn2(lambda v: w * s(v), lambda v: s(w * v), A.shape[0])
        xm = np.abs(X[:, j]).max()
        out[j] = est / xm if xm != 0.0 else est
    return out


def rand_spd(n, kappa, seed=0):
    """Q diag(logspace(0, -log10 kappa, n)) Q^T, symmetrised, Q from a seeded QR of a Gaussian matrix"""
    rng = np.random.default_rng(1000 * seed + n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0.0, -np.log10(kappa), n)) @ Q.T
    return (A + A.T) / 2


def lap(n):
    """the tridiagonal 2, -1 matrix"""
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


NS = (1, 2, 3, 127, 128, 129, 257, 300, 1000)
