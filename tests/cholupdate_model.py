"""NumPy restatement of the rank-k update / downdate of the Cholesky factor (csrc/cholupdate.hip): the row sweep that turns the upper
factor R of A into that of A + sigma V V^T, k columns of V in passes of at most 16.  The GPU tests compare the kernels with it; it is
checked on its own, against np.linalg.cholesky, in tests/test_cholupdate_model.py."""
import numpy as np

PASS = 16       # columns of V per pass
BACKWARD_GATE = 1e-14       # |R'^T R' - A'|_F / |A'|_F
ELEMENT_GATE = 1e-13        # max |R' - chol(A')| / max |chol(A')|


def spd(n, seed):
    """A = G G^T / n + I with G uniform in [-1, 1): cond(A) < 10"""
    g = np.random.default_rng(seed)
    G = g.random((n, n)) * 2 - 1
    return G @ G.T / n + np.eye(n)


def thin(n, k, seed):
    """V (n x k) uniform in [-1, 1) * 0.1"""
    return (np.random.default_rng(seed).random((n, k)) * 2 - 1) * 0.1


def sweep(R, V, sigma):
    """(R', info): the upper factor of R^T R + sigma V V^T and 0, or the 1-based first row at which that matrix was found not positive
    definite (the sweep carries on with NaN).  R: n x n upper triangular (the strictly lower part is ignored and returned as it came),
    V: n x k, sigma: +1.0 / -1.0."""
    R = R.copy()
    n = R.shape[0]
    info = 0
    for k0 in range(0, V.shape[1], PASS):
        W = V[:, k0:k0 + PASS].T.copy()
        for r in range(n):
            w = W[:, r].copy()
            rr = R[r, r]
            rho2 = rr * rr + sigma * (w @ w)
            if not (rho2 > 0) or not np.isfinite(rho2):
                if info == 0:
                    info = r + 1
                rho2 = np.nan
            rho = np.sqrt(rho2)
            a, b, g = rr / rho, sigma / rho, 1.0 / (rr + rho)
            old = R[r, r + 1:].copy()
            new = a * old + b * (w @ W[:, r + 1:])
            W[:, r + 1:] -= np.outer(w, (old + new) * g)       # the mixed form: the NEW row updates w_c
            R[r, r + 1:] = new
            R[r, r] = rho
    return R, info


def backward_error(R, A):
    Ru = np.triu(R)
    return np.linalg.norm(Ru.T @ Ru - A) / np.linalg.norm(A)


def element_error(R, Rref):
    return np.abs(np.triu(R) - np.triu(Rref)).max() / np.abs(np.triu(Rref)).max()
