"""TEST INFRASTRUCTURE: the table of the batched block-tridiagonal Cholesky tests (cap_dpotrf_blocktri_batched, cap_dpotrs_blocktri_batched,
csrc/blocktri_batched.hip) and the two families of chains they run on.  No GPU, no torch: NumPy only.

A ROW is (n, T, batch, nrhs, layout).  n takes every padded class NP = 8 / 16 / 32 / 64 at its upper edge and one above the class below,
T = 1 (no coupling block at all), 2, 3, 5 and one long chain, batch = 1, G = 64 / NP (a full wavefront) and 2 G + 1 (a ragged last
one), nrhs = 1, 3, 16, 17 and one row above 64 (a second pass at every NP), the layouts packed / a leading dimension above n / gaps
between blocks and chains / a right-hand side with ldb > T n.

Everything here is in the C ABI's COLUMN-major reading: a chain is A = R^T R with R block upper bidiagonal, U_i = R[i, i] upper
triangular, W_i = R[i, i + 1]; the diagonal blocks are D_i = U_i^T U_i + W_(i-1)^T W_(i-1), the coupling blocks B_i = A[i, i + 1] =
U_i^T W_i.  Arrays are indexed [chain, position, row, col] mathematically; the runner puts them into memory.

THE EXACT FAMILY (that of tests/test_gpu_chol_exact.py, block by block): U_i = diag(2^k)(I + N) with N strictly upper triangular, entries
-1 / 0 / 1, and W_i = diag(2^k) M with entries -2 .. 2, k = 0 .. 2.  Every number of the recurrence is then a small integer: the factor of
A = R^T R is R itself and the solution of A x = A X is X with no rounding anywhere, whatever the order of a sum.  tests/test_blocktri_cases.py
proves that premise row by row.
THE RANDOM FAMILY: diagonally dominant chains with non-integer entries, for the composition, independence and error-bound tests."""
import numpy as np

NS = (1, 3, 8, 9, 16, 17, 32, 33, 63, 64)
TS = (1, 2, 3, 5)
NRHS = (1, 3, 16, 17)
LAYOUTS = ("packed", "ld", "gaps", "ldb")
LONG = (8, 257, 9, 3, "gaps")            # one long chain row: 257 positions, a ragged second wavefront
WIDE = (9, 3, 5, 70, "ld")               # more than 64 right-hand sides: further passes inside the launch at NP = 16
SEVENTEEN = ((8, 2, 8, 17, "ld"), (17, 3, 5, 17, "packed"), (9, 2, 4, 17, "ldb"), (64, 2, 1, 17, "gaps"))   # one column above 16, at every NP


def padded(n):
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


def rows():
    out, k = [], 0
    for n in NS:
        G = 64 // padded(n)
        for T in TS:
            batch = (1, G, 2 * G + 1)[(k + k // 4) % 3]
            out.append((n, T, batch, NRHS[(k + k // 3) % 4], LAYOUTS[(k + k // 5) % 4]))
            k += 1
    return out + [LONG, WIDE] + list(SEVENTEEN)


def exact_rows():
    return rows()


def random_rows():
    return rows()


def layout(row):
    """(ldd, step_d, stride_d, lde, step_e, stride_e, ldb, stride_b) of a row, in elements"""
    n, T, batch, nrhs, lay = row
    ld = n + 3 if lay == "ld" else n + 1 if lay == "ldb" else n
    step = ld * n + (5 if lay == "gaps" else 0)
    stride_d = step * T + (7 if lay == "gaps" else 0)
    stride_e = step * max(T - 1, 1) + (11 if lay == "gaps" else 0)
    ldb = T * n + (4 if lay == "ldb" else 0)
    stride_b = ldb * nrhs + (3 if lay in ("ldb", "gaps") else 0)
    return ld, step, stride_d, ld, step, stride_e, ldb, stride_b


def exact_factor(row, seed=0):
    """U (batch, T, n, n) upper, W (batch, T - 1, n, n), X (batch, T n, nrhs): int64"""
    n, T, batch, nrhs, _ = row
    rng = np.random.default_rng(1000 * n + 10 * T + batch + seed)
    s = 2 ** rng.integers(0, 3, size=(batch, T, n, 1))
    N = np.triu(rng.integers(-1, 2, size=(batch, T, n, n)), 1)
    U = s * (np.eye(n, dtype=np.int64) + N)
    W = s[:, :max(T - 1, 0)] * rng.integers(-2, 3, size=(batch, max(T - 1, 0), n, n))
    X = rng.integers(-3, 4, size=(batch, T * n, nrhs))
    return U.astype(np.int64), W.astype(np.int64), X.astype(np.int64)


def assemble(U, W):
    """D (batch, T, n, n) full symmetric, Bc (batch, T - 1, n, n) = A[i, i + 1] from the factor R (exact for integer input)"""
    Ut = np.swapaxes(U, -1, -2)
    D = Ut @ U
    if W.shape[1]:
        D[:, 1:] += np.swapaxes(W, -1, -2) @ W
    Bc = Ut[:, :W.shape[1]] @ W
    return D, Bc


def dense(D, Bc):
    """the (batch, T n, T n) matrices of the chains"""
    batch, T, n, _ = D.shape
    A = np.zeros((batch, T * n, T * n), dtype=D.dtype)
    for i in range(T):
        A[:, i * n:(i + 1) * n, i * n:(i + 1) * n] = D[:, i]
        if i + 1 < T:
            A[:, i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = Bc[:, i]
            A[:, (i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] = np.swapaxes(Bc[:, i], -1, -2)
    return A


def dense_factor(U, W):
    """R (batch, T n, T n), block upper bidiagonal"""
    batch, T, n, _ = U.shape
    R = np.zeros((batch, T * n, T * n), dtype=U.dtype)
    for i in range(T):
        R[:, i * n:(i + 1) * n, i * n:(i + 1) * n] = U[:, i]
        if i + 1 < T:
            R[:, i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = W[:, i]
    return R


def exact_chain(row, seed=0):
    """D, Bc, X, RHS = A X, and the expected factor U, W, logdet - all exactly representable"""
    U, W, X = exact_factor(row, seed)
    D, Bc = assemble(U, W)
    rhs = dense(D, Bc) @ X
    logdet = 2.0 * np.log2(np.diagonal(U, axis1=-2, axis2=-1).astype(np.float64)).sum(axis=(1, 2)) * np.log(2.0)
    return D, Bc, X, rhs, U, W, logdet


def random_chain(row, seed=0):
    """diagonally dominant SPD chains with non-integer entries: D (full symmetric), Bc, RHS - float64"""
    n, T, batch, nrhs, _ = row
    rng = np.random.default_rng(77 + 1000 * n + 10 * T + batch + seed)
    Bc = rng.uniform(-1.0, 1.0, size=(batch, max(T - 1, 0), n, n))
    S = rng.uniform(-1.0, 1.0, size=(batch, T, n, n))
    D = 0.5 * (S + np.swapaxes(S, -1, -2)) + (3.0 * n + 1.5) * np.eye(n)     # row sums of |off-diagonal| stay below 3 n
    rhs = rng.uniform(-1.0, 1.0, size=(batch, T * n, nrhs))
    return D, Bc, rhs
