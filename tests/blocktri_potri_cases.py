"""TEST INFRASTRUCTURE: the table of the batched block-tridiagonal selected inverse tests (cap_dpotri_blocktri_batched,
csrc/blocktri_potri_batched.hip) and the exact family of factors they run on.  No GPU, no torch: NumPy only.

A ROW is (n, T, batch, fill, layout): the axes of tests/blocktri_cases.py's rows() - n at and just above every padded class NP, T = 1 (no
E, no recurrence), 2 (one step), 3 (the carried mirror is reused), 5, batch = 1 / G / 2 G + 1 (a ragged last wavefront), the four
layouts, the 257-position chain - with fill = 0 / 1 dealt round so that every n and every T meets both.

Everything here is in the C ABI's COLUMN-major reading: A = R^T R, R block upper bidiagonal, U_i = R[i, i] upper triangular, W_i =
R[i, i + 1]; Sigma = A^-1; with G_i = U_i^-1 W_i, positions descending,
    P_i = U_i^-1 U_i^-T;  Sigma_(T-1,T-1) = P_(T-1);  C_i = Sigma_(i,i+1) = -G_i Sigma_(i+1,i+1);  Sigma_(i,i) = P_i - C_i G_i^T.
Arrays are indexed [chain, position, row, col] mathematically; the runner puts them into memory.

THE EXACT FAMILY.  U_i = potri_batched_cases.block(fam, n, False, idx)[0] (power-of-two diagonals, every value of its inverse route a dyadic
rational, premise asserted there) and W_i a SIGNED PERMUTATION scaled by powers of two: one entry of +-{1/2, 1, 2} per row and column (a
dense W_i overflows 2^53 at T = 5).  exact_chain() evaluates the recurrence in exact integer arithmetic (Python integers at a power-of-two
scale) and PROVES, element by element, that no rounding can occur on any route and in any order of summation: for every sum of products
the kernel or the host-driven composition forms - the substitution U G = W, G Sigma, C G^T, P - (C G^T) - the sum of the ABSOLUTE values of
its terms, at the scale 2^-f of which every term is a multiple, is below 2^53; every partial sum is then an integer of fewer than 53 bits
at that scale.  A chain that fails raises: it is replaced (another block index), never loosened.
THE RANDOM FAMILY is blocktri_cases.random_chain factored by blocktri_potrf on the device; reference() evaluates the same recurrence from
that factor in np.longdouble and in NumPy fp64."""
import functools

import numpy as np

from tests import blocktri_cases as BC
from tests import potri_batched_cases as PC

LIMIT = 1 << 53
FAMILIES = ("F2", "F1", "F2i")


def rows():
    out = []
    for k, (n, T, batch, _, lay) in enumerate(BC.rows()[:len(BC.NS) * len(BC.TS)]):
        out.append((n, T, batch, (k % 4 + k // 4) % 2, lay))
    n, T, batch, _, lay = BC.LONG
    return out + [(n, T, batch, 1, lay)]


def random_rows():
    return rows()


def exact_rows():
    """(row, family): F2 on every (n, T) of the table, F1 and F2i on every n at T = 2 and 3 (and F1 at T = 1); the long chain is random only"""
    out = [(r, "F2") for r in rows() if r[1] <= 5]
    for r in rows():
        if r[1] in (2, 3):
            out += [(r, "F1"), (r, "F2i")]
        elif r[1] == 1:
            out.append((r, "F1" if r[0] % 2 else "F2i"))
    return out


def row_id(r):
    return "n%d-T%d-b%d-fill%d-%s" % r


def layout(row):
    """(ldd, step_d, stride_d, lde, step_e, stride_e) of a row, in elements: blocktri_cases.layout's"""
    n, T, batch, _, lay = row
    return BC.layout((n, T, batch, 1, lay))[:6]


# ------------------------------------------------------------------------------------------------------------ exact integer arithmetic
def _ints(X):
    """a float64 array of dyadic rationals -> (object array of Python integers M, f) with X = M / 2^f exactly, f minimal"""
    X = np.asarray(X, dtype=np.float64)
    f = 0
    while not np.array_equal(np.ldexp(X, f), np.floor(np.ldexp(X, f))):
        f += 1
        assert f < 200
    S = np.ldexp(X, f)
    assert np.all(np.abs(S) < 2.0 ** 62)
    return np.vectorize(int, otypes=[object])(S) if X.size else S.astype(object), f


def _norm(M, f):
    """strip the factors of two every entry shares: the smallest scale of which every entry is a multiple"""
    while f > 0 and all(int(v) % 2 == 0 for v in M.flat):
        M = M // 2
        f -= 1
    return M, f


def _mag(M):
    return np.vectorize(abs, otypes=[object])(M) if M.size else M


def _below(bound, what, worst):
    """every entry of an integer bound below 2^53; records the largest"""
    m = max((int(v) for v in bound.flat), default=0)
    assert m < LIMIT, "%s: a sum of absolute terms reaches 2^%.1f at its scale" % (what, np.log2(float(m)))
    worst[0] = max(worst[0], m)


def _floats(M, f):
    assert all(abs(int(v)) < LIMIT for v in M.flat)
    return np.ldexp(M.astype(np.float64), -f)


def _perm(n, rng):
    W = np.zeros((n, n))
    W[rng.permutation(n), np.arange(n)] = rng.choice([-1.0, 1.0], size=n) * rng.choice([0.5, 1.0, 2.0], size=n)
    return W


@functools.lru_cache(maxsize=None)
def exact_chain(row, fam):
    """U (batch, T, n, n) upper, W (batch, T - 1, n, n), Sd (batch, T, n, n) = Sigma_(i,i) full symmetric, Sc (batch, T - 1, n, n) = C_i:
    float64, every number exactly representable; and log2 of the largest bound met - the premise is proved on the way (see the head)"""
    n, T, batch, _, _ = row
    U = np.zeros((batch, T, n, n))
    W = np.zeros((batch, max(T - 1, 0), n, n))
    Sd = np.zeros((batch, T, n, n))
    Sc = np.zeros((batch, max(T - 1, 0), n, n))
    worst = [1]
    for c in range(batch):
        sig = None
        for i in range(T - 1, -1, -1):
            M, Mi, Cu = PC.block(fam, n, False, c * T + i)
            U[c, i] = M
            P = _ints(Cu + np.triu(Cu, 1).T)
            if i == T - 1:
                sig = P
            else:
                W[c, i] = _perm(n, np.random.default_rng([31, n, T, c, i]))
                (Ui, fu), (Vi, fv), (Wi, fw) = _ints(M), _ints(Mi), _ints(W[c, i])
                G, fg = _norm(Vi.dot(Wi), fv + fw)                                 # exact: a permutation picks one term per sum
                # the substitution U G = W: every intermediate is w - (a partial sum of u g), bounded by |W| + |U||G| at the scale of u g
                f = max(fw, fu + fg)
                _below(_mag(Wi) * (1 << (f - fw)) + _mag(Ui).dot(_mag(G)) * (1 << (f - fu - fg)), "%s n=%d T=%d chain %d position %d: U G = W" % (fam, n, T, c, i), worst)
                S, fs = sig
                _below(_mag(G).dot(_mag(S)), "%s n=%d T=%d chain %d position %d: G Sigma" % (fam, n, T, c, i), worst)
                C, fc = _norm(-G.dot(S), fg + fs)
                _below(_mag(C).dot(_mag(G).T), "%s n=%d T=%d chain %d position %d: C G^T" % (fam, n, T, c, i), worst)
                Q, fq = C.dot(G.T), fc + fg
                Pm, fp = P
                f = max(fp, fq)                                                    # P - Q: both at the finer scale
                Pa, Qa = Pm * (1 << (f - fp)), Q * (1 << (f - fq))
                _below(_mag(Pa) + _mag(Qa), "%s n=%d T=%d chain %d position %d: P - C G^T" % (fam, n, T, c, i), worst)
                sig = _norm(Pa - Qa, f)
                assert all(sig[0][a, b] == sig[0][b, a] for a in range(n) for b in range(a))
                Sc[c, i] = _floats(C, fc)
            Sd[c, i] = _floats(*sig)
    for a in (U, W, Sd, Sc):
        a.setflags(write=False)
    return U, W, Sd, Sc, float(np.log2(float(worst[0])))


# ------------------------------------------------------------------------------------------------------------ the recurrence, two precisions
def reference(U, W, dtype):
    """(Sd, Sc) of ONE chain from its factor U (T, n, n) upper, W (T - 1, n, n) by the recurrence of the head, evaluated in `dtype`
    (np.longdouble: the reference; np.float64: the yardstick of the accuracy test, which differs from the kernel in summation order only)"""
    T, n, _ = U.shape
    U, W = np.triu(U).astype(dtype), W.astype(dtype)
    Sd, Sc = np.zeros((T, n, n), dtype=dtype), np.zeros((max(T - 1, 0), n, n), dtype=dtype)

    def solve_upper(R, B):                           # R X = B by substitution, all columns at once
        X = np.array(B, dtype=dtype, copy=True)
        for j in range(n - 1, -1, -1):
            X[j] = (X[j] - R[j, j + 1:] @ X[j + 1:]) / R[j, j]
        return X
    for i in range(T - 1, -1, -1):
        Vi = solve_upper(U[i], np.eye(n, dtype=dtype))
        P = Vi @ Vi.T
        if i == T - 1:
            Sd[i] = P
        else:
            G = solve_upper(U[i], W[i])
            Sc[i] = -(G @ Sd[i + 1])
            S = P - Sc[i] @ G.T
            Sd[i] = np.triu(S) + np.triu(S, 1).T     # the upper triangle counts, as in the kernel
    return Sd, Sc
