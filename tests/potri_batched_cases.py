"""Exact and random operands for the batched triangular inverse and SPD inverse (cap_dtrtri_batched, cap_dpotri_batched), shared by
tests/test_potri_batched_cases.py (no GPU) and tests/test_gpu_potri_batched.py (-m gpu).  NumPy only, nothing of torch or the GPU is
imported here.

EXACT BLOCKS.  The constructions of tests/tri_cases.py (F1 "three classes", F2 "dense", F2i "bidiagonal": power-of-two diagonals, so
that every value an inverse route forms is a dyadic rational) with a seed that includes the block index: every block of a batch is a
different matrix.  signed = True (TRTRI) gives the diagonal random signs; signed = False (POTRI and the factor-then-invert chain) gives a
POSITIVE diagonal - in F2 / F2i the two sign matrices are then equal, T = D S C S, so that T is the Cholesky factor of T^T T.
block() returns T, T^-1 and triu(T^-1 T^-T) from the closed forms and asserts, per block,
  * T T^-1 = I = T^-1 T elementwise,
  * the exactness premise as tri_cases.bounds does: |T^-1||T||T^-1| 2^5 and |T^-1||T^-1|^T 2^4 below 2^53 (every partial sum of the inverse
    route - T12 T22^-1, T11^-1 (T12 T22^-1), the sweeps' T T^-1 - and of the triangular product, in any order, is bounded by these),
  * for the chain, (|T|^T |T|) 2^4 below 2^53 (the partial sums of the factorization of T^T T; T has at most 2 fraction bits).
A block that fails is a bad block, not a reason to loosen anything.

RANDOM BLOCKS.  random_spd(n, kappa, count): Q diag(logspace(0, -log10 kappa)) Q^T; reference(R): W* = R^-1 by substitution and X* = W* W*^T
in np.longdouble, with the two componentwise bounds |W - W*| <= gamma_3n |W*||R||W*| and |X - X*| <= gamma_8n |W*||R||W*||W*|^T on the
upper triangle."""
import functools
import math

import numpy as np

from tests import tri_cases as T

FAMILIES = ("F1", "F2", "F2i")
SMALL_N = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)
SMALL_BATCHES = (1, 2, 3, 5, 63, 64, 65, 257)
LARGE_N = (65, 66, 80, 96, 127, 128, 129, 130, 160, 191, 192, 193, 200, 255, 256)
LARGE_BATCHES = (1, 2, 5, 33)
LAYOUTS = ((0, 0), (0, 3), (1, 3), (6, 0))          # (ld - n, stride - ld n)
KAPPAS = (1e1, 1e6, 1e10)
RANDOM_N = (7, 33, 64, 65, 130, 256)
U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


@functools.lru_cache(maxsize=300)
def block(fam, n, signed, idx):
    """(T, Tinv, C = triu(Tinv Tinv^T)) of block idx, exact, read-only, premise asserted"""
    rng = np.random.default_rng([{"F1": 1, "F2": 2, "F2i": 2}[fam], n, int(signed), idx])
    d = T.DIAG[rng.integers(0, 4, size=n)]
    if signed:
        d = d * rng.choice([-1.0, 1.0], size=n)
    if fam == "F1":
        cls = T.classes(n)
        allowed = np.triu(cls[:, None] < cls[None, :], 1)
        N = np.where(allowed, rng.choice([-2.0, -1.0, 1.0, 2.0], size=(n, n)), 0.0)
        M = d[:, None] * (np.eye(n) + N)
        Mi = (np.eye(n) - N + T._square_of_n(N, cls)) / d[None, :]
    else:
        s1, s2 = rng.choice([-1.0, 1.0], size=n), rng.choice([-1.0, 1.0], size=n)
        if not signed:
            s2 = s1                       # diagonal d s1 s2 = d > 0
        M = (d * s1)[:, None] * np.triu(np.ones((n, n))) * s2[None, :]
        Mi = s2[:, None] * (np.eye(n) - np.eye(n, k=1)) * (s1 / d)[None, :]
        if fam == "F2i":
            M, Mi = Mi, M
    T._check_inverse(M, Mi)
    if not signed:
        assert np.all(np.diagonal(M) > 0)
    b = premise(M, Mi)
    for name, v in b.items():
        assert np.isfinite(v) and v < T.LIMIT, "%s n=%d block %d: %s = 2^%.1f is not below 2^53" % (fam, n, idx, name, np.log2(v))
    C = np.triu(Mi @ Mi.T)
    for a in (M, Mi, C):
        a.setflags(write=False)
    return M, Mi, C


def premise(M, Mi):
    """{name: bound x 2^fraction bits}; all must be < 2^53"""
    aM, aI = np.abs(M), np.abs(Mi)
    mi = aM @ aI
    return {"inverse |Tinv||T||Tinv| x 2^5": max(mi.max(), (aI @ aM).max(), (aI @ mi).max()) * 32,
            "product |Tinv||Tinv|^T x 2^4": (aI @ aI.T).max() * 16,
            "chain |T|^T|T| x 2^4": (aM.T @ aM).max() * 16}


def batch(fam, n, signed, count):
    """(T, Tinv, C), each (count, n, n)"""
    bl = [block(fam, n, bool(signed), i) for i in range(count)]
    return tuple(np.stack([b[k] for b in bl]) for k in range(3))


def stored(a):
    """NaN in the strictly lower triangle of every block"""
    a = np.array(a, dtype=np.float64, copy=True)
    lo = np.tril_indices(a.shape[-1], -1)
    a[..., lo[0], lo[1]] = np.nan
    return a


def exact_rows():
    """(n, fam, batch, (dl, ds)) for the exact tests: every n with every family, the batch sizes and layouts dealt round; then every NP and
    every NBLK with an odd leading dimension"""
    rows = []
    for sizes, batches in ((SMALL_N, SMALL_BATCHES), (LARGE_N, LARGE_BATCHES)):
        for k, n in enumerate(sizes):
            for f, fam in enumerate(FAMILIES):
                rows.append((n, fam, batches[(k + 3 * f) % len(batches)], LAYOUTS[(k + f) % 4]))
    for n, fam in ((8, "F1"), (16, "F2"), (32, "F2i"), (64, "F1"), (128, "F2"), (192, "F2i"), (256, "F1")):
        rows.append((n, fam, 3, (1, 3)))            # even n, ld = n + 1
    return rows


def row_id(r):
    return "n%d-%s-b%d-ld+%d-st+%d" % (r[0], r[1], r[2], r[3][0], r[3][1])


# ------------------------------------------------------------------------------------------------------------------- random blocks
def random_spd(n, kappa, count=1, seed=0):
    rng = np.random.default_rng([77, n, int(round(math.log10(kappa))), seed])
    out = np.empty((count, n, n))
    for i in range(count):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        d = np.logspace(0, -math.log10(kappa), n) if n > 1 else np.ones(1)
        M = (Q * d) @ Q.T
        out[i] = (M + M.T) / 2
    return out


def reference(R):
    """(W*, X*, bound_W, bound_X) in np.longdouble from the upper triangle of the float64 factor R: W* = R^-1 by substitution (column by column,
    all columns at once), X* = W* W*^T; bound_W = gamma_3n |W*||R||W*|, bound_X = gamma_8n |W*||R||W*||W*|^T"""
    n = R.shape[0]
    Rl = np.triu(R).astype(np.longdouble)
    W = np.eye(n, dtype=np.longdouble)
    for j in range(n - 1, -1, -1):                  # R W = I, row j of W from the rows below
        W[j, :] = (W[j, :] - Rl[j, j + 1:] @ W[j + 1:, :]) / Rl[j, j]
    W = np.triu(W)
    X = W @ W.T
    aW = np.abs(W)
    E = aW @ np.abs(Rl) @ aW
    return W, X, np.longdouble(gamma(3 * n)) * E, np.longdouble(gamma(8 * n)) * (E @ aW.T)


def check_random(R, What, Xhat):
    """the two componentwise bounds on the upper triangle; returns the largest fractions of the bounds used"""
    n = R.shape[0]
    W, X, bw, bx = reference(R)
    iu = np.triu_indices(n)
    ew = np.abs(What.astype(np.longdouble) - W)[iu]
    ex = np.abs(Xhat.astype(np.longdouble) - X)[iu]
    fw = float(np.max(ew / bw[iu]))
    fx = float(np.max(ex / bx[iu]))
    assert np.all(ew <= bw[iu]), "triangular inverse: %.3g of the bound at n = %d" % (fw, n)
    assert np.all(ex <= bx[iu]), "inverse: %.3g of the bound at n = %d" % (fx, n)
    return fw, fx
