"""Exact operands for the batched symmetric rank-k products (cap_dsyrk_batched, cap_dsyrk_vbatched), shared by
tests/test_syrk_batched_cases.py (no GPU) and tests/test_gpu_syrk_batched.py / test_gpu_syrk_vbatched.py (-m gpu).  NumPy only, nothing of
torch or the GPU is imported here.

V (n x k: C = alpha V V^T + beta C_old + lambda I, whatever layout hands V over) has entries in {-2 .. 2}, C_old even integers in [-8, 8],
lambda integers in [-3, 3], alpha and beta multiples of 1/2.
THE EXACTNESS PREMISE (premise(), asserted per row by tests/test_syrk_batched_cases.py): every value the call forms - a partial sum of
v_rq v_cq in ANY order, alpha times the sum, beta c_old, their sum, and that plus lambda - is a multiple of 1/2 (2 alpha and 2 beta are
integers, c_old is even so beta c_old is an integer) bounded by |alpha| (|V||V|^T).max() + |beta| 8 + |lambda|, far below 2^52: a float64.
The expected result is therefore the one NumPy forms in float64, whatever order either side sums in."""
import functools

import numpy as np

from tests import trsm_batched_cases as TC

WAVE_N, GROUP_N, LAYOUTS = TC.WAVE_N, TC.GROUP_N, TC.LAYOUTS
KS = (1, 3, 4, 5, 16, 17, 40)
BATCHES = (1, 3, 65, 257)
AB = ((1.0, 0.0), (-1.0, 1.0), (2.0, -1.0), (0.5, 0.5), (0.0, 1.0))          # and (1, 0) with k = 0: rows with k == 0
LIMIT = 2.0 ** 52
DISTINCT = 5                            # different blocks per (n, k); a batch repeats them round
ROWS_PER_N = 4


def exact_rows():
    """(n, k, batch, trans, fill, (alpha, beta), shift, layout_c, layout_v): four rows per n; the sixteen (trans, fill, shift, beta == 0)
    combinations, k, batch, (alpha, beta) and the layouts dealt round (the large batches go to n <= 80 only: a test stays within seconds)"""
    rows = []
    for sizes in (WAVE_N, GROUP_N):
        zero, nonzero = 0, 0                                                # rows of this path with beta == 0 / != 0 so far
        for i, n in enumerate(sizes):
            for j in range(ROWS_PER_N):
                t = ROWS_PER_N * i + j
                c = t % 16
                trans, fill, shift, beta0 = c & 1, (c >> 1) & 1, (c >> 2) & 1, (c >> 3) & 1
                k = KS[(t + i) % len(KS)]
                if beta0:
                    ab = AB[0]
                    if zero % 3 == 1:
                        k = 0                                               # (1, 0) with k = 0: C <- (+ lambda I)
                    zero += 1
                else:
                    ab = AB[1 + (nonzero + nonzero // 4) % 4]
                    nonzero += 1
                b = BATCHES[(t + 2 * j) % len(BATCHES)]
                if n > 80 and b > 3:
                    b = 3 if b == 65 else 1
                rows.append((n, k, b, trans, fill, ab, shift, LAYOUTS[t % 4], LAYOUTS[(t // 4 + j) % 4]))
    return rows


def row_id(r):
    return "n%d-k%d-b%d-%s-fill%d-a%g-b%g-shift%d-c+%d+%d-v+%d+%d" % (r[0], r[1], r[2], "T" if r[3] else "N", r[4], r[5][0], r[5][1], r[6],
                                                                      r[7][0], r[7][1], r[8][0], r[8][1])


def path(n):
    return "wave" if n <= 64 else "group"


@functools.lru_cache(maxsize=None)
def operands(n, k, idx):
    """(V n x k, C_old n x n symmetric, lambda) of block idx, read-only"""
    rng = np.random.default_rng([73, n, k, idx % DISTINCT])
    V = rng.integers(-2, 3, size=(n, k)).astype(np.float64)
    C = 2.0 * rng.integers(-4, 5, size=(n, n)).astype(np.float64)
    C = np.triu(C) + np.triu(C, 1).T
    lam = float(rng.integers(-3, 4))
    V.setflags(write=False)
    C.setflags(write=False)
    return V, C, lam


def premise(V, C, lam, alpha, beta):
    """the figures the premise bounds"""
    return {"bound": abs(alpha) * (np.abs(V) @ np.abs(V).T).max(initial=0.0) + abs(beta) * 8.0 + abs(lam),
            "2 alpha": 2.0 * alpha, "2 beta": 2.0 * beta, "|C|": np.abs(C).max(initial=0.0), "|V|": np.abs(V).max(initial=0.0)}


def expected(V, C, lam, alpha, beta, shift):
    """the symmetric n x n result (its upper triangle is what the call writes); exact under the premise.  beta == 0: C is not used."""
    E = alpha * (V @ V.T)
    if beta != 0.0:
        E = E + beta * C
    if shift:
        E = E + lam * np.eye(V.shape[0])
    return E + 0.0                          # no negative zeros: t = alpha * (+0.0) is compared through positive_zero on the other side too
