"""Exact operands and tables for the batched general products (cap_dgemm_batched, cap_dgemm_vbatched_inner, cap_dgemm_vbatched_combine),
shared by tests/test_gemm_batched_cases.py, tests/test_gemm_batched_addr.py (no GPU) and tests/test_gpu_gemm_batched.py /
test_gpu_gemm_vbatched.py (-m gpu).  NumPy only, nothing of torch or the GPU is imported here.

op(A) (m x k) and op(B) (k x n) have entries in {-2 .. 2}, C_old even integers in [-8, 8], alpha and beta multiples of 1/2
(syrk_batched_cases.AB).
THE EXACTNESS PREMISE (premise(), asserted per row by tests/test_gemm_batched_cases.py): every value either side can form - a partial sum
of a_rq b_qc in ANY order, alpha times the sum, beta c_old and their sum - is a multiple of 1/2 (2 alpha and 2 beta are integers, c_old is
even so beta c_old is an integer) bounded by |alpha| (|A||B|).max() + 8 |beta|, far below 2^52: a float64.  The expected result is therefore
the one NumPy forms in float64, whatever order either side sums in, with no tolerance."""
import functools

import numpy as np

from tests import syrk_batched_cases as SC
from tests import trsm_batched_cases as TC
from tests import vbatched_cases as VC

WAVE_N, GROUP_N, LAYOUTS = TC.WAVE_N, TC.GROUP_N, TC.LAYOUTS
ALL_N = WAVE_N + GROUP_N
RECTANGLES = ((1, 200), (200, 1), (5, 64), (64, 65), (65, 3), (17, 130), (255, 256), (256, 256))
KS = (0, 1, 3, 4, 5, 16, 17, 40)
BATCHES = (1, 3, 65, 257)
AB = SC.AB
TRANS_PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1))
LIMIT = 2.0 ** 52
DISTINCT = 5                            # different blocks per (m, n, k); a batch repeats them round
MAX_DIM = 256


def shapes():
    """(m, n): every size of TC.WAVE_N and TC.GROUP_N as a square and as m with two partners drawn round from both lists (so that the
    wave path, the workgroup path and the pairs that straddle 64 all occur), then the rectangles"""
    out = []
    for i, m in enumerate(ALL_N):
        for n in (m, ALL_N[(3 * i + 1) % len(ALL_N)], ALL_N[(7 * i + 12) % len(ALL_N)]):
            if (m, n) not in out:
                out.append((m, n))
    return out + [r for r in RECTANGLES if r not in out]


def exact_rows():
    """(m, n, k, batch, transa, transb, (alpha, beta), layout_a, layout_b, layout_c): k, batch, the four trans pairs, (alpha, beta) and the
    layouts dealt round (the large batches go to max(m, n) <= 80 only: a test stays within seconds)"""
    rows = []
    for t, (m, n) in enumerate(shapes()):
        k = KS[(t + t // len(KS)) % len(KS)]
        b = BATCHES[(t + t // 4) % len(BATCHES)]
        if max(m, n) > 80 and b > 3:
            b = 3 if b == 65 else 1
        ta, tb = TRANS_PAIRS[t % 4]
        rows.append((m, n, k, b, ta, tb, AB[(t + t // 5) % len(AB)], LAYOUTS[t % 4], LAYOUTS[(t // 4) % 4], LAYOUTS[(t // 2 + 1) % 4]))
    return rows


def row_id(r):
    return "m%d-n%d-k%d-b%d-%s%s-a%g-b%g-A+%d+%d-B+%d+%d-C+%d+%d" % (r[0], r[1], r[2], r[3], "NT"[r[4]], "NT"[r[5]], r[6][0], r[6][1],
                                                                   r[7][0], r[7][1], r[8][0], r[8][1], r[9][0], r[9][1])


def path(m, n):
    return "wave" if max(m, n) <= 64 else "group"


def launches(row):
    """the launches the library is to make for a row of exact_rows()"""
    return 1 if row[0] > 0 and row[1] > 0 and row[3] > 0 else 0


@functools.lru_cache(maxsize=None)
def operands(m, n, k, idx):
    """(op(A) m x k, op(B) k x n, C_old m x n) of block idx, read-only"""
    rng = np.random.default_rng([97, m, n, k, idx % DISTINCT])
    A = rng.integers(-2, 3, size=(m, k)).astype(np.float64)
    B = rng.integers(-2, 3, size=(k, n)).astype(np.float64)
    C = 2.0 * rng.integers(-4, 5, size=(m, n)).astype(np.float64)
    for a in (A, B, C):
        a.setflags(write=False)
    return A, B, C


def premise(A, B, C, alpha, beta):
    """the figures the premise bounds"""
    return {"bound": abs(alpha) * (np.abs(A) @ np.abs(B)).max(initial=0.0) + abs(beta) * 8.0, "2 alpha": 2.0 * alpha, "2 beta": 2.0 * beta,
            "|C|": np.abs(C).max(initial=0.0), "|A|": np.abs(A).max(initial=0.0), "|B|": np.abs(B).max(initial=0.0)}


def premise_holds(A, B, C, alpha, beta):
    f = premise(A, B, C, alpha, beta)
    return (f["bound"] < LIMIT and f["2 alpha"] == round(f["2 alpha"]) and f["2 beta"] == round(f["2 beta"]) and f["|C|"] <= 8.0
            and f["|A|"] <= 2.0 and f["|B|"] <= 2.0 and np.array_equal(C % 2.0, np.zeros(C.shape))
            and np.array_equal(A, np.round(A)) and np.array_equal(B, np.round(B)))


def expected(A, B, C, alpha, beta):
    """the m x n result, exact under the premise.  beta == 0: C is not used.  No negative zeros: alpha * (+0.0) with alpha < 0 is -0.0 on
    either side, the comparison adds +0.0 to both."""
    E = alpha * (A @ B)
    if beta != 0.0:
        E = E + beta * C
    return E + 0.0


# ---- plans ----------------------------------------------------------------------------------------------------------------------------------------
def _jacobi():
    """a block-Jacobi-style mix: four in five blocks of at most 16 rows, the rest of 100 .. 200"""
    rng = np.random.default_rng([22, 40, 2])
    return tuple(int(rng.integers(1, 17)) if rng.random() < 0.8 else int(rng.integers(100, 201)) for _ in range(40))


PLAN_LISTS = {"EVERY": VC.EVERY, "WAVES": VC.WAVES, "JACOBI": _jacobi(), "EMPTIES": (0, 5, 0, 0, 70, 8, 0), "LONE256": (256,)}
INNER_PQ = ((1, 1), (3, 16), (17, 5), (64, 65))
COMBINE_NK = ((1, 1), (16, 4), (17, 40), (3, 0))
PLAN_KINDS = VC.LAYOUTS


def plan_rows():
    """(entry, list name, layout kind, (p, q) or (nrhs, k), (alpha, beta)): every list with every shape pair of both entries"""
    rows = []
    for i, name in enumerate(PLAN_LISTS):
        for j, pq in enumerate(INNER_PQ):
            rows.append(("inner", name, PLAN_KINDS[(i + j) % 4], pq, AB[(i + 2 * j) % len(AB)]))
        for j, nk in enumerate(COMBINE_NK):
            rows.append(("combine", name, PLAN_KINDS[(i + j + 1) % 4], nk, AB[(i + 2 * j + 1) % len(AB)]))
    return rows


def plan_row_id(r):
    return "%s-%s-%s-%dx%d-a%g-b%g" % (r[0], r[1], r[2], r[3][0], r[3][1], r[4][0], r[4][1])


def plan_launches(row):
    """inner: ONE launch whatever the classes (empty blocks are written too); combine: one per occurring size class"""
    sizes = PLAN_LISTS[row[1]]
    if row[0] == "inner":
        return 1 if len(sizes) and row[3][0] > 0 and row[3][1] > 0 else 0
    return len({VC.class_of(n) for n in sizes if n}) if row[3][0] > 0 else 0


@functools.lru_cache(maxsize=None)
def plan_operands(entry, name, a, b):
    """inner (p, q): per block (X_i n_i x p, Y_i n_i x q, G_old p x q); combine (nrhs, k): per block (V_i n_i x k, Z_i k x nrhs, C_old
    n_i x nrhs) - in either case the (op(A), op(B), C_old) of the block's product, from operands()"""
    out = []
    for i, n in enumerate(PLAN_LISTS[name]):
        if entry == "inner":
            A, B, C = operands(a, b, n, i)              # op(A) = X_i^T (p x n_i), op(B) = Y_i (n_i x q)
        else:
            A, B, C = operands(n, a, b, i)              # op(A) = V_i (n_i x k), op(B) = Z_i (k x nrhs)
        out.append((A, B, C))
    return out
