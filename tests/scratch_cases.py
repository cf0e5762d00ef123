"""The rows of the scratch-contract tests: the entry points that keep tickets, flags and state words in caller-provided scratch
(cap_dcholupdate, cap_dpstrf, cap_dlansy, cap_dsymm_thin, cap_dpocon, cap_dpoerr), their operands, what is expected of them, and the four
fills a scratch buffer is handed over with.  Shared by tests/test_scratch_cases.py (no GPU: the premises) and
tests/test_gpu_scratch_contract.py (-m gpu).  NumPy only, nothing of torch or the GPU is imported here.

A ROW is (entry, shape, layout): the entry point, its sizes, and the leading dimension of every operand (all above the extent - the pad
rows, and the strictly lower triangle of a triangular or symmetric operand, hold NaN).  `operands(row)` builds the logical matrices once
(they are never written), `expected(row)` what the result must be - or None where the expectation is only "the same bits for every fill"
(the estimator rows: their model runs on the factor the GPU made, tests/test_gpu_scratch_contract.py section 4).

The shapes sit on the edges of each kernel's blocking:
  update   (n, k): tile 64, NK 1 / 2 / 4 / 4 / 16 / 16 + 1 / 16 + 16 + 1; several block rows, so the `parts` counters go above 1
  pstrf    (n, max_rank): 64 columns per workgroup; lanes per column switch at steps 16 and 128; both record sets; a stop in front of the cap
  lansy    n: super-block 512 - 1, 1, 1, 3 and 6 part slots; 256-row reduce workgroups
  symm     (n, nrhs, absolute): NR 1 / 4 / 16, the 16 + 1 chunks use one work area at two widths
  pocon    (family, n): substitution block 128 - one, two, three blocks; the n = 1 shortcut
  poerr    (n, nrhs, what): one column, lock-step columns, a full chunk, a second chunk of one column; ferr and berr, ferr only, berr only"""
import collections
import functools

import numpy as np

from tests import cholupdate_model as cm
from tests import poerr_model as pm
from tests import pstrf_model as psm
from tests.vbatched_cases import nan_pattern           # quiet NaNs with a payload of their own per element

NAN = float("nan")
PRE, SENTINEL = 64, 4096                # doubles in front of and behind the work area
FILLS = ("nan", "ones32", "ff", "zero")

Row = collections.namedtuple("Row", "entry shape layout")


def row_id(r):
    return "%s-%s" % (r.entry, "x".join(str(s) for s in r.shape))


# ---- the fills ----------------------------------------------------------------------------------------------------------------------------
def fill(kind, count, salt=0):
    """`count` doubles: "nan" distinct quiet NaNs; "ones32" every 32-bit word 1 (finite denormal doubles; as ints every flag reads
    published, skip reads 1, state reads gave-up); "ff" every byte 0xFF (ints -1, doubles NaN); "zero"."""
    if kind == "nan":
        return nan_pattern(count, salt)
    if kind == "ones32":
        return np.ones(2 * count, dtype=np.int32).view(np.float64).copy()
    if kind == "ff":
        return np.full(8 * count, 0xFF, dtype=np.uint8).view(np.float64).copy()
    assert kind == "zero"
    return np.zeros(count)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def window(M, ld, upper=False):
    """the column-major window of M (rows x cols) with leading dimension ld as a flat array: pad rows - and with `upper` the strictly lower
    triangle - are NaN"""
    M = np.asarray(M, dtype=np.float64)
    rows, cols = M.shape
    assert ld >= rows
    buf = np.full((cols, ld), NAN)
    buf[:, :rows] = M.T
    if upper:
        c, r = np.triu_indices(cols, 1, rows)          # buffer (col, row) with row > col
        buf[c, r] = NAN
    return buf.reshape(-1)


def unwindow(flat, rows, cols, ld):
    return np.asarray(flat).reshape(cols, ld)[:, :rows].T.copy()


# ---- the rows -----------------------------------------------------------------------------------------------------------------------------
UPDATE_SHAPES = ((1, 1), (63, 2), (64, 3), (65, 4), (129, 9), (200, 17), (130, 33))
PSTRF_SHAPES = ((65, 65), (130, 17), (130, 130), (300, 140))
LANSY_SHAPES = ((1,), (511,), (512,), (513,), (1025,))
SYMM_SHAPES = tuple((n, r, ab) for n, r in ((513, 1), (513, 3), (300, 17), (1025, 16)) for ab in (0, 1))
POCON_NS = (1, 2, 127, 128, 129, 300)
POCON_SHAPES = tuple((fam, n) for n in POCON_NS for fam in ("rand", "lap"))
POERR_SHAPES = tuple((n, r, what) for n, r in ((129, 1), (129, 3), (300, 16), (129, 17)) for what in ("both", "ferr", "berr"))
POCON_KAPPA = 1e4           # rand_spd(n, 1e4): rcond is compared with the model at 1e-8
POERR_KAPPA = 1e2           # rand_spd(n, 1e2): ferr is compared with the model at 1e-6

UPDATE_ROWS = [Row("cap_dcholupdate", s, {"R": s[0] + 3, "V": s[0] + 5}) for s in UPDATE_SHAPES]
PSTRF_ROWS = [Row("cap_dpstrf", s, {"A": s[0] + 3, "R": s[1] + 2}) for s in PSTRF_SHAPES]
LANSY_ROWS = [Row("cap_dlansy", s, {"A": s[0] + 3}) for s in LANSY_SHAPES]
SYMM_ROWS = [Row("cap_dsymm_thin", s, {"A": s[0] + 3, "X": s[0] + 1, "B": s[0] + 5, "Y": s[0] + 7}) for s in SYMM_SHAPES]
POCON_ROWS = [Row("cap_dpocon", s, {"R": s[1] + 1}) for s in POCON_SHAPES]
POERR_ROWS = [Row("cap_dpoerr", s, {"A": s[0] + 3, "R": s[0] + 1, "B": s[0] + 3, "X": s[0] + 2}) for s in POERR_SHAPES]
ROWS = UPDATE_ROWS + PSTRF_ROWS + LANSY_ROWS + SYMM_ROWS + POCON_ROWS + POERR_ROWS


def find(entry, *shape):
    return next(r for r in ROWS if r.entry == entry and r.shape == tuple(shape))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- operands -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def update_operands(n, k):
    """A, V, R = chol(A)^T, A' = A + V V^T, chol(A')^T: the matrices of tests/test_gpu_cholupdate.py"""
    A, V = cm.spd(n, 10 + n), cm.thin(n, k, 100 + n)
    A1 = A + V @ V.T
    return _frozen(A, V, np.linalg.cholesky(A).T.copy(), A1, np.linalg.cholesky(A1).T.copy())


PSTRF_MATRIX = {(65, 65): ("dominant", 65, 0, 1), (130, 17): ("gram", 130, 12, 1), (130, 130): ("dominant", 130, 0, 2),
                (300, 140): ("dominant", 300, 0, 1)}


@functools.lru_cache(maxsize=None)
def pstrf_operands(n, max_rank):
    """(A, the model's (R, piv, rank, resid, info, trace)): full rank with well separated pivots, and a rank-12 Gram matrix whose
    factorization stops in front of the cap (the remaining step launches leave through the stop word)"""
    kind, n_, k, seed = PSTRF_MATRIX[(n, max_rank)]
    A = psm.dominant(n_, seed) if kind == "dominant" else psm.gram(n_, k, seed)
    return A, psm.pstrf(A, max_rank)


def _ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


@functools.lru_cache(maxsize=None)
def sym_int(n, seed):
    """a symmetric matrix of small integers: every sum over it is exact in any order"""
    u = np.triu(_ints(np.random.default_rng(seed), (n, n)))
    return _frozen(u + np.triu(u, 1).T)[0]


SYMM_COEF = ((1.0, 1.0), (-1.0, 1.0), (2.0, -1.0), (1.0, 2.0))


@functools.lru_cache(maxsize=None)
def symm_operands(n, nrhs, absolute):
    """A (symmetric), X, B of small integers, alpha, beta from {1, -1, 2}"""
    rng = np.random.default_rng(31 * n + nrhs)
    alpha, beta = SYMM_COEF[(n + nrhs + absolute) % len(SYMM_COEF)]
    return _frozen(sym_int(n, 17 * n), _ints(rng, (n, nrhs)), _ints(rng, (n, nrhs))) + (alpha, beta)


POCON_SEED = {}             # (family, n) -> seed of rand_spd, where the default (0) hangs on a last bit (tests/test_scratch_cases.py)


@functools.lru_cache(maxsize=None)
def pocon_matrix(family, n):
    A = pm.lap(n) if family == "lap" else pm.rand_spd(n, POCON_KAPPA, POCON_SEED.get((family, n), 0))
    return _frozen(A)[0]


POERR_SEED = {}             # n -> seed of rand_spd, as POCON_SEED
# seeds of spiked() with which the estimator of that column takes 7 solves - the second of each list 9 - where the plain columns take 5
# (found by running the model over 40000 seeds per n; none of them takes all 11)
POERR_SPIKES = {129: (32, 3399, 65, 89, 124, 134), 300: (32, 803, 45, 55, 75, 78)}


def spiked(n, seed):
    """a residual of 1e-9 with two to four entries of 0.5e-3 .. 1e-3: weights with which dlacn2's first arg max is not the last"""
    rng = np.random.default_rng(seed)
    m = int(rng.integers(2, 5))
    idx = rng.choice(n, m, replace=False)
    g = np.full(n, 1e-9)
    g[idx] = rng.uniform(0.5, 1.0, m) * 1e-3
    return g


@functools.lru_cache(maxsize=None)
def poerr_operands(n, nrhs):
    """A = rand_spd(n, 1e2), B, and X, a computed solution of A X = B.  The columns cycle through three kinds: a random b, the same with
    A^-1 spiked() added to the solution (the residual is the spikes, the estimator takes 7 or 9 solves), and a b graded over eight
    decades (tests/test_gpu_poerr._rhs).  On rand_spd(n, 1e2) every right-hand side of _rhs - random, A times ones, graded - takes
    exactly 5 solves (the first arg max is the last), so without the spiked columns no finished column would sit through a later solve:
    the lock-step premise, tests/test_scratch_cases.py.
    Every other solution is the host's Cholesky solution PERTURBED by 1e-4 relative per element (as test_berr_of_a_perturbed_solution).  The
    residual of an unperturbed fp64 solution is rounding noise of the size of the (n + 1) eps (|A||x| + |b|) term beside it, and a
    residual summed in another order - the GPU's - then moves ferr by 5e-4 relative (measured), which says nothing about the
    estimator.  With |r| about 1e-5 (|A||x| + |b|) its rounding, at most (n + 1) eps relative to the same quantity, stays below 1e-8 of
    it, far inside the 1e-6 the bound is compared at.  No element of B is zero (the power-of-two scaling test needs |A||X| + |B| far
    above the guard)."""
    import scipy.linalg as sl
    A = pm.rand_spd(n, POERR_KAPPA, POERR_SEED.get(n, 0))
    fac = (np.linalg.cholesky(A), True)
    rng = np.random.default_rng(9000 + 100 * n + nrhs)
    B, X = np.empty((n, nrhs)), np.empty((n, nrhs))
    for c in range(nrhs):
        B[:, c] = rng.standard_normal(n) * (np.logspace(0, -8, n) if c % 3 == 2 else 1.0)
        X[:, c] = sl.cho_solve(fac, B[:, c])
        if c % 3 == 1:                                   # (the spikes, 1e-3, are the residual; its 1e-9 floor carries 1e-7 of the weights)
            X[:, c] += sl.cho_solve(fac, spiked(n, POERR_SPIKES[n][(c // 3) % len(POERR_SPIKES[n])]))
        else:
            X[:, c] *= 1.0 + 1e-4 * rng.standard_normal(n)
    assert (np.abs(B) > 0).all()
    return _frozen(A, B, X)


# ---- expectations -------------------------------------------------------------------------------------------------------------------------
def expected(row):
    """what the row's outputs must be, or None where only fill independence is asked (cap_dpocon / cap_dpoerr: section 4 of the GPU file
    compares them with the model on the factor the GPU made).
      update   {"model": the sweep of cholupdate_model, "ref": chol(A'), "R": chol(A), "A", "A1"} for the gates of cholupdate_model
      pstrf    the model's (R, piv, rank, resid, info, trace) for the pivots and check_properties
      lansy    the norm, exact
      symm     Y, exact"""
    e, s = row.entry, row.shape
    if e == "cap_dcholupdate":
        A, V, R, A1, ref = update_operands(*s)
        model, info = cm.sweep(R, V, +1.0)
        assert info == 0
        return {"model": model, "ref": ref, "R": R, "A": A, "A1": A1}
    if e == "cap_dpstrf":
        return pstrf_operands(*s)[1]
    if e == "cap_dlansy":
        return float(np.abs(sym_int(s[0], 23 * s[0])).sum(0).max())
    if e == "cap_dsymm_thin":
        a, x, b, alpha, beta = symm_operands(*s)
        if s[2]:
            a, x, b = np.abs(a), np.abs(x), np.abs(b)
        return beta * b + alpha * (a @ x)
    return None


# ---- the estimator's path, in two precisions ------------------------------------------------------------------------------------------------
def solver64(R):
    return pm._solver(R)


def solver_ld(R):
    """A^-1 v = R^-1 R^-T v with both substitutions written out in long double"""
    Rl = np.asarray(R, dtype=np.longdouble)
    n = Rl.shape[0]
    dg = np.diag(Rl).copy()

    def solve(v):
        y = np.asarray(v, dtype=np.longdouble).copy()
        for i in range(n):                               # R^T y = v, column-oriented: row i of R
            y[i] /= dg[i]
            y[i + 1:] -= Rl[i, i + 1:] * y[i]
        for i in range(n - 1, -1, -1):                   # R x = y
            y[i] /= dg[i]
            y[:i] -= Rl[:i, i] * y[i]
        return y
    return solve


def pocon_trace(R, solver=solver64):
    """(est, solves, trace) of the estimator behind cap_dpocon on A = R^T R"""
    s, tr = solver(R), []
    est, solves = pm.lacn2(s, s, R.shape[0], tr)
    return float(est), solves, tr


def poerr_traces(A, R, B, X, solver=solver64):
    """per column (est, solves, trace) of the estimator behind ferr: lacn2 on diag(w) A^-1 / A^-1 diag(w)"""
    s, W, out = solver(R), pm.ferr_weights(A, B, X), []
    for j in range(X.shape[1]):
        w, tr = W[:, j], []
        est, solves = pm.lacn2(lambda v: w * s(v), lambda v: s(w * v), A.shape[0], tr)
        out.append((float(est), solves, tr))
    return out


def traces_agree(t64, tld, rel=1e-10):
    """the same stages, the same indices, the same number of solves, every estimate within `rel`"""
    (e0, s0, a), (e1, s1, b) = t64, tld
    if s0 != s1 or len(a) != len(b) or [x[:2] for x in a] != [x[:2] for x in b]:
        return False
    return all(abs(x[2] - y[2]) <= rel * abs(y[2]) for x, y in zip(a + [(0, 0, e0)], b + [(0, 0, e1)]))


def work_size(L, row):
    e, s = row.entry, row.shape
    if e == "cap_dcholupdate":
        return int(L.cap_dcholupdate_work_size(*s))
    if e == "cap_dpstrf":
        return int(L.cap_dpstrf_work_size(*s))
    if e == "cap_dlansy":
        return int(L.cap_dlansy_work_size(s[0]))
    if e == "cap_dsymm_thin":
        return int(L.cap_dsymm_thin_work_size(s[0], s[1]))
    if e == "cap_dpocon":
        return int(L.cap_dpocon_work_size(s[1]))
    assert e == "cap_dpoerr"
    return int(L.cap_dpoerr_work_size(s[0], s[1]))
