"""-m gpu: the pivoted Cholesky factorization cap_dpstrf (csrc/pstrf.hip) on padded windows - exact cases bit for bit, the fixture matrices
of tests/pstrf_model.py (same pivots as the NumPy model, then the properties of tests/pstrf_model.check_properties; the premises are
checked on the CPU in tests/test_pstrf_model.py), the stopping rules, a NaN, determinism and the Python layer.

Every call runs on windows with lda > n and ldr > max_rank whose padding - and the strictly lower triangle of A - is NaN, and A and all
padding are compared bit for bit afterwards.  Shapes: one and two columns, 63 / 64 / 65 and 129 / 130 columns (a workgroup owns 64), ranks
that cross the 16- and 128-step switches of the lanes-per-column split and, at n = 1100, the 1024-entry LDS chunk of the pivot column."""
import functools

import numpy as np
import pytest
import torch

from tests import pstrf_model as pm
from tests.gpu_util import NanWork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK = 0
NAN = float("nan")


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int64)


def _a_window(A, pad=3):
    """column-major device window of the symmetric NumPy matrix A, ld = n + pad: padding rows and the strictly lower triangle are NaN"""
    n = A.shape[0]
    buf = torch.full((n, n + pad), NAN, dtype=torch.float64, device=DEV)
    buf[:, :n] = torch.from_numpy(np.array(A.T, order="C")).to(DEV)
    low = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), diagonal=1)       # buffer (col, row) with row > col
    buf[:, :n][low] = NAN
    return buf


def _dpstrf(A, max_rank=None, tol=-1.0):
    """(R, piv, rank, info, resid) of cap_dpstrf on padded windows, as NumPy / Python values; asserts CAP_OK and that A, the padding of R
    and nothing else changed"""
    L = _L()
    n = A.shape[0]
    mr = n if max_rank is None else max_rank
    Abuf = _a_window(A)
    abits = _bits(Abuf).clone()
    ldr = mr + 2
    Rbuf = torch.full((n, ldr), NAN, dtype=torch.float64, device=DEV)
    piv = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    out_rank = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    out_info = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    out_resid = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
    work = NanWork(L.cap_dpstrf_work_size(n, mr))                    # all NaN, exactly the stated size, a sentinel of 4096 behind it
    st = L.cap_dpstrf(1, n, mr, float(tol), Abuf.data_ptr(), Abuf.shape[1], Rbuf.data_ptr(), ldr, piv.data_ptr(), out_rank.data_ptr(),
                      out_resid.data_ptr(), out_info.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == OK
    assert torch.equal(_bits(Abuf), abits), "A or its padding was written"
    assert bool(torch.isnan(Rbuf[:, mr:]).all()), "padding rows of R were written"
    assert int(piv[n]) == -7 and int(out_rank[1]) == -7 and int(out_info[1]) == -7 and bool(torch.isnan(out_resid[1]))
    work.check("cap_dpstrf(n = %d, max_rank = %d)" % (n, mr))
    R = Rbuf[:, :mr].t().cpu().numpy().copy()
    return R, piv[:n].cpu().numpy(), int(out_rank[0]), int(out_info[0]), float(out_resid[0])


@functools.lru_cache(maxsize=None)
def _model(kind, n, k, seed, max_rank=None, tol=-1.0):
    A = {"gram": lambda: pm.gram(n, k, seed), "dominant": lambda: pm.dominant(n, seed), "rbf": lambda: pm.rbf(n, seed),
         "graded": lambda: pm.graded(n, k, seed)}[kind]()
    out = pm.pstrf(A, max_rank, tol)
    for x in out[:2]:
        x.setflags(write=False)
    return (A,) + out


def _same_as_model(got, want):
    """R, piv, rank, info and resid bit for bit"""
    R, piv, rank, info, resid = got
    Rm, pivm, rankm, residm, infom, _ = want
    assert (rank, info) == (rankm, infom)
    assert np.array_equal(piv, pivm)
    assert np.array_equal(np.ascontiguousarray(R).view(np.int64), np.ascontiguousarray(Rm).view(np.int64)), "R differs from the model"
    assert resid == residm


# ---- 1. exact cases: no tolerance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_diagonal_of_perfect_squares(n):
    A = pm.squares(n)
    dg = np.diag(A)
    order = np.argsort(-dg, kind="stable")
    for mr in sorted({0, 1, n // 2, n}):
        R, piv, rank, info, resid = _dpstrf(A, mr)
        assert rank == mr and info == (0 if mr == n else 1)
        assert np.array_equal(piv[:mr], order[:mr]) and np.array_equal(piv[mr:], np.sort(order[mr:]))
        want = np.zeros((mr, n))
        want[np.arange(mr), np.arange(mr)] = np.sqrt(dg[order[:mr]])              # exact roots
        assert np.array_equal(R.view(np.int64), want.view(np.int64))
        assert resid == dg[order[mr:]].sum()
        _same_as_model((R, piv, rank, info, resid), pm.pstrf(A, mr))


def test_ties_go_to_the_lowest_index():
    n = 130
    A = 2.0 * np.eye(n)
    R, piv, rank, info, resid = _dpstrf(A)
    assert np.array_equal(piv, np.arange(n)) and (rank, info, resid) == (n, 0, 0.0)
    assert np.array_equal(R, np.sqrt(2.0) * np.eye(n))
    R, piv, rank, info, resid = _dpstrf(A, 70)
    assert np.array_equal(piv, np.arange(n)) and (rank, info, resid) == (70, 1, 120.0)


@pytest.mark.parametrize("flip", [0, 1, 2])
@pytest.mark.parametrize("n", [2, 7, 12])
def test_integer_matrices_bit_for_bit(n, flip):
    """the largest diagonal entry at index 0 (every A(p, c) is A[p, c]), at n - 1 (every A(p, c) is A[c, p]) and shuffled (both), nonzero
    integers off the diagonal, every operation exact: the model's bits"""
    A, T, perm = pm.exact_integer(n, flip)
    for mr in (n, n // 2):
        got = _dpstrf(A, mr)
        _same_as_model(got, pm.pstrf(A, mr))
        assert np.array_equal(got[1][:mr], perm[:mr])
        assert np.array_equal(got[0][:, np.argsort(got[1])], T[:mr][:, np.argsort(perm)])


# ---- 2. the model's pivots, then the properties -------------------------------------------------------------------------------------------------
def _check(A, got, want, tol_used, rows=None, same_piv=True):
    R, piv, rank, info, resid = got
    Rm, pivm, rankm, residm, infom, trace = want
    if same_piv:
        assert (rank, info) == (rankm, infom)
        assert np.array_equal(piv, pivm), "pivots differ from the model's"
    ratio = pm.check_properties(A, R, piv, rank, info, tol_used, rows)
    mine = pm.remaining_diagonal(A, R, piv, rank).sum()
    bound = 2 * pm.gamma(A.shape[0]) * np.trace(A)
    print("n=%d rank=%d info=%d: backward error %.3f of the bound, resid %.6e (own remaining diagonal %.6e, bound on the difference %.2e)"
          % (A.shape[0], rank, info, ratio, resid, mine, bound))
    assert abs(resid - mine) <= bound
    return ratio


GRAM = [(300, 40), (513, 64), (1030, 17), (63, 9), (64, 9), (129, 12)]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n,k", GRAM)
def test_gram_matrices(n, k, seed):
    A, *want = _model("gram", n, k, seed)
    assert pm.min_gap(want[5]) >= 64 * pm.gamma(want[2] + 2) * np.diag(A).max()
    _check(A, _dpstrf(A, min(n, k + 8)), want, pm.default_tol(A))


@pytest.mark.parametrize("n,seed", [(65, 1), (65, 2), (65, 3), (200, 1), (200, 2), (200, 3), (1100, 3)])
def test_full_rank_matrices(n, seed):
    A, *want = _model("dominant", n, 0, seed)
    assert pm.min_gap(want[5]) >= 64 * pm.gamma(want[2] + 2) * np.diag(A).max()
    _check(A, _dpstrf(A), want, pm.default_tol(A), None if n <= 600 else pm.sample_rows(n))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rbf_kernel_matrix(seed):
    """pivots tie: properties only, and the rank within 2 of the model's"""
    A, *want = _model("rbf", 400, 0, seed)
    got = _dpstrf(A, 64)
    assert got[3] == 0 and abs(got[2] - want[2]) <= 2
    _check(A, got, want, pm.default_tol(A), same_piv=False)


# ---- 3. stopping --------------------------------------------------------------------------------------------------------------------------------
def test_rank_cap():
    A, *full = _model("gram", 300, 40, 1)
    _, *want = _model("gram", 300, 40, 1, 25)
    got = _dpstrf(A, 25)
    assert (got[2], got[3]) == (25, 1)
    _check(A, got, want, pm.default_tol(A))
    assert got[4] > 1e3 * pm.default_tol(A)


def test_absolute_tolerance_between_two_pivots():
    A, *full = _model("graded", 80, 6, 1)
    k = 3
    tol = pm.tol_between([b for b, _ in full[5]["picks"]], k)
    _, *want = _model("graded", 80, 6, 1, None, tol)
    got = _dpstrf(A, None, tol)
    assert (got[2], got[3]) == (k, 0)
    _check(A, got, want, tol)
    got = _dpstrf(A, 20, tol)                            # the cap above the stop changes nothing
    assert (got[2], got[3]) == (k, 0)


def test_zero_matrix_and_rank_zero():
    R, piv, rank, info, resid = _dpstrf(np.zeros((70, 70)))
    assert (rank, info, resid) == (0, 0, 0.0) and np.array_equal(piv, np.arange(70)) and np.all(R == 0)
    A = pm.dominant(65, 1)
    R, piv, rank, info, resid = _dpstrf(A, 0)
    assert (rank, info) == (0, 1) and np.array_equal(piv, np.arange(65))
    assert abs(resid - np.trace(A)) <= 2 * pm.gamma(65) * np.trace(A)
    R, piv, rank, info, resid = _dpstrf(A, 0, 5.0)       # every diagonal entry is below 5
    assert (rank, info) == (0, 0)


# ---- 4. NaN ---------------------------------------------------------------------------------------------------------------------------------------
def test_nan_in_the_upper_triangle():
    A = pm.dominant(65, 1).copy()
    A[3, 40] = NAN
    Rm, pivm, rankm, residm, infom, _ = pm.pstrf(A)
    R, piv, rank, info, resid = _dpstrf(A)              # asserts CAP_OK
    assert infom == 2 and (rank, info) == (rankm, 2)
    assert np.array_equal(piv[:rank], pivm[:rank]) and sorted(piv.tolist()) == list(range(65)) and np.all(np.diff(piv[rank:]) > 0)
    assert np.all(R[rank:] == 0)
    A = pm.dominant(65, 1).copy()
    A[64, 64] = NAN
    R, piv, rank, info, resid = _dpstrf(A)
    assert (rank, info) == (0, 2) and np.array_equal(piv, np.arange(65)) and np.all(R == 0)


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    A = pm.gram(513, 64, 2)
    a, b = _dpstrf(A, 80), _dpstrf(A, 80)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1])
    assert a[2:4] == b[2:4] and np.float64(a[4]).view(np.int64) == np.float64(b[4]).view(np.int64)
    A = pm.dominant(200, 2)
    a, b = _dpstrf(A), _dpstrf(A)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 6. the Python layer ------------------------------------------------------------------------------------------------------------------------
def test_python_layer():
    from capital_amd import cholinv, lapack
    from capital_amd.matrix import matrix
    A, *want = _model("gram", 300, 40, 1)
    n = 300
    Am = matrix(n, n, 1, 1).from_numpy(A)
    f = cholinv.factor_pivoted(Am)                       # max_rank = None: n
    assert f.R.num_rows_global() == n and f.R.num_columns_global() == n and f.piv.dtype == torch.int64
    assert (f.rank, f.info) == (40, 0)
    _check(A, (f.R.to_numpy(), f.piv.cpu().numpy(), f.rank, f.info, f.residual_trace), want, pm.default_tol(A))
    f0 = cholinv.factor_pivoted(Am, 0)
    assert f0.R is None and (f0.rank, f0.info) == (0, 1)
    with pytest.raises(Exception):
        cholinv.factor_pivoted(Am, n + 1)
    # the engine call on caller-owned windows
    Abuf = _a_window(A)
    mr, ldr = 48, 50
    Rbuf = torch.full((n, ldr), NAN, dtype=torch.float64, device=DEV)
    piv = torch.empty(n, dtype=torch.int64, device=DEV)
    pack = lapack.ArgPack_pstrf(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    rank, info, resid = lapack.engine._pstrf(Abuf, Rbuf, piv, n, mr, Abuf.shape[1], ldr, -1.0, pack)
    assert (rank, info) == (40, 0)
    _check(A, (Rbuf[:, :mr].t().cpu().numpy().copy(), piv.cpu().numpy(), rank, info, resid), want, pm.default_tol(A))
    assert bool(torch.isnan(Rbuf[:, mr:]).all())
