"""CPU-only: the premises of tests/test_gpu_scratch_contract.py - what include/capital_amd.h promises of the work sizes (through the
library's own cap_*_work_size, which touch no device), that the four scratch fills are what they claim to be, that the estimator's
decision path on every cap_dpocon / cap_dpoerr row does not hang on a last bit (the float64 model and a long double one walk the same
stages, indices and number of solves), and that the lock-step rows really hold columns that finish at different solves."""
import os

import numpy as np
import pytest

from tests import poerr_model as pm
from tests import pstrf_model as psm
from tests import scratch_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


# every multiple of 64 (hence of 128, 256 and 512) up to 1100, plus and minus one
NS = sorted({m + d for m in range(64, 1101, 64) for d in (-1, 0, 1)} | {1, 2, 3, 1100})
KS = tuple(range(1, 41))


# ---- work sizes -----------------------------------------------------------------------------------------------------------------------------
def test_work_sizes_are_zero_for_an_empty_problem(L):
    for n in (0, -1):
        assert L.cap_dcholupdate_work_size(n, 5) == 0 and L.cap_dpstrf_work_size(n, 0) == 0 and L.cap_dlansy_work_size(n) == 0
        assert L.cap_dsymm_thin_work_size(n, 5) == 0 and L.cap_dpocon_work_size(n) == 0 and L.cap_dpoerr_work_size(n, 5) == 0
    for k in (0, -1):
        assert L.cap_dcholupdate_work_size(65, k) == 0 and L.cap_dsymm_thin_work_size(65, k) == 0 and L.cap_dpoerr_work_size(65, k) == 0
    for r in sc.ROWS:
        assert sc.work_size(L, r) > 0, r


def test_symm_thin_and_pstrf_work_sizes_are_monotone(L):
    for f, name in ((L.cap_dsymm_thin_work_size, "symm_thin"), (L.cap_dpstrf_work_size, "pstrf")):
        table = np.array([[f(n, k) for k in KS] for n in NS], dtype=np.int64)
        assert (table > 0).all()
        assert (np.diff(table, axis=0) >= 0).all(), "%s: not monotone in n" % name
        assert (np.diff(table, axis=1) >= 0).all(), "%s: not monotone in the second argument" % name
    # the header's lower bound of cap_dpstrf's: the factor in natural column order
    assert all(L.cap_dpstrf_work_size(n, k) >= n * k for n in NS for k in KS if k <= n)


def test_symm_thin_work_size_is_constant_beyond_sixteen_columns(L):
    for n in NS:
        at16 = L.cap_dsymm_thin_work_size(n, 16)
        assert all(L.cap_dsymm_thin_work_size(n, k) == at16 for k in range(16, 41)), n
        assert L.cap_dsymm_thin_work_size(n, 1000) == at16


def test_the_other_work_sizes_grow_with_n(L):
    """(not promised in so many words, but what every caller that sizes one buffer for several problems relies on)"""
    for f in (L.cap_dlansy_work_size, L.cap_dpocon_work_size):
        assert (np.diff([f(n) for n in NS]) >= 0).all()
    for k in KS:
        assert (np.diff([L.cap_dcholupdate_work_size(n, k) for n in NS]) >= 0).all()
        assert (np.diff([L.cap_dpoerr_work_size(n, k) for n in NS]) >= 0).all()


# ---- the fills --------------------------------------------------------------------------------------------------------------------------------
def test_the_fills_are_what_they_claim():
    count = 1000
    nan = sc.fill("nan", count)
    assert nan.dtype == np.float64 and nan.size == count and np.isnan(nan).all()
    assert np.unique(nan.view(np.int64)).size == count, "the NaN payloads are not distinct"
    assert (nan.view(np.int64) >> 51 == 0xfff).all(), "not quiet NaNs"
    assert not sc.same_bits(sc.fill("nan", count, 1), nan) and np.intersect1d(sc.fill("nan", count, 1).view(np.int64), nan.view(np.int64)).size == 0
    ones = sc.fill("ones32", count)
    assert ones.size == count and (ones.view(np.int32) == 1).all()
    assert np.isfinite(ones).all() and (ones > 0).all() and (ones < np.finfo(np.float64).tiny).all(), "not finite denormals"
    ff = sc.fill("ff", count)
    assert ff.size == count and (ff.view(np.int32) == -1).all() and (ff.view(np.uint8) == 0xFF).all() and np.isnan(ff).all()
    zero = sc.fill("zero", count)
    assert zero.size == count and (zero.view(np.int64) == 0).all()
    assert sc.FILLS == ("nan", "ones32", "ff", "zero")


def test_windows_pad_with_nan():
    M = np.arange(1.0, 13.0).reshape(3, 4)
    w = sc.window(M, 5).reshape(4, 5)
    assert np.array_equal(w[:, :3], M.T) and np.isnan(w[:, 3:]).all()
    assert np.array_equal(sc.unwindow(w.reshape(-1), 3, 4, 5), M)
    S = np.arange(1.0, 17.0).reshape(4, 4)
    u = sc.unwindow(sc.window(S, 6, upper=True), 4, 4, 6)
    assert np.array_equal(np.triu(u), np.triu(S)) and np.isnan(u[np.tril_indices(4, -1)]).all()


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_issue_table():
    assert [r.shape for r in sc.UPDATE_ROWS] == [(1, 1), (63, 2), (64, 3), (65, 4), (129, 9), (200, 17), (130, 33)]
    assert [r.shape for r in sc.PSTRF_ROWS] == [(65, 65), (130, 17), (130, 130), (300, 140)]
    assert [r.shape[0] for r in sc.LANSY_ROWS] == [1, 511, 512, 513, 1025]
    assert sorted({r.shape[:2] for r in sc.SYMM_ROWS}) == [(300, 17), (513, 1), (513, 3), (1025, 16)]
    assert {r.shape[2] for r in sc.SYMM_ROWS} == {0, 1} and len(sc.SYMM_ROWS) == 8
    assert sorted({r.shape[1] for r in sc.POCON_ROWS}) == [1, 2, 127, 128, 129, 300] and {r.shape[0] for r in sc.POCON_ROWS} == {"rand", "lap"}
    assert sorted({r.shape[:2] for r in sc.POERR_ROWS}) == [(129, 1), (129, 3), (129, 17), (300, 16)]
    assert {r.shape[2] for r in sc.POERR_ROWS} == {"both", "ferr", "berr"} and len(sc.POERR_ROWS) == 12
    for r in sc.ROWS:                                   # leading dimensions above the extent
        for name, ld in r.layout.items():
            rows = r.shape[1] if (r.entry, name) in (("cap_dpstrf", "R"), ("cap_dpocon", "R")) else r.shape[0]
            assert ld > rows, (r, name)


@pytest.mark.parametrize("row", sc.PSTRF_ROWS, ids=sc.row_id)
def test_pstrf_rows_have_separated_pivots(row):
    """the premise of "the model's pivots" (as tests/test_gpu_pstrf.py): the best and the second-best remaining diagonal never come close"""
    A, (R, piv, rank, resid, info, trace) = sc.pstrf_operands(*row.shape)
    assert psm.min_gap(trace) >= 64 * psm.gamma(rank + 2) * np.diag(A).max()
    n, mr = row.shape
    assert (rank, info) == {(65, 65): (65, 0), (130, 17): (12, 0), (130, 130): (130, 0), (300, 140): (140, 1)}[row.shape]
    psm.check_properties(A, R, piv, rank, info, psm.default_tol(A))


@pytest.mark.parametrize("row", sc.UPDATE_ROWS + sc.LANSY_ROWS + sc.SYMM_ROWS, ids=sc.row_id)
def test_expectations_exist(row):
    e = sc.expected(row)
    if row.entry == "cap_dcholupdate":
        from tests import cholupdate_model as cm
        assert cm.element_error(e["model"], e["ref"]) <= cm.ELEMENT_GATE and cm.backward_error(e["model"], e["A1"]) <= cm.BACKWARD_GATE
    elif row.entry == "cap_dlansy":
        assert e == float(int(e)) and e > 0
    else:
        assert e.shape == row.shape[:2] and np.array_equal(e, np.rint(e)) and np.abs(e).max() < 2.0 ** 40     # integers: exact in any order


# ---- the estimator's path ---------------------------------------------------------------------------------------------------------------------
def _host_factor(A):
    return np.linalg.cholesky(A).T.copy()


@pytest.mark.parametrize("row", sc.POCON_ROWS, ids=sc.row_id)
def test_pocon_rows_do_not_hang_on_a_last_bit(row):
    R = _host_factor(sc.pocon_matrix(*row.shape))
    t64, tld = sc.pocon_trace(R), sc.pocon_trace(R, sc.solver_ld)
    assert sc.traces_agree(t64, tld), (t64, tld)
    assert 1 <= t64[1] <= 11 and t64[1] == len(t64[2])
    if row.shape[1] == 1:
        assert t64[1] == 1, "the n = 1 shortcut"


@pytest.mark.parametrize("n,nrhs", sorted({r.shape[:2] for r in sc.POERR_ROWS}))
def test_poerr_rows_do_not_hang_on_a_last_bit_and_finish_at_different_solves(n, nrhs):
    A, B, X = sc.poerr_operands(n, nrhs)
    R = _host_factor(A)
    t64, tld = sc.poerr_traces(A, R, B, X), sc.poerr_traces(A, R, B, X, sc.solver_ld)
    for c in range(nrhs):
        assert sc.traces_agree(t64[c], tld[c]), (c, t64[c], tld[c])
    counts = [t[1] for t in t64]
    print("n=%d nrhs=%d: solves per column %s" % (n, nrhs, counts))
    for c0 in range(0, nrhs, 16):
        chunk = counts[c0:c0 + 16]
        if len(chunk) > 1:
            assert len(set(chunk)) > 1, "every column of the chunk finishes at the same solve: no finished column sits through a later one"
    # the guard of the backward error is far away, also when B and A are scaled by 4^-100
    d = np.abs(A) @ np.abs(X) + np.abs(B)
    assert d.min() * 4.0 ** -100 > 1e100 * pm.safe(n)[1]


def test_the_trace_does_not_change_the_result():
    R = _host_factor(sc.pocon_matrix("rand", 129))
    s = pm._solver(R)
    tr = []
    assert pm.lacn2(s, s, 129) == pm.lacn2(s, s, 129, tr) == pm.inv_norm_est(R)
    assert [t[0] for t in tr][0] == 1 and tr[-1][0] == 5 and tr[-1][2] == pm.inv_norm_est(R)[0]


def test_the_solve_count_sees_a_changed_iteration_limit(monkeypatch):
    """what the GPU test's equality of cap_pocon_last_solves and the model's count can tell apart.  The rows reach 9 solves (iteration 4 of
    dlacn2), so an iteration limit of 3 - or any stop one step early - gives another count; a limit of 4 instead of 5 would show only on a
    column that takes all 11 solves, and none was found on this family (scratch_cases.POERR_SPIKES)."""
    def counts():
        A, B, X = sc.poerr_operands(129, 17)
        return [t[1] for t in sc.poerr_traces(A, _host_factor(A), B, X)]
    base = counts()
    assert sorted(set(base)) == [5, 7, 9] and base[16] == 7, "the last chunk (one column) differs from the largest of the first"
    for limit, changed in ((4, False), (3, True), (2, True)):
        monkeypatch.setattr(pm, "ITMAX", limit)
        assert (counts() != base) == changed, limit
        monkeypatch.undo()
    assert counts() == base
