"""-m gpu: the fp64 Cholesky factorization - cap_cholinv_factor on every schedule path and cap_dpotrf - against EXACT results.

The rows of tests/chol_cases.py (tests/test_chol_cases.py shows, without a GPU, what each of them launches and that the premise of
exactness holds for it) through the C ABI.  R = diag(d) (I + N) has a power-of-two diagonal and small integer off-diagonals and
A = R^T R, so every value the factorization forms - the sweep, the explicit inverses of the diagonal blocks, the block-row products, the
Schur updates in any order and pairing, the inverse tree - is a dyadic rational far below 2^53: R and R^-1 must come out bit for bit,
whatever the schedule.  "A dropped K slice", "an update applied twice", "a strip read one event early" or "a ragged edge handled wrongly"
changes a dyadic rational, it cannot hide in rounding, and it cannot hide behind a second schedule that is wrong in the same way.

The one operation of the factorization that is not a multiplication or an addition is 1 / sqrt(pivot) in leaf.hip (v_rsq_f64 and two
Newton steps), so the first test is the probe of that premise on the device; it stays in the suite.

Everything a call must not write holds NaNs: the strictly lower triangle and the pad rows of A, and cap_dpotrf's `work`, which is all
NaN, exactly cap_dpotrf_work_size doubles long, with a 4096-double NaN sentinel behind it.  A plan's input A must be unchanged bit for
bit.  Whole buffers are compared as int64 after mapping -0.0 to +0.0 in outputs only.  There is no tolerance in this file."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import chol_cases as T  # noqa: E402
from tests.blas3_cases import describe_mismatch, place, same_bits  # noqa: E402
from tests.gpu_util import DEV  # noqa: E402

SENTINEL = 4096


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(flat):
    return torch.from_numpy(flat).to(DEV)


def _plan_outputs(L, plan, n, want_inverse):
    """(R, Rinv or None) as cap_cholinv_get_R / get_Rinv hand them out: flat column-major, ld = n"""
    out = []
    for get in (L.cap_cholinv_get_R,) + ((L.cap_cholinv_get_Rinv,) if want_inverse else ()):
        buf = _dev(np.full(n * n, T.NAN))
        assert get(plan, buf.data_ptr(), n, _stream()) == 0
        torch.cuda.synchronize()
        out.append(T.positive_zero(buf.cpu().numpy()))
    return out[0], (out[1] if want_inverse else None)


def _run_plan(c):
    L = _L()
    n, lda = c.n, c.n + c.pad
    plan = T.create_plan(L, c)
    try:
        for second in ((False, True) if c.second else (False,)):
            host = place(T.operand(c, second), lda)
            A = _dev(host)
            assert L.cap_cholinv_factor(plan, A.data_ptr(), lda, _stream()) == 0, c.id
            info = T.plan_info(L, plan, _stream())
            if c.pivot is not None:
                assert info == c.pivot + 1, (c.id, info)
                continue
            assert info == 0, (c.id, info)
            assert int(L.cap_cholinv_get_option(plan, b"count_paired")) == c.k2, (c.id, "count_paired")
            R, Rinv = T.references(c, second)
            got_r, got_i = _plan_outputs(L, plan, n, Rinv is not None)
            what = c.id + (" (second matrix)" if second else "")
            assert same_bits(got_r, place(R, n)), "%s, R: %s" % (what, describe_mismatch(got_r, place(R, n), n))
            if Rinv is not None:
                assert same_bits(got_i, place(Rinv, n)), "%s, Rinv: %s" % (what, describe_mismatch(got_i, place(Rinv, n), n))
            assert same_bits(A.cpu().numpy(), host), "%s: the input A changed" % what
    finally:
        assert L.cap_cholinv_plan_destroy(plan) == 0


def _run_dpotrf(c, host=None, want=None):
    L = _L()
    n, lda = c.n, c.n + c.pad
    host = place(T.operand(c), lda) if host is None else host
    want = place(T.dpotrf_reference(c), lda) if want is None else want
    ws = int(L.cap_dpotrf_work_size(n))
    A, work = _dev(host), _dev(np.full(ws + SENTINEL, T.NAN))
    info = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    assert L.cap_dpotrf(T.UPPER, n, A.data_ptr(), lda, info.data_ptr(), work.data_ptr(), _stream()) == 0, c.id
    torch.cuda.synchronize()
    assert int(info.item()) == 0, (c.id, int(info.item()))
    got = T.positive_zero(A.cpu().numpy())                      # the NaN lower triangle and the NaN pad rows must come back untouched
    assert same_bits(got, T.positive_zero(want)), "%s: %s" % (c.id, describe_mismatch(got, T.positive_zero(want), lda))
    tail = work[ws:].cpu().numpy()
    assert tail.size == SENTINEL and same_bits(tail, np.full(SENTINEL, T.NAN)), "%s: the sentinel behind the work buffer changed" % c.id


def test_probe_rsqrt_of_power_of_two_pivots_is_exact():
    """THE PREMISE: leaf.hip's fast_rsqrt (v_rsq_f64 + two Newton steps) returns exactly 2^-k for the pivots 1/4, 1, 4 and 16.  The factor
    of diag(d_i), n = 64, d_i cycling through the four values, must be diag(sqrt(d_i)) and its inverse diag(1 / sqrt(d_i)) bit for bit,
    through cap_dpotrf and through cap_cholinv_factor (complete_inv = 1).  Each value's outcome is printed before anything is asserted
    (profiles/r19_chol_exact.txt keeps the record)."""
    L = _L()
    n = 64
    d = np.array(T.PROBE_PIVOTS)[np.arange(n) % 4]
    A, R, Rinv = np.diag(d), np.diag(np.sqrt(d)), np.diag(1.0 / np.sqrt(d))
    assert np.array_equal(R * R, A) and np.array_equal(R * Rinv, np.eye(n))
    c = T.Case(entry="dpotrf", n=n, ci=-1, split=1, opts=(), pad=0, second=False, pivot=None, why="probe", kernels={}, gemms=0, cin=0, k2=0)
    ws = int(L.cap_dpotrf_work_size(n))
    buf, work = _dev(place(T.stored(A), n)), _dev(np.full(ws + SENTINEL, T.NAN))
    assert L.cap_dpotrf(T.UPPER, n, buf.data_ptr(), n, None, work.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got_p = np.diagonal(buf.cpu().numpy().reshape(n, n)).copy()
    plan = T.create_plan(L, T.Case(c, entry="plan", ci=1))
    src = _dev(place(T.stored(A), n))
    assert L.cap_cholinv_factor(plan, src.data_ptr(), n, _stream()) == 0
    assert T.plan_info(L, plan, _stream()) == 0
    got_r, got_i = _plan_outputs(L, plan, n, True)
    assert L.cap_cholinv_plan_destroy(plan) == 0
    diag_r, diag_i = np.diagonal(got_r.reshape(n, n)), np.diagonal(got_i.reshape(n, n))
    for k, v in enumerate(T.PROBE_PIVOTS):
        sel = np.arange(n) % 4 == k
        print("probe: pivot %-5g sqrt exact (dpotrf) %s, sqrt exact (plan) %s, 1/sqrt exact %s; first values %r %r %r" % (
            v, same_bits(got_p[sel], np.sqrt(d[sel])), same_bits(diag_r[sel], np.sqrt(d[sel])), same_bits(diag_i[sel], 1.0 / np.sqrt(d[sel])),
            float(got_p[sel][0]), float(diag_r[sel][0]), float(diag_i[sel][0])))
    assert same_bits(T.positive_zero(buf.cpu().numpy()), place(T.stored(R), n)), "cap_dpotrf of diag(d) is not diag(sqrt(d))"
    assert same_bits(got_r, place(R, n)), "R of diag(d) is not diag(sqrt(d))"
    assert same_bits(got_i, place(Rinv, n)), "R^-1 of diag(d) is not diag(1 / sqrt(d))"


@pytest.mark.parametrize("case", T.LEAF_CASES + T.BLOCK_CASES, ids=lambda c: c.id)
def test_leaf_and_diagonal_block_exact(case):
    (_run_plan if case.entry == "plan" else _run_dpotrf)(case)


@pytest.mark.parametrize("case", T.SWEEP_CASES, ids=lambda c: c.id)
def test_blocked_sweep_exact(case):
    _run_plan(case)


@pytest.mark.parametrize("case", T.DPOTRF_CASES, ids=lambda c: c.id)
def test_dpotrf_exact(case):
    _run_dpotrf(case)


@pytest.mark.parametrize("case", T.REUSE_CASES, ids=lambda c: c.id)
def test_plan_reuse_gives_the_second_matrix_exact(case):
    _run_plan(case)


@pytest.mark.parametrize("case", T.PIVOT_CASES, ids=lambda c: c.id)
def test_failing_pivot_is_reported(case):
    _run_plan(case)
