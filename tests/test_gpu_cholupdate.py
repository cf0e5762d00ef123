"""-m gpu: the rank-k update / downdate of the fp64 Cholesky factor - cap_dcholupdate on padded windows against np.linalg.cholesky and the
NumPy model of the sweep (tests/cholupdate_model.py: same inputs, same gates), failing downdates, cap_cholinv_update on a plan (the caches
of solve / inverse follow the new factor), both drivers bit for bit, the recovery launch, and the Python layer."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import cholupdate_model as cm
from tests.gpu_util import NanWork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, 1, 4
NAN = float("nan")


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(n, k):
    """(A, V, R = chol(A)^T, A' = A + V V^T, chol(A')^T), all NumPy, computed once per shape and never written"""
    A, V = cm.spd(n, 10 + n), cm.thin(n, k, 100 + n)
    A1 = A + V @ V.T
    out = (A, V, np.linalg.cholesky(A).T, A1, np.linalg.cholesky(A1).T)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _model(n, k):
    A, V, R, A1, ref = _case(n, k)
    R1, info = cm.sweep(R, V, +1.0)
    assert info == 0
    R1.setflags(write=False)
    return R1


def _window(M, ld, tri):
    """column-major device window of the NumPy matrix M (rows x cols) with leading dimension ld: (buffer[col, row], view[row, col]);
    padding rows - and with tri the strictly lower triangle - are NaN"""
    rows, cols = M.shape
    buf = torch.full((cols, ld), NAN, dtype=torch.float64, device=DEV)
    buf[:, :rows] = torch.from_numpy(np.array(M.T, order="C")).to(DEV)
    if tri:
        low = torch.triu(torch.ones(cols, rows, dtype=torch.bool, device=DEV), diagonal=1)     # buffer (col, row) with row > col
        buf[:, :rows][low] = NAN
    return buf, buf[:, :rows].t()


def _only_upper_touched(buf, n):
    low = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), diagonal=1)
    up = ~low
    return (bool(torch.isnan(buf[:, :n][low]).all()) and bool(torch.isnan(buf[:, n:]).all()) and bool(torch.isfinite(buf[:, :n][up]).all()))


def _bits(t):
    return t.contiguous().view(torch.int64)


def _dcholupdate(sign, n, k, Rbuf, Vbuf, info=None):
    """(scratch: all NaN, exactly the stated size, a sentinel behind it)"""
    L = _L()
    work = NanWork(L.cap_dcholupdate_work_size(n, k))
    st = L.cap_dcholupdate(1, sign, n, k, Rbuf.data_ptr(), Rbuf.shape[1], Vbuf.data_ptr(), Vbuf.shape[1],
                           info.data_ptr() if info is not None else None, work.data_ptr(), _stream())
    work.check("cap_dcholupdate(n = %d, k = %d)" % (n, k))
    return st


def _upper(view):
    return np.triu(view.cpu().numpy())


# ---- 1. the operator --------------------------------------------------------------------------------------------------------------------------
# every n (one and two rows, around one and two tiles of 64, several block rows, a ragged last block) and every k (one column, a padded
# pass, a full pass, a second pass of one column, three passes) appear
OPERATOR_CASES = [(1, 1), (1, 17), (2, 5), (2, 40), (63, 16), (63, 1), (64, 17), (64, 5), (65, 40), (65, 16), (127, 1), (127, 17),
                  (128, 5), (128, 40), (129, 17), (129, 16), (300, 1), (300, 40), (517, 5), (517, 40),
                  # launch_pass<2> and <4> (k = 2 and 3 / 4) and a 1 / 8 / 16 + 16 + 1 mix on several block rows: the two instantiations the
                  # rows above do not reach get an accuracy check of their own
                  (65, 2), (129, 2), (64, 3), (200, 4), (129, 9), (130, 33)]


@pytest.mark.parametrize("n,k", OPERATOR_CASES)
def test_update_then_downdate_on_padded_windows(n, k):
    A, V, R, A1, ref = _case(n, k)
    Rbuf, Rv = _window(R, n + 3, True)
    Vbuf, Vv = _window(V, n + 5, False)
    vbits = _bits(Vbuf).clone()
    info = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    assert _dcholupdate(+1, n, k, Rbuf, Vbuf, info) == OK
    assert int(info.item()) == 0
    assert _only_upper_touched(Rbuf, n), "strictly lower triangle or padding rows of R written, or the upper triangle is not finite"
    assert torch.equal(_bits(Vbuf), vbits), "V was written"
    R1 = _upper(Rv)
    scale = np.abs(ref).max()
    e_ref, e_model, e_b = cm.element_error(R1, ref), np.abs(R1 - _model(n, k)).max() / scale, cm.backward_error(R1, A1)
    print("n=%d k=%d update: elementwise %.2e (NumPy cholesky) %.2e (model), backward %.2e" % (n, k, e_ref, e_model, e_b))
    assert e_ref <= cm.ELEMENT_GATE and e_model <= cm.ELEMENT_GATE and e_b <= cm.BACKWARD_GATE
    info.fill_(77)
    assert _dcholupdate(-1, n, k, Rbuf, Vbuf, info) == OK
    assert int(info.item()) == 0
    assert _only_upper_touched(Rbuf, n) and torch.equal(_bits(Vbuf), vbits)
    R2 = _upper(Rv)
    d_e, d_b = cm.element_error(R2, R), cm.backward_error(R2, A)
    print("n=%d k=%d downdate: elementwise %.2e (the original R), backward %.2e" % (n, k, d_e, d_b))
    assert d_e <= cm.ELEMENT_GATE and d_b <= cm.BACKWARD_GATE


@pytest.mark.parametrize("n,k", [(4229, 16), (2125, 33)])
def test_larger_sizes(n, k):
    """4229: 67 block rows, 2278 items - more than the chip holds workgroups at once, so tickets outlive the first residency.  2125 x 33:
    three passes over 34 block rows.  (Errors formed on the GPU.)"""
    A, V, R, A1, ref = _case(n, k)
    Rbuf, Rv = _window(R, n + 1, True)
    Vbuf, _ = _window(V, n, False)
    info = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    assert _dcholupdate(+1, n, k, Rbuf, Vbuf, info) == OK
    assert int(info.item()) == 0 and _only_upper_touched(Rbuf, n)

    def errors(Rview, target, factor):
        U = torch.triu(Rview)
        T, F = torch.from_numpy(target).to(DEV), torch.triu(torch.from_numpy(factor).to(DEV))
        return ((torch.linalg.norm(U.T @ U - T) / torch.linalg.norm(T)).item(), ((U - F).abs().max() / F.abs().max()).item())
    e_b, e_e = errors(Rv, A1, ref)
    assert _dcholupdate(-1, n, k, Rbuf, Vbuf, info) == OK
    assert int(info.item()) == 0 and _only_upper_touched(Rbuf, n)
    d_b, d_e = errors(Rv, A, R)
    print("n=%d k=%d: update backward %.2e elementwise %.2e | downdate backward %.2e elementwise %.2e" % (n, k, e_b, e_e, d_b, d_e))
    assert e_b <= cm.BACKWARD_GATE and d_b <= cm.BACKWARD_GATE and e_e <= cm.ELEMENT_GATE and d_e <= cm.ELEMENT_GATE


@pytest.mark.parametrize("r0", [0, 127, 128, 299])
def test_failing_downdate_reports_its_row(r0):
    n = 300
    R = _case(n, 1)[2]
    V = 1.5 * R[r0, :].reshape(n, 1)
    Rbuf, Rv = _window(R, n + 3, True)
    Vbuf, _ = _window(V, n, False)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _dcholupdate(-1, n, 1, Rbuf, Vbuf, info) == OK
    assert int(info.item()) == r0 + 1
    got = Rv.cpu().numpy()
    for r in range(r0):
        assert np.array_equal(got[r, r:], R[r, r:]), "row %d above the failing one changed" % r
    assert math.isnan(got[r0, r0])
    low = torch.triu(torch.ones(n, n, dtype=torch.bool, device=DEV), diagonal=1)
    assert bool(torch.isnan(Rbuf[:, :n][low]).all()) and bool(torch.isnan(Rbuf[:, n:]).all())


def test_info_may_be_null_and_empty_calls_touch_nothing():
    n, k = 65, 5
    A, V, R, A1, ref = _case(n, k)
    Rbuf, Rv = _window(R, n, True)
    Vbuf, _ = _window(V, n, False)
    assert _dcholupdate(+1, n, k, Rbuf, Vbuf, None) == OK
    assert cm.element_error(_upper(Rv), ref) <= cm.ELEMENT_GATE
    before = _bits(Rbuf).clone()
    info = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    assert _dcholupdate(+1, n, 0, Rbuf, Vbuf, info) == OK and _dcholupdate(-1, 0, k, Rbuf, Vbuf, info) == OK
    assert torch.equal(_bits(Rbuf), before) and int(info.item()) == 77
    assert _L().cap_dcholupdate(0, 1, n, k, Rbuf.data_ptr(), n, Vbuf.data_ptr(), n, None, Rbuf.data_ptr(), _stream()) == UNSUPPORTED


# ---- 2. the plan ------------------------------------------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, n, ci=-1, driver=None):
        self.n, self.h = n, C.c_void_p()
        assert _L().cap_cholinv_plan_create(C.byref(self.h), n, ci, 1, -2, b"U", None) == 0
        if driver is not None:
            assert _L().cap_cholinv_set_option(self.h, b"chud_kernel", driver) == 0
            assert _L().cap_cholinv_get_option(self.h, b"chud_kernel") == driver

    def factor(self, a):
        A = torch.from_numpy(np.array(a, order="C")).to(DEV)                # symmetric: column-major as well
        assert _L().cap_cholinv_factor(self.h, A.data_ptr(), self.n, _stream()) == 0

    def update(self, sign, Vbuf, k=None):
        return _L().cap_cholinv_update(self.h, sign, Vbuf.data_ptr(), Vbuf.shape[1], Vbuf.shape[0] if k is None else k, _stream())

    def solve(self, b):
        Bbuf, _ = _window(b, self.n, False)
        Xbuf = torch.empty_like(Bbuf)
        assert _L().cap_cholinv_solve(self.h, Bbuf.data_ptr(), self.n, Xbuf.data_ptr(), self.n, b.shape[1], _stream()) == 0
        torch.cuda.synchronize()
        return Xbuf.t().cpu().numpy()

    def inverse(self):
        X = torch.empty(self.n, self.n, dtype=torch.float64, device=DEV)
        assert _L().cap_cholinv_inverse(self.h, X.data_ptr(), self.n, 1, _stream()) == 0
        torch.cuda.synchronize()
        return X.cpu().numpy()

    def logdet(self):
        out = torch.zeros(1, dtype=torch.float64, device=DEV)
        assert _L().cap_cholinv_logdet(self.h, out.data_ptr(), _stream()) == 0
        return out.item()

    def R(self):
        R = torch.empty(self.n, self.n, dtype=torch.float64, device=DEV)
        assert _L().cap_cholinv_get_R(self.h, R.data_ptr(), self.n, _stream()) == 0
        torch.cuda.synchronize()
        return R                                                        # buffer [col, row]

    def info(self):
        v = C.c_int64(0)
        _L().cap_cholinv_info(self.h, _stream(), C.byref(v))
        return v.value

    def __del__(self):
        _L().cap_cholinv_plan_destroy(self.h)


def _rel(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


def test_plan_update_refreshes_what_solve_and_inverse_cache():
    """factor, solve and inverse (they fill the block-inverse cache and the cached R^-1), update, then all three must speak of A' - they
    speak of A if the update does not start a new generation.  1e-12: the bound of the solve and inverse tests at cond < 10; the
    log-determinant against slogdet within the factor's backward error 16 n cond 2^-53, as in the test of cap_cholinv_logdet."""
    n, k = 517, 5
    A, V, R, A1, ref = _case(n, k)
    b = np.random.default_rng(7).random((n, 3)) * 2 - 1
    p = Plan(n)
    Vbuf, _ = _window(V, n + 2, False)
    p.factor(A)
    assert _rel(p.solve(b), np.linalg.solve(A, b)) <= 1e-12
    assert _rel(p.inverse(), np.linalg.inv(A)) <= 1e-12
    assert p.update(+1, Vbuf) == OK
    assert _rel(p.solve(b), np.linalg.solve(A1, b)) <= 1e-12
    assert _rel(p.inverse(), np.linalg.inv(A1)) <= 1e-12
    assert abs(p.logdet() - np.linalg.slogdet(A1)[1]) <= 16 * n * np.linalg.cond(A1) * 2.0 ** -53
    assert p.info() == 0
    assert p.update(-1, Vbuf) == OK
    assert _rel(p.solve(b), np.linalg.solve(A, b)) <= 1e-12
    assert _rel(p.inverse(), np.linalg.inv(A)) <= 1e-12
    assert abs(p.logdet() - np.linalg.slogdet(A)[1]) <= 16 * n * np.linalg.cond(A) * 2.0 ** -53
    assert p.info() == 0
    assert p.update(+1, Vbuf, 0) == OK                                    # k = 0: nothing to do


def test_plan_refusals():
    n, k = 129, 5
    A, V, R, A1, ref = _case(n, k)
    Vbuf, _ = _window(V, n, False)
    for ci in (0, 1):
        p = Plan(n, ci)
        p.factor(A)
        assert p.update(+1, Vbuf) == UNSUPPORTED and p.update(-1, Vbuf) == UNSUPPORTED
    p = Plan(n)
    assert p.update(+1, Vbuf) == ARG                                      # never factored
    p.factor(A)
    before = _bits(p.R()).clone()
    L = _L()
    assert p.update(0, Vbuf) == ARG and p.update(2, Vbuf) == ARG
    assert L.cap_cholinv_update(p.h, 1, None, n, k, _stream()) == ARG
    assert L.cap_cholinv_update(p.h, 1, Vbuf.data_ptr(), n - 1, k, _stream()) == ARG
    assert L.cap_cholinv_update(p.h, 1, Vbuf.data_ptr(), n, -1, _stream()) == ARG
    assert torch.equal(_bits(p.R()), before), "a refused call changed the factor"
    assert L.cap_cholinv_set_option(p.h, b"chud_kernel", 2) == ARG


def test_plan_failing_downdate_is_reported_until_the_next_factor():
    n, r0 = 300, 128
    A = _case(n, 1)[0]
    b = np.ones((n, 2))
    p = Plan(n)
    p.factor(A)
    row = p.R()[:, r0].clone()                                             # row r0 of R: buffer [col, row]
    Vbuf = (1.5 * row).reshape(1, n).contiguous()
    assert p.update(-1, Vbuf) == OK
    assert p.info() == r0 + 1
    assert np.isnan(p.solve(b)).all() and math.isnan(p.logdet()) and np.isnan(p.inverse()).all()
    # the report is already nonzero: R and the report stay as they are
    lost = _bits(p.R()).clone()
    good, _ = _window(cm.thin(n, 3, 5), n, False)
    assert p.update(+1, good) == OK
    assert p.info() == r0 + 1 and torch.equal(_bits(p.R()), lost)
    p.factor(A)
    assert p.info() == 0
    assert _rel(p.solve(b), np.linalg.solve(A, b)) <= 1e-12


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------------
def _plan_result(n, k, sign, driver):
    A, V, R, A1, ref = _case(n, k)
    p = Plan(n, -1, driver)
    p.factor(A if sign > 0 else A1)                                        # the downdate starts from A' (A - V V^T need not be definite)
    Vbuf, _ = _window(V, n, False)
    assert p.update(sign, Vbuf) == OK
    out = p.R()
    assert p.info() == 0
    return p, Vbuf, out


@pytest.mark.parametrize("n,k", [(517, 40), (4229, 16)])
@pytest.mark.parametrize("sign", [+1, -1])
def test_both_drivers_give_the_same_bits_twice(n, k, sign):
    _, _, one = _plan_result(n, k, sign, 1)
    _, _, again = _plan_result(n, k, sign, 1)
    _, _, step = _plan_result(n, k, sign, 0)
    assert torch.equal(_bits(one), _bits(again)), "two runs of the one-launch driver differ"
    assert torch.equal(_bits(one), _bits(step)), "the stepwise driver and the one-launch driver differ"
    A, V, R, A1, ref = _case(n, k)
    target = ref if sign > 0 else R
    assert cm.element_error(one.t().cpu().numpy(), target) <= cm.ELEMENT_GATE


def test_recovery_launch_finishes_an_injected_give_up():
    L = _L()
    n, k = 517, 40
    _, _, want = _plan_result(n, k, +1, 1)
    before = L.cap_update_fallbacks()
    assert before >= 0
    assert L.cap_update_inject_timeouts(1) == 0
    p, Vbuf, got = _plan_result(n, k, +1, 1)
    assert L.cap_update_fallbacks() == before + 1
    assert torch.equal(_bits(got), _bits(want)), "the recovery launch computes other bits"
    assert p.update(-1, Vbuf) == OK and p.info() == 0
    assert L.cap_update_fallbacks() == before + 1                         # the hook was used up
    assert cm.element_error(p.R().t().cpu().numpy(), _case(n, k)[2]) <= cm.ELEMENT_GATE


# ---- 4. Python --------------------------------------------------------------------------------------------------------------------------------
def test_python_interfaces():
    from capital_amd import cholinv, lapack
    from capital_amd.matrix import matrix
    n, k = 300, 5
    A, V, R, A1, ref = _case(n, k)
    Am = matrix(n, n, 1, 1); Am.from_numpy(A)
    Vm = matrix(k, n, 1, 1); Vm.from_numpy(V)
    pack = cholinv.info(-1, 1, -2, 'U')
    with pytest.raises(Exception):
        cholinv.update(Vm, pack)                                           # no factor yet
    cholinv.factor(Am, pack, None)
    cholinv.update(Vm, pack)
    assert cm.element_error(cholinv.construct_R(pack).to_numpy(), ref) <= cm.ELEMENT_GATE
    cholinv.downdate(Vm, pack)
    assert cm.element_error(cholinv.construct_R(pack).to_numpy(), R) <= cm.ELEMENT_GATE
    rowmajor = torch.from_numpy(V.copy()).to(DEV)                          # (n, k) row-major: goes through a column-major copy
    assert rowmajor.stride(0) != 1
    cholinv.update(rowmajor, pack, sign=+1)
    assert cm.element_error(cholinv.construct_R(pack).to_numpy(), ref) <= cm.ELEMENT_GATE
    assert torch.equal(rowmajor.cpu(), torch.from_numpy(V.copy()))
    colmajor = torch.from_numpy(np.ascontiguousarray(V.T)).to(DEV).t()     # (n, k) column-major: used in place
    cholinv.downdate(colmajor, pack)
    assert cm.element_error(cholinv.construct_R(pack).to_numpy(), R) <= cm.ELEMENT_GATE
    v1 = torch.from_numpy(V[:, 0].copy()).to(DEV)                          # (n,)
    cholinv.update(v1, pack)
    assert cm.element_error(cholinv.construct_R(pack).to_numpy(), np.linalg.cholesky(A + np.outer(V[:, 0], V[:, 0])).T) <= cm.ELEMENT_GATE
    assert pack.last_info() == 0
    with pytest.raises(Exception):
        cholinv.update(Vm, pack, sign=0)
    with pytest.raises(Exception):
        cholinv.update(torch.zeros(n + 1, 2, dtype=torch.float64, device=DEV), pack)
    # lapack::engine
    up, cmaj = lapack.UpLo.AlapackUpper, lapack.Order.AlapackColumnMajor
    assert lapack.ArgPack_cholupdate(cmaj, up).method == lapack.Method.AlapackCholupdate
    Rt = torch.from_numpy(np.ascontiguousarray(A.T)).to(DEV)
    assert lapack.engine._potrf(Rt, n, n, lapack.ArgPack_potrf(cmaj, up)) == 0
    Vt = torch.from_numpy(np.ascontiguousarray(V.T)).to(DEV)               # buffer [col, row]
    assert lapack.engine._cholupdate(Rt, Vt, n, k, n, n, +1, lapack.ArgPack_cholupdate(cmaj, up)) == 0
    assert cm.element_error(Rt.t().cpu().numpy(), ref) <= cm.ELEMENT_GATE
    assert lapack.engine._cholupdate(Rt, Vt, n, k, n, n, -1, lapack.ArgPack_cholupdate(cmaj, up)) == 0
    assert cm.element_error(Rt.t().cpu().numpy(), R) <= cm.ELEMENT_GATE
    big = torch.from_numpy(np.ascontiguousarray((1.5 * R[7, :]).reshape(1, n))).to(DEV)
    assert lapack.engine._cholupdate(Rt, big, n, 1, n, n, -1, lapack.ArgPack_cholupdate(cmaj, up)) == 8
