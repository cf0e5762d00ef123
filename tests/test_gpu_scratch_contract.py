"""-m gpu: the scratch contract and the decision paths of the entry points that keep tickets, flags and state words in caller-provided
scratch - cap_dcholupdate, cap_dpstrf, cap_dlansy, cap_dsymm_thin, cap_dpocon, cap_dpoerr - on the rows of tests/scratch_cases.py
(tests/test_scratch_cases.py checks their premises without a GPU).

a. THE CONTRACT.  The buffer is [pre-guard][work: exactly cap_*_work_size doubles][sentinel of 4096 doubles], guard and sentinel distinct
   NaNs; `work` is filled four ways (distinct NaNs; every 32-bit word 1; every byte 0xFF; zeros) and handed over at an even and at an odd
   offset (16- and 8-byte aligned).  After every call: status 0, guard and sentinel bit-identical, every input bit-identical, the pad rows
   and untouched triangles of the outputs bit-identical, no fallback counted - and EVERY OUTPUT BIT-IDENTICAL ACROSS THE EIGHT RUNS: a
   read of scratch the call never wrote, a counter block some path forgets to clear or a state word left unset changes bits (or counts
   a recovery launch) under at least one of the fills.  The NaN run also meets the row's expectation (scratch_cases.expected).
   The odd offset is RUN for all six entries: every access of theirs to the scratch is an 8-byte (or 4-byte) one - cholupdate.hip,
   symv.hip, pocon.hip and potrs.hip read and write single doubles and ints; pstrf.hip, whose dots load 16-byte pairs, rounds `work` up
   to a 16-byte boundary inside the size it asks for; the inverses of R's diagonal blocks (cap_dpocon / cap_dpoerr) are made by the
   window copy, the leaf inverse and the GEMM launcher, which test the alignment themselves and change only how they load.
b. LEFTOVERS.  One buffer, filled once, goes unrefreshed through a sequence of nine calls and through the reverse sequence: every call's
   outputs have the bits of the same call from (a).
c. THE PLAN ROUTES (cap_cholinv_update, cap_cholinv_rcond, cap_cholinv_error_bounds keep their scratch inside the plan, where it cannot
   be poisoned) give the bits of the caller-scratch entries on NaN-filled work, and their own scratch is reused across shapes.
d. DECISION PATHS.  cap_pocon_last_solves EQUALS the solve count of the NumPy model (tests/poerr_model.lacn2) run on the factor the GPU
   made; rcond within 1e-8 and every ferr within 1e-6 of the model, berr within (n + 2) eps of the long double quotient (the bounds of
   tests/test_gpu_pocon.py / test_gpu_poerr.py); a column's bounds do not depend on its company or its place in the chunk, and scaling
   by powers of two changes no bit.

No tolerance here is new, and every non-zero one compares with the NumPy model, never with another GPU result."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cholupdate_model as cm
from tests import poerr_model as pm
from tests import pstrf_model as psm
from tests import scratch_cases as sc
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

OK = 0
NAN = float("nan")
EPS = pm.EPS


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(flat):
    return torch.from_numpy(np.ascontiguousarray(flat)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _fallbacks():
    L = _L()
    return (L.cap_update_fallbacks(), L.cap_solve_fallbacks(), L.cap_chain_fallbacks())


class Scratch:
    """[pre-guard: PRE (+ 1 at the odd offset) doubles][work: exactly `size` doubles][sentinel: SENTINEL doubles]"""

    def __init__(self, size, kind="nan", odd=0):
        self.size, self.off = size, sc.PRE + odd
        host = sc.nan_pattern(sc.PRE + 1 + size + sc.SENTINEL, salt=7)
        host[self.off:self.off + size] = sc.fill(kind, size, salt=3)
        self.host = host
        self.buf = _dev(host)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + 8 * self.off

    def check(self, what):
        after, end = _host(self.buf), self.off + self.size
        assert sc.same_bits(after[:self.off], self.host[:self.off]), "%s: the guard in front of the work buffer changed" % what
        assert after[end:].size >= sc.SENTINEL and sc.same_bits(after[end:], self.host[end:]), \
            "%s: the sentinel behind the work buffer changed" % what


def _unchanged(t, flat, what):
    assert sc.same_bits(_host(t), flat), "%s was written" % what


def _pads_unchanged(after, before, what):
    """the NaN positions of `before` (pad rows, untouched triangles) hold the same bits in `after`"""
    m = np.isnan(before)
    assert sc.same_bits(after[m], before[m]), "%s: pad rows or an untouched triangle were written" % what


# ---- the factor the GPU makes (cap_dpotrf), once per matrix ----------------------------------------------------------------------------------
_FACTORS = {}


def _gpu_factor(key, A):
    """(the window of R with leading dimension n + 1, NaN pad rows and NaN strictly lower triangle, as a host array; R upper as n x n)"""
    if key not in _FACTORS:
        L = _L()
        n = A.shape[0]
        ld = n + 1
        buf = _dev(sc.window(A, ld))                                         # symmetric: column-major as well
        info = torch.zeros(1, dtype=torch.int32, device=DEV)
        w = Scratch(int(L.cap_dpotrf_work_size(n)))
        assert L.cap_dpotrf(1, n, buf.data_ptr(), ld, info.data_ptr(), w.ptr, _stream()) == OK
        assert int(_host(info)[0]) == 0
        R = np.triu(sc.unwindow(_host(buf), n, n, ld))
        R.setflags(write=False)
        _FACTORS[key] = (sc.window(R, ld, upper=True), R)
    return _FACTORS[key]


# ---- one call per entry: -> {output name: host array}, after the assertions on status, inputs and pads ------------------------------------------
def _run_update(row, wptr):
    L = _L()
    n, k = row.shape
    A, V, R, A1, ref = sc.update_operands(n, k)
    ldr, ldv = row.layout["R"], row.layout["V"]
    r0, v0 = sc.window(R, ldr, upper=True), sc.window(V, ldv)
    Rd, Vd = _dev(r0), _dev(v0)
    info = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    out = {}
    for sign, tag in ((+1, "up"), (-1, "down")):
        info[0] = 77
        assert L.cap_dcholupdate(1, sign, n, k, Rd.data_ptr(), ldr, Vd.data_ptr(), ldv, info.data_ptr(), wptr, _stream()) == OK
        out["R_" + tag], out["info_" + tag] = _host(Rd).copy(), _host(info).copy()
        assert out["info_" + tag][1] == 77
        _pads_unchanged(out["R_" + tag], r0, sc.row_id(row))
    _unchanged(Vd, v0, "V")
    return out


def _run_pstrf(row, wptr):
    L = _L()
    n, mr = row.shape
    A = sc.pstrf_operands(n, mr)[0]
    lda, ldr = row.layout["A"], row.layout["R"]
    a0, r0 = sc.window(A, lda, upper=True), sc.nan_pattern(n * ldr, salt=11)
    Ad, Rd = _dev(a0), _dev(r0)
    piv = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    rank = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    info = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    resid = _dev(np.array([-5.0, -5.0]))
    assert L.cap_dpstrf(1, n, mr, -1.0, Ad.data_ptr(), lda, Rd.data_ptr(), ldr, piv.data_ptr(), rank.data_ptr(), resid.data_ptr(),
                        info.data_ptr(), wptr, _stream()) == OK
    out = {"R": _host(Rd), "piv": _host(piv), "rank": _host(rank), "resid": _host(resid), "info": _host(info)}
    _unchanged(Ad, a0, "A")
    pad = np.zeros((n, ldr), dtype=bool); pad[:, mr:] = True
    assert sc.same_bits(out["R"][pad.reshape(-1)], r0[pad.reshape(-1)]), "pad rows of R were written"
    assert out["piv"][n] == -7 and out["rank"][1] == -7 and out["info"][1] == -7 and out["resid"][1] == -5.0
    return out


def _run_lansy(row, wptr):
    L = _L()
    n = row.shape[0]
    lda = row.layout["A"]
    a0 = sc.window(sc.sym_int(n, 23 * n), lda, upper=True)
    Ad = _dev(a0)
    out = _dev(np.array([-5.0, -5.0, -5.0]))
    assert L.cap_dlansy(ord('1'), 1, n, Ad.data_ptr(), lda, out.data_ptr() + 8, wptr, _stream()) == OK
    o = _host(out)
    assert o[0] == -5.0 and o[2] == -5.0
    _unchanged(Ad, a0, "A")
    return {"norm": o[1:2].copy()}


def _run_symm(row, wptr):
    L = _L()
    n, nrhs, ab = row.shape
    a, x, b, alpha, beta = sc.symm_operands(n, nrhs, ab)
    ld = row.layout
    a0, x0, b0 = sc.window(a, ld["A"], upper=True), sc.window(x, ld["X"]), sc.window(b, ld["B"])
    y0 = sc.nan_pattern(nrhs * ld["Y"], salt=13)
    Ad, Xd, Bd, Yd = _dev(a0), _dev(x0), _dev(b0), _dev(y0)
    assert L.cap_dsymm_thin(1, ab, n, nrhs, alpha, Ad.data_ptr(), ld["A"], Xd.data_ptr(), ld["X"], beta, Bd.data_ptr(), ld["B"],
                            Yd.data_ptr(), ld["Y"], wptr, _stream()) == OK
    y = _host(Yd)
    pad = np.zeros((nrhs, ld["Y"]), dtype=bool); pad[:, n:] = True
    assert sc.same_bits(y[pad.reshape(-1)], y0[pad.reshape(-1)]), "pad rows of Y were written"
    for t, f, name in ((Ad, a0, "A"), (Xd, x0, "X"), (Bd, b0, "B")):
        _unchanged(t, f, name)
    return {"Y": y}


def _pocon(key, A, wptr, p=0):
    """cap_dpocon on the GPU's factor of A, scaled: R 2^p, anorm 4^p -> (rcond as an array of one, the solves it took)"""
    L = _L()
    n = A.shape[0]
    r0, R = _gpu_factor(key, A)
    r0 = r0 * 2.0 ** p
    Rd = _dev(r0)
    an = _dev(np.array([np.abs(A).sum(0).max() * 4.0 ** p]))
    out = _dev(np.array([-5.0, -5.0, -5.0]))
    assert L.cap_dpocon(1, n, Rd.data_ptr(), n + 1, an.data_ptr(), out.data_ptr() + 8, wptr, _stream()) == OK
    o = _host(out)
    assert o[0] == -5.0 and o[2] == -5.0
    _unchanged(Rd, r0, "R")
    return o[1:2].copy(), int(L.cap_pocon_last_solves())


def _run_pocon(row, wptr):
    rcond, solves = _pocon(row.shape, sc.pocon_matrix(*row.shape), wptr)
    return {"rcond": rcond, "solves": np.array([solves])}


def _poerr(n, nrhs, cols, what, wptr, p=0):
    """cap_dpoerr on the columns `cols` of the (n, nrhs) operands, A and B scaled by 4^p, R by 2^p -> {"ferr", "berr", "solves"}"""
    L = _L()
    A, B, X = sc.poerr_operands(n, nrhs)
    cols = list(cols)
    row = sc.find("cap_dpoerr", n, nrhs, "both")
    ld = row.layout
    r0, R = _gpu_factor(("poerr", n), A)
    a0, r0 = sc.window(A, ld["A"], upper=True) * 4.0 ** p, r0 * 2.0 ** p
    b0, x0 = sc.window(B[:, cols], ld["B"]) * 4.0 ** p, sc.window(X[:, cols], ld["X"])
    Ad, Rd, Bd, Xd = _dev(a0), _dev(r0), _dev(b0), _dev(x0)
    m = len(cols)
    fe, be = _dev(np.full(m + 2, -5.0)), _dev(np.full(m + 2, -5.0))
    assert L.cap_dpoerr(1, n, m, Ad.data_ptr(), ld["A"], Rd.data_ptr(), ld["R"], Bd.data_ptr(), ld["B"], Xd.data_ptr(), ld["X"],
                        fe.data_ptr() + 8 if what != "berr" else None, be.data_ptr() + 8 if what != "ferr" else None, wptr, _stream()) == OK
    f, e = _host(fe), _host(be)
    for o, asked in ((f, what != "berr"), (e, what != "ferr")):
        assert o[0] == -5.0 and o[-1] == -5.0 and (asked or (o == -5.0).all())
    for t, flat, name in ((Ad, a0, "A"), (Rd, r0, "R"), (Bd, b0, "B"), (Xd, x0, "X")):
        _unchanged(t, flat, name)
    out = {"ferr": f[1:-1].copy(), "berr": e[1:-1].copy()}
    if what != "berr":
        out["solves"] = np.array([int(L.cap_pocon_last_solves())])
    return out


def _run_poerr(row, wptr):
    n, nrhs, what = row.shape
    return _poerr(n, nrhs, range(nrhs), what, wptr)


RUNNERS = {"cap_dcholupdate": _run_update, "cap_dpstrf": _run_pstrf, "cap_dlansy": _run_lansy, "cap_dsymm_thin": _run_symm,
           "cap_dpocon": _run_pocon, "cap_dpoerr": _run_poerr}


def _same_outputs(got, want, what):
    assert got.keys() == want.keys()
    for name in want:
        assert sc.same_bits(got[name], want[name]), "%s: %s differs (%d of %d elements)" % (
            what, name, int((np.ascontiguousarray(got[name]).view(np.uint8) != np.ascontiguousarray(want[name]).view(np.uint8)).sum()),
            got[name].size)


# ---- expectations of the NaN run ----------------------------------------------------------------------------------------------------------------
def _check_expectation(row, out):
    e = sc.expected(row)
    if row.entry == "cap_dcholupdate":
        n, k = row.shape
        ldr = row.layout["R"]
        R1, R2 = (np.triu(sc.unwindow(out["R_" + t], n, n, ldr)) for t in ("up", "down"))
        assert out["info_up"][0] == 0 and out["info_down"][0] == 0
        assert np.isfinite(R1).all() and np.isfinite(R2).all()
        scale = np.abs(e["ref"]).max()
        figs = (cm.element_error(R1, e["ref"]), np.abs(R1 - np.triu(e["model"])).max() / scale, cm.backward_error(R1, e["A1"]),
                cm.element_error(R2, e["R"]), cm.backward_error(R2, e["A"]))
        print("%s: update elementwise %.2e (cholesky) %.2e (model) backward %.2e | downdate elementwise %.2e backward %.2e"
              % ((sc.row_id(row),) + figs))
        assert figs[0] <= cm.ELEMENT_GATE and figs[1] <= cm.ELEMENT_GATE and figs[2] <= cm.BACKWARD_GATE
        assert figs[3] <= cm.ELEMENT_GATE and figs[4] <= cm.BACKWARD_GATE
    elif row.entry == "cap_dpstrf":
        n, mr = row.shape
        A = sc.pstrf_operands(n, mr)[0]
        Rm, pivm, rankm, residm, infom, _ = e
        R, piv, rank, info, resid = sc.unwindow(out["R"], mr, n, row.layout["R"]), out["piv"][:n], int(out["rank"][0]), int(out["info"][0]), \
            float(out["resid"][0])
        assert (rank, info) == (rankm, infom) and np.array_equal(piv, pivm), "pivots differ from the model's"
        ratio = psm.check_properties(A, R, piv, rank, info, psm.default_tol(A))
        mine = psm.remaining_diagonal(A, R, piv, rank).sum()
        print("%s: rank %d info %d, backward error %.3f of the bound, resid %.6e (own %.6e)" % (sc.row_id(row), rank, info, ratio, resid, mine))
        assert abs(resid - mine) <= 2 * psm.gamma(n) * np.trace(A)
    elif row.entry == "cap_dlansy":
        assert out["norm"][0] == e
    elif row.entry == "cap_dsymm_thin":
        n, nrhs, _ = row.shape
        assert np.array_equal(sc.unwindow(out["Y"], n, nrhs, row.layout["Y"]), e)
    else:
        assert e is None                    # the estimator rows: section d


# ---- a. the contract ------------------------------------------------------------------------------------------------------------------------------
_BASE = {}


def _base(row):
    """the outputs of the row on NaN scratch at the even offset (the run every other one is compared with), with its contract checked"""
    key = (row.entry, row.shape)
    if key not in _BASE:
        w = Scratch(sc.work_size(_L(), row))
        _BASE[key] = RUNNERS[row.entry](row, w.ptr)
        w.check(sc.row_id(row))
    return _BASE[key]


@pytest.mark.parametrize("row", sc.ROWS, ids=sc.row_id)
def test_scratch_contract(row):
    before = _fallbacks()
    assert min(before) >= 0
    base = _base(row)
    _check_expectation(row, base)
    size = sc.work_size(_L(), row)
    for kind in sc.FILLS:
        for odd in (0, 1):
            if (kind, odd) == ("nan", 0):
                continue
            w = Scratch(size, kind, odd)
            out = RUNNERS[row.entry](row, w.ptr)
            w.check("%s, fill %s, offset %d" % (sc.row_id(row), kind, odd))
            _same_outputs(out, base, "%s, fill %s, offset %d against the NaN fill at offset 0" % (sc.row_id(row), kind, odd))
    assert _fallbacks() == before, "a recovery launch ran"


# ---- b. leftovers of other calls --------------------------------------------------------------------------------------------------------------
SEQUENCE = [("cap_dcholupdate", 129, 9), ("cap_dpocon", "rand", 300), ("cap_dcholupdate", 65, 4), ("cap_dpoerr", 129, 17, "both"),
            ("cap_dpstrf", 130, 130), ("cap_dlansy", 1025), ("cap_dsymm_thin", 300, 17, 0), ("cap_dpocon", "rand", 129),
            ("cap_dcholupdate", 129, 9)]


def test_leftovers_of_other_calls():
    """one buffer as large as the largest row, filled once, never refreshed: each call finds what the calls in front of it left"""
    L = _L()
    rows = [sc.find(*s) for s in SEQUENCE]
    before = _fallbacks()
    w = Scratch(max(sc.work_size(L, r) for r in sc.ROWS))
    for order in (rows, rows[::-1]):
        for i, row in enumerate(order):
            out = RUNNERS[row.entry](row, w.ptr)
            _same_outputs(out, _base(row), "call %d of the sequence (%s) on the leftovers of the calls in front of it" % (i + 1, sc.row_id(row)))
            w.check(sc.row_id(row))
    assert _fallbacks() == before, "a recovery launch ran"


# ---- c. the plan routes -----------------------------------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, n, driver=None):
        self.n, self.h = n, C.c_void_p()
        assert _L().cap_cholinv_plan_create(C.byref(self.h), n, -1, 1, -2, b"U", None) == 0
        if driver is not None:
            assert _L().cap_cholinv_set_option(self.h, b"chud_kernel", driver) == 0

    def factor(self, a):
        A = _dev(np.array(a, order="C"))                                     # symmetric: column-major as well
        assert _L().cap_cholinv_factor(self.h, A.data_ptr(), self.n, _stream()) == 0
        torch.cuda.synchronize()

    def R(self):
        R = torch.empty(self.n * self.n, dtype=torch.float64, device=DEV)
        assert _L().cap_cholinv_get_R(self.h, R.data_ptr(), self.n, _stream()) == 0
        return _host(R).copy()                                               # column-major, ld n

    def R_ptr(self):
        ld = C.c_int64(0)
        return _L().cap_cholinv_R_ptr(self.h, C.byref(ld)), ld.value

    def info(self):
        v = C.c_int64(0)
        _L().cap_cholinv_info(self.h, _stream(), C.byref(v))
        return v.value

    def __del__(self):
        _L().cap_cholinv_plan_destroy(self.h)


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("n,k", [(129, 9), (129, 33), (300, 9), (300, 33)])
def test_plan_update_reads_the_bits_of_the_caller_scratch_entry(n, k, sign):
    L = _L()
    A, V = cm.spd(n, 10 + n), cm.thin(n, k, 100 + n)
    start = A if sign > 0 else A + V @ V.T                                   # the downdate starts from A' (A - V V^T need not be definite)
    v0 = sc.window(V, n + 5)
    before = _fallbacks()
    want = None
    for driver in (1, 0):
        p = Plan(n, driver)
        p.factor(start)
        r_plan = p.R()
        if want is None:                                                     # cap_dcholupdate on a copy of the plan's factor
            Rd, Vd = _dev(r_plan), _dev(v0)
            info = torch.full((1,), 77, dtype=torch.int32, device=DEV)
            w = Scratch(int(L.cap_dcholupdate_work_size(n, k)))
            assert L.cap_dcholupdate(1, sign, n, k, Rd.data_ptr(), n, Vd.data_ptr(), n + 5, info.data_ptr(), w.ptr, _stream()) == OK
            want, want_info = _host(Rd).copy(), int(_host(info)[0])
            w.check("cap_dcholupdate")
            assert want_info == 0
        Vd = _dev(v0)
        assert L.cap_cholinv_update(p.h, sign, Vd.data_ptr(), n + 5, k, _stream()) == OK
        got = p.R()
        assert p.info() == want_info
        up = np.triu(np.ones((n, n), dtype=bool)).T.reshape(-1)              # column-major: (col, row) with row <= col
        assert sc.same_bits(got[up], want[up]), "driver %d: the plan's update and cap_dcholupdate differ" % driver
    assert _fallbacks() == before


def _plan_case(n, nrhs):
    A, B, X = sc.poerr_operands(n, nrhs)
    row = sc.find("cap_dpoerr", n, nrhs, "both")
    p = Plan(n)
    p.factor(A)
    ld = row.layout
    dev = {"A": _dev(sc.window(A, ld["A"], upper=True)), "B": _dev(sc.window(B, ld["B"])), "X": _dev(sc.window(X, ld["X"]))}
    return p, ld, dev, A


def _plan_bounds(p, ld, dev, nrhs):
    fe, be = _dev(np.full(nrhs + 2, -5.0)), _dev(np.full(nrhs + 2, -5.0))
    assert _L().cap_cholinv_error_bounds(p.h, dev["A"].data_ptr(), ld["A"], dev["B"].data_ptr(), ld["B"], dev["X"].data_ptr(), ld["X"], nrhs,
                                         fe.data_ptr() + 8, be.data_ptr() + 8, _stream()) == OK
    f, e = _host(fe), _host(be)
    assert f[0] == f[-1] == e[0] == e[-1] == -5.0
    return f[1:-1].copy(), e[1:-1].copy()


def _plan_rcond(p, anorm):
    an, out = _dev(np.array([anorm])), _dev(np.array([-5.0, -5.0, -5.0]))
    assert _L().cap_cholinv_rcond(p.h, None, 0, an.data_ptr(), out.data_ptr() + 8, _stream()) == OK
    o = _host(out)
    assert o[0] == -5.0 and o[2] == -5.0
    return o[1:2].copy()


@pytest.mark.parametrize("n", [127, 128, 129, 300])
def test_plan_rcond_reads_the_bits_of_cap_dpocon(n):
    L = _L()
    A = sc.pocon_matrix("rand", n)
    anorm = np.abs(A).sum(0).max()
    p = Plan(n)
    p.factor(A)
    got = _plan_rcond(p, anorm)
    Rp, ldr = p.R_ptr()
    an, out = _dev(np.array([anorm])), _dev(np.array([-5.0, -5.0, -5.0]))
    for kind in ("nan", "ones32"):
        w = Scratch(int(L.cap_dpocon_work_size(n)), kind)
        assert L.cap_dpocon(1, n, Rp, ldr, an.data_ptr(), out.data_ptr() + 8, w.ptr, _stream()) == OK
        assert sc.same_bits(_host(out)[1:2], got), "cap_cholinv_rcond and cap_dpocon on the plan's factor differ (%s fill)" % kind
        w.check("cap_dpocon")
    assert got[0] > 0


@pytest.mark.parametrize("n,nrhs", [(300, 16), (129, 3), (129, 17)])
def test_plan_error_bounds_read_the_bits_of_cap_dpoerr(n, nrhs):
    L = _L()
    p, ld, dev, A = _plan_case(n, nrhs)
    f, e = _plan_bounds(p, ld, dev, nrhs)
    Rp, ldr = p.R_ptr()
    fe, be = _dev(np.full(nrhs, -5.0)), _dev(np.full(nrhs, -5.0))
    w = Scratch(int(L.cap_dpoerr_work_size(n, nrhs)))
    assert L.cap_dpoerr(1, n, nrhs, dev["A"].data_ptr(), ld["A"], Rp, ldr, dev["B"].data_ptr(), ld["B"], dev["X"].data_ptr(), ld["X"],
                        fe.data_ptr(), be.data_ptr(), w.ptr, _stream()) == OK
    assert sc.same_bits(_host(fe), f) and sc.same_bits(_host(be), e), "cap_cholinv_error_bounds and cap_dpoerr on the plan's factor differ"
    w.check("cap_dpoerr")
    assert (f > 0).all() and (e > 0).all()


def test_plan_scratch_is_reused_across_shapes():
    """error bounds for 17, 3 and 17 columns with rcond between them: the plan's scratch holds what the other shape left, the first and
    the last results are the same bits"""
    n = 129
    p, ld, dev, A = _plan_case(n, 17)
    anorm = np.abs(A).sum(0).max()
    f17, e17 = _plan_bounds(p, ld, dev, 17)
    rc = _plan_rcond(p, anorm)
    f3, e3 = _plan_bounds(p, ld, dev, 3)
    assert sc.same_bits(_plan_rcond(p, anorm), rc)
    again = _plan_bounds(p, ld, dev, 17)
    assert sc.same_bits(again[0], f17) and sc.same_bits(again[1], e17)
    assert sc.same_bits(f3, f17[:3]) and sc.same_bits(e3, e17[:3]), "the first three columns alone"
    assert sc.same_bits(_plan_bounds(p, ld, dev, 3)[0], f3)


# ---- d. decision paths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sc.POCON_ROWS, ids=sc.row_id)
def test_pocon_takes_the_models_path(row):
    """the solve count EQUALS the model's on the GPU's own factor; rcond within 1e-8 of the model (kappa <= 1e4: the bound of
    tests/test_gpu_pocon.py)"""
    A = sc.pocon_matrix(*row.shape)
    base = _base(row)
    R = _gpu_factor(row.shape, A)[1]
    est, solves, trace = sc.pocon_trace(R)
    want = pm.rcond(R, np.abs(A).sum(0).max())
    got = float(base["rcond"][0])
    print("%s: gpu %.17g model %.17g, gpu / model - 1 = %.2e, solves %d (model %d, stages %s)"
          % (sc.row_id(row), got, want, got / want - 1, int(base["solves"][0]), solves, [t[0] for t in trace]))
    assert int(base["solves"][0]) == solves
    assert abs(got - want) <= 1e-8 * want


def _model_bounds(n, nrhs):
    A, B, X = sc.poerr_operands(n, nrhs)
    R = _gpu_factor(("poerr", n), A)[1]
    traces = sc.poerr_traces(A, R, B, X)
    return pm.ferr(A, R, B, X), pm.berr(A, B, X, dtype=np.longdouble).astype(np.float64), [t[1] for t in traces]


POERR_SHAPES = sorted({r.shape[:2] for r in sc.POERR_ROWS})


@pytest.mark.parametrize("n,nrhs", POERR_SHAPES)
def test_poerr_takes_the_models_path_in_every_column(n, nrhs):
    """every column of every chunk: ferr within 1e-6 of the model, berr within (n + 2) eps of the long double quotient (the bounds of
    tests/test_gpu_poerr.py), and cap_pocon_last_solves equals the largest model count over the columns of the LAST chunk"""
    base = _base(sc.find("cap_dpoerr", n, nrhs, "both"))
    fm, bm, counts = _model_bounds(n, nrhs)
    last = counts[16 * ((nrhs - 1) // 16):]
    ratio = base["ferr"] / fm - 1
    print("n=%d nrhs=%d: worst ferr / model - 1 = %.2e, worst |berr - long double| = %.2f eps, solves %d (model, per column: %s)"
          % (n, nrhs, np.abs(ratio).max(), np.abs(base["berr"] - bm).max() / EPS, int(base["solves"][0]), counts))
    assert int(base["solves"][0]) == max(last)
    assert (np.abs(base["ferr"] - fm) <= 1e-6 * fm).all(), ratio
    assert (np.abs(base["berr"] - bm) <= (n + 2) * EPS).all()
    only_f, only_b = _base(sc.find("cap_dpoerr", n, nrhs, "ferr")), _base(sc.find("cap_dpoerr", n, nrhs, "berr"))
    assert sc.same_bits(only_f["ferr"], base["ferr"]) and sc.same_bits(only_b["berr"], base["berr"]), "a NULL output changed the other"


@pytest.mark.parametrize("n,nrhs", [s for s in POERR_SHAPES if s[1] > 1])
def test_a_columns_bounds_do_not_depend_on_its_company(n, nrhs):
    """Bit equality.  Every per-column order of summation is independent of the number of columns that travel with it and of its place:
    symm_thin_part_kernel<NR> carries one accumulator per column (pacc[r], acc[r], Qs[r S + row]) over the same tiles in the same order
    whatever NR is - NR only sets the stride of the X copies in LDS - symm_thin_reduce_kernel adds the parts of (row, column) in slot
    order, potrs_item<NR> likewise keeps acc[r] / sold[r] per column, and pocon_init / pocon_step work one workgroup per column.  A
    finished column sits through the solves of the slower ones (the model counts differ: tests/test_scratch_cases.py); it must not move."""
    L = _L()
    base = _base(sc.find("cap_dpoerr", n, nrhs, "both"))
    w = Scratch(int(L.cap_dpoerr_work_size(n, nrhs)))
    for c in range(nrhs):
        alone = _poerr(n, nrhs, [c], "both", w.ptr)
        assert sc.same_bits(alone["ferr"], base["ferr"][c:c + 1]) and sc.same_bits(alone["berr"], base["berr"][c:c + 1]), \
            "column %d alone differs from column %d in lock-step" % (c, c)
    perm = list(np.roll(np.arange(nrhs), 5))[::-1]
    moved = _poerr(n, nrhs, perm, "both", w.ptr)
    assert sc.same_bits(moved["ferr"], base["ferr"][perm]) and sc.same_bits(moved["berr"], base["berr"][perm]), "a column moved within the chunk"
    w.check("cap_dpoerr")


SCALES = (-100, -20, 20, 100)


@pytest.mark.parametrize("row", sc.POCON_ROWS, ids=sc.row_id)
def test_pocon_power_of_two_scaling_changes_no_bit(row):
    """A 4^p, R 2^p, anorm 4^p: a power of two commutes with every rounding while nothing overflows or underflows"""
    A = sc.pocon_matrix(*row.shape)
    base = _base(row)
    w = Scratch(sc.work_size(_L(), row))
    for p in SCALES:
        rcond, solves = _pocon(row.shape, A, w.ptr, p)
        assert sc.same_bits(rcond, base["rcond"]) and solves == int(base["solves"][0]), "p = %d" % p
    w.check(sc.row_id(row))


@pytest.mark.parametrize("n,nrhs", POERR_SHAPES)
def test_poerr_power_of_two_scaling_changes_no_bit(n, nrhs):
    """A 4^p, R 2^p, B 4^p, X unchanged: berr and ferr keep their bits (|A||X| + |B| stays far above the guard: checked on the host in
    tests/test_scratch_cases.py).  At p = -100 a finished column of the lock-step call is multiplied by about 4^100 kappa at every later
    solve and runs to Inf and NaN over the remaining ones: ordinary data of a column the algorithm ignores, which must disturb neither
    its own stored estimate nor its neighbours."""
    base = _base(sc.find("cap_dpoerr", n, nrhs, "both"))
    w = Scratch(int(_L().cap_dpoerr_work_size(n, nrhs)))
    before = _fallbacks()
    for p in SCALES:
        out = _poerr(n, nrhs, range(nrhs), "both", w.ptr, p)
        _same_outputs(out, base, "n = %d, nrhs = %d, p = %d" % (n, nrhs, p))
    w.check("cap_dpoerr")
    assert _fallbacks() == before
