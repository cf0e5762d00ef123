"""-m gpu: the triangular inverse and solve paths - cap_dtrtri, cap_dtrsm, cap_dpotrs (one launch per substitution and the blocked
route) and cap_dpotri - against EXACT results.

The rows of tests/tri_cases.py (tests/test_tri_cases.py shows, without a GPU, what each of them launches and that the premise of
exactness holds for it) through the C ABI.  The operands have power-of-two diagonals and small integer off-diagonals, so every value
these routes form is a dyadic rational far below 2^53 and a float64 NumPy product of the closed-form inverse IS the result, whatever the
summation order: "the substitution picked up a part of S_i one ticket early" or "one element on the edge of a ragged block" changes a
dyadic rational, it cannot hide in rounding.  Everything a call must not write holds NaNs - the pad rows, the strictly lower triangle of
T (also of the TRTRI / POTRI window, which is the output), and `work`, which is all NaN, exactly cap_*_work_size doubles long, with a
4096-double NaN sentinel behind it: a read of scratch the call never wrote shows as NaN in the result, a write past the scratch in the
sentinel.  Whole buffers are compared as int64 after mapping -0.0 to +0.0 in the output (an alpha = -1 product of exact zeros is
legitimately -0.0); the read-only operands are compared as they are.  There is no tolerance in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import tri_cases as T  # noqa: E402
from tests.blas3_cases import describe_mismatch, place, same_bits  # noqa: E402
from tests.gpu_util import DEV  # noqa: E402

SENTINEL = 4096


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_buffer(size):
    return torch.from_numpy(np.full(size, T.NAN)).to(DEV)


def _check_sentinel(work, used, what):
    tail = work[used:].cpu().numpy()
    assert tail.size == SENTINEL and same_bits(tail, np.full(SENTINEL, T.NAN)), "%s: the sentinel behind the work buffer changed" % what


def _run_exact(c, ops=None, inject=False):
    """one row through the C ABI; -> the output buffer as the device left it (after every assertion of this file held)"""
    L = _L()
    ops = ops or T.operands(c)
    ld = T.lds(c)
    host = {"T": place(T.stored(ops["T"]), ld["T"])}
    if "B" in ops:
        host["B"] = place(ops["B"], ld["B"])
    dev = {name: torch.from_numpy(flat).to(DEV) for name, flat in host.items()}
    ws = T.work_size(L, c)
    work = _nan_buffer(c.woff + ws + SENTINEL)
    if inject:                                      # the existing test hook: the next substitution goes through the normal give-up path
        assert L.cap_solve_inject_timeouts(1) == 0
    st = T.call(L, c, dev["T"].data_ptr(), dev["B"].data_ptr() if "B" in dev else None, work.data_ptr() + 8 * c.woff, ld, _stream())
    assert st == 0, (c.id, st)
    out = "T" if c.op in ("trtri", "potri") else "B"
    want = dict(host)
    want[out] = place(T.reference(c, ops), ld[out])
    got = {name: buf.cpu().numpy() for name, buf in dev.items()}
    for name in host:
        g, w = (T.positive_zero(got[name]), T.positive_zero(want[name])) if name == out else (got[name], want[name])
        assert same_bits(g, w), "%s, %s: %s" % (c.id, name, describe_mismatch(g, w, ld[name]))
    _check_sentinel(work, c.woff + ws, c.id)
    return got[out]


@pytest.mark.parametrize("case", T.TRTRI_CASES, ids=lambda c: c.id)
def test_trtri_exact(case):
    _run_exact(case)


@pytest.mark.parametrize("case", T.TRSM_CASES, ids=lambda c: c.id)
def test_trsm_exact(case):
    _run_exact(case)


@pytest.mark.parametrize("case", T.POTRS_CASES, ids=lambda c: c.id)
def test_potrs_exact(case):
    _run_exact(case)


@pytest.mark.parametrize("case", T.POTRI_CASES, ids=lambda c: c.id)
def test_potri_exact(case):
    _run_exact(case)


def test_potrs_recovery_launch_gives_the_same_exact_result():
    """the give-up path (cap_solve_inject_timeouts: the workgroups of the next substitution leave at its first ticket) hands the whole
    substitution to the recovery launch, which runs the items in ticket order by itself: the same exact result, one fallback counted"""
    L = _L()
    c = T.RECOVERY_CASE
    assert (c.n, c.other) == (1153, 5)
    before = L.cap_solve_fallbacks()
    _run_exact(c, inject=True)
    assert L.cap_solve_fallbacks() == before + 1
    _run_exact(c)                                   # the hook was used up
    assert L.cap_solve_fallbacks() == before + 1


def test_potrs_one_launch_and_blocked_routes_agree():
    """the same columns padded to 17 right-hand sides take the blocked route: both are exact, so the first columns are equal"""
    c = T.AGREEMENT_CASE
    ops = T.operands(c)
    ld = T.lds(c)["B"]
    one = _run_exact(c, ops).reshape(c.other, ld)[:, :c.n]
    wide = T.Case(c, other=17)
    extra = T.RHS_VALUES[np.random.default_rng(5).integers(0, len(T.RHS_VALUES), size=(c.n, 17 - c.other))]
    blocked = _run_exact(wide, dict(ops, B=np.hstack([ops["B"], extra]))).reshape(17, ld)[:, :c.n]
    assert same_bits(T.positive_zero(blocked[:c.other]), T.positive_zero(one))


@pytest.mark.parametrize("entry,what,want", T.REFUSALS, ids=["%s-%s" % r[:2] for r in T.REFUSALS])
def test_refusals_touch_nothing(entry, what, want):
    """uplo = LOWER, negative sizes, a leading dimension below the extent and NULL operands return the documented status; nothing is written"""
    n, ld = T.REFUSAL_N, T.REFUSAL_N + 2
    sizes = (ld * n, ld * n, 1 << 16)
    a, b, work = (_nan_buffer(s) for s in sizes)
    assert T.refusal_call(_L(), entry, what, a.data_ptr(), b.data_ptr(), work.data_ptr(), _stream()) == want
    torch.cuda.synchronize()
    for buf, size in zip((a, b, work), sizes):
        assert same_bits(buf.cpu().numpy(), np.full(size, T.NAN)), (entry, what)
