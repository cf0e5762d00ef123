"""-m gpu: stream order of cap_dgemm_batched, cap_dgemm_vbatched_inner and cap_dgemm_vbatched_combine as ORDERED CALLS
(tests/stream_order.py): the caller's stream is a non-blocking stream of the test's own, the call is enqueued behind a device-side delay,
every buffer is poison until that stream's own copies deliver the contents, a snapshot and a poison fill follow the call, the host waits
for that stream only.  The premise - everything was enqueued before the delay ended - is asserted by the helper.  The plan is made
beforehand: cap_vbatch_plan_create may synchronise, the entries may not.

Exact: the operands are those of tests/gemm_batched_cases.py, so every output is held bit for bit to NumPy's, and every word outside the
outputs to what the buffer held before."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import gemm_batched_cases as GC  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402

SIZES = (5, 0, 70, 8, 17, 1, 16, 130, 0, 2, 7, 64, 8, 8, 3, 65)


@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


def _lib():
    from capital_amd import _lib
    return _lib.lib()


def _lay(mats, ld, stride, salt):
    """`batch` column-major matrices in a buffer of distinct NaNs -> (buffer, index arrays of every block)"""
    rows, cols = mats[0].shape
    buf = V.nan_pattern(stride * (len(mats) - 1) + ld * max(cols, 1) + 8, salt=salt)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    idx = [i * stride + r + c * ld for i in range(len(mats))]
    for i, M in enumerate(mats):
        buf[idx[i]] = M
    return buf, idx


@pytest.mark.parametrize("m,n,k,ta,tb", ((33, 17, 19, 1, 0), (130, 70, 17, 0, 1)))
def test_fixed_size_entry_in_stream_order(env, m, n, k, ta, tb):
    L = _lib()
    batch, alpha, beta = 5, -1.0, 0.5
    ops = [GC.operands(m, n, k, i) for i in range(batch)]
    sa, sb = (k, m) if ta else (m, k), (n, k) if tb else (k, n)
    lda, ldb, ldc = sa[0] + 1, sb[0] + 2, m + 3
    A, _ = _lay([o[0].T if ta else o[0] for o in ops], lda, lda * sa[1] + 3, 1)
    B, _ = _lay([o[1].T if tb else o[1] for o in ops], ldb, ldb * sb[1] + 1, 2)
    Cb, idx = _lay([o[2] for o in ops], ldc, ldc * n + 5, 3)
    job = SO.Job({"A": A, "B": B, "C": Cb}, lambda p, s: L.cap_dgemm_batched(ta, tb, m, n, k, alpha, p["A"], lda, lda * sa[1] + 3, p["B"], ldb,
                                                                           ldb * sb[1] + 1, beta, p["C"], ldc, ldc * n + 5, batch, s),
                 label="gemm_batched")
    with env.ordered(job, label="cap_dgemm_batched %d x %d x %d" % (m, n, k)) as j:
        assert j.ret == 0
        assert SO.same_bits(j.snap["A"], A) and SO.same_bits(j.snap["B"], B)
        keep = np.ones(Cb.shape, dtype=bool)
        for i, o in enumerate(ops):
            keep[idx[i]] = False
            assert SO.same_bits(j.snap["C"][idx[i]] + 0.0, GC.expected(o[0], o[1], o[2], alpha, beta)), "block %d" % i
        assert np.array_equal(j.snap["C"].view(np.int64)[keep], Cb.view(np.int64)[keep])


def _plan(L):
    arr = (C.c_int64 * len(SIZES))(*SIZES)
    plan = C.c_void_p()
    assert L.cap_vbatch_plan_create(len(SIZES), arr, None, None, C.byref(plan)) == 0      # beforehand
    return plan


def _stack(mats, cols, ld, salt):
    buf = V.nan_pattern(ld * max(cols, 1) + 8, salt=salt)
    at = 0
    for M in mats:
        for c in range(cols):
            buf[c * ld + at:c * ld + at + M.shape[0]] = M[:, c]
        at += M.shape[0]
    return buf


@pytest.mark.parametrize("m,n", ((3, 16), (64, 65)))
def test_inner_in_stream_order(env, m, n):
    L = _lib()
    plan = _plan(L)
    try:
        alpha, beta, rows = 2.0, -1.0, sum(SIZES)
        ops = [GC.operands(m, n, s, i) for i, s in enumerate(SIZES)]
        ldx, ldy, ldg = rows + 2, rows + 3, m + 1
        X, Y = _stack([o[0].T for o in ops], m, ldx, 1), _stack([o[1] for o in ops], n, ldy, 2)
        Gb, idx = _lay([o[2] for o in ops], ldg, ldg * n + 3, 3)
        job = SO.Job({"X": X, "Y": Y, "G": Gb}, lambda p, s: L.cap_dgemm_vbatched_inner(plan, m, n, alpha, p["X"], ldx, p["Y"], ldy, beta, p["G"], ldg,
                                                                                     ldg * n + 3, s), label="gemm_vbatched_inner")
        with env.ordered(job, label="cap_dgemm_vbatched_inner %d x %d" % (m, n)) as j:
            assert j.ret == 0
            assert SO.same_bits(j.snap["X"], X) and SO.same_bits(j.snap["Y"], Y)
            keep = np.ones(Gb.shape, dtype=bool)
            for i, o in enumerate(ops):
                keep[idx[i]] = False
                assert SO.same_bits(j.snap["G"][idx[i]] + 0.0, GC.expected(o[0], o[1], o[2], alpha, beta)), "block %d" % i
            assert np.array_equal(j.snap["G"].view(np.int64)[keep], Gb.view(np.int64)[keep])
    finally:
        L.cap_vbatch_plan_destroy(plan)


@pytest.mark.parametrize("nrhs,k", ((16, 4), (17, 40)))
def test_combine_in_stream_order(env, nrhs, k):
    L = _lib()
    plan = _plan(L)
    try:
        alpha, beta, rows = 0.5, 0.5, sum(SIZES)
        ops = [GC.operands(s, nrhs, k, i) for i, s in enumerate(SIZES)]
        ldv, ldc, ldz = rows + 2, rows + 3, k + 1
        Vb, Cb = _stack([o[0] for o in ops], k, ldv, 1), _stack([o[2] for o in ops], nrhs, ldc, 3)
        Z, _ = _lay([o[1] for o in ops], ldz, ldz * nrhs + 3, 2)
        job = SO.Job({"V": Vb, "Z": Z, "C": Cb}, lambda p, s: L.cap_dgemm_vbatched_combine(plan, nrhs, k, alpha, p["V"], ldv, p["Z"], ldz, ldz * nrhs + 3,
                                                                                        beta, p["C"], ldc, s), label="gemm_vbatched_combine")
        with env.ordered(job, label="cap_dgemm_vbatched_combine %d x %d" % (nrhs, k)) as j:
            assert j.ret == 0
            assert SO.same_bits(j.snap["V"], Vb) and SO.same_bits(j.snap["Z"], Z)
            want = _stack([GC.expected(o[0], o[1], o[2], alpha, beta) for o in ops], nrhs, ldc, 3)
            live = np.zeros(Cb.shape, dtype=bool)
            for c in range(nrhs):
                live[c * ldc:c * ldc + rows] = True
            assert SO.same_bits(j.snap["C"][live] + 0.0, want[live])
            assert np.array_equal(j.snap["C"].view(np.int64)[~live], Cb.view(np.int64)[~live])
    finally:
        L.cap_vbatch_plan_destroy(plan)
