"""-m gpu: stream order of cap_dpotrf_vbatched, cap_dpotrs_vbatched and cap_dpotri_vbatched as ORDERED CALLS (tests/stream_order.py): the
caller's stream is a non-blocking stream of the test's own, the call is enqueued behind a device-side delay, every buffer is poison until
that stream's own copies deliver the contents, a snapshot and a poison fill follow the call, the host waits for that stream only.  The
premise - everything was enqueued before the delay ended - is asserted by the helper.  The plan is made beforehand: cap_vbatch_plan_create
may synchronise, the three entries may not.

Exact: the operands are the tables of tests/test_gpu_vbatched.py's first test (family F1 on the list EVERY, with gaps), so the factor must be
T_i and the inverse triu(T_i^-1 T_i^-T) bit for bit; the solve is held against the same call in a plain synchronous run (bits)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import stream_order as SO  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402
from tests.tri_cases import positive_zero  # noqa: E402

UPPER = 1
NRHS = 17


@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def case():
    from capital_amd import _lib
    L = _lib.lib()
    lay = V.Layout(V.EVERY, "gaps")
    arr = lambda a: None if a is None else (C.c_int64 * len(a))(*[int(x) for x in a])
    plan = C.c_void_p()
    assert L.cap_vbatch_plan_create(lay.batch, arr(lay.sizes), arr(lay.ld_arg), arr(lay.off_arg), C.byref(plan)) == 0
    blocks = V.exact_blocks("F1", V.EVERY)
    yield L, lay, plan, blocks
    L.cap_vbatch_plan_destroy(plan)


def exact(a):
    return positive_zero(a).view(np.int64)


def live(lay):
    return [i for i in range(lay.batch) if lay.sizes[i]]


def rest_untouched(before, after, lay, which):
    keep = ~lay.written(which)
    assert np.array_equal(before.view(np.int64)[keep], after.view(np.int64)[keep])


def test_factor_in_stream_order(env, case):
    L, lay, plan, blocks = case
    A = lay.buffer([None if b is None else b[0].T @ b[0] for b in blocks])
    bufs = {"A": A, "info": np.full(lay.batch, -7, dtype=np.int32), "logdet": np.full(lay.batch, 123.5)}
    job = SO.Job(bufs, lambda p, s: L.cap_dpotrf_vbatched(plan, UPPER, p["A"], p["info"], p["logdet"], s), label="potrf_vbatched")
    with env.ordered(job, label="cap_dpotrf_vbatched EVERY") as j:
        assert j.ret == 0
        for i in live(lay):
            iu = np.triu_indices(int(lay.sizes[i]))
            assert np.array_equal(exact(j.snap["A"][lay.index(i, "upper")[0]]), exact(blocks[i][0][iu])), "block %d" % i
            assert j.snap["info"][i] == 0 and np.isfinite(j.snap["logdet"][i])
        assert all(j.snap["info"][i] == -7 and j.snap["logdet"][i] == 123.5 for i in range(lay.batch) if not lay.sizes[i])
        rest_untouched(A, j.snap["A"], lay, "upper")


def test_solve_in_stream_order(env, case):
    L, lay, plan, blocks = case
    R = lay.buffer([None if b is None else b[0] for b in blocks])
    ldb = lay.rows + 2
    B = V.nan_pattern(ldb * NRHS + 8, salt=3)
    rhs = np.random.default_rng(17).integers(-8, 9, size=(lay.rows, NRHS)).astype(np.float64)
    for k in range(NRHS):
        B[k * ldb:k * ldb + lay.rows] = rhs[:, k]
    bufs = {"R": R, "B": B, "info": np.zeros(lay.batch, dtype=np.int32)}
    job = SO.Job(bufs, lambda p, s: L.cap_dpotrs_vbatched(plan, UPPER, NRHS, p["R"], p["B"], ldb, p["info"], s), label="potrs_vbatched")
    want, ret = env.plain(job)
    assert ret == 0 and not np.isnan(want["B"][:lay.rows]).any()
    with env.ordered(job, label="cap_dpotrs_vbatched EVERY nrhs 17") as j:
        assert j.ret == 0
        assert SO.same_bits(j.snap["B"], want["B"]) and SO.same_bits(j.snap["R"], R) and SO.same_bits(j.snap["info"], bufs["info"])
        # (the plain run itself: A_i X_i = B_i to the last bit is not claimed; the solutions are finite and the padding rows untouched)
        pad = np.ones(B.shape, dtype=bool)
        for k in range(NRHS):
            pad[k * ldb:k * ldb + lay.rows] = False
        assert np.array_equal(j.snap["B"].view(np.int64)[pad], B.view(np.int64)[pad])


@pytest.mark.parametrize("fill", (0, 1))
def test_inverse_in_stream_order(env, case, fill):
    L, lay, plan, blocks = case
    R = lay.buffer([None if b is None else b[0] for b in blocks])
    bufs = {"R": R, "info": np.zeros(lay.batch, dtype=np.int32)}
    job = SO.Job(bufs, lambda p, s: L.cap_dpotri_vbatched(plan, UPPER, p["R"], p["info"], fill, s), label="potri_vbatched")
    with env.ordered(job, label="cap_dpotri_vbatched EVERY fill %d" % fill) as j:
        assert j.ret == 0
        for i in live(lay):
            n = int(lay.sizes[i])
            iu, il = np.triu_indices(n), np.tril_indices(n, -1)
            got = lay.block(j.snap["R"], i)
            assert np.array_equal(exact(got[iu]), exact(blocks[i][2][iu])), "block %d" % i
            if fill:
                assert np.array_equal(got[il].view(np.int64), got.T[il].view(np.int64))
        rest_untouched(R, j.snap["R"], lay, "window" if fill else "upper")
