"""-m gpu: stream order of the entries of csrc/symm_batched.hip as ORDERED CALLS (tests/stream_order.py): the caller's stream is a
non-blocking stream of the test's own, the call is enqueued behind a device-side delay, every buffer is poison until that stream's own
copies deliver the contents, a snapshot and a poison fill follow the call, the host waits for that stream only.  The premise - everything
was enqueued before the delay ended - is asserted by the helper.  Plans are made beforehand: cap_vbatch_plan_create may synchronise, the
entries may not.

cap_dsymm_batched / _vbatched and cap_dlansy_batched / _vbatched: exact rows (integer operands of tests/symm_batched_cases.py, any
summation order gives these bits), against NumPy.  cap_dpocon_* and cap_dpoerr_* (several launches each, the library's own potri in the
middle, a work buffer): bit for bit against the same call in a plain synchronous run on the NULL stream."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import potri_batched_cases as P  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import symm_batched_cases as SC  # noqa: E402
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
def L():
    from capital_amd import _lib
    return _lib.lib()


def blocks_flat(mats, tri):
    """column-major blocks back to back, NaN in the strictly lower triangles with tri"""
    out = []
    for m in mats:
        m = np.array(m, dtype=np.float64)
        if tri:
            m[np.tril_indices(m.shape[0], -1)] = np.nan
        out.append(m.T.reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize("n,batch", ((8, 65), (33, 5), (64, 3), (130, 5), (256, 2)))
def test_exact_rows_in_stream_order(env, L, n, batch):
    ops = [SC.operands(n, NRHS, i % 7) for i in range(batch)]
    assert all(SC.premise(o[0], o[1], o[2], 2.0, -0.5) < SC.LIMIT for o in ops)
    bufs = {"A": blocks_flat([o[0] for o in ops], True), "X": blocks_flat([o[1] for o in ops], False), "B": blocks_flat([o[2] for o in ops], False),
            "Y": np.full(batch * n * NRHS, np.nan), "norm": np.full(batch, np.nan)}

    def enqueue(p, s):
        a = L.cap_dsymm_batched(UPPER, 0, n, NRHS, 2.0, p["A"], n, n * n, p["X"], n, n * NRHS, -0.5, p["B"], n, n * NRHS, p["Y"], n, n * NRHS, batch, s)
        b = L.cap_dsymm_batched(UPPER, 1, n, NRHS, 1.0, p["A"], n, n * n, p["X"], n, n * NRHS, 1.0, p["B"], n, n * NRHS, p["B"], n, n * NRHS, batch, s)
        c = L.cap_dlansy_batched(ord('1'), UPPER, n, p["A"], n, n * n, batch, p["norm"], s)
        return a, b, c
    with env.ordered(SO.Job(bufs, enqueue, label="symm_batched"), label="cap_dsymm_batched n %d" % n) as j:
        assert j.ret == (0, 0, 0)
        Y = j.snap["Y"].reshape(batch, NRHS, n)
        Bn = j.snap["B"].reshape(batch, NRHS, n)
        for i, (A, X, B) in enumerate(ops):
            assert SO.same_bits(positive_zero(Y[i].T), positive_zero(SC.expected(A, X, B, 2.0, -0.5, 0))), "block %d" % i
            assert SO.same_bits(Bn[i].T, SC.expected(A, X, B, 1.0, 1.0, 1)), "block %d in place" % i
            assert j.snap["norm"][i] == SC.norm1(A)
        assert SO.same_bits(j.snap["A"], bufs["A"]) and SO.same_bits(j.snap["X"], bufs["X"])


@pytest.fixture(scope="module")
def plan(L):
    lay = V.Layout(V.EVERY, "gaps")
    arr = lambda a: None if a is None else (C.c_int64 * len(a))(*[int(x) for x in a])
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(lay.batch, arr(lay.sizes), arr(lay.ld_arg), arr(lay.off_arg), C.byref(p)) == 0
    yield lay, p
    L.cap_vbatch_plan_destroy(p)


def stacked(lay, mats, ld):
    buf = V.nan_pattern(ld * NRHS + 8, salt=3)
    for i, m in enumerate(mats):
        if lay.sizes[i]:
            for k in range(NRHS):
                at = k * ld + int(lay.row_off[i])
                buf[at:at + int(lay.sizes[i])] = m[:, k]
    return buf


def test_plan_exact_rows_in_stream_order(env, L, plan):
    lay, p = plan
    ops = [None if not n else SC.operands(int(n), NRHS, i % 3) for i, n in enumerate(lay.sizes)]
    ld = lay.rows + 2
    bufs = {"A": lay.buffer([None if o is None else o[0] for o in ops]), "X": stacked(lay, [None if o is None else o[1] for o in ops], ld),
            "B": stacked(lay, [None if o is None else o[2] for o in ops], ld), "Y": V.nan_pattern(ld * NRHS + 8, salt=4),
            "norm": np.full(lay.batch, -7.5)}

    def enqueue(q, s):
        return (L.cap_dsymm_vbatched(p, UPPER, 0, NRHS, -1.0, q["A"], q["X"], ld, 1.0, q["B"], ld, q["Y"], ld, s),
                L.cap_dlansy_vbatched(p, ord('I'), UPPER, q["A"], q["norm"], s))
    with env.ordered(SO.Job(bufs, enqueue, label="symm_vbatched"), label="cap_dsymm_vbatched EVERY") as j:
        assert j.ret == (0, 0)
        for i, o in enumerate(ops):
            if o is None:
                assert j.snap["norm"][i] == -7.5
                continue
            n, r0 = int(lay.sizes[i]), int(lay.row_off[i])
            got = np.array([j.snap["Y"][k * ld + r0:k * ld + r0 + n] for k in range(NRHS)]).T
            assert SO.same_bits(positive_zero(got), positive_zero(SC.expected(o[0], o[1], o[2], -1.0, 1.0, 0))), "block %d" % i
            assert j.snap["norm"][i] == SC.norm1(o[0])
        pad = np.ones(bufs["Y"].shape, dtype=bool)
        for k in range(NRHS):
            pad[k * ld:k * ld + lay.rows] = False
        assert np.array_equal(j.snap["Y"].view(np.int64)[pad], bufs["Y"].view(np.int64)[pad])
        assert SO.same_bits(j.snap["A"], bufs["A"]) and SO.same_bits(j.snap["B"], bufs["B"])


def spd_case(n, batch):
    rng = np.random.default_rng([313, n])
    As = [P.random_spd(n, 1e2, 1, seed=i)[0] for i in range(batch)]
    Rs = [np.linalg.cholesky(A).T for A in As]
    Xs = [rng.standard_normal((n, NRHS)) for _ in range(batch)]
    Bs = [A @ x * (1 + 1e-12 * rng.standard_normal((n, NRHS))) for A, x in zip(As, Xs)]
    return As, Rs, Xs, Bs


@pytest.mark.parametrize("n,batch", ((8, 65), (64, 3), (130, 5)))
def test_rcond_and_error_bounds_in_stream_order(env, L, n, batch):
    As, Rs, Xs, Bs = spd_case(n, batch)
    info = np.zeros(batch, dtype=np.int32)
    info[batch // 2] = 1
    bufs = {"A": blocks_flat(As, True), "R": blocks_flat(Rs, True), "X": blocks_flat(Xs, False), "B": blocks_flat(Bs, False), "info": info,
            "anorm": np.array([SC.norm1(A) for A in As]), "rcond": np.full(batch, np.nan), "ferr": np.full(batch * NRHS, np.nan),
            "berr": np.full(batch * NRHS, np.nan), "work": np.full(int(L.cap_dpoerr_batched_work_size(n, NRHS, batch)), np.nan)}
    assert L.cap_dpocon_batched_work_size(n, batch) <= bufs["work"].size

    def enqueue(p, s):
        return (L.cap_dpocon_batched(UPPER, n, p["R"], n, n * n, batch, p["anorm"], p["info"], p["rcond"], p["work"], s),
                L.cap_dpoerr_batched(UPPER, n, NRHS, p["A"], n, n * n, p["R"], n, n * n, p["B"], n, n * NRHS, p["X"], n, n * NRHS, batch, p["info"],
                                     p["ferr"], p["berr"], NRHS, p["work"], s))
    job = SO.Job(bufs, enqueue, scratch=("work",), label="pocon_poerr_batched")
    want, ret = env.plain(job)
    assert ret == (0, 0)
    ok = info == 0
    assert np.isfinite(want["rcond"][ok]).all() and np.isnan(want["rcond"][~ok]).all()
    assert np.isfinite(want["ferr"].reshape(batch, NRHS)[ok]).all() and np.isnan(want["berr"].reshape(batch, NRHS)[~ok]).all()
    with env.ordered(job, label="cap_dpocon_batched + cap_dpoerr_batched n %d" % n) as j:
        assert j.ret == (0, 0)
        for name in ("rcond", "ferr", "berr", "A", "R", "X", "B", "info", "anorm"):
            assert SO.same_bits(j.snap[name], want[name]), name


def test_plan_rcond_and_error_bounds_in_stream_order(env, L, plan):
    lay, p = plan
    cases = [None if not n else spd_case(int(n), 1) for n in lay.sizes]
    pick = lambda k: [None if c is None else c[k][0] for c in cases]
    ld = lay.rows + 2
    lde = NRHS + 1
    bufs = {"A": lay.buffer(pick(0)), "R": lay.buffer(pick(1)), "X": stacked(lay, pick(2), ld), "B": stacked(lay, pick(3), ld),
            "info": np.zeros(lay.batch, dtype=np.int32), "anorm": np.array([1.0 if c is None else SC.norm1(c[0][0]) for c in cases]),
            "rcond": np.full(lay.batch, -7.5), "ferr": np.full(lay.batch * lde, -7.5), "berr": np.full(lay.batch * lde, -7.5),
            "work": np.full(int(L.cap_dpoerr_vbatched_work_size(p, NRHS)), np.nan)}
    assert L.cap_dpocon_vbatched_work_size(p) == lay.total <= bufs["work"].size

    def enqueue(q, s):
        return (L.cap_dpocon_vbatched(p, UPPER, q["R"], q["anorm"], q["info"], q["rcond"], q["work"], s),
                L.cap_dpoerr_vbatched(p, UPPER, NRHS, q["A"], q["R"], q["B"], ld, q["X"], ld, q["info"], q["ferr"], q["berr"], lde, q["work"], s))
    job = SO.Job(bufs, enqueue, scratch=("work",), label="pocon_poerr_vbatched")
    want, ret = env.plain(job)
    assert ret == (0, 0)
    live = np.asarray(lay.sizes) > 0
    assert np.all(want["rcond"][live] > 0) and np.all(want["rcond"][~live] == -7.5)
    fe = want["ferr"].reshape(lay.batch, lde)
    assert np.all(fe[live, :NRHS] > 0) and np.all(fe[~live] == -7.5) and np.all(fe[:, NRHS] == -7.5)
    with env.ordered(job, label="cap_dpocon_vbatched + cap_dpoerr_vbatched EVERY") as j:
        assert j.ret == (0, 0)
        for name in ("rcond", "ferr", "berr", "A", "R", "X", "B", "info", "anorm"):
            assert SO.same_bits(j.snap[name], want[name]), name
