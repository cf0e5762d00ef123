"""-m gpu: stream order of cap_dpstrf_batched and cap_dpstrf_vbatched as ORDERED CALLS (tests/stream_order.py): the caller's stream is a
non-blocking stream of the test's own, the call is enqueued behind a device-side delay, every buffer is poison until that stream's own
copies deliver the contents, a snapshot and a poison fill follow the call, the host waits for that stream only.  The premise - everything
was enqueued before the delay ended - is asserted by the helper.  The plan is made beforehand: cap_vbatch_plan_create may synchronise, the
two entries may not.

Exact: the blocks are the exact families of tests/pstrf_batched_cases.py at sizes where their answer is known from their construction,
so R, piv, rank, resid and info are held bit for bit to it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import pstrf_batched_cases as PC  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402

UPPER = 1
SIZES = (5, 0, 12, 8, 17, 1, 16, 9, 0, 2, 7, 13, 8, 8, 3, 17, 4, 6, 10, 11, 15, 14, 12, 9)


@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


def _lib():
    from capital_amd import _lib
    return _lib.lib()


def _outputs(batch, npiv):
    return {"piv": np.full(npiv, -7, dtype=np.int64), "rank": np.full(batch, -7, dtype=np.int32), "info": np.full(batch, -7, dtype=np.int32),
            "resid": np.full(batch, 123.5), "logdet": np.full(batch, 123.5)}


def test_fixed_size_entry_in_stream_order(env):
    L = _lib()
    n, batch, mr = 12, 21, 7
    lda, ldr = n + 1, mr + 2
    sa, sr = lda * n + 3, ldr * n + 5
    A = V.nan_pattern(sa * batch, salt=1)
    r, c = np.triu_indices(n)
    for i in range(batch):
        A[i * sa + r + c * lda] = PC.exact_matrix(n, PC.FAMILY[i % 4])[r, c]
    R = V.nan_pattern(sr * batch, salt=2)
    bufs = dict(_outputs(batch, batch * n), A=A, R=R)
    job = SO.Job(bufs, lambda p, s: L.cap_dpstrf_batched(UPPER, n, mr, -1.0, p["A"], lda, sa, p["R"], ldr, sr, p["piv"], p["rank"], p["resid"],
                                                         p["logdet"], p["info"], batch, s), label="pstrf_batched")
    with env.ordered(job, label="cap_dpstrf_batched n 12 batch 21") as j:
        assert j.ret == 0
        assert SO.same_bits(j.snap["A"], A)
        rr, cc = np.meshgrid(np.arange(mr), np.arange(n), indexing="ij")
        written = np.zeros(R.shape, dtype=bool)
        for i in range(batch):
            Rw, piv, rank, resid, info = PC.known_answer(n, PC.FAMILY[i % 4], mr)
            idx = i * sr + rr + cc * ldr
            written[idx] = True
            assert PC.same(j.snap["R"][idx], Rw), "block %d" % i
            assert np.array_equal(j.snap["piv"][i * n:(i + 1) * n], piv)
            assert (j.snap["rank"][i], j.snap["info"][i], j.snap["resid"][i]) == (rank, info, resid) and np.isfinite(j.snap["logdet"][i])
        assert np.array_equal(j.snap["R"].view(np.int64)[~written], R.view(np.int64)[~written])


def test_plan_entry_in_stream_order(env):
    L = _lib()
    lay = V.Layout(SIZES, "gaps")
    arr = lambda a: None if a is None else (C.c_int64 * len(a))(*[int(x) for x in a])
    plan = C.c_void_p()
    assert L.cap_vbatch_plan_create(lay.batch, arr(lay.sizes), arr(lay.ld_arg), arr(lay.off_arg), C.byref(plan)) == 0      # beforehand
    try:
        which = [PC.FAMILY[i % 4] for i in range(lay.batch)]
        A = lay.buffer([PC.exact_matrix(int(n), w) if n else None for n, w in zip(lay.sizes, which)])
        R = V.nan_pattern(lay.total + V.GUARD, salt=2)
        bufs = dict(_outputs(lay.batch, lay.rows), A=A, R=R)
        mr = 6
        job = SO.Job(bufs, lambda p, s: L.cap_dpstrf_vbatched(plan, UPPER, mr, -1.0, p["A"], p["R"], p["piv"], p["rank"], p["resid"], p["logdet"],
                                                              p["info"], s), label="pstrf_vbatched")
        with env.ordered(job, label="cap_dpstrf_vbatched %d blocks" % lay.batch) as j:
            assert j.ret == 0
            assert SO.same_bits(j.snap["A"], A)
            for i in range(lay.batch):
                n = int(lay.sizes[i])
                if n == 0:
                    assert j.snap["rank"][i] == -7 and j.snap["info"][i] == -7 and j.snap["resid"][i] == 123.5 and j.snap["logdet"][i] == 123.5
                    continue
                cap = min(mr, n)
                Rw, piv, rank, resid, info = PC.known_answer(n, which[i], cap)
                got = lay.block(j.snap["R"], i)
                assert PC.same(got[:cap], Rw) and PC.same(got[cap:], np.zeros((n - cap, n))), "block %d" % i
                ro = int(lay.row_off[i])
                assert np.array_equal(j.snap["piv"][ro:ro + n], piv)
                assert (j.snap["rank"][i], j.snap["info"][i], j.snap["resid"][i]) == (rank, info, resid) and np.isfinite(j.snap["logdet"][i])
            keep = ~lay.written("window")
            assert np.array_equal(j.snap["R"].view(np.int64)[keep], R.view(np.int64)[keep])
    finally:
        L.cap_vbatch_plan_destroy(plan)
