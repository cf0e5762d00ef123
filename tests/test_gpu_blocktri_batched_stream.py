"""-m gpu: stream order of cap_dpotrf_blocktri_batched and cap_dpotrs_blocktri_batched as ORDERED CALLS (tests/stream_order.py): the
caller's stream is a non-blocking stream of the test's own, the calls are enqueued behind a device-side delay, every buffer is poison
until that stream's own copies deliver the contents, a snapshot and a poison fill follow the calls, the host waits for that stream only.
The premise - everything was enqueued before the delay ended - is asserted by the helper.

Exact: the chains are those of tests/blocktri_cases.py's exact family, so the factor is held to R and the solution to X with no
tolerance, and every word outside the blocks to what the buffer held before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import blocktri_cases as BC  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402

ROWS = [r for r in BC.exact_rows() if r[1] in (1, 3, 257) or r[3] > 64]
UPPER = 1


@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


def _lib():
    from capital_amd import _lib
    return _lib.lib()


def _lay(mats, ld, step, stride, salt, upper=False):
    """mats[chain][position] column-major in a buffer of distinct NaNs -> (buffer, flat index of every element laid in, in order)"""
    batch, blocks = len(mats), len(mats[0])
    rows, cols = mats[0][0].shape if blocks else (1, 1)
    buf = V.nan_pattern(stride * (batch - 1) + step * max(blocks - 1, 0) + ld * cols + 8, salt=salt)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    keep = (r <= c) if upper else (r >= 0)
    idx = np.array([[ch * stride + i * step + r[keep] + c[keep] * ld for i in range(blocks)] for ch in range(batch)], dtype=np.int64).reshape(batch, blocks, -1)
    for ch in range(batch):
        for i in range(blocks):
            buf[idx[ch, i]] = np.asarray(mats[ch][i], dtype=np.float64)[keep]
    return buf, idx, keep


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "n%d-T%d-b%d-k%d-%s" % r)
def test_factor_then_solve_in_stream_order(env, row):
    L = _lib()
    n, T, batch, nrhs, _ = row
    ldd, step_d, stride_d, lde, step_e, stride_e, ldb, stride_b = BC.layout(row)
    D, Bc, X, rhs, Uf, W, _ = BC.exact_chain(row)
    Db, di, up = _lay(D, ldd, step_d, stride_d, 1, upper=True)
    Bb, bi, _ = _lay(rhs[:, None], ldb, 0, stride_b, 3)
    bufs = {"D": Db, "B": Bb, "info": np.full(batch, 77, dtype=np.int32), "logdet": V.nan_pattern(batch, salt=4)}
    if T > 1:
        Eb, ei, _ = _lay(Bc, lde, step_e, stride_e, 2)
        bufs["E"] = Eb

    def enqueue(p, s):
        E = p["E"] if T > 1 else None
        st = L.cap_dpotrf_blocktri_batched(UPPER, n, T, p["D"], ldd, step_d, stride_d, E, lde, step_e, stride_e, p["info"], p["logdet"], batch, s)
        return st or L.cap_dpotrs_blocktri_batched(UPPER, 0, n, T, nrhs, p["D"], ldd, step_d, stride_d, E, lde, step_e, stride_e, p["B"], ldb, stride_b,
                                                   p["info"], batch, s)
    job = SO.Job(bufs, enqueue, label="blocktri")
    with env.ordered(job, label="blocktri factor + solve n=%d T=%d" % (n, T)) as j:
        assert j.ret == 0
        assert not j.snap["info"].any() and np.isfinite(j.snap["logdet"]).all()
        keep = np.ones(Db.shape, dtype=bool)
        keep[di.reshape(-1)] = False
        assert np.array_equal(j.snap["D"][di], np.array([[Uf[c, i][up] for i in range(T)] for c in range(batch)], dtype=np.float64))
        assert np.array_equal(j.snap["D"].view(np.int64)[keep], Db.view(np.int64)[keep])
        if T > 1:
            keep = np.ones(Eb.shape, dtype=bool)
            keep[ei.reshape(-1)] = False
            assert np.array_equal(j.snap["E"][ei], W.reshape(batch, T - 1, -1).astype(np.float64))
            assert np.array_equal(j.snap["E"].view(np.int64)[keep], Eb.view(np.int64)[keep])
        keep = np.ones(Bb.shape, dtype=bool)
        keep[bi.reshape(-1)] = False
        assert np.array_equal(j.snap["B"][bi[:, 0]], X.reshape(batch, -1).astype(np.float64))
        assert np.array_equal(j.snap["B"].view(np.int64)[keep], Bb.view(np.int64)[keep])
