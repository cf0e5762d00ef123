"""-m gpu: stream order of cap_dpotri_blocktri_batched as an ORDERED CALL (tests/stream_order.py): the caller's stream is a non-blocking
stream of the test's own, the call is enqueued behind a device-side delay, every buffer is poison until that stream's own copies
deliver the contents, a snapshot and a poison fill follow the call, the host waits for that stream only.  The premise - everything was
enqueued before the delay ended - is asserted by the helper.

Exact: the factors are those of tests/blocktri_potri_cases.py's exact family, so D and E are held to the closed forms with no tolerance,
and every word outside what the call writes to what the buffer held before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import blocktri_potri_cases as IC  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402

ROWS = [(r, f) for r, f in IC.exact_rows() if (r[0], r[1], f) in ((9, 1, "F1"), (17, 3, "F2"), (64, 2, "F2i"))]
UPPER = 1


@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


def _lay(mats, ld, step, stride, salt, upper):
    """mats[chain][position] column-major in a buffer of distinct NaNs -> (buffer, flat index of every element laid in, the mask)"""
    batch, blocks = len(mats), len(mats[0])
    n = mats[0][0].shape[0]
    buf = V.nan_pattern(stride * (batch - 1) + step * max(blocks - 1, 0) + ld * n + 8, salt=salt)
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = (r <= c) if upper else (r >= 0)
    idx = np.array([[ch * stride + i * step + r[keep] + c[keep] * ld for i in range(blocks)] for ch in range(batch)], dtype=np.int64).reshape(batch, blocks, -1)
    for ch in range(batch):
        for i in range(blocks):
            buf[idx[ch, i]] = np.asarray(mats[ch][i], dtype=np.float64)[keep]
    return buf, idx, keep


@pytest.mark.parametrize("row,fam", ROWS, ids=lambda v: IC.row_id(v) if isinstance(v, tuple) else v)
def test_selected_inverse_in_stream_order(env, row, fam):
    from capital_amd import _lib
    L = _lib.lib()
    n, T, batch, fill, _ = row
    ldd, step_d, stride_d, lde, step_e, stride_e = IC.layout(row)
    U, W, Sd, Sc, _ = IC.exact_chain(row, fam)
    Db, di, up = _lay(U, ldd, step_d, stride_d, 1, upper=True)
    bufs = {"D": Db, "info": np.zeros(batch, dtype=np.int32)}
    if T > 1:
        Eb, ei, _ = _lay(W, lde, step_e, stride_e, 2, upper=False)
        bufs["E"] = Eb

    def enqueue(p, s):
        return L.cap_dpotri_blocktri_batched(UPPER, fill, n, T, p["D"], ldd, step_d, stride_d, p["E"] if T > 1 else None, lde, step_e, stride_e,
                                             p["info"], batch, s)
    job = SO.Job(bufs, enqueue, label="blocktri potri")
    with env.ordered(job, label="blocktri potri n=%d T=%d" % (n, T)) as j:
        assert j.ret == 0 and not j.snap["info"].any()
        _, wi, wk = _lay(U, ldd, step_d, stride_d, 1, upper=not fill)          # what the call writes: the triangles, or the blocks with fill
        keep = np.ones(Db.shape, dtype=bool)
        keep[wi.reshape(-1)] = False
        assert np.array_equal(j.snap["D"][wi], np.array([[Sd[c, i][wk] for i in range(T)] for c in range(batch)], dtype=np.float64))
        assert np.array_equal(j.snap["D"].view(np.int64)[keep], Db.view(np.int64)[keep])
        if T > 1:
            keep = np.ones(Eb.shape, dtype=bool)
            keep[ei.reshape(-1)] = False
            assert np.array_equal(j.snap["E"][ei], Sc.reshape(batch, T - 1, -1))
            assert np.array_equal(j.snap["E"].view(np.int64)[keep], Eb.view(np.int64)[keep])
