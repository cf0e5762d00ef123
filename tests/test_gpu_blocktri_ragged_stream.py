"""-m gpu: stream order of cap_dpotrf_blocktri_vbatched, cap_dpotrs_blocktri_vbatched and cap_dpotri_blocktri_vbatched as ORDERED CALLS
(tests/stream_order.py): the caller's stream is a non-blocking stream of the test's own, the calls are enqueued behind a device-side
delay, every buffer is poison until that stream's own copies deliver the contents, a snapshot and a poison fill follow the calls, the
host waits for that stream only.  The premise - everything was enqueued before the delay ended - is asserted by the helper.  The plan is
made in front of the ordered section: making it may synchronise, using it must not.

Exact: the chains are tests/blocktri_ragged_cases.py's exact family.  Factor -> solve -> inverse run on ONE stream: the solve reads the
factor, the inverse overwrites it behind the solve.  The solution is held to X with no tolerance; the factor is seen through a second
pair of buffers that only the factor touches (held to R); the selected inverse is held, bit for bit, to what the same three calls give
on the default stream with a host synchronisation after each; every word outside what the calls write to what the buffer held before,
the info / logdet entries of empty chains included."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import blocktri_ragged_cases as RC  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402

UPPER = 1
ROW_ID = lambda r: "n%d-T%s" % (r[0], "_".join(str(t) for t in r[1]))


@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


def _lay(row, mats, salt, upper):
    """mats[chain][position] column-major in the slots of a buffer of distinct NaNs -> (buffer, flat index of every element laid in)"""
    n, lengths = row[0], row[1]
    first, _, slots, _, _ = RC.geometry(row)
    ld, step, _ = RC.layout(row)
    buf = V.nan_pattern(step * max(slots - 1, 0) + ld * n + 8, salt=salt)
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = (r <= c) if upper else (r >= 0)
    idx = []
    for ch, blocks in enumerate(mats):
        for i, m in enumerate(blocks):
            at = (first[ch] + i) * step + r[keep] + c[keep] * ld
            buf[at] = np.asarray(m, dtype=np.float64)[keep]
            idx.append(at)
    return buf, (np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)), keep


@pytest.mark.parametrize("row", RC.STREAM_ROWS, ids=ROW_ID)
def test_factor_solve_inverse_in_stream_order(env, row):
    import torch
    from capital_amd import _lib
    L = _lib.lib()
    n, lengths, mode, nrhs, _ = row
    batch = len(lengths)
    first, rows_at, slots, eslots, rows = RC.geometry(row)
    ld, step, ldb = RC.layout(row)
    chains = [RC.exact_chain(row, c) for c in range(batch)]
    Db, di, up = _lay(row, [ch[0] for ch in chains], 1, upper=True)
    Eb, ei, _ = _lay(row, [ch[1] for ch in chains], 2, upper=False)
    Bb = V.nan_pattern(ldb * (nrhs - 1) + rows * n + 8, salt=3)
    bi = np.array([k * ldb + (rows_at[c] + i // n) * n + i % n for c in range(batch) for i in range(lengths[c] * n) for k in range(nrhs)], dtype=np.int64)
    Bb[bi] = np.array([chains[c][3][i, k] for c in range(batch) for i in range(lengths[c] * n) for k in range(nrhs)], dtype=np.float64)
    bufs = {"D": Db, "E": Eb, "B": Bb, "D2": Db.copy(), "E2": Eb.copy(), "info": np.full(batch, 77, dtype=np.int32),
            "info2": np.full(batch, 77, dtype=np.int32), "logdet": V.nan_pattern(batch, salt=4)}
    plan = C.c_void_p()
    fs = RC.first_slots(lengths, mode)
    arr = lambda seq: (C.c_int64 * len(seq))(*seq)
    assert L.cap_blocktri_plan_create(batch, arr(list(lengths)), arr(fs) if fs is not None else None, C.byref(plan)) == 0

    def three(D, E, B, info, logdet, s):
        st = L.cap_dpotrf_blocktri_vbatched(plan, UPPER, n, D, ld, step, E, ld, step, info, logdet, s)
        st = st or L.cap_dpotrs_blocktri_vbatched(plan, UPPER, 0, n, nrhs, D, ld, step, E, ld, step, B, ldb, info, s)
        return st or L.cap_dpotri_blocktri_vbatched(plan, UPPER, 1, n, D, ld, step, E, ld, step, info, s)

    # the reference for the inverse: the same calls on the default stream, a host synchronisation behind each
    ref = {k: torch.from_numpy(bufs[k].copy()).cuda() for k in ("D", "E", "B", "info", "logdet")}
    for call in (lambda: L.cap_dpotrf_blocktri_vbatched(plan, UPPER, n, ref["D"].data_ptr(), ld, step, ref["E"].data_ptr(), ld, step, ref["info"].data_ptr(),
                                                         ref["logdet"].data_ptr(), None),
                 lambda: L.cap_dpotrs_blocktri_vbatched(plan, UPPER, 0, n, nrhs, ref["D"].data_ptr(), ld, step, ref["E"].data_ptr(), ld, step,
                                                         ref["B"].data_ptr(), ldb, ref["info"].data_ptr(), None),
                 lambda: L.cap_dpotri_blocktri_vbatched(plan, UPPER, 1, n, ref["D"].data_ptr(), ld, step, ref["E"].data_ptr(), ld, step, ref["info"].data_ptr(),
                                                         None)):
        assert call() == 0
        torch.cuda.synchronize()
    ref = {k: v.cpu().numpy() for k, v in ref.items()}

    def enqueue(p, s):
        st = three(p["D"], p["E"], p["B"], p["info"], p["logdet"], s)
        return st or L.cap_dpotrf_blocktri_vbatched(plan, UPPER, n, p["D2"], ld, step, p["E2"], ld, step, p["info2"], None, s)
    job = SO.Job(bufs, enqueue, label="ragged blocktri")
    try:
        with env.ordered(job, label="ragged blocktri factor + solve + inverse n=%d" % n) as j:
            assert j.ret == 0
            live = np.array([t > 0 for t in lengths])
            for name in ("info", "info2"):
                assert not j.snap[name][live].any() and (j.snap[name][~live] == 77).all()
            assert np.isfinite(j.snap["logdet"][live]).all()
            assert np.array_equal(j.snap["logdet"].view(np.int64)[~live], bufs["logdet"].view(np.int64)[~live])
            # the factor, through the pair only the factor touched
            keep = np.ones(Db.shape, dtype=bool)
            keep[di] = False
            assert np.array_equal(j.snap["D2"][di], np.concatenate([ch[4][i][up] for ch in chains for i in range(ch[4].shape[0])] or [np.zeros(0)]).astype(np.float64))
            assert np.array_equal(j.snap["D2"].view(np.int64)[keep], Db.view(np.int64)[keep])
            keep = np.ones(Eb.shape, dtype=bool)
            keep[ei] = False
            assert np.array_equal(j.snap["E2"][ei], np.concatenate([ch[5][i].reshape(-1) for ch in chains for i in range(ch[5].shape[0])] or [np.zeros(0)]).astype(np.float64))
            assert np.array_equal(j.snap["E2"].view(np.int64)[keep], Eb.view(np.int64)[keep])
            # the solution
            keep = np.ones(Bb.shape, dtype=bool)
            keep[bi] = False
            want = np.array([chains[c][2][i, k] for c in range(batch) for i in range(lengths[c] * n) for k in range(nrhs)], dtype=np.float64)
            assert np.array_equal(j.snap["B"][bi], want)
            assert np.array_equal(j.snap["B"].view(np.int64)[keep], Bb.view(np.int64)[keep])
            # the selected inverse behind the solve: the bits of the synchronous run, whole buffers
            for name in ("D", "E", "B", "logdet"):
                assert np.array_equal(j.snap[name].view(np.int64), ref[name].view(np.int64)), name
            short = max(lengths) < 64            # (the covariances of the exact family grow with the chain: the 257-long one overflows, in both runs alike)
            assert not short or (np.isfinite(j.snap["D"][di]).all() and np.isfinite(j.snap["E"][ei]).all())
    finally:
        L.cap_blocktri_plan_destroy(plan)
