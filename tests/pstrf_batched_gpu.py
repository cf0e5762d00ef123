"""The calls of the batched pivoted Cholesky GPU tests: cap_dpstrf_batched and cap_dpstrf_vbatched through ctypes on PADDED WINDOWS - lda > n,
ldr > max_rank, strides with gaps; a NaN with a payload of its own in A's strictly lower triangle, in all padding and behind every
output; a sentinel after piv, rank, info, resid and logdet.  Every call asserts CAP_OK, that A and all padding are unchanged bit for bit and
that the sentinels stand.  Imported by tests/test_gpu_pstrf_batched.py and tests/test_gpu_pstrf_vbatched.py (-m gpu)."""
import ctypes as C

import numpy as np
import torch

from tests import vbatched_cases as V

DEV = "cuda:0"
UPPER = 1
SENT_I = -7
SENT_F = 123.5


def lib():
    from capital_amd import _lib
    return _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _outputs(batch, npiv):
    piv = torch.full((npiv + 1,), SENT_I, dtype=torch.int64, device=DEV)
    rank = torch.full((batch + 1,), SENT_I, dtype=torch.int32, device=DEV)
    info = torch.full((batch + 1,), SENT_I, dtype=torch.int32, device=DEV)
    resid = torch.full((batch + 1,), SENT_F, dtype=torch.float64, device=DEV)
    logdet = torch.full((batch + 1,), SENT_F, dtype=torch.float64, device=DEV)
    return piv, rank, info, resid, logdet


def fixed(mats, max_rank=None, tol=-1.0, pad_a=3, pad_r=2, gap_a=5, gap_r=7):
    """cap_dpstrf_batched on the n x n NumPy matrices `mats` (their upper triangles are laid out, everything else is NaN): a list of
    (R [max_rank x n], piv, rank, resid, info, logdet) per block, as NumPy / Python values"""
    batch, n = len(mats), mats[0].shape[0]
    mr = n if max_rank is None else max_rank
    lda, ldr = n + pad_a, mr + pad_r
    sa, sr = lda * n + gap_a, ldr * n + gap_r
    A = V.nan_pattern(sa * batch + 4, salt=1)
    r, c = np.triu_indices(n)
    for i, M in enumerate(mats):
        A[i * sa + r + c * lda] = np.asarray(M, dtype=np.float64)[r, c]
    R = V.nan_pattern(sr * batch + 4, salt=2)
    written = np.zeros(R.shape, dtype=bool)
    rr, cc = np.meshgrid(np.arange(mr), np.arange(n), indexing="ij")
    for i in range(batch):
        written[i * sr + rr + cc * ldr] = True
    Ad, Rd = _dev(A), _dev(R)
    piv, rank, info, resid, logdet = _outputs(batch, batch * n)
    st = lib().cap_dpstrf_batched(UPPER, n, mr, float(tol), Ad.data_ptr(), lda, sa, Rd.data_ptr(), ldr, sr, piv.data_ptr(), rank.data_ptr(),
                                  resid.data_ptr(), logdet.data_ptr(), info.data_ptr(), batch, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    assert np.array_equal(Ad.cpu().numpy().view(np.int64), A.view(np.int64)), "A or its padding was written"
    Rh = Rd.cpu().numpy()
    assert np.array_equal(Rh.view(np.int64)[~written], R.view(np.int64)[~written]), "padding or gaps of R were written"
    assert not np.isnan(Rh[written]).any() or any(np.isnan(np.triu(M)).any() for M in mats), "an element of R was not written"
    assert int(piv[-1]) == SENT_I and int(rank[-1]) == SENT_I and int(info[-1]) == SENT_I
    assert float(resid[-1]) == SENT_F and float(logdet[-1]) == SENT_F
    piv, rank, info, resid, logdet = (t.cpu().numpy() for t in (piv, rank, info, resid, logdet))
    out = []
    for i in range(batch):
        Ri = Rh[i * sr + rr + cc * ldr] if mr else np.zeros((0, n))
        out.append((Ri, piv[i * n:(i + 1) * n].copy(), int(rank[i]), float(resid[i]), int(info[i]), float(logdet[i])))
    return out


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*[int(x) for x in a])


class Plan:
    def __init__(self, lay):
        self.L, self.lay, self.p = lib(), lay, C.c_void_p()
        assert self.L.cap_vbatch_plan_create(lay.batch, arr(lay.sizes), arr(lay.ld_arg), arr(lay.off_arg), C.byref(self.p)) == 0

    def close(self):
        self.L.cap_vbatch_plan_destroy(self.p)


def plan(pl, mats, max_rank, tol=-1.0, expect=0):
    """cap_dpstrf_vbatched on the plan `pl` (Plan) with the matrices `mats` (None for an empty block): per block
    (R [n_i x n_i], piv, rank, resid, info, logdet), None for an empty one - whose outputs must still hold the sentinels"""
    lay = pl.lay
    A = lay.buffer(mats)
    R = V.nan_pattern(lay.total + V.GUARD, salt=2)
    Ad, Rd = _dev(A), _dev(R)
    piv, rank, info, resid, logdet = _outputs(lay.batch, lay.rows)
    st = pl.L.cap_dpstrf_vbatched(pl.p, UPPER, max_rank, float(tol), Ad.data_ptr(), Rd.data_ptr(), piv.data_ptr(), rank.data_ptr(),
                                  resid.data_ptr(), logdet.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == expect
    assert np.array_equal(Ad.cpu().numpy().view(np.int64), A.view(np.int64)), "A or its padding was written"
    Rh = Rd.cpu().numpy()
    keep = ~lay.written("window") if expect == 0 else np.ones(R.shape, dtype=bool)
    assert np.array_equal(Rh.view(np.int64)[keep], R.view(np.int64)[keep]), "padding or gaps of R were written"
    assert int(piv[-1]) == SENT_I and int(rank[-1]) == SENT_I and int(info[-1]) == SENT_I
    assert float(resid[-1]) == SENT_F and float(logdet[-1]) == SENT_F
    piv, rank, info, resid, logdet = (t.cpu().numpy() for t in (piv, rank, info, resid, logdet))
    if expect != 0:
        assert np.all(piv == SENT_I) and np.all(rank == SENT_I) and np.all(info == SENT_I) and np.all(resid == SENT_F) and np.all(logdet == SENT_F)
        return None
    out = []
    for i in range(lay.batch):
        n = int(lay.sizes[i])
        if n == 0:
            assert rank[i] == SENT_I and info[i] == SENT_I and resid[i] == SENT_F and logdet[i] == SENT_F
            out.append(None)
            continue
        ro = int(lay.row_off[i])
        out.append((lay.block(Rh, i), piv[ro:ro + n].copy(), int(rank[i]), float(resid[i]), int(info[i]), float(logdet[i])))
    return out
