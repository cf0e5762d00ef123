"""-m gpu: the batched pivoted Cholesky factorization on a plan, cap_dpstrf_vbatched (csrc/pstrf_batched.hip), and VarBatch.pstrf /
VarBatch.permute.  NO TOLERANCE: every block of a plan call must equal, bit for bit and in all five outputs (and logdet), what the
fixed-size entry gives for it alone with n = n_i, max_rank = min(max_rank, n_i) and batch = 1; the rows min(max_rank, n_i) .. n_i - 1 of
its R block are +0.0, padding and gaps are untouched, the outputs of empty blocks are not written.

Size lists within n <= 64: every size 0 .. 64 (shuffled), a list with empty blocks and mixed waves, a single-class list, a lone block of
1 and of 64 - in the layouts of tests/vbatched_cases.Layout.  The blocks are full rank, of rank n // 3 + 1 and numerically low rank in
turn (tests/pstrf_batched_cases.plan_matrix).  The fixed-size results are computed once per (list, cap, tol) and shared by the layouts.  A
plan that holds a block of 65 is refused with nothing written."""
import functools

import numpy as np
import pytest
import torch

from tests import pstrf_batched_cases as PC
from tests import pstrf_batched_gpu as G
from tests import pstrf_model as pm
from tests import vbatched_cases as V

pytestmark = pytest.mark.gpu


def _every():
    sizes = list(range(65))
    np.random.default_rng(2701).shuffle(sizes)
    return tuple(int(x) for x in sizes)


LISTS = {"EVERY": _every(), "EMPTIES": (0, 5, 0, 8, 9, 0, 16, 17, 3, 0, 33, 7, 7, 6, 5, 8, 8, 1, 2, 0), "ONE_CLASS": (12,) * 9, "LONE1": (1,),
         "LONE64": (64,)}
CALLS = ((64, -1.0), (5, -1.0), (0, -1.0), (64, 1e-3))


def _mats(name):
    return [PC.plan_matrix(n, i) for i, n in enumerate(LISTS[name])]


@functools.lru_cache(maxsize=None)
def _alone(name, mr, tol):
    """the fixed-size entry on every block of the list alone"""
    return [None if M is None else G.fixed([M], min(mr, M.shape[0]), tol)[0] for M in _mats(name)]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("kind", V.LAYOUTS)
@pytest.mark.parametrize("name", sorted(LISTS))
def test_every_block_has_the_bits_of_the_fixed_size_entry(name, kind):
    lay = V.Layout(LISTS[name], kind)
    pl = G.Plan(lay)
    try:
        for mr, tol in CALLS if name in ("EVERY", "EMPTIES") or kind == "gaps" else CALLS[:1]:
            got = G.plan(pl, _mats(name), mr, tol)
            for i, (g, w) in enumerate(zip(got, _alone(name, mr, tol))):
                if w is None:
                    assert g is None
                    continue
                n = int(lay.sizes[i])
                cap = min(mr, n)
                assert g[0].shape == (n, n) and np.array_equal(_bits(g[0][:cap]), _bits(w[0])), "R of block %d (n = %d)" % (i, n)
                assert np.array_equal(_bits(g[0][cap:]), np.zeros((n - cap, n), dtype=np.int64)), "rows >= the cap of block %d are not +0.0" % i
                assert np.array_equal(g[1], w[1]) and (g[2], g[4]) == (w[2], w[4]), "piv, rank or info of block %d" % i
                assert np.array_equal(_bits(g[3]), _bits(w[3])) and np.array_equal(_bits(g[5]), _bits(w[5])), "resid or logdet of block %d" % i
    finally:
        pl.close()


def test_a_plan_with_a_block_of_65_is_refused_with_nothing_written():
    lay = V.Layout((8, 65, 3), "gaps")
    pl = G.Plan(lay)
    try:
        mats = [pm.dominant(int(n), 3) for n in lay.sizes]
        assert G.plan(pl, mats, 64, -1.0, expect=4) is None         # CAP_ERR_UNSUPPORTED; the helper asserts that every buffer is untouched
    finally:
        pl.close()


def test_python_varbatch_pstrf_and_permute():
    from capital_amd import _lib, batched
    sizes = LISTS["EMPTIES"]
    mats = _mats("EMPTIES")
    vb = batched.VarBatch(sizes)
    lay = V.Layout(sizes, "packed")
    buf = lay.buffer(mats)
    A = torch.from_numpy(buf[:max(lay.total, 1)].copy()).to(G.DEV)[:lay.total]
    R, piv, rank, resid, info, logdet = vb.pstrf(A, logdet=True)
    torch.cuda.synchronize()
    assert np.array_equal(A.cpu().numpy().view(np.int64), buf[:lay.total].view(np.int64))
    assert R.shape == (vb.total,) and piv.shape == (vb.rows,) and piv.dtype == torch.int64 and rank.shape == (vb.batch,)
    want = _alone("EMPTIES", 64, -1.0)
    for i, w in enumerate(want):
        if w is None:
            assert (int(rank[i]), int(info[i]), float(resid[i]), float(logdet[i])) == (0, 0, 0.0, 0.0)      # an empty block
            continue
        n = sizes[i]
        Li = vb.block(R, i).cpu().numpy()                       # torch's reading: L = R^T
        assert np.array_equal(_bits(Li.T), _bits(w[0])) and np.all(np.triu(Li, 1) == 0)
        ro = vb.row_offsets[i]
        assert np.array_equal(piv[ro:ro + n].cpu().numpy(), w[1]) and (int(rank[i]), int(info[i])) == (w[2], w[4])
        assert np.array_equal(_bits(float(resid[i])), _bits(w[3])) and np.array_equal(_bits(float(logdet[i])), _bits(w[5]))
    b = torch.arange(float(vb.rows), dtype=torch.float64, device=G.DEV)
    fwd = vb.permute(b, piv)
    for i, n in enumerate(sizes):
        ro = vb.row_offsets[i]
        assert torch.equal(fwd[ro:ro + n], b[ro:ro + n][piv[ro:ro + n]])
    assert torch.equal(vb.permute(fwd, piv, inverse=True), b)
    b2 = torch.stack([b, 2 * b])
    assert torch.equal(vb.permute(vb.permute(b2, piv), piv, inverse=True), b2) and torch.equal(vb.permute(b2, piv)[1], 2 * fwd)
    big = batched.VarBatch((8, 65))
    with pytest.raises(_lib.CapitalError, match="factor_pivoted"):
        big.pstrf(torch.zeros(big.total, dtype=torch.float64, device=G.DEV))
    for bad in (lambda: vb.pstrf(A, max_rank=-1), lambda: vb.pstrf(A, tol=float("nan")), lambda: vb.pstrf(A[:5]), lambda: vb.pstrf(A.float()),
                lambda: vb.permute(b[:-1], piv), lambda: vb.permute(b, piv.int())):
        with pytest.raises(_lib.CapitalError):
            bad()
    capped = vb.pstrf(A, max_rank=200)                          # a cap above every n_i is no cap
    assert torch.equal(capped[0], R) and torch.equal(capped[1], piv)
