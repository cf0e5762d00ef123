"""-m gpu: CONTRACT 1 of csrc/symm_batched.hip - every block of a call on a cap_vbatch_plan gets, bit for bit, what the fixed-size entry gives
for it alone with batch = 1 - for the four operations (cap_dsymm_vbatched, cap_dlansy_vbatched, cap_dpocon_vbatched, cap_dpoerr_vbatched),
outputs included, on the mixed size lists of tests/vbatched_cases.py: every class, lone blocks, empty blocks, shuffled order, padded
leading dimensions, gaps.  Random data with full mantissas (any difference in a summation order would show); the flat buffers are NaN
outside the upper triangles, the stacked systems NaN in their pad rows, the entries of empty blocks keep their bits."""
import functools

import numpy as np
import pytest

from tests import potri_batched_cases as P
from tests import symm_batched_gpu as G
from tests import vbatched_cases as V

pytestmark = pytest.mark.gpu

CASES = (("EVERY", "gaps"), ("EVERY", "ld+3"), ("WAVES", "packed"), ("EDGES", "reverse"), ("ONE_CLASS", "ld+3"), ("LONE1", "packed"),
         ("LONE64", "gaps"), ("LONE65", "ld+3"), ("LONE256", "reverse"))
NRHS = 17


@functools.lru_cache(maxsize=None)
def alone(n, seed):
    """the block of size n and seed `seed` through the fixed-size entries with batch = 1: (A, X, B, R, solution, info-free results)"""
    rng = np.random.default_rng([4242, n, seed])
    A = P.random_spd(n, 1e2, 1, seed=seed)[0]
    X = rng.standard_normal((n, NRHS))
    B = A @ X * (1 + 1e-12 * rng.standard_normal((n, NRHS)))
    R = G.factor([A])[0]
    res = {"y": G.symm([A], [X], [B], -1.0, 1.0)[0], "yabs": G.symm([A], [X], [B], 0.5, 2.0, 1)[0], "y0": G.symm([A], [X], None, 1.0, 0.0)[0],
           "norm": G.norm([A])[0]}
    res["rcond"] = G.rcond([R], np.array([res["norm"]]))[0]
    fe, be = G.poerr([A], [R], [B], [X])
    res["ferr"], res["berr"] = fe[0], be[0]
    return A, X, B, R, res


@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_every_block_gets_the_bits_of_the_fixed_size_entry_on_it_alone(name, kind):
    sizes = V.LISTS[name]
    ops = [None if not n else alone(int(n), i % 2) for i, n in enumerate(sizes)]
    pick = lambda k: [None if o is None else o[k] for o in ops]
    pl = G.Plan(sizes, kind)
    try:
        y = pl.symm(pick(0), pick(1), pick(2), NRHS, -1.0, 1.0)
        yabs = pl.symm(pick(0), pick(1), pick(2), NRHS, 0.5, 2.0, 1, inplace=True)
        y0 = pl.symm(pick(0), pick(1), pick(2), NRHS, 1.0, 0.0)
        nm = pl.norm(pick(0))
        anorm = np.where(np.asarray(sizes) > 0, nm, 1.0)
        rc = pl.rcond(pick(3), anorm)
        fe, be = pl.poerr(pick(0), pick(3), pick(2), pick(1), NRHS)
        fe1, be1 = pl.poerr(pick(0), pick(3), pick(2), pick(1), NRHS, want_ferr=False)
        assert fe1 is None
        info = np.zeros(len(sizes), dtype=np.int32)
        live = pl.live()
        info[live[len(live) // 2]] = 4
        rci = pl.rcond(pick(3), anorm, info)
        fei, bei = pl.poerr(pick(0), pick(3), pick(2), pick(1), NRHS, info)
    finally:
        pl.close()
    for i in live:
        res = ops[i][4]
        assert G.same(y[i], res["y"]) and G.same(yabs[i], res["yabs"]) and G.same(y0[i], res["y0"]), "symm, block %d (n = %d)" % (i, sizes[i])
        assert G.same(nm[i], res["norm"]), "norm, block %d" % i
        assert G.same(rc[i], res["rcond"]), "rcond, block %d" % i
        assert G.same(fe[i], res["ferr"]) and G.same(be[i], res["berr"]) and G.same(be1[i], res["berr"]), "bounds, block %d" % i
        if info[i]:
            assert np.isnan(rci[i]) and np.isnan(fei[i]).all() and np.isnan(bei[i]).all()
        else:
            assert G.same(rci[i], res["rcond"]) and G.same(fei[i], res["ferr"]) and G.same(bei[i], res["berr"])


def test_python_layer_on_a_plan():
    import torch
    from capital_amd import batched
    sizes = (5, 0, 100, 8, 64, 200, 0)
    vb = batched.VarBatch(sizes)
    ops = [None if not n else alone(n, 0) for n in sizes]
    A = vb.pack([torch.zeros(0, 0) if o is None else torch.from_numpy(o[0]) for o in ops])
    stack = lambda k: torch.from_numpy(np.concatenate([o[k] for o in ops if o is not None], axis=0).T.copy()).to(A.device)
    X, B = stack(1), stack(2)
    y = vb.symm(A, X, B, alpha=-1.0, beta=1.0)
    nm = vb.norm1(A)
    R = A.clone()
    info = vb.potrf(R)
    rc = vb.rcond(R, nm, info)
    fe, be = vb.error_bounds(A, R, B, X, info)
    f1, b1 = vb.error_bounds(A, R, B[3], X[3], info, ferr=False)
    assert f1 is None and b1.shape == (len(sizes),)
    for i, n in enumerate(sizes):
        if not n:
            assert nm[i] == 0 and rc[i] == 0 and not fe[i].any() and not be[i].any()
            continue
        r0, res = vb.row_offsets[i], ops[i][4]
        assert G.same(y[:, r0:r0 + n].cpu().numpy().T, res["y"]) and G.same(nm[i].item(), res["norm"])
        assert G.same(be[i].cpu().numpy(), res["berr"]) and G.same(b1[i].item(), res["berr"][3])
        # (the plan's potrf leaves the bits of the fixed-size factor: rcond and ferr follow)
        assert G.same(rc[i].item(), res["rcond"]) and G.same(fe[i].cpu().numpy(), res["ferr"])
