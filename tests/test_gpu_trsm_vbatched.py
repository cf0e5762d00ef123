"""-m gpu: the batched triangular solves and products on a cap_vbatch_plan (cap_dtrsm_vbatched, cap_dtrmm_vbatched, VarBatch.trsm / trmm /
mahalanobis).

1. exact results on the list EVERY (no tolerance, nothing else touched), 2. CONTRACT 2: every block of a plan call against the fixed-size
entry on it alone with batch = 1, sumsq included, on the lists of tests/vbatched_cases.py in two layouts, 3. the two halves against
cap_dpotrs_vbatched, 4. failed and empty blocks, 5. stream order, 6. the Python layer."""
import functools

import numpy as np
import pytest
import torch

from tests import stream_order as SO
from tests import trsm_batched_cases as TC
from tests import trsm_batched_gpu as G
from tests import vbatched_cases as V
from tests.tri_cases import positive_zero

pytestmark = pytest.mark.gpu

TRANS, NOTRANS = G.TRANS, G.NOTRANS
NRHS = 17
OPS = (("trsm", TRANS), ("trsm", NOTRANS), ("trmm", TRANS), ("trmm", NOTRANS))


def _exact(a):
    return positive_zero(np.asarray(a)).view(np.int64)


@functools.lru_cache(maxsize=None)
def _data(name):
    """(triangles, right-hand sides) of a size list: random, seeded by position, None for an empty block; never written"""
    sizes = V.LISTS[name]
    Rs = [G.triangle(n, i) if n else None for i, n in enumerate(sizes)]
    Bs = [np.random.default_rng([6, n, i]).standard_normal((n, NRHS)) if n else None for i, n in enumerate(sizes)]
    for a in Rs + Bs:
        if a is not None:
            a.setflags(write=False)
    return tuple(Rs), tuple(Bs)


@functools.lru_cache(maxsize=None)
def _alone(name, entry, trans, i):
    """the fixed-size entry on block i alone, batch = 1 -> (result, sumsq row or None); computed once, shared by the layouts"""
    Rs, Bs = _data(name)
    got, q = G.run(entry, trans, [Rs[i]], [Bs[i]], (0, 0), sumsq=entry == "trsm")
    return got[0], (None if q is None else q[0])


# ---- 1. exact ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", V.FAMILIES)
def test_exact_results_on_every_size_of_a_plan(fam):
    sizes = V.EVERY
    blocks = V.exact_blocks(fam, sizes)
    ops = [None if b is None else TC.operands(fam, int(n), 3, i % 5) for i, (b, n) in enumerate(zip(blocks, sizes))]
    for o, b in zip(ops, blocks):
        assert o is None or o[0] is b[0]
        if o is not None:                # EVERY holds sizes the fixed-size rows do not: the exactness premise, per block
            assert all(v < TC.LIMIT for v in TC.premise(o[0], o[1], o[2]).values())
    p = G.Plan(sizes, "gaps")
    try:
        Ts = [None if o is None else o[0] for o in ops]
        Xs = [None if o is None else o[2] for o in ops]
        for trans, at in ((TRANS, 3), (NOTRANS, 4)):
            rhs = [None if o is None else o[at] for o in ops]
            got, q = p.run("trsm", trans, Ts, rhs, 3, info=[0] * len(sizes), sumsq=True)
            prod, _ = p.run("trmm", trans, Ts, Xs, 3)
            for i, o in enumerate(ops):
                if o is None:
                    continue
                assert np.array_equal(_exact(got[i]), _exact(o[2])), "trsm trans=%d block %d (n = %d)" % (trans, i, sizes[i])
                assert np.array_equal(q[i], (o[2] ** 2).sum(axis=0))
                assert np.array_equal(_exact(prod[i]), _exact(o[at])), "trmm trans=%d block %d (n = %d)" % (trans, i, sizes[i])
    finally:
        p.close()


# ---- 2. contract 2: plan = fixed --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(V.LISTS))
@pytest.mark.parametrize("kind", ("gaps", "ld+3"))
def test_every_block_of_a_plan_gets_the_bits_of_the_fixed_size_entry(name, kind):
    sizes = V.LISTS[name]
    Rs, Bs = _data(name)
    p = G.Plan(sizes, kind)
    try:
        for entry, trans in OPS:
            got, q = p.run(entry, trans, Rs, Bs, NRHS, sumsq=entry == "trsm")
            for i, n in enumerate(sizes):
                if not n:
                    continue
                want, wq = _alone(name, entry, trans, i)
                assert G.same(got[i], want), "%s trans=%d block %d (n = %d)" % (entry, trans, i, n)
                if wq is not None:
                    assert G.same(q[i], wq), "%s trans=%d block %d (n = %d): sumsq" % (entry, trans, i, n)
    finally:
        p.close()


# ---- 3. the halves against cap_dpotrs_vbatched ------------------------------------------------------------------------------------------------
def test_the_two_halves_leave_the_bits_of_potrs_on_a_plan():
    sizes = V.EVERY
    Rs, Bs = _data("EVERY")
    info = [0] * len(sizes)
    info[3] = info[10] = 2
    p = G.Plan(sizes, "reverse")
    try:
        want, _ = p.run("potrs", 0, Rs, Bs, NRHS, info=info)
        half, _ = p.run("trsm", TRANS, Rs, Bs, NRHS, info=info)
        got, _ = p.run("trsm", NOTRANS, Rs, half, NRHS, info=info)
        for i, n in enumerate(sizes):
            if n:
                assert G.same(got[i], want[i]), "block %d (n = %d)" % (i, n)
                assert bool(np.isnan(got[i]).all()) == (info[i] != 0)
    finally:
        p.close()


# ---- 4. failed and empty blocks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,trans", OPS)
def test_failed_blocks_get_nan_and_empty_blocks_nothing(entry, trans):
    sizes = V.WAVES                      # eight blocks per wavefront; run() checks that the sumsq rows of empty blocks keep their bits
    sizes = sizes[:20] + (0,) + sizes[20:]
    Rs = [G.triangle(n, i) if n else None for i, n in enumerate(sizes)]
    Bs = [np.random.default_rng([7, n, i]).standard_normal((n, 3)) if n else None for i, n in enumerate(sizes)]
    info = [0] * len(sizes)
    for i in (1, 9, 20, len(sizes) - 1):  # (20 is the empty block: its word is not read)
        info[i] = 5
    ss = entry == "trsm"
    p = G.Plan(sizes, "packed")
    try:
        free, qf = p.run(entry, trans, Rs, Bs, 3, info=None, sumsq=ss)
        got, q = p.run(entry, trans, Rs, Bs, 3, info=info, sumsq=ss)
        for i, n in enumerate(sizes):
            if not n:
                continue
            if info[i]:
                assert np.isnan(got[i]).all() and (not ss or np.isnan(q[i]).all())
            else:
                assert np.isfinite(free[i]).all() and G.same(got[i], free[i]) and (not ss or G.same(q[i], qf[i]))
    finally:
        p.close()


# ---- 5. stream order ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


@pytest.mark.parametrize("entry", ("trsm", "trmm"))
def test_plan_entries_in_stream_order(env, entry):
    L = G.lib()
    Rs, Bs = _data("EVERY")
    p = G.Plan(V.EVERY, "gaps")          # made beforehand: cap_vbatch_plan_create may synchronise, the entries may not
    try:
        lay = p.lay
        R0 = lay.buffer(Rs)
        B0, ldb = p.stacked(Bs, NRHS)
        bufs = {"R": R0, "B": B0, "info": np.zeros(lay.batch, dtype=np.int32), "q": np.full(lay.batch * NRHS, 5.0)}

        def enqueue(ptr, s):
            if entry == "trsm":
                return L.cap_dtrsm_vbatched(p.plan, 1, NOTRANS, NRHS, ptr["R"], ptr["B"], ldb, ptr["info"], ptr["q"], NRHS, s)
            return L.cap_dtrmm_vbatched(p.plan, 1, TRANS, NRHS, ptr["R"], ptr["B"], ldb, ptr["info"], s)
        job = SO.Job(bufs, enqueue, label=entry + "_vbatched")
        want, ret = env.plain(job)
        assert ret == 0 and not np.isnan(want["B"][:lay.rows]).any()
        with env.ordered(job, label="cap_d%s_vbatched EVERY nrhs 17" % entry) as j:
            assert j.ret == 0
            for name in bufs:
                assert SO.same_bits(j.snap[name], want[name]), name
            assert SO.same_bits(j.snap["R"], R0) and not SO.same_bits(j.snap["B"], B0)
    finally:
        p.close()


# ---- 6. the Python layer -----------------------------------------------------------------------------------------------------------------------
def test_varbatch_methods_give_the_bits_of_the_c_abi():
    from capital_amd import batched
    sizes = V.EDGES[:7] + (0, 5)
    Rs = [G.triangle(n, i) if n else None for i, n in enumerate(sizes)]
    Bs = [np.random.default_rng([9, n, i]).standard_normal((n, 4)) if n else None for i, n in enumerate(sizes)]
    p = G.Plan(sizes, "packed")
    vb = batched.VarBatch(sizes)
    try:
        assert vb.total == p.lay.total and vb.rows == p.lay.rows
        Rt = torch.from_numpy(np.nan_to_num(p.lay.buffer(Rs)[:vb.total], nan=0.0)).to(G.DEV)
        stack = lambda: torch.from_numpy(np.concatenate([b.T for b in Bs if b is not None], axis=1).copy()).to(G.DEV)     # (nrhs, rows)
        rows = lambda t, i: t.cpu().numpy()[:, p.lay.row_off[i]:p.lay.row_off[i] + sizes[i]].T
        info = torch.zeros(len(sizes), dtype=torch.int32, device=G.DEV)
        info[2] = 1
        inf = info.cpu().numpy().tolist()
        for trans in (True, False):
            want, q = p.run("trsm", int(trans), Rs, Bs, 4, info=inf, sumsq=True)
            B = stack()
            out, qq = vb.trsm(Rt, B, trans=trans, info=info, sumsq=True)
            assert out is B and qq.shape == (len(sizes), 4)
            prod, _ = p.run("trmm", int(trans), Rs, Bs, 4, info=inf)
            M = stack()
            assert vb.trmm(Rt, M, trans=trans, info=info) is M
            for i, n in enumerate(sizes):
                if n:
                    assert G.same(rows(B, i), want[i]) and G.same(qq.cpu().numpy()[i], q[i]) and G.same(rows(M, i), prod[i])
                else:
                    assert not qq.cpu().numpy()[i].any()           # an empty block reads 0
        want, q = p.run("trsm", TRANS, Rs, [None if b is None else b[:, :1] for b in Bs], 1, sumsq=True)
        b1 = stack()[0].contiguous()
        d2 = vb.mahalanobis(Rt, b1)
        assert d2.shape == (len(sizes),)
        for i, n in enumerate(sizes):
            assert G.same(d2.cpu().numpy()[i], q[i, 0] if n else 0.0)
    finally:
        p.close()
