"""-m gpu: cap_dgemm_vbatched_inner and cap_dgemm_vbatched_combine (csrc/gemm_batched.hip) on an MI355X.
1. the exact plan rows of tests/gemm_batched_cases.py through both entries, bit for bit against NumPy; X, Y, V, Z keep every bit, NaN
sentinels between and behind the G blocks and in the rows of the stacked C that belong to no block keep theirs
(tests/gemm_batched_gpu.Plan asserts that), 2. CONTRACT 1 (PLAN = FIXED) block by block against the fixed-size entry with batch = 1 on
random data, 3. the empty-block rule of `inner`, 4. VarBatch.inner / .combine against a per-block torch loop on the exact data."""
import numpy as np
import pytest
import torch

from tests import gemm_batched_cases as GC
from tests import gemm_batched_gpu as G

pytestmark = pytest.mark.gpu

NOTRANS, TRANS = G.NOTRANS, G.TRANS


@pytest.mark.parametrize("row", GC.plan_rows(), ids=GC.plan_row_id)
def test_exact_plan_rows_bit_for_bit(row):
    entry, name, kind, (a, b), (alpha, beta) = row
    ops = GC.plan_operands(entry, name, a, b)
    p = G.Plan(GC.PLAN_LISTS[name], kind)
    try:
        old = None if beta == 0.0 else [o[2] for o in ops]
        if entry == "inner":
            out = p.inner([o[0].T for o in ops], [o[1] for o in ops], old, alpha, beta)
        else:
            out = p.combine([o[0] for o in ops], [o[1] for o in ops], old, alpha, beta)
        assert len(out) == len(ops)
        for i, o in enumerate(ops):
            assert G.same(out[i] + 0.0, GC.expected(o[0], o[1], o[2], alpha, beta)), "block %d (n = %d)" % (i, GC.PLAN_LISTS[name][i])
    finally:
        p.close()


MIXED = (0, 1, 64, 65, 256, 7, 8, 9, 16, 17, 33, 0, 130, 192, 193, 5, 6, 7, 8, 3, 2, 1, 8, 8, 8, 12)


@pytest.mark.parametrize("m,n", ((3, 16), (17, 5), (64, 65)))
def test_contract_1_inner_blocks_have_the_bits_of_the_fixed_size_entry(m, n):
    alpha, beta = 1.375, -0.625
    p = G.Plan(MIXED, "gaps")
    try:
        bl = [G.real(m, n, k, i) for i, k in enumerate(MIXED)]
        out = p.inner([b[0].T for b in bl], [b[1] for b in bl], [b[2] for b in bl], alpha, beta)
        for i, b in enumerate(bl):
            alone = G.run(TRANS, NOTRANS, [b[0]], [b[1]], [b[2]], alpha, beta)[0]
            assert G.same(out[i], alone), "block %d (n_i = %d)" % (i, MIXED[i])
    finally:
        p.close()


@pytest.mark.parametrize("nrhs,k", ((16, 4), (17, 40), (70, 3)))
def test_contract_1_combine_blocks_have_the_bits_of_the_fixed_size_entry(nrhs, k):
    alpha, beta = -0.75, 1.25
    p = G.Plan(MIXED, "ld+3")
    try:
        bl = [G.real(n, nrhs, k, i) for i, n in enumerate(MIXED)]
        out = p.combine([b[0] for b in bl], [b[1] for b in bl], [b[2] for b in bl], alpha, beta)
        for i, b in enumerate(bl):
            if MIXED[i] == 0:
                assert out[i].shape == (0, nrhs)
                continue
            alone = G.run(NOTRANS, NOTRANS, [b[0]], [b[1]], [b[2]], alpha, beta)[0]
            assert G.same(out[i], alone), "block %d (n_i = %d)" % (i, MIXED[i])
    finally:
        p.close()


@pytest.mark.parametrize("sizes", ((0, 5, 0, 0, 70, 8, 0), (0, 0, 0)))
def test_an_empty_block_of_inner_is_an_empty_sum(sizes):
    p = G.Plan(sizes, "packed")
    try:
        m, n = 3, 5
        bl = [G.real(m, n, k, i) for i, k in enumerate(sizes)]
        out = p.inner([b[0].T for b in bl], [b[1] for b in bl], [b[2] for b in bl], 2.0, 0.5)          # G_i <- beta G_i
        for i, b in enumerate(bl):
            if sizes[i] == 0:
                assert G.same(out[i], 0.5 * b[2]), i
        out = p.inner([b[0].T for b in bl], [b[1] for b in bl], None, 2.0, 0.0)                        # beta == 0: +0.0 over the NaN
        for i in range(len(sizes)):
            if sizes[i] == 0:
                assert G.same(out[i], np.zeros((m, n))), i
            else:
                assert np.isfinite(out[i]).all()
    finally:
        p.close()


@pytest.mark.parametrize("name", ("JACOBI", "EMPTIES"))
def test_varbatch_inner_and_combine_against_a_torch_loop(name):
    from capital_amd import batched
    sizes = GC.PLAN_LISTS[name]
    vb = batched.VarBatch(sizes)
    p, q, k = 3, 16, 4
    io = GC.plan_operands("inner", name, p, q)
    X = torch.from_numpy(np.ascontiguousarray(np.concatenate([o[0] for o in io], axis=1))).to(G.DEV)                 # (p, rows)
    Y = torch.from_numpy(np.ascontiguousarray(np.concatenate([o[1].T for o in io], axis=1))).to(G.DEV)               # (q, rows)
    got = vb.inner(X, Y)
    assert got.shape == (len(sizes), p, q)
    old = torch.from_numpy(np.ascontiguousarray(np.stack([o[2] for o in io]))).to(G.DEV)
    upd = vb.inner(X, Y, out=old.clone(), alpha=-1.0, beta=0.5)
    for i, n in enumerate(sizes):
        r0 = vb.row_offsets[i]
        want = X[:, r0:r0 + n] @ Y[:, r0:r0 + n].T
        assert torch.equal(got[i] + 0.0, want + 0.0), i
        assert torch.equal(upd[i] + 0.0, 0.5 * old[i] - want + 0.0), i
    vec = vb.inner(X[0], Y)
    assert vec.shape == (len(sizes), q) and torch.equal(vec, got[:, 0, :])
    assert vb.inner(X[0], Y[1]).shape == (len(sizes),)

    co = GC.plan_operands("combine", name, q, k)                                               # V_i n_i x k, Z_i k x q
    V = torch.from_numpy(np.ascontiguousarray(np.concatenate([o[0].T for o in co], axis=1))).to(G.DEV)               # (k, rows)
    Z = torch.from_numpy(np.ascontiguousarray(np.stack([o[1].T for o in co]))).to(G.DEV)                             # (batch, q, k)
    base = torch.full((q, vb.rows + 2), float("nan"), dtype=torch.float64, device=G.DEV)
    out = base[:, :vb.rows]
    res = vb.combine(Z, V, out=out)
    assert res is out and torch.isnan(base[:, vb.rows:]).all()
    for i, n in enumerate(sizes):
        r0 = vb.row_offsets[i]
        assert torch.equal(out[:, r0:r0 + n] + 0.0, Z[i] @ V[:, r0:r0 + n] + 0.0), i
    fresh = vb.combine(Z, V)
    assert torch.equal(fresh, out)
    from capital_amd import _lib
    for bad in (lambda: vb.inner(X.cpu(), Y), lambda: vb.inner(X, Y[:, :-1]), lambda: vb.inner(X, Y, beta=1.0), lambda: vb.inner(X.float(), Y),
                lambda: vb.combine(Z[:, :, :2], V), lambda: vb.combine(Z, V, beta=2.0), lambda: vb.combine(Z[:-1], V),
                lambda: vb.inner(X, Y, out=torch.zeros(len(sizes), p, q + 1, dtype=torch.float64, device=G.DEV))):
        with pytest.raises(_lib.CapitalError):
            bad()
