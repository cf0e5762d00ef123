"""-m gpu: the ragged block-tridiagonal entries (batched.VarChains -> cap_dpotrf_blocktri_vbatched, cap_dpotrs_blocktri_vbatched,
cap_dpotri_blocktri_vbatched, csrc/blocktri_vbatched.hip) on every row of tests/blocktri_ragged_cases.py.

THE BIT CONTRACT, no tolerance anywhere: every chain gets what the fixed-size entry gives for it alone.  The reference is one fixed-size
call per chain (batch = 1) on views of a clone, and the comparison is of the WHOLE flat buffers, which start as distinct NaNs around the
blocks, in the gaps between chains, in each chain's unused E slot and in the strictly lower triangles (tests/blocktri_ragged_gpu.py) - so
the same comparison shows that nothing outside what a call may write changed a bit.  Checked: the factor (D, E, info, logdet), the three
solve halves (and forward then backward = the full solve), the inverse with and without symmetric; info / logdet of T = 0 chains are not
written by the C entry.  On the EXACT family the factor equals R, the solution X and log det the closed form; that family is also the
trap for stale images: a stored U read again as a symmetric block has a non-positive second pivot wherever N[0, 1] != 0, so a kernel
that keeps accumulating after a chain's end shows a spurious info or other log-det bits on the short chains.  Company independence,
a failing chain in the middle of a wavefront, failures through solve and inverse, equal lengths against the batched fixed-size call."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import blocktri_ragged_cases as RC  # noqa: E402
from tests import blocktri_ragged_gpu as G  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402

ROW_ID = lambda r: "n%d-T%s-%s-k%d-%s" % (r[0], "_".join(str(t) for t in r[1][:11]), r[2], r[3], r[4])


def _walk(new, fam):
    """factor, the solves and the inverses of `new` against the fixed-size route on a clone, bit for bit"""
    old = new.clone()
    info, ld = new.factor()
    info0, ld0 = old.fixed_factor()
    new.same_as(old, ("D", "E"))
    assert np.array_equal(info, info0), (info, info0)
    assert np.array_equal(ld.view(np.int64), ld0.view(np.int64)), (ld, ld0)
    dinfo = torch.from_numpy(info).to(G.DEV)
    new.solve(info=dinfo)
    old.fixed_solve(info=dinfo)
    new.same_as(old, ("D", "E", "B"))
    full = new.flat["B"].clone()
    for half in ("forward", "backward"):
        if half == "forward":
            new.reset_rhs(); old.reset_rhs()
        new.solve(info=dinfo, half=half)
        old.fixed_solve(info=dinfo, half=half)
        new.same_as(old, ("D", "E", "B"))
    assert np.array_equal(G.bits(new.flat["B"]), G.bits(full)), "forward then backward does not leave the bits of the full solve"
    factors = new.clone()
    for symmetric in (False, True):
        a, b = factors.clone(), factors.clone()
        a.inverse(info=dinfo, symmetric=symmetric)
        b.fixed_inverse(info=dinfo, symmetric=symmetric)
        a.same_as(b, ("D", "E"))
    return info, ld, factors, full


@pytest.mark.parametrize("row", RC.rows(), ids=ROW_ID)
def test_exact_family_bit_for_bit_and_exact(row):
    n, lengths, _, nrhs, _ = row
    new = G.Ragged(row, "exact")
    info, ld, factors, full = _walk(new, "exact")
    assert not info.any()
    Dv, Ev = factors.view("D").cpu().numpy(), factors.view("E").cpu().numpy()
    Bv = full.as_strided(*new.shapes["B"]).cpu().numpy()
    for c, T in enumerate(lengths):
        U, W, X, logdet = new.exact[c]
        f, r = new.first[c], new.rows_at[c]
        for i in range(T):
            assert np.array_equal(np.tril(Dv[f + i]), U[i].T.astype(np.float64)), (c, i)       # torch reads L = U^T
            if i + 1 < T:
                assert np.array_equal(Ev[f + i], W[i].T.astype(np.float64)), (c, i)
        assert np.array_equal(Bv[:, r * n:(r + T) * n], X.T.astype(np.float64)), c
        if T:
            np.testing.assert_allclose(ld[c], logdet, rtol=1e-13, atol=1e-12)
        else:
            assert ld[c] == 0.0


@pytest.mark.parametrize("row", [RC.ROWS[1], RC.ROWS[4], RC.ROWS[7], RC.ROWS[10]], ids=ROW_ID)
def test_random_family_bit_for_bit(row):
    info, _, _, _ = _walk(G.Ragged(row, "random"), "random")
    assert not info.any()


@pytest.mark.parametrize("row", [RC.ROWS[0], RC.ROWS[8]], ids=ROW_ID)
def test_the_entries_of_empty_chains_are_not_written(row):
    """the C entry on sentinel-filled info / logdet: batched.VarChains hands out zeros, so this goes to the library directly"""
    from capital_amd import _lib
    L = _lib.lib()
    new = G.Ragged(row, "exact")
    n, lengths = new.n, new.lengths
    info = torch.full((len(lengths),), 77, dtype=torch.int32, device=G.DEV)
    ld = torch.from_numpy(V.nan_pattern(len(lengths), salt=9)).to(G.DEV)
    before = ld.cpu().numpy().view(np.int64).copy()
    (_, (step, ldd, _)) = new.shapes["D"]
    st = L.cap_dpotrf_blocktri_vbatched(new.plan._plan, 1, n, new.flat["D"].data_ptr(), ldd, step, new.flat["E"].data_ptr(), ldd, step, info.data_ptr(),
                                        ld.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0
    got, gl = info.cpu().numpy(), ld.cpu().numpy()
    for c, T in enumerate(lengths):
        if T:
            assert got[c] == 0 and np.isfinite(gl[c])
        else:
            assert got[c] == 77 and gl.view(np.int64)[c] == before[c]


@pytest.mark.parametrize("row", [RC.ROWS[1], RC.ROWS[5], RC.ROWS[6], RC.ROWS[8]], ids=ROW_ID)
def test_company_independence(row):
    """the batch permuted (other neighbours in the sorted list, other slots, other rows of B): every chain keeps its bits"""
    n, lengths = row[0], row[1]
    rng = np.random.default_rng(5)
    a = G.Ragged(row, "random")
    perm = [int(x) for x in rng.permutation(len(lengths))]
    b = G.Ragged(row, "random", batch_order=perm)
    outs = []
    for obj in (a, b):
        info, ld = obj.factor()
        obj.solve(info=torch.from_numpy(info).to(G.DEV))
        solved = obj.clone()
        obj.inverse(symmetric=True)
        outs.append((info, ld, solved, obj))
    for k, c in enumerate(perm):
        assert outs[0][0][c] == outs[1][0][k] and outs[0][1].view(np.int64)[c] == outs[1][1].view(np.int64)[k]
        for stage in (2, 3):
            for x, y in zip(outs[0][stage].chain_bits(c), outs[1][stage].chain_bits(k)):
                assert np.array_equal(x, y), (c, k, stage)


@pytest.mark.parametrize("row,chain,pos", [(RC.ROWS[0], 4, 2), (RC.ROWS[5], 1, 1), (RC.ROWS[10], 2, 1)], ids=["np8", "np16", "np64"])
def test_a_failing_chain_in_the_middle_of_a_wavefront(row, chain, pos):
    """one non-positive pivot at an inner position, shorter and longer neighbours around it: info is the row inside the chain's OWN
    system, NaN lands exactly where the fixed-size entry puts it, the neighbours' bits are those of the run without the failure; then the
    solve and the inverse with that info and with info = None"""
    n, lengths = row[0], row[1]
    new = G.Ragged(row, "exact", fail=(chain, pos))
    good = G.Ragged(row, "exact")
    info, ld, factors, full = _walk(new, "exact")
    assert info[chain] == pos * n + min(1, n - 1) + 1 and np.isnan(ld[chain])
    assert not np.delete(info, chain).any()
    ginfo, gld = good.factor()
    good.solve()
    cur = factors.clone()
    cur.flat["B"] = full
    for c in range(len(lengths)):
        if c != chain:
            assert ld.view(np.int64)[c] == gld.view(np.int64)[c]
            for x, y in zip(cur.chain_bits(c), good.chain_bits(c)):
                assert np.array_equal(x, y), c
    a, b = factors.clone(), factors.clone()          # info = None: the failed chain's NaN travels through the arithmetic, as in the fixed-size entries
    a.reset_rhs(); b.reset_rhs()
    a.solve(info=None); b.fixed_solve(info=None)
    a.inverse(info=None); b.fixed_inverse(info=None)
    a.same_as(b, ("D", "E", "B"))


@pytest.mark.parametrize("row", [RC.ROWS[11], RC.ROWS[12]], ids=ROW_ID)
def test_equal_lengths_give_the_bits_of_the_fixed_size_entry_on_the_whole_batch(row):
    from capital_amd import batched
    n, lengths, _, nrhs, _ = row
    T, batch = lengths[0], len(lengths)
    new = G.Ragged(row, "random")
    old = new.clone()
    info, ld = new.factor()
    D4 = old.view("D")[:batch * T].unflatten(0, (batch, T))
    E4 = old.view("E")[:batch * T].unflatten(0, (batch, T))[:, :T - 1]
    B3 = old.view("B").unflatten(1, (batch, T * n)).transpose(0, 1).contiguous()      # (the stacked layout is not a fixed-size operand: a copy)
    info0, ld0 = batched.blocktri_potrf(D4, E4, logdet=True)
    torch.cuda.synchronize()
    new.same_as(old, ("D", "E"))
    assert np.array_equal(info, info0.cpu().numpy()) and np.array_equal(ld.view(np.int64), G.bits(ld0))
    new.solve(info=info0)
    batched.blocktri_potrs(D4, E4, B3, info=info0)
    torch.cuda.synchronize()
    assert np.array_equal(G.bits(new.view("B").unflatten(1, (batch, T * n)).transpose(0, 1).contiguous()), G.bits(B3))
    new.inverse(info=info0, symmetric=True)
    batched.blocktri_potri(D4, E4, info=info0, symmetric=True)
    torch.cuda.synchronize()
    new.same_as(old, ("D", "E"))
