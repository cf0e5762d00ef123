"""-m gpu: the batched block-tridiagonal Cholesky factor and solve (batched.blocktri_potrf / blocktri_potrs, cap_dpotrf_blocktri_batched /
cap_dpotrs_blocktri_batched, csrc/blocktri_batched.hip) on an MI355X, over the rows of tests/blocktri_cases.py on NaN-guarded strided
buffers (tests/blocktri_gpu.py asserts after every call that nothing outside the blocks was written and that the solve left D and E alone).
1. COMPOSITION: every row on random SPD chains, bit for bit (NaN equal to NaN by position) against the host-driven loop over
   batched.potrf / trsm / syrk (schur) / gemm on views of a copy: D, E, info, logdet, both half sweeps, the full solve; "forward" then
   "backward" has the bits of the full solve.
2. EXACT: chains whose every intermediate is a small integer (tests/test_blocktri_cases.py proves it): the factor equals R and the
   solution equals X with no tolerance.
3. INDEPENDENCE: a chain alone against the same chain first, in the middle and last of a ragged batch under another layout; a column
   alone against the column among 17.
4. FAILURE: a good chain, a zero pivot at position 2, a NaN in D_0 and a failure at the last position side by side in one wavefront.
5. BOUND: |A - L L^T| <= gamma_(2n+2) |L| |L|^T componentwise (Higham: inner products of at most 2 n terms, any summation order), the
   residual evaluated in extended precision on the CPU from the device result.
6. PYTHON: torch.equal with torch.linalg.cholesky of the assembled matrix on the exact family, and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import blocktri_cases as BC  # noqa: E402
from tests import blocktri_gpu as G  # noqa: E402

ROWS = BC.rows()
IDS = ["n%d-T%d-b%d-k%d-%s" % r for r in ROWS]
U = 2.0 ** -53


def sw(a):
    return np.swapaxes(a, -1, -2)


def cpu(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_composition_bit_for_bit(row):
    D, Bc, rhs = BC.random_chain(row)
    new = G.Chains(row, D, Bc, rhs)
    old = new.clone()
    info, ld = new.factor()
    info0, ld0 = old.compose_factor()
    assert np.array_equal(cpu(info), cpu(info0)) and not cpu(info).any()
    assert G.same(cpu(ld), cpu(ld0))
    assert G.same(new.host("D"), old.host("D"))
    if row[1] > 1:
        assert G.same(new.host("E"), old.host("E"))
    factored = new.snapshot()
    results = {}
    for half in (None, "forward", "backward"):
        a, b = new.clone(), old.clone()
        a.solve(info=info, half=half)
        b.compose_solve(info=info0, half=half)
        assert G.same(a.host("B"), b.host("B")), half
        a.unchanged_since(factored, ("D", "E"))
        results[half] = a
    both = results["forward"]
    both.solve(info=info, half="backward")
    assert G.same(both.host("B"), results[None].host("B"))
    # and it is a solution: the residual of the assembled system is small
    A = BC.dense(D, Bc)
    X = sw(results[None].host("B"))
    assert np.abs(A @ X - rhs).max() <= 1e-10 * np.abs(rhs).max() * (3 * row[0] + 2)


@pytest.mark.parametrize("row", BC.exact_rows(), ids=IDS)
def test_exact_family_factor_is_R_and_solution_is_X(row):
    D, Bc, X, rhs, Uf, W, logdet = BC.exact_chain(row)
    c = G.Chains(row, D, Bc, rhs)
    info, ld = c.factor()
    assert not cpu(info).any()
    assert np.array_equal(c.host("D"), sw(Uf).astype(np.float64))
    if row[1] > 1:
        assert np.array_equal(c.host("E"), sw(W).astype(np.float64))
    np.testing.assert_allclose(cpu(ld), logdet, rtol=1e-13, atol=1e-12)
    fwd = c.clone()
    c.solve(info=info)
    assert np.array_equal(c.host("B"), sw(X).astype(np.float64))
    fwd.solve(half="forward")                    # R^-T (A X) = R X, exact as well
    assert np.array_equal(sw(fwd.host("B")), (BC.dense_factor(Uf, W) @ X).astype(np.float64))
    fwd.solve(half="backward")
    assert np.array_equal(fwd.host("B"), sw(X).astype(np.float64))


@pytest.mark.parametrize("n,T", ((8, 3), (9, 2), (17, 3), (33, 2), (64, 2)))
def test_a_chain_does_not_depend_on_its_company_or_its_layout(n, T):
    Gp = 64 // BC.padded(n)
    batch = 2 * Gp + 1
    row = (n, T, batch, 17, "gaps")
    D, Bc, rhs = BC.random_chain(row)
    chosen = D[batch - 1].copy(), Bc[batch - 1].copy(), rhs[batch - 1].copy()
    alone = G.Chains((n, T, 1, 17, "packed"), chosen[0][None], chosen[1][None], chosen[2][None])
    info_a, ld_a = alone.factor()
    alone.solve(info=info_a)
    col = G.Chains((n, T, 1, 1, "packed"), chosen[0][None], chosen[1][None], chosen[2][None][:, :, 5:6])
    col.factor()
    col.solve()
    assert G.same(col.host("B")[0, 0], alone.host("B")[0, 5])
    for at in (0, batch // 2, batch - 1):
        Dm, Bm, rm = D.copy(), Bc.copy(), rhs.copy()
        Dm[[at, batch - 1]], Bm[[at, batch - 1]], rm[[at, batch - 1]] = Dm[[batch - 1, at]], Bm[[batch - 1, at]], rm[[batch - 1, at]]
        many = G.Chains(row, Dm, Bm, rm)
        info, ld = many.factor()
        many.solve(info=info)
        assert G.same(many.host("D")[at], alone.host("D")[0]) and G.same(many.host("B")[at], alone.host("B")[0])
        if T > 1:
            assert G.same(many.host("E")[at], alone.host("E")[0])
        assert G.same(cpu(ld)[at], cpu(ld_a)[0]) and cpu(info)[at] == 0


@pytest.mark.parametrize("n", (8, 9, 17))
def test_failures_stay_in_their_chain(n):
    T, batch, r = 4, 4, n // 2
    assert batch <= 64 // BC.padded(n) or n > 16      # n = 8, 9: the four chains share a wavefront
    row = (n, T, batch, 3, "ld")
    D, Bc, X, rhs, Uf, W, _ = BC.exact_chain(row)
    D = D.astype(np.float64)
    D[1, 2, r, r] -= float(Uf[1, 2, r, r]) ** 2       # the pivot of row r of position 2 becomes exactly zero
    D[2, 0, 1, 1] = np.nan
    D[3, T - 1, r, r] -= float(Uf[3, T - 1, r, r]) ** 2
    new = G.Chains(row, D, Bc, rhs)
    old = new.clone()
    info, ld = new.factor()
    info0, ld0 = old.compose_factor()
    want = np.array([0, 2 * n + r + 1, 2, (T - 1) * n + r + 1], dtype=np.int32)
    assert np.array_equal(cpu(info), want) and np.array_equal(cpu(info0), want)
    assert G.same(new.host("D"), old.host("D")) and G.same(new.host("E"), old.host("E")) and G.same(cpu(ld), cpu(ld0))
    assert np.isnan(cpu(ld)[1:]).all() and not np.isnan(cpu(ld)[0])
    Dh, Eh = new.host("D"), new.host("E")
    low = np.tril(np.ones((n, n), dtype=bool))
    assert np.array_equal(Dh[1, :2], sw(Uf[1, :2]).astype(np.float64)) and np.array_equal(Eh[1, :2], sw(W[1, :2]).astype(np.float64))
    assert np.array_equal(sw(Dh[1, 2])[:r], Uf[1, 2, :r].astype(np.float64)) and np.isnan(sw(Dh[1, 2])[r:, r:][np.triu(np.ones((n - r, n - r), dtype=bool))]).all()
    assert np.isnan(Eh[1, 2:]).all() and np.isnan(Dh[1, 3][low]).all()
    assert np.isnan(Eh[2]).all() and np.isnan(Dh[2, 1:][:, low]).all() and Dh[2, 0, 0, 0] == float(Uf[2, 0, 0, 0])
    assert np.array_equal(Dh[3, :T - 1], sw(Uf[3, :T - 1]).astype(np.float64)) and np.array_equal(Eh[3], sw(W[3]).astype(np.float64))
    # the good chain keeps the bits it has alone
    alone = G.Chains((n, T, 1, 3, "packed"), D[:1], Bc[:1], rhs[:1])
    ia, la = alone.factor()
    assert G.same(Dh[0], alone.host("D")[0]) and G.same(Eh[0], alone.host("E")[0]) and G.same(cpu(ld)[0], cpu(la)[0])
    new.solve(info=info)
    old.compose_solve(info=info0)
    Bh = new.host("B")
    assert G.same(Bh, old.host("B"))
    assert np.array_equal(Bh[0], sw(X[0]).astype(np.float64)) and np.isnan(Bh[1:]).all()
    alone.solve(info=ia)
    assert G.same(Bh[0], alone.host("B")[0])


def _gamma(m):
    return np.longdouble(m) * np.longdouble(U) / (1 - np.longdouble(m) * np.longdouble(U))


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_componentwise_backward_error_bound(row):
    assert np.finfo(np.longdouble).nmant >= 63, "the residual needs extended precision"
    n, T = row[0], row[1]
    D, Bc, _ = BC.random_chain(row)
    c = G.Chains(row, D, Bc)
    info, _ = c.factor()
    assert not cpu(info).any()
    Uh = sw(c.host("D")).astype(np.longdouble)                    # U_i, upper
    Wh = sw(c.host("E")).astype(np.longdouble) if T > 1 else np.zeros((row[2], 0, n, n), dtype=np.longdouble)
    g = _gamma(2 * n + 2)
    worst = np.longdouble(0)
    for i in range(T):
        prod, mag = sw(Uh[:, i]) @ Uh[:, i], sw(np.abs(Uh[:, i])) @ np.abs(Uh[:, i])
        if i > 0:
            prod, mag = prod + sw(Wh[:, i - 1]) @ Wh[:, i - 1], mag + sw(np.abs(Wh[:, i - 1])) @ np.abs(Wh[:, i - 1])
        res = np.abs(D[:, i].astype(np.longdouble) - prod)
        print("row", row, "position", i, "diagonal block: max |A - LL^T| / (gamma |L||L|^T) =", float((res / (g * mag)).max()))
        worst = max(worst, (res / (g * mag)).max())
        assert (res <= g * mag).all()
        if i + 1 < T:
            res = np.abs(Bc[:, i].astype(np.longdouble) - sw(Uh[:, i]) @ Wh[:, i])
            mag = sw(np.abs(Uh[:, i])) @ np.abs(Wh[:, i])
            worst = max(worst, (res / (g * mag)).max())
            assert (res <= g * mag).all()
    assert worst > 0


def test_python_layer_matches_torch_cholesky_and_refuses_what_it_cannot_do():
    from capital_amd import _lib, batched
    row = (9, 3, 5, 3, "packed")
    D, Bc, X, rhs, Uf, W, _ = BC.exact_chain(row)
    A = torch.from_numpy(BC.dense(D, Bc).astype(np.float64)).to(G.DEV)
    Dt = torch.from_numpy(D.astype(np.float64)).to(G.DEV)
    Et = torch.from_numpy(np.ascontiguousarray(sw(Bc)).astype(np.float64)).to(G.DEV)
    Bt = torch.from_numpy(np.ascontiguousarray(sw(rhs)).astype(np.float64)).to(G.DEV)
    info, ld = batched.blocktri_potrf(Dt, Et, logdet=True)
    L = torch.linalg.cholesky(A)
    n, T = row[0], row[1]
    for i in range(T):
        assert torch.equal(torch.tril(Dt[:, i]), L[:, i * n:(i + 1) * n, i * n:(i + 1) * n])
        if i + 1 < T:
            assert torch.equal(Et[:, i], L[:, (i + 1) * n:(i + 2) * n, i * n:(i + 1) * n])
    assert not info.cpu().numpy().any() and torch.allclose(ld, torch.logdet(A), rtol=1e-12)
    assert batched.blocktri_potrs(Dt, Et, Bt, info=info) is Bt
    assert torch.equal(Bt, torch.from_numpy(np.ascontiguousarray(sw(X)).astype(np.float64)).to(G.DEV))
    one = batched.blocktri_potrs(Dt, Et, Bt[:, 0].clone())          # (batch, T n)
    assert one.shape == (5, 27)
    # T = 1 without E is potrf
    D1 = torch.from_numpy(D[:, :1].astype(np.float64)).to(G.DEV)
    D2 = D1[:, 0].clone()
    assert not batched.blocktri_potrf(D1, None).cpu().numpy().any() and not batched.potrf(D2).cpu().numpy().any()
    assert torch.equal(torch.tril(D1[:, 0]), torch.tril(D2))
    bad = (lambda: batched.blocktri_potrf(Dt.cpu(), Et.cpu()), lambda: batched.blocktri_potrf(Dt.float(), Et.float()),
           lambda: batched.blocktri_potrf(Dt, None), lambda: batched.blocktri_potrf(Dt, Et[:, :1]), lambda: batched.blocktri_potrf(Dt[:, 0], Et),
           lambda: batched.blocktri_potrf(Dt.as_strided((5, 3, 9, 9), (0, 81, 9, 1)), Et),
           lambda: batched.blocktri_potrf(torch.zeros(2, 2, 65, 65, dtype=torch.float64, device=G.DEV), torch.zeros(2, 1, 65, 65, dtype=torch.float64, device=G.DEV)),
           lambda: batched.blocktri_potrs(Dt, Et, Bt, half="both"), lambda: batched.blocktri_potrs(Dt, Et, Bt[:, :, :26]),
           lambda: batched.blocktri_potrs(Dt, Et, Bt.cpu()), lambda: batched.blocktri_potrs(Dt, Et, Dt.view(5, 9, 27)))
    for f in bad:
        with pytest.raises(_lib.CapitalError):
            f()
