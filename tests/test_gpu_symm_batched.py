"""-m gpu: cap_dsymm_batched, cap_dlansy_batched, cap_dpocon_batched and cap_dpoerr_batched (csrc/symm_batched.hip) on an MI355X.
(a) exact rows of tests/symm_batched_cases.py, bit for bit (no tolerance; NaN in everything the call must not read or write, still there
afterwards; beta == 0 with NaN in B; alpha == 0 with NULL A / X; in place), (b) norm1: exact on integer blocks, NaN in the upper triangle
seen, NaN in the lower one not, (c) CONTRACTS 2 - 4: a block alone against the same block in a batch, at another index, with other leading
dimensions and strides; a column alone against the same column among others and in another pass; the fused modes against the public entries,
(d) rcond: exact on the dyadic factor families, against cond_1 in np.longdouble on random blocks, failed blocks, anorm 0 / NaN, (e)
error_bounds: berr exact on integer data, ferr against NumPy on the exact families, the bound that matters - the true error of a solve with
a known integer solution is below ferr, with no tolerance - x_j = 0, a failed block, berr alone, (f) the Python layer.
(CONTRACT 1: tests/test_gpu_symm_vbatched.py.)"""
import numpy as np
import pytest
import torch

from tests import potri_batched_cases as P
from tests import symm_batched_cases as SC
from tests import symm_batched_gpu as G
from tests.tri_cases import positive_zero

pytestmark = pytest.mark.gpu

BOTH = (7, 8, 16, 33, 64, 65, 130, 256)           # every NP, both paths


def real(n, nrhs, seed):
    rng = np.random.default_rng([733, n, nrhs, seed])
    A = rng.standard_normal((n, n))
    return A + A.T, rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))


# ---- (a) exact rows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SC.exact_rows(), ids=SC.row_id)
def test_exact_rows_bit_for_bit(row):
    n, nrhs, batch, absolute, (alpha, beta), la, lx, inplace = row
    ops = [SC.operands(n, nrhs, i % 7) for i in range(batch)]
    for A, X, B in ops[:7]:
        assert SC.premise(A, X, B, alpha, beta) < SC.LIMIT                       # every summation order gives these bits
    out = G.symm([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops], alpha, beta, absolute, la, lx, inplace)
    for i, (o, got) in enumerate(zip(ops, out)):
        assert G.same(positive_zero(got), positive_zero(SC.expected(o[0], o[1], o[2], alpha, beta, absolute))), "block %d" % i


@pytest.mark.parametrize("n", (8, 130))
def test_alpha_zero_never_addresses_a_or_x(n):
    ops = [SC.operands(n, 5, i) for i in range(3)]
    out = G.symm([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops], 0.0, 2.0, 0, null_ax=True)
    for o, got in zip(ops, out):
        assert G.same(got, 2.0 * o[2] + 0.0)
    out = G.symm([o[0] for o in ops], [o[1] for o in ops], None, 0.0, 0.0, 1, null_ax=True)
    for got in out:
        assert G.same(got, np.zeros((n, 5)))


# ---- (b) norm1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,la", [(n, SC.WAVE_BATCHES[k % 4], SC.LAYOUTS[k % 4]) for k, n in enumerate(SC.WAVE_N)] +
                         [(n, SC.GROUP_BATCHES[k % 3], SC.LAYOUTS[(k + 1) % 4]) for k, n in enumerate(SC.GROUP_N)])
def test_norm1_exact_and_nan(n, batch, la):
    As = [SC.operands(n, 1, i % 7)[0] for i in range(batch)]
    got = G.norm(As, la)
    assert G.same(got, np.array([SC.norm1(A) for A in As]))
    up = [np.array(A) for A in As]
    r = n // 2
    up[batch // 2][r // 2, r] = np.nan                                           # a NaN in the upper triangle: that block, no other
    got = G.norm(As, la, upper=up)
    for i, A in enumerate(As):
        assert np.isnan(got[i]) if i == batch // 2 else got[i] == SC.norm1(A)    # (the strictly lower triangles are NaN throughout)


# ---- (c) contracts 2 - 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOTH)
def test_layout_independence(n):
    nrhs, alpha, beta = 19, -0.75, 1.25
    blocks = [real(n, nrhs, s) for s in range(6)]
    alone = [G.symm([b[0]], [b[1]], [b[2]], alpha, beta)[0] for b in blocks[:3]]
    alone_n = [G.norm([b[0]])[0] for b in blocks[:3]]
    for la, lx, order in (((0, 0), (0, 0), (0, 1, 2, 3, 4, 5)), ((1, 3), (6, 0), (5, 4, 2, 1, 0, 3)), ((6, 0), (0, 3), (3, 0, 5, 1, 4, 2))):
        bl = [blocks[i] for i in order] * 3                                      # 18 blocks: more than one wavefront for every NP
        out = G.symm([b[0] for b in bl], [b[1] for b in bl], [b[2] for b in bl], alpha, beta, 0, la, lx)
        nm = G.norm([b[0] for b in bl], la)
        for pos, i in enumerate(list(order) * 3):
            if i < 3:
                assert G.same(out[pos], alone[i]) and G.same(nm[pos], alone_n[i]), "layouts %s %s, position %d" % (la, lx, pos)


@pytest.mark.parametrize("n", BOTH)
def test_column_independence(n):
    A, X, B = real(n, 35, 1)
    whole = G.symm([A], [X], [B], 1.5, -0.5)[0]
    wabs = G.symm([A], [X], [B], 1.0, 1.0, 1)[0]
    for j in (0, 15, 16, 34):                                                    # the first and the last pass, both edges of a pass
        assert G.same(G.symm([A], [X[:, j:j + 1]], [B[:, j:j + 1]], 1.5, -0.5)[0][:, 0], whole[:, j]), "column %d alone" % j
        assert G.same(G.symm([A], [X[:, j:j + 1]], [B[:, j:j + 1]], 1.0, 1.0, 1)[0][:, 0], wabs[:, j]), "column %d alone, absolute" % j
    part = G.symm([A], [X[:, 14:20]], [B[:, 14:20]], 1.5, -0.5)[0]               # columns that change their pass and their place in it
    assert G.same(part, whole[:, 14:20])


@pytest.mark.parametrize("n", BOTH)
def test_composition_of_the_fused_modes(n):
    batch, nrhs = 3, 18
    rng = np.random.default_rng([88, n])
    As = [P.random_spd(n, 1e3, 1, seed=i)[0] for i in range(batch)]
    Xs = [rng.standard_normal((n, nrhs)) for _ in range(batch)]
    Bs = [A @ x * (1 + 1e-13 * rng.standard_normal((n, nrhs))) for A, x in zip(As, Xs)]          # a small nonzero residual
    ones = [np.ones((n, 1)) for _ in range(batch)]
    # norm1 = max of symm(absolute) against ones
    col = G.symm(As, ones, None, 1.0, 0.0, 1)
    anorm = G.norm(As)
    assert G.same(anorm, np.array([c.max() for c in col]))
    # rcond = 1 / (anorm * norm1(potri(copy of R)))
    Rs = G.factor(As)
    inv = G.potri(Rs)
    ainv = G.norm(inv)
    assert G.same(G.rcond(Rs, anorm), 1.0 / (anorm * ainv))
    # berr and ferr from symm's r, s and |A^-1| w
    r = G.symm(As, Xs, Bs, -1.0, 1.0)
    s = G.symm(As, Xs, Bs, 1.0, 1.0, 1)
    w = [SC.weights(ri, si, n) for ri, si in zip(r, s)]
    y = G.symm(inv, w, None, 1.0, 0.0, 1)
    fe, be = G.poerr(As, Rs, Bs, Xs, pad=3)
    for i in range(batch):
        assert G.same(be[i], SC.berr(r[i], s[i], n)), "berr of block %d" % i
        assert G.same(fe[i], SC.ferr(y[i], Xs[i])), "ferr of block %d" % i
    # a column's bounds do not depend on the columns that travel with it
    fe1, be1 = G.poerr(As, Rs, [b[:, 16:17] for b in Bs], [x[:, 16:17] for x in Xs])
    assert G.same(fe1[:, 0], fe[:, 16]) and G.same(be1[:, 0], be[:, 16])
    # layout independence of the diagnostics
    fe2, be2 = G.poerr(As[::-1], Rs[::-1], Bs[::-1], Xs[::-1], la=(1, 3), lx=(6, 0))
    assert G.same(fe2[::-1], fe) and G.same(be2[::-1], be)
    assert G.same(G.rcond(Rs[::-1], anorm[::-1], lr=(6, 5))[::-1], G.rcond(Rs, anorm))


# ---- (d) rcond ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fam,batch", [(n, P.FAMILIES[k % 3], (1, 3, 65)[k % 3]) for k, n in enumerate((1, 2, 7, 8, 9, 16, 17, 33, 63, 64))] +
                         [(n, P.FAMILIES[k % 3], (1, 5)[k % 2]) for k, n in enumerate((65, 96, 129, 200, 255, 256))])
def test_rcond_exact_on_the_dyadic_families(n, fam, batch):
    T, Ti, C = P.batch(fam, n, False, min(batch, 5))                             # block() asserted the exactness premise
    idx = [i % T.shape[0] for i in range(batch)]
    Rs = [T[i] for i in idx]
    anorm = np.array([SC.norm1(T[i].T @ T[i]) for i in idx])
    for i in set(idx):
        assert SC.sums_exact(SC.sym(C[i])) and SC.sums_exact(T[i].T @ T[i])          # the norms are exact in any summation order
    want = np.array([1.0 / (anorm[k] * SC.norm1(SC.sym(C[i]))) for k, i in enumerate(idx)])
    assert G.same(G.rcond(Rs, anorm, lr=P.LAYOUTS[n % 4]), want)


@pytest.mark.parametrize("n", (7, 33, 64, 65, 130, 256))
def test_rcond_against_cond1_in_longdouble(n):
    """rcond * cond_1(A) within 1 +- 1e-6: the inverse's error bound is c n eps kappa, about 3e-10 c at n = 256 and kappa = 1e4"""
    As = [P.random_spd(n, k, 1, seed=3)[0] for k in (1e1, 1e2, 1e4)]
    As = [A for A in As if np.linalg.cond(A, 1) <= 1e4] or As[:1]
    Rs = G.factor(As)
    anorm = G.norm(As)
    got = G.rcond(Rs, anorm)
    for A, g in zip(As, got):
        Al = A.astype(np.longdouble)
        inv = np.linalg.inv(A).astype(np.longdouble)
        inv = inv + inv @ (np.eye(n, dtype=np.longdouble) - Al @ inv)            # one Newton step in extended precision
        inv = inv + inv @ (np.eye(n, dtype=np.longdouble) - Al @ inv)
        cond = np.abs(Al).sum(axis=0).max() * np.abs(inv).sum(axis=0).max()
        assert abs(float(np.longdouble(g) * cond) - 1.0) <= 1e-6, (n, float(g), float(cond))


@pytest.mark.parametrize("n", (8, 130))
def test_rcond_failed_blocks_and_special_norms(n):
    As = [P.random_spd(n, 1e2, 1, seed=i)[0] for i in range(5)]
    Rs = G.factor(As)
    anorm = G.norm(As)
    base = G.rcond(Rs, anorm)
    info = np.array([0, 3, 0, 0, 0], dtype=np.int32)
    an = anorm.copy()
    an[2], an[3] = 0.0, np.nan
    got = G.rcond(Rs, an, info)
    assert G.same(got[[0, 4]], base[[0, 4]]) and np.isnan(got[1]) and got[2] == 0.0 and np.isnan(got[3])


# ---- (e) error bounds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nrhs,batch", ((1, 1, 3), (7, 3, 65), (8, 17, 3), (16, 16, 1), (17, 33, 3), (33, 1, 257), (63, 3, 3), (64, 17, 1),
                                          (65, 3, 5), (96, 16, 1), (129, 17, 1), (200, 33, 1), (255, 1, 5), (256, 3, 33)))
def test_berr_exact_on_integer_data(n, nrhs, batch):
    """integer A, X, B with a nonzero residual: r and s are exact, berr is the guarded quotient of exact values - and berr alone (ferr NULL)
    needs no factor"""
    ops = [SC.operands(n, nrhs, i % 5) for i in range(batch)]
    As, Xs, Bs = ([o[k] for o in ops] for k in range(3))
    fe, be = G.poerr(As, As, Bs, Xs, want_ferr=False, la=P.LAYOUTS[n % 4], lx=P.LAYOUTS[(n + 1) % 4], pad=1)
    assert fe is None
    for i, (A, X, B) in enumerate(ops):
        assert SC.premise(A, X, B, 1.0, 1.0) < SC.LIMIT
        assert G.same(be[i], SC.berr(B - A @ X, np.abs(A) @ np.abs(X) + np.abs(B), n)), "block %d" % i


@pytest.mark.parametrize("n,fam", [(n, P.FAMILIES[k % 3]) for k, n in enumerate((1, 7, 8, 9, 16, 17, 33, 63, 64, 65, 96, 129, 200, 255, 256))])
def test_ferr_on_the_exact_families(n, fam):
    """A = T^T T and A^-1 are exact dyadics, X and B integers with a nonzero residual: w has identical bits, the sums |A^-1| w are of
    non-negative terms, so any summation order stays within 2 (n + 2) 2^-52 relative of NumPy's value"""
    nrhs = 5
    T, Ti, C = P.batch(fam, n, False, 3)
    As = [T[i].T @ T[i] for i in range(3)]
    rng = np.random.default_rng([61, n])
    Xs = [rng.integers(-4, 5, size=(n, nrhs)).astype(np.float64) for _ in range(3)]
    for x in Xs:
        x[:, 2] = 0.0                                                            # x_j = 0: the numerator alone
    Bs = [rng.integers(-4, 5, size=(n, nrhs)).astype(np.float64) for _ in range(3)]
    fe, be = G.poerr(As, [T[i] for i in range(3)], Bs, Xs)
    for i in range(3):
        r, s = Bs[i] - As[i] @ Xs[i], np.abs(As[i]) @ np.abs(Xs[i]) + np.abs(Bs[i])
        assert np.abs(As[i]).sum(axis=1).max() * 8 * 16 < SC.LIMIT               # r and s are exact
        assert G.same(be[i], SC.berr(r, s, n))
        want = SC.ferr(np.abs(SC.sym(C[i])) @ SC.weights(r, s, n), Xs[i])
        assert np.all(np.abs(fe[i] - want) <= 2 * (n + 2) * 2.0 ** -52 * want), (i, fe[i], want)
        assert np.isfinite(fe[i]).all()


@pytest.mark.parametrize("n,batch", ((7, 65), (8, 3), (16, 3), (33, 5), (64, 3), (65, 3), (129, 2), (256, 2)))
def test_the_true_error_is_below_ferr(n, batch):
    """integer SPD A = M M^T + I and an integer x*: B = A x* is exact and x* is known.  Factor and solve with the batched entries; then
    |X - x*|_inf / |X|_inf <= ferr for every block and column, with no tolerance."""
    from capital_amd import batched
    nrhs = 3
    sysm = [SC.spd_system(n, nrhs, i % 4) for i in range(batch)]
    A = torch.from_numpy(np.ascontiguousarray(np.stack([s[0] for s in sysm]))).to(G.DEV)
    B = torch.from_numpy(np.ascontiguousarray(np.stack([s[2].T for s in sysm]))).to(G.DEV)
    R, A0, B0 = A.clone(), A.clone(), B.clone()
    info = batched.potrf(R)
    X = batched.potrs(R, B.clone(), info)
    R0, X0 = R.clone(), X.clone()
    fe, be = batched.error_bounds(A, R, B, X, info)
    assert not info.cpu().numpy().any()
    assert torch.equal(A, A0) and torch.equal(B, B0) and torch.equal(R, R0) and torch.equal(X, X0)
    Xh, fe, be = X.cpu().numpy(), fe.cpu().numpy(), be.cpu().numpy()
    xs = np.stack([s[1].T for s in sysm])
    err = np.abs(Xh - xs).max(axis=2) / np.abs(Xh).max(axis=2)
    assert np.all(err <= fe), (err.max(), fe.min())
    assert np.isfinite(be).all()


@pytest.mark.parametrize("n", (8, 130))
def test_a_failed_block_does_not_disturb_its_neighbours(n):
    nrhs = 4
    As = [P.random_spd(n, 1e2, 1, seed=i)[0] for i in range(5)]
    rng = np.random.default_rng([5, n])
    Xs = [rng.standard_normal((n, nrhs)) for _ in range(5)]
    Bs = [A @ x for A, x in zip(As, Xs)]
    Rs = G.factor(As)
    fe0, be0 = G.poerr(As, Rs, Bs, Xs)
    info = np.array([0, 0, 2, 0, 0], dtype=np.int32)
    fe, be = G.poerr(As, Rs, Bs, Xs, info)
    keep = [0, 1, 3, 4]
    assert G.same(fe[keep], fe0[keep]) and G.same(be[keep], be0[keep])
    assert np.isnan(fe[2]).all() and np.isnan(be[2]).all()
    fe1, be1 = G.poerr(As, Rs, Bs, Xs, info, want_ferr=False)
    assert fe1 is None and G.same(be1[keep], be0[keep]) and np.isnan(be1[2]).all()
    fe2, be2 = G.poerr(As, Rs, Bs, Xs, info, want_berr=False)
    assert be2 is None and G.same(fe2[keep], fe0[keep]) and np.isnan(fe2[2]).all()


# ---- (f) the Python layer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (5, 100))
def test_python_layer_matches_the_c_entries(n):
    from capital_amd import batched
    batch, nrhs = 4, 3
    blocks = [real(n, nrhs, s) for s in range(batch)]
    spd = [P.random_spd(n, 1e2, 1, seed=s)[0] for s in range(batch)]
    buf = torch.full((batch, n + 2, n + 1), float("nan"), dtype=torch.float64, device=G.DEV)
    A = buf[:, :n, :n]                                                           # stride(1) = n + 1: torch's rows are the columns
    A.copy_(torch.from_numpy(np.stack([np.tril(b[0]) for b in blocks])))
    A[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = float("nan")       # what torch reads as the strictly upper triangle
    X = torch.from_numpy(np.ascontiguousarray(np.stack([b[1].T for b in blocks]))).to(G.DEV)
    B = torch.from_numpy(np.ascontiguousarray(np.stack([b[2].T for b in blocks]))).to(G.DEV)
    want = G.symm([b[0] for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks], 2.0, -1.0)
    got = batched.symm(A, X, B, alpha=2.0, beta=-1.0)
    assert all(G.same(got[i].cpu().numpy().T, want[i]) for i in range(batch))
    assert G.same(batched.symm(A, X[:, 0], B[:, 0], alpha=2.0, beta=-1.0).cpu().numpy(), got[:, 0].cpu().numpy())
    assert batched.symm(A, X, B, alpha=2.0, beta=-1.0, out=B) is B and torch.equal(B, got)
    assert G.same(batched.norm1(A).cpu().numpy(), G.norm([b[0] for b in blocks]))
    S = torch.from_numpy(np.stack(spd)).to(G.DEV)
    R = S.clone()
    an = batched.norm1(S)
    info = batched.potrf(R)
    R0 = R.clone()
    Rs = [np.triu(R[i].cpu().numpy().T) for i in range(batch)]
    assert G.same(batched.rcond(R, an, info).cpu().numpy(), G.rcond(Rs, an.cpu().numpy()))
    Bs = torch.from_numpy(np.ascontiguousarray(np.stack([b[2].T for b in blocks]))).to(G.DEV)
    Xs = batched.potrs(R, Bs.clone(), info)
    fe, be = batched.error_bounds(S, R, Bs, Xs, info)
    wf, wb = G.poerr(spd, Rs, [b[2] for b in blocks], [Xs[i].cpu().numpy().T for i in range(batch)])
    assert G.same(fe.cpu().numpy(), wf) and G.same(be.cpu().numpy(), wb)
    f1, b1 = batched.error_bounds(S, R, Bs[:, 1], Xs[:, 1], info, ferr=False)
    assert f1 is None and b1.shape == (batch,) and G.same(b1.cpu().numpy(), wb[:, 1])
    assert torch.equal(R, R0)
    empty = torch.zeros((3, 0, 0), dtype=torch.float64, device=G.DEV)
    assert batched.norm1(empty).tolist() == [0.0, 0.0, 0.0] and batched.rcond(empty, batched.norm1(empty)).tolist() == [0.0, 0.0, 0.0]
