"""-m gpu: the batched block-tridiagonal selected inverse (batched.blocktri_potri, cap_dpotri_blocktri_batched,
csrc/blocktri_potri_batched.hip) on an MI355X, over the rows of tests/blocktri_potri_cases.py on NaN-guarded strided buffers
(tests/blocktri_potri_gpu.py asserts after every call that nothing outside what the call may write was written).
1. COMPOSITION: every row on random chains factored by blocktri_potrf, bit for bit (NaN equal to NaN by position) against the
   host-driven loop over batched.trsm / potri / gemm on a scratch copy; fill = 0 compares the triangle and the other triangle keeps its
   NaN sentinels, fill = 1 compares the whole block with the mirror of that triangle.
2. EXACT: chains on which no sum can round (tests/test_blocktri_potri_cases.py proves it): the results equal Sigma_(i,i) and
   Sigma_(i,i+1) from the closed forms with no tolerance.
3. INDEPENDENCE: a chain alone, first, in the middle and last of a ragged batch, in every layout, with and without fill: the same bits.
4. FAILURE: chains whose info != 0 comes from a real failed blocktri_potrf get NaN in exactly what the call writes; their wavefront
   neighbours have the bits of a run without them; info=None is accepted.
5. ACCURACY on the random family: max |S - S*| / max |S*| per chain, S* the recurrence in np.longdouble from the same factor, is at most
   8 x the error of a NumPy fp64 evaluation of that recurrence and n 2^-53 where that is larger.  The two fp64 evaluations differ in the
   order of their sums only, so their errors are of one order but not equal: three bits of margin.  Both errors are printed per row.
6. PYTHON: blocktri_potrf then blocktri_potri against the tridiagonal blocks of torch.linalg.inv of the assembled matrix, and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import blocktri_cases as BC  # noqa: E402
from tests import blocktri_potri_cases as IC  # noqa: E402
from tests import blocktri_potri_gpu as P  # noqa: E402

ROWS = IC.rows()
U53 = 2.0 ** -53
sw = P.sw


@pytest.fixture(scope="module")
def factored():
    """the random family: every row's chains factored on the device ONCE, shared and left unchanged"""
    cache = {}

    def get(row):
        if row not in cache:
            U, W, info = P.from_device_factor(row)
            assert not info.cpu().numpy().any()
            U.setflags(write=False)
            W.setflags(write=False)
            cache[row] = (U, W)
        return cache[row]
    return get


def _check(row, new, Sd, Sc, same=P.same):
    """the call's D and E against (Sd, Sc) in torch's reading, Sd full mirrored blocks; same: bit for bit, or - against closed forms, whose
    zeros carry no sign - equal as numbers"""
    n, T, batch, fill, _ = row
    Dn, En = new.result()
    assert same(Dn, Sd if fill else np.tril(Sd))
    if fill:
        assert P.same(Dn, sw(Dn))                                     # the mirror is bit-identical
    if T > 1:
        assert same(En, Sc)


@pytest.mark.parametrize("row", ROWS, ids=IC.row_id)
def test_composition_bit_for_bit(row, factored):
    U, W = factored(row)
    new = P.Factors(row, U, W)
    old = new.clone()
    new.potri()
    Sd, Sc = old.compose()
    assert np.isfinite(Sd).all()
    _check(row, new, Sd, Sc)


@pytest.mark.parametrize("row,fam", IC.exact_rows(), ids=lambda v: IC.row_id(v) if isinstance(v, tuple) else v)
def test_exact_family_equals_the_closed_forms(row, fam):
    U, W, Sd, Sc, _ = IC.exact_chain(row, fam)
    new = P.Factors(row, U, W).potri()
    _check(row, new, Sd, sw(Sc), same=np.array_equal)                 # Sd is symmetric; E[c, i] = C_i^T in torch's reading; -0.0 == +0.0


@pytest.mark.parametrize("n,T", ((8, 3), (9, 2), (17, 3), (33, 2), (64, 3)))
def test_a_chain_does_not_depend_on_its_company_its_layout_or_fill(n, T, factored):
    Gp = 64 // BC.padded(n)
    batch = 2 * Gp + 1
    U, W = factored((n, T, batch, 0, "gaps"))
    alone = P.Factors((n, T, 1, 0, "packed"), U[-1:], W[-1:]).potri()
    Da, Ea = alone.result()
    k = 0
    for at in (0, batch // 2, batch - 1):
        Um, Wm = U.copy(), W.copy()
        Um[[at, batch - 1]], Wm[[at, batch - 1]] = Um[[batch - 1, at]], Wm[[batch - 1, at]]
        for lay in BC.LAYOUTS if at == batch // 2 else (BC.LAYOUTS[k % 4],):
            for fill in (0, 1):
                many = P.Factors((n, T, batch, fill, lay), Um, Wm).potri()
                Dm, Em = many.result()
                assert P.same(np.tril(Dm[at]), Da[0]) and P.same(Em[at], Ea[0]), (at, lay, fill)
                if fill:
                    assert P.same(Dm[at], sw(Dm[at]))
        k += 1


@pytest.mark.parametrize("n,fill", ((8, 0), (9, 1), (17, 0)))
def test_failed_chains_get_nan_and_their_neighbours_keep_their_bits(n, fill):
    from tests import blocktri_gpu as G
    T, batch, r = 4, 4, n // 2
    crow = (n, T, batch, 3, "ld")
    D, Bc, _, _, Uf, _, _ = BC.exact_chain(crow)
    D = D.astype(np.float64)
    D[1, 2, r, r] -= float(Uf[1, 2, r, r]) ** 2                       # a zero pivot at position 2
    D[3, T - 1, r, r] -= float(Uf[3, T - 1, r, r]) ** 2               # and one at the last position
    c = G.Chains(crow, D, Bc)
    info, _ = c.factor()
    assert np.array_equal(info.cpu().numpy() != 0, [False, True, False, True])
    U, W = sw(c.host("D")), sw(c.host("E"))                           # the factor as the failed call left it, NaN included
    row = (n, T, batch, fill, "ld")
    new = P.Factors(row, U, W).potri(info=info)
    Dn, En = new.result()
    low = np.ones((n, n), dtype=bool) if fill else np.tril(np.ones((n, n), dtype=bool))
    for bad in (1, 3):
        assert np.isnan(Dn[bad][:, low]).all() and np.isnan(En[bad]).all()
    good = P.Factors((n, T, 2, fill, "packed"), U[[0, 2]], W[[0, 2]]).potri()          # a run without them, info=None
    Dg, Eg = good.result()
    assert np.isfinite(Dg[:, :, low]).all() and np.isfinite(Eg).all()
    assert P.same(Dn[[0, 2]], Dg) and P.same(En[[0, 2]], Eg)
    old = P.Factors(row, U, W)
    Sd, Sc = old.compose(info=info)
    _check(row, new, Sd, Sc)


def _errors(U, W, Dn, En):
    """per chain: (the call's error, the NumPy fp64 evaluation's error), max |S - S*| / max |S*| over the band"""
    out = []
    for c in range(U.shape[0]):
        Sd, Sc = IC.reference(U[c], W[c], np.longdouble)
        Fd, Fc = IC.reference(U[c], W[c], np.float64)
        Hd = np.tril(Dn[c]) + sw(np.tril(Dn[c], -1))                  # the call's triangle, mirrored
        top = max(np.abs(Sd).max(), np.abs(Sc).max() if Sc.size else 0)
        e_gpu = max(np.abs(Hd - Sd).max(), np.abs(sw(En[c]) - Sc).max() if Sc.size else 0) / top
        e_np = max(np.abs(Fd - Sd).max(), np.abs(Fc - Sc).max() if Sc.size else 0) / top
        out.append((float(e_gpu), float(e_np)))
    return out


@pytest.mark.parametrize("row", ROWS, ids=IC.row_id)
def test_accuracy_against_the_recurrence_in_extended_precision(row, factored):
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs extended precision"
    n, T = row[0], row[1]
    U, W = factored(row)
    new = P.Factors(row, U, W).potri()
    Dn, En = new.result()
    if En is None:
        En = np.zeros((row[2], 0, n, n))
    errs = _errors(U, W, Dn, En)
    e_gpu, e_np = max(e[0] for e in errs), max(e[1] for e in errs)
    print("ACCURACY %s: kernel %.3e  numpy fp64 %.3e  (units of 2^-53: %.1f / %.1f)" % (IC.row_id(row), e_gpu, e_np, e_gpu / U53, e_np / U53))
    for g, f in errs:
        assert g <= max(8 * f, n * U53), (g, f)


def test_python_layer_matches_torch_inv_and_refuses_what_it_cannot_do():
    from capital_amd import _lib, batched
    n, T, batch = 9, 3, 5
    D, Bc, _ = BC.random_chain((n, T, batch, 1, "packed"))
    A = torch.from_numpy(BC.dense(D, Bc)).to(P.DEV)
    Dt = torch.from_numpy(D.copy()).to(P.DEV)
    Et = torch.from_numpy(np.ascontiguousarray(sw(Bc))).to(P.DEV)
    info = batched.blocktri_potrf(Dt, Et)
    out = batched.blocktri_potri(Dt, Et, info=info, symmetric=True)
    assert out[0] is Dt and out[1] is Et
    X = torch.linalg.inv(A)
    # the chains are diagonally dominant (eigenvalues in [1.5, 55.5]: condition number below 37), T n = 27: each route is within about
    # 27 x 37 x 2^-53 = 1.1e-13 of the inverse, relative to its largest entry
    tol = 1e-12 * float(X.abs().max())
    for i in range(T):
        assert torch.allclose(Dt[:, i], X[:, i * n:(i + 1) * n, i * n:(i + 1) * n], rtol=0, atol=tol)
        assert torch.equal(Dt[:, i], Dt[:, i].transpose(-1, -2))
        if i + 1 < T:
            assert torch.allclose(Et[:, i], X[:, (i + 1) * n:(i + 2) * n, i * n:(i + 1) * n], rtol=0, atol=tol)
    # T = 1 without E is potri
    D1 = torch.from_numpy(D[:, :1].copy()).to(P.DEV)
    batched.blocktri_potrf(D1, None)
    D2 = D1[:, 0].clone()
    assert batched.blocktri_potri(D1, None)[1] is None
    batched.potri(D2)
    assert torch.equal(torch.tril(D1[:, 0]), torch.tril(D2))
    big = torch.zeros(2, 2, 65, 65, dtype=torch.float64, device=P.DEV)
    flat = torch.zeros(5 * 3 * 81 + 5 * 2 * 81, dtype=torch.float64, device=P.DEV)
    bad = (lambda: batched.blocktri_potri(Dt.cpu(), Et.cpu()), lambda: batched.blocktri_potri(Dt.float(), Et.float()),
           lambda: batched.blocktri_potri(Dt, None), lambda: batched.blocktri_potri(Dt, Et[:, :1]), lambda: batched.blocktri_potri(Dt[:, 0], Et),
           lambda: batched.blocktri_potri(Dt.as_strided((5, 3, 9, 9), (0, 81, 9, 1)), Et),
           lambda: batched.blocktri_potri(big, big[:, :1].clone()),
           lambda: batched.blocktri_potri(flat[:5 * 3 * 81].view(5, 3, 9, 9), flat[81:81 + 5 * 2 * 81].view(5, 2, 9, 9)),      # D and E overlap
           lambda: batched.blocktri_potri(Dt, Et, info=torch.zeros(5, dtype=torch.int64, device=P.DEV)))
    for f in bad:
        with pytest.raises(_lib.CapitalError):
            f()
