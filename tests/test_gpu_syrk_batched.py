"""-m gpu: cap_dsyrk_batched (csrc/syrk_batched.hip) on an MI355X.
1. exact results on the rows of tests/syrk_batched_cases.py (no tolerance; everything the call must not touch is still NaN, with beta == 0
the old triangle is NaN too and the result is clean), 2. alpha == 0 / k == 0 with a NULL V, 3. CONTRACTS 2 and 3: a block alone against the
same block in a batch, at another index, with other leading dimensions and strides, and in the other layout, 4. CONTRACT 4: elements
against the 2 x 2 / 1 x 1 blocks of their rows, on both paths, 5. random data under the derived elementwise bound in np.longdouble, 6. the
Python layer: potrf(syrk(X, shift)), schur with a failed block.  (CONTRACT 1: tests/test_gpu_syrk_vbatched.py.)

THE OUTCOME OF THE CONTRACT-4 CHECK on the MI355X is recorded in profiles/r25_syrk_batched.txt."""
import numpy as np
import pytest
import torch

from tests import syrk_batched_cases as SC
from tests import syrk_batched_gpu as G

pytestmark = pytest.mark.gpu

TRANS, NOTRANS = G.TRANS, G.NOTRANS
REAL_N = (7, 33, 64, 65, 130, 256)          # every NP but 16 ... and 16 below; both paths
REAL_K = (5, 40)


# ---- 1. exact rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SC.exact_rows(), ids=SC.row_id)
def test_exact_rows_bit_for_bit(row):
    n, k, batch, trans, fill, (alpha, beta), shift, lc, lv = row
    ops = [SC.operands(n, k, i) for i in range(batch)]
    out = G.run(trans, [o[0] for o in ops], None if beta == 0.0 else [o[1] for o in ops], alpha, beta,
                [o[2] for o in ops] if shift else None, fill, lc, lv)
    G.check_exact(out, [SC.expected(o[0], o[1], o[2], alpha, beta, shift) for o in ops], fill)


# ---- 2. V is not addressed ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 130))
@pytest.mark.parametrize("alpha,k", ((0.0, 5), (1.0, 0)))
def test_alpha_zero_or_k_zero_never_addresses_v(n, alpha, k):
    ops = [SC.operands(n, k, i) for i in range(3)]
    out = G.run(NOTRANS, [o[0] for o in ops], [o[1] for o in ops], alpha, 1.0, [o[2] for o in ops], 0, null_v=True)
    G.check_exact(out, [o[1] + o[2] * np.eye(n) for o in ops], 0)
    out = G.run(TRANS, [o[0] for o in ops], None, alpha, 0.0, None, 1, null_v=True)
    G.check_exact(out, [np.zeros((n, n)) for _ in ops], 1)


# ---- 3. CONTRACTS 2 and 3 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", REAL_N + (16,))
def test_layout_independence_and_trans_is_a_layout(n):
    k, alpha, beta = 21, -0.75, 1.25
    blocks = [G.real(n, k, s) for s in range(6)]
    alone = [G.run(NOTRANS, [b[0]], [b[1]], alpha, beta, [b[2]], 1)[0] for b in blocks[:3]]
    for trans in (NOTRANS, TRANS):
        for lc, lv, order in (((0, 0), (0, 0), (0, 1, 2, 3, 4, 5)), ((1, 3), (6, 0), (5, 4, 2, 1, 0, 3)), ((6, 0), (0, 3), (3, 0, 5, 1, 4, 2))):
            bl = [blocks[i] for i in order] * 3                   # 18 blocks: more than one wavefront for every NP
            out = G.run(trans, [b[0] for b in bl], [b[1] for b in bl], alpha, beta, [b[2] for b in bl], 1, lc, lv)
            for pos, i in enumerate(list(order) * 3):
                if i < 3:
                    assert G.same(out[pos], alone[i]), "trans %d, layouts %s %s, position %d" % (trans, lc, lv, pos)
    # the fill does not change the triangle
    out = G.run(TRANS, [blocks[0][0]], [blocks[0][1]], alpha, beta, [blocks[0][2]], 0)
    assert G.same(np.triu(out[0]), np.triu(alone[0]))


# ---- 4. CONTRACT 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", (0.0, 1.5))
@pytest.mark.parametrize("n", (8, 40, 64, 100, 256))
def test_an_element_is_a_function_of_its_two_rows(n, beta):
    k, alpha = 23, 0.625
    V, C, lam = G.real(n, k, 4)
    big = G.run(NOTRANS, [V], None if beta == 0.0 else [C], alpha, beta, [lam], 0, (1, 3), (6, 0))[0]
    pairs = {(0, 0), (0, n - 1), (n - 1, n - 1), (n // 2, n // 2), (n // 3, n - 2), (1, 2), (min(15, n - 2), min(16, n - 1)), (n - 2, n - 1), (3, n // 2 + 1)}
    if n > 64:
        pairs |= {(5, 70), (63, 64), (64, 64), (65, 99), (n - 36, n - 1)}
    for r, c in sorted(pairs):
        assert 0 <= r <= c < n
        if r == c:
            small = G.run(TRANS, [V[[r]]], None if beta == 0.0 else [C[[r]][:, [r]]], alpha, beta, [lam], 0)[0]
            assert G.same(small[0, 0], big[r, r]), "n %d element (%d, %d): %r against %r" % (n, r, c, big[r, r], small[0, 0])
        else:
            rows = [r, c]
            small = G.run(NOTRANS, [V[rows]], None if beta == 0.0 else [C[rows][:, rows]], alpha, beta, [lam], 0)[0]
            assert G.same(small[0, 1], big[r, c]), "n %d element (%d, %d): %r against %r" % (n, r, c, big[r, c], small[0, 1])


# ---- 5. accuracy --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", REAL_K)
@pytest.mark.parametrize("n", REAL_N)
def test_random_data_within_the_derived_bound(n, k):
    """s is a sum of k products (gamma_k, any order), t = alpha s one more rounding, the fma and the shift one each: with
    |beta c + t| <= |beta||c| + |t| the error is at most gamma_{k+2} (|alpha| |V||V|^T + |beta| |C| + |lambda|) elementwise"""
    alpha, beta = 1.75, -0.5
    bl = [G.real(n, k, 10 + s) for s in range(3)]
    for trans in (NOTRANS, TRANS):
        out = G.run(trans, [b[0] for b in bl], [b[1] for b in bl], alpha, beta, [b[2] for b in bl], 1, (1, 3), (0, 3))
        for (V, C, lam), got in zip(bl, out):
            Vl, Cl = V.astype(np.longdouble), C.astype(np.longdouble)
            want = alpha * (Vl @ Vl.T) + beta * Cl + np.longdouble(lam) * np.eye(n)
            bound = G.gamma(k + 2) * (abs(alpha) * (np.abs(Vl) @ np.abs(Vl).T) + abs(beta) * np.abs(Cl) + abs(lam) * np.eye(n))
            err = np.abs(got.astype(np.longdouble) - want)
            print("n %d k %d trans %d: error / bound = %.3f" % (n, k, trans, float(np.max(err / bound))))
            assert np.all(err <= bound)


# ---- 6. the Python layer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (9, 130))
def test_potrf_of_syrk_against_torch(n):
    """potrf(syrk(X, shift)) against torch.linalg.cholesky of the matrix torch forms in fp64.  Both formed matrices are within
    gamma_{k+2} (|X|^T|X| + lambda) of the exact one, the factor satisfies potrf's bound |A - L L^T| <= gamma_{n+2} |L||L|^T (tests/test_gpu_potrf_batched.py):
    |A_torch - L L^T| <= gamma_{n+2} |L||L|^T + 2 gamma_{k+2} (|X|^T|X| + lambda), and with kappa = cond(A) the factor itself is within
    kappa (gamma_{n+2} + 2 gamma_{k+2}) ||L_ref||_F of torch's."""
    from capital_amd import batched
    batch, k = 4, 37
    rng = np.random.default_rng([88, n])
    X = torch.from_numpy(rng.standard_normal((batch, k, n))).to(G.DEV)
    lam = torch.from_numpy(np.full(batch, float(n)) + rng.random(batch)).to(G.DEV)
    A = batched.syrk(X, shift=lam)
    ref = X.transpose(1, 2) @ X + torch.diag_embed(lam.unsqueeze(1).expand(batch, n))
    assert torch.equal(torch.triu(A, 1), torch.zeros_like(A).triu(1)), "the strictly upper triangle (torch's reading) of a fresh C is not zero"
    info = batched.potrf(A)
    assert not info.cpu().numpy().any()
    Lo, Lref = torch.tril(A).cpu().numpy(), torch.linalg.cholesky(ref).cpu().numpy()
    Xh, refh = X.cpu().numpy(), ref.cpu().numpy()
    for i in range(batch):
        l = Lo[i].astype(np.longdouble)
        form = np.abs(Xh[i]).T @ np.abs(Xh[i]) + float(lam[i]) * np.eye(n)
        assert np.all(np.abs(refh[i] - l @ l.T) <= G.gamma(n + 2) * (np.abs(l) @ np.abs(l).T) + 2 * G.gamma(k + 2) * form)
        kappa = np.linalg.cond(refh[i])
        assert np.linalg.norm(Lo[i] - Lref[i]) <= kappa * (G.gamma(n + 2) + 2 * G.gamma(k + 2)) * np.linalg.norm(Lref[i])
    # trans=True is the other layout of the same product; symmetric=True fills the other triangle
    A2 = batched.syrk(X.transpose(1, 2).contiguous(), trans=True, shift=lam, symmetric=True)
    B = batched.syrk(X, shift=lam)
    assert torch.equal(torch.tril(A2), torch.tril(B)) and torch.equal(A2, A2.transpose(1, 2))


@pytest.mark.parametrize("n,m", ((12, 7), (70, 100)))
def test_schur_against_torch_with_a_failed_block(n, m):
    from capital_amd import batched
    batch = 3
    rng = np.random.default_rng([89, n, m])
    X = rng.standard_normal((batch, n + 5, n))
    A = np.einsum("bki,bkj->bij", X, X) + n * np.eye(n)
    A[1] = -A[1]                                                       # not positive definite: info[1] = 1
    Bm = rng.standard_normal((batch, m, n))
    Cm = np.einsum("bmi,bni->bmn", Bm, Bm) + m * np.eye(m)
    R, B, C = (torch.from_numpy(x.copy()).to(G.DEV) for x in (A, Bm, Cm))
    info = batched.potrf(R)
    assert info.cpu().numpy().tolist() == [0, 1, 0]
    C0 = C.clone()
    out = batched.schur(R, B, C, info)
    assert out is C
    Ch, Bh = C.cpu().numpy(), B.cpu().numpy()
    assert np.isnan(Ch[1][np.tril_indices(m)]).all() and np.isnan(Bh[1]).all()
    assert torch.equal(torch.triu(C, 1), torch.triu(C0, 1)), "the triangle potrf does not read was written"
    for i in (0, 2):
        # the reference in np.longdouble from the device's own factor L (torch's reading: the lower triangle of R[i])
        Lf = np.tril(R[i].cpu().numpy()).astype(np.longdouble)
        Bl, Cl = Bm[i].astype(np.longdouble), Cm[i].astype(np.longdouble)
        W = np.linalg.solve(Lf.astype(np.float64), Bm[i].T).astype(np.longdouble)              # n x m, columns w_j = L^-1 b_j
        W = W + np.linalg.solve(Lf.astype(np.float64), (Bl.T - Lf @ W).astype(np.float64))     # one step of refinement in longdouble
        # substitution: (L + dL) w = b with |dL| <= gamma_n |L|, so ||dw_j|| <= cw ||w_j||, cw = 2 gamma_n n cond(L) (first order, doubled)
        cw = 2 * G.gamma(n) * n * np.linalg.cond(Lf.astype(np.float64))
        norms = np.linalg.norm(W.astype(np.float64), axis=0)
        assert np.all(np.linalg.norm(Bh[i].T - W.astype(np.float64), axis=0) <= cw * norms)
        # the product of the perturbed rows: 2 cw ||w_j|| ||w_l|| (first order, doubled: + cw^2) beside syrk's own gamma_{n+2} bound
        want = Cl - W.T @ W
        tol = G.gamma(n + 2) * (np.abs(Cl) + np.abs(W.T) @ np.abs(W)) + (2 * cw + cw * cw) * np.outer(norms, norms)
        assert np.all(np.abs(np.tril(Ch[i]) - np.tril(want)) <= np.tril(tol))
