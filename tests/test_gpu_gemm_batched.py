"""-m gpu: cap_dgemm_batched (csrc/gemm_batched.hip) on an MI355X.
1. every exact row of tests/gemm_batched_cases.py bit for bit against NumPy - NaN in every pad row, gap and tail, and in C where beta == 0,
still there bit for bit afterwards, A and B unchanged (tests/gemm_batched_gpu.run asserts all that), 2. the bit contracts on random
non-integer data: LAYOUT INDEPENDENCE, TRANS IS A LAYOUT, ELEMENT INDEPENDENCE on both paths, COMPOSITION with cap_dsyrk_batched and
cap_dsymm_batched, 3. batched.gemm against torch.baddbmm on the exact data, 4. the refusals."""
import numpy as np
import pytest
import torch

from tests import gemm_batched_cases as GC
from tests import gemm_batched_gpu as G
from tests import symm_batched_gpu as SG
from tests import syrk_batched_gpu as YG

pytestmark = pytest.mark.gpu

NOTRANS, TRANS = G.NOTRANS, G.TRANS
ARG, UNSUPPORTED = 1, 4


@pytest.mark.parametrize("row", GC.exact_rows(), ids=GC.row_id)
def test_exact_rows_bit_for_bit(row):
    m, n, k, batch, ta, tb, (alpha, beta), la, lb, lc = row
    ops = [GC.operands(m, n, k, i) for i in range(batch)]
    out = G.run(ta, tb, [o[0] for o in ops], [o[1] for o in ops], None if beta == 0.0 else [o[2] for o in ops], alpha, beta, la, lb, lc,
                null_ab=(alpha == 0.0 or k == 0) and batch % 2 == 1)
    for i, o in enumerate(ops):
        assert G.same(out[i] + 0.0, GC.expected(o[0], o[1], o[2], alpha, beta)), "block %d" % i


SHAPES = ((7, 9, 5), (33, 64, 21), (64, 64, 16), (65, 3, 17), (130, 100, 19), (17, 130, 4))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_contracts_2_and_3_layout_and_trans_do_not_change_a_bit(m, n, k):
    alpha, beta = 1.375, -0.625
    bl = [G.real(m, n, k, i) for i in range(5)]
    As, Bs, Cs = [b[0] for b in bl], [b[1] for b in bl], [b[2] for b in bl]
    ref = G.run(NOTRANS, NOTRANS, As, Bs, Cs, alpha, beta)
    for ta, tb in GC.TRANS_PAIRS[1:]:                                                  # CONTRACT 3
        got = G.run(ta, tb, As, Bs, Cs, alpha, beta)
        assert all(G.same(g, r) for g, r in zip(got, ref)), (ta, tb)
    got = G.run(TRANS, NOTRANS, As, Bs, Cs, alpha, beta, (1, 3), (6, 0), (0, 3))       # CONTRACT 2: ld, stride, alignment
    assert all(G.same(g, r) for g, r in zip(got, ref))
    for i in (4, 0):                                                                   # batch and index
        alone = G.run(NOTRANS, TRANS, [As[i]], [Bs[i]], [Cs[i]], alpha, beta, (6, 0), (1, 3), (1, 3))[0]
        assert G.same(alone, ref[i]), i
    many = G.run(NOTRANS, NOTRANS, [As[i % 5] for i in range(23)], [Bs[i % 5] for i in range(23)], [Cs[i % 5] for i in range(23)], alpha, beta)
    assert all(G.same(many[i], ref[i % 5]) for i in range(23))
    zero = G.run(NOTRANS, NOTRANS, As, Bs, None, alpha, 0.0)                           # beta == 0: t = alpha s alone
    assert all(np.isfinite(z).all() for z in zero)


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_contract_4_every_element_is_the_one_by_one_product(m, n, k):
    alpha, beta = -0.75, 1.25
    A, B, C = G.real(m, n, k, 9)
    ref = G.run(NOTRANS, NOTRANS, [A], [B], [C], alpha, beta)[0]
    rng = np.random.default_rng([5, m, n])
    picks = sorted({(0, 0), (m - 1, n - 1), (m - 1, 0), (0, n - 1)} | {(int(rng.integers(m)), int(rng.integers(n))) for _ in range(12)})
    ones = G.run(NOTRANS, NOTRANS, [A[r:r + 1, :] for r, c in picks], [B[:, c:c + 1] for r, c in picks], [C[r:r + 1, c:c + 1] for r, c in picks],
                 alpha, beta)
    for (r, c), o in zip(picks, ones):
        assert G.same(o, ref[r:r + 1, c:c + 1]), (r, c)
    c = n // 2                                                                         # a column's bits do not depend on its company
    col = G.run(TRANS, TRANS, [A], [B[:, c:c + 1]], [C[:, c:c + 1]], alpha, beta)[0]
    assert G.same(col, ref[:, c:c + 1])


@pytest.mark.parametrize("n,k", ((9, 5), (64, 17), (130, 19)))
def test_contract_5_composition_with_syrk_and_symm(n, k):
    alpha, beta = 1.375, -0.625
    bl = [YG.real(n, k, i) for i in range(3)]
    Vs, Cs = [b[0] for b in bl], [b[1] for b in bl]
    syrk = YG.run(NOTRANS, Vs, Cs, alpha, beta)
    mine = G.run(NOTRANS, TRANS, Vs, [v.T for v in Vs], Cs, alpha, beta)
    for s, g in zip(syrk, mine):
        assert G.same(np.triu(s), np.triu(g)), "gemm(N, T) with B = A against cap_dsyrk_batched"
    rng = np.random.default_rng([6, n, k])
    Xs, Bs = [rng.standard_normal((n, k)) for _ in bl], [rng.standard_normal((n, k)) for _ in bl]
    symm = SG.symm(Cs, Xs, Bs, alpha, beta)
    mine = G.run(NOTRANS, NOTRANS, Cs, Xs, Bs, alpha, beta)
    for s, g in zip(symm, mine):
        assert G.same(s, g), "gemm(N, N) with the symmetrised block against cap_dsymm_batched"


@pytest.mark.parametrize("row", [r for r in GC.exact_rows() if r[3] <= 65][::6], ids=GC.row_id)
def test_python_gemm_against_baddbmm_on_the_exact_data(row):
    from capital_amd import batched
    m, n, k, batch, ta, tb, (alpha, beta) = row[:7]
    ops = [GC.operands(m, n, k, i) for i in range(batch)]
    A = torch.from_numpy(np.ascontiguousarray(np.stack([o[0].T if ta else o[0] for o in ops]))).to(G.DEV)
    B = torch.from_numpy(np.ascontiguousarray(np.stack([o[1].T if tb else o[1] for o in ops]))).to(G.DEV)
    pad = torch.full((batch, m + 1, n + 3), float("nan"), dtype=torch.float64, device=G.DEV)
    C = pad[:, :m, :n]                                                                 # a free stride(1) and gaps between the blocks
    C.copy_(torch.from_numpy(np.stack([o[2] for o in ops])))
    want = torch.baddbmm(C, A.transpose(1, 2) if ta else A, B.transpose(1, 2) if tb else B, beta=beta, alpha=alpha)
    got = batched.gemm(A, B, C, transa=bool(ta), transb=bool(tb), alpha=alpha, beta=beta)
    assert got is C and torch.equal(got + 0.0, want + 0.0)
    assert torch.isnan(pad[:, m:, :]).all() and torch.isnan(pad[:, :, n:]).all()
    if beta == 0.0:
        fresh = batched.gemm(A, B, transa=bool(ta), transb=bool(tb), alpha=alpha)
        assert fresh.shape == (batch, m, n) and torch.equal(fresh + 0.0, want + 0.0)


def test_refusals_on_the_device():
    from capital_amd import _lib, batched
    L = G.lib()
    d = torch.zeros(4096, dtype=torch.float64, device=G.DEV)
    p = d.data_ptr()
    big = torch.zeros(257 * 257 * 2, dtype=torch.float64, device=G.DEV)

    def call(ta=0, tb=0, m=4, n=5, k=3, alpha=1.0, A=p, lda=4, sa=12, B=p + 8 * 100, ldb=3, sb=15, beta=0.0, C=p + 8 * 1000, ldc=4, sc=20, batch=2):
        return L.cap_dgemm_batched(ta, tb, m, n, k, alpha, A, lda, sa, B, ldb, sb, beta, C, ldc, sc, batch, G.stream())
    assert call() == 0
    assert call(ta=2) == ARG and call(m=-1) == ARG and call(C=None) == ARG and call(A=None) == ARG and call(ldc=3) == ARG and call(sb=14) == ARG
    assert call(C=p) == ARG and call(C=p + 8 * 110) == ARG                             # C overlaps A, C overlaps B
    assert call(C=p, alpha=0.0) == 0 and call(A=None, B=None, k=0) == 0
    assert L.cap_dgemm_batched(0, 0, 257, 1, 1, 1.0, big.data_ptr(), 257, 257, big.data_ptr() + 8 * 600, 1, 1, 0.0, big.data_ptr() + 8 * 1000, 257, 257, 1,
                               G.stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    a = torch.zeros(2, 4, 3, dtype=torch.float64, device=G.DEV)
    b = torch.zeros(2, 3, 5, dtype=torch.float64, device=G.DEV)
    buf = torch.zeros(64, dtype=torch.float64, device=G.DEV)
    for bad in (lambda: batched.gemm(a.cpu(), b), lambda: batched.gemm(a.float(), b.float()), lambda: batched.gemm(a, b[:, :2]),
                lambda: batched.gemm(a, b, beta=1.0), lambda: batched.gemm(a, b, torch.zeros(2, 4, 4, dtype=torch.float64, device=G.DEV)),
                lambda: batched.gemm(a, b.transpose(1, 2)), lambda: batched.gemm(a, b, torch.zeros(4, 5, dtype=torch.float64, device=G.DEV).expand(2, 4, 5)),
                lambda: batched.gemm(torch.zeros(1, 257, 2, dtype=torch.float64, device=G.DEV), torch.zeros(1, 2, 2, dtype=torch.float64, device=G.DEV)),
                lambda: batched.gemm(buf[:24].view(2, 4, 3), b, buf[10:50].view(2, 4, 5)), lambda: batched.gemm(a, b[:, :, 0]),
                lambda: batched.gemm(a, b, torch.zeros(2, 5, 4, dtype=torch.float64, device=G.DEV).transpose(1, 2))):
        with pytest.raises(_lib.CapitalError):
            bad()
