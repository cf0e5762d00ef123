"""-m gpu: the batched pivoted Cholesky factorization cap_dpstrf_batched (csrc/pstrf_batched.hip) and its Python layer.  NO TOLERANCE
anywhere except logdet (4 spacing(|want|), the bound of tests/test_gpu_potrf_batched.py): R, piv, rank, info and resid are held BIT FOR
BIT (through positive_zero) to the Fraction model of the stated recurrence (tests/pstrf_batched_model.py) and, for the exact families, to
the answer known from their construction.

Every call runs on padded windows with NaN in A's strictly lower triangle, in all padding and behind every output, and a sentinel after
every per-block output; A and all padding are compared bit for bit afterwards (tests/pstrf_batched_gpu.py).
Sizes 1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64 - both sides of every NP - in batches of 1, G - 1, G, G + 1 and 2 G + 1 blocks with
G = 64 / NP: a full wave, a tail, dead groups.  The batch of a size cycles through its four exact blocks, so one model run per block
serves every batch and every cap (the model derives a capped run from the uncapped one).
exact_integer(n, flip) is exact while 2^(2n) + n fits into 53 bits (n <= 17: the known answer); the larger sizes are ordinary
matrices whose small pivots lie below the default tolerance, held to the model alone."""
import math

import numpy as np
import pytest
import torch

from tests import pstrf_batched_cases as PC
from tests import pstrf_batched_gpu as G
from tests import pstrf_batched_model as bm
from tests import pstrf_model as pm

pytestmark = pytest.mark.gpu

DEV = G.DEV


def _check_logdet(got, want):
    if math.isnan(want):
        assert math.isnan(got)
    else:
        assert abs(got - want) <= 4 * np.spacing(abs(want)), (got, want)


def _same_as_model(got, A, mr=None, tol=-1.0):
    R, piv, rank, resid, info, logdet = got
    Rm, pivm, rankm, residm, infom = bm.pstrf(A, mr, tol)
    assert (rank, info) == (rankm, infom), ((rank, info), (rankm, infom))
    assert np.array_equal(piv, pivm), "pivots differ from the model's"
    assert PC.same(R, Rm), "R differs from the model"
    assert PC.same(resid, residm), (resid, residm)
    _check_logdet(logdet, bm.logdet(Rm, rankm, infom))


# ---- 1. the exact families on every size, batch and cap -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PC.SIZES)
def test_exact_families_bit_for_bit(n):
    mats = [PC.exact_matrix(n, w) for w in PC.FAMILY]
    for batch in PC.batches(n):
        for mr in PC.caps(n):
            got = G.fixed([mats[i % 4] for i in range(batch)], mr)
            for i, g in enumerate(got):
                which = PC.FAMILY[i % 4]
                _same_as_model(g, mats[i % 4], mr)
                if which == "squares" or n <= PC.EXACT_KNOWN_MAX:
                    R, piv, rank, resid, info = PC.known_answer(n, which, mr)
                    assert PC.same(g[0], R) and np.array_equal(g[1], piv) and (g[2], g[3], g[4]) == (rank, resid, info), (which, batch, mr, i)


# ---- 2. the fixtures against the Fraction model, then the properties on the device output ----------------------------------------------------------
@pytest.mark.parametrize("kind,args", PC.FIXTURES + PC.MORE)
def test_fixtures_bit_for_bit_against_the_model(kind, args):
    A = PC.matrix(kind, args)
    n = A.shape[0]
    for mr in (n, n // 2):
        got = G.fixed([A, A.T.copy()], mr)
        for g in got:
            _same_as_model(g, A, mr)
        if kind != "graded":
            pm.check_properties(A, got[0][0], got[0][1], got[0][2], got[0][4], pm.default_tol(A))
    if kind == "dominant":
        assert got[0][2] == n // 2 and G.fixed([A])[0][2] == n      # dominant(64, 2): the full 64 steps


@pytest.mark.parametrize("kind,args,k", [("graded", (32, 8, 6), 3), ("graded", (17, 6, 13), 2), ("graded", (32, 8, 6), 1)])
def test_absolute_tolerance_between_two_pivots(kind, args, k):
    A = PC.matrix(kind, args)
    tol = pm.tol_between(bm.picks(A), k)
    for mr in (None, k, k + 2):
        got = G.fixed([A, A, A], mr, tol)
        for g in got:
            assert (g[2], g[4]) == (k, 0)
            _same_as_model(g, A, mr, tol)
            pm.check_properties(A, g[0], g[1], g[2], g[4], tol)


# ---- 3. stopping --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, 16, 33])
def test_stopping_rules(n):
    Z, I2, N = np.zeros((n, n)), 2.0 * np.eye(n), -np.diag(np.arange(1.0, n + 1))
    D = pm.dominant(n, 5)
    z, i2, d = G.fixed([Z, I2, D])
    assert (z[2], z[3], z[4], z[5]) == (0, 0.0, 0, 0.0) and np.array_equal(z[1], np.arange(n)) and PC.same(z[0], np.zeros((n, n)))
    assert (i2[2], i2[3], i2[4]) == (n, 0.0, 0) and np.array_equal(i2[1], np.arange(n)) and PC.same(i2[0], math.sqrt(2.0) * np.eye(n))
    _same_as_model(d, D)
    neg, = G.fixed([N], None, 0.0)                           # an absolute tolerance: no pivot is above it
    assert (neg[2], neg[3], neg[4]) == (0, -n * (n + 1) / 2.0, 0) and np.array_equal(neg[1], np.arange(n)) and PC.same(neg[0], np.zeros((n, n)))
    M = N.copy()
    M[n // 2, n // 2] = 0.0                                  # the default tolerance n eps max_i a_ii is 0: !(0 > 0)
    mix, = G.fixed([M])
    assert (mix[2], mix[4]) == (0, 0)
    _same_as_model(mix, M)
    for mr in PC.caps(n):                                    # the cap: info 1 while a pivot above the tolerance is left
        c, = G.fixed([D], mr)
        assert (c[2], c[4]) == (mr, 0 if mr == n else 1)
        _same_as_model(c, D, mr)
        if mr == 0:
            assert np.array_equal(c[1], np.arange(n)) and abs(c[3] - np.trace(D)) <= 2 * pm.gamma(n) * np.trace(D)
    c, = G.fixed([D], 0, 5.0)                                # every diagonal entry is below 5
    assert (c[2], c[4]) == (0, 0)


# ---- 4. mixed waves: the bits depend on (n, data) only -------------------------------------------------------------------------------------------
def _mixed_blocks(n):
    full = pm.dominant(n, 21)
    low = pm.gram(n, max(n // 3, 1), 22)
    nan_diag = pm.dominant(n, 23).copy()
    nan_diag[n // 2, n // 2] = np.nan
    nan_off = pm.dominant(n, 24).copy()
    order = bm.pstrf(nan_off)[1]
    a, b = int(order[min(2, n - 2)]), int(order[n - 1])
    nan_off[min(a, b), max(a, b)] = np.nan                   # read when the third pivot is taken: rank = 3, the rows before it finished
    return [full, low, np.zeros((n, n)), nan_diag, nan_off, pm.rbf(n, 25)]


@pytest.mark.parametrize("n", [8, 16, 29, 64])
def test_mixed_waves_have_the_bits_of_every_block_alone(n):
    blocks = _mixed_blocks(n)
    alone = [G.fixed([B])[0] for B in blocks]
    assert alone[0][2] == n and alone[0][4] == 0 and 0 < alone[1][2] < n and alone[2][2] == 0
    assert (alone[3][2], alone[3][4]) == (0, 2) and (alone[4][2], alone[4][4]) == (min(3, n - 1), 2) and math.isnan(alone[4][5])
    for B, g in zip(blocks, alone):
        _same_as_model(g, B)                                 # info 2 included: rank = the steps done, the finished rows intact
    bits = lambda g: (g[0].tobytes(), g[1].tobytes(), g[2], np.float64(g[3]).tobytes(), g[4], np.float64(g[5]).tobytes())
    want = [bits(g) for g in alone]
    for order, kw in ((range(6), {}), (range(5, -1, -1), {}), ((3, 0, 4, 1, 1, 2, 5, 0, 3), dict(pad_a=7, pad_r=1, gap_a=0, gap_r=13))):
        order = list(order)
        got = G.fixed([blocks[i] for i in order], **kw)
        for i, g in zip(order, got):
            assert bits(g) == want[i], "block %d changes its bits with its neighbours (order %s)" % (i, order)


# ---- 5. composition through the Python layer -----------------------------------------------------------------------------------------------------
def _torch_blocks(mats, pad=2):
    """(batch, n, n) view with stride(1) = n + pad whose LOWER triangle in torch's reading holds the matrices, NaN above it and in the padding"""
    batch, n = len(mats), mats[0].shape[0]
    buf = torch.full((batch, n, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=DEV))
    for i, M in enumerate(mats):
        buf[i, :, :n][low] = torch.from_numpy(np.array(M, dtype=np.float64)).to(DEV)[low]
    return buf[:, :, :n]


def test_python_pstrf_factor_and_properties():
    from capital_amd import batched
    n = 33
    mats = [pm.dominant(n, 1), pm.gram(n, 12, 12), pm.rbf(n, 7), np.zeros((n, n))]
    A = _torch_blocks(mats)
    before = A.clone()
    L, piv, rank, resid, info, logdet = batched.pstrf(A, logdet=True)
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(A, nan=7.0), torch.nan_to_num(before, nan=7.0))
    assert L.shape == (4, n, n) and piv.shape == (4, n) and piv.dtype == torch.int64 and rank.dtype == torch.int32 and info.dtype == torch.int32
    for i, M in enumerate(mats):
        Li, pi, ri = L[i].cpu().numpy(), piv[i].cpu().numpy(), int(rank[i])
        _same_as_model((Li.T, pi, ri, float(resid[i]), int(info[i]), float(logdet[i])), M)
        assert np.all(np.triu(Li, 1) == 0) and np.all(Li[:, ri:] == 0)
        pm.check_properties(M, Li.T, pi, ri, int(info[i]), pm.default_tol(M))          # L L^T against A[piv][:, piv]
    Lc, pc, rc, sc, ic = batched.pstrf(A, max_rank=5, tol=0.0)
    assert Lc.shape == (4, n, 5) and rc.tolist() == [5, 5, 5, 0] and ic.tolist() == [1, 1, 1, 0]
    assert torch.equal(Lc[:3, :5], L[:3, :5, :5]) and torch.equal(pc[:3, :5], piv[:3, :5])      # the first five steps do not know the cap
    for i, M in enumerate(mats):
        Rm, pivm, rankm, residm, infom = bm.pstrf(M, 5, 0.0)
        assert PC.same(Lc[i].cpu().numpy().T, Rm) and np.array_equal(pc[i].cpu().numpy(), pivm) and PC.same(float(sc[i]), residm)


def test_python_solve_through_the_permutation_is_exact():
    from capital_amd import batched
    n, rng = 12, np.random.default_rng(3)
    built = [pm.exact_integer(n, f) for f in (0, 1, 2, 2, 1)]
    A = _torch_blocks([b[0] for b in built])
    x = rng.integers(-4, 5, size=(len(built), 3, n)).astype(np.float64)
    b = np.stack([xi @ bi[0] for xi, bi in zip(x, built)])                 # rows: (A x)^T, exact integers
    L, piv, rank, resid, info = batched.pstrf(A)
    assert rank.tolist() == [n] * len(built) and info.tolist() == [0] * len(built)
    B = batched.permute(torch.from_numpy(b).to(DEV), piv)
    sol = batched.permute(batched.potrs(L, B), piv, inverse=True)
    assert np.array_equal(sol.cpu().numpy(), x)
    v = torch.from_numpy(b[:, 0].copy()).to(DEV)                            # (batch, n) right-hand sides
    assert torch.equal(batched.permute(batched.permute(v, piv), piv, inverse=True), v)
    assert torch.equal(batched.permute(v, piv), torch.gather(v, 1, piv))


def test_python_semidefinite_products():
    """syrk(L, trans=True) = L L^T and trmm(L, z) = L z on integer rank-k blocks: exact, whatever the order of summation; the columns
    >= rank of L contribute nothing"""
    from capital_amd import batched
    n, k, rng = 12, 5, np.random.default_rng(4)
    built = [PC.semidefinite_integer(n, k, f) for f in (0, 1, 2)]
    A = _torch_blocks([b[0] for b in built])
    L, piv, rank, resid, info = batched.pstrf(A)
    assert rank.tolist() == [k] * 3 and info.tolist() == [0] * 3 and resid.tolist() == [0.0] * 3
    C = batched.syrk(L, trans=True, symmetric=True)
    C2 = batched.syrk(L.transpose(1, 2).contiguous(), trans=False, symmetric=True)
    assert torch.equal(C, C2)                                               # syrk's contract: the same bits for any layout or trans
    for i, (Ai, Tk, perm) in enumerate(built):
        p = piv[i].cpu().numpy()
        assert np.array_equal(C[i].cpu().numpy(), Ai[np.ix_(p, p)])
    z = rng.integers(-4, 5, size=(3, 2, n)).astype(np.float64)
    z2 = z.copy()
    z2[:, :, k:] = rng.integers(10, 20, size=(3, 2, n - k))                 # only the entries that meet the zero columns differ
    y = batched.permute(batched.trmm(L, torch.from_numpy(z).to(DEV)), piv, inverse=True)
    y2 = batched.permute(batched.trmm(L, torch.from_numpy(z2).to(DEV)), piv, inverse=True)
    assert torch.equal(y, y2)
    for i, (Ai, Tk, perm) in enumerate(built):
        assert np.array_equal(y[i].cpu().numpy(), (z[i][:, :k] @ Tk)[:, np.argsort(perm)])


def test_python_logdet_equals_potrf_without_pivoting():
    """a diagonally graded SPD batch whose natural order is already the pivot order"""
    from capital_amd import batched
    n, rng = 33, np.random.default_rng(6)
    mats = []
    for s in range(5):
        g = rng.standard_normal((n, n))
        mats.append(0.01 * (g @ g.T) / n + np.diag(np.linspace(3.0, 1.0, n) * (s + 1)))
    mats.append(pm.exact_integer(12, 0)[0])
    for group in (mats[:5], mats[5:]):
        A = _torch_blocks(group)
        L, piv, rank, resid, info, ld = batched.pstrf(A, logdet=True)
        m = group[0].shape[0]
        assert torch.equal(piv.cpu(), torch.arange(m).expand(len(group), m)) and rank.tolist() == [m] * len(group)
        F = A.clone()
        finfo, fld = batched.potrf(F, logdet=True)
        assert finfo.tolist() == [0] * len(group)
        for got, want in zip(ld.tolist(), fld.tolist()):
            _check_logdet(got, want)


def test_python_refusals_on_the_device():
    from capital_amd import _lib, batched
    a = torch.zeros(2, 65, 65, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.CapitalError, match="factor_pivoted"):
        batched.pstrf(a)
    a = torch.zeros(2, 8, 8, dtype=torch.float64, device=DEV)
    for bad in (lambda: batched.pstrf(a, max_rank=9), lambda: batched.pstrf(a, max_rank=-1), lambda: batched.pstrf(a, tol=float("nan")),
                lambda: batched.pstrf(a.float()), lambda: batched.pstrf(a[:, :, :7]), lambda: batched.pstrf(a.cpu()),
                lambda: batched.permute(a[:, 0], torch.zeros(2, 7, dtype=torch.int64, device=DEV)),
                lambda: batched.permute(a[:, 0], torch.zeros(2, 8, dtype=torch.int32, device=DEV))):
        with pytest.raises(_lib.CapitalError):
            bad()
    from capital_amd import lapack
    pack = lapack.ArgPack_pstrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    piv = torch.zeros(16, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.CapitalError, match="overlaps"):
        lapack.engine._pstrf_batched(a, a, piv, 8, 8, 8, 64, 8, 64, 2, -1.0, pack)
    e = batched.pstrf(a[:0])
    assert e[0].shape == (0, 8, 8) and e[1].shape == (0, 8) and e[2].shape == (0,)
