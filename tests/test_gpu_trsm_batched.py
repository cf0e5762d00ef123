"""-m gpu: the batched triangular solves and products on the fp64 Cholesky factors (cap_dtrsm_batched, cap_dtrmm_batched, batched.trsm /
trmm / mahalanobis).

1. exact results on the rows of tests/trsm_batched_cases.py (no tolerance; everything the call must not touch is still NaN), 2. sumsq bit
for bit against the stated fma recurrence on the device's own result, 3. CONTRACT 1: the two halves against cap_dpotrs_batched_blocked,
4. CONTRACT 3: a column alone, among 17 and as the last of 40, 5. failed blocks and info = NULL, 6. random factors under the textbook
componentwise bounds in np.longdouble, 7. stream order, 8. the Python layer.  (CONTRACT 2: tests/test_gpu_trsm_vbatched.py.)"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import potri_batched_cases as P
from tests import stream_order as SO
from tests import trsm_batched_cases as TC
from tests import trsm_batched_gpu as G
from tests.tri_cases import positive_zero

pytestmark = pytest.mark.gpu

TRANS, NOTRANS = G.TRANS, G.NOTRANS
ALL_N = TC.WAVE_N + TC.GROUP_N


def _wave_batch(n):
    """one block more than a wavefront carries (n <= 64), three above"""
    np_ = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    return 64 // np_ + 1 if n <= 64 else 3


def _exact(a):
    return positive_zero(np.asarray(a)).view(np.int64)


# ---- 1. exact results -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", TC.exact_rows(), ids=TC.row_id)
def test_exact_results_and_nothing_else_touched(row):
    n, fam, batch, nrhs, layout = row
    ops = [TC.operands(fam, n, nrhs, i % TC.DISTINCT) for i in range(batch)]
    Ts, Xs = [o[0] for o in ops], [o[2] for o in ops]
    sq = [(o[2] ** 2).sum(axis=0) for o in ops]
    for trans, rhs in ((TRANS, [o[3] for o in ops]), (NOTRANS, [o[4] for o in ops])):
        got, q = G.run("trsm", trans, Ts, rhs, layout, info=[0] * batch, sumsq=True)
        for i in range(batch):
            assert np.array_equal(_exact(got[i]), _exact(Xs[i])), "trsm trans=%d block %d: not X" % (trans, i)
            assert np.array_equal(q[i], sq[i]), "trsm trans=%d block %d: sumsq is not the integer column sum of X^2" % (trans, i)
        got, _ = G.run("trmm", trans, Ts, Xs, layout, info=None)
        for i in range(batch):
            assert np.array_equal(_exact(got[i]), _exact(rhs[i])), "trmm trans=%d block %d: not the exact product" % (trans, i)


# ---- the shared random factors: factored once by the library, never written ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _factors(n, kappa, count):
    Rs = G.factor(list(P.random_spd(n, kappa, count)))
    for r in Rs:
        r.setflags(write=False)
    return tuple(Rs)


@functools.lru_cache(maxsize=None)
def _rhs(n, nrhs, count):
    out = [np.random.default_rng([5, n, nrhs, i]).standard_normal((n, nrhs)) for i in range(count)]
    for b in out:
        b.setflags(write=False)
    return tuple(out)


# ---- 2. sumsq ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (7, 33, 64, 65, 130, 256))
@pytest.mark.parametrize("trans", (TRANS, NOTRANS))
def test_sumsq_is_the_stated_recurrence_on_the_stored_column(n, trans):
    batch, nrhs = _wave_batch(n), 17
    got, q = G.run("trsm", trans, _factors(n, 1e6, batch), _rhs(n, nrhs, batch), (1, 3), sumsq=True)
    for i in (0, batch - 1):
        for k in range(nrhs):
            want = TC.sumsq_model(got[i][:, k])
            assert np.float64(want).view(np.int64) == q[i, k].view(np.int64), (i, k, want, q[i, k])
            if hasattr(math, "fma"):
                w = 0.0
                for v in got[i][:, k]:
                    w = math.fma(float(v), float(v), w)
                assert w == want


# ---- 3. contract 1: halves = whole --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_N)
def test_the_two_halves_leave_the_bits_of_potrs(n):
    batch = _wave_batch(n)
    Rs = _factors(n, 1e6, batch)
    info = [0] * batch
    if batch > 1:
        info[1] = 3                      # a failed block: NaN from both routes
    layout = TC.LAYOUTS[n % 4]
    for nrhs in (1, 17, 40):
        Bs = _rhs(n, nrhs, batch)
        want, _ = G.run("potrs", 0, Rs, Bs, layout, info=info)
        half, _ = G.run("trsm", TRANS, Rs, Bs, layout, info=info)
        got, _ = G.run("trsm", NOTRANS, Rs, half, layout, info=info)
        for i in range(batch):
            assert G.same(got[i], want[i]), "n=%d nrhs=%d block %d" % (n, nrhs, i)
            assert np.isnan(want[i]).all() == (info[i] != 0) and np.isnan(want[i]).any() == (info[i] != 0)


# ---- 4. contract 3: column independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (7, 33, 64, 65, 200))
@pytest.mark.parametrize("entry,trans", (("trsm", TRANS), ("trsm", NOTRANS), ("trmm", TRANS), ("trmm", NOTRANS)))
def test_a_column_does_not_depend_on_its_company(n, entry, trans):
    batch, j = 2, 11
    Rs, B17, B40 = _factors(n, 1e6, 3)[:batch], _rhs(n, 17, batch), _rhs(n, 40, batch)
    ss = entry == "trsm"
    g17, q17 = G.run(entry, trans, Rs, B17, sumsq=ss)
    alone, q1 = G.run(entry, trans, Rs, [b[:, j:j + 1] for b in B17], sumsq=ss)
    last = [np.concatenate([b40[:, :39], b17[:, j:j + 1]], axis=1) for b40, b17 in zip(B40, B17)]
    g40, q40 = G.run(entry, trans, Rs, last, sumsq=ss)
    for i in range(batch):
        assert G.same(g17[i][:, j], alone[i][:, 0]) and G.same(g17[i][:, j], g40[i][:, 39])
        if ss:
            assert G.same(q17[i, j], q1[i, 0]) and G.same(q17[i, j], q40[i, 39])


# ---- 5. failed blocks, info = NULL -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (5, 8, 33, 64, 65, 130))
@pytest.mark.parametrize("entry,trans", (("trsm", TRANS), ("trsm", NOTRANS), ("trmm", TRANS), ("trmm", NOTRANS)))
def test_failed_blocks_get_nan_and_their_neighbours_keep_their_bits(n, entry, trans):
    batch, nrhs = _wave_batch(n) + 1, 17
    Rs, Bs = _factors(n, 1e1, batch), _rhs(n, nrhs, batch)
    ss = entry == "trsm"
    free, qf = G.run(entry, trans, Rs, Bs, (0, 3), info=None, sumsq=ss)            # info = NULL: every block is served
    info = [0] * batch
    info[1], info[batch - 1] = 2, -1
    got, q = G.run(entry, trans, Rs, Bs, (0, 3), info=info, sumsq=ss)
    for i in range(batch):
        assert np.isfinite(free[i]).all()
        if info[i]:
            assert np.isnan(got[i]).all() and (not ss or np.isnan(q[i]).all())
        else:
            assert G.same(got[i], free[i]) and (not ss or G.same(q[i], qf[i]))


# ---- 6. random factors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.RANDOM_N)
@pytest.mark.parametrize("kappa", P.KAPPAS)
def test_random_factors_meet_the_componentwise_bounds(n, kappa):
    """T = R^T or R.  Substitution in any order: (T + dT) x^ = b with |dT| <= gamma_n |T|, so |T x^ - b| <= gamma_n |T||x^|; an inner
    product of length n in any order: |y^ - T z| <= gamma_n |T||z|.  One more index covers the host's own longdouble evaluation."""
    batch, nrhs = 2, 17
    Rs, Bs = _factors(n, kappa, 2), _rhs(n, nrhs, batch)
    g = np.longdouble(G.gamma(n + 1))
    for trans in (TRANS, NOTRANS):
        xs, _ = G.run("trsm", trans, Rs, Bs, (1, 3))
        ys, _ = G.run("trmm", trans, Rs, Bs, (1, 3))
        for i in range(batch):
            T = (Rs[i].T if trans else Rs[i]).astype(np.longdouble)
            x, b, y = xs[i].astype(np.longdouble), Bs[i].astype(np.longdouble), ys[i].astype(np.longdouble)
            assert np.isfinite(xs[i]).all() and np.isfinite(ys[i]).all()
            assert np.all(np.abs(T @ x - b) <= g * (np.abs(T) @ np.abs(x))), "trsm trans=%d block %d" % (trans, i)
            assert np.all(np.abs(y - T @ b) <= g * (np.abs(T) @ np.abs(b))), "trmm trans=%d block %d" % (trans, i)


# ---- 7. stream order ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    e = SO.Env(nstreams=1)
    yield e
    e.close()


@pytest.mark.parametrize("n", (33, 130))
@pytest.mark.parametrize("entry", ("trsm", "trmm"))
def test_fixed_size_entries_in_stream_order(env, entry, n):
    L = G.lib()
    batch, nrhs = 5, 17
    ldr, sr, ldb, sb = G.shape_of(n, nrhs, (1, 3))
    Rf = G.Flat([G.triangle(n, i) for i in range(batch)], ldr, sr, True)
    Bf = G.Flat(list(_rhs(n, nrhs, batch)), ldb, sb, False)
    bufs = {"R": Rf.host0, "B": Bf.host0, "info": np.zeros(batch, dtype=np.int32), "q": np.full(batch * nrhs, 5.0)}

    def enqueue(p, s):
        if entry == "trsm":
            return L.cap_dtrsm_batched(1, TRANS, n, nrhs, p["R"], ldr, sr, p["B"], ldb, sb, batch, p["info"], p["q"], nrhs, s)
        return L.cap_dtrmm_batched(1, NOTRANS, n, nrhs, p["R"], ldr, sr, p["B"], ldb, sb, batch, p["info"], s)
    job = SO.Job(bufs, enqueue, label=entry + "_batched")
    want, ret = env.plain(job)
    assert ret == 0 and np.isfinite(want["B"][Bf.touched]).all()
    with env.ordered(job, label="cap_d%s_batched n %d nrhs 17" % (entry, n)) as j:
        assert j.ret == 0
        for name in bufs:
            assert SO.same_bits(j.snap[name], want[name]), name
        assert SO.same_bits(j.snap["R"], Rf.host0) and not SO.same_bits(j.snap["B"], Bf.host0)
        assert (entry == "trsm") == (not SO.same_bits(j.snap["q"], bufs["q"]))


# ---- 8. the Python layer ------------------------------------------------------------------------------------------------------------------------
def _torch_blocks(Rs):
    """(batch, n, n) device tensor whose column-major reading of block i is Rs[i]: torch reads the transpose"""
    return torch.from_numpy(np.stack([r.T for r in Rs]).copy()).to(G.DEV)


@pytest.mark.parametrize("n", (9, 130))
def test_python_functions_give_the_bits_of_the_c_abi(n):
    from capital_amd import batched
    batch, nrhs = 3, 5
    Rs, Bs = _factors(n, 1e1, 3), _rhs(n, nrhs, batch)
    Rt = _torch_blocks(Rs)
    bt = lambda: torch.from_numpy(np.stack([b.T for b in Bs]).copy()).to(G.DEV)
    info = torch.tensor([0, 4, 0], dtype=torch.int32, device=G.DEV)
    for trans in (True, False):
        want, q = G.run("trsm", int(trans), Rs, Bs, info=[0, 4, 0], sumsq=True)
        B = bt()
        out, qq = batched.trsm(Rt, B, trans=trans, info=info, sumsq=True)
        assert out is B and qq.shape == (batch, nrhs)
        assert G.same(B.cpu().numpy(), np.stack([w.T for w in want])) and G.same(qq.cpu().numpy(), q)
        assert batched.trsm(Rt, bt(), trans=trans).shape == (batch, nrhs, n)
        want, _ = G.run("trmm", int(trans), Rs, Bs, info=[0, 4, 0])
        B = bt()
        assert batched.trmm(Rt, B, trans=trans, info=info) is B and G.same(B.cpu().numpy(), np.stack([w.T for w in want]))
    want, q = G.run("trsm", TRANS, Rs, [b[:, :1] for b in Bs], sumsq=True)
    b2 = torch.from_numpy(np.stack([b[:, 0] for b in Bs]).copy()).to(G.DEV)           # a 2-D B: one right-hand side per block
    d2 = batched.mahalanobis(Rt, b2)
    assert d2.shape == (batch,) and G.same(d2.cpu().numpy(), q[:, 0]) and G.same(b2.cpu().numpy(), np.stack([w[:, 0] for w in want]))
    assert torch.equal(Rt, _torch_blocks(Rs))


@pytest.mark.parametrize("n,fam", ((9, "F1"), (33, "F2"), (129, "F2i")))
def test_sampling_undoes_whitening_exactly_on_an_exact_row(n, fam):
    from capital_amd import batched
    ops = [TC.operands(fam, n, 3, i) for i in range(3)]
    Rt = _torch_blocks([o[0] for o in ops])
    B0 = np.stack([o[3].T for o in ops])                       # T^T X
    B = torch.from_numpy(B0.copy()).to(G.DEV)
    batched.trsm(Rt, B, trans=True)
    assert np.array_equal(_exact(B.cpu().numpy()), _exact(np.stack([o[2].T for o in ops])))
    batched.trmm(Rt, B, trans=True)
    assert np.array_equal(_exact(B.cpu().numpy()), _exact(B0))


def test_mahalanobis_against_numpy_on_five_by_five_blocks():
    """d^2 = b^T A^-1 b with x = np.linalg.solve(A, b).  The computed q^ is sum y^_r^2 with (R + dR)^T y^ = b, |dR| <= gamma_(n+1) |R| (the
    bound of the trsm test), so q^ = b^T (A + E)^-1 b with |E| <= ((1 + gamma_(n+1))^2 - 1) |R|^T |R| <= gamma_(2n+2) |R|^T |R| and, to first
    order, |q^ - d^2| = |x^T E x| <= gamma_(2n+2) sum_r (|R||x|)_r^2: the terms of the sum are the squares of the rows of |R||x|."""
    from capital_amd import batched
    n, batch, nrhs = 5, 6, 3
    A = P.random_spd(n, 1e1, batch)
    b = np.stack([np.random.default_rng([8, i]).standard_normal((nrhs, n)) for i in range(batch)])
    At, Bt = torch.from_numpy(A.copy()).to(G.DEV), torch.from_numpy(b.copy()).to(G.DEV)
    info, logdet = batched.potrf(At, logdet=True)
    q = batched.mahalanobis(At, Bt, info=info).cpu().numpy()
    Rh = np.triu(At.cpu().numpy().transpose(0, 2, 1))
    assert q.shape == (batch, nrhs) and not info.cpu().numpy().any()
    g = G.gamma(2 * n + 2)
    for i in range(batch):
        for k in range(nrhs):
            x = np.linalg.solve(A[i], b[i, k])
            d2 = float(b[i, k] @ x)
            terms = (np.abs(Rh[i]) @ np.abs(x)) ** 2
            assert abs(q[i, k] - d2) <= g * terms.sum(), (i, k, q[i, k], d2, abs(q[i, k] - d2) / (g * terms.sum()))
    # the Gaussian log-density of the recipe is finite
    dens = -0.5 * (q + logdet.cpu().numpy()[:, None] + n * math.log(2 * math.pi))
    assert np.isfinite(dens).all()
