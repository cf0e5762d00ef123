"""-m gpu: the batched Cholesky factor and solve for many small blocks (cap_dpotrf_batched / cap_dpotrs_batched, csrc/potrf_batched.hip)
through the C ABI, lapack.engine and capital_amd.batched.

Every device buffer starts as a fixed pattern of distinct NaN payloads and finite sentinels (the batched form of gpu_util.to_dev's NaN fill)
into which only the elements the call may read are written; afterwards everything the call must not write is compared as int64.

What is exact and what is bounded:
 * R with integer entries in [-3, 3] and a diagonal from {1, 2, 4}, A = R^T R: every intermediate of a Cholesky factorization of A in any
   order, with or without FMA, is a small integer, pivots are 1, 4 or 16 and quotients integers - the factor must equal R bit for bit, and
   so must X from B = A X with integer X in [-4, 4].  log det is compared with 2 sum log r_jj, added in the same ascending order with
   math.log: the additions are the same IEEE operations, the device logarithm may differ from math.log in the last place, hence 4 ulp of the
   sum are allowed (a sum of up to 64 non-negative terms each within one ulp of a term <= the sum).
 * random SPD blocks: Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3 / 10.4 with each constant one step looser (a device
   square root that is faithfully rather than correctly rounded): |A - R^T R| <= gamma_{n+2} |R|^T |R| and |B - A X| <= gamma_{3n+4} |R|^T
   |R| |X| componentwise, the residuals formed in np.longdouble."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV  # noqa: E402

UPPER = 1
U = 2.0 ** -53
SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)
BATCHES = (1, 2, 3, 5, 63, 64, 65, 257, 1000)
LAYOUTS = ((0, 0), (0, 3), (1, 3), (6, 0))          # (lda - n, stride - lda n): odd lda for even n, odd strides (blocks alternately 16-byte aligned)
NRHS = (1, 2, 3, 16, 17, 40)
GUARD = 37


def gamma(k):
    return k * U / (1 - k * U)


@pytest.fixture(scope="module")
def L():
    from capital_amd import _lib
    return _lib.lib()


def pattern(count):
    """`count` doubles: distinct NaN payloads, every fourth one a distinct finite sentinel"""
    p = np.arange(count, dtype=np.int64)
    bits = np.int64(0x7ff8000000000000) + 1 + p
    fin = (-1000.25 - p.astype(np.float64)).view(np.int64)
    return np.where(p % 4 == 3, fin, bits).view(np.float64)


def positions(n, ld, stride, batch, cols=None, tri=True):
    """flat offsets (batch, k) of the elements of each block a call may touch - the upper triangle of n x n, or all of n x cols - and the
    matching (row, col) index arrays"""
    cols = n if cols is None else cols
    r, c = np.triu_indices(n) if tri else [x.ravel() for x in np.meshgrid(np.arange(n), np.arange(cols), indexing="ij")]
    return np.arange(batch, dtype=np.int64)[:, None] * stride + (r + c * ld)[None, :], r, c


class Buf:
    """blocks[i][row, col] laid out column-major at i * stride (leading dimension ld) inside a pattern-filled buffer with a guard behind"""

    def __init__(self, blocks, ld, stride, tri=True, lower_nan=False):
        blocks = np.asarray(blocks, dtype=np.float64)
        self.batch, self.n, self.cols = blocks.shape
        self.ld, self.stride = ld, stride
        self.count = (self.batch - 1) * stride + ld * self.cols + GUARD
        self.pos, self.r, self.c = positions(self.n, ld, stride, self.batch, self.cols, tri)
        self.init = pattern(self.count)
        if lower_nan:                       # strictly lower triangles: NaN only (no finite sentinel a kernel could use unnoticed)
            lo = np.tril_indices(self.n, -1)
            lp = np.arange(self.batch, dtype=np.int64)[:, None] * stride + (lo[0] + lo[1] * ld)[None, :]
            self.init[lp] = np.nan
        self.init[self.pos] = blocks[:, self.r, self.c]
        self.dev = torch.from_numpy(self.init).to(DEV)
        self.other = np.ones(self.count, dtype=bool)
        self.other[self.pos.ravel()] = False

    def ptr(self):
        return self.dev.data_ptr()

    def host(self):
        return self.dev.cpu().numpy()

    def blocks(self, host=None):
        """(batch, n, cols) with zeros where the buffer holds no element of the block"""
        host = self.host() if host is None else host
        out = np.zeros((self.batch, self.n, self.cols))
        out[:, self.r, self.c] = host[self.pos]
        return out

    def assert_rest_untouched(self, host=None):
        host = self.host() if host is None else host
        a, b = host.view(np.int64)[self.other], self.init.view(np.int64)[self.other]
        assert np.array_equal(a, b), "%d elements outside the blocks were written" % int((a != b).sum())


def factor(L, buf, n, want_info=True, want_logdet=True):
    info = torch.full((buf.batch,), -7, dtype=torch.int32, device=DEV) if want_info else None
    logdet = torch.full((buf.batch,), 123.5, dtype=torch.float64, device=DEV) if want_logdet else None
    st = L.cap_dpotrf_batched(UPPER, n, buf.ptr(), buf.ld, buf.stride, buf.batch, info.data_ptr() if want_info else None,
                              logdet.data_ptr() if want_logdet else None, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return info, logdet


def solve(L, rbuf, bbuf, n, nrhs, info=None):
    st = L.cap_dpotrs_batched(UPPER, n, nrhs, rbuf.ptr(), rbuf.ld, rbuf.stride, bbuf.ptr(), bbuf.ld, bbuf.stride, rbuf.batch,
                              info.data_ptr() if info is not None else None, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()


_INT = {}


def integer_batch(n, batch):
    """(R, A, X, B, logdet) of `batch` different integer factors, drawn once per n and shared (read only)"""
    key = (n, batch > 1000)
    if key not in _INT:
        m = max(batch, 1000)
        rng = np.random.default_rng(1000 + n)
        R = np.triu(rng.integers(-3, 4, size=(m, n, n)), 1).astype(np.float64)
        dg = rng.choice([1.0, 2.0, 4.0], size=(m, n))
        R[:, np.arange(n), np.arange(n)] = dg
        A = np.matmul(R.transpose(0, 2, 1), R)
        X = rng.integers(-4, 5, size=(m, n, max(NRHS))).astype(np.float64)
        B = np.matmul(A, X)
        ld = np.zeros(m)
        for j in range(n):                                   # ascending j, one IEEE addition per term: as the kernel adds
            ld = ld + np.array([math.log(v) for v in dg[:, j]])
        for a in (R, A, X, B, ld):
            a.setflags(write=False)
        _INT[key] = (R, A, X, B, 2.0 * ld)
    return [a[:batch] for a in _INT[key]]


def check_logdet(got, want):
    got = np.asarray(got)
    assert np.all(np.abs(got - want) <= 4 * np.spacing(np.abs(want))), np.max(np.abs(got - want))


def exact_case(L, n, batch, dl, ds, nrhs_list):
    R, A, X, B, ld = integer_batch(n, batch)
    lda = n + dl
    buf = Buf(A, lda, lda * n + ds)
    info, logdet = factor(L, buf, n)
    host = buf.host()
    assert np.array_equal(buf.blocks(host), R), (n, batch, dl, ds)
    buf.assert_rest_untouched(host)
    assert not info.cpu().numpy().any()
    check_logdet(logdet.cpu().numpy(), ld)
    for nrhs in nrhs_list:
        ldb = n + dl
        bb = Buf(B[:, :, :nrhs], ldb, ldb * nrhs + ds, tri=False)
        solve(L, buf, bb, n, nrhs, info)
        hb = bb.host()
        assert np.array_equal(bb.blocks(hb), X[:, :, :nrhs]), (n, batch, dl, ds, nrhs)
        bb.assert_rest_untouched(hb)
    assert np.array_equal(buf.host().view(np.int64), host.view(np.int64))          # the solve writes nothing of R's buffer


@pytest.mark.parametrize("n", SIZES)
def test_exact_integer_factors_and_solutions(L, n):
    """1. factor == R, logdet, X == the integer solution, for every batch size and layout; and nothing outside the blocks is written"""
    for batch in BATCHES:
        for dl, ds in LAYOUTS:
            exact_case(L, n, batch, dl, ds, NRHS)


def test_exact_more_blocks_than_a_16_bit_grid(L):
    """batch = 70 000 at n = 4: more than 65 535 blocks in one grid dimension (9 MB)"""
    exact_case(L, 4, 70000, 0, 0, (1,))


@pytest.mark.parametrize("n,batch,dl,ds", [(5, 9, 3, 5), (16, 65, 1, 3), (33, 3, 6, 3), (64, 5, 1, 1)])
def test_nothing_else_is_touched(L, n, batch, dl, ds):
    """2. strictly lower triangles (all NaN here), pad rows, gaps between blocks, the guard behind the last block, rows >= n of B: identical
    as int64 after the factor and after the solve, with and without info / logdet"""
    R, A, X, B, _ = integer_batch(n, batch)
    lda = n + dl
    for want in (True, False):
        buf = Buf(A, lda, lda * n + ds, lower_nan=True)
        info, _ = factor(L, buf, n, want_info=want, want_logdet=want)
        host = buf.host()
        buf.assert_rest_untouched(host)
        assert np.array_equal(buf.blocks(host), R)
        for nrhs in (1, 17):
            bb = Buf(B[:, :, :nrhs], n + dl, (n + dl) * nrhs + ds, tri=False)
            solve(L, buf, bb, n, nrhs, info)
            hb = bb.host()
            bb.assert_rest_untouched(hb)
            assert np.array_equal(bb.blocks(hb), X[:, :, :nrhs])
        assert np.array_equal(buf.host().view(np.int64), host.view(np.int64))


def random_spd(rng, n, kappa, count=1):
    out = np.empty((count, n, n))
    for i in range(count):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        d = np.logspace(0, -math.log10(kappa), n) if n > 1 else np.ones(1)
        M = (Q * d) @ Q.T
        out[i] = (M + M.T) / 2
    return out


@pytest.mark.parametrize("n", (5, 16, 33, 64))
def test_position_and_layout_independence(L, n):
    """3. one random SPD block at every position of batches of 1, 7, 64 and 1000, at even and odd lda and stride, twice: one set of bits.
    The same for the solve with 1 and 17 right-hand sides; column k of the 17-column solve is the 1-column solve of that column."""
    rng = np.random.default_rng(7 + n)
    A1 = random_spd(rng, n, 1e3)
    B1 = rng.standard_normal((1, n, 17))
    ref = refx = None
    for batch in (1, 7, 64, 1000):
        for dl, ds in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 2)):
            lda = n + dl
            for rep in range(2 if batch == 7 else 1):
                buf = Buf(np.repeat(A1, batch, axis=0), lda, lda * n + ds)
                info, logdet = factor(L, buf, n)
                host = buf.host()
                got = host[buf.pos].view(np.int64)
                ref = got[0] if ref is None else ref
                assert np.array_equal(got, np.broadcast_to(ref, got.shape)), (batch, dl, ds, rep)
                lg = logdet.cpu().numpy().view(np.int64)
                assert (lg == lg[0]).all() and not info.cpu().numpy().any()
            xs = {}
            for nrhs in (1, 17):
                bb = Buf(np.repeat(B1[:, :, :nrhs], batch, axis=0), lda, lda * nrhs + ds, tri=False)
                solve(L, buf, bb, n, nrhs, info)
                x = bb.blocks().view(np.int64)
                assert np.array_equal(x, np.broadcast_to(x[0], x.shape)), (batch, dl, ds, nrhs)
                xs[nrhs] = x[0]
            refx = xs[17] if refx is None else refx
            assert np.array_equal(xs[17], refx) and np.array_equal(xs[1][:, 0], refx[:, 0]), (batch, dl, ds)
            if batch == 7 and dl == 1 and ds == 1:
                for k in range(1, 17):                       # every column on its own
                    bb = Buf(np.repeat(B1[:, :, k:k + 1], batch, axis=0), lda, lda + ds, tri=False)
                    solve(L, buf, bb, n, 1, None)
                    assert np.array_equal(bb.blocks().view(np.int64)[0][:, 0], refx[:, k]), k


@pytest.mark.parametrize("poison", ("zero", "nan"))
@pytest.mark.parametrize("n,batch", [(8, 131), (16, 70), (33, 9), (64, 6)])
def test_failing_blocks(L, n, batch, poison):
    """4. a pivot that is exactly 0 (or NaN) at step p in chosen blocks - the first, the last, two neighbours that share a wavefront when
    n <= 32: info = p + 1, the rows above p are R's, everything from row p on is NaN, logdet NaN, every other block as without failures;
    the solve gives NaN there with info and does not fault without it.  NaN is ordinary data: nothing here provokes a fault."""
    R, A, X, B, ld = integer_batch(n, batch)
    A = A.copy()
    ps = (0, 1, n // 2, n - 1)
    chosen = sorted({0, batch - 1, 2, 3, batch // 2})
    fail = {b: ps[i % 4] for i, b in enumerate(chosen)}
    for b, p in fail.items():
        A[b, p, p] = A[b, p, p] - R[b, p, p] ** 2 if poison == "zero" else np.nan
    for dl, ds in ((0, 0), (1, 3)):
        lda = n + dl
        clean = Buf(integer_batch(n, batch)[1], lda, lda * n + ds)
        factor(L, clean, n)
        buf = Buf(A, lda, lda * n + ds)
        info, logdet = factor(L, buf, n)
        host, hinfo, hld = buf.host(), info.cpu().numpy(), logdet.cpu().numpy()
        buf.assert_rest_untouched(host)
        got = host[buf.pos]
        good = np.array([b not in fail for b in range(batch)])
        assert np.array_equal(got[good].view(np.int64), clean.host()[clean.pos][good].view(np.int64))
        assert not hinfo[good].any()
        check_logdet(hld[good], ld[good])
        for b, p in fail.items():
            assert hinfo[b] == p + 1, (b, p, hinfo[b])
            assert np.isnan(hld[b])
            rows = buf.r
            assert np.array_equal(got[b][rows < p], R[b][buf.r, buf.c][rows < p]), (b, p)
            assert np.isnan(got[b][rows >= p]).all(), (b, p)
        for nrhs in (1, 17):
            for with_info in (True, False):
                bb = Buf(B[:, :, :nrhs], lda, lda * nrhs + ds, tri=False)
                solve(L, buf, bb, n, nrhs, info if with_info else None)
                hb = bb.host()
                bb.assert_rest_untouched(hb)
                x = bb.blocks(hb)
                assert np.array_equal(x[good], X[good][:, :, :nrhs])
                if with_info:
                    assert np.isnan(x[~good]).all()


@pytest.mark.parametrize("kappa", (1.0, 1e6, 1e12))
@pytest.mark.parametrize("n", (2, 8, 17, 33, 64))
def test_random_spd_within_the_proved_bounds(L, n, kappa):
    """5. A = Q diag(d) Q^T, batch 50: componentwise backward-error bounds of the factor and of the solve (residuals in np.longdouble), info = 0;
    at kappa = 1 also the forward bound kappa gamma_{n+2} ||R||_F against np.linalg.cholesky."""
    rng = np.random.default_rng(int(n * 100 + math.log10(kappa)))
    batch, nrhs = 50, 3
    A = random_spd(rng, n, kappa, batch)
    Bm = rng.standard_normal((batch, n, nrhs))
    lda = n + 1
    buf = Buf(A, lda, lda * n + 3)
    info, _ = factor(L, buf, n, want_logdet=False)
    assert not info.cpu().numpy().any()
    R = buf.blocks()
    bb = Buf(Bm, lda, lda * nrhs + 3, tri=False)
    solve(L, buf, bb, n, nrhs, info)
    Xc = bb.blocks()
    ld = np.longdouble
    Rl, Al, Xl, Bl = R.astype(ld), A.astype(ld), Xc.astype(ld), Bm.astype(ld)
    res = np.abs(Al - np.matmul(Rl.transpose(0, 2, 1), Rl))
    absR2 = np.matmul(np.abs(Rl).transpose(0, 2, 1), np.abs(Rl))
    bound = gamma(n + 2) * absR2
    print("n %d kappa %g: factor residual / bound = %.3f" % (n, kappa, float(np.max(res[bound > 0] / bound[bound > 0]))))
    assert np.all(res <= bound)
    res = np.abs(Bl - np.matmul(Al, Xl))
    bound = gamma(3 * n + 4) * np.matmul(absR2, np.abs(Xl))
    print("n %d kappa %g: solve residual / bound = %.3f" % (n, kappa, float(np.max(res[bound > 0] / bound[bound > 0]))))
    assert np.all(res <= bound)
    if kappa == 1.0:
        for i in range(batch):
            ref = np.linalg.cholesky(A[i]).T
            assert np.linalg.norm(R[i] - ref) <= kappa * gamma(n + 2) * np.linalg.norm(ref), i


def test_python_layers(L):
    """6. capital_amd.batched on torch tensors (in torch's reading the lower triangle takes L, the upper one stays), lapack.engine gives the
    C calls' bits, wrong dtype / device / strides raise CapitalError"""
    from capital_amd import _lib, batched, lapack
    rng = np.random.default_rng(42)
    n, batch, nrhs = 19, 33, 5
    for kappa in (1.0, 1e6):
        A = random_spd(rng, n, kappa, batch)
        Bm = rng.standard_normal((batch, nrhs, n))
        base = torch.full((batch, n, n + 3), float("nan"), dtype=torch.float64, device=DEV)
        T = base[:, :, :n]
        T.copy_(torch.from_numpy(A))
        info, logdet = batched.potrf(T, logdet=True)
        out = T.cpu().numpy()
        assert not info.cpu().numpy().any()
        iu = np.triu_indices(n, 1)
        assert np.array_equal(out[:, iu[0], iu[1]].view(np.int64), A[:, iu[0], iu[1]].view(np.int64))     # torch's upper triangle: untouched
        assert torch.isnan(base[:, :, n:]).all()
        Lw = np.tril(out)
        ld = np.longdouble
        res = np.abs(A.astype(ld) - np.matmul(Lw.astype(ld), Lw.astype(ld).transpose(0, 2, 1)))
        assert np.all(res <= gamma(n + 2) * np.matmul(np.abs(Lw), np.abs(Lw).transpose(0, 2, 1)).astype(ld))
        if kappa == 1.0:
            for i in range(batch):
                ref = np.linalg.cholesky(A[i])
                assert np.linalg.norm(Lw[i] - ref) <= gamma(n + 2) * np.linalg.norm(ref)
        assert np.allclose(logdet.cpu().numpy(), np.linalg.slogdet(A)[1], rtol=0, atol=1e-9 * max(1.0, math.log10(kappa)) * n)
        Bt = torch.from_numpy(Bm).to(DEV)
        assert batched.potrs(T, Bt, info) is Bt
        Xc = Bt.cpu().numpy().transpose(0, 2, 1)
        res = np.abs(Bm.transpose(0, 2, 1).astype(ld) - np.matmul(A.astype(ld), Xc.astype(ld)))
        absR2 = np.matmul(np.abs(Lw), np.abs(Lw).transpose(0, 2, 1))
        assert np.all(res <= gamma(3 * n + 4) * np.matmul(absR2, np.abs(Xc)).astype(ld))
        b1 = torch.from_numpy(np.ascontiguousarray(Bm[:, 2, :])).to(DEV)
        batched.potrs(T, b1)
        assert np.array_equal(b1.cpu().numpy().view(np.int64), Bt.cpu().numpy()[:, 2, :].view(np.int64))
        # the engine and the C call: same bits
        T2 = torch.from_numpy(A).to(DEV)
        pf = lapack.ArgPack_potrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
        ps = lapack.ArgPack_potrs_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
        info2, ld2 = lapack.engine._potrf_batched(T2, n, n, n * n, batch, pf, want_logdet=True)
        assert isinstance(info2, torch.Tensor) and info2.is_cuda and ld2.is_cuda
        T3 = torch.from_numpy(A).to(DEV)
        i3 = torch.zeros(batch, dtype=torch.int32, device=DEV)
        l3 = torch.zeros(batch, dtype=torch.float64, device=DEV)
        assert L.cap_dpotrf_batched(UPPER, n, T3.data_ptr(), n, n * n, batch, i3.data_ptr(), l3.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(T2.cpu().numpy().view(np.int64), T3.cpu().numpy().view(np.int64))
        assert np.array_equal(ld2.cpu().numpy().view(np.int64), l3.cpu().numpy().view(np.int64)) and np.array_equal(info2.cpu().numpy(), i3.cpu().numpy())
        assert np.array_equal(np.tril(T2.cpu().numpy()).view(np.int64), Lw.view(np.int64))                 # and batched.potrf's
        B2, B3 = torch.from_numpy(Bm).to(DEV), torch.from_numpy(Bm).to(DEV)
        lapack.engine._potrs_batched(T2, B2, n, nrhs, n, n * n, n, n * nrhs, batch, info2, ps)
        assert L.cap_dpotrs_batched(UPPER, n, nrhs, T3.data_ptr(), n, n * n, B3.data_ptr(), n, n * nrhs, batch, i3.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(B2.cpu().numpy().view(np.int64), B3.cpu().numpy().view(np.int64))
        assert np.array_equal(B2.cpu().numpy().view(np.int64), Bt.cpu().numpy().view(np.int64))
    good = torch.from_numpy(random_spd(rng, 4, 10.0, 3)).to(DEV)
    for bad in (good.cpu(), good.float(), good.transpose(1, 2).contiguous().transpose(1, 2), good[0], good[:, :, :3]):
        with pytest.raises(_lib.CapitalError):
            batched.potrf(bad)
    rhs = torch.ones(3, 2, 4, dtype=torch.float64, device=DEV)
    for bad in (rhs.cpu(), rhs.float(), rhs.transpose(1, 2).contiguous().transpose(1, 2), rhs[:2], torch.ones(3, 2, 5, dtype=torch.float64, device=DEV)):
        with pytest.raises(_lib.CapitalError):
            batched.potrs(good, bad)
    with pytest.raises(_lib.CapitalError):
        batched.potrs(good, rhs, info=torch.zeros(3, dtype=torch.int64, device=DEV))
