"""-m gpu: the batched Cholesky factor and solve for blocks of 65 .. 256 rows (cap_dpotrf_batched_blocked / cap_dpotrs_batched_blocked,
csrc/potrf_batched_blocked.hip) through the C ABI, lapack.engine and capital_amd.batched.

The method is that of tests/test_gpu_potrf_batched.py, whose helpers are used: every device buffer starts as a pattern of distinct NaN
payloads and finite sentinels into which only the elements a call may read are written (NaN in the strictly lower triangles), a guard lies
behind the last block, and afterwards everything a call must not write is compared as int64.

What is exact and what is bounded:
 * R with integer entries in [-3, 3] and a diagonal from {1, 2, 4}, A = R^T R, integer X in [-4, 4], B = A X: every intermediate of a
   substitution-based Cholesky factorization and solve is an integer far below 2^53 - the factor must equal R and the solution X bit for bit.
 * random SPD blocks A = G^T G + n I (condition number about 5): |A - R^T R| <= gamma_{n+2} |R|^T |R| and |B - A X| <= gamma_{3n+4} |R|^T |R|
   |X| componentwise (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3 / 10.4, each constant one step looser), residuals in
   np.longdouble.  These hold for any summation order, the MFMA's included.
 * logdet against the np.longdouble sum 2 sum log r_jj of the device's own diagonal: gamma_{n+2} 2 sum |log r_jj| - n - 1 additions in
   recursive summation (gamma_{n-1}), a logarithm within one ulp (2u per term), the doubling exact.
 * against torch.linalg.cholesky: two factors of the same A, each with a backward error ||dA||_F <= gamma_{n+2} || |R|^T |R| ||_F <=
   n gamma_{n+2} ||A||_2 (Higham eq. 10.7), differ by at most 2 * 2^-1/2 kappa_2(A) n gamma_{n+2} ||R||_2 in the Frobenius norm to first
   order (Sun's perturbation bound, Higham Thm 10.8); the test allows exactly that with kappa_2 from numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import DEV  # noqa: E402
from tests.test_gpu_potrf_batched import Buf, gamma  # noqa: E402

UPPER = 1
SIZES = (65, 66, 79, 80, 81, 96, 127, 128, 129, 191, 192, 193, 255, 256)
LAYOUTS = ((0, 0), (0, 3), (1, 3), (6, 0))          # (lda - n, stride - lda n)
NRHS = (1, 2, 15, 16, 17, 64, 65, 100)
LD = np.longdouble


@pytest.fixture(scope="module")
def L():
    from capital_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def factor(L, buf, n, old=False):
    info = torch.full((buf.batch,), -7, dtype=torch.int32, device=DEV)
    logdet = torch.full((buf.batch,), 123.5, dtype=torch.float64, device=DEV)
    fn = L.cap_dpotrf_batched if old else L.cap_dpotrf_batched_blocked
    assert fn(UPPER, n, buf.ptr(), buf.ld, buf.stride, buf.batch, info.data_ptr(), logdet.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    return info, logdet


def solve(L, rbuf, bbuf, n, nrhs, info=None, old=False):
    fn = L.cap_dpotrs_batched if old else L.cap_dpotrs_batched_blocked
    assert fn(UPPER, n, nrhs, rbuf.ptr(), rbuf.ld, rbuf.stride, bbuf.ptr(), bbuf.ld, bbuf.stride, rbuf.batch,
              info.data_ptr() if info is not None else None, stream()) == 0
    torch.cuda.synchronize()


_INT = {}


def integer_batch(n, batch):
    """(R, A, X, B) of `batch` different integer factors with max(NRHS) right-hand sides, drawn once per (n, batch) and shared (read only)"""
    if (n, batch) not in _INT:
        rng = np.random.default_rng(2000 + n)
        R = np.triu(rng.integers(-3, 4, size=(batch, n, n)), 1).astype(np.float64)
        R[:, np.arange(n), np.arange(n)] = rng.choice([1.0, 2.0, 4.0], size=(batch, n))
        A = np.matmul(R.transpose(0, 2, 1), R)
        X = rng.integers(-4, 5, size=(batch, n, max(NRHS))).astype(np.float64)
        B = np.matmul(A, X)
        for a in (R, A, X, B):
            a.setflags(write=False)
        _INT[(n, batch)] = (R, A, X, B)
    return _INT[(n, batch)]


def random_spd(rng, n, count):
    G = rng.standard_normal((count, n, n))
    A = np.matmul(G.transpose(0, 2, 1), G) + n * np.eye(n)
    return (A + A.transpose(0, 2, 1)) / 2


def check_logdet(got, Rdev):
    """got[i] against 2 sum_j log r_jj of the device's own factor in np.longdouble"""
    n = Rdev.shape[1]
    lg = np.log(np.diagonal(Rdev, axis1=1, axis2=2).astype(LD))
    want, scale = 2 * lg.sum(axis=1), 2 * np.abs(lg).sum(axis=1)
    err = np.abs(np.asarray(got).astype(LD) - want)
    print("n %d: logdet error / bound = %.3g" % (n, float(np.max(err / np.maximum(gamma(n + 2) * scale, LD(1e-300))))))
    assert np.all(err <= gamma(n + 2) * scale), (err, gamma(n + 2) * scale)


def factor_residual_ok(A, R, rows=None, tag=""):
    """|A - R^T R| <= gamma_{n+2} |R|^T |R| on the upper triangle, restricted to the first `rows` rows of R when given (the later ones zeroed:
    element (i, j), i <= j, of R^T R takes rows 0 .. i of R only)"""
    n = A.shape[-1]
    Rl = np.array(R, dtype=LD)
    if rows is not None:
        Rl[rows:, :] = 0
    res = np.abs(A.astype(LD) - Rl.T @ Rl)
    bound = gamma(n + 2) * (np.abs(Rl).T @ np.abs(Rl))
    iu = np.triu_indices(n)
    keep = iu[0] < (n if rows is None else rows)
    res, bound = res[iu][keep], bound[iu][keep]
    if res.size:
        print("%s n %d: factor residual / bound = %.3f" % (tag, n, float(np.max(res[bound > 0] / bound[bound > 0]))))
    assert np.all(res <= bound)


def solve_residual_ok(A, R, X, Bm, tag=""):
    n = A.shape[-1]
    Rl, Xl = R.astype(LD), X.astype(LD)
    res = np.abs(Bm.astype(LD) - A.astype(LD) @ Xl)
    bound = gamma(3 * n + 4) * ((np.abs(Rl).T @ np.abs(Rl)) @ np.abs(Xl))
    print("%s n %d: solve residual / bound = %.3f" % (tag, n, float(np.max(res[bound > 0] / bound[bound > 0]))))
    assert np.all(res <= bound)


def exact_case(L, n, batch, dl, ds, nrhs_list):
    R, A, X, B = integer_batch(n, batch)
    lda = n + dl
    buf = Buf(A, lda, lda * n + ds, lower_nan=True)
    info, logdet = factor(L, buf, n)
    host = buf.host()
    got = buf.blocks(host)
    assert np.array_equal(got.view(np.int64), R.view(np.int64)), (n, batch, dl, ds, int((got != R).sum()))
    buf.assert_rest_untouched(host)
    assert not info.cpu().numpy().any()
    check_logdet(logdet.cpu().numpy(), got)
    for nrhs in nrhs_list:
        bb = Buf(B[:, :, :nrhs], lda, lda * nrhs + ds, tri=False)
        solve(L, buf, bb, n, nrhs, info)
        hb = bb.host()
        gx = bb.blocks(hb)
        assert np.array_equal(gx.view(np.int64), X[:, :, :nrhs].view(np.int64)), (n, batch, dl, ds, nrhs, int((gx != X[:, :, :nrhs]).sum()))
        bb.assert_rest_untouched(hb)
    assert np.array_equal(buf.host().view(np.int64), host.view(np.int64))          # the solve writes nothing of R's buffer


@pytest.mark.parametrize("n", SIZES)
def test_exact_integer_factors_and_solutions(L, n):
    """factor == R and X == the integer solution bit for bit, nothing outside the permitted elements is written: every size with batches 1, 2, 3
    over the four layouts, two of the eight right-hand side counts with each layout, so that every size meets every count"""
    k = SIZES.index(n)
    for b, (batch, (dl, ds)) in enumerate(zip((1, 2, 3, 2), LAYOUTS)):
        exact_case(L, n, batch, dl, ds, (NRHS[(k + 2 * b) % 8], NRHS[(k + 2 * b + 1) % 8]))


@pytest.mark.parametrize("n,dl,ds,nrhs", [(65, 1, 3, (17,)), (129, 0, 3, (1, 65)), (192, 6, 0, (16,)), (256, 0, 0, (1, 100))])
def test_exact_more_blocks_than_compute_units(L, n, dl, ds, nrhs):
    """batch = 257, one more than the chip has compute units"""
    exact_case(L, n, 257, dl, ds, nrhs)


@pytest.mark.parametrize("n", SIZES)
def test_random_spd_within_the_proved_bounds(L, n):
    rng = np.random.default_rng(300 + n)
    batch, nrhs = 2, 3
    A = random_spd(rng, n, batch)
    Bm = rng.standard_normal((batch, n, nrhs))
    lda = n + 1
    buf = Buf(A, lda, lda * n + 3, lower_nan=True)
    info, logdet = factor(L, buf, n)
    assert not info.cpu().numpy().any()
    host = buf.host()
    buf.assert_rest_untouched(host)
    R = buf.blocks(host)
    bb = Buf(Bm, lda, lda * nrhs + 3, tri=False)
    solve(L, buf, bb, n, nrhs, info)
    hb = bb.host()
    bb.assert_rest_untouched(hb)
    Xc = bb.blocks(hb)
    for i in range(batch):
        factor_residual_ok(A[i], R[i])
        solve_residual_ok(A[i], R[i], Xc[i], Bm[i])
    check_logdet(logdet.cpu().numpy(), R)


@pytest.mark.parametrize("k", (1, 64, 65, 66, 128, 129, 193))
def test_failing_blocks(L, k):
    """a batch of five at n = 193 whose blocks 1 and 3 have an indefinite leading minor of order k (its Schur pivot is about -1): info = k, the
    rows before k within the factor bound, row k and every later one NaN, logdet NaN, potrs gives NaN there; the three healthy blocks are
    bit for bit what a batch of their own gives.  NaN is ordinary data: nothing here provokes a fault."""
    n, batch, nrhs = 193, 5, 2
    rng = np.random.default_rng(500 + k)
    A = random_spd(rng, n, batch)
    Bm = rng.standard_normal((batch, n, nrhs))
    fail, good = (1, 3), (0, 2, 4)
    for b in fail:
        if k == 1:
            A[b, 0, 0] = -1.0
        else:
            w = np.linalg.solve(np.linalg.cholesky(A[b, :k - 1, :k - 1]), A[b, :k - 1, k - 1])
            A[b, k - 1, k - 1] = w @ w - 1.0
    lda = n + 1
    buf = Buf(A, lda, lda * n + 3, lower_nan=True)
    info, logdet = factor(L, buf, n)
    host, hinfo, hld = buf.host(), info.cpu().numpy(), logdet.cpu().numpy()
    buf.assert_rest_untouched(host)
    R = buf.blocks(host)
    own = Buf(A[list(good)], lda, lda * n + 3, lower_nan=True)
    oinfo, old = factor(L, own, n)
    assert np.array_equal(host[buf.pos][list(good)].view(np.int64), own.host()[own.pos].view(np.int64))
    assert np.array_equal(hld[list(good)].view(np.int64), old.cpu().numpy().view(np.int64))
    assert not hinfo[list(good)].any() and not oinfo.cpu().numpy().any()
    for b in fail:
        assert hinfo[b] == k, (b, k, hinfo[b])
        assert np.isnan(hld[b])
        got = host[buf.pos][b]
        assert np.isnan(got[buf.r >= k - 1]).all() and not np.isnan(got[buf.r < k - 1]).any()
        factor_residual_ok(A[b], R[b], rows=k - 1, tag="k %d" % k)
    bb = Buf(Bm, lda, lda * nrhs + 3, tri=False)
    solve(L, buf, bb, n, nrhs, info)
    hb = bb.host()
    bb.assert_rest_untouched(hb)
    x = bb.blocks(hb)
    assert np.isnan(x[list(fail)]).all() and not np.isnan(x[list(good)]).any()
    for b in good:
        solve_residual_ok(A[b], R[b], x[b], Bm[b])
    nb = Buf(Bm, lda, lda * nrhs + 3, tri=False)                 # without info: NaN from the factor's NaN rows, no fault, the rest as before
    solve(L, buf, nb, n, nrhs, None)
    assert np.array_equal(nb.blocks()[list(good)].view(np.int64), x[list(good)].view(np.int64))


@pytest.mark.parametrize("n", (81, 200))
def test_bits_depend_on_n_and_data_only(L, n):
    """one random block at positions 0, 1 and 256 of a batch of 257 (other data around it), alone, and in every layout: one set of bits for
    the factor, logdet and the solve; column 3 of a 17-column solve == that column alone == the same column as column 70 of 100"""
    rng = np.random.default_rng(900 + n)
    A1 = random_spd(rng, n, 1)[0]
    others = random_spd(rng, n, 3)
    B100 = rng.standard_normal((n, 100))
    col = B100[:, 70].copy()
    B17 = rng.standard_normal((n, 17))
    B17[:, 3] = col
    big = others[np.arange(257) % 3].copy()
    where = (0, 1, 256)
    big[list(where)] = A1
    ref = refld = refx = None
    cases = [(big, where, 0, 0)] + [(np.stack([A1]), (0,), dl, ds) for dl, ds in LAYOUTS] + [(np.stack([others[0], A1, others[1]]), (1,), 1, 3)]
    for blocks, at, dl, ds in cases:
        lda, batch = n + dl, len(blocks)
        buf = Buf(blocks, lda, lda * n + ds, lower_nan=True)
        info, logdet = factor(L, buf, n)
        host = buf.host()
        buf.assert_rest_untouched(host)
        assert not info.cpu().numpy().any()
        got, lg = host[buf.pos].view(np.int64), logdet.cpu().numpy().view(np.int64)
        ref, refld = (got[at[0]], lg[at[0]]) if ref is None else (ref, refld)
        for b in at:
            assert np.array_equal(got[b], ref) and lg[b] == refld, (batch, b, dl, ds)
        if batch > 3:
            continue
        for rhs, j in ((B17, 3), (col[:, None], 0), (B100, 70)):
            nrhs = rhs.shape[1]
            bb = Buf(np.repeat(rhs[None], batch, axis=0), lda, lda * nrhs + ds, tri=False)
            solve(L, buf, bb, n, nrhs, info)
            x = bb.blocks()[at[0]][:, j].view(np.int64)
            refx = x if refx is None else refx
            assert np.array_equal(x, refx), (batch, dl, ds, nrhs)
    solve_residual_ok(A1, buf.blocks()[1], refx.view(np.float64)[:, None], col[:, None])


@pytest.mark.parametrize("n", (8, 33, 64))
def test_small_blocks_are_forwarded(L, n):
    """n <= 64: the new entries run the existing kernels - identical bits for factor, info, logdet and solve (one block of the batch fails)"""
    rng = np.random.default_rng(40 + n)
    batch, nrhs = 9, 17
    A = random_spd(rng, n, batch)
    A[4, n // 2, n // 2] = -1.0
    Bm = rng.standard_normal((batch, n, nrhs))
    out = []
    for old in (False, True):
        buf = Buf(A, n + 1, (n + 1) * n + 3, lower_nan=True)
        info, logdet = factor(L, buf, n, old=old)
        bb = Buf(Bm, n + 1, (n + 1) * nrhs + 3, tri=False)
        solve(L, buf, bb, n, nrhs, info, old=old)
        out.append((buf.host().view(np.int64), info.cpu().numpy(), logdet.cpu().numpy().view(np.int64), bb.host().view(np.int64)))
    assert out[0][1][4] == n // 2 + 1
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", (65, 200, 256))
def test_python_layers(L, n):
    """capital_amd.batched on torch tensors, lapack.engine and the C entry: the same bits for factor, info, logdet and solve; in torch's
    reading the lower triangle holds torch.linalg.cholesky's L within the bound of the docstring above, the upper one is untouched"""
    from capital_amd import batched, lapack
    rng = np.random.default_rng(70 + n)
    batch, nrhs = 3, 5
    A = random_spd(rng, n, batch)
    Bm = rng.standard_normal((batch, nrhs, n))
    T = torch.from_numpy(A).to(DEV)
    info, logdet = batched.potrf(T, logdet=True)
    out = T.cpu().numpy()
    assert not info.cpu().numpy().any()
    iu = np.triu_indices(n, 1)
    assert np.array_equal(out[:, iu[0], iu[1]].view(np.int64), A[:, iu[0], iu[1]].view(np.int64))     # torch's upper triangle: untouched
    Lw = np.tril(out)
    Lt = torch.linalg.cholesky(torch.from_numpy(A).to(DEV)).cpu().numpy()
    for i in range(batch):
        factor_residual_ok(A[i], Lw[i].T)
        s = np.linalg.svd(A[i], compute_uv=False)
        allowed = 2 * 2 ** -0.5 * (s[0] / s[-1]) * n * gamma(n + 2) * np.sqrt(s[0])
        print("n %d: ||L - L_torch||_F / allowed = %.3g" % (n, np.linalg.norm(Lw[i] - Lt[i]) / allowed))
        assert np.linalg.norm(Lw[i] - Lt[i]) <= allowed
    Bt = torch.from_numpy(Bm).to(DEV)
    assert batched.potrs(T, Bt, info) is Bt
    Xc = Bt.cpu().numpy().transpose(0, 2, 1)
    for i in range(batch):
        solve_residual_ok(A[i], Lw[i].T, Xc[i], Bm[i].T)
    pf = lapack.ArgPack_potrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    ps = lapack.ArgPack_potrs_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    T2 = torch.from_numpy(A).to(DEV)
    info2, ld2 = lapack.engine._potrf_batched(T2, n, n, n * n, batch, pf, want_logdet=True)
    T3 = torch.from_numpy(A).to(DEV)
    i3 = torch.zeros(batch, dtype=torch.int32, device=DEV)
    l3 = torch.zeros(batch, dtype=torch.float64, device=DEV)
    assert L.cap_dpotrf_batched_blocked(UPPER, n, T3.data_ptr(), n, n * n, batch, i3.data_ptr(), l3.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    for t in (T2, T3):
        assert np.array_equal(t.cpu().numpy().view(np.int64), out.view(np.int64))
    for l in (ld2, l3):
        assert np.array_equal(l.cpu().numpy().view(np.int64), logdet.cpu().numpy().view(np.int64))
    assert np.array_equal(info2.cpu().numpy(), i3.cpu().numpy())
    B2, B3 = torch.from_numpy(Bm).to(DEV), torch.from_numpy(Bm).to(DEV)
    lapack.engine._potrs_batched(T2, B2, n, nrhs, n, n * n, n, n * nrhs, batch, info2, ps)
    assert L.cap_dpotrs_batched_blocked(UPPER, n, nrhs, T3.data_ptr(), n, n * n, B3.data_ptr(), n, n * nrhs, batch, i3.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    for b in (B2, B3):
        assert np.array_equal(b.cpu().numpy().view(np.int64), Bt.cpu().numpy().view(np.int64))


def test_more_than_256_rows_are_refused(L):
    from capital_amd import _lib, batched
    T = torch.eye(257, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
    with pytest.raises(_lib.CapitalError, match="256"):
        batched.potrf(T)
    with pytest.raises(_lib.CapitalError, match="256"):
        batched.potrs(T, torch.ones(2, 257, dtype=torch.float64, device=DEV))
    assert np.array_equal(T.cpu().numpy(), np.tile(np.eye(257), (2, 1, 1)))
