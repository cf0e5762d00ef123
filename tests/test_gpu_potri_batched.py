"""-m gpu: the batched triangular inverse and SPD inverse (cap_dtrtri_batched / cap_dpotri_batched, csrc/potri_batched.hip) through the C ABI,
lapack.engine and capital_amd.batched.

The method is that of tests/test_gpu_potrf_batched.py, whose Buf is used: every device buffer starts as a pattern of distinct NaN payloads
and finite sentinels, the strictly lower triangles hold NaN only, a guard follows the last block; afterwards everything the call must not
write is compared as int64.

What is exact and what is bounded:
 * the operand families of tests/potri_batched_cases.py (tri_cases' F1 / F2 / F2i with a seed per block): under the asserted premise every
   value the inverse, the triangular product and the factorization of T^T T form is a dyadic rational below 2^53, so T^-1 and
   triu(T^-1 T^-T) must come out bit for bit (after -0 -> +0), whatever the order of the block steps - a block overwritten while a later
   step still needs its old value shows as a wrong bit.
 * random SPD blocks, factored by the library's own batched factor, against a reference formed in np.longdouble from the device's R:
   |W - W*| <= gamma_3n |W*||R||W*| and |X - X*| <= gamma_8n |W*||R||W*||W*|^T componentwise on the upper triangle (the derivation is in
   potri_batched_cases.reference / the issue; LAPACK on the CPU uses a few percent of either, tests/test_potri_batched_cases.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import potri_batched_cases as P  # noqa: E402
from tests.gpu_util import DEV  # noqa: E402
from tests.test_gpu_potrf_batched import Buf  # noqa: E402
from tests.tri_cases import positive_zero  # noqa: E402

UPPER = 1
ROWS = P.exact_rows()


@pytest.fixture(scope="module")
def L():
    from capital_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None else None


def trtri(L, buf, n, info=None):
    assert L.cap_dtrtri_batched(UPPER, n, buf.ptr(), buf.ld, buf.stride, buf.batch, ptr(info), stream()) == 0
    torch.cuda.synchronize()


def potri(L, buf, n, info=None, fill=0):
    assert L.cap_dpotri_batched(UPPER, n, buf.ptr(), buf.ld, buf.stride, buf.batch, ptr(info), fill, stream()) == 0
    torch.cuda.synchronize()


def factor(L, buf, n):
    info = torch.full((buf.batch,), -7, dtype=torch.int32, device=DEV)
    fn = L.cap_dpotrf_batched if n <= 64 else L.cap_dpotrf_batched_blocked
    assert fn(UPPER, n, buf.ptr(), buf.ld, buf.stride, buf.batch, info.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    return info


def tri_buf(blocks, n, dl, ds):
    """upper triangles in a pattern buffer, NaN-only strictly lower triangles"""
    ld = n + dl
    return Buf(blocks, ld, ld * n + ds, lower_nan=True)


def win_buf(blocks, n, dl, ds):
    """whole n x n windows (fill = 1), the strictly lower triangles of the input NaN"""
    ld = n + dl
    return Buf(P.stored(blocks), ld, ld * n + ds, tri=False)


def same_bits(got, want):
    return np.array_equal(positive_zero(got).view(np.int64), positive_zero(want).view(np.int64))


def check_upper(buf, want, what):
    host = buf.host()
    got = buf.blocks(host)
    iu = np.triu_indices(buf.n)
    bad = [i for i in range(buf.batch) if not same_bits(got[i][iu], want[i][iu])]
    assert not bad, "%s: blocks %s differ" % (what, bad[:8])
    buf.assert_rest_untouched(host)
    return got


def check_window(buf, want, what):
    """fill = 1: upper triangle == want, strictly lower == its bitwise mirror, nothing outside the windows written"""
    host = buf.host()
    got = buf.blocks(host)
    iu, il = np.triu_indices(buf.n), np.tril_indices(buf.n, -1)
    for i in range(buf.batch):
        assert same_bits(got[i][iu], want[i][iu]), "%s: block %d differs" % (what, i)
        assert np.array_equal(got[i][il].view(np.int64), got[i].T[il].view(np.int64)), "%s: block %d is not mirrored bit for bit" % (what, i)
    buf.assert_rest_untouched(host)


@pytest.mark.parametrize("row", ROWS, ids=P.row_id)
def test_trtri_exact(L, row):
    """1. signed diagonals: the upper triangles equal T^-1 bit for bit, everything else in the buffer is untouched"""
    n, fam, batch, (dl, ds) = row
    T, Ti, _ = P.batch(fam, n, True, batch)
    buf = tri_buf(T, n, dl, ds)
    trtri(L, buf, n)
    check_upper(buf, Ti, "trtri %s" % (row,))


@pytest.mark.parametrize("row", ROWS, ids=P.row_id)
def test_potri_exact(L, row):
    """2. positive diagonals as R: triu(T^-1 T^-T) bit for bit; with fill = 1 the lower triangle is the bitwise mirror and the pad rows,
    gaps and guard are untouched"""
    n, fam, batch, (dl, ds) = row
    T, _, C = P.batch(fam, n, False, batch)
    buf = tri_buf(T, n, dl, ds)
    potri(L, buf, n)
    check_upper(buf, C, "potri %s" % (row,))
    buf = win_buf(T, n, dl, ds)
    potri(L, buf, n, fill=1)
    check_window(buf, C, "potri fill=1 %s" % (row,))


@pytest.mark.parametrize("row", ROWS, ids=P.row_id)
def test_factor_then_invert_exact(L, row):
    """3. A = T^T T (exact under the premise; pivots 1/16 .. 16 with exact square roots) through the batched factor, then the inverse:
    triu(T^-1 T^-T) bit for bit"""
    n, fam, batch, (dl, ds) = row
    T, _, C = P.batch(fam, n, False, batch)
    A = np.matmul(T.transpose(0, 2, 1), T)
    buf = tri_buf(A, n, dl, ds)
    info = factor(L, buf, n)
    assert not info.cpu().numpy().any()
    assert same_bits(buf.blocks()[:, np.triu_indices(n)[0], np.triu_indices(n)[1]], T[:, np.triu_indices(n)[0], np.triu_indices(n)[1]])
    potri(L, buf, n, info)
    check_upper(buf, C, "chain %s" % (row,))


@pytest.mark.parametrize("n,batch", [(5, 19), (33, 7), (64, 5), (100, 5), (256, 4)])
def test_failed_blocks(L, n, batch):
    """4. blocks with info != 0 (from a real failing factor, and from a hand-set info) are NaN exactly where the call writes - the triangle,
    or the window with fill = 1 - and their neighbours are bit-identical to a run without them; info = NULL treats every block as good"""
    T, Ti, C = P.batch("F1", n, False, batch)
    iu, il = np.triu_indices(n), np.tril_indices(n, -1)
    A = np.matmul(T.transpose(0, 2, 1), T)
    fail = sorted({0, batch // 2, batch - 1} if batch > 4 else {1})
    good = [i for i in range(batch) if i not in fail]
    for k, b in enumerate(fail):
        p = (0, n // 2, n - 1)[k % 3]
        A[b, p, p] = -1.0
    for fill in (0, 1):
        buf = (win_buf if fill else tri_buf)(A, n, 1, 3)
        info = factor(L, buf, n)
        hi = info.cpu().numpy()
        assert all(hi[b] != 0 for b in fail) and not hi[good].any()
        potri(L, buf, n, info, fill)
        host = buf.host()
        got = buf.blocks(host)
        buf.assert_rest_untouched(host)
        for b in fail:
            assert np.isnan(got[b][iu]).all()
            if fill:
                assert np.isnan(got[b]).all()
        for b in good:
            assert same_bits(got[b][iu], C[b][iu])
            if fill:
                assert np.array_equal(got[b][il].view(np.int64), got[b].T[il].view(np.int64))
    # a hand-set info on good factors, for both entries; then the same buffers with info = NULL
    hand = np.zeros(batch, dtype=np.int32)
    hand[fail] = 7
    info = torch.from_numpy(hand).to(DEV)
    for op, want in ((trtri, Ti), (potri, C)):
        buf = tri_buf(T, n, 1, 3)
        op(L, buf, n, info)
        host = buf.host()
        got = buf.blocks(host)
        buf.assert_rest_untouched(host)
        for b in range(batch):
            assert np.isnan(got[b][iu]).all() if b in fail else same_bits(got[b][iu], want[b][iu])
        buf = tri_buf(T, n, 1, 3)
        op(L, buf, n, None)
        check_upper(buf, want, "info = NULL")


@pytest.mark.parametrize("kappa", P.KAPPAS)
@pytest.mark.parametrize("n", P.RANDOM_N)
def test_random_spd_blocks(L, n, kappa):
    """5. random SPD blocks factored by the library's batched factor; the two componentwise bounds against the np.longdouble reference
    formed from the device's R"""
    A = P.random_spd(n, kappa, 2)
    fbuf = tri_buf(A, n, 1, 3)
    info = factor(L, fbuf, n)
    assert not info.cpu().numpy().any()
    R = np.triu(fbuf.blocks())
    wbuf, xbuf = tri_buf(R, n, 1, 3), tri_buf(R, n, 0, 0)
    trtri(L, wbuf, n, info)
    potri(L, xbuf, n, info)
    W, X = wbuf.blocks(), xbuf.blocks()
    wbuf.assert_rest_untouched()
    xbuf.assert_rest_untouched()
    for i in range(2):
        fw, fx = P.check_random(R[i], W[i], X[i])
        print("n = %d kappa = %g block %d: %.3f / %.3f of the bounds" % (n, kappa, i, fw, fx))


@pytest.mark.parametrize("n", (5, 16, 33, 64, 65, 130, 256))
def test_position_and_layout_independence(L, n):
    """6. one random block at every position of batches of 1, 7, 64 and 257 (33 for n > 64), at even and odd ld and stride: one set of bits;
    fill = 0 and fill = 1 give the same upper triangle"""
    R1 = np.triu(np.linalg.cholesky(P.random_spd(n, 1e3, 1, seed=5)[0]).T)[None]
    ref = {}
    for batch in (1, 7, 64, 257) if n <= 64 else (1, 7, 33):
        for dl, ds in ((0, 0), (1, 0), (0, 1), (1, 1)):
            blocks = np.repeat(R1, batch, axis=0)
            for name, run, mk in (("trtri", lambda b: trtri(L, b, n), tri_buf), ("potri", lambda b: potri(L, b, n), tri_buf),
                                  ("potri", lambda b: potri(L, b, n, fill=1), win_buf)):
                buf = mk(blocks, n, dl, ds)
                run(buf)
                got = buf.blocks()[:, np.triu_indices(n)[0], np.triu_indices(n)[1]].view(np.int64)
                ref.setdefault(name, got[0])
                assert np.array_equal(got, np.broadcast_to(ref[name], got.shape)), (name, batch, dl, ds)


def test_python_layer(L):
    """7. batched.potrf -> batched.potri(symmetric=True) against torch.cholesky_inverse of torch's own factor, to the bound of 5; batched.trtri
    on a strided tensor against the exact families; a call on a non-default stream; the refusal of n = 257"""
    from capital_amd import _lib, batched
    # kappa = 10: torch inverts from ITS factor, which differs from the library's by rounding; the two inverses then differ by about
    # X (dA1 - dA2) X with |dA| <= gamma_{n+1} |R|^T |R|, which the bound of 5 (formed from the library's R) covers for a well-conditioned
    # block and would not for kappa = 1e6 and up - there the library's result is held against its own reference (test 5)
    for n, batch in ((20, 9), (150, 3)):
        A = P.random_spd(n, 1e1, batch, seed=3)
        At = torch.from_numpy(A).to(DEV)
        want = torch.cholesky_inverse(torch.linalg.cholesky(At)).cpu().numpy()
        mine = At.clone()
        info = batched.potrf(mine)
        Rdev = np.triu(mine.cpu().numpy().transpose(0, 2, 1))          # torch's lower triangle is the column-major upper one
        assert batched.potri(mine, info, symmetric=True) is mine
        got = mine.cpu().numpy()
        assert not info.cpu().numpy().any()
        iu = np.triu_indices(n)
        for i in range(batch):
            assert np.array_equal(got[i], got[i].T)
            _, X, _, bx = P.reference(Rdev[i])
            err = np.abs(got[i].astype(np.longdouble) - want[i].astype(np.longdouble))[iu]
            print("n = %d block %d: %.3f of the bound against torch.cholesky_inverse" % (n, i, float(np.max(err / bx[iu]))))
            assert np.all(err <= bx[iu])
            assert np.all(np.abs(got[i].astype(np.longdouble) - X)[iu] <= bx[iu])
    # trtri on a non-contiguous tensor: blocks of 40 inside rows of 44, 47 rows per block
    n, batch = 40, 6
    T, Ti, _ = P.batch("F2i", n, True, batch)
    big = torch.full((batch, 47, 44), float("nan"), dtype=torch.float64, device=DEV)
    view = big[:, :n, :n]
    view.copy_(torch.from_numpy(np.tril(T.transpose(0, 2, 1)) + np.triu(np.full((n, n), np.nan), 1)))
    assert batched.trtri(view) is view
    got = view.cpu().numpy()
    il = np.tril_indices(n)
    for i in range(batch):
        assert same_bits(got[i][il], Ti[i].T[il])
        assert np.isnan(got[i][np.triu_indices(n, 1)]).all()
    assert torch.isnan(big[:, n:, :]).all() and torch.isnan(big[:, :, n:]).all()
    # a stream of its own, read on that stream only
    s = torch.cuda.Stream()
    T, _, C = P.batch("F1", 70, False, 4)
    with torch.cuda.stream(s):
        t = torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1))).to(DEV, non_blocking=False)
        batched.potri(t)
        out = t.to("cpu", non_blocking=False)
    s.synchronize()
    il = np.tril_indices(70)
    for i in range(4):
        assert same_bits(out.numpy()[i][il], C[i].T[il])
    with pytest.raises(_lib.CapitalError, match="256"):
        batched.potri(torch.zeros(2, 257, 257, dtype=torch.float64, device=DEV))
    with pytest.raises(_lib.CapitalError, match="256"):
        batched.trtri(torch.zeros(2, 257, 257, dtype=torch.float64, device=DEV))
