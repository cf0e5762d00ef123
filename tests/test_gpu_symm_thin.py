"""-m gpu: cap_dsymm_thin (Y = beta opB(B) + alpha op(A) opX(X), A symmetric with only its upper triangle read) and cap_dlansy, bit for bit:
A, X and B hold small integers and alpha, beta come from {0, 1, -1, 2}, so every sum is exact in any order and no tolerance is needed.
Every operand sits in a NaN-padded window (odd leading dimension, the pointer one element into its buffer): NaN in the strictly lower
triangle of A and in all padding must not reach Y, and nothing outside Y's n rows may change."""
import numpy as np
import pytest
import torch

from tests.gpu_util import NanWork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = 512                                 # the super-block edge of csrc/symv.hip
OK, ARG = 0, 1
NAN = float("nan")
NS = (1, 2, 63, 64, 65, 127, 128, 129, S - 1, S, S + 1, 2 * S + 1, 1300)
NRHS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 33)
GRID = sorted({(n, r) for n in NS for r in (1, 16)} | {(n, r) for n in (129, 2 * S + 1) for r in NRHS})
COEF = ((1.0, 1.0), (-1.0, 1.0), (2.0, -1.0), (1.0, 2.0), (-1.0, -1.0), (2.0, 2.0))


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Win:
    """a rows x cols column-major window with leading dimension ld, one element into a NaN-filled buffer"""

    def __init__(self, a, ld, fill=NAN):
        a = np.asarray(a, dtype=np.float64)
        self.rows, self.cols, self.ld = a.shape[0], a.shape[1], ld
        host = np.full(1 + ld * self.cols + 3, fill)
        w = host[1:1 + ld * self.cols].reshape(self.cols, ld)
        w[:, :self.rows] = a.T
        self.host0 = host
        self.buf = torch.from_numpy(host.copy()).to(DEV)
        self.ptr = self.buf.data_ptr() + 8

    def get(self):
        h = self.buf.cpu().numpy()
        return h[1:1 + self.ld * self.cols].reshape(self.cols, self.ld)[:, :self.rows].T.copy()

    def outside_unchanged(self):
        h = self.buf.cpu().numpy().copy()
        ref = self.host0.copy()
        for m in (h, ref):
            m[1:1 + self.ld * self.cols].reshape(self.cols, self.ld)[:, :self.rows] = 0.0
        return np.array_equal(h, ref, equal_nan=True)


def _ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def _sym(rng, n):
    u = np.triu(_ints(rng, (n, n)))
    full = u + np.triu(u, 1).T
    upper_only = u.copy()
    upper_only[np.tril_indices(n, -1)] = NAN            # the strictly lower triangle must never be read
    return full, upper_only


def _work(n, nrhs):
    """all NaN, exactly the stated size, a sentinel behind it (check())"""
    return NanWork(_L().cap_dsymm_thin_work_size(n, nrhs))


def _call(ab, n, nrhs, alpha, A, X, beta, B, Y, work):
    return _L().cap_dsymm_thin(1, ab, n, nrhs, alpha, A.ptr if A else None, A.ld if A else 0, X.ptr if X else None, X.ld if X else 0, beta,
                               B.ptr if B else None, B.ld if B else 0, Y.ptr, Y.ld, work.data_ptr(), _stream())


def _ref(ab, alpha, a, x, beta, b):
    if ab:
        a, x, b = np.abs(a), np.abs(x), np.abs(b)
    return beta * b + alpha * (a @ x)


@pytest.mark.parametrize("n,nrhs", GRID)
def test_exact_on_padded_windows(n, nrhs):
    rng = np.random.default_rng(17 * n + nrhs)
    a, a_up = _sym(rng, n)
    x, b = _ints(rng, (n, nrhs)), _ints(rng, (n, nrhs))
    A, X, B = Win(a_up, n + 3 - (n & 1)), Win(x, n + 1 - (n & 1) + 2), Win(b, n + 5 - (n & 1))       # odd leading dimensions
    work = _work(n, nrhs)
    for k, ab in enumerate((0, 1)):
        alpha, beta = COEF[(n + nrhs + k) % len(COEF)]
        Y = Win(np.full((n, nrhs), NAN), n + 7 - (n & 1), fill=-3.0)
        assert _call(ab, n, nrhs, alpha, A, X, beta, B, Y, work) == OK
        torch.cuda.synchronize()
        assert np.array_equal(Y.get(), _ref(ab, alpha, a, x, beta, b)), (ab, alpha, beta)
        assert Y.outside_unchanged(), "written outside Y's n rows"
        work.check("cap_dsymm_thin")
    for w in (A, X, B):
        assert np.array_equal(w.buf.cpu().numpy(), w.host0, equal_nan=True), "an input was written"


@pytest.mark.parametrize("n,nrhs", [(129, 5), (2 * S + 1, 17)])
def test_beta_zero_alpha_zero_and_in_place(n, nrhs):
    rng = np.random.default_rng(n)
    a, a_up = _sym(rng, n)
    x, b = _ints(rng, (n, nrhs)), _ints(rng, (n, nrhs))
    A, X, B = Win(a_up, n + 2), Win(x, n + 4), Win(b, n + 6)
    work = _work(n, nrhs)
    # beta = 0: B is never read - NULL, or all NaN
    for Bz in (None, Win(np.full((n, nrhs), NAN), n + 6)):
        Y = Win(np.full((n, nrhs), NAN), n + 2, fill=-3.0)
        assert _call(0, n, nrhs, 2.0, A, X, 0.0, Bz, Y, work) == OK
        torch.cuda.synchronize()
        assert np.array_equal(Y.get(), 2.0 * (a @ x)) and Y.outside_unchanged()
    # alpha = 0: A, X and work are never read - all NaN, or NULL
    An, Xn = Win(np.full((n, n), NAN), n + 2), Win(np.full((n, nrhs), NAN), n + 4)
    for Az, Xz in ((An, Xn), (None, None)):
        Y = Win(np.full((n, nrhs), NAN), n + 2, fill=-3.0)
        assert _call(1, n, nrhs, 0.0, Az, Xz, -1.0, B, Y, work) == OK
        torch.cuda.synchronize()
        assert np.array_equal(Y.get(), -np.abs(b)) and Y.outside_unchanged()
    # Y = B in place
    Yb = Win(b, n + 6)
    assert _L().cap_dsymm_thin(1, 0, n, nrhs, -1.0, A.ptr, A.ld, X.ptr, X.ld, 1.0, Yb.ptr, Yb.ld, Yb.ptr, Yb.ld, work.data_ptr(), _stream()) == OK
    torch.cuda.synchronize()
    assert np.array_equal(Yb.get(), b - a @ x) and Yb.outside_unchanged()
    work.check("cap_dsymm_thin")
    # Y on top of A, X or work is refused
    assert _L().cap_dsymm_thin(1, 0, n, nrhs, 1.0, A.ptr, A.ld, X.ptr, X.ld, 0.0, None, 0, X.ptr, X.ld, work.data_ptr(), _stream()) == ARG
    assert _L().cap_dsymm_thin(1, 0, n, nrhs, 1.0, A.ptr, A.ld, X.ptr, X.ld, 0.0, None, 0, work.data_ptr(), n, work.data_ptr(), _stream()) == ARG


def test_two_calls_give_the_same_bits_and_the_right_product():
    n, nrhs = 1300, 7
    rng = np.random.default_rng(3)
    g = rng.standard_normal((n, n))
    a = (g + g.T) / 2
    a_up = np.triu(a); a_up[np.tril_indices(n, -1)] = NAN
    x, b = rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))
    A, X, B = Win(a_up, n + 1), Win(x, n + 1), Win(b, n + 1)
    work = _work(n, nrhs)
    out = []
    for _ in range(2):
        Y = Win(np.full((n, nrhs), NAN), n + 1, fill=-3.0)
        assert _call(0, n, nrhs, -1.0, A, X, 1.0, B, Y, work) == OK
        torch.cuda.synchronize()
        out.append(Y.get())
    assert np.array_equal(out[0], out[1])
    work.check("cap_dsymm_thin")
    ref = b - a @ x
    # a sum of n products in any order: |error| <= gamma_n (|A||X| + |B|) componentwise, gamma_n = n u / (1 - n u), u = 2^-53
    bound = (n * 2.0 ** -53 / (1 - n * 2.0 ** -53)) * (np.abs(a) @ np.abs(x) + np.abs(b))
    assert (np.abs(out[0] - ref) <= 2 * bound).all()          # (twice: the host's own reference carries the same bound)


def _lansy(n, A):
    L = _L()
    out = torch.full((3,), -5.0, dtype=torch.float64, device=DEV)
    work = NanWork(L.cap_dlansy_work_size(n))
    assert L.cap_dlansy(ord('1'), 1, n, A.ptr if A else None, A.ld if A else 0, out.data_ptr() + 8, work.data_ptr(), _stream()) == OK
    work.check("cap_dlansy(n = %d)" % n)
    o = out.cpu().numpy()
    assert o[0] == -5.0 and o[2] == -5.0
    return o[1]


@pytest.mark.parametrize("n", NS)
def test_lansy_exact(n):
    rng = np.random.default_rng(23 * n)
    a, a_up = _sym(rng, n)
    A = Win(a_up, n + 3 - (n & 1))
    assert _lansy(n, A) == np.abs(a).sum(0).max()
    for norm in (b'O', b'I'):
        out = torch.zeros(1, dtype=torch.float64, device=DEV)
        work = NanWork(_L().cap_dlansy_work_size(n))
        assert _L().cap_dlansy(ord(norm), 1, n, A.ptr, A.ld, out.data_ptr(), work.data_ptr(), _stream()) == OK
        assert out.item() == np.abs(a).sum(0).max()
        work.check("cap_dlansy(n = %d)" % n)


@pytest.mark.parametrize("n", (65, 2 * S + 1))
def test_lansy_nan_and_empty(n):
    rng = np.random.default_rng(n)
    a, a_up = _sym(rng, n)
    d = a_up.copy(); d[n // 2, n // 2] = NAN                  # one NaN on the diagonal
    assert np.isnan(_lansy(n, Win(d, n + 2)))
    o = a_up.copy(); o[0, n - 1] = NAN                         # one NaN in an off-diagonal element of the last column
    assert np.isnan(_lansy(n, Win(o, n + 2)))
    assert _lansy(0, None) == 0.0
