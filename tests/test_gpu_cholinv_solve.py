"""-m gpu: the fp64 Cholesky solve - cap_cholinv_solve on the plan's last factor, cap_dpotrs beside cap_dpotrf, the one-launch
substitutions (option "solve_kernel" = 1, nrhs <= 16) against the blocked path, the recovery launch, and the failure cases."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNSUPPORTED = 4


def _L():
    from capital_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _spd(n, seed):
    """Well-conditioned SPD test matrix G G^T / n + I on the GPU (symmetric: its buffer is column-major as well)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    G = torch.rand(n, n, dtype=torch.float64, device=DEV, generator=g) * 2 - 1
    return G @ G.T / n + torch.eye(n, dtype=torch.float64, device=DEV)


def _rhs(n, nrhs, ld, seed):
    """n x nrhs column-major buffer with leading dimension ld (padding rows NaN): returns (buffer, view[row, col])."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.full((nrhs, ld), float("nan"), dtype=torch.float64, device=DEV)
    buf[:, :n] = torch.rand(nrhs, n, dtype=torch.float64, device=DEV, generator=g) - 0.5
    return buf, buf[:, :n].t()


class Plan:
    def __init__(self, n, ci):
        self.n, self.h = n, C.c_void_p()
        assert _L().cap_cholinv_plan_create(C.byref(self.h), n, ci, 1, -2, b"U", None) == 0

    def factor(self, A):
        assert _L().cap_cholinv_factor(self.h, A.data_ptr(), A.shape[0], _stream()) == 0

    def solve(self, B, X, nrhs):
        return _L().cap_cholinv_solve(self.h, B.data_ptr(), B.shape[1], X.data_ptr(), X.shape[1], nrhs, _stream())

    def option(self, key, value):
        assert _L().cap_cholinv_set_option(self.h, key.encode(), value) == 0

    def info(self):
        v = C.c_int64(0)
        _L().cap_cholinv_info(self.h, _stream(), C.byref(v))
        return v.value

    def __del__(self):
        _L().cap_cholinv_plan_destroy(self.h)


# (n, nrhs, complete_inv, in place): a sparse cross product of the sizes, right-hand side counts and modes
CASES = [(1, 1, -1, False), (1, 3, 1, True), (100, 3, 0, True), (100, 17, 1, False), (100, 16, -1, False), (1000, 8, -1, False),
         (1000, 130, 0, True), (1000, 1, 1, False), (4096, 16, 1, False), (4096, 1, -1, True), (4096, 17, -1, False),
         (4096, 130, 1, False), (16384, 8, -1, False), (16384, 3, 1, True), (16384, 17, 0, False)]


@pytest.mark.parametrize("n,nrhs,ci,inplace", CASES)
def test_solve_accuracy(n, nrhs, ci, inplace):
    A = _spd(n, 1 + n)
    p = Plan(n, ci)
    p.factor(A)
    Bbuf, B = _rhs(n, nrhs, n + 3, 7)
    B0 = Bbuf.clone()
    if inplace:
        Xbuf = Bbuf
    else:
        Xbuf = torch.full((nrhs, n + 5), -7.0, dtype=torch.float64, device=DEV)
    assert p.solve(Bbuf, Xbuf, nrhs) == 0
    torch.cuda.synchronize()
    X = Xbuf[:, :n].t()
    if not inplace:
        assert torch.equal(torch.nan_to_num(Bbuf, nan=1e300), torch.nan_to_num(B0, nan=1e300)), "B was written"
        assert torch.all(Xbuf[:, n:] == -7.0), "X written outside its n rows"
    Bref = B0[:, :n].t()
    if n <= 4096:
        ref = np.linalg.solve(A.cpu().numpy(), Bref.cpu().numpy())
        err = np.linalg.norm(X.cpu().numpy() - ref) / np.linalg.norm(ref)
        assert err <= 1e-12, err
    else:
        berr = (torch.linalg.norm(Bref - A @ X) / (torch.linalg.norm(A) * torch.linalg.norm(X))).item()
        assert berr <= 1e-15, berr


@pytest.mark.parametrize("n,nrhs", [(1000, 8), (4096, 16), (4096, 1)])
def test_one_launch_against_blocked_path_and_repeatable(n, nrhs):
    A = _spd(n, 3)
    p = Plan(n, -1)
    p.factor(A)
    Bbuf, _ = _rhs(n, nrhs, n, 11)
    X1 = torch.empty_like(Bbuf); X2 = torch.empty_like(Bbuf); X0 = torch.empty_like(Bbuf)
    assert p.solve(Bbuf, X1, nrhs) == 0 and p.solve(Bbuf, X2, nrhs) == 0
    p.option("solve_kernel", 0)
    assert p.solve(Bbuf, X0, nrhs) == 0
    torch.cuda.synchronize()
    assert torch.equal(X1, X2), "two solves differ"
    assert (torch.linalg.norm(X1 - X0) / torch.linalg.norm(X0)).item() <= 1e-13


@pytest.mark.parametrize("kernel", [1, 0])
def test_a_new_factor_call_makes_the_cached_inverses_stale(kernel):
    n, nrhs = 1500, 4
    A1, A2 = _spd(n, 21), _spd(n, 22) + 3 * torch.eye(n, dtype=torch.float64, device=DEV)
    p = Plan(n, 0)
    p.option("solve_kernel", kernel)
    Bbuf, B = _rhs(n, nrhs, n, 5)
    X = torch.empty_like(Bbuf)
    p.factor(A1)
    assert p.solve(Bbuf, X, nrhs) == 0
    p.factor(A2)
    assert p.solve(Bbuf, X, nrhs) == 0
    torch.cuda.synchronize()
    ref = np.linalg.solve(A2.cpu().numpy(), B.cpu().numpy())
    assert np.linalg.norm(X.t().cpu().numpy() - ref) / np.linalg.norm(ref) <= 1e-12


@pytest.mark.parametrize("nrhs,kernel", [(4, 1), (4, 0), (20, 1)])
def test_not_spd_gives_nan_and_no_error(nrhs, kernel):
    n = 300
    A = torch.eye(n, dtype=torch.float64, device=DEV) * 2
    A[150, 150] = -1.0
    p = Plan(n, -1)
    p.option("solve_kernel", kernel)
    p.factor(A)
    Bbuf, _ = _rhs(n, nrhs, n, 1)
    X = torch.zeros_like(Bbuf)
    assert p.solve(Bbuf, X, nrhs) == 0
    torch.cuda.synchronize()
    assert torch.isnan(X).all()
    assert p.info() != 0


def _noop_comm(size):
    from capital_amd import _lib
    AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    BC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)
    AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    cbs = (AG(lambda *a: 0), BC(lambda *a: 0), AR(lambda *a: 0))
    h = C.c_void_p()
    _lib.check(_lib.lib().cap_comm_create_callbacks(C.byref(h), 0, size, *[C.cast(c, C.c_void_p) for c in cbs], None), "comm")
    return h, cbs


def test_unsupported_plans_and_lower_uplo():
    L = _L()
    n, nrhs = 512, 2
    Bbuf, _ = _rhs(n, nrhs, n, 1)
    X = torch.empty_like(Bbuf)
    comm, cbs = _noop_comm(4)
    try:
        h = C.c_void_p()
        assert L.cap_cholinv_plan_create(C.byref(h), n, -1, 1, -2, b"U", comm) == 0
        assert L.cap_cholinv_solve(h, Bbuf.data_ptr(), n, X.data_ptr(), n, nrhs, _stream()) == UNSUPPORTED
        assert L.cap_cholinv_set_option(h, b"cyclic_c", 1) == 0 and L.cap_cholinv_get_option(h, b"cyclic_c") == 1
        assert L.cap_cholinv_solve(h, Bbuf.data_ptr(), n, X.data_ptr(), n, nrhs, _stream()) == UNSUPPORTED
        L.cap_cholinv_plan_destroy(h)
    finally:
        L.cap_comm_destroy(comm)
    R = torch.eye(n, dtype=torch.float64, device=DEV)
    work = torch.empty(L.cap_dpotrs_work_size(n, nrhs), dtype=torch.float64, device=DEV)
    assert L.cap_dpotrs(0, n, nrhs, R.data_ptr(), n, Bbuf.data_ptr(), n, work.data_ptr(), _stream()) == UNSUPPORTED


def test_recovery_launch_finishes_an_injected_give_up():
    L = _L()
    n, nrhs = 1000, 5
    A = _spd(n, 9)
    p = Plan(n, -1)
    p.factor(A)
    Bbuf, B = _rhs(n, nrhs, n, 2)
    Xref, X = torch.empty_like(Bbuf), torch.empty_like(Bbuf)
    assert p.solve(Bbuf, Xref, nrhs) == 0
    before = L.cap_solve_fallbacks()
    assert before >= 0
    assert L.cap_solve_inject_timeouts(1) == 0
    assert p.solve(Bbuf, X, nrhs) == 0
    assert L.cap_solve_fallbacks() == before + 1
    torch.cuda.synchronize()
    assert torch.equal(X, Xref), "the recovery launch sums in the same order"
    ref = np.linalg.solve(A.cpu().numpy(), B.cpu().numpy())
    assert np.linalg.norm(X.t().cpu().numpy() - ref) / np.linalg.norm(ref) <= 1e-12
    assert p.solve(Bbuf, X, nrhs) == 0 and L.cap_solve_fallbacks() == before + 1        # the hook was used up


@pytest.mark.parametrize("n,nrhs", [(777, 3), (700, 20), (2048, 16)])
def test_dpotrs_after_dpotrf_on_a_padded_window(n, nrhs):
    L = _L()
    lda, ldb = n + 7, n + 2
    A = _spd(n, 30 + n)
    a = A.cpu().numpy()
    buf = torch.full((n + 1, lda), 5.0, dtype=torch.float64, device=DEV)    # an extra column: the window sits inside a bigger buffer
    buf[:n, :n] = A
    win = buf.data_ptr()
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    w1 = torch.empty(L.cap_dpotrf_work_size(n), dtype=torch.float64, device=DEV)
    assert L.cap_dpotrf(1, n, win, lda, info.data_ptr(), w1.data_ptr(), _stream()) == 0
    Bbuf, B = _rhs(n, nrhs, ldb, 4)
    b = B.cpu().numpy()
    w2 = torch.empty(L.cap_dpotrs_work_size(n, nrhs), dtype=torch.float64, device=DEV)
    assert L.cap_dpotrs(1, n, nrhs, win, lda, Bbuf.data_ptr(), ldb, w2.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    ref = np.linalg.solve(a, b)
    assert np.linalg.norm(Bbuf[:, :n].t().cpu().numpy() - ref) / np.linalg.norm(ref) <= 1e-12
    assert torch.isnan(Bbuf[:, n:]).all()


def test_python_interfaces():
    from capital_amd import cholinv, lapack
    from capital_amd.matrix import matrix
    n, nrhs = 600, 6
    a = _spd(n, 41).cpu().numpy()
    b = np.random.default_rng(0).standard_normal((n, nrhs))
    A = matrix(n, n, 1, 1); A.from_numpy(a)
    Bm = matrix(nrhs, n, 1, 1); Bm.from_numpy(b)
    pack = cholinv.info(-1, 1, -2, 'U')
    cholinv.factor(A, pack, None)
    X = cholinv.solve(Bm, pack)
    ref = np.linalg.solve(a, b)
    assert np.linalg.norm(X.to_numpy() - ref) / np.linalg.norm(ref) <= 1e-12
    assert np.array_equal(Bm.to_numpy(), b)
    R = torch.from_numpy(a.T.copy()).to(DEV)
    Bt = torch.from_numpy(b.T.copy()).to(DEV)
    up = lapack.UpLo.AlapackUpper
    assert lapack.engine._potrf(R, n, n, lapack.ArgPack_potrf(lapack.Order.AlapackColumnMajor, up)) == 0
    lapack.engine._potrs(R, Bt, n, nrhs, n, n, lapack.ArgPack_potrs(lapack.Order.AlapackColumnMajor, up))
    assert np.linalg.norm(Bt.t().cpu().numpy() - ref) / np.linalg.norm(ref) <= 1e-12
