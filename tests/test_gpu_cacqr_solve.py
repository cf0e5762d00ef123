"""-m gpu: the least-squares solve on CholeskyQR2 - the tall-skinny Q^T B kernel (exact on integers), cacqr.solve / apply_Qt against
numpy.linalg.lstsq within 10 x the error of the oracle's own arithmetic, refusals, and the 2^21 x 256 shape."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import capital_oracle as orc  # noqa: E402
from tests.gpu_util import DEV, relerr, to_dev, to_host  # noqa: E402


# ------------------------------------------------------------------------------------------------ the kernel, exact
def _tall(q, b, ldq=None, ldb=None, ldz=None, q_off=0, runs=1):
    """cap_dgemm_tall_tn on host arrays; NaN in every padding row of Q, B and Z.  Returns the list of Z buffers (cols, ldz) of `runs` runs."""
    import torch
    from capital_amd import _lib
    from capital_amd._util import cur_stream
    L = _lib.lib()
    m, n = q.shape
    nrhs = b.shape[1]
    ldq, ldb, ldz = ldq or m, ldb or m, ldz or n
    if q_off:            # an operand that starts 8 bytes past a 16-byte boundary
        flat = torch.full((n * ldq + q_off,), float("nan"), dtype=torch.float64, device=DEV)
        qv = flat[q_off:].view(n, ldq)
        qv[:, :m] = torch.from_numpy(np.ascontiguousarray(q.T)).to(DEV)
        qbuf = qv
    else:
        qbuf, _ = to_dev(q, ldq)
    bbuf, _ = to_dev(b, ldb)
    work = torch.full((max(int(L.cap_dgemm_tall_tn_work_size(m, n, nrhs)), 2),), float("nan"), dtype=torch.float64, device=DEV)
    outs = []
    for _ in range(runs):
        z = torch.full((nrhs, ldz), float("nan"), dtype=torch.float64, device=DEV)
        _lib.check(L.cap_dgemm_tall_tn(m, n, nrhs, qbuf.data_ptr(), ldq, bbuf.data_ptr(), ldb, z.data_ptr(), ldz, work.data_ptr(),
                                       cur_stream()), "cap_dgemm_tall_tn")
        outs.append(to_host(z))
    return outs


def _ints(m, n, nrhs, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, size=(m, n)).astype(np.float64), rng.integers(-3, 4, size=(m, nrhs)).astype(np.float64))


# (m, n, nrhs, pad of ldq, ldb, ldz, offset of Q in doubles).  Slabs are >= 512 rows and a multiple of 64, one per CU:
KERNEL_CASES = [
    (256, 16, 1, 0, 0, 0, 0),           # one slab, one wave
    (512, 128, 16, 0, 0, 0, 0),         # one full slab
    (5000, 128, 5, 6, 2, 3, 0),         # 10 slabs, the last one 392 rows (6 blocks of 64 + one step of 8); every ld padded, ldz odd
    (8192, 256, 16, 0, 4, 0, 0),        # 16 waves, all 16 right-hand sides
    (70272, 256, 8, 2, 0, 5, 0),        # 138 slabs, the last one 128 rows
    (600000, 16, 8, 0, 0, 0, 0),        # slabs taller than the minimum: 254 of 2368 rows on 256 CUs, the last one 896
    (4096, 256, 40, 2, 2, 1, 0),        # more than 16 right-hand sides: chunks of 16 + 16 + 8
    (4096, 64, 100, 0, 0, 0, 0),        # beyond the crossover: the tile product
    (4096, 37, 3, 0, 0, 0, 0),          # composed routes: n not a multiple of 16 ...
    (4096, 64, 8, 1, 0, 0, 0),          # ... odd ldq ...
    (4096, 64, 8, 0, 3, 0, 0),          # ... odd ldb ...
    (5001, 64, 8, 1, 1, 0, 0),          # ... m not a multiple of 8 ...
    (4096, 64, 8, 0, 0, 0, 1),          # ... Q not 16-byte aligned
]


@pytest.mark.parametrize("m,n,nrhs,pq,pb,pz,off", KERNEL_CASES)
def test_tall_tn_is_exact_on_integers(m, n, nrhs, pq, pb, pz, off):
    """Entries in -3 .. 3: every partial sum is an integer below 2^53, so any summation order gives the same doubles."""
    q, b = _ints(m, n, nrhs, 1000 + m + n + nrhs)
    z, = _tall(q, b, m + pq, m + pb, n + pz, q_off=off)
    assert np.array_equal(z[:, :n].T, q.T @ b)
    assert np.isnan(z[:, n:]).all()                                  # Z's padding rows are not written


def test_tall_tn_is_bit_identical_from_run_to_run():
    rng = np.random.default_rng(7)
    q, b = rng.standard_normal((70272, 256)), rng.standard_normal((70272, 8))
    z0, z1 = _tall(q, b, runs=2)
    assert np.array_equal(z0, z1)
    assert relerr(z0.T, q.T @ b) < 1e-14


# ------------------------------------------------------------------------------------------------ the solve
def _factor(a_or_shape, variant=2, CommInfo=None):
    from capital_amd import cacqr, cholinv
    from capital_amd.matrix import matrix
    if isinstance(a_or_shape, tuple):
        m, n = a_or_shape
        A = matrix(n, m, 1, 1)
        A.distribute_random(0, 0, 1, 1, 0)
    else:
        m, n = a_or_shape.shape
        A = matrix(n, m, 1, 1)
        A.from_numpy(a_or_shape)
    pack = cacqr.info(variant, cholinv.info(1, 1, 0, 'U'))
    cacqr.factor(A, pack, CommInfo)
    return A, pack


def _rhs_matrix(b):
    from capital_amd.matrix import matrix
    B = matrix(b.shape[1], b.shape[0], 1, 1)
    B.from_numpy(b)
    return B


def _opt(a, x, b):
    """the optimality condition of least squares, ||A^T (A x - b)||_F / (||A||_F ||b||_F)"""
    return float(np.linalg.norm(a.T @ (a @ x - b)) / (np.linalg.norm(a) * np.linalg.norm(b)))


def _bounds(a, b):
    """(x_ref, error bound, optimality bound): lstsq is the reference; the bounds are 10 x what the NumPy restatement of the same algorithm
    (oracle cacqr_1d, then solve(triu(R), Q^T b)) leaves on the same inputs - for the optimality 10 x the larger of restatement and lstsq."""
    x_ref = np.linalg.lstsq(a, b, rcond=None)[0]
    q, r = orc.cacqr_1d([a], 2)
    x_rs = np.linalg.solve(np.triu(r), q[0].T @ b)
    err_rs, opt_rs, opt_ref = relerr(x_rs, x_ref), _opt(a, x_rs, b), _opt(a, x_ref, b)
    return x_ref, max(10.0 * err_rs, 1e-14), 10.0 * max(opt_rs, opt_ref), (err_rs, opt_rs, opt_ref)


def _check_solve(a, b, pack, label):
    from capital_amd import cacqr
    x = cacqr.solve(pack, _rhs_matrix(b)).to_numpy()
    assert pack.last_info() == 0
    x_ref, ebound, obound, rs = _bounds(a, b)
    err, opt = relerr(x, x_ref), _opt(a, x, b)
    print("%s: error %.2e (restatement %.2e, bound %.2e)  optimality %.2e (restatement %.2e, lstsq %.2e, bound %.2e)"
          % (label, err, rs[0], ebound, opt, rs[1], rs[2], obound))
    assert err < ebound
    assert opt < obound
    return x


GEN_SHAPES = [(4096, 64), (5000, 37), (8192, 256), (70272, 256), (100000, 128)]


@pytest.mark.parametrize("m,n", GEN_SHAPES)
def test_solve_matches_lstsq_on_generator_matrices(m, n):
    A, pack = _factor((m, n))
    a = A.to_numpy()
    b = np.random.default_rng(m + n).standard_normal((m, 8))
    _check_solve(a, b, pack, "solve %d x %d" % (m, n))


@pytest.mark.parametrize("m,n", GEN_SHAPES)
def test_consistent_system_returns_its_solution(m, n):
    A, pack = _factor((m, n))
    a = A.to_numpy()
    x0 = np.random.default_rng(3 * m + n).standard_normal((n, 8))
    b = a @ x0
    from capital_amd import cacqr
    x = cacqr.solve(pack, _rhs_matrix(b)).to_numpy()
    q, r = orc.cacqr_1d([a], 2)
    err_rs = relerr(np.linalg.solve(np.triu(r), q[0].T @ b), x0)
    err = relerr(x, x0)
    print("consistent %d x %d: error %.2e (restatement %.2e)" % (m, n, err, err_rs))
    assert err < max(10.0 * err_rs, 1e-14)


@pytest.mark.parametrize("kappa", [1e2, 1e4, 1e6])
def test_solve_over_condition_numbers(kappa):
    m, n = 16384, 256
    rng = np.random.default_rng(int(math.log10(kappa)))
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (u * np.logspace(0, -math.log10(kappa), n)) @ v.T
    b = rng.standard_normal((m, 3))
    A, pack = _factor(a)
    _check_solve(a, b, pack, "kappa %.0e" % kappa)


def test_apply_Qt_is_the_product_with_the_plans_Q():
    from capital_amd import cacqr
    for (m, n) in ((8192, 256), (5000, 37)):
        A, pack = _factor((m, n))
        b = np.random.default_rng(11).standard_normal((m, 8))
        z = cacqr.apply_Qt(pack, _rhs_matrix(b)).to_numpy()
        q = cacqr.construct_Q(pack).to_numpy()
        assert relerr(z, q.T @ b) < 1e-14


def test_right_hand_sides_as_device_tensors():
    """a column-major view is used in place, a row-major tensor and a vector through a copy: the same X as from a `matrix`"""
    import torch
    from capital_amd import cacqr
    m, n = 4096, 64
    A, pack = _factor((m, n))
    b = np.random.default_rng(5).standard_normal((m, 4))
    x = cacqr.solve(pack, _rhs_matrix(b)).to_numpy()
    rowmajor = torch.from_numpy(b).to(DEV)
    colmajor = rowmajor.t().contiguous().t()
    assert np.array_equal(cacqr.solve(pack, rowmajor).to_numpy(), x)
    assert np.array_equal(cacqr.solve(pack, colmajor).to_numpy(), x)
    assert np.array_equal(cacqr.solve(pack, rowmajor[:, 0].contiguous()).to_numpy(), x[:, :1])


def test_size_one_communicator_gives_the_same_bits():
    from capital_amd import cacqr, topo
    m, n = 8192, 256
    b = np.random.default_rng(13).standard_normal((m, 8))
    A, pack = _factor((m, n))
    x = cacqr.solve(pack, _rhs_matrix(b)).to_numpy()
    T = topo.rect(1)
    try:
        assert T.world is not None
        A1, pack1 = _factor((m, n), CommInfo=T)
        x1 = cacqr.solve(pack1, _rhs_matrix(b), T).to_numpy()
        z1 = cacqr.apply_Qt(pack1, _rhs_matrix(b), T).to_numpy()
        pack1._release()
    finally:
        T.close()
    assert np.array_equal(x, x1)
    assert np.array_equal(z1, cacqr.apply_Qt(pack, _rhs_matrix(b)).to_numpy())


# ------------------------------------------------------------------------------------------------ failure and refusal
def test_failed_factor_gives_nan():
    """two equal columns of ones, m = 64^2: G00 = G01 = G11 = 4096 exactly, r00 = r01 = 64 and the second pivot is exactly zero"""
    from capital_amd import cacqr
    m, n = 4096, 64
    a = np.random.default_rng(17).standard_normal((m, n))
    a[:, 0] = 1.0
    a[:, 1] = 1.0
    A, pack = _factor(a)
    B = _rhs_matrix(np.ones((m, 3)))
    x = cacqr.solve(pack, B).to_numpy()
    assert pack.last_info() != 0
    assert x.shape == (n, 3) and np.isnan(x).all()
    assert np.isnan(cacqr.apply_Qt(pack, B).to_numpy()).all()


def test_solve_before_factor_raises():
    from capital_amd import _lib, cacqr, cholinv
    m, n = 4096, 64
    B = _rhs_matrix(np.ones((m, 2)))
    pack = cacqr.info(2, cholinv.info(1, 1, 0, 'U'))
    with pytest.raises(_lib.CapitalError):
        cacqr.solve(pack, B)                       # no plan at all
    pack._ensure(m, n, None)                       # a plan, never factored: the library refuses (CAP_ERR_ARG)
    pack._gm, pack._gn = m, n
    with pytest.raises(_lib.CapitalError, match="status 1"):
        cacqr.solve(pack, B)
    with pytest.raises(_lib.CapitalError, match="status 1"):
        cacqr.apply_Qt(pack, B)


def test_grid_plan_is_unsupported():
    from capital_amd import _lib, cacqr, cholinv, topo
    from capital_amd.matrix import matrix
    from capital_amd._util import cur_stream
    m, n = 4096, 64
    T = topo.rect(1)
    try:
        A = matrix(n, m, 1, 1)
        A.distribute_random(0, 0, 1, 1, 0)
        pack = cacqr.info(2, cholinv.info(1, 1, 0, 'U'))
        pack._gm, pack._gn = m, n
        pack._ensure_grid(A, T)                    # the c x d x c path on a 1 x 1 x 1 grid
        _lib.check(_lib.lib().cap_cacqr_factor(pack._plan, A.data_ptr(), A.ld(), cur_stream()), "cacqr::factor")
        assert pack.last_info() == 0
        B = _rhs_matrix(np.ones((m, 2)))
        with pytest.raises(_lib.CapitalError, match="status 4"):
            cacqr.solve(pack, B, T)
        with pytest.raises(_lib.CapitalError, match="status 4"):
            cacqr.apply_Qt(pack, B, T)
        pack._release()
    finally:
        T.close()


# ------------------------------------------------------------------------------------------------ at scale
def test_solve_at_scale_optimality():
    """2^21 x 256, CholeskyQR2, 8 right-hand sides: ||A^T (A x - b)||_F / (||A||_F ||b||_F) < 1e-14, computed on the device in fp64 with
    the library's own cap_dgemm and cap_sumsq (properties only at this size; the small cases sit two orders below the bound)."""
    import torch
    from capital_amd import _lib, cacqr
    from capital_amd._util import cur_stream
    from capital_amd.matrix import matrix
    m, n, nrhs = 1 << 21, 256, 8
    A, pack = _factor((m, n))
    assert pack.last_info() == 0
    B = matrix(nrhs, m, 1, 1)
    g = torch.Generator(device=DEV); g.manual_seed(21)
    B.data().copy_(torch.randn(nrhs, m, dtype=torch.float64, device=DEV, generator=g))
    X = cacqr.solve(pack, B)
    L, s = _lib.lib(), cur_stream()
    R = torch.empty_like(B.data()); R.copy_(B.data())
    _lib.check(L.cap_dgemm(0, 0, m, nrhs, n, 1.0, A.data_ptr(), A.ld(), X.data_ptr(), X.ld(), -1.0, R.data_ptr(), B.ld(), s), "A x - b")
    G = torch.zeros(nrhs, n, dtype=torch.float64, device=DEV)
    _lib.check(L.cap_dgemm(1, 0, n, nrhs, m, 1.0, A.data_ptr(), A.ld(), R.data_ptr(), B.ld(), 0.0, G.data_ptr(), n, s), "A^T r")
    out = torch.zeros(3, dtype=torch.float64, device=DEV)
    for i, (t, ld, rows, cols) in enumerate(((G, n, n, nrhs), (A.data(), A.ld(), m, n), (B.data(), B.ld(), m, nrhs))):
        _lib.check(L.cap_sumsq(t.data_ptr(), ld, rows, cols, 0, 0, out[i:].data_ptr(), s), "sumsq")
    gg, aa, bb = out.tolist()
    opt = math.sqrt(gg) / (math.sqrt(aa) * math.sqrt(bb))
    print("2^21 x 256: optimality %.2e" % opt)
    assert math.isfinite(opt) and opt < 1e-14
    assert torch.isfinite(X.data()).all()
