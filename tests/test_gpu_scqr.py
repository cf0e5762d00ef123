"""-m gpu: shifted CholeskyQR3 (cacqr.info(3 | 4)): num_iter - 2 shifted, equilibrated sweeps in front of CholeskyQR2.

Every case carries a NumPy restatement of the algorithm in fp64 on the CPU (`restate` below: csrc/cacqr.hip's sweeps with the shift of
DESIGN.md section 4, "Shifted CholeskyQR3").  The restatement must succeed and the condition number of Q entering the final CholeskyQR2 must be <= 1e7 BEFORE the
GPU is touched: a case that misses that guard is a badly chosen input.  Bars: validate.qr.residual < 1e-13 and orthogonality < 1e-15
(tests/test_gpu_cacqr.py); R and Q each within 10 x the distance between the restatement and Householder QR, sign-normalised so that diag(R) > 0
(the 10 x-of-restatement rule of DESIGN.md section 7: R against R, Q against Q)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_util import relerr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1e7


# ------------------------------------------------------------------------------------------------ inputs and the restatement
def shift_of(m, n):
    """s = 11 (m n + n (n + 1)) 2^-53 n with the GLOBAL row count: every factor is an integer or a power of two and the product stays below
    2^53 for every shape here, so the value is exact and does not depend on the order of the multiplications"""
    return 11.0 * float(m * n + n * (n + 1)) * 2.0 ** -53 * float(n)


def make_input(m, n, kappa, scaled=False, seed=None):
    """A = U diag(logspace(0, -log10 kappa, n)) V^T as in test_solve_over_condition_numbers, optionally times diag(logspace(0, 8, n))"""
    rng = np.random.default_rng(int(round(math.log10(kappa))) + m + n if seed is None else seed)
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (u * np.logspace(0, -math.log10(kappa), n)) @ v.T
    if scaled:
        a = a * np.logspace(0, 8, n)
    return np.ascontiguousarray(a)


def _inv_upper(r):
    return np.triu(np.linalg.solve(r, np.eye(r.shape[0])))


def _sweep(pieces, shift):
    """one sweep on the row pieces of Q: (new pieces, R_k).  shift > 0: the Gram is equilibrated to unit diagonal, the diagonal set to
    1 + shift, and the scaling is undone on the factor (R' D) and on its inverse (D^-1 R'^-1)"""
    g = sum(np.triu(p.T @ p) for p in pieces)
    g = np.triu(g) + np.triu(g, 1).T
    n = g.shape[0]
    d = np.ones(n)
    if shift > 0.0:
        dg = np.diag(g).copy()
        ok = np.isfinite(dg) & (dg > 0)
        d[ok] = np.sqrt(dg[ok])
        g = g / d[:, None] / d[None, :]
        g[np.arange(n), np.arange(n)] = 1.0 + shift
    rp = np.linalg.cholesky(g).T
    ri = _inv_upper(rp)
    if shift > 0.0:
        rp, ri = rp * d[None, :], ri / d[:, None]
    return [p @ ri for p in pieces], rp


def restate(a_pieces, num_iter, gram_guard=False):
    """(Q pieces, R, condition number of Q entering the final CholeskyQR2).  gram_guard: the condition number from the eigenvalues of the
    n x n Gram (2^20 rows: an SVD of Q would take minutes; at cond <= 1e7 the Gram's smallest eigenvalue still has 2 digits)"""
    if not isinstance(a_pieces, (list, tuple)):
        a_pieces = [a_pieces]
    m = sum(p.shape[0] for p in a_pieces)
    n = a_pieces[0].shape[1]
    q, r = list(a_pieces), np.eye(n)
    for _ in range(num_iter - 2):
        q, rk = _sweep(q, shift_of(m, n))
        r = rk @ r
    if gram_guard:
        w = np.linalg.eigvalsh(sum(p.T @ p for p in q))
        cond = math.sqrt(w[-1] / w[0]) if w[0] > 0 else float("inf")
    else:
        cond = float(np.linalg.cond(np.vstack(q)))
    for _ in range(2):
        q, rk = _sweep(q, 0.0)
        r = rk @ r
    return q, np.triu(r), cond


def householder_R(a):
    r = np.linalg.qr(a, mode="r")
    return np.triu(r * np.sign(np.diag(r))[:, None])


def householder_QR(a):
    """Householder QR with the signs that make diag(R) positive"""
    q, r = np.linalg.qr(a)
    sg = np.sign(np.diag(r))
    return q * sg[None, :], np.triu(r * sg[:, None])


def guarded(a, num_iter, gram_guard=False):
    """the restatement of a case, checked before the GPU is touched"""
    q, r, cond = restate(a, num_iter, gram_guard)
    assert np.isfinite(r).all() and np.isfinite(q[0]).all()
    assert cond <= GUARD, "badly chosen input: kappa(Q) entering CholeskyQR2 is %.2e" % cond
    return q[0], r, cond


# ------------------------------------------------------------------------------------------------ the plan
def _factor(a, num_iter):
    from capital_amd import cacqr, cholinv
    from capital_amd.matrix import matrix
    m, n = a.shape
    A = matrix(n, m, 1, 1)
    A.from_numpy(a)
    pack = cacqr.info(num_iter, cholinv.info(1, 1, 0, 'U'))
    cacqr.factor(A, pack, None)
    return A, pack


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rhs_matrix(b):
    from capital_amd.matrix import matrix
    B = matrix(b.shape[1], b.shape[0], 1, 1)
    B.from_numpy(b)
    return B


# (m, n, kappa, num_iter, columns scaled by logspace(0, 8, n)).  n = 256 with m % 128 == 0: gram256 / qrapply256; the others: the generic path
CASES = [
    (8192, 256, 1e9, 3, False),
    (8192, 256, 1e10, 3, False),                # (1e11 enters CholeskyQR2 at 1.3e7 here, 1.7e7 at 16384 rows: above the guard at n = 256)
    (8192, 256, 1e13, 4, False),
    (8192, 256, 1e14, 4, False),
    (16384, 256, 1e10, 3, True),
    (16384, 256, 1e13, 4, False),
    (4100, 96, 1e9, 3, False),
    (4100, 96, 1e11, 3, False),
    (4100, 96, 1e14, 4, False),
    (5000, 37, 1e11, 3, True),
    (5000, 37, 1e13, 4, False),
]


def _check_factor(a, A, pack, num_iter, q_rs, r_rs, r_hh, label, q_hh):
    from capital_amd import cacqr, validate
    m, n = a.shape
    assert pack.last_info() == 0
    Q = cacqr.construct_Q(pack).to_numpy(); R = cacqr.construct_R(pack).to_numpy()
    res, orth = validate.qr.residual(A, pack), validate.qr.orthogonality(A, pack)
    bound = 10.0 * relerr(r_rs, r_hh)
    er, eq = relerr(R, r_rs), relerr(Q, q_rs)
    print("%s: residual %.2e orthogonality %.2e  R vs restatement %.2e  Q vs restatement %.2e  (bound %.2e)  shift %.3e"
          % (label, res, orth, er, eq, bound, pack.shift()))
    assert res < 1e-13
    assert orth < 1e-15
    assert er <= bound
    # the 10 x-of-restatement rule, like for like: R against the restatement's R within 10 x the restatement's distance from Householder's
    # sign-normalised R (above), Q against the restatement's Q within 10 x the restatement's distance from the Q of that same Householder
    # factorization.  The distance of the two R (~ 1.5e-14) cannot bound Q: R is determined to a few u, Q = A R^-1 to kappa(A) u - two
    # evaluations of the restatement on the CPU that differ only in the summation order of the Gram matrix sit 1.3e-15 ... 2.6e-15 apart
    # in R and 1.07e-08 ... 7.31e-04 apart in Q on the inputs of CASES (profiles/r10_scqr.txt, section 5)
    qbound = 10.0 * relerr(q_rs, q_hh)
    print("    Q: restatement vs Householder %.2e, bound %.2e" % (qbound / 10.0, qbound))
    assert eq <= qbound
    assert np.array_equal(np.tril(R, -1), np.zeros_like(R))
    assert (np.diag(R) > 0).all()
    assert pack.shift() == shift_of(m, n)                              # bit for bit
    return Q, R


@pytest.mark.parametrize("m,n,kappa,num_iter,scaled", CASES)
def test_shifted_factor(m, n, kappa, num_iter, scaled):
    a = make_input(m, n, kappa, scaled)
    q_rs, r_rs, cond = guarded(a, num_iter)
    q_hh, r_hh = householder_QR(a)
    A, pack = _factor(a, num_iter)
    label = "%d x %d kappa %.0e%s num_iter %d (kappa entering CholeskyQR2 %.1e)" % (m, n, kappa, " scaled" if scaled else "", num_iter, cond)
    Q, R = _check_factor(a, A, pack, num_iter, q_rs, r_rs, r_hh, label, q_hh)
    # the same plan again: the same bits
    from capital_amd import cacqr
    cacqr.factor(A, pack, None)
    assert pack.last_info() == 0
    assert np.array_equal(cacqr.construct_R(pack).to_numpy(), R)
    assert np.array_equal(cacqr.construct_Q(pack).to_numpy(), Q)


def test_shifted_factor_at_2_to_the_20_rows():
    """2^20 x 256, kappa 1e9, one shifted sweep, the same assertions as the cases above.  Host time stays in seconds: the guard's condition
    number comes from the n x n Gram of the restatement's Q, and Householder's factorization is that of the n x n factor diag(sigma) V^T
    (A = U diag(sigma) V^T with orthonormal U: the same R, and Q = U Q_small)."""
    from capital_amd import cacqr
    m, n, kappa = 1 << 20, 256, 1e9
    rng = np.random.default_rng(20)
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    small = np.logspace(0, -math.log10(kappa), n)[:, None] * v.T
    a = np.ascontiguousarray(u @ small)
    q_small, r_hh = householder_QR(small)
    q_hh = u @ q_small
    del u
    q_rs, r_rs, cond = restate(a, 3, gram_guard=True)
    assert np.isfinite(r_rs).all() and np.isfinite(q_rs[0]).all() and cond <= GUARD, cond
    A, pack = _factor(a, 3)
    Q, R = _check_factor(a, A, pack, 3, q_rs[0], r_rs, r_hh, "2^20 x 256 kappa 1e9 (kappa entering CholeskyQR2 %.1e)" % cond, q_hh)
    del q_rs, q_hh
    cacqr.factor(A, pack, None)                                        # the same plan again: the same bits
    assert pack.last_info() == 0
    assert np.array_equal(cacqr.construct_R(pack).to_numpy(), R)
    assert np.array_equal(cacqr.construct_Q(pack).to_numpy(), Q)


# ------------------------------------------------------------------------------------------------ why the feature exists
def test_cholesky_qr2_alone_fails_at_kappa_1e11():
    from capital_amd import cacqr
    a = make_input(8192, 256, 1e11)
    A, pack = _factor(a, 2)
    assert pack.last_info() != 0
    x = cacqr.solve(pack, _rhs_matrix(np.ones((8192, 2)))).to_numpy()
    assert np.isnan(x).all()


# ------------------------------------------------------------------------------------------------ least squares
def _opt(a, x, b):
    return float(np.linalg.norm(a.T @ (a @ x - b)) / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.mark.parametrize("kappa", [1e9, 1e10])
def test_consistent_least_squares(kappa):
    """b = A x0: the error against x0 within max(10 x the restatement's, 1e-14), the optimality within 10 x the larger of the restatement's
    and lstsq's (lstsq is a fair reference up to kappa ~ 1e11: beyond, its default rcond truncates singular values)"""
    from capital_amd import cacqr
    m, n = 16384, 256
    a = make_input(m, n, kappa)
    x0 = np.random.default_rng(5).standard_normal((n, 3))
    b = a @ x0
    q_rs, r_rs, _ = guarded(a, 3)
    x_rs = np.linalg.solve(r_rs, q_rs.T @ b)
    x_ls = np.linalg.lstsq(a, b, rcond=None)[0]
    A, pack = _factor(a, 3)
    x = cacqr.solve(pack, _rhs_matrix(b)).to_numpy()
    assert pack.last_info() == 0
    err, err_rs = relerr(x, x0), relerr(x_rs, x0)
    opt, opt_rs, opt_ls = _opt(a, x, b), _opt(a, x_rs, b), _opt(a, x_ls, b)
    print("kappa %.0e: error %.2e (restatement %.2e)  optimality %.2e (restatement %.2e, lstsq %.2e)" % (kappa, err, err_rs, opt, opt_rs, opt_ls))
    assert err <= max(10.0 * err_rs, 1e-14)
    assert opt <= 10.0 * max(opt_rs, opt_ls)


# ------------------------------------------------------------------------------------------------ factor_robust
def _matrix_of(a):
    from capital_amd.matrix import matrix
    A = matrix(a.shape[1], a.shape[0], 1, 1)
    A.from_numpy(a)
    return A


def test_factor_robust_escalates():
    from capital_amd import _lib, cacqr, cholinv, validate
    from capital_amd.matrix import matrix
    m, n = 8192, 256
    G = matrix(n, m, 1, 1)
    G.distribute_random(0, 0, 1, 1, 0)
    hard = {3: make_input(m, n, 1e10), 4: make_input(m, n, 1e14)}
    for it, a in hard.items():
        guarded(a, it)
    for A, want in ((G, 2), (_matrix_of(hard[3]), 3), (_matrix_of(hard[4]), 4)):
        pack = cacqr.info(2, cholinv.info(1, 1, 0, 'U'))
        assert cacqr.factor_robust(A, pack) == want
        assert pack.num_iter == want and pack.last_info() == 0
        assert validate.qr.residual(A, pack) < 1e-13 and validate.qr.orthogonality(A, pack) < 1e-15
        x = cacqr.solve(pack, A.view()[:, :2].contiguous()).to_numpy()           # b = the first two columns: x = e_0, e_1
        assert np.isfinite(x).all() and x.shape == (n, 2)
        assert (np.diag(cacqr.construct_R(pack).to_numpy()) > 0).all()
    pack = cacqr.info(2, cholinv.info(1, 1, 0, 'U'))
    with pytest.raises(_lib.CapitalError):
        cacqr.factor_robust(_matrix_of(hard[3]), pack, max_iter=2)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    import ctypes as C
    from capital_amd import _lib, topo
    L = _lib.lib()
    for it in (0, 5):
        h = C.c_void_p()
        assert L.cap_cacqr_plan_create(C.byref(h), 4096, 64, it, None) == 1          # CAP_ERR_ARG
    for it in (1, 2, 3, 4):
        h = C.c_void_p()
        assert L.cap_cacqr_plan_create(C.byref(h), 4096, 64, it, None) == 0
        s = C.c_double(-1.0)
        assert L.cap_cacqr_shift(h, C.byref(s), None) == 0 and s.value == 0.0        # no factor call yet
        L.cap_cacqr_plan_destroy(h)
    T = topo.rect(1)
    try:
        for it in (3, 4):
            h = C.c_void_p()
            assert L.cap_cacqr_plan_create_grid(C.byref(h), 4096, 64, it, T.handle) == 4   # CAP_ERR_UNSUPPORTED
    finally:
        T.close()


def test_unshifted_plans_report_a_zero_shift():
    a = make_input(4100, 96, 1e3)
    for it in (1, 2):
        A, pack = _factor(a, it)
        assert pack.last_info() == 0 and pack.shift() == 0.0


# ------------------------------------------------------------------------------------------------ two ranks on one GPU
def test_two_ranks_unequal_rows():
    """two processes share cuda:0 through the host-staged communicator (tests/scqr_worker.py), 2600 and 1500 rows, num_iter 3, kappa 1e10:
    R bit-identical on both ranks and within 1e-11 of the one-rank R of the stacked matrix; the same shift on both"""
    import tempfile
    import time
    m0, m1, n, kappa = 2600, 1500, 96, 1e10
    a = make_input(m0 + m1, n, kappa)
    guarded(a, 3)
    guarded([a[:m0], a[m0:]], 3)
    A, pack = _factor(a, 3)
    from capital_amd import cacqr
    assert pack.last_info() == 0
    R1 = cacqr.construct_R(pack).to_numpy()
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "a.npy"), a)
        worker = [os.path.join(ROOT, "tests", "scqr_worker.py"), "--dir", d, "--rows", "%d,%d" % (m0, m1), "--num-iter", "3"]
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", OMP_NUM_THREADS="4")
        logs = [open(os.path.join(d, "rank%d.log" % r), "w+") for r in range(2)]
        procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable] + worker, stdout=logs[r], stderr=subprocess.STDOUT, text=True,
                                  env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
        while any(p.poll() is None for p in procs):
            if any(p.returncode for p in procs):                   # a rank that failed leaves its peer inside a collective
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                break
            time.sleep(0.2)
        for p in procs:
            p.wait()
        out = []
        for f in logs:
            f.seek(0); out.append(f.read()); f.close()
        assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in out)
        got = [np.load(os.path.join(d, "rank%d.npz" % r)) for r in range(2)]
    assert int(got[0]["info"]) == 0 and int(got[1]["info"]) == 0
    assert np.array_equal(got[0]["R"], got[1]["R"])
    assert float(got[0]["shift"]) == float(got[1]["shift"]) == shift_of(m0 + m1, n)
    print("two ranks: R vs the one-rank R %.2e" % relerr(got[0]["R"], R1))
    assert relerr(got[0]["R"], R1) < 1e-11
    q = np.vstack([got[0]["Q"], got[1]["Q"]])
    assert np.linalg.norm(q.T @ q - np.eye(n)) / n < 1e-15
    assert relerr(q @ got[0]["R"], a) < 1e-13
