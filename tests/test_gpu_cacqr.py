"""-m gpu: CholeskyQR / CholeskyQR2 1D path through the C ABI vs reference dumps and the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import capital_oracle as orc  # noqa: E402
from tests.gpu_util import relerr  # noqa: E402


def _run(m, n, variant, a=None):
    from capital_amd import cacqr, cholinv
    from capital_amd.matrix import matrix
    A = matrix(n, m, 1, 1)
    if a is None:
        A.distribute_random(0, 0, 1, 1, 0)
    else:
        A.from_numpy(a)
    pack = cacqr.info(variant, cholinv.info(1, 1, 0, 'U'))
    cacqr.factor(A, pack, None)
    return A, pack


@pytest.mark.parametrize("name", ["cacqr1_m192_n12.npz", "cacqr2_m256_n16.npz"])
def test_matches_reference_dump(golden_dir, name):
    from capital_amd import cacqr, validate
    g = np.load(os.path.join(golden_dir, name))
    m, n, variant = int(g["m"]), int(g["n"]), int(g["variant"])
    A, pack = _run(m, n, variant)
    assert np.array_equal(A.to_numpy(), g["A"])                       # upstream's distribute_random, bit exact
    Q = cacqr.construct_Q(pack).to_numpy(); R = cacqr.construct_R(pack).to_numpy()
    assert pack.last_info() == 0
    assert relerr(Q, g["Q"]) < 1e-12
    assert relerr(R, np.triu(g["R"])) < 1e-13
    assert validate.qr.residual(A, pack) < 1e-13                     # SURVEY App. A bars
    assert validate.qr.orthogonality(A, pack) < max(1e-15, 10 * float(g["ref_orthogonality"]))


@pytest.mark.parametrize("name", ["cacqr2_p8_c1_m256_n16.npz", "cacqr2_p8_c2_m256_n16.npz", "cacqr1_p8_c2_m200_n12.npz"])
def test_matches_multirank_reference_dump(golden_dir, name):
    """Q and R of the REAL reference run on 8 MPI ranks (1D path and sweep_3d on 2 x 2 x 2; gathered from the ranks' cyclic
    pieces): the GPU plan on the same global matrix gives the same factorization."""
    from capital_amd import cacqr, validate
    g = np.load(os.path.join(golden_dir, name))
    m, n, variant = int(g["m"]), int(g["n"]), int(g["variant"])
    A, pack = _run(m, n, variant, a=np.ascontiguousarray(g["A"]))
    Q = cacqr.construct_Q(pack).to_numpy(); R = cacqr.construct_R(pack).to_numpy()
    assert pack.last_info() == 0
    assert relerr(Q, g["Q"]) < 1e-12
    assert relerr(R, np.triu(g["R"])) < 1e-13
    assert validate.qr.residual(A, pack) < 1e-13
    assert validate.qr.orthogonality(A, pack) < max(1e-15, 10 * float(g["ref_orthogonality"]))


# (n = 256, m % 128 == 0 runs the dedicated gram256 / qrapply256 kernels: 8192 = one row tile per workgroup, 33024 = 258 row tiles (two per
#  workgroup on 129 workgroups), 70272 = 549 row tiles (three per workgroup, the last workgroup short) - the persistent K loop across row tiles)
@pytest.mark.parametrize("m,n,variant", [(4096, 64, 2), (5000, 37, 2), (8192, 256, 1), (8192, 256, 2), (33024, 256, 1), (70272, 256, 2), (100000, 128, 2), (130, 130, 2)])
def test_matches_oracle(m, n, variant):
    from capital_amd import cacqr, validate
    A, pack = _run(m, n, variant)
    a = A.to_numpy()
    assert np.array_equal(a, orc.random_local(m, n, 0, 0, 1, 1, 0))
    q_ref, r_ref = orc.cacqr_1d([a], variant)
    Q = cacqr.construct_Q(pack).to_numpy(); R = cacqr.construct_R(pack).to_numpy()
    assert pack.last_info() == 0
    assert relerr(R, r_ref) < 1e-11
    assert relerr(Q, q_ref[0]) < 1e-10
    res, orth = validate.qr.residual(A, pack), validate.qr.orthogonality(A, pack)
    assert abs(res - orc.qr_residual(a, Q, R)) < 1e-15
    assert abs(orth - orc.qr_orthogonality(Q)) < 1e-15
    assert res < 1e-13
    if variant == 2:
        assert orth < 1e-15
    assert np.array_equal(np.tril(R, -1), np.zeros_like(R))


def test_tall_skinny_properties_at_scale():
    """2^21 x 256 per GPU (the per-rank shape of BASELINE config 4): properties only."""
    from capital_amd import validate
    A, pack = _run(1 << 21, 256, 2)
    assert pack.last_info() == 0
    assert validate.qr.residual(A, pack) < 1e-13
    assert validate.qr.orthogonality(A, pack) < 1e-15


# ------------------------------------------------------------------------------------------------ plan state across a failed call
# csrc/cacqr.hip sweep() zero-fills Gi once per plan (n = 256: gi_clean) and relies on the 64-blocked factor rewriting every entry of Gi
# it ever wrote and never touching the blocks below.  m = 1024, n = 256 runs gram256 / qrapply256 and, in cap_rec_cholinv_full, the
# one-launch chain of csrc/cholinv.hip blocked_cholinv (n = 256 = 4 blocks of 64, 32 cooperative workgroups by default: `coop >= 2 &&
# nblk >= 4`), so both ways a factor call can leave the clean path are reachable here: a failed factorization and the chain's recovery launch.
REUSE_M, REUSE_N = 1024, 256


def _reuse_inputs():
    rng = np.random.default_rng(20)
    a = rng.standard_normal((REUSE_M, REUSE_N))
    b = rng.standard_normal((REUSE_M, REUSE_N))
    b[:, 100] = 0.0                                   # a zero column: the Gram matrix has a zero pivot, the factorization fails
    return a, b


def _factor_on(pack, a):
    from capital_amd import cacqr
    from capital_amd.matrix import matrix
    A = matrix(REUSE_N, REUSE_M, 1, 1)
    A.from_numpy(a)
    cacqr.factor(A, pack, None)
    info = pack.last_info()
    return cacqr.construct_Q(pack).to_numpy(), cacqr.construct_R(pack).to_numpy(), info


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))


@pytest.mark.parametrize("variant", [1, 2])
def test_plan_is_clean_after_a_failed_factor_call(variant):
    """factor A, factor a matrix with a zero column on the SAME plan (info != 0), factor A again: Q and R have the bits of the first call
    and of a fresh plan - nothing of the failed call's R^-1 survives in the blocks the next call does not rewrite"""
    from capital_amd import cacqr, cholinv
    a, b = _reuse_inputs()
    pack = cacqr.info(variant, cholinv.info(1, 1, 0, 'U'))
    q0, r0, info0 = _factor_on(pack, a)
    assert info0 == 0 and np.isfinite(q0).all() and np.isfinite(r0).all()
    plan = pack._plan
    _, _, info1 = _factor_on(pack, b)
    assert info1 != 0
    q2, r2, info2 = _factor_on(pack, a)
    assert pack._plan is plan and info2 == 0
    assert _same_bits(q2, q0) and _same_bits(r2, r0)
    qf, rf, infof = _factor_on(cacqr.info(variant, cholinv.info(1, 1, 0, 'U')), a)
    assert infof == 0 and _same_bits(qf, q0) and _same_bits(rf, r0)


@pytest.mark.parametrize("variant", [1, 2])
def test_plan_is_clean_after_a_chain_fallback(variant):
    """the same with the middle call's first diagonal-block chain giving up at its first meeting (cap_chain_inject_timeouts: the recovery
    launch restores the block and re-runs the sweep): that call itself and the next one give the bits of an undisturbed call"""
    from capital_amd import _lib, cacqr, cholinv
    L = _lib.lib()
    a, b = _reuse_inputs()
    b[:, 100] = a[:, 3]                               # (a full-rank matrix for the middle call)
    pack = cacqr.info(variant, cholinv.info(1, 1, 0, 'U'))
    q0, r0, info0 = _factor_on(pack, a)
    qb, rb, infob = _factor_on(cacqr.info(variant, cholinv.info(1, 1, 0, 'U')), b)
    assert info0 == 0 and infob == 0
    before = L.cap_chain_fallbacks()
    assert before >= 0
    _lib.check(L.cap_chain_inject_timeouts(1), "cap_chain_inject_timeouts")
    try:
        q1, r1, info1 = _factor_on(pack, b)
    finally:
        _lib.check(L.cap_chain_inject_timeouts(0), "cap_chain_inject_timeouts")       # (never leave a pending injection behind)
    assert L.cap_chain_fallbacks() == before + 1, "the factor of n = 256 did not take the chain"
    assert info1 == 0 and _same_bits(q1, qb) and _same_bits(r1, rb)
    q2, r2, info2 = _factor_on(pack, a)
    assert info2 == 0 and _same_bits(q2, q0) and _same_bits(r2, r0)
