"""-m gpu: STREAM ORDER.  Every other GPU test passes the NULL stream, fills its inputs with synchronous copies and synchronises the device
before it reads a result, so a helper stream that does not wait for the caller's earlier work, or is not joined back before the call "ends"
in stream order, is invisible to it.  Here every entry runs as an ORDERED CALL (tests/stream_order.py): on a non-blocking stream of the
test's own, behind a device-side delay, with inputs that are poison until a device-to-device copy on that stream delivers them, with
snapshots and a poison fill of every buffer behind the call on that stream, and with a host that waits for that stream alone.  The
premise - the host had enqueued everything before the delay ran out - is asserted for every case ("premise not met" otherwise).

References.  The exact-result tables of the other suites (blas3_cases, tri_cases, chol_cases, cqr256_cases, the integer batches of the
batched tests, the integer operands of the thin-product, tall-product and pivoted tests): a reordered read cannot hide in rounding there.
Where no exact reference exists (update / downdate, condition estimate, error bounds, mixed precision, CholeskyQR) the reference is the
same call on the NULL stream with synchronous inputs and a device synchronisation, in a fresh plan, BIT FOR BIT: the value is the business
of the other suites, what is asserted here is that ordering does not change a bit.

No test of this file synchronises the device before its snapshots are compared: torch.cuda.synchronize() appears in the harness only, in
the dangling-work check behind each case and in the reference runs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import blas3_cases as B3  # noqa: E402
from tests import chol_cases as CH  # noqa: E402
from tests import cholupdate_model as cm  # noqa: E402
from tests import cqr256_cases as Q256  # noqa: E402
from tests import pstrf_model as pm  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import tri_cases as TR  # noqa: E402
from tests.stream_order import Job, positive_zero, same_bits  # noqa: E402

NAN = np.float64("nan")
UPPER = 1
# Delays.  20 ms unless a case's calls took more than 3 ms to enqueue on the MI355X host (profiles/r20_stream_order.txt): cap_dpotrf (6.8 ms:
# it makes its panel stream and events per call) and the first column-split factor of a plan (14.2 ms: a third stream, eight events and its
# buffers on first use) get 60 ms, the sequences of up to 13 calls on one plan 40 ms.
SEQUENCE_DELAY_MS = 40.0
SLOW_ENQUEUE_DELAY_MS = 60.0


def _L():
    from capital_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def env():
    e = SO.Env(2)
    L = _L()
    # the counter words that potrs.hip, cholupdate.hip, pocon.hip and leaf.hip keep per device are made (and the device synchronised once)
    # by the first call of the process that needs them: make them here, outside every timed call
    for f in (L.cap_solve_fallbacks, L.cap_update_fallbacks, L.cap_chain_fallbacks, L.cap_pocon_last_solves):
        assert f() >= 0
    yield e
    print("stream order: %d ordered calls; longest enqueue %.2f ms of a %.0f ms delay" % (
        len(e.records), max([max(r[2]) for r in e.records if not r[4]] or [0.0]), max([r[1] for r in e.records] or [0.0])))
    e.close()


def _nan(count):
    return np.full(max(int(count), 1), NAN)


def _check(job, want=None, zero_fix=(), what="", skip=()):
    """every snapshot bit for bit: `want` where given, else the buffer's own contents before the call (an input must come back unchanged);
    `skip`: outputs that this comparison has no reference for"""
    want = want or {}
    for name, got in job.snap.items():
        if name in skip:
            continue
        w = want.get(name, job.bufs[name])
        g = got
        if name in zero_fix:
            g, w = positive_zero(g), positive_zero(w)
        assert same_bits(g, w), "%s %s, %s: %s" % (job.label, what, name, B3.describe_mismatch(g, w, max(len(w), 1)) if g.dtype == np.float64 else (g, w))


def _row(cases, cid):
    hit = [c for c in cases if c.id == cid]
    assert len(hit) == 1, (cid, [c.id for c in cases][:50])
    return hit[0]


def test_the_caller_streams_are_non_blocking_and_not_the_null_stream(env):
    import torch
    for s in env.streams:
        assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.default_stream().cuda_stream
        assert env.flags(s) == SO.HIP_STREAM_NON_BLOCKING
    assert env.cycles_per_ms > 1000


# ============================================================================================================ exact reference, plan-less
def _blas3_job(c, seed, ab=0):
    L = _L()
    alpha, beta = c.ab[ab]
    ops, ld = B3.operands(c, seed), B3.lds(c)
    offs = dict(zip(("T", "B") if c.op == "trmm" else ("A", "B"), c.offs))
    out = "B" if c.op == "trmm" else "C"
    host = {name: B3.place(B3.initial_output(c, ops, beta) if name == out else mat, ld[name], offs.get(name, 0)) for name, mat in ops.items()}
    if c.op == "trmm":
        host["work"] = _nan(L.cap_dtrmm_work_size(0 if c.form[0] == "L" else 1, c.m, c.n))
    tr = B3.CAP_TRANS

    def enqueue(ptr, stream):
        p = {k: v + 8 * offs.get(k, 0) for k, v in ptr.items()}
        if c.op == "gemm":
            st = L.cap_dgemm(tr[c.form[0]], tr[c.form[1]], c.m, c.n, c.k, alpha, p["A"], ld["A"], p["B"], ld["B"], beta, p["C"], ld["C"], stream)
        elif c.op == "syrk":
            st = L.cap_dsyrk(1 if c.form[0] == "U" else 0, tr[c.form[1]], c.n, c.k, alpha, p["A"], ld["A"], beta, p["C"], ld["C"], stream)
        else:
            st = L.cap_dtrmm(0 if c.form[0] == "L" else 1, UPPER, tr[c.form[1]], 0, c.m, c.n, alpha, p["T"], ld["T"], p["B"], ld["B"], p["work"], stream)
        assert st == 0, (c.id, st)
    want = {out: B3.place(B3.exact_reference(c, ops, alpha, beta), ld[out], offs.get(out, 0))}
    return Job(host, enqueue, scratch=("work",) if c.op == "trmm" else (), label=c.id), want


# one tile-kernel row, one split-K row and one skinny / small-kernel row per operator (TRMM has no split-K route: a ragged row instead)
BLAS3_IDS = ("gemm-TN-384x256x48", "gemm-TN-256x256x5008", "gemm-NT-130x258x4100-pad2", "gemm-TN-2048x8x1024", "gemm-NN-2048x8x1024",
             "syrk-UT-384x384x80", "syrk-UT-256x256x6000", "syrk-LN-130x130x512-pad1",
             "trmm-LN-1024x1024x1024-pad2", "trmm-RN-1024x1152x1152-pad2", "trmm-LT-1000x700x1000-pad2")


@pytest.mark.parametrize("cid", BLAS3_IDS)
def test_blas3_ordered(env, cid):
    c = _row(B3.CASES, cid)
    job, want = _blas3_job(c, 100 + B3.CASES.index(c))
    with env.ordered(job, label=cid) as j:
        _check(j, want)


def _tri_job(c):
    L = _L()
    ops, ld = TR.operands(c), TR.lds(c)
    host = {"T": B3.place(TR.stored(ops["T"]), ld["T"])}
    if "B" in ops:
        host["B"] = B3.place(ops["B"], ld["B"])
    host["work"] = _nan(c.woff + TR.work_size(L, c))

    def enqueue(ptr, stream):
        assert TR.call(L, c, ptr["T"], ptr.get("B"), ptr["work"] + 8 * c.woff, ld, stream) == 0, c.id
    out = "T" if c.op in ("trtri", "potri") else "B"
    return Job(host, enqueue, scratch=("work",), label=c.id), {out: B3.place(TR.reference(c, ops), ld[out])}, out


def _tri_rows():
    pick = lambda rows, **kw: next(c for c in rows if all(c[k] == v for k, v in kw.items()))          # noqa: E731
    return [pick(TR.TRTRI_CASES, n=640, fam="F1"), pick(TR.TRTRI_CASES, n=1000, fam="F2i"),
            pick(TR.TRSM_CASES, n=640, form="LN"), pick(TR.TRSM_CASES, n=1000, form="RT"),
            pick(TR.POTRS_CASES, n=1153, other=1), pick(TR.POTRS_CASES, n=1153, other=16), pick(TR.POTRS_CASES, n=640),
            pick(TR.POTRS_CASES, n=1000, other=40),                                                   # the blocked route
            pick(TR.POTRI_CASES, n=640), pick(TR.POTRI_CASES, n=1155)]


@pytest.mark.parametrize("c", _tri_rows(), ids=lambda c: c.id)
def test_triangular_ordered(env, c):
    TR.check_premise(c)
    job, want, out = _tri_job(c)
    with env.ordered(job, label=c.id) as j:
        _check(j, want, zero_fix=(out,))


def _dpotrf_job(c):
    L = _L()
    lda = c.n + c.pad
    host = {"A": B3.place(CH.operand(c), lda), "info": np.full(2, -1, dtype=np.int32), "work": _nan(L.cap_dpotrf_work_size(c.n))}

    def enqueue(ptr, stream):
        assert L.cap_dpotrf(UPPER, c.n, ptr["A"], lda, ptr["info"], ptr["work"], stream) == 0, c.id
    return Job(host, enqueue, scratch=("work",), label=c.id), {"A": B3.place(CH.dpotrf_reference(c), lda), "info": np.array([0, -1], dtype=np.int32)}


@pytest.mark.parametrize("cid", ("dpotrf-n1100-pad2", "dpotrf-n4096-pad2"))
def test_dpotrf_ordered(env, cid):
    """several panels; n = 4096 is where cap_dpotrf's look-ahead starts using the panel stream it keeps per device"""
    c = _row(CH.DPOTRF_CASES, cid)
    job, want = _dpotrf_job(c)
    with env.ordered(job, label=cid, delay_ms=SLOW_ENQUEUE_DELAY_MS) as j:
        _check(j, want, zero_fix=("A",))


def test_gram256_and_qrapply256_ordered(env):
    L = _L()
    N = Q256.N
    m, cap, ldq, ldg = 2560, 0, 2560 + 2, N + 3                 # 5 slabs: the reduce adds two of them in one group
    q = Q256.panel(m)
    host = {"Q": Q256.place_cols(q, ldq).ravel(), "G": _nan(N * ldg), "work": _nan(L.cap_dgram256_work_size(m))}

    def gram(ptr, stream):
        assert L.cap_dgram256(m, ptr["Q"], ldq, ptr["G"], ldg, ptr["work"], cap, stream) == 0
    with env.ordered(Job(host, gram, scratch=("work",), label="gram256 m=2560"), label="gram256 m=2560") as j:
        _check(j, {"G": Q256.place_cols(Q256.gram_reference(m), ldg).ravel()})
    m, cap, ldin, ldout = 1664, 3, 1664 + 2, 1664 + 6           # 13 row tiles on 3 persistent workgroups
    q, ri = Q256.panel(m), Q256.ri_dense(m + cap)
    host = {"Qin": Q256.place_cols(q, ldin).ravel(), "Ri": ri.ravel().copy(), "Qout": _nan(N * ldout)}

    def apply(ptr, stream):
        assert L.cap_dqrapply256(m, ptr["Qin"], ldin, ptr["Ri"], ptr["Qout"], ldout, cap, stream) == 0
    with env.ordered(Job(host, apply, label="qrapply256 m=1664"), label="qrapply256 m=1664") as j:
        _check(j, {"Qout": Q256.place_cols(Q256.apply_reference(q, ri), ldout).ravel()})


def _blocks(blocks, ld, stride, upper_only):
    """flat buffer of blocks[i] (rows x cols, column-major, leading dimension ld) at i * stride; NaN everywhere else and, with upper_only,
    in the strictly lower triangles"""
    batch, rows, cols = blocks.shape
    flat = np.full((batch - 1) * stride + ld * cols + 5, NAN)
    for i in range(batch):
        w = flat[i * stride:i * stride + ld * cols].reshape(cols, ld)
        b = blocks[i].copy()
        if upper_only:
            b[np.tril_indices(rows, -1)] = NAN
        w[:, :rows] = b.T
    return flat


def _batched_job(n, batch, nrhs, seed_shift=0):
    L = _L()
    if n <= 64:
        from tests.test_gpu_potrf_batched import integer_batch
        R, A, X, B = integer_batch(n, batch + seed_shift)[:4]
        fac, sol = L.cap_dpotrf_batched, L.cap_dpotrs_batched
    else:
        from tests.test_gpu_potrf_batched_blocked import integer_batch
        R, A, X, B = integer_batch(n, batch + seed_shift)
        fac, sol = L.cap_dpotrf_batched_blocked, L.cap_dpotrs_batched_blocked
    R, A, X, B = R[seed_shift:], A[seed_shift:], X[seed_shift:, :, :nrhs], B[seed_shift:, :, :nrhs]
    lda = n + 1
    sa, sb = lda * n + 3, lda * nrhs + 3
    host = {"A": _blocks(A, lda, sa, True), "B": _blocks(B, lda, sb, False), "info": np.full(batch + 1, SO.POISON_I32 ^ 0x1111, dtype=np.int32),
            "logdet": _nan(batch + 1)}

    def enqueue(ptr, stream):          # factor, then solve with the factor and the info the first call wrote: one sequence
        assert fac(UPPER, n, ptr["A"], lda, sa, batch, ptr["info"], ptr["logdet"], stream) == 0
        assert sol(UPPER, n, nrhs, ptr["A"], lda, sa, ptr["B"], lda, sb, batch, ptr["info"], stream) == 0
    info = host["info"].copy()
    info[:batch] = 0
    want = {"A": _blocks(R, lda, sa, True), "B": _blocks(X, lda, sb, False), "info": info}
    return Job(host, enqueue, label="batched n=%d batch=%d nrhs=%d" % (n, batch, nrhs)), want


@pytest.mark.parametrize("n", (33, 64, 65, 193))
def test_batched_factor_then_solve_ordered(env, n):
    job, want = _batched_job(n, 37, 17)
    ref, _ = env.plain(job)                                       # logdet has no exact reference: the NULL-stream run's bits
    assert not np.isnan(ref["logdet"][:37]).any() and np.isnan(ref["logdet"][37])
    want["logdet"] = ref["logdet"]
    _check(_as_snap(job, ref), want)
    with env.ordered(job, label=job.label) as j:
        _check(j, want)


def _as_snap(job, snap):
    """a reference run's buffers dressed as a job, so that _check applies to them as well"""
    j = Job(job.bufs, None, job.scratch, job.label + " (NULL-stream reference)")
    j.snap = snap
    return j


def test_symm_thin_and_lansy_ordered(env):
    from tests.test_gpu_symm_thin import _ints, _sym
    L = _L()
    n, nrhs, alpha, beta = 2 * 512 + 1, 17, 2.0, -1.0           # three super-block rows, two chunks of right-hand sides
    rng = np.random.default_rng(17 * n + nrhs)
    a, a_up = _sym(rng, n)
    x, b = _ints(rng, (n, nrhs)), _ints(rng, (n, nrhs))
    lda, ldx, ldb, ldy = n + 2, n + 1, n + 4, n + 6
    host = {"A": B3.place(a_up, lda), "X": B3.place(x, ldx), "B": B3.place(b, ldb), "Y": _nan(ldy * nrhs),
            "work": _nan(max(L.cap_dsymm_thin_work_size(n, nrhs), 2))}

    def symm(ptr, stream):
        assert L.cap_dsymm_thin(UPPER, 0, n, nrhs, alpha, ptr["A"], lda, ptr["X"], ldx, beta, ptr["B"], ldb, ptr["Y"], ldy, ptr["work"], stream) == 0
    with env.ordered(Job(host, symm, scratch=("work",), label="dsymm_thin n=1025 nrhs=17"), label="dsymm_thin n=1025 nrhs=17") as j:
        _check(j, {"Y": B3.place(beta * b + alpha * (a @ x), ldy)})
    host = {"A": B3.place(a_up, lda), "out": np.full(3, -5.0), "work": _nan(max(L.cap_dlansy_work_size(n), 2))}

    def lansy(ptr, stream):
        assert L.cap_dlansy(ord("1"), UPPER, n, ptr["A"], lda, ptr["out"] + 8, ptr["work"], stream) == 0
    with env.ordered(Job(host, lansy, scratch=("work",), label="dlansy n=1025"), label="dlansy n=1025") as j:
        _check(j, {"out": np.array([-5.0, np.abs(a).sum(0).max(), -5.0])})


@pytest.mark.parametrize("m,n,nrhs", [(4096, 256, 8), (4096, 64, 100)])
def test_tall_tn_ordered(env, m, n, nrhs):
    """nrhs = 8: the streaming kernel with its slab reduce; nrhs = 100: beyond 48 right-hand sides, the tile kernels of cap_dgemm"""
    from tests.test_gpu_cacqr_solve import _ints
    L = _L()
    q, b = _ints(m, n, nrhs, 1000 + m + n + nrhs)
    ldq, ldb, ldz = m + 2, m + 2, n + 1
    host = {"Q": B3.place(q, ldq), "B": B3.place(b, ldb), "Z": _nan(ldz * nrhs), "work": _nan(max(L.cap_dgemm_tall_tn_work_size(m, n, nrhs), 2))}

    def enqueue(ptr, stream):
        assert L.cap_dgemm_tall_tn(m, n, nrhs, ptr["Q"], ldq, ptr["B"], ldb, ptr["Z"], ldz, ptr["work"], stream) == 0
    label = "dgemm_tall_tn %dx%d nrhs=%d" % (m, n, nrhs)
    with env.ordered(Job(host, enqueue, scratch=("work",), label=label), label=label) as j:
        _check(j, {"Z": B3.place(q.T @ b, ldz)}, zero_fix=("Z",))


@pytest.mark.parametrize("n,flip,cap", [(12, 2, 12), (12, 1, 6), (7, 0, 7)])
def test_pstrf_ordered(env, n, flip, cap):
    """the exact integer matrices of tests/test_gpu_pstrf.py: one launch per possible step, every one behind the other on the caller's stream"""
    L = _L()
    A, _, _ = pm.exact_integer(n, flip)
    Rm, pivm, rankm, residm, infom, _ = pm.pstrf(A, cap)
    lda, ldr = n + 3, cap + 2
    a_up = np.array(A)
    a_up[np.tril_indices(n, -1)] = NAN
    host = {"A": B3.place(a_up, lda), "R": _nan(ldr * n), "piv": np.full(n + 1, -7, dtype=np.int64), "rank": np.full(2, -7, dtype=np.int64),
            "info": np.full(2, -7, dtype=np.int32), "resid": _nan(2), "work": _nan(L.cap_dpstrf_work_size(n, cap) + 1)}

    def enqueue(ptr, stream):
        assert L.cap_dpstrf(UPPER, n, cap, -1.0, ptr["A"], lda, ptr["R"], ldr, ptr["piv"], ptr["rank"], ptr["resid"], ptr["info"], ptr["work"], stream) == 0
    label = "dpstrf n=%d flip=%d max_rank=%d" % (n, flip, cap)
    want = {"R": B3.place(np.asarray(Rm, dtype=np.float64), ldr), "piv": np.append(pivm, -7).astype(np.int64), "rank": np.array([rankm, -7], dtype=np.int64),
            "info": np.array([infom, -7], dtype=np.int32), "resid": np.array([residm, NAN])}
    with env.ordered(Job(host, enqueue, scratch=("work",), label=label), label=label) as j:
        _check(j, want)


# =========================================================================================================== exact reference, cap_cholinv plan
def _plan_factor_job(c, plan, seconds=(False,)):
    """factor -> get_R (-> get_Rinv) for each matrix of `seconds`, back to back on the one plan"""
    L = _L()
    n, lda = c.n, c.n + c.pad
    host, want = {}, {}
    for s in seconds:
        R, Rinv = CH.references(c, s)
        host["A%d" % s], host["R%d" % s], want["R%d" % s] = B3.place(CH.operand(c, s), lda), _nan(n * n), B3.place(R, n)
        if Rinv is not None:
            host["Rinv%d" % s], want["Rinv%d" % s] = _nan(n * n), B3.place(Rinv, n)

    def enqueue(ptr, stream):
        for s in seconds:
            assert L.cap_cholinv_factor(plan, ptr["A%d" % s], lda, stream) == 0, c.id
            assert L.cap_cholinv_get_R(plan, ptr["R%d" % s], n, stream) == 0
            if "Rinv%d" % s in ptr:
                assert L.cap_cholinv_get_Rinv(plan, ptr["Rinv%d" % s], n, stream) == 0
    return Job(host, enqueue, label=c.id), want


def _chol_rows():
    """rows of chol_cases with n <= 1280 where the table has one, else the table's option set at such a size (CH._row derives what it launches)"""
    def pick(n, ci, **opts):
        return next(c for c in CH.SWEEP_CASES if c.n == n and ci in (None, c.ci) and all(c.opt.get(k) == v for k, v in opts.items()))
    rows = [CH._row("plan", 1280, "column-split look-ahead", ci=-1, opts={"nb": 128, "outer": 256, "inner_la": 1}, pad=2),
            pick(1024, None, fuse_copy=1, use_sb=1), pick(1024, None, fuse_copy=1, use_sb=0),            # strip buffers on / off
            pick(1280, -1, depth2=1, pair_rest=1),                                                   # exactly one paired far update
            pick(1100, 1, nb=128),                                                                   # the inverse tree, overlapped
            CH._row("plan", 1100, "tree after the join", ci=1, opts={"nb": 128, "inv_overlap": 0}, pad=2),
            CH._row("plan", 1280, "tree enqueued from the first panel on", ci=0, opts={"nb": 128, "inv_start_m": 1 << 30}, pad=0)]
    return rows


@pytest.mark.parametrize("c", _chol_rows(), ids=lambda c: c.id)
def test_cholinv_factor_get_R_get_Rinv_ordered(env, c):
    """the look-ahead, strip-buffer, far-update and inverse-tree streams of a factor call fork from the caller's stream behind the copy that
    delivers A and are joined before get_R / get_Rinv (and the poison fill of A) run"""
    CH.check_premise(c)
    L = _L()
    plan = CH.create_plan(L, c)
    try:
        job, want = _plan_factor_job(c, plan)
        with env.ordered(job, label=c.id, delay_ms=SLOW_ENQUEUE_DELAY_MS if c.opt.get("inner_la") else SO.DEFAULT_DELAY_MS) as j:
            _check(j, want, zero_fix=tuple(want))
        assert CH.plan_info(L, plan, None) == 0
        assert int(L.cap_cholinv_get_option(plan, b"count_paired")) == c.k2, (c.id, "count_paired")
    finally:
        assert L.cap_cholinv_plan_destroy(plan) == 0


@pytest.mark.parametrize("c", CH.REUSE_CASES[:2], ids=lambda c: c.id)
def test_second_factor_does_not_touch_R_before_the_caller_has_copied_it(env, c):
    """REUSE HAZARD: factor(A1) -> get_R -> factor(A2) -> get_R back to back.  The first copy must be R1 exactly: the second factor's helper
    streams may not write the plan's R (or its strip buffers) before the caller's stream has read it"""
    CH.check_premise(c)
    L = _L()
    plan = CH.create_plan(L, c)
    try:
        job, want = _plan_factor_job(c, plan, seconds=(False, True))
        with env.ordered(job, label=c.id + " (two factors back to back)", delay_ms=SEQUENCE_DELAY_MS) as j:
            _check(j, want, zero_fix=tuple(want))
        assert CH.plan_info(L, plan, None) == 0
    finally:
        assert L.cap_cholinv_plan_destroy(plan) == 0


SEQ_N, SEQ_NB = 1024, 128
SEQ_INEXACT = ("logdet", "rcond", "ferr", "berr", "X3", "X4")          # no exact reference: the bits of the NULL-stream run


def _sequence_operands():
    """dyadic data: R = diag(2^k) (I + N) of chol_cases, integer X, B = A X exactly; V small dyadic columns"""
    R, Rinv, N, d = CH.factor_pair(SEQ_N)
    A = CH.spd(SEQ_N)
    rng = np.random.default_rng(2020)
    X = TR.RHS_VALUES[rng.integers(0, 6, size=(SEQ_N, 17))]
    B = A @ X
    V = TR.RHS_VALUES[rng.integers(0, 6, size=(SEQ_N, 3))] / 8.0
    # the premise of exactness of the solves (tri_cases.bounds for POTRS, with these right-hand sides) and of the inverse (POTRI)
    Mi, Tsu = TR._comparison(N, d), np.abs(np.triu(R, 1))
    bf, Yc = TR._substitution_bound(Mi, Tsu, np.abs(B), True)
    bb, _ = TR._substitution_bound(Mi, Tsu, Yc, False)
    assert max(bf, bb) * 32 < TR.LIMIT and (np.abs(A) @ np.abs(X)).max() * 4 < TR.LIMIT, "the premise of exactness of the solves"
    assert (np.abs(Rinv) @ np.abs(Rinv).T).max() * 16 < TR.LIMIT and TR._inverse_route_bound(R, Rinv, SEQ_N) * 32 < TR.LIMIT, "... of the inverse"
    Ainv = Rinv @ Rinv.T
    return A, X, B, V, Ainv


def _sequence_job(plan, ci, with_info=False):
    """factor -> solve(3) -> solve(17) -> logdet -> inverse(fill = 1) [-> update(+V) -> solve -> update(-V) -> solve] -> rcond -> error_bounds ->
    factor -> solve, no host synchronisation in between; every call writes buffers of its own so that the snapshots keep all of them"""
    L = _L()
    n = SEQ_N
    A, X, B, V, Ainv = _sequence_operands()
    host = {"A": B3.place(CH.stored(A), n + 2), "B": B3.place(B, n), "V": B3.place(V, n + 1), "Ainv": _nan(n * n), "logdet": _nan(2), "rcond": _nan(2),
            "ferr": _nan(4), "berr": _nan(4)}
    for k, w in (("X1", 3), ("X2", 17), ("X3", 3), ("X4", 3), ("X5", 3)):
        host[k] = _nan(n * w)

    def enqueue(ptr, stream):
        def solve(name, nrhs):
            assert L.cap_cholinv_solve(plan, ptr["B"], n, ptr[name], n, nrhs, stream) == 0
        assert L.cap_cholinv_factor(plan, ptr["A"], n + 2, stream) == 0
        solve("X1", 3)
        solve("X2", 17)
        assert L.cap_cholinv_logdet(plan, ptr["logdet"], stream) == 0
        assert L.cap_cholinv_inverse(plan, ptr["Ainv"], n, 1, stream) == 0
        if ci == -1:
            assert L.cap_cholinv_update(plan, 1, ptr["V"], n + 1, 3, stream) == 0
            solve("X3", 3)
            assert L.cap_cholinv_update(plan, -1, ptr["V"], n + 1, 3, stream) == 0
            solve("X4", 3)
        assert L.cap_cholinv_rcond(plan, ptr["A"], n + 2, None, ptr["rcond"], stream) == 0
        assert L.cap_cholinv_error_bounds(plan, ptr["A"], n + 2, ptr["B"], n, ptr["X1"], n, 3, ptr["ferr"], ptr["berr"], stream) == 0
        assert L.cap_cholinv_factor(plan, ptr["A"], n + 2, stream) == 0
        solve("X5", 3)
        if with_info:                     # (the reference run only: cap_cholinv_info synchronises the stream)
            return {"info": CH.plan_info(L, plan, stream)}
    exact = {"X1": B3.place(X[:, :3], n), "X2": B3.place(X, n), "X5": B3.place(X[:, :3], n), "Ainv": B3.place(Ainv, n)}
    return Job(host, enqueue, label="cholinv sequence ci=%d" % ci), exact


def _seq_plan(ci, opts=()):
    c = CH._row("plan", SEQ_N, "sequence", ci=ci, opts=dict((("nb", SEQ_NB),) + tuple(opts)))
    return CH.create_plan(_L(), c)


@pytest.mark.parametrize("ci,opts", [(-1, ()), (-1, (("solve_kernel", 0),)), (-1, (("chud_kernel", 0),)), (0, ()), (1, ())],
                         ids=["ci-1", "ci-1-solve_kernel0", "ci-1-chud_kernel0", "ci0", "ci1"])
def test_cholinv_plan_sequence_ordered(env, ci, opts):
    """the calls that share the plan's block inverses ("whichever runs first makes them"), its first-use scratch and its helper streams, in one
    sequence behind the delay.  The solves in front of the first update, the inverse and the solve behind the second factor are EXACT; what
    follows an update (and logdet, rcond, the error bounds) is compared bit for bit with the same sequence on the NULL stream in a fresh plan"""
    L = _L()
    ref_plan = _seq_plan(ci, opts)
    try:
        rjob, exact = _sequence_job(ref_plan, ci, with_info=True)
        ref, rret = env.plain(rjob)
        assert rret["info"] == 0, "the downdate of the reference run failed: the data of this test is wrong"
    finally:
        assert L.cap_cholinv_plan_destroy(ref_plan) == 0
    for k in ("logdet", "rcond"):
        assert np.isfinite(ref[k][0]) and np.isnan(ref[k][1])
    assert np.isfinite(ref["ferr"][:3]).all() and np.isfinite(ref["berr"][:3]).all() and np.isnan(ref["ferr"][3])
    if ci == -1:
        assert np.isfinite(ref["X3"]).all() and np.isfinite(ref["X4"]).all()
    _check(_as_snap(rjob, ref), exact, zero_fix=tuple(exact), skip=SEQ_INEXACT)           # the reference run itself: exact where that is defined
    plan = _seq_plan(ci, opts)
    try:
        # first pass over a fresh plan: solve(17) after solve(3) and error_bounds after rcond need more plan scratch than the call in front of
        # them, and growing it is the one host synchronisation the header allows these calls - exempt from the timing premise, like the calls
        # documented as synchronising.  Second pass, same plan: nothing grows any more, so NOTHING may synchronise: the premise holds in full.
        for first_pass in (True, False):
            job, exact = _sequence_job(plan, ci, with_info=first_pass)          # (cap_cholinv_info synchronises the stream: in the exempt pass only)
            label = "cholinv sequence ci=%d %s, %s pass" % (ci, dict(opts) or "", "first" if first_pass else "second")
            with env.ordered(job, label=label, delay_ms=SEQUENCE_DELAY_MS, exempt=first_pass) as j:
                assert not first_pass or j.ret["info"] == 0
                want = dict(ref)          # the NULL-stream run's bits for what has no exact reference (and the untouched inputs) ...
                want.update(exact)        # ... and the exact results where they are defined
                _check(j, want, zero_fix=tuple(exact))
            assert CH.plan_info(L, plan, None) == 0
    finally:
        assert L.cap_cholinv_plan_destroy(plan) == 0


# =================================================================================== no exact reference: the NULL-stream run, bit for bit
def _against_plain(env, make_job, label, delay_ms=SO.DEFAULT_DELAY_MS, exempt=False, sane=None):
    """make_job() -> (Job, release): once for the reference run (NULL stream, synchronous inputs, device synchronised), once ordered"""
    job, release = make_job()
    try:
        ref, rret = env.plain(job)
    finally:
        release()
    if sane:
        sane(ref, rret)
    job, release = make_job()
    try:
        with env.ordered(job, label=label, delay_ms=delay_ms, exempt=exempt) as j:
            _check(j, ref, what="(against the NULL-stream run)")
            if isinstance(rret, dict):
                for k, v in rret.items():
                    got = j.ret[k]
                    assert same_bits(got, v) if isinstance(v, np.ndarray) else got == v, "%s: %s differs from the NULL-stream run" % (label, k)
    finally:
        release()
    return ref, rret


def _cholupdate_job(n, k, sign, seed=0):
    L = _L()
    A, V = cm.spd(n, 10 + n + seed), cm.thin(n, k, 100 + n + seed)
    R = np.linalg.cholesky(A + (V @ V.T if sign < 0 else 0.0)).T
    ldr, ldv = n + 1, n + 2
    host = {"R": B3.place(TR.stored(R), ldr), "V": B3.place(V, ldv), "info": np.full(2, -9, dtype=np.int32), "work": _nan(L.cap_dcholupdate_work_size(n, k))}

    def enqueue(ptr, stream):
        assert L.cap_dcholupdate(UPPER, sign, n, k, ptr["R"], ldr, ptr["V"], ldv, ptr["info"], ptr["work"], stream) == 0
    return Job(host, enqueue, scratch=("work",), label="dcholupdate n=%d k=%d sign=%+d" % (n, k, sign))


@pytest.mark.parametrize("n,k,sign", [(300, 17, 1), (300, 16, -1), (1000, 1, 1)])
def test_cholupdate_ordered(env, n, k, sign):
    def sane(ref, _):
        assert ref["info"][0] == 0 and ref["info"][1] == -9 and np.isfinite(ref["R"].reshape(n, n + 1)[:, :n][np.tril_indices(n)]).all()
    _against_plain(env, lambda: (_cholupdate_job(n, k, sign), lambda: None), "dcholupdate n=%d k=%d sign=%+d" % (n, k, sign), sane=sane)


def _spd_solved(n, nrhs):
    A = cm.spd(n, 40 + n)
    R = np.linalg.cholesky(A).T
    B = np.random.default_rng(n).standard_normal((n, nrhs))
    X = np.linalg.solve(A, B)
    a_up = A.copy()
    a_up[np.tril_indices(n, -1)] = NAN
    return A, a_up, R, B, X


@pytest.mark.parametrize("n", (300, 1000))
def test_pocon_ordered(env, n):
    L = _L()
    A, _, R, _, _ = _spd_solved(n, 1)
    ld = n + 1

    def make():
        host = {"R": B3.place(TR.stored(R), ld), "anorm": np.array([np.abs(A).sum(0).max(), NAN]), "rcond": np.full(3, -5.0), "work": _nan(max(L.cap_dpocon_work_size(n), 2))}

        def enqueue(ptr, stream):
            assert L.cap_dpocon(UPPER, n, ptr["R"], ld, ptr["anorm"], ptr["rcond"] + 8, ptr["work"], stream) == 0
        return Job(host, enqueue, scratch=("work",), label="dpocon n=%d" % n), lambda: None

    def sane(ref, _):
        assert ref["rcond"][0] == -5.0 and ref["rcond"][2] == -5.0 and 0.0 < ref["rcond"][1] <= 1.0
    _against_plain(env, make, "dpocon n=%d" % n, sane=sane)


@pytest.mark.parametrize("n,nrhs", [(300, 1), (300, 17)])
def test_poerr_ordered(env, n, nrhs):
    L = _L()
    A, a_up, R, B, X = _spd_solved(n, nrhs)
    lda, ldr, ldb, ldx = n + 2, n + 1, n + 3, n

    def make():
        host = {"A": B3.place(a_up, lda), "R": B3.place(TR.stored(R), ldr), "B": B3.place(B, ldb), "X": B3.place(X, ldx), "ferr": _nan(nrhs + 1),
                "berr": _nan(nrhs + 1), "work": _nan(max(L.cap_dpoerr_work_size(n, nrhs), 2))}

        def enqueue(ptr, stream):
            assert L.cap_dpoerr(UPPER, n, nrhs, ptr["A"], lda, ptr["R"], ldr, ptr["B"], ldb, ptr["X"], ldx, ptr["ferr"], ptr["berr"], ptr["work"], stream) == 0
        return Job(host, enqueue, scratch=("work",), label="dpoerr n=%d nrhs=%d" % (n, nrhs)), lambda: None

    def sane(ref, _):
        for k in ("ferr", "berr"):
            assert np.isfinite(ref[k][:nrhs]).all() and (ref[k][:nrhs] >= 0).all() and np.isnan(ref[k][nrhs])
    _against_plain(env, make, "dpoerr n=%d nrhs=%d" % (n, nrhs), sane=sane)


_MP = {}


def _mp_operands(n, nrhs=8):
    if n not in _MP:
        g = np.random.default_rng(n)
        G = g.random((n, n)) * 2 - 1
        A = G @ G.T / n + np.eye(n)
        A = (A + A.T) / 2
        B = g.standard_normal((n, nrhs))
        _MP[n] = (A, B)
    return _MP[n]


def _mpchol_job(env, n, solve):
    """cap_mpchol_factor (split schedule, strips of two panels: the defaults) and the fp32 factor it leaves in the plan; with `solve` the
    refinement on top of it, which synchronises the stream once per sweep by contract"""
    import torch
    L = _L()
    A, B = _mp_operands(n)
    nrhs = B.shape[1]
    plan = C.c_void_p()
    assert L.cap_mpchol_plan_create(C.byref(plan), n, nrhs) == 0
    host = {"A": A.ravel().copy(), "B": B3.place(B, n), "X": _nan(n * nrhs)}

    def enqueue(ptr, stream):
        assert L.cap_mpchol_factor(plan, ptr["A"], n, stream) == 0
        ld = C.c_int64(0)
        r32 = L.cap_mpchol_R32_ptr(plan, C.byref(ld))
        assert r32 and ld.value >= n
        out = {"R32": torch.empty(n * ld.value, dtype=torch.float32, device=SO.DEV)}
        env.copy_raw(out["R32"], r32, stream)
        if solve:
            it, rr = C.c_int(0), C.c_double(0)
            assert L.cap_mpchol_solve(plan, ptr["A"], n, ptr["B"], n, ptr["X"], n, nrhs, 5, 1e-14, C.byref(it), C.byref(rr), stream) == 0
            assert rr.value < 1e-12          # (the norm behind relres is summed with floating-point atomics: not reproducible bit for bit)
            out["iters"] = it.value
            info = C.c_int64(-1)             # (cap_mpchol_info synchronises the stream as well)
            assert L.cap_mpchol_info(plan, stream, C.byref(info)) == 0
            out["info"] = info.value
        return out
    return Job(host, enqueue, label="mpchol n=%d%s" % (n, " + solve" if solve else "")), lambda: L.cap_mpchol_plan_destroy(plan)


@pytest.mark.parametrize("n", (2048, 3072))
def test_mpchol_factor_ordered(env, n):
    def sane(ref, rret):
        r = rret["R32"]
        assert np.isfinite(r).any() and np.isnan(ref["X"]).all()
    _against_plain(env, lambda: _mpchol_job(env, n, False), "mpchol_factor n=%d" % n, sane=sane)


@pytest.mark.parametrize("n", (2048, 3072))
def test_mpchol_factor_and_solve_ordered(env, n):
    """cap_mpchol_solve is documented as host-synchronising (one synchronisation per sweep): exempt from the timing premise, still ordered
    behind the delayed inputs and in front of the snapshots"""
    def sane(ref, rret):
        A, B = _mp_operands(n)
        x = ref["X"].reshape(B.shape[1], n).T
        assert rret["iters"] >= 1 and rret["info"] == 0 and np.linalg.norm(B - A @ x) / np.linalg.norm(B) < 1e-12
    _against_plain(env, lambda: _mpchol_job(env, n, True), "mpchol_factor + solve n=%d" % n, exempt=True, sane=sane)


def _cacqr_job(env, m, n, num_iter, nrhs=5):
    import torch
    L = _L()
    g = np.random.default_rng(m + n)
    A, B = g.standard_normal((m, n)), g.standard_normal((m, nrhs))
    plan = C.c_void_p()
    assert L.cap_cacqr_plan_create(C.byref(plan), m, n, num_iter, None) == 0
    lda = m + 2 if m % 2 == 0 else m
    host = {"A": B3.place(A, lda), "B": B3.place(B, m), "X": _nan((n + 1) * nrhs), "Z": _nan(n * nrhs)}

    def enqueue(ptr, stream):
        assert L.cap_cacqr_factor(plan, ptr["A"], lda, stream) == 0
        assert L.cap_cacqr_solve(plan, ptr["B"], m, nrhs, ptr["X"], n + 1, stream) == 0
        assert L.cap_cacqr_apply_qt(plan, ptr["B"], m, nrhs, ptr["Z"], n, stream) == 0
        out = {}
        for name, get, cols in (("Q", L.cap_cacqr_Q_ptr, n), ("R", L.cap_cacqr_R_ptr, n)):
            ld = C.c_int64(0)
            p = get(plan, C.byref(ld))
            assert p and ld.value > 0
            out[name] = torch.empty(cols * ld.value, dtype=torch.float64, device=SO.DEV)
            env.copy_raw(out[name], p, stream)
        return out
    return Job(host, enqueue, label="cacqr %dx%d iter=%d" % (m, n, num_iter)), lambda: L.cap_cacqr_plan_destroy(plan)


@pytest.mark.parametrize("m,n,num_iter", [(1024, 256, 3), (5000, 37, 3), (1024, 256, 2), (5000, 37, 4)])
def test_cacqr_factor_solve_apply_qt_ordered(env, m, n, num_iter):
    def sane(ref, rret):
        assert np.isfinite(ref["Z"]).all() and np.isfinite(ref["X"].reshape(-1, n + 1)[:, :n]).all() and np.isnan(ref["X"].reshape(-1, n + 1)[:, n]).all()
    _against_plain(env, lambda: _cacqr_job(env, m, n, num_iter), "cacqr factor + solve + apply_qt %dx%d iter=%d" % (m, n, num_iter),
                   delay_ms=SEQUENCE_DELAY_MS, sane=sane)


# ============================================================================================================================ two callers at once
def test_two_split_k_products_at_once(env):
    """gemm.hip keeps its split-K slabs per (device, stream): two products in flight on two streams must not share them"""
    c = _row(B3.CASES, "gemm-TN-256x256x5008")
    (ja, wa), (jb, wb) = _blas3_job(c, 501), _blas3_job(c, 502, ab=1)
    with env.ordered([ja, jb], label="2 x split-K dgemm") as (a, b):
        _check(a, wa)
        _check(b, wb)


def test_two_one_launch_potrs_at_once(env):
    """the substitutions claim tickets from counters in `work` and report give-ups in words the process keeps per device"""
    ca = next(c for c in TR.POTRS_CASES if c.n == 1153 and c.other == 5)
    cb = next(c for c in TR.POTRS_CASES if c.n == 1000 and c.other <= 16)
    (ja, wa, oa), (jb, wb, ob) = _tri_job(ca), _tri_job(cb)
    with env.ordered([ja, jb], label="2 x one-launch dpotrs") as (a, b):
        _check(a, wa, zero_fix=(oa,))
        _check(b, wb, zero_fix=(ob,))


def test_two_cholupdates_at_once_give_their_solo_bits(env):
    ja, jb = _cholupdate_job(1000, 17, 1), _cholupdate_job(640, 16, -1, seed=1)
    (ra, _), (rb, _) = env.plain(ja), env.plain(jb)
    assert ra["info"][0] == 0 and rb["info"][0] == 0
    with env.ordered([ja, jb], label="2 x dcholupdate") as (a, b):
        _check(a, ra)
        _check(b, rb)


def test_two_blocked_batched_factors_at_once(env):
    (ja, wa), (jb, wb) = _batched_job(129, 37, 17), _batched_job(193, 20, 3, seed_shift=5)
    for j, w in ((ja, wa), (jb, wb)):
        w["logdet"] = env.plain(j)[0]["logdet"]
    with env.ordered([ja, jb], label="2 x dpotrf_batched_blocked + solve") as (a, b):
        _check(a, wa)
        _check(b, wb)


def test_two_cholinv_plans_factor_at_once(env):
    L = _L()
    rows = _chol_rows()
    ca, cb = rows[3], rows[4]                                   # the paired far update beside the overlapped inverse tree
    pa, pb = CH.create_plan(L, ca), CH.create_plan(L, cb)
    try:
        (ja, wa), (jb, wb) = _plan_factor_job(ca, pa), _plan_factor_job(cb, pb)
        with env.ordered([ja, jb], label="2 cholinv plans") as (a, b):
            _check(a, wa, zero_fix=tuple(wa))
            _check(b, wb, zero_fix=tuple(wb))
        assert CH.plan_info(L, pa, None) == 0 and CH.plan_info(L, pb, None) == 0
    finally:
        assert L.cap_cholinv_plan_destroy(pa) == 0 and L.cap_cholinv_plan_destroy(pb) == 0
