"""CPU-only: argument handling of the batched symmetric products and diagnostics (cap_dsymm_batched, cap_dlansy_batched, cap_dpocon_batched,
cap_dpoerr_batched and their _vbatched forms, csrc/symm_batched.hip) - the argument rules of include/capital_amd.h in their order, every
case decided before the library touches a device - the header / ctypes agreement, the Python names and refusals, and the compiler's resource
remarks of every new kernel instance.  The last test drives the entries through the recording stand-in of tests/hipshim in a process of
its own (this file run as a script): the launch counts the header states (symm, lansy: 1, on a plan 1 per occurring class; pocon: 4, on a
plan 3 per class + 1; poerr: 1 for berr alone and 4 with ferr, on a plan per class), every launch annotated, no finding, nothing for an
empty call."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, HIP, UNSUPPORTED = 0, 1, 2, 4
ONE = ord('1')
TRACE_N = (8, 64, 65, 256)
TRACE_NRHS = (1, 17)
TRACE_LISTS = ("EVERY", "WAVES", "ONE_CLASS", "LONE1")
NAMES = ("cap_dsymm_batched", "cap_dsymm_vbatched", "cap_dlansy_batched", "cap_dlansy_vbatched", "cap_dpocon_batched", "cap_dpocon_vbatched",
         "cap_dpoerr_batched", "cap_dpoerr_vbatched")
SIZES = ("cap_dpocon_batched_work_size", "cap_dpocon_vbatched_work_size", "cap_dpoerr_batched_work_size", "cap_dpoerr_vbatched_work_size")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


A_ = C.c_void_p(1 << 20)                 # never dereferenced: every call below returns before any device work
X_ = C.c_void_p(1 << 24)
B_ = C.c_void_p(1 << 28)
Y_ = C.c_void_p(1 << 32)
R_ = C.c_void_p(1 << 36)
O_ = C.c_void_p(1 << 40)
W_ = C.c_void_p(1 << 44)


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*a)


def test_symm_arguments_are_checked_in_the_documented_order(L):
    def call(uplo=UPPER, absolute=0, n=10, nrhs=3, alpha=1.0, A=A_, lda=10, stride_a=100, X=X_, ldx=10, stride_x=30, beta=1.0, B=B_, ldb=10,
             stride_b=30, Y=Y_, ldy=10, stride_y=30, batch=5):
        return L.cap_dsymm_batched(uplo, absolute, n, nrhs, alpha, A, lda, stride_a, X, ldx, stride_x, beta, B, ldb, stride_b, Y, ldy, stride_y,
                                   batch, None)
    big = dict(n=257, lda=257, ldx=257, ldb=257, ldy=257, stride_a=257 * 257, stride_x=257 * 3, stride_b=257 * 3, stride_y=257 * 3)
    # 1. absolute, negative sizes
    for ab in (2, -1):
        assert call(absolute=ab, batch=0) == ARG and call(absolute=ab, uplo=LOWER, n=0) == ARG and call(absolute=ab, **big) == ARG
    assert call(n=-1, batch=0) == ARG and call(nrhs=-1, uplo=LOWER) == ARG and call(batch=-1) == ARG
    # 2. NULL pointers when something would be computed
    assert call(Y=None, uplo=LOWER) == ARG and call(A=None, uplo=LOWER) == ARG and call(X=None, uplo=LOWER) == ARG and call(B=None, uplo=LOWER) == ARG
    assert call(A=None, X=None, alpha=0.0, uplo=LOWER) == UNSUPPORTED and call(B=None, beta=0.0, uplo=LOWER) == UNSUPPORTED
    assert call(Y=None, A=None, X=None, B=None, batch=0) == OK and call(Y=None, nrhs=0) == OK and call(Y=None, n=0, A=None) == OK
    # 3. leading dimensions and strides
    for kw in (dict(lda=9), dict(ldx=9), dict(ldy=9), dict(ldb=9), dict(stride_a=99), dict(stride_x=29), dict(stride_y=29), dict(stride_b=29),
               dict(stride_a=-1), dict(lda=12, stride_a=119), dict(ldx=12, stride_x=35)):
        assert call(uplo=LOWER, **kw) == ARG and call(**dict(big, **kw)) == ARG, kw
    assert call(ldb=9, beta=0.0, uplo=LOWER) == UNSUPPORTED and call(stride_b=0, beta=0.0, B=None, uplo=LOWER) == UNSUPPORTED
    assert call(stride_a=0, stride_x=0, stride_b=0, stride_y=0, batch=1, uplo=LOWER) == UNSUPPORTED     # one block needs no stride
    assert call(lda=1 << 40, stride_a=1 << 62, n=1 << 30, ldx=1 << 30, ldb=1 << 30, ldy=1 << 30) == ARG       # the clipped product
    # 4. Y overlaps A or X (Y = B is allowed)
    assert call(Y=A_, uplo=LOWER) == ARG and call(Y=X_, uplo=LOWER) == ARG and call(Y=C.c_void_p((1 << 24) + 8 * 149), uplo=LOWER) == ARG
    assert call(Y=C.c_void_p((1 << 24) + 8 * 150), uplo=LOWER) == UNSUPPORTED and call(Y=B_, uplo=LOWER) == UNSUPPORTED
    assert call(Y=A_, alpha=0.0, uplo=LOWER) == UNSUPPORTED                                               # A is not addressed
    # 5. LOWER, 6. n > 256, 7. the grid, 8. nothing to do
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7, n=0) == UNSUPPORTED and call(uplo=LOWER, batch=0) == UNSUPPORTED
    assert call(**big) == UNSUPPORTED and call(batch=0, **big) == UNSUPPORTED and call(uplo=LOWER, **big) == UNSUPPORTED
    g65 = dict(n=65, lda=65, ldx=65, ldb=65, ldy=65, stride_a=65 * 65, stride_x=65 * 3, stride_b=65 * 3, stride_y=65 * 3)
    assert call(batch=1 << 31, Y=C.c_void_p(1 << 60), **g65) == UNSUPPORTED
    assert call(n=0) == OK and call(nrhs=0) == OK and call(batch=0) == OK
    for sz in (64, 65, 256):
        kw = dict(n=sz, lda=sz, ldx=sz, ldb=sz, ldy=sz, stride_a=sz * sz, stride_x=sz * 3, stride_b=sz * 3, stride_y=sz * 3)
        assert call(batch=0, **kw) == OK and call(nrhs=0, stride_x=0, stride_b=0, stride_y=0, **{k: v for k, v in kw.items() if not k.startswith("stride_")
                                                                                           or k == "stride_a"}) == OK
        assert call(**dict(kw, lda=sz - 1)) == ARG and call(uplo=LOWER, **kw) == UNSUPPORTED


def test_lansy_pocon_poerr_arguments_are_checked_in_the_documented_order(L):
    def lansy(norm=ONE, uplo=UPPER, n=10, A=A_, lda=10, stride_a=100, batch=5, out=O_):
        return L.cap_dlansy_batched(norm, uplo, n, A, lda, stride_a, batch, out, None)
    assert lansy(n=-1, norm=ord('F')) == ARG and lansy(batch=-1, uplo=LOWER) == ARG
    assert lansy(A=None, uplo=LOWER) == ARG and lansy(out=None, norm=ord('F')) == ARG and lansy(lda=9, uplo=LOWER) == ARG and lansy(stride_a=99, n=10) == ARG
    assert lansy(norm=ord('F')) == UNSUPPORTED and lansy(norm=ord('M'), batch=0) == UNSUPPORTED and lansy(uplo=LOWER) == UNSUPPORTED
    for nm in "1OoIi":
        assert lansy(norm=ord(nm), batch=0) == OK and lansy(norm=ord(nm), n=0, A=None, out=None) == OK
    assert lansy(n=257, lda=257, stride_a=257 * 257) == UNSUPPORTED and lansy(n=257, lda=256) == ARG
    assert lansy(n=65, lda=65, stride_a=65 * 65, batch=1 << 31) == UNSUPPORTED

    def pocon(uplo=UPPER, n=10, R=R_, ldr=10, stride_r=100, batch=5, anorm=A_, info=None, rcond=O_, work=W_):
        return L.cap_dpocon_batched(uplo, n, R, ldr, stride_r, batch, anorm, info, rcond, work, None)
    assert pocon(n=-1, uplo=LOWER) == ARG and pocon(batch=-1) == ARG
    for kw in (dict(R=None), dict(anorm=None), dict(rcond=None), dict(work=None), dict(ldr=9), dict(stride_r=99)):
        assert pocon(uplo=LOWER, **kw) == ARG, kw
    assert pocon(uplo=LOWER) == UNSUPPORTED and pocon(n=257, ldr=257, stride_r=257 * 257) == UNSUPPORTED
    assert pocon(n=0, R=None, anorm=None, rcond=None, work=None) == OK and pocon(batch=0, R=None, work=None) == OK
    assert L.cap_dpocon_batched_work_size(10, 5) == 500 and L.cap_dpocon_batched_work_size(0, 5) == 0 and L.cap_dpocon_batched_work_size(256, 0) == 0

    def poerr(uplo=UPPER, n=10, nrhs=3, A=A_, lda=10, stride_a=100, R=R_, ldr=10, stride_r=100, B=B_, ldb=10, stride_b=30, X=X_, ldx=10, stride_x=30,
              batch=5, info=None, ferr=O_, berr=Y_, lde=3, work=W_):
        return L.cap_dpoerr_batched(uplo, n, nrhs, A, lda, stride_a, R, ldr, stride_r, B, ldb, stride_b, X, ldx, stride_x, batch, info, ferr, berr, lde,
                                    work, None)
    assert poerr(n=-1, uplo=LOWER) == ARG and poerr(nrhs=-1) == ARG and poerr(batch=-1) == ARG
    for kw in (dict(A=None), dict(B=None), dict(X=None), dict(R=None), dict(work=None), dict(lda=9), dict(ldr=9), dict(ldb=9), dict(ldx=9),
               dict(stride_a=99), dict(stride_r=99), dict(stride_b=29), dict(stride_x=29), dict(lde=2)):
        assert poerr(uplo=LOWER, **kw) == ARG, kw
    for kw in (dict(R=None), dict(work=None), dict(ldr=9), dict(stride_r=99)):                           # berr alone needs no factor and no work
        assert poerr(uplo=LOWER, ferr=None, **kw) == UNSUPPORTED, kw
    assert poerr(ferr=None, berr=None, A=None, B=None, X=None, lde=0) == OK and poerr(ferr=None, berr=None, uplo=LOWER) == UNSUPPORTED
    assert poerr(uplo=LOWER) == UNSUPPORTED and poerr(n=257, lda=257, ldr=257, ldb=257, ldx=257, stride_a=1 << 20, stride_r=1 << 20, stride_b=1 << 20,
                                                      stride_x=1 << 20) == UNSUPPORTED
    assert poerr(n=0, A=None, R=None, B=None, X=None, work=None) == OK and poerr(nrhs=0, lde=0, A=None) == OK and poerr(batch=0, A=None) == OK
    n, nrhs, batch = 10, 3, 5
    assert L.cap_dpoerr_batched_work_size(n, nrhs, batch) == batch * n * (n + nrhs) <= batch * n * (n + 2 * nrhs)
    assert L.cap_dpoerr_batched_work_size(0, 3, 5) == 0 and L.cap_dpoerr_batched_work_size(10, 0, 5) == 0


def create(L, n):
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(len(n), arr(n), None, None, C.byref(p)) == OK
    return p


def test_plan_entry_arguments_are_checked_in_the_documented_order(L):
    """no call here reaches a launch: in a process without a device the accepted calls on a non-empty plan end in CAP_ERR_HIP"""
    p, p0, p1 = create(L, [5, 0, 100]), create(L, [0, 0, 0]), create(L, [])
    big = 1 << 20

    def symm(p=p, uplo=UPPER, absolute=0, nrhs=3, alpha=1.0, A=A_, X=X_, ldx=big, beta=1.0, B=B_, ldb=big, Y=Y_, ldy=big):
        return L.cap_dsymm_vbatched(p, uplo, absolute, nrhs, alpha, A, X, ldx, beta, B, ldb, Y, ldy, None)
    assert symm(p=None, uplo=LOWER) == ARG and symm(absolute=2, uplo=LOWER) == ARG and symm(nrhs=-1, p=p0) == ARG
    for kw in (dict(Y=None), dict(A=None), dict(X=None), dict(B=None), dict(ldx=104), dict(ldy=104), dict(ldb=104), dict(Y=A_), dict(Y=X_)):
        assert symm(uplo=LOWER, **kw) == ARG, kw                         # sum n_i = 105
    assert symm(ldx=105, ldy=105, ldb=105, uplo=LOWER) == UNSUPPORTED and symm(ldb=104, beta=0.0, B=None, uplo=LOWER) == UNSUPPORTED
    assert symm(A=None, X=None, alpha=0.0, uplo=LOWER) == UNSUPPORTED and symm(Y=B_, uplo=LOWER) == UNSUPPORTED
    for q in (p0, p1):
        assert symm(p=q, A=None, X=None, B=None, Y=None) == OK and symm(p=q, uplo=LOWER) == UNSUPPORTED and symm(p=q, ldx=-1) == ARG
    assert symm(nrhs=0, Y=None) == OK

    def lansy(p=p, norm=ONE, uplo=UPPER, A=A_, out=O_):
        return L.cap_dlansy_vbatched(p, norm, uplo, A, out, None)
    assert lansy(p=None, norm=ord('F')) == ARG and lansy(A=None, uplo=LOWER) == ARG and lansy(out=None, norm=ord('F')) == ARG
    assert lansy(norm=ord('F')) == UNSUPPORTED and lansy(uplo=LOWER) == UNSUPPORTED
    assert lansy(p=p0, A=None, out=None) == OK and lansy(p=p1, uplo=LOWER) == UNSUPPORTED

    def pocon(p=p, uplo=UPPER, R=R_, anorm=A_, info=None, rcond=O_, work=W_):
        return L.cap_dpocon_vbatched(p, uplo, R, anorm, info, rcond, work, None)
    assert pocon(p=None, uplo=LOWER) == ARG
    for kw in (dict(R=None), dict(anorm=None), dict(rcond=None), dict(work=None)):
        assert pocon(uplo=LOWER, **kw) == ARG, kw
    assert pocon(uplo=LOWER) == UNSUPPORTED and pocon(p=p0, R=None, anorm=None, rcond=None, work=None) == OK

    def poerr(p=p, uplo=UPPER, nrhs=3, A=A_, R=R_, B=B_, ldb=big, X=X_, ldx=big, info=None, ferr=O_, berr=Y_, lde=3, work=W_):
        return L.cap_dpoerr_vbatched(p, uplo, nrhs, A, R, B, ldb, X, ldx, info, ferr, berr, lde, work, None)
    assert poerr(p=None, uplo=LOWER) == ARG and poerr(nrhs=-1, uplo=LOWER) == ARG
    for kw in (dict(A=None), dict(B=None), dict(X=None), dict(R=None), dict(work=None), dict(ldb=104), dict(ldx=104), dict(lde=2)):
        assert poerr(uplo=LOWER, **kw) == ARG, kw
    assert poerr(uplo=LOWER, ferr=None, R=None, work=None) == UNSUPPORTED and poerr(uplo=LOWER) == UNSUPPORTED
    assert poerr(p=p0, A=None, R=None, B=None, X=None, work=None) == OK and poerr(nrhs=0, lde=0) == OK and poerr(ferr=None, berr=None) == OK
    assert L.cap_dpocon_vbatched_work_size(p) == L.cap_vbatch_plan_info(p, 1) and L.cap_dpocon_vbatched_work_size(None) == -1
    assert L.cap_dpoerr_vbatched_work_size(p, 3) == L.cap_vbatch_plan_info(p, 1) + 105 * 3 and L.cap_dpoerr_vbatched_work_size(p, -1) == -1
    import torch
    if not torch.cuda.is_available():
        assert symm() == HIP and lansy() == HIP and pocon() == HIP and poerr() == HIP and poerr(ferr=None) == HIP   # a plan made without a device
    for q in (p, p0, p1):
        L.cap_vbatch_plan_destroy(q)


def test_header_declares_the_symbols_with_the_ctypes_signatures(L):
    from capital_amd import _lib
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in NAMES + SIZES:
        m = re.search(r"^(int|int64_t) %s\(([^;]*)\);" % name, header, re.M)
        assert m, name + " is not declared"
        want = []
        for a in m.group(2).replace("\n", " ").split(","):
            a = a.strip()
            want.append(C.c_void_p if "*" in a else kinds[a.replace("const ", "").split()[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)] and list(args) == want, (name, args, want)
        assert getattr(L, name).argtypes == want
    section = header[header.index("csrc/symm_batched.hip"):]
    for s in ("THE BIT CONTRACTS", "PLAN = FIXED", "LAYOUT INDEPENDENCE", "COLUMN INDEPENDENCE", "COMPOSITION", "fma(beta, b, t)",
              "Argument rules, in this order", "FOUR launches", "THREE per class plus ONE", "n (n + nrhs) batch"):
        assert s in section, s
    assert header.index("csrc/syrk_batched.hip") < header.index("csrc/symm_batched.hip")
    with open(os.path.join(ROOT, "capital_amd", "csrc", "symm_batched.hip")) as f:
        head = f.read().split("#include", 1)[0]
    for s in ("THE ARITHMETIC", "THE BIT CONTRACTS", "fma(beta, b, t)", "THE FUSED MODES", "safe1"):
        assert s in head, s


def test_python_layer_names_and_refusals():
    import torch
    from capital_amd import _lib, batched, blas, lapack
    for fn in (blas.engine._symm_batched, blas.engine._symm_vbatched, lapack.engine._lansy_batched, lapack.engine._lansy_vbatched,
               lapack.engine._pocon_batched, lapack.engine._pocon_vbatched, lapack.engine._poerr_batched, lapack.engine._poerr_vbatched):
        assert callable(fn) and "256" in fn.__doc__
    for fn in (batched.symm, batched.norm1, batched.rcond, batched.error_bounds, batched.VarBatch.symm, batched.VarBatch.norm1,
               batched.VarBatch.rcond, batched.VarBatch.error_bounds):
        assert callable(fn) and "LOWER" in fn.__doc__
    for fn in (batched.norm1, batched.error_bounds, batched.VarBatch.norm1, batched.VarBatch.error_bounds):
        assert "BEFORE" in fn.__doc__
    assert len({int(m) for m in lapack.Method}) == len(list(lapack.Method)) and len({int(m) for m in blas.Method}) == len(list(blas.Method))
    row = blas.ArgPack_symm(blas.Order.AblasRowMajor, blas.UpLo.AblasUpper, 1.0, 0.0)
    with pytest.raises(_lib.CapitalError, match="AblasColumnMajor"):
        blas.engine._symm_batched(None, None, None, None, 4, 1, 4, 16, 4, 4, 4, 4, 4, 4, 1, row)
    col = blas.ArgPack_symm(blas.Order.AblasColumnMajor, blas.UpLo.AblasUpper, 1.0, 0.0, absolute=True)
    with pytest.raises(_lib.CapitalError, match="256"):
        blas.engine._symm_batched(None, None, None, None, 257, 1, 257, 257 * 257, 257, 257, 257, 257, 257, 257, 1, col)
    rowl = lapack.ArgPack_lansy_batched(lapack.Order.AlapackRowMajor, lapack.UpLo.AlapackUpper)
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        lapack.engine._lansy_batched(None, 4, 4, 16, 1, None, rowl)
    with pytest.raises(_lib.CapitalError, match="256"):
        lapack.engine._pocon_batched(None, 257, 257, 257 * 257, 1, None, None, None,
                                     lapack.ArgPack_pocon_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper))
    a = torch.zeros(3, 10, 10, dtype=torch.float64)
    x = torch.zeros(3, 2, 10, dtype=torch.float64)
    vb = batched.VarBatch([3, 5])
    with pytest.raises(_lib.CapitalError, match="^A must"):                   # the messages name the operand that is wrong
        batched.symm(a, x)
    with pytest.raises(_lib.CapitalError, match="^A must"):
        vb.symm(torch.zeros(34, dtype=torch.float64), torch.zeros(8, dtype=torch.float64))
    with pytest.raises(_lib.CapitalError, match="^R must"):
        batched.error_bounds(a, a, x, x)
    for bad in (lambda: batched.symm(a, x), lambda: batched.symm(None, None), lambda: batched.norm1(a), lambda: batched.norm1(a.to(torch.float32)),
                lambda: batched.rcond(a, torch.zeros(3, dtype=torch.float64)), lambda: batched.error_bounds(a, a, x, x),
                lambda: vb.symm(torch.zeros(34, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)), lambda: vb.norm1(None),
                lambda: vb.rcond(torch.zeros(34, dtype=torch.float64), None), lambda: vb.error_bounds(None, None, None, None)):
        with pytest.raises(_lib.CapitalError):
            bad()


def test_every_new_kernel_instance_keeps_its_accumulators_in_registers(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR - four modes x (4 NP + the workgroup kernel) x (fixed
    size, plan), the copy of the triangles (fixed size, plan) and the last step of rcond"""
    from capital_amd import build
    all_res = build.kernel_resources()
    res = {k: v for k, v in all_res.items() if re.search(r"\d+symm_v?batched(_blocked)?_kernelI", k)}
    assert len(res) == 4 * (4 + 1) * 2, sorted(res)
    res.update({k: v for k, v in all_res.items() if re.search(r"\d+symm_(copy_upper|rcond)_kernel", k)})
    assert len(res) == 4 * (4 + 1) * 2 + 3, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
    for name in ("symm_batched_kernel", "symm_vbatched_kernel", "symm_batched_blocked_kernel", "symm_vbatched_blocked_kernel",
                 "symm_copy_upper_kernel", "symm_rcond_kernel"):
        assert name in build.NO_SCRATCH


def test_the_stated_launch_counts_on_the_recording_stand_in(tmp_path):
    """the fixed-size entries at n = 8, 64, 65, 256 with nrhs = 1 and 17, the plan entries on four size lists; the caller on the NULL stream
    and on a stream of its own"""
    from capital_amd import build
    build.build(verbose=False)
    out = tmp_path / "trace.json"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    res = json.load(open(out))
    assert len(res) == 2 * (len(TRACE_N) + len(TRACE_LISTS))
    for x in res:
        assert not x["findings"], (x["name"], x["findings"][:4])
        assert x["stats"]["kernels"] == x["expected"] and not x["stats"].get("unannotated"), (x["name"], x["stats"], x["expected"])
        assert x["stats"]["oob"] == 0 and x["stats"].get("races", 0) == 0
        assert all(k.startswith("K ") and ("symm_" in k or "potri_" in k) for k in x["launches"]), x["launches"]
        for (name, lines), want in zip(x["per_call"], x["per_launches"]):
            assert len(lines) == want and all(l.startswith("K ") for l in lines), (x["name"], name, lines, want)   # launches and nothing else
        assert len(x["per_call"]) == len(x["per_launches"])
        assert x["empty_calls"] == []


def _marks(r):
    per, cur, empties = [], None, []
    for l in r.lines:                  # what the trace holds between the marks of one call
        if l.startswith("MARK begin "):
            cur = (l[len("MARK begin "):], [])
        elif l.startswith("MARK end "):
            (empties if cur[0].startswith("empty") else per).append(cur)
            cur = None
        elif cur is not None and not l.startswith(("ACC ", "A ")):
            cur[1].append(l)
    return per, [e for e in empties if e[1]]


def _trace_main(out_path):
    """runs in a process of its own (no torch: the stand-in takes the place of the HIP runtime)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipshim"))
    sys.path.insert(0, ROOT)
    import run_scenarios as S
    from tests import vbatched_cases as VC
    lib = S.L
    results = []
    for user_stream in (0, 1):
        tag = " [user stream]" if user_stream else " [NULL stream]"
        for n in TRACE_N:
            r = S.Run("symm batched n=%d%s" % (n, tag), user_stream)
            batch, lda, kmax = 37, n + 1, max(TRACE_NRHS)
            ldx = n + 2
            Ad, Rd = S.dmalloc(8 * (lda * n + 3) * batch), S.dmalloc(8 * (lda * n + 3) * batch)
            Xd, Bd, Yd = (S.dmalloc(8 * (ldx * kmax + 5) * batch) for _ in range(3))
            an, rc, fe, be, info = (S.dmalloc(8 * batch * (kmax + 1)) for _ in range(5))
            Wd = S.dmalloc(8 * lib.cap_dpoerr_batched_work_size(n, kmax, batch))
            want = []
            for k in TRACE_NRHS:
                sx = ldx * k + 5
                for absolute, alpha, beta, Bp, Yp in ((0, -1.0, 1.0, Bd, Yd), (1, 1.0, 0.0, None, Yd), (0, 2.0, 0.5, Bd, Bd), (0, 0.0, 1.0, Bd, Yd)):
                    S.ok(r.call("dsymm_batched nrhs=%d abs=%d beta=%g" % (k, absolute, beta), lib.cap_dsymm_batched, 1, absolute, n, k, alpha,
                                Ad if alpha else None, lda, lda * n + 3, Xd if alpha else None, ldx, sx, beta, Bp, ldx, sx, Yp, ldx, sx, batch,
                                r.stream), "cap_dsymm_batched")
                    want.append(1)
                S.ok(r.call("dpoerr_batched nrhs=%d" % k, lib.cap_dpoerr_batched, 1, n, k, Ad, lda, lda * n + 3, Rd, lda, lda * n + 3, Bd, ldx, sx, Xd,
                            ldx, sx, batch, info, fe, be, k + 1, Wd, r.stream), "cap_dpoerr_batched")
                S.ok(r.call("dpoerr_batched nrhs=%d berr alone" % k, lib.cap_dpoerr_batched, 1, n, k, Ad, lda, lda * n + 3, None, 0, 0, Bd, ldx, sx, Xd,
                            ldx, sx, batch, None, None, be, k, None, r.stream), "cap_dpoerr_batched")
                S.ok(r.call("dpoerr_batched nrhs=%d ferr alone" % k, lib.cap_dpoerr_batched, 1, n, k, Ad, lda, lda * n + 3, Rd, lda, lda * n + 3, Bd, ldx,
                            sx, Xd, ldx, sx, batch, None, fe, None, k, Wd, r.stream), "cap_dpoerr_batched")
                want += [4, 1, 4]
            S.ok(r.call("dsymm_batched one block", lib.cap_dsymm_batched, 1, 0, n, 3, 1.0, Ad, n, 0, Xd, n, 0, 0.0, None, n, 0, Yd, n, 0, 1, r.stream),
                 "cap_dsymm_batched")
            S.ok(r.call("dlansy_batched", lib.cap_dlansy_batched, ord('1'), 1, n, Ad, lda, lda * n + 3, batch, an, r.stream), "cap_dlansy_batched")
            S.ok(r.call("dpocon_batched", lib.cap_dpocon_batched, 1, n, Rd, lda, lda * n + 3, batch, an, info, rc, Wd, r.stream), "cap_dpocon_batched")
            S.ok(r.call("dpocon_batched no info", lib.cap_dpocon_batched, 1, n, Rd, n, n * n, 1, an, None, rc, Wd, r.stream), "cap_dpocon_batched")
            want += [1, 1, 4, 4]
            for c in (("empty symm batch=0", lib.cap_dsymm_batched, 1, 0, n, 1, 1.0, None, n, 0, None, n, 0, 0.0, None, n, 0, None, n, 0, 0),
                      ("empty symm nrhs=0", lib.cap_dsymm_batched, 1, 0, n, 0, 1.0, Ad, n, n * n, Xd, n, 0, 1.0, Bd, n, 0, Yd, n, 0, batch),
                      ("empty lansy n=0", lib.cap_dlansy_batched, ord('1'), 1, 0, None, 0, 0, batch, None),
                      ("empty pocon batch=0", lib.cap_dpocon_batched, 1, n, None, n, 0, 0, None, None, None, None),
                      ("empty poerr no output", lib.cap_dpoerr_batched, 1, n, 1, Ad, n, n * n, Rd, n, n * n, Bd, n, n, Xd, n, n, batch, None, None, None,
                       1, Wd),
                      ("empty poerr nrhs=0", lib.cap_dpoerr_batched, 1, n, 0, Ad, n, n * n, Rd, n, n * n, Bd, n, 0, Xd, n, 0, batch, None, fe, be, 0, Wd)):
                S.ok(r.call(c[0], c[1], *c[2:], r.stream), c[0])
            out = r.finish()
            out["expected"], out["per_launches"] = sum(want), want
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Ad, Rd, Xd, Bd, Yd, an, rc, fe, be, info, Wd):
                S.shim.hipFree(q)
            results.append(out)
        for name in TRACE_LISTS:
            lay = VC.Layout(VC.LISTS[name], "gaps")
            plan, empty = C.c_void_p(), C.c_void_p()
            S.ok(lib.cap_vbatch_plan_create(lay.batch, arr(list(lay.sizes)), None, arr(list(lay.off_arg)), C.byref(plan)), "cap_vbatch_plan_create")
            S.ok(lib.cap_vbatch_plan_create(3, arr([0, 0, 0]), None, None, C.byref(empty)), "cap_vbatch_plan_create")
            r = S.Run("symm vbatched %s%s" % (name, tag), user_stream)
            kmax = max(TRACE_NRHS)
            ld = lay.rows + 2
            Ad, Rd = S.dmalloc(8 * lay.total), S.dmalloc(8 * lay.total)
            Xd, Bd, Yd = (S.dmalloc(8 * ld * (kmax + 2)) for _ in range(3))
            an, rc, fe, be, info = (S.dmalloc(8 * lay.batch * (kmax + 1)) for _ in range(5))
            Wd = S.dmalloc(8 * lib.cap_dpoerr_vbatched_work_size(plan, kmax))
            classes = int(lib.cap_vbatch_plan_info(plan, 4))
            assert classes >= 1
            want = []
            for k in TRACE_NRHS:
                for absolute, alpha, beta, Bp, Yp in ((0, -1.0, 1.0, Bd, Yd), (1, 1.0, 0.0, None, Yd), (0, 2.0, 0.5, Bd, Bd)):
                    S.ok(r.call("dsymm_vbatched nrhs=%d abs=%d beta=%g" % (k, absolute, beta), lib.cap_dsymm_vbatched, plan, 1, absolute, k, alpha, Ad, Xd,
                                ld, beta, Bp, ld, Yp, ld, r.stream), "cap_dsymm_vbatched")
                    want.append(classes)
                S.ok(r.call("dpoerr_vbatched nrhs=%d" % k, lib.cap_dpoerr_vbatched, plan, 1, k, Ad, Rd, Bd, ld, Xd, ld, info, fe, be, k + 1, Wd,
                            r.stream), "cap_dpoerr_vbatched")
                S.ok(r.call("dpoerr_vbatched nrhs=%d berr alone" % k, lib.cap_dpoerr_vbatched, plan, 1, k, Ad, None, Bd, ld, Xd, ld, None, None, be, k,
                            None, r.stream), "cap_dpoerr_vbatched")
                want += [4 * classes, classes]
            S.ok(r.call("dlansy_vbatched", lib.cap_dlansy_vbatched, plan, ord('I'), 1, Ad, an, r.stream), "cap_dlansy_vbatched")
            S.ok(r.call("dpocon_vbatched", lib.cap_dpocon_vbatched, plan, 1, Rd, an, info, rc, Wd, r.stream), "cap_dpocon_vbatched")
            want += [classes, 3 * classes + 1]
            for c in (("empty plan symm", lib.cap_dsymm_vbatched, empty, 1, 0, 3, 1.0, None, None, 3, 0.0, None, 3, None, 3),
                      ("empty plan lansy", lib.cap_dlansy_vbatched, empty, ord('1'), 1, None, None),
                      ("empty plan pocon", lib.cap_dpocon_vbatched, empty, 1, None, None, None, None, None),
                      ("empty plan poerr", lib.cap_dpoerr_vbatched, empty, 1, 3, None, None, None, 3, None, 3, None, None, None, 3, None),
                      ("empty nrhs=0", lib.cap_dsymm_vbatched, plan, 1, 0, 0, 1.0, Ad, Xd, ld, 0.0, None, ld, Yd, ld)):
                S.ok(r.call(c[0], c[1], *c[2:], r.stream), c[0])
            out = r.finish()
            out["expected"], out["per_launches"] = sum(want), want
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Ad, Rd, Xd, Bd, Yd, an, rc, fe, be, info, Wd):
                S.shim.hipFree(q)
            S.ok(lib.cap_vbatch_plan_destroy(plan), "cap_vbatch_plan_destroy")
            S.ok(lib.cap_vbatch_plan_destroy(empty), "cap_vbatch_plan_destroy")
            results.append(out)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
