"""CPU-only: argument handling of the batched general products (cap_dgemm_batched, cap_dgemm_vbatched_inner, cap_dgemm_vbatched_combine) -
the argument rules of include/capital_amd.h in their order, every case decided before the library touches a device - the header / ctypes
agreement, the Python names and refusals, and the compiler's resource remarks of every new kernel instance.  The last test drives the
three entries through the recording stand-in of tests/hipshim in a process of its own (this file run as a script): one launch per
fixed-size call, ONE per `inner` call whatever the plan's classes, one per occurring class for `combine`, every launch annotated, no
finding, nothing for an empty call."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
NOTRANS, TRANS = 0, 1
OK, ARG, HIP, UNSUPPORTED = 0, 1, 2, 4
TRACE_MN = ((8, 5), (64, 64), (65, 3), (17, 130), (256, 256))
TRACE_K = (0, 1, 17)
TRACE_LISTS = ("EVERY", "WAVES", "ONE_CLASS", "LONE1")
NAMES = ("cap_dgemm_batched", "cap_dgemm_vbatched_inner", "cap_dgemm_vbatched_combine")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


A = C.c_void_p(1 << 20)                  # never dereferenced: every call below returns before any device work
B = C.c_void_p(1 << 24)
CC = C.c_void_p(1 << 28)


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*a)


def fixed(L):
    def call(ta=NOTRANS, tb=NOTRANS, m=10, n=7, k=3, alpha=1.0, A=A, lda=10, sa=30, B=B, ldb=3, sb=21, beta=0.0, C=CC, ldc=10, sc=70, batch=5):
        return L.cap_dgemm_batched(ta, tb, m, n, k, alpha, A, lda, sa, B, ldb, sb, beta, C, ldc, sc, batch, None)
    return call


def test_fixed_size_arguments_are_checked_in_the_documented_order(L):
    call = fixed(L)
    big = dict(m=257, lda=257, ldc=257, sa=257 * 3, sc=257 * 7)
    wide = dict(n=257, sb=3 * 257, sc=10 * 257)
    # 1. trans, negative sizes
    for t in (2, -1, 255):
        assert call(ta=t) == ARG and call(tb=t) == ARG and call(ta=t, **big) == ARG and call(tb=t, batch=0) == ARG and call(ta=t, m=0) == ARG
    assert call(m=-1) == ARG and call(n=-1) == ARG and call(k=-1) == ARG and call(batch=-1) == ARG and call(k=-1, batch=0) == ARG
    # NULL C, NULL A / B (only with m n k batch > 0 and alpha != 0)
    assert call(C=None) == ARG and call(C=None, k=0) == ARG and call(C=None, alpha=0.0) == ARG and call(C=None, **big) == ARG
    assert call(A=None) == ARG and call(B=None) == ARG and call(A=None, **big) == ARG
    assert call(A=None, B=None, batch=0) == OK and call(C=None, batch=0) == OK and call(C=None, m=0) == OK and call(C=None, n=0) == OK
    assert call(A=None, B=None, alpha=0.0, **big) == UNSUPPORTED and call(A=None, B=None, k=0, **big) == UNSUPPORTED
    # ldc, lda / ldb as stored, the strides
    assert call(ldc=9) == ARG and call(ldc=9, **wide) == ARG
    assert call(lda=9) == ARG and call(lda=9, alpha=0.0) == ARG and call(ldb=2) == ARG
    assert call(ta=TRANS, lda=2) == ARG and call(ta=TRANS, lda=3, sa=30, **wide) == UNSUPPORTED and call(ta=TRANS, lda=3, sa=29) == ARG
    assert call(tb=TRANS, ldb=6) == ARG and call(tb=TRANS, ldb=7, sb=21, **dict(big, sc=257 * 7)) == UNSUPPORTED and call(tb=TRANS, ldb=7, sb=20) == ARG
    assert call(sc=69) == ARG and call(sa=29) == ARG and call(sb=20) == ARG
    assert call(ldc=12, sc=12 * 7 - 1) == ARG and call(lda=12, sa=35) == ARG and call(ldb=5, sb=34) == ARG
    assert call(sc=-1) == ARG and call(sa=-1) == ARG and call(sb=-1) == ARG
    assert call(sb=0, batch=1, **dict(big, sa=0, sc=0)) == UNSUPPORTED                       # one block needs no stride ...
    assert call(sc=0, batch=2) == ARG and call(sa=0, batch=2) == ARG and call(sb=0, batch=2) == ARG      # ... two do
    assert call(m=16, n=16, ldc=1 << 60, sc=0, lda=16, sa=48, sb=48, batch=2) == ARG                     # 2^64 does not wrap to 0
    assert call(k=0, **dict(big, sa=0)) == UNSUPPORTED and call(k=0, sb=20, **big) == ARG    # A is stored as m x 0, B as 0 x n: n columns
    assert call(**dict(big, ldc=256)) == ARG and call(**dict(big, lda=256)) == ARG           # the argument rules come before the size limit
    # C overlaps A or B (with alpha != 0 and k > 0)
    near = C.c_void_p((1 << 20) + 8 * 100)
    assert call(C=near) == ARG and call(C=near, **dict(big, sa=257 * 3)) == ARG and call(C=A) == ARG and call(C=B) == ARG
    span = 4 * 257 * 3 + 2 * 257 + 257                                                       # elements the five blocks of A span (with big)
    assert call(C=C.c_void_p((1 << 20) + 8 * (span - 1)), **big) == ARG and call(C=C.c_void_p((1 << 20) + 8 * span), **big) == UNSUPPORTED
    assert call(C=A, alpha=0.0, **big) == UNSUPPORTED and call(C=A, k=0, **dict(big, sa=0)) == UNSUPPORTED
    # 2. m, n > 256, 3. the grid
    assert call(**big) == UNSUPPORTED and call(**wide) == UNSUPPORTED and call(batch=0, **big) == UNSUPPORTED
    g65 = dict(m=65, lda=65, ldc=65, sa=65 * 3, sc=65 * 7)
    far = dict(B=C.c_void_p(1 << 50), C=C.c_void_p(1 << 56))                                 # 2^31 blocks of one operand stay clear of the next
    assert call(batch=1 << 31, **g65, **far) == UNSUPPORTED and call(batch=1 << 31, **dict(g65, ldc=64), **far) == ARG
    assert call(batch=1 << 31, **g65) == ARG                                                 # ... where they do not, the overlap is refused first
    assert call(m=8, n=8, lda=8, ldc=8, sa=24, sb=24, sc=64, batch=1 << 34, **far) == UNSUPPORTED       # eight blocks per wavefront: 2^31 workgroups
    # 4. nothing to do: no launch, whatever the pointers
    assert call(m=0, A=None, B=None, C=None, lda=0, ldc=0, sa=0, sc=0) == OK
    assert call(n=0, A=None, B=None, C=None, sb=0, sc=0) == OK
    assert call(batch=0, A=None, B=None, C=None, sa=-5, sb=-5, sc=-5) == OK


def create(L, n):
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(len(n), arr(n), None, None, C.byref(p)) == OK
    return p


def test_plan_entry_arguments_are_checked_in_the_documented_order(L):
    """no call here reaches a launch: in a process without a device the accepted calls that would launch end in CAP_ERR_HIP"""
    import torch
    nodev = not torch.cuda.is_available()
    p, p0, p1 = create(L, [5, 0, 100]), create(L, [0, 0, 0]), create(L, [])                 # sum n_i = 105

    def inner(p=p, m=4, n=6, alpha=1.0, X=A, ldx=105, Y=B, ldy=105, beta=0.0, G=CC, ldg=4, sg=24):
        return L.cap_dgemm_vbatched_inner(p, m, n, alpha, X, ldx, Y, ldy, beta, G, ldg, sg, None)
    assert inner(p=None) == ARG and inner(p=None, m=300) == ARG
    assert inner(m=-1) == ARG and inner(n=-1) == ARG and inner(m=-1, p=p1) == ARG
    assert inner(G=None) == ARG and inner(X=None) == ARG and inner(Y=None) == ARG and inner(G=None, m=300, ldg=300, sg=1800) == ARG
    assert inner(G=None, p=p0) == ARG                                  # the empty blocks of `inner` are written: G is needed
    assert inner(ldx=104) == ARG and inner(ldy=104) == ARG and inner(ldx=104, m=300, ldg=300, sg=1800) == ARG
    assert inner(ldg=3) == ARG and inner(sg=23) == ARG and inner(ldg=5, sg=29) == ARG and inner(sg=-1) == ARG
    assert inner(sg=0, p=p1) == OK and inner(ldx=-1, p=p1) == ARG
    assert inner(m=257, ldg=257, sg=257 * 6) == UNSUPPORTED and inner(n=257, sg=4 * 257) == UNSUPPORTED and inner(m=257, ldg=256, sg=257 * 6) == ARG
    assert inner(m=257, ldg=257, sg=257 * 6, p=p1) == UNSUPPORTED
    assert inner(m=0, G=None, X=None, Y=None, ldg=0, sg=0) == OK and inner(n=0, G=None, sg=0) == OK
    assert inner(p=p1, G=None, X=None, Y=None) == OK
    if nodev:
        assert inner() == HIP and inner(alpha=0.0, X=None, Y=None) == HIP and inner(p=p0, X=None, Y=None, ldx=0, ldy=0) == HIP

    def combine(p=p, nrhs=6, k=3, alpha=1.0, V=A, ldv=105, Z=B, ldz=3, sz=18, beta=0.0, Cp=CC, ldc=105):
        return L.cap_dgemm_vbatched_combine(p, nrhs, k, alpha, V, ldv, Z, ldz, sz, beta, Cp, ldc, None)
    assert combine(p=None) == ARG and combine(p=None, nrhs=300) == ARG
    assert combine(nrhs=-1) == ARG and combine(k=-1) == ARG and combine(k=-1, p=p0) == ARG
    assert combine(Cp=None) == ARG and combine(V=None) == ARG and combine(Z=None) == ARG and combine(Cp=None, nrhs=300, sz=900) == ARG
    assert combine(ldv=104) == ARG and combine(ldc=104) == ARG and combine(ldv=104, nrhs=300, sz=900) == ARG
    assert combine(ldz=2) == ARG and combine(sz=17) == ARG and combine(ldz=4, sz=23) == ARG and combine(sz=-1) == ARG
    assert combine(nrhs=257, sz=3 * 257) == UNSUPPORTED and combine(nrhs=257, sz=3 * 257, p=p0) == UNSUPPORTED
    for q in (p0, p1):                                                 # nothing to launch: pointers may be NULL
        assert combine(p=q, V=None, Z=None, Cp=None, ldv=0, ldc=0) == OK and combine(p=q, ldv=-1) == ARG
    assert combine(nrhs=0, Cp=None, V=None, Z=None, sz=0) == OK
    if nodev:
        assert combine() == HIP and combine(k=0, V=None, Z=None) == HIP and combine(alpha=0.0, V=None, Z=None) == HIP
    for q in (p, p0, p1):
        L.cap_vbatch_plan_destroy(q)


def test_header_declares_the_symbols_with_the_ctypes_signatures(L):
    from capital_amd import _lib
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in NAMES:
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name + " is not declared"
        want = []
        for a in m.group(1).replace("\n", " ").split(","):
            a = a.strip()
            want.append(C.c_void_p if "*" in a else kinds[a.replace("const ", "").split()[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and list(args) == want, (name, args, want)
        assert getattr(L, name).argtypes == want
    section = header[header.index("csrc/gemm_batched.hip"):]
    for s in ("THE BIT CONTRACTS", "PLAN = FIXED", "LAYOUT INDEPENDENCE", "TRANS IS A LAYOUT", "ELEMENT INDEPENDENCE", "COMPOSITION",
              "fma(beta, c_old, t)", "Argument rules, in this order", "EMPTY block", "ONE launch whatever the plan's classes"):
        assert s in section, s
    with open(os.path.join(ROOT, "capital_amd", "csrc", "gemm_batched.hip")) as f:
        head = f.read().split("#include", 1)[0]
    for s in ("THE ARITHMETIC", "THE BIT CONTRACTS", "fma(beta, c_old, t)", "out of scope", "gemm_batched_addr.h"):
        assert s in head, s


def test_python_layer_names_and_refusals():
    import torch
    from capital_amd import _lib, batched, blas
    for fn in (blas.engine._gemm_batched, blas.engine._gemm_vbatched_inner, blas.engine._gemm_vbatched_combine):
        assert callable(fn) and "256" in fn.__doc__
    for fn in (batched.gemm, batched.VarBatch.inner, batched.VarBatch.combine):
        assert callable(fn) and "256" in fn.__doc__ and "beta == 0" in fn.__doc__
    assert "gemm" in batched.__doc__ and "inner" in batched.VarBatch.__doc__ and "empty" in batched.VarBatch.inner.__doc__
    T, O = blas.Transpose, blas.Order
    row = blas.ArgPack_gemm(O.AblasRowMajor, T.AblasNoTrans, T.AblasNoTrans, 1.0, 0.0)
    col = blas.ArgPack_gemm(O.AblasColumnMajor, T.AblasNoTrans, T.AblasNoTrans, 1.0, 0.0)
    tn = blas.ArgPack_gemm(O.AblasColumnMajor, T.AblasTrans, T.AblasNoTrans, 1.0, 0.0)
    with pytest.raises(_lib.CapitalError, match="AblasColumnMajor"):
        blas.engine._gemm_batched(None, None, None, 4, 4, 1, 4, 4, 1, 4, 4, 16, 1, row)
    with pytest.raises(_lib.CapitalError, match="AblasColumnMajor"):
        blas.engine._gemm_vbatched_inner(None, None, None, None, 1, 1, 1, 1, 1, 1, row)
    with pytest.raises(_lib.CapitalError, match="AblasColumnMajor"):
        blas.engine._gemm_vbatched_combine(None, None, None, None, 1, 1, 1, 1, 1, 1, row)
    with pytest.raises(_lib.CapitalError, match="256"):
        blas.engine._gemm_batched(None, None, None, 257, 4, 1, 257, 257, 1, 4, 257, 257 * 4, 1, col)
    with pytest.raises(_lib.CapitalError, match="256"):
        blas.engine._gemm_vbatched_inner(None, None, None, None, 1, 257, 1, 1, 1, 257, tn)
    with pytest.raises(_lib.CapitalError, match="AblasTrans"):
        blas.engine._gemm_vbatched_inner(None, None, None, None, 1, 1, 1, 1, 1, 1, col)
    with pytest.raises(_lib.CapitalError, match="AblasNoTrans"):
        blas.engine._gemm_vbatched_combine(None, None, None, None, 1, 1, 1, 1, 1, 1, tn)
    a = torch.zeros(3, 4, 2, dtype=torch.float64)
    b = torch.zeros(3, 2, 5, dtype=torch.float64)
    vb = batched.VarBatch([3, 5])
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        batched.gemm(a, b)
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        vb.inner(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64))
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        vb.combine(torch.zeros(2, 3, 2, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.float64))
    for bad in (lambda: batched.gemm(None, b), lambda: batched.gemm(a, None), lambda: vb.inner(None, None), lambda: vb.combine(None, None)):
        with pytest.raises(_lib.CapitalError):
            bad()


def test_every_new_kernel_instance_keeps_its_accumulators_in_registers(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR - (4 NP + the workgroup kernel) x (fixed, inner,
    combine); the workgroup kernel at two waves per SIMD"""
    from capital_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if re.search(r"\d+gemm_batched(_blocked)?_kernelI", k)}
    assert len(res) == (4 + 1) * 3, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
        if "blocked" in k:
            assert int(v["Occupancy"]) >= 2, (k, v)
    for name in ("gemm_batched_kernel", "gemm_batched_blocked_kernel"):
        assert name in build.NO_SCRATCH


def test_one_annotated_launch_per_call_and_class_on_the_recording_stand_in(tmp_path):
    """the fixed-size entry on both paths with k = 0, 1 and 17, the four trans pairs, beta == 0 and != 0; `inner` (ONE launch for any
    plan) and `combine` (one per occurring class) on four size lists; the caller on the NULL stream and on a stream of its own"""
    from capital_amd import build
    build.build(verbose=False)
    out = tmp_path / "trace.json"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    res = json.load(open(out))
    assert len(res) == 2 * (len(TRACE_MN) + 2 * len(TRACE_LISTS))
    for x in res:
        assert not x["findings"], (x["name"], x["findings"][:4])
        assert x["stats"]["kernels"] == x["expected"] and not x["stats"].get("unannotated"), (x["name"], x["stats"], x["expected"])
        assert x["stats"]["oob"] == 0 and x["stats"].get("races", 0) == 0
        assert all(k.startswith("K ") and "gemm_batched" in k for k in x["launches"]), x["launches"]
        for name, lines in x["per_call"]:
            assert len(lines) == x["per_launches"] and all(l.startswith("K ") for l in lines), (x["name"], name, lines)   # launches and nothing else
        assert x["empty_calls"] == []
    inner = [x for x in res if x["name"].startswith("gemm inner")]
    assert inner and all(x["per_launches"] == 1 for x in inner)
    assert any(x["per_launches"] == 7 for x in res if x["name"].startswith("gemm combine EVERY"))


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
    results = []

    def finish(r, expected, per, bufs):
        out = r.finish()
        out["expected"], out["per_launches"] = expected, per
        out["launches"] = [l for l in r.lines if l.startswith("K ")]
        out["per_call"], out["empty_calls"] = _marks(r)
        for q in bufs:
            S.shim.hipFree(q)
        results.append(out)

    for user_stream in (0, 1):
        tag = " [user stream]" if user_stream else " [NULL stream]"
        for (m, n) in TRACE_MN:
            r = S.Run("gemm batched %dx%d%s" % (m, n, tag), user_stream)
            batch, ldc, kmax = 37, m + 1, max(TRACE_K)
            big = max(m, n, kmax) + 2
            Ad, Bd, Cd = S.dmalloc(8 * (big * big + 5) * batch), S.dmalloc(8 * (big * big + 5) * batch), S.dmalloc(8 * (ldc * n + 3) * batch)
            calls = 0
            for k in TRACE_K:
                for ta in (NOTRANS, TRANS):
                    for tb in (NOTRANS, TRANS):
                        lda, ldb = (k if ta else m) + 2, (n if tb else k) + 1
                        sa, sb = lda * (m if ta else k) + 5, ldb * (k if tb else n) + 2
                        for beta, sc in ((0.0, ldc * n), (1.0, ldc * n + 3)):
                            S.ok(r.call("dgemm_batched k=%d %d%d beta=%g" % (k, ta, tb, beta), S.L.cap_dgemm_batched, ta, tb, m, n, k, -1.0, Ad, lda, sa,
                                        Bd, ldb, sb, beta, Cd, ldc, sc, batch, r.stream), "cap_dgemm_batched")
                            calls += 1
                S.ok(r.call("dgemm_batched k=%d one block" % k, S.L.cap_dgemm_batched, TRANS, NOTRANS, m, n, k, 1.0, Ad, max(k, 1), 0, Bd, max(k, 1), 0,
                            0.0, Cd, m, 0, 1, r.stream), "cap_dgemm_batched")
                S.ok(r.call("dgemm_batched k=%d alpha=0, no A, B" % k, S.L.cap_dgemm_batched, NOTRANS, NOTRANS, m, n, k, 0.0, None, m, m * k, None,
                            max(k, 1), max(k, 1) * n, 1.0, Cd, ldc, ldc * n, batch, r.stream), "cap_dgemm_batched")
                calls += 2
            for c in (("empty batch=0", S.L.cap_dgemm_batched, 0, 0, m, n, 1, 1.0, None, m, 0, None, 1, 0, 0.0, None, m, 0, 0),
                      ("empty m=0", S.L.cap_dgemm_batched, 1, 1, 0, n, 1, 1.0, None, 1, 0, None, n, n, 0.0, None, 0, 0, batch),
                      ("empty n=0", S.L.cap_dgemm_batched, 0, 0, m, 0, 1, 1.0, None, m, m, None, 1, 0, 0.0, None, m, 0, batch)):
                S.ok(r.call(c[0], c[1], *c[2:], r.stream), c[0])
            finish(r, calls, 1, (Ad, Bd, Cd))
        for name in TRACE_LISTS:
            lay = VC.Layout(VC.LISTS[name], "gaps")
            plan, empty, none = C.c_void_p(), C.c_void_p(), C.c_void_p()
            S.ok(S.L.cap_vbatch_plan_create(lay.batch, arr(list(lay.sizes)), None, arr(list(lay.off_arg)), C.byref(plan)), "cap_vbatch_plan_create")
            S.ok(S.L.cap_vbatch_plan_create(3, arr([0, 0, 0]), None, None, C.byref(empty)), "cap_vbatch_plan_create")
            S.ok(S.L.cap_vbatch_plan_create(0, arr([]), None, None, C.byref(none)), "cap_vbatch_plan_create")
            classes = int(S.L.cap_vbatch_plan_info(plan, 4))
            assert classes >= 1
            # inner: ONE launch for any plan, the all-empty one included
            r = S.Run("gemm inner %s%s" % (name, tag), user_stream)
            Xd, Yd, Gd = S.dmalloc(8 * (lay.rows + 2) * 70), S.dmalloc(8 * (lay.rows + 3) * 70), S.dmalloc(8 * (70 * 66 + 3) * lay.batch)
            calls = []
            for (m, n) in ((1, 1), (3, 16), (17, 5), (64, 65)):
                for alpha, beta in ((2.0, 0.0), (1.0, 1.0), (0.0, 0.5)):
                    calls.append(("dgemm_vbatched_inner %dx%d alpha=%g beta=%g" % (m, n, alpha, beta), S.L.cap_dgemm_vbatched_inner, plan, m, n, alpha,
                                  Xd if alpha else None, lay.rows + 2, Yd if alpha else None, lay.rows + 3, beta, Gd, m + 1, (m + 1) * n + 3, r.stream))
            calls.append(("dgemm_vbatched_inner all blocks empty", S.L.cap_dgemm_vbatched_inner, empty, 3, 5, 1.0, None, 0, None, 0, 0.5, Gd, 3, 15,
                          r.stream))
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty no blocks", S.L.cap_dgemm_vbatched_inner, none, 3, 5, 1.0, None, 0, None, 0, 0.0, None, 3, 15, r.stream),
                      ("empty m=0", S.L.cap_dgemm_vbatched_inner, plan, 0, 5, 1.0, Xd, lay.rows, Yd, lay.rows, 0.0, None, 0, 0, r.stream)):
                S.ok(r.call(*c), c[0])
            finish(r, len(calls), 1, (Xd, Yd, Gd))
            # combine: one launch per occurring class
            r = S.Run("gemm combine %s%s" % (name, tag), user_stream)
            Vd, Zd, Cd = S.dmalloc(8 * (lay.rows + 2) * 42), S.dmalloc(8 * (42 * 17 + 3) * lay.batch), S.dmalloc(8 * (lay.rows + 3) * 17)
            calls = []
            for (nrhs, k) in ((1, 1), (16, 4), (17, 40), (3, 0)):
                for alpha, beta in ((2.0, 0.0), (1.0, 1.0)):
                    calls.append(("dgemm_vbatched_combine %dx%d beta=%g" % (nrhs, k, beta), S.L.cap_dgemm_vbatched_combine, plan, nrhs, k, alpha, Vd,
                                  lay.rows + 2, Zd, k + 1, (k + 1) * nrhs + 3, beta, Cd, lay.rows + 3, r.stream))
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty plan", S.L.cap_dgemm_vbatched_combine, empty, 3, 2, 1.0, None, 0, None, 2, 6, 0.0, None, 0, r.stream),
                      ("empty nrhs=0", S.L.cap_dgemm_vbatched_combine, plan, 0, 2, 1.0, Vd, lay.rows, Zd, 2, 0, 0.0, None, lay.rows, r.stream)):
                S.ok(r.call(*c), c[0])
            finish(r, len(calls) * classes, classes, (Vd, Zd, Cd))
            for q in (plan, empty, none):
                S.ok(S.L.cap_vbatch_plan_destroy(q), "cap_vbatch_plan_destroy")
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
