"""CPU-only: argument handling of the batched symmetric rank-k products (cap_dsyrk_batched, cap_dsyrk_vbatched) - the argument rules of
include/capital_amd.h in their order, every case decided before the library touches a device - the header / ctypes agreement, the Python
names and refusals, and the compiler's resource remarks of every new kernel instance.  The last test drives the two entries through the
recording stand-in of tests/hipshim in a process of its own (this file run as a script): one launch per fixed-size call, one per occurring
class on a plan, every launch annotated, no finding, nothing for an empty call."""
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
NOTRANS, TRANS = 0, 1
OK, ARG, HIP, UNSUPPORTED = 0, 1, 2, 4
TRACE_N = (8, 64, 65, 256)
TRACE_K = (1, 17)
TRACE_LISTS = ("EVERY", "WAVES", "ONE_CLASS", "LONE1")
NAMES = ("cap_dsyrk_batched", "cap_dsyrk_vbatched")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


V = C.c_void_p(1 << 20)                  # never dereferenced: every call below returns before any device work
CC = C.c_void_p(1 << 24)
SH = C.c_void_p(1 << 31)


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*a)


def fixed(L):
    def call(uplo=UPPER, trans=NOTRANS, n=10, k=3, alpha=1.0, V=V, ldv=10, stride_v=30, beta=0.0, C=CC, ldc=10, stride_c=100, shift=SH, fill=0, batch=5):
        return L.cap_dsyrk_batched(uplo, trans, n, k, alpha, V, ldv, stride_v, beta, C, ldc, stride_c, shift, fill, batch, None)
    return call


def test_fixed_size_arguments_are_checked_in_the_documented_order(L):
    call = fixed(L)
    n = 10
    big = dict(n=257, ldv=257, ldc=257, stride_v=257 * 3, stride_c=257 * 257)
    # 1. trans, negative sizes, fill
    for trans in (2, -1, 255):
        assert call(trans=trans) == ARG and call(trans=trans, uplo=LOWER) == ARG and call(trans=trans, **big) == ARG
        assert call(trans=trans, batch=0) == ARG and call(trans=trans, k=0) == ARG and call(trans=trans, n=0) == ARG
    assert call(n=-1) == ARG and call(k=-1) == ARG and call(batch=-1) == ARG
    assert call(n=-1, uplo=LOWER) == ARG and call(k=-1, batch=0) == ARG
    for fill in (2, -1):
        assert call(fill=fill) == ARG and call(fill=fill, uplo=LOWER) == ARG and call(fill=fill, batch=0) == ARG and call(fill=fill, **big) == ARG
    assert call(fill=1, batch=0) == OK
    # 2. C, 3. V (only with n k batch > 0 and alpha != 0)
    assert call(C=None) == ARG and call(C=None, uplo=LOWER) == ARG and call(C=None, k=0) == ARG and call(C=None, ldc=9) == ARG
    assert call(V=None) == ARG and call(V=None, uplo=LOWER) == ARG and call(V=None, ldv=9) == ARG
    assert call(V=None, alpha=0.0, uplo=LOWER) == UNSUPPORTED and call(V=None, k=0, uplo=LOWER) == UNSUPPORTED
    assert call(V=None, batch=0) == OK and call(C=None, batch=0) == OK
    # 4. ldc, 5. ldv (n or k), 6. strides
    assert call(ldc=n - 1) == ARG and call(ldc=n - 1, uplo=LOWER) == ARG
    assert call(ldv=n - 1) == ARG and call(ldv=n - 1, uplo=LOWER) == ARG and call(ldv=n - 1, alpha=0.0) == ARG
    assert call(trans=TRANS, ldv=2) == ARG and call(trans=TRANS, ldv=3, stride_v=30, uplo=LOWER) == UNSUPPORTED
    assert call(trans=TRANS, ldv=3, stride_v=29) == ARG and call(trans=TRANS, k=12, ldv=11) == ARG
    assert call(stride_c=n * n - 1) == ARG and call(stride_v=n * 3 - 1) == ARG
    assert call(ldc=n + 2, stride_c=(n + 2) * n - 1) == ARG and call(ldv=n + 2, stride_v=(n + 2) * 3 - 1) == ARG
    assert call(stride_c=-1) == ARG and call(stride_v=-1) == ARG
    assert call(stride_c=0, stride_v=0, batch=1, uplo=LOWER) == UNSUPPORTED       # one block needs no stride ...
    assert call(stride_c=0, batch=2, uplo=LOWER) == ARG and call(stride_v=0, batch=2, uplo=LOWER) == ARG   # ... two do
    assert call(ldc=1 << 40, stride_c=1 << 62, n=1 << 30, ldv=1 << 30, stride_v=1 << 62) == ARG            # the clipped product
    assert call(n=16, ldc=1 << 60, stride_c=0, ldv=16, stride_v=48, batch=2) == ARG                        # 2^64 does not wrap to 0
    assert call(**dict(big, ldc=256)) == ARG and call(**dict(big, ldv=256)) == ARG          # the argument rules come before the size limit
    # 8. LOWER, 9. n > 256, 10. the grid
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7) == UNSUPPORTED
    assert call(uplo=LOWER, n=0) == UNSUPPORTED and call(uplo=LOWER, k=0) == UNSUPPORTED and call(uplo=LOWER, batch=0) == UNSUPPORTED
    assert call(uplo=LOWER, **big) == UNSUPPORTED
    assert call(**big) == UNSUPPORTED and call(batch=0, **big) == UNSUPPORTED
    g65 = dict(n=65, ldv=65, ldc=65, stride_v=65 * 3, stride_c=65 * 65)
    assert call(batch=1 << 31, **g65) == UNSUPPORTED
    assert call(batch=1 << 31, **dict(g65, ldc=64)) == ARG
    assert call(n=8, ldv=8, ldc=8, stride_v=24, stride_c=64, batch=1 << 34) == UNSUPPORTED       # eight blocks per wavefront: 2^31 workgroups
    # 11. nothing to do: no launch, whatever the pointers
    assert call(n=0, V=None, C=None, ldv=0, ldc=0, stride_v=0, stride_c=0, shift=None) == OK
    assert call(batch=0, V=None, C=None, stride_v=-5, stride_c=-5, shift=None) == OK
    assert call(n=0) == OK and call(batch=0) == OK
    for sz in (64, 65, 256):
        kw = dict(n=sz, ldv=sz, ldc=sz, stride_v=sz * 3, stride_c=sz * sz)
        assert call(batch=0, **kw) == OK and call(batch=0, V=None, C=None, **kw) == OK
        assert call(**dict(kw, ldc=sz - 1)) == ARG and call(**dict(kw, stride_v=sz * 3 - 1)) == ARG
        assert call(C=None, **kw) == ARG and call(uplo=LOWER, **kw) == UNSUPPORTED


def create(L, n):
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(len(n), arr(n), None, None, C.byref(p)) == OK
    return p


def test_plan_entry_arguments_are_checked_in_the_documented_order(L):
    """no call here reaches a launch: in a process without a device the accepted calls on a non-empty plan would end in CAP_ERR_HIP"""
    p, p0, p1 = create(L, [5, 0, 100]), create(L, [0, 0, 0]), create(L, [])

    def call(p=p, uplo=UPPER, trans=NOTRANS, k=3, alpha=1.0, V=V, ldv=1 << 20, beta=0.0, C=CC, shift=SH, fill=0):
        return L.cap_dsyrk_vbatched(p, uplo, trans, k, alpha, V, ldv, beta, C, shift, fill, None)
    assert call(p=None) == ARG and call(p=None, uplo=LOWER) == ARG
    for trans in (2, -1):
        assert call(trans=trans) == ARG and call(trans=trans, uplo=LOWER) == ARG and call(trans=trans, p=p0) == ARG
    assert call(k=-1) == ARG and call(k=-1, uplo=LOWER) == ARG and call(k=-1, p=p1) == ARG
    assert call(fill=2) == ARG and call(fill=-1, uplo=LOWER) == ARG and call(fill=2, p=p0) == ARG
    assert call(C=None) == ARG and call(V=None) == ARG and call(C=None, uplo=LOWER) == ARG and call(C=None, k=0) == ARG
    assert call(V=None, alpha=0.0, uplo=LOWER) == UNSUPPORTED and call(V=None, k=0, uplo=LOWER) == UNSUPPORTED
    assert call(ldv=104) == ARG and call(ldv=104, uplo=LOWER) == ARG and call(ldv=104, k=0) == ARG      # sum n_i = 105
    assert call(ldv=105, uplo=LOWER) == UNSUPPORTED
    assert call(trans=TRANS, ldv=2) == ARG and call(trans=TRANS, ldv=3, uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7) == UNSUPPORTED
    for q in (p0, p1):                                                 # nothing to launch: pointers may be NULL, LOWER is still refused
        assert call(p=q, V=None, C=None, shift=None, ldv=3) == OK and call(p=q) == OK and call(p=q, trans=TRANS) == OK
        assert call(p=q, uplo=LOWER) == UNSUPPORTED
        assert call(p=q, ldv=-1) == ARG
    import torch
    if not torch.cuda.is_available():
        assert call() == HIP and call(k=0) == HIP                      # a plan made without a device
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
    section = header[header.index("csrc/syrk_batched.hip"):]
    for s in ("THE BIT CONTRACTS", "PLAN = FIXED", "LAYOUT INDEPENDENCE", "TRANS IS A LAYOUT", "ELEMENT INDEPENDENCE", "fma(beta, c_old, t)",
              "Argument rules, in this order"):
        assert s in section, s
    with open(os.path.join(ROOT, "capital_amd", "csrc", "syrk_batched.hip")) as f:
        head = f.read().split("#include", 1)[0]
    for s in ("THE ARITHMETIC", "THE BIT CONTRACTS", "fma(beta, c_old, t)", "out of scope"):
        assert s in head, s


def test_python_layer_names_and_refusals():
    import torch
    from capital_amd import _lib, batched, blas
    for fn in (blas.engine._syrk_batched, blas.engine._syrk_vbatched):
        assert callable(fn) and "256" in fn.__doc__
    for fn in (batched.syrk, batched.VarBatch.syrk, batched.schur):
        assert callable(fn) and "LOWER" in fn.__doc__
    assert "WHITENED" in batched.schur.__doc__ and "NaN" in batched.schur.__doc__
    row = blas.ArgPack_syrk(blas.Order.AblasRowMajor, blas.UpLo.AblasUpper, blas.Transpose.AblasNoTrans, 1.0, 0.0)
    with pytest.raises(_lib.CapitalError, match="AblasColumnMajor"):
        blas.engine._syrk_batched(None, None, 4, 1, 4, 4, 4, 16, 1, row)
    with pytest.raises(_lib.CapitalError, match="AblasColumnMajor"):
        blas.engine._syrk_vbatched(None, None, None, 1, 4, 1, row)
    col = blas.ArgPack_syrk(blas.Order.AblasColumnMajor, blas.UpLo.AblasUpper, blas.Transpose.AblasNoTrans, 1.0, 0.0)
    with pytest.raises(_lib.CapitalError, match="256"):
        blas.engine._syrk_batched(None, None, 257, 1, 257, 257, 257, 257 * 257, 1, col)
    v = torch.zeros(3, 2, 10, dtype=torch.float64)
    c = torch.zeros(3, 10, 10, dtype=torch.float64)
    vb = batched.VarBatch([3, 5])
    for bad in (lambda: batched.syrk(v), lambda: batched.syrk(v, c), lambda: batched.syrk(None), lambda: batched.syrk(v.to(torch.float32)),
                lambda: batched.schur(c, v, c), lambda: vb.syrk(torch.zeros(2, 8, dtype=torch.float64)), lambda: vb.syrk(None),
                lambda: vb.syrk(torch.zeros(8, dtype=torch.float64), trans=True)):
        with pytest.raises(_lib.CapitalError):
            bad()


def test_every_new_kernel_instance_keeps_its_accumulators_in_registers(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR - (4 NP + the workgroup kernel) x 2 layouts x
    (fixed size, plan)"""
    from capital_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if re.search(r"\d+syrk_v?batched(_blocked)?_kernelI", k)}
    assert len(res) == (4 + 1) * 2 * 2, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
    for name in ("syrk_batched_kernel", "syrk_vbatched_kernel", "syrk_batched_blocked_kernel", "syrk_vbatched_blocked_kernel"):
        assert name in build.NO_SCRATCH


def test_one_annotated_launch_per_call_and_class_on_the_recording_stand_in(tmp_path):
    """the fixed-size entry at n = 8, 64, 65, 256 with k = 1 and 17, both layouts, beta == 0 and != 0, with and without shift and fill; the
    plan entry on four size lists; the caller on the NULL stream and on a stream of its own"""
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
        assert all(k.startswith("K ") and "syrk_" in k and "batched" in k for k in x["launches"]), x["launches"]
        for name, lines in x["per_call"]:
            assert len(lines) == x["per_launches"] and all(l.startswith("K ") for l in lines), (x["name"], name, lines)   # launches and nothing else
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
    results = []
    for user_stream in (0, 1):
        tag = " [user stream]" if user_stream else " [NULL stream]"
        for n in TRACE_N:
            r = S.Run("syrk batched n=%d%s" % (n, tag), user_stream)
            batch, ldc, kmax = 37, n + 1, max(TRACE_K)
            Vd, Cd, sh = S.dmalloc(8 * ((max(n, kmax) + 2) * max(n, kmax) + 5) * batch), S.dmalloc(8 * (ldc * n + 3) * batch), S.dmalloc(8 * batch)
            calls = 0
            for k in TRACE_K:
                for trans in (TRANS, NOTRANS):
                    ldv = (k if trans else n) + 2
                    sv = ldv * (n if trans else k)
                    for beta, shift, fill, sc, dv in ((0.0, sh, 1, ldc * n, 0), (1.0, None, 0, ldc * n + 3, 5)):
                        S.ok(r.call("dsyrk_batched k=%d trans=%d beta=%g fill=%d" % (k, trans, beta, fill), S.L.cap_dsyrk_batched, 1, trans, n, k, -1.0,
                                    Vd, ldv, sv + dv, beta, Cd, ldc, sc, shift, fill, batch, r.stream), "cap_dsyrk_batched")
                        calls += 1
                S.ok(r.call("dsyrk_batched k=%d one block" % k, S.L.cap_dsyrk_batched, 1, TRANS, n, k, 1.0, Vd, k, 0, 0.0, Cd, ldc, 0, None, 0, 1,
                            r.stream), "cap_dsyrk_batched")
                S.ok(r.call("dsyrk_batched k=%d alpha=0, no V" % k, S.L.cap_dsyrk_batched, 1, NOTRANS, n, k, 0.0, None, n, n * k, 1.0, Cd, ldc, ldc * n, sh,
                            0, batch, r.stream), "cap_dsyrk_batched")
                calls += 2
            for c in (("empty batch=0", S.L.cap_dsyrk_batched, 1, 0, n, 1, 1.0, None, n, 0, 0.0, None, n, 0, None, 0, 0),
                      ("empty n=0", S.L.cap_dsyrk_batched, 1, 1, 0, 1, 1.0, None, 1, 0, 0.0, None, 0, 0, None, 0, batch)):
                S.ok(r.call(c[0], c[1], *c[2:], r.stream), c[0])
            out = r.finish()
            out["expected"], out["per_launches"] = calls, 1
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Vd, Cd, sh):
                S.shim.hipFree(q)
            results.append(out)
        for name in TRACE_LISTS:
            lay = VC.Layout(VC.LISTS[name], "gaps")
            plan, empty = C.c_void_p(), C.c_void_p()
            S.ok(S.L.cap_vbatch_plan_create(lay.batch, arr(list(lay.sizes)), None, arr(list(lay.off_arg)), C.byref(plan)), "cap_vbatch_plan_create")
            S.ok(S.L.cap_vbatch_plan_create(3, arr([0, 0, 0]), None, None, C.byref(empty)), "cap_vbatch_plan_create")
            r = S.Run("syrk vbatched %s%s" % (name, tag), user_stream)
            kmax = max(TRACE_K)
            Cd, Vd, sh = S.dmalloc(8 * lay.total), S.dmalloc(8 * (lay.rows + 2) * (kmax + 2)), S.dmalloc(8 * lay.batch)
            calls = []
            for k in TRACE_K:
                for trans in (TRANS, NOTRANS):
                    ldv = (k + 2) if trans else (lay.rows + 2)
                    for beta, shift, fill in ((0.0, sh, 1), (1.0, None, 0)):
                        calls.append(("dsyrk_vbatched k=%d trans=%d beta=%g" % (k, trans, beta), S.L.cap_dsyrk_vbatched, plan, 1, trans, k, 2.0, Vd, ldv,
                                      beta, Cd, shift, fill, r.stream))
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty plan", S.L.cap_dsyrk_vbatched, empty, 1, 1, 3, 1.0, None, 3, 0.0, None, None, 0, r.stream),):
                S.ok(r.call(*c), c[0])
            out = r.finish()
            classes = int(S.L.cap_vbatch_plan_info(plan, 4))
            assert classes >= 1
            out["expected"], out["per_launches"] = len(calls) * classes, classes
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Cd, Vd, sh):
                S.shim.hipFree(q)
            S.ok(S.L.cap_vbatch_plan_destroy(plan), "cap_vbatch_plan_destroy")
            S.ok(S.L.cap_vbatch_plan_destroy(empty), "cap_vbatch_plan_destroy")
            results.append(out)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
