"""CPU-only: argument handling of the batched triangular solves and products (cap_dtrsm_batched, cap_dtrmm_batched, cap_dtrsm_vbatched,
cap_dtrmm_vbatched) - the argument rules of include/capital_amd.h in their order, every case decided before the library touches a device -
the header / ctypes agreement, the Python names and refusals, and the compiler's resource remarks of every new kernel instance.  The last
test drives the four entries through the recording stand-in of tests/hipshim in a process of its own (this file run as a script): one
launch per fixed-size call, one per occurring class on a plan, every launch annotated, no finding, nothing for an empty call."""
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
TRACE_NRHS = (1, 17)
TRACE_LISTS = ("EVERY", "WAVES", "ONE_CLASS", "LONE1")
NAMES = ("cap_dtrsm_batched", "cap_dtrmm_batched", "cap_dtrsm_vbatched", "cap_dtrmm_vbatched")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


R = C.c_void_p(1 << 20)                  # never dereferenced: every call below returns before any device work
B = C.c_void_p(1 << 24)
INFO = C.c_void_p(1 << 31)
Q = C.c_void_p(1 << 33)


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*a)


def fixed(L, mul):
    def call(uplo=UPPER, trans=TRANS, n=10, nrhs=3, R=R, ldr=10, stride_r=100, B=B, ldb=10, stride_b=30, batch=5, info=INFO, sumsq=None, ldq=0):
        if mul:
            return L.cap_dtrmm_batched(uplo, trans, n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, None)
        return L.cap_dtrsm_batched(uplo, trans, n, nrhs, R, ldr, stride_r, B, ldb, stride_b, batch, info, sumsq, ldq, None)
    return call


@pytest.mark.parametrize("mul", (0, 1), ids=("trsm", "trmm"))
def test_fixed_size_arguments_are_checked_in_the_documented_order(L, mul):
    call = fixed(L, mul)
    n = 10
    big = dict(n=257, ldr=257, ldb=257, stride_r=257 * 257, stride_b=257 * 3)
    # 1. trans, negative sizes
    for trans in (2, -1, 255):
        assert call(trans=trans) == ARG and call(trans=trans, uplo=LOWER) == ARG and call(trans=trans, **big) == ARG
        assert call(trans=trans, batch=0) == ARG and call(trans=trans, nrhs=0) == ARG and call(trans=trans, n=0) == ARG
    assert call(trans=NOTRANS, batch=0) == OK
    assert call(n=-1) == ARG and call(nrhs=-1) == ARG and call(batch=-1) == ARG
    assert call(n=-1, uplo=LOWER) == ARG and call(nrhs=-1, batch=0) == ARG
    # pointers (with n nrhs batch > 0), leading dimensions, strides
    assert call(R=None) == ARG and call(B=None) == ARG and call(R=None, uplo=LOWER) == ARG
    assert call(ldr=n - 1) == ARG and call(ldb=n - 1) == ARG and call(ldb=n - 1, uplo=LOWER) == ARG
    assert call(stride_r=n * n - 1) == ARG and call(stride_b=n * 3 - 1) == ARG
    assert call(ldr=n + 2, stride_r=(n + 2) * n - 1) == ARG and call(ldb=n + 2, stride_b=(n + 2) * 3 - 1) == ARG
    assert call(stride_r=-1) == ARG and call(stride_b=-1) == ARG
    assert call(n=16, ldr=1 << 60, stride_r=0, ldb=16, batch=2) == ARG and call(n=16, nrhs=16, ldr=16, ldb=1 << 60, stride_b=0, batch=2) == ARG   # 2^64 does not wrap to 0
    assert call(stride_r=0, stride_b=0, batch=1, uplo=LOWER) == UNSUPPORTED       # one block needs no stride ...
    assert call(stride_r=0, batch=2, uplo=LOWER) == ARG and call(stride_b=0, batch=2, uplo=LOWER) == ARG   # ... two do
    assert call(**dict(big, ldr=256)) == ARG and call(**dict(big, ldb=256)) == ARG          # the argument rules come before the size limit
    if not mul:
        assert call(sumsq=Q, ldq=2) == ARG and call(sumsq=Q, ldq=2, uplo=LOWER) == ARG and call(sumsq=Q, ldq=2, **big) == ARG
        assert call(sumsq=Q, ldq=2, batch=0) == ARG and call(sumsq=Q, ldq=-1, nrhs=0) == ARG
        assert call(sumsq=None, ldq=-5, batch=0) == OK and call(sumsq=Q, ldq=3, batch=0) == OK and call(sumsq=Q, ldq=0, nrhs=0) == OK
    # 2. LOWER, 3. n > 256, 4. the grid
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7) == UNSUPPORTED
    assert call(uplo=LOWER, n=0) == UNSUPPORTED and call(uplo=LOWER, nrhs=0) == UNSUPPORTED and call(uplo=LOWER, batch=0) == UNSUPPORTED
    assert call(uplo=LOWER, **big) == UNSUPPORTED
    assert call(**big) == UNSUPPORTED and call(batch=0, **big) == UNSUPPORTED and call(**dict(big, nrhs=0)) == UNSUPPORTED
    assert call(n=1 << 20, ldr=1 << 20, ldb=1 << 20, stride_r=1 << 40, stride_b=1 << 22) == UNSUPPORTED
    g65 = dict(n=65, ldr=65, ldb=65, stride_r=65 * 65, stride_b=65 * 3)
    assert call(batch=1 << 31, **g65) == UNSUPPORTED and call(batch=(1 << 31) - 1, nrhs=0, **g65) == OK
    assert call(batch=1 << 31, **dict(g65, ldr=64)) == ARG
    assert call(batch=1 << 31, **dict(g65, nrhs=0)) == UNSUPPORTED                 # before the empty case
    assert call(n=8, ldr=8, ldb=8, stride_r=64, stride_b=24, batch=1 << 34, nrhs=0) == UNSUPPORTED       # eight blocks per wavefront: 2^31 workgroups
    assert call(n=8, ldr=8, ldb=8, stride_r=64, stride_b=24, batch=(1 << 34) - 8, nrhs=0) == OK
    # 5. nothing to do: no launch, whatever the pointers
    assert call(n=0, R=None, B=None, ldr=0, ldb=0, stride_r=0, stride_b=0, info=None) == OK
    assert call(nrhs=0, R=None, B=None, stride_r=100, stride_b=0, info=None) == OK
    assert call(batch=0, R=None, B=None, stride_r=-5, stride_b=-5, info=None) == OK
    assert call(n=0) == OK and call(nrhs=0) == OK and call(batch=0) == OK
    for sz in (64, 65, 256):
        kw = dict(n=sz, ldr=sz, ldb=sz, stride_r=sz * sz, stride_b=sz * 3)
        assert call(batch=0, **kw) == OK and call(batch=0, R=None, B=None, **kw) == OK
        assert call(**dict(kw, ldr=sz - 1)) == ARG and call(**dict(kw, stride_b=sz * 3 - 1)) == ARG
        assert call(R=None, **kw) == ARG and call(uplo=LOWER, **kw) == UNSUPPORTED


def create(L, n):
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(len(n), arr(n), None, None, C.byref(p)) == OK
    return p


@pytest.mark.parametrize("mul", (0, 1), ids=("trsm", "trmm"))
def test_plan_entry_arguments_are_checked_in_the_documented_order(L, mul):
    """no call here reaches a launch: in a process without a device the accepted calls on a non-empty plan would end in CAP_ERR_HIP"""
    p, p0, p1 = create(L, [5, 0, 100]), create(L, [0, 0, 0]), create(L, [])

    def call(p=p, uplo=UPPER, trans=TRANS, nrhs=3, R=R, B=B, ldb=1 << 20, info=INFO, sumsq=None, ldq=0):
        if mul:
            return L.cap_dtrmm_vbatched(p, uplo, trans, nrhs, R, B, ldb, info, None)
        return L.cap_dtrsm_vbatched(p, uplo, trans, nrhs, R, B, ldb, info, sumsq, ldq, None)
    assert call(p=None) == ARG and call(p=None, uplo=LOWER) == ARG
    for trans in (2, -1):
        assert call(trans=trans) == ARG and call(trans=trans, uplo=LOWER) == ARG and call(trans=trans, p=p0) == ARG and call(trans=trans, nrhs=0) == ARG
    assert call(nrhs=-1) == ARG and call(nrhs=-1, uplo=LOWER) == ARG and call(nrhs=-1, p=p1) == ARG
    assert call(R=None) == ARG and call(B=None) == ARG and call(R=None, uplo=LOWER) == ARG
    assert call(ldb=104) == ARG and call(ldb=104, uplo=LOWER) == ARG and call(ldb=104, nrhs=0) == ARG      # sum n_i = 105
    assert call(ldb=105, uplo=LOWER) == UNSUPPORTED
    if not mul:
        assert call(sumsq=Q, ldq=2) == ARG and call(sumsq=Q, ldq=2, uplo=LOWER) == ARG and call(sumsq=Q, ldq=2, p=p0) == ARG
        assert call(sumsq=Q, ldq=3, nrhs=0) == OK and call(sumsq=None, ldq=-1, nrhs=0) == OK
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7) == UNSUPPORTED
    assert call(nrhs=0) == OK and call(nrhs=0, R=None, B=None, ldb=105, info=None) == OK and call(nrhs=0, trans=NOTRANS) == OK
    assert call(nrhs=0, uplo=LOWER) == UNSUPPORTED
    for q in (p0, p1):                                                 # nothing to launch: pointers may be NULL, LOWER is still refused
        assert call(p=q, R=None, B=None, info=None, ldb=0) == OK and call(p=q) == OK and call(p=q, trans=NOTRANS) == OK
        assert call(p=q, uplo=LOWER) == UNSUPPORTED
        assert call(p=q, ldb=-1) == ARG
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
    section = header[header.index("csrc/trsm_batched.hip"):]
    for s in ("THE BIT CONTRACTS", "HALVES = WHOLE", "PLAN = FIXED", "COLUMN INDEPENDENCE", "q = fma(x_r, x_r, q)", "Argument rules, in this order"):
        assert s in section, s


def test_python_layer_names():
    from capital_amd import _lib, batched, lapack
    cm, up = lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper
    packs = (lapack.ArgPack_trsm_batched(cm, up), lapack.ArgPack_trmm_batched(cm, up), lapack.ArgPack_trsm_vbatched(cm, up),
             lapack.ArgPack_trmm_vbatched(cm, up))
    assert [int(p.method) for p in packs] == [0x14, 0x15, 0x16, 0x17]
    assert [p.method for p in packs] == [lapack.Method.AlapackTrsmBatched, lapack.Method.AlapackTrmmBatched, lapack.Method.AlapackTrsmVbatched,
                                         lapack.Method.AlapackTrmmVbatched]
    assert len({int(m) for m in lapack.Method}) == len(list(lapack.Method))
    for fn in (lapack.engine._trsm_batched, lapack.engine._trmm_batched, lapack.engine._trsm_vbatched, lapack.engine._trmm_vbatched):
        assert callable(fn) and "256" in fn.__doc__
    for fn in (batched.trsm, batched.trmm, batched.mahalanobis, batched.VarBatch.trsm, batched.VarBatch.trmm, batched.VarBatch.mahalanobis):
        assert callable(fn) and "LOWER triangle" in fn.__doc__ and "L = R^T" in fn.__doc__
    assert "L^-1 b" in batched.trsm.__doc__ and "L^-T b" in batched.trsm.__doc__ and "L z" in batched.trmm.__doc__ and "L^T z" in batched.trmm.__doc__
    with pytest.raises(_lib.CapitalError, match="256"):
        lapack.engine._trsm_batched(None, None, 257, 1, 257, 257 * 257, 257, 257, 1, True, None, packs[0])
    with pytest.raises(_lib.CapitalError, match="256"):
        lapack.engine._trmm_batched(None, None, 257, 1, 257, 257 * 257, 257, 257, 1, False, None, packs[1])


def test_cpu_tensors_wrong_types_and_shapes_are_refused():
    import torch
    from capital_amd import _lib, batched
    r = torch.eye(10, dtype=torch.float64).repeat(3, 1, 1)
    b = torch.zeros(3, 2, 10, dtype=torch.float64)
    vb = batched.VarBatch([3, 5])
    flat = torch.zeros(vb.total, dtype=torch.float64)
    for fn in (batched.trsm, batched.trmm, batched.mahalanobis):
        for bad in (lambda: fn(r, b), lambda: fn(r.to(torch.float32), b), lambda: fn(torch.eye(4, dtype=torch.float64), b), lambda: fn(None, b),
                    lambda: fn(r, None)):
            with pytest.raises(_lib.CapitalError):
                bad()
    for fn in (vb.trsm, vb.trmm, vb.mahalanobis):
        for bad in (lambda: fn(flat, torch.zeros(8, dtype=torch.float64)), lambda: fn(flat.to(torch.float32), torch.zeros(8, dtype=torch.float64)),
                    lambda: fn(None, None), lambda: fn(flat, torch.zeros(2, 7, dtype=torch.float64))):
            with pytest.raises(_lib.CapitalError):
                bad()


def test_every_new_kernel_instance_keeps_its_columns_in_registers(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR - 4 operations x (4 NP + the workgroup kernel) x
    (fixed size, plan)"""
    from capital_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if re.search(r"\d+tri_v?batched(_blocked)?_kernelI", k)}      # (not potri_...)
    assert len(res) == 4 * (4 + 1) * 2, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
    for name in ("tri_batched_kernel", "tri_vbatched_kernel", "tri_batched_blocked_kernel", "tri_vbatched_blocked_kernel"):
        assert name in build.NO_SCRATCH


def test_one_annotated_launch_per_call_and_class_on_the_recording_stand_in(tmp_path):
    """the fixed-size entries at n = 8, 64, 65, 256 with nrhs = 1 and 17, both trans values, with and without sumsq; the plan entries on four
    size lists; the caller on the NULL stream and on a stream of its own"""
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
        assert all(k.startswith("K ") and "tri_" in k and "batched" in k for k in x["launches"]), x["launches"]
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
            r = S.Run("trsm batched n=%d%s" % (n, tag), user_stream)
            batch, ldr, ldb, kmax = 37, n + 1, n + 2, max(TRACE_NRHS)
            Rd, Bd = S.dmalloc(8 * (ldr * n + 3) * batch), S.dmalloc(8 * (ldb * kmax + 5) * batch)
            info, Qd = S.dmalloc(4 * batch), S.dmalloc(8 * (kmax + 1) * batch)
            calls = 0
            for k in TRACE_NRHS:
                for trans in (TRANS, NOTRANS):
                    for inf, sr, sb, q, ldq in ((info, ldr * n, ldb * k, Qd, k + 1), (None, ldr * n + 3, ldb * k + 5, None, 0)):
                        S.ok(r.call("dtrsm_batched k=%d trans=%d sumsq=%d" % (k, trans, q is not None), S.L.cap_dtrsm_batched, 1, trans, n, k, Rd, ldr,
                                    sr, Bd, ldb, sb, batch, inf, q, ldq, r.stream), "cap_dtrsm_batched")
                        S.ok(r.call("dtrmm_batched k=%d trans=%d" % (k, trans), S.L.cap_dtrmm_batched, 1, trans, n, k, Rd, ldr, sr, Bd, ldb, sb,
                                    batch, inf, r.stream), "cap_dtrmm_batched")
                        calls += 2
                S.ok(r.call("dtrsm_batched k=%d one block" % k, S.L.cap_dtrsm_batched, 1, TRANS, n, k, Rd, ldr, 0, Bd, ldb, 0, 1, None, Qd, k,
                            r.stream), "cap_dtrsm_batched")
                calls += 1
            for c in (("empty nrhs=0", S.L.cap_dtrsm_batched, 1, 1, n, 0, Rd, ldr, ldr * n, Bd, ldb, 0, batch, info, Qd, 0),
                      ("empty batch=0", S.L.cap_dtrsm_batched, 1, 0, n, 1, None, ldr, 0, None, ldb, 0, 0, None, None, 0),
                      ("empty n=0", S.L.cap_dtrsm_batched, 1, 1, 0, 1, None, 0, 0, None, 0, 0, batch, None, None, 0),
                      ("empty trmm nrhs=0", S.L.cap_dtrmm_batched, 1, 1, n, 0, Rd, ldr, ldr * n, Bd, ldb, 0, batch, info),
                      ("empty trmm batch=0", S.L.cap_dtrmm_batched, 1, 0, n, 1, None, ldr, 0, None, ldb, 0, 0, None)):
                S.ok(r.call(c[0], c[1], *c[2:], r.stream), c[0])
            out = r.finish()
            out["expected"], out["per_launches"] = calls, 1
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Rd, Bd, info, Qd):
                S.shim.hipFree(q)
            results.append(out)
        for name in TRACE_LISTS:
            lay = VC.Layout(VC.LISTS[name], "gaps")
            plan, empty = C.c_void_p(), C.c_void_p()
            S.ok(S.L.cap_vbatch_plan_create(lay.batch, arr(list(lay.sizes)), None, arr(list(lay.off_arg)), C.byref(plan)), "cap_vbatch_plan_create")
            S.ok(S.L.cap_vbatch_plan_create(3, arr([0, 0, 0]), None, None, C.byref(empty)), "cap_vbatch_plan_create")
            r = S.Run("trsm vbatched %s%s" % (name, tag), user_stream)
            ldb, kmax = lay.rows + 2, max(TRACE_NRHS)
            Rd, Bd, info, Qd = S.dmalloc(8 * lay.total), S.dmalloc(8 * ldb * kmax), S.dmalloc(4 * lay.batch), S.dmalloc(8 * (kmax + 1) * lay.batch)
            calls = []
            for k in TRACE_NRHS:
                for trans in (TRANS, NOTRANS):
                    for inf, q, ldq in ((info, Qd, k + 1), (None, None, 0)):
                        calls.append(("dtrsm_vbatched k=%d trans=%d sumsq=%d" % (k, trans, q is not None), S.L.cap_dtrsm_vbatched, plan, 1, trans, k, Rd, Bd,
                                      ldb, inf, q, ldq, r.stream))
                        calls.append(("dtrmm_vbatched k=%d trans=%d" % (k, trans), S.L.cap_dtrmm_vbatched, plan, 1, trans, k, Rd, Bd, ldb, inf, r.stream))
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty plan", S.L.cap_dtrsm_vbatched, empty, 1, 1, 3, None, None, 0, None, None, 0, r.stream),
                      ("empty nrhs=0", S.L.cap_dtrsm_vbatched, plan, 1, 0, 0, None, None, ldb, None, None, 0, r.stream),
                      ("empty trmm plan", S.L.cap_dtrmm_vbatched, empty, 1, 1, 3, None, None, 0, None, r.stream),
                      ("empty trmm nrhs=0", S.L.cap_dtrmm_vbatched, plan, 1, 0, 0, None, None, ldb, None, r.stream)):
                S.ok(r.call(*c), c[0])
            out = r.finish()
            classes = int(S.L.cap_vbatch_plan_info(plan, 4))
            assert classes >= 1
            out["expected"], out["per_launches"] = len(calls) * classes, classes
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Rd, Bd, info, Qd):
                S.shim.hipFree(q)
            S.ok(S.L.cap_vbatch_plan_destroy(plan), "cap_vbatch_plan_destroy")
            S.ok(S.L.cap_vbatch_plan_destroy(empty), "cap_vbatch_plan_destroy")
            results.append(out)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
