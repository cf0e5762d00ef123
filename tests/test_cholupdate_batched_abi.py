"""CPU-only: argument handling of the batched rank-k update / downdate (cap_dcholupdate_batched, cap_dcholupdate_vbatched) - the argument
rules of include/capital_amd.h in their order, every case decided before the library touches a device - the header / ctypes agreement and
the Python names.  The last test drives both entries through the recording stand-in of tests/hipshim in a process of its own (this file run
as a script): one launch per fixed-size call, one per occurring class on a plan, every launch annotated, no finding, nothing for an empty
call."""
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
TRACE_N = (8, 64, 65, 256)
TRACE_K = (1, 17)
TRACE_LISTS = ("EVERY", "WAVES", "ONE_CLASS", "LONE1")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


R = C.c_void_p(1 << 20)                  # never dereferenced: every call below returns before any device work
V = C.c_void_p(1 << 24)
INFO = C.c_void_p(1 << 31)


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*a)


def fixed(L):
    def call(uplo=UPPER, sign=1, n=10, k=3, R=R, ldr=10, stride_r=100, V=V, ldv=10, stride_v=30, batch=5, info=INFO):
        return L.cap_dcholupdate_batched(uplo, sign, n, k, R, ldr, stride_r, V, ldv, stride_v, batch, info, None)
    return call


def test_fixed_size_arguments_are_checked_first(L):
    call = fixed(L)
    n = 10
    # 1. sign, n, k, batch
    for sign in (0, 2, -2, 255):
        assert call(sign=sign) == ARG
        assert call(sign=sign, uplo=LOWER) == ARG                      # before LOWER ...
        assert call(sign=sign, n=257, ldr=257, ldv=257, stride_r=257 * 257, stride_v=257 * 3) == ARG       # ... before the size limit ...
        assert call(sign=sign, batch=0) == ARG and call(sign=sign, k=0) == ARG and call(sign=sign, n=0) == ARG   # ... and the empty case
    assert call(n=-1) == ARG and call(k=-1) == ARG and call(batch=-1) == ARG
    assert call(n=-1, uplo=LOWER) == ARG and call(k=-1, batch=0) == ARG
    # 2. pointers, leading dimensions, strides - with n k batch > 0 only
    assert call(R=None) == ARG and call(V=None) == ARG
    assert call(ldr=n - 1) == ARG and call(ldv=n - 1) == ARG
    assert call(stride_r=n * n - 1) == ARG and call(stride_v=n * 3 - 1) == ARG
    assert call(ldr=n + 2, stride_r=(n + 2) * n - 1) == ARG and call(ldv=n + 2, stride_v=(n + 2) * 3 - 1) == ARG
    assert call(stride_r=-1) == ARG and call(stride_v=-1) == ARG
    assert call(n=16, ldr=1 << 60, stride_r=0, ldv=16, stride_v=48, batch=2) == ARG          # ld * n = 2^64 does not wrap to 0
    assert call(stride_r=0, stride_v=0, batch=1, uplo=LOWER) == UNSUPPORTED       # one block needs no stride ...
    assert call(stride_r=0, batch=2, uplo=LOWER) == ARG and call(stride_v=0, batch=2, uplo=LOWER) == ARG   # ... two do
    assert call(R=None, uplo=LOWER) == ARG and call(ldv=n - 1, uplo=LOWER) == ARG
    assert call(n=257, ldr=256, ldv=257, stride_r=257 * 257, stride_v=257 * 3) == ARG          # the argument rules come first
    assert call(n=257, ldr=257, ldv=256, stride_r=257 * 257, stride_v=257 * 3) == ARG
    # 3. LOWER, 4. n > 256, 5. the grid
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7) == UNSUPPORTED
    assert call(uplo=LOWER, n=0) == UNSUPPORTED and call(uplo=LOWER, k=0) == UNSUPPORTED and call(uplo=LOWER, batch=0) == UNSUPPORTED
    assert call(n=257, ldr=257, ldv=257, stride_r=257 * 257, stride_v=257 * 3) == UNSUPPORTED
    assert call(n=1 << 20, ldr=1 << 20, ldv=1 << 20, stride_r=1 << 40, stride_v=1 << 22) == UNSUPPORTED
    assert call(n=257, ldr=257, ldv=257, stride_r=0, stride_v=0, batch=0) == UNSUPPORTED       # for an empty batch too
    assert call(n=257, k=0, ldr=0, ldv=0) == UNSUPPORTED
    assert call(n=65, ldr=65, ldv=65, stride_r=65 * 65, stride_v=65 * 3, batch=1 << 31) == UNSUPPORTED
    assert call(n=65, ldr=64, ldv=65, stride_r=65 * 65, stride_v=65 * 3, batch=1 << 31) == ARG
    assert call(n=65, ldr=65, ldv=65, stride_r=65 * 65, stride_v=65 * 3, batch=1 << 31, k=0) == UNSUPPORTED    # before the empty case
    # 6. nothing to do: no launch, whatever the pointers
    assert call(n=0, R=None, V=None, ldr=0, ldv=0, stride_r=0, stride_v=0, info=None) == OK
    assert call(k=0, R=None, V=None, ldr=0, ldv=0, stride_r=-5, stride_v=-5, info=None) == OK
    assert call(batch=0, R=None, V=None, stride_r=-5, info=None) == OK
    assert call(n=0) == OK and call(k=0) == OK and call(batch=0) == OK
    assert call(sign=-1, batch=0) == OK
    for big in (64, 65, 256):
        kw = dict(n=big, ldr=big, ldv=big, stride_r=big * big, stride_v=big * 3)
        assert call(batch=0, **kw) == OK and call(batch=0, R=None, V=None, **kw) == OK
        assert call(**dict(kw, ldr=big - 1)) == ARG and call(**dict(kw, stride_v=big * 3 - 1)) == ARG
        assert call(R=None, **kw) == ARG and call(uplo=LOWER, **kw) == UNSUPPORTED


def create(L, n):
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(len(n), arr(n), None, None, C.byref(p)) == OK
    return p


def test_plan_entry_arguments_are_checked_first(L):
    """no call here reaches a launch: in a process without a device the accepted calls on a non-empty plan would end in CAP_ERR_HIP"""
    p, p0, p1 = create(L, [5, 0, 100]), create(L, [0, 0, 0]), create(L, [])

    def call(p=p, uplo=UPPER, sign=1, k=3, R=R, V=V, ldv=1 << 20, info=INFO):
        return L.cap_dcholupdate_vbatched(p, uplo, sign, k, R, V, ldv, info, None)
    assert call(p=None) == ARG and call(p=None, uplo=LOWER) == ARG
    for sign in (0, 2, -3):
        assert call(sign=sign) == ARG and call(sign=sign, uplo=LOWER) == ARG and call(sign=sign, p=p0) == ARG and call(sign=sign, k=0) == ARG
    assert call(k=-1) == ARG and call(k=-1, uplo=LOWER) == ARG and call(k=-1, p=p1) == ARG
    assert call(R=None) == ARG and call(V=None) == ARG and call(R=None, uplo=LOWER) == ARG
    assert call(ldv=104) == ARG and call(ldv=104, uplo=LOWER) == ARG and call(ldv=104, k=0) == ARG      # sum n_i = 105
    assert call(ldv=105, uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7) == UNSUPPORTED
    assert call(k=0) == OK and call(k=0, R=None, V=None, ldv=105, info=None) == OK
    assert call(k=0, uplo=LOWER) == UNSUPPORTED
    for q in (p0, p1):                                                 # nothing to launch: pointers may be NULL, LOWER is still refused
        assert call(p=q, R=None, V=None, info=None, ldv=0) == OK and call(p=q) == OK and call(p=q, sign=-1) == OK
        assert call(p=q, uplo=LOWER) == UNSUPPORTED
        assert call(p=q, ldv=-1) == ARG
    for q in (p, p0, p1):
        L.cap_vbatch_plan_destroy(q)


def test_header_declares_both_symbols_with_the_ctypes_signatures(L):
    from capital_amd import _lib
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in ("cap_dcholupdate_batched", "cap_dcholupdate_vbatched"):
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name + " is not declared"
        want = []
        for a in m.group(1).replace("\n", " ").split(","):
            a = a.strip()
            want.append(C.c_void_p if "*" in a else kinds[a.replace("const ", "").split()[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and list(args) == want, (name, args, want)
        assert getattr(L, name).argtypes == want
    for s in ("THE BIT CONTRACT", "INPUT AND OUTPUT", "csrc/chud_step.h", "plain store"):
        assert s in header[header.index("csrc/cholupdate_batched.hip"):], s


def test_python_layer_names():
    from capital_amd import _lib, batched, lapack
    pu = lapack.ArgPack_cholupdate_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    pv = lapack.ArgPack_cholupdate_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    assert pu.method == lapack.Method.AlapackCholupdateBatched and pv.method == lapack.Method.AlapackCholupdateVbatched
    assert len({int(m) for m in lapack.Method}) == len(list(lapack.Method))
    assert callable(lapack.engine._cholupdate_batched) and callable(lapack.engine._cholupdate_vbatched)
    for fn in (batched.update, batched.downdate, batched.VarBatch.update, batched.VarBatch.downdate):
        assert callable(fn) and "LOWER triangle" in fn.__doc__ and "L' L'^T" in fn.__doc__
    assert "256" in lapack.engine._cholupdate_batched.__doc__ and "256" in lapack.engine._cholupdate_vbatched.__doc__
    with pytest.raises(_lib.CapitalError, match="256"):
        lapack.engine._cholupdate_batched(None, None, 257, 1, 257, 257 * 257, 257, 257, 1, 1, None, pu)


def test_cpu_tensors_wrong_types_and_shapes_are_refused():
    import torch
    from capital_amd import _lib, batched
    r = torch.eye(10, dtype=torch.float64).repeat(3, 1, 1)
    v = torch.zeros(3, 2, 10, dtype=torch.float64)
    vb = batched.VarBatch([3, 5])
    flat = torch.zeros(vb.total, dtype=torch.float64)
    for fn in (batched.update, batched.downdate):
        for bad in (lambda: fn(r, v), lambda: fn(r.to(torch.float32), v), lambda: fn(torch.eye(4, dtype=torch.float64), v), lambda: fn(None, v)):
            with pytest.raises(_lib.CapitalError):
                bad()
    for fn in (vb.update, vb.downdate):
        for bad in (lambda: fn(flat, torch.zeros(8, dtype=torch.float64)), lambda: fn(flat.to(torch.float32), torch.zeros(8, dtype=torch.float64)),
                    lambda: fn(None, None)):
            with pytest.raises(_lib.CapitalError):
                bad()


def test_one_annotated_launch_per_call_and_class_on_the_recording_stand_in(tmp_path):
    """the fixed-size entry at n = 8, 64, 65, 256 with k = 1 and 17, the plan entry on four size lists, the caller on the NULL stream and
    on a stream of its own"""
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
        assert all(k.startswith("K ") and "chud_" in k and "batched" in k for k in x["launches"]), x["launches"]
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
            r = S.Run("cholupdate batched n=%d%s" % (n, tag), user_stream)
            batch, ldr, ldv, kmax = 37, n + 1, n + 2, max(TRACE_K)
            Rd, Vd = S.dmalloc(8 * (ldr * n + 3) * batch), S.dmalloc(8 * (ldv * kmax + 5) * batch)
            info = S.dmalloc(4 * batch)
            calls = 0
            for k in TRACE_K:
                for sign, inf, sr, sv in ((1, info, ldr * n, ldv * k), (-1, None, ldr * n + 3, ldv * k + 5)):
                    S.ok(r.call("dcholupdate_batched k=%d sign=%d" % (k, sign), S.L.cap_dcholupdate_batched, 1, sign, n, k, Rd, ldr, sr, Vd, ldv, sv,
                                batch, inf, r.stream), "cap_dcholupdate_batched")
                    calls += 1
                S.ok(r.call("dcholupdate_batched k=%d one block" % k, S.L.cap_dcholupdate_batched, 1, 1, n, k, Rd, ldr, 0, Vd, ldv, 0, 1, None,
                            r.stream), "cap_dcholupdate_batched")
                calls += 1
            for c in (("empty k=0", 1, 1, n, 0, Rd, ldr, ldr * n, Vd, ldv, 0, batch, info), ("empty batch=0", 1, -1, n, 1, None, ldr, 0, None, ldv, 0, 0, None),
                      ("empty n=0", 1, 1, 0, 1, None, 0, 0, None, 0, 0, batch, None)):
                S.ok(r.call(c[0], S.L.cap_dcholupdate_batched, *c[1:], r.stream), c[0])
            out = r.finish()
            out["expected"], out["per_launches"] = calls, 1
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Rd, Vd, info):
                S.shim.hipFree(q)
            results.append(out)
        for name in TRACE_LISTS:
            lay = VC.Layout(VC.LISTS[name], "gaps")
            plan, empty = C.c_void_p(), C.c_void_p()
            S.ok(S.L.cap_vbatch_plan_create(lay.batch, arr(list(lay.sizes)), None, arr(list(lay.off_arg)), C.byref(plan)), "cap_vbatch_plan_create")
            S.ok(S.L.cap_vbatch_plan_create(3, arr([0, 0, 0]), None, None, C.byref(empty)), "cap_vbatch_plan_create")
            r = S.Run("cholupdate vbatched %s%s" % (name, tag), user_stream)
            ldv = lay.rows + 2
            Rd, Vd, info = S.dmalloc(8 * lay.total), S.dmalloc(8 * ldv * max(TRACE_K)), S.dmalloc(4 * lay.batch)
            calls = [("dcholupdate_vbatched k=%d sign=%d" % (k, sign), S.L.cap_dcholupdate_vbatched, plan, 1, sign, k, Rd, Vd, ldv, inf, r.stream)
                     for k in TRACE_K for sign, inf in ((1, info), (-1, None))]
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty plan", S.L.cap_dcholupdate_vbatched, empty, 1, 1, 3, None, None, 0, None, r.stream),
                      ("empty k=0", S.L.cap_dcholupdate_vbatched, plan, 1, -1, 0, None, None, ldv, None, r.stream)):
                S.ok(r.call(*c), c[0])
            out = r.finish()
            classes = int(S.L.cap_vbatch_plan_info(plan, 4))
            assert classes >= 1
            out["expected"], out["per_launches"] = len(calls) * classes, classes
            out["launches"] = [l for l in r.lines if l.startswith("K ")]
            out["per_call"], out["empty_calls"] = _marks(r)
            for q in (Rd, Vd, info):
                S.shim.hipFree(q)
            S.ok(S.L.cap_vbatch_plan_destroy(plan), "cap_vbatch_plan_destroy")
            S.ok(S.L.cap_vbatch_plan_destroy(empty), "cap_vbatch_plan_destroy")
            results.append(out)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
