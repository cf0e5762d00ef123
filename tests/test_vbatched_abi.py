"""CPU-only: argument handling of the variable-size batched Cholesky (cap_vbatch_plan_create / _destroy / _info / _table, cap_dpotrf_vbatched,
cap_dpotrs_vbatched, cap_dpotri_vbatched) - the argument rules of include/capital_amd.h in their order, every case decided before the
library touches a device - and the Python names.  The last test drives the three entries through the recording stand-in of tests/hipshim
in a process of its own (this file run as a script): one launch per non-empty class and call, every launch annotated, no finding, and
nothing but launches inside a call."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, HIP, UNSUPPORTED = 0, 1, 2, 4
TRACE_LISTS = ("EVERY", "WAVES", "EDGES", "LONE1", "LONE256", "ONE_CLASS")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


A = C.c_void_p(1 << 20)                  # never dereferenced: every call below returns before any device work
B = C.c_void_p(1 << 24)
INFO = C.c_void_p(1 << 31)


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*a)


def create(L, n, ld=None, off=None, batch=None):
    p = C.c_void_p()
    st = L.cap_vbatch_plan_create(len(n) if batch is None else batch, arr(n), arr(ld), arr(off), C.byref(p))
    assert (p.value is not None) == (st == OK)
    return st, p


def refused(L, *a, **k):
    st, p = create(L, *a, **k)
    if st == OK:
        L.cap_vbatch_plan_destroy(p)
    return st


def test_plan_arguments_are_checked_first(L):
    assert refused(L, [3, 4]) == OK
    assert L.cap_vbatch_plan_create(1, arr([3]), None, None, None) == ARG
    assert refused(L, [3], batch=-1) == ARG
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(2, None, None, None, C.byref(p)) == ARG and p.value is None
    assert refused(L, [3, -1]) == ARG
    assert refused(L, [3, 4], ld=[3, 3]) == ARG
    assert refused(L, [3, 4], ld=[3, 4]) == OK
    assert refused(L, [3, 0], ld=[3, 0]) == OK                         # an empty block needs no leading dimension
    assert refused(L, [3, 4], off=[0, -1]) == ARG
    assert refused(L, [257]) == UNSUPPORTED
    assert refused(L, [3, 257, 4]) == UNSUPPORTED
    assert refused(L, [1 << 40]) == UNSUPPORTED
    assert refused(L, [257, -1]) == ARG                                # the argument rules come first ...
    assert refused(L, [257, 4], ld=[257, 3]) == ARG
    assert refused(L, [257, 4], ld=[256, 4]) == ARG
    assert refused(L, [257, 4], off=[0, 10]) == ARG                    # ... the overlap among them
    assert refused(L, [257, 4], off=[0, 257 * 257]) == UNSUPPORTED
    assert L.cap_vbatch_plan_destroy(None) == OK


def test_overlapping_blocks_are_refused(L):
    assert refused(L, [3, 3], off=[0, 9]) == OK
    assert refused(L, [3, 3], off=[0, 8]) == ARG
    assert refused(L, [3, 3], off=[9, 0]) == OK                        # any order
    assert refused(L, [3, 3], off=[8, 0]) == ARG
    assert refused(L, [3, 3], off=[5, 5]) == ARG                       # equal offsets
    assert refused(L, [3, 0, 3], off=[5, 5, 14]) == OK                 # an empty block lies nowhere
    assert refused(L, [0, 0], off=[5, 5]) == OK
    assert refused(L, [3, 3], ld=[5, 3], off=[0, 12]) == ARG           # the last column of a block ends after n rows, not after ld
    assert refused(L, [3, 3], ld=[5, 3], off=[0, 13]) == OK
    assert refused(L, [4, 1], ld=[8, 1], off=[0, 5]) == ARG            # a block inside another one's padding rows
    assert refused(L, [4, 1], ld=[8, 1], off=[0, 28]) == OK
    assert refused(L, [4, 2, 5], off=[100, 0, 50]) == OK
    assert refused(L, [4, 2, 60], off=[100, 0, 50]) == ARG
    assert refused(L, [200, 3], off=[0, 200 * 199 + 199]) == ARG       # the last element of the window
    assert refused(L, [200, 3], off=[0, 200 * 199 + 200]) == OK


def test_defaults_and_info(L):
    st, p = create(L, [3, 0, 70, 9])
    assert st == OK
    info = lambda w: L.cap_vbatch_plan_info(p, w)
    assert [info(w) for w in range(5)] == [4, 9 + 4900 + 81, 82, 70, 3]
    assert [info(5 + c) for c in range(7)] == [1, 1, 0, 0, 1, 0, 0]
    buf = (C.c_int64 * 4)()
    assert L.cap_vbatch_plan_table(p, 4, buf, 4) == OK and buf[0] == 2
    assert L.cap_vbatch_plan_table(p, 7, buf, 4) == ARG and L.cap_vbatch_plan_table(p, -1, buf, 4) == ARG
    assert L.cap_vbatch_plan_table(p, 0, None, 1) == ARG and L.cap_vbatch_plan_table(p, 0, None, 0) == OK
    assert L.cap_vbatch_plan_table(p, 0, buf, -1) == ARG and L.cap_vbatch_plan_table(None, 0, buf, 1) == ARG
    assert L.cap_vbatch_plan_info(None, 0) == -1
    L.cap_vbatch_plan_destroy(p)
    st, p = create(L, [3, 0, 70, 9], ld=[5, 0, 70, 12])                # offsets from the leading dimensions
    assert L.cap_vbatch_plan_info(p, 1) == 15 + 4900 + 8 * 12 + 9
    L.cap_vbatch_plan_destroy(p)


def entries(L, p):
    def potrf(p=p, uplo=UPPER, A=A, info=INFO, nrhs=1, ldb=1 << 20, fill=0):
        return L.cap_dpotrf_vbatched(p, uplo, A, info, None, None)

    def potrs(p=p, uplo=UPPER, A=A, info=INFO, nrhs=1, ldb=1 << 20, fill=0, Bp=B):
        return L.cap_dpotrs_vbatched(p, uplo, nrhs, A, Bp, ldb, info, None)

    def potri(p=p, uplo=UPPER, A=A, info=INFO, nrhs=1, ldb=1 << 20, fill=0):
        return L.cap_dpotri_vbatched(p, uplo, A, info, fill, None)
    return potrf, potrs, potri


@pytest.mark.parametrize("which", (0, 1, 2))
def test_entry_arguments_are_checked_first(L, which):
    """on a plan that has launches to make; no call here reaches one: in a process without a device the accepted calls would end in
    CAP_ERR_HIP, so every accepted case below is an empty one"""
    st, p = create(L, [5, 0, 100])
    st0, p0 = create(L, [0, 0, 0])
    st1, p1 = create(L, [])
    assert st == st0 == st1 == OK
    call = entries(L, p)[which]
    assert call(p=None) == ARG
    assert call(p=None, uplo=LOWER) == ARG
    assert call(A=None) == ARG
    assert call(A=None, uplo=LOWER) == ARG
    assert call(uplo=LOWER) == UNSUPPORTED
    assert call(uplo=7) == UNSUPPORTED
    for q in (p0, p1):                                                 # nothing to launch: pointers may be NULL, LOWER is still refused
        assert call(p=q, A=None, info=None) == OK
        assert call(p=q) == OK
        assert call(p=q, uplo=LOWER) == UNSUPPORTED
    if which == 1:
        assert call(nrhs=-1) == ARG
        assert call(nrhs=-1, uplo=LOWER) == ARG
        assert call(ldb=104) == ARG                                    # sum n_i = 105
        assert call(ldb=104, uplo=LOWER) == ARG
        assert call(ldb=104, nrhs=0) == ARG
        assert call(ldb=105, uplo=LOWER) == UNSUPPORTED
        assert call(Bp=None) == ARG
        assert call(nrhs=0) == OK and call(nrhs=0, A=None, Bp=None, ldb=105) == OK
        assert call(nrhs=0, uplo=LOWER) == UNSUPPORTED
        assert call(p=p0, ldb=-1) == ARG and call(p=p0, ldb=0, A=None, Bp=None) == OK
    if which == 2:
        for fill in (2, -1, 255):
            assert call(fill=fill) == ARG
            assert call(fill=fill, uplo=LOWER) == ARG                  # before LOWER
            assert call(fill=fill, p=p0) == ARG                        # and before the empty case
        assert call(fill=1, uplo=LOWER) == UNSUPPORTED and call(fill=1, p=p0) == OK
    for q in (p, p0, p1):
        L.cap_vbatch_plan_destroy(q)


def test_python_layer_names():
    from capital_amd import _lib, batched, lapack
    packs = [f(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
             for f in (lapack.ArgPack_potrf_vbatched, lapack.ArgPack_potrs_vbatched, lapack.ArgPack_potri_vbatched)]
    assert [p.method for p in packs] == [lapack.Method.AlapackPotrfVbatched, lapack.Method.AlapackPotrsVbatched, lapack.Method.AlapackPotriVbatched]
    assert len({int(m) for m in lapack.Method}) == len(list(lapack.Method))
    for fn in (lapack.engine._potrf_vbatched, lapack.engine._potrs_vbatched, lapack.engine._potri_vbatched):
        assert callable(fn) and "256" in fn.__doc__
    vb = batched.VarBatch([3, 0, 70, 9])
    assert (vb.offsets, vb.row_offsets, vb.total, vb.rows, vb.launches) == ((0, 9, 9, 4909), (0, 3, 3, 73), 4990, 82, 3)
    for name in ("potrf", "potrs", "potri", "block", "pack"):
        assert callable(getattr(vb, name))
    assert "LOWER triangle" in vb.potrf.__doc__ and "LOWER triangle" in vb.block.__doc__ and "torch.cholesky_inverse" in vb.potri.__doc__
    assert "synchronise" in batched.VarBatch.__doc__
    for bad in ([3, 257], [3, -1]):
        with pytest.raises(_lib.CapitalError):
            batched.VarBatch(bad)
    with pytest.raises(_lib.CapitalError):
        batched.VarBatch([3, 3], offsets=[0, 8])
    with pytest.raises(_lib.CapitalError):
        batched.VarBatch([3, 3], ld=[3])
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    for s in ("cap_vbatch_plan_create(", "cap_dpotrf_vbatched(", "cap_dpotrs_vbatched(", "cap_dpotri_vbatched(", "THE BIT CONTRACT", "MAY SYNCHRONISE"):
        assert s in header, s


def test_cpu_tensors_wrong_types_and_shapes_are_refused():
    import torch
    from capital_amd import _lib, batched
    vb = batched.VarBatch([3, 5])
    a = torch.zeros(vb.total, dtype=torch.float64)
    for call in (lambda: vb.potrf(a), lambda: vb.potri(a), lambda: vb.potrs(a, torch.zeros(8, dtype=torch.float64)),
                 lambda: vb.potrf(a.to(torch.float32)), lambda: vb.potrf(a[:-1]), lambda: vb.potrf(a.reshape(2, -1)),
                 lambda: vb.potrf(None), lambda: vb.pack([torch.zeros(3, 3)]), lambda: vb.pack([torch.zeros(3, 3), torch.zeros(4, 4)])):
        with pytest.raises(_lib.CapitalError):
            call()
    if torch.cuda.is_available():
        d = torch.zeros(vb.total, dtype=torch.float64, device="cuda")
        for bad in (torch.zeros(7, dtype=torch.float64, device="cuda"), torch.zeros(8, 2, dtype=torch.float64, device="cuda"),
                    torch.zeros(8, dtype=torch.float32, device="cuda"), torch.zeros(8, dtype=torch.float64),
                    torch.zeros(2, 16, dtype=torch.float64, device="cuda")[:, ::2]):
            with pytest.raises(_lib.CapitalError):
                vb.potrs(d, bad)
        with pytest.raises(_lib.CapitalError):
            vb.potrf(d[:-1])


def test_one_annotated_launch_per_class_on_the_recording_stand_in(tmp_path):
    """the three entries on the lists of TRACE_LISTS in two layouts, the caller on the NULL stream and on a stream of its own"""
    from capital_amd import build
    build.build(verbose=False)
    out = tmp_path / "trace.json"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    res = json.load(open(out))
    assert len(res) == 2 * 2 * len(TRACE_LISTS)
    for x in res:
        assert not x["findings"], (x["name"], x["findings"][:4])
        assert x["classes"] >= 1
        assert x["stats"]["kernels"] == x["calls"] * x["classes"] and not x["stats"].get("unannotated"), (x["name"], x["stats"])
        assert x["stats"]["oob"] == 0 and x["stats"].get("races", 0) == 0
        assert sorted(x["entries"]) == ["cap_dpotrf_vbatched", "cap_dpotri_vbatched", "cap_dpotrs_vbatched"]
        assert all(k.startswith("K ") and "vbatched" in k for k in x["launches"]), x["launches"]
        for name, lines in x["per_call"]:
            assert len(lines) == x["classes"] and all(l.startswith("K ") for l in lines), (x["name"], name, lines)   # launches and nothing else
        assert x["empty_calls"] == []


def _trace_main(out_path):
    """runs in a process of its own (no torch: the stand-in takes the place of the HIP runtime)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipshim"))
    sys.path.insert(0, ROOT)
    import run_scenarios as S
    from tests import vbatched_cases as V
    results = []
    for user_stream in (0, 1):
        for name in TRACE_LISTS:
            for kind in ("packed", "gaps"):
                lay = V.Layout(V.LISTS[name], kind)
                plan = C.c_void_p()
                S.ok(S.L.cap_vbatch_plan_create(lay.batch, arr(list(lay.sizes)), arr(None if lay.ld_arg is None else list(lay.ld_arg)),
                                                arr(None if lay.off_arg is None else list(lay.off_arg)), C.byref(plan)), "cap_vbatch_plan_create")
                empty = C.c_void_p()
                S.ok(S.L.cap_vbatch_plan_create(3, arr([0, 0, 0]), None, None, C.byref(empty)), "cap_vbatch_plan_create")
                r = S.Run("vbatched %s %s%s" % (name, kind, " [user stream]" if user_stream else " [NULL stream]"), user_stream)
                ldb = lay.rows + 2
                Ad, Bd = S.dmalloc(8 * lay.total), S.dmalloc(8 * ldb * 33)
                info, logdet = S.dmalloc(4 * lay.batch), S.dmalloc(8 * lay.batch)
                calls = [("dpotrf_vbatched", S.L.cap_dpotrf_vbatched, plan, 1, Ad, info, logdet, r.stream),
                         ("dpotrf_vbatched no info", S.L.cap_dpotrf_vbatched, plan, 1, Ad, None, None, r.stream)]
                for nrhs in (1, 17, 33):
                    calls.append(("dpotrs_vbatched nrhs=%d" % nrhs, S.L.cap_dpotrs_vbatched, plan, 1, nrhs, Ad, Bd, ldb, info, r.stream))
                for fill, inf in ((0, info), (1, None)):
                    calls.append(("dpotri_vbatched fill=%d" % fill, S.L.cap_dpotri_vbatched, plan, 1, Ad, inf, fill, r.stream))
                for c in calls:
                    S.ok(r.call(*c), c[0])
                for c in (("empty dpotrf_vbatched", S.L.cap_dpotrf_vbatched, empty, 1, None, None, None, r.stream),
                          ("empty dpotrs_vbatched", S.L.cap_dpotrs_vbatched, plan, 1, 0, None, None, ldb, None, r.stream),
                          ("empty dpotri_vbatched", S.L.cap_dpotri_vbatched, empty, 1, None, None, 1, r.stream)):
                    S.ok(r.call(*c), c[0])
                out = r.finish()
                out["calls"] = len(calls)
                out["classes"] = int(S.L.cap_vbatch_plan_info(plan, 4))
                out["launches"] = [l for l in r.lines if l.startswith("K ")]
                per, cur, empties = [], None, []
                for l in r.lines:                  # what the trace holds between the marks of one call
                    if l.startswith("MARK begin "):
                        cur = (l[len("MARK begin "):], [])
                    elif l.startswith("MARK end "):
                        (empties if cur[0].startswith("empty") else per).append(cur)
                        cur = None
                    elif cur is not None and not l.startswith(("ACC ", "A ")):
                        cur[1].append(l)
                out["per_call"] = per
                out["empty_calls"] = [e for e in empties if e[1]]
                for q in (Ad, Bd, info, logdet):
                    S.shim.hipFree(q)
                S.ok(S.L.cap_vbatch_plan_destroy(plan), "cap_vbatch_plan_destroy")
                S.ok(S.L.cap_vbatch_plan_destroy(empty), "cap_vbatch_plan_destroy")
                results.append(out)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
