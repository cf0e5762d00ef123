"""TEST INFRASTRUCTURE: every row of tests/chol_cases.py through the library's own object files on the recording stand-in.

    python tests/hipshim/run_chol.py out.json          # what tests/test_chol_cases.py starts
    python tests/hipshim/run_chol.py --table           # the row -> kernel table (profiles/r19_chol_exact.txt)

Per row: the status of cap_cholinv_factor (+ cap_cholinv_get_R / get_Rinv / info) or cap_dpotrf, the launches the FIRST factor call made
(the stand-in's `K` trace lines: the launches per kernel of leaf_cholinv_kernel / panel64_solve_update_kernel / chain64_coop_kernel /
trinv_merge_kernel<RBW>, the folded and `direct` forms of panel64_solve_update_kernel from its grids, the dgemm_* instances, and from the
run-time modes the CPU models log how many products read their C input from another matrix and the K of each), the plan's count_paired,
and whether the CPU models' result equals the exact reference bit for bit (-0.0 = +0.0 in outputs) with every NaN of the buffers where it
was: the strictly lower triangle and the pad rows of A, cap_dpotrf's `work` (all NaN, exactly cap_dpotrf_work_size long, with a NaN
sentinel behind it).  The stand-in hands out all-NaN allocations, so a model that reads plan scratch nobody wrote shows as well.  All
rows run in compute mode.  Also lists every registered kernel name of the family.  Its own process (no torch)."""
import collections
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import run_scenarios as rs          # noqa: E402  (builds and loads the libraries, installs the access hook)
from run_blas3 import short, text_of   # noqa: E402
from run_tri import upload, download   # noqa: E402
from tests import chol_cases as T    # noqa: E402
from tests.blas3_cases import place, same_bits, describe_mismatch   # noqa: E402

L, shim = rs.L, rs.shim
shim.shim_set_compute.argtypes = [C.c_int]
shim.shim_unmodelled.restype = C.c_longlong
for f in (shim.shim_kernel_names, shim.shim_gemm_modes):
    f.restype, f.argtypes = C.c_longlong, [C.c_char_p, C.c_longlong]

SENTINEL = 4096


def registered():
    return sorted({short(n) for n in text_of(shim.shim_kernel_names).split() if any(w in n for w in T.FAMILY)})


def launches():
    path = os.path.join(rs.build_shim.OUT, "trace_chol_%d.txt" % os.getpid())
    shim.shim_dump(path.encode())
    lines = open(path).read().splitlines()
    os.unlink(path)
    bad = [l for l in lines if l.split()[0] in ("OOB", "ORPHAN", "BADLAUNCH", "UNMODELLED", "BADFREE")]
    k = [l.split() for l in lines if l.startswith("K ")]
    fam = [(short(x[2]), int(x[3])) for x in k if any(w in x[2] for w in T.FAMILY)]
    modes = [dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in l.split()) for l in text_of(shim.shim_gemm_modes).splitlines()]
    return {"kernels": dict(sorted(collections.Counter(n for n, _ in fam).items())),
            "panel_grids": sorted({g for n, g in fam if n == T.PANEL}),
            "gemm_names": dict(sorted(collections.Counter(short(x[2]) for x in k if "dgemm_" in x[2]).items())),
            "gemms": sum(1 for x in k if "dgemm_" in x[2]),
            "cin": sum(m["cin"] for m in modes), "ks": sorted({m["k"] for m in modes}), "ksplit": max([m["ksplit"] for m in modes] or [1])}, bad


def run_plan(c):
    detail = []
    n, lda = c.n, c.n + c.pad
    plan = T.create_plan(L, c)
    out = rs.dmalloc(8 * n * n)
    seen, st = None, 0
    for second in ((False, True) if c.second else (False,)):
        host = place(T.operand(c, second), lda)
        A = upload(host)
        shim.shim_reset(); text_of(shim.shim_gemm_modes)
        st = st or int(L.cap_cholinv_factor(plan, A, lda, None))
        info = T.plan_info(L, plan)
        if seen is None:
            seen, bad = launches()
            seen["paired"] = int(L.cap_cholinv_get_option(plan, b"count_paired"))
            detail += bad
        if c.pivot is not None:
            if info != c.pivot + 1:
                detail.append("info = %d, expected %d" % (info, c.pivot + 1))
        else:
            if info != 0:
                detail.append("info = %d" % info)
            R, Rinv = T.references(c, second)
            st = st or int(L.cap_cholinv_get_R(plan, out, n, None))
            got = T.positive_zero(download(out, n * n))
            if not same_bits(got, place(R, n)):
                detail.append("R%s: %s" % (" (second)" if second else "", describe_mismatch(got, place(R, n), n)))
            if Rinv is not None:
                st = st or int(L.cap_cholinv_get_Rinv(plan, out, n, None))
                got = T.positive_zero(download(out, n * n))
                if not same_bits(got, place(Rinv, n)):
                    detail.append("Rinv%s: %s" % (" (second)" if second else "", describe_mismatch(got, place(Rinv, n), n)))
        if not same_bits(download(A, host.size), host):
            detail.append("the input A changed")
        shim.hipFree(A)
    L.cap_cholinv_plan_destroy(plan)
    shim.hipFree(out)
    seen.update(status=st, exact=not detail, detail=detail)
    return seen


def run_dpotrf(c):
    detail = []
    n, lda = c.n, c.n + c.pad
    ws = int(L.cap_dpotrf_work_size(n))
    host = place(T.operand(c), lda)
    A, work, info = upload(host), upload(np.full(ws + SENTINEL, T.NAN)), rs.dmalloc(8)
    shim.shim_reset(); text_of(shim.shim_gemm_modes)
    st = int(L.cap_dpotrf(T.UPPER, n, A, lda, info, work, None))
    seen, bad = launches()
    seen["paired"] = 0
    got, want = T.positive_zero(download(A, host.size)), T.positive_zero(place(T.dpotrf_reference(c), lda))
    if not same_bits(got, want):
        detail.append("A: %s" % describe_mismatch(got, want, lda))
    if C.c_int.from_address(info.value).value != 0:
        detail.append("info = %d" % C.c_int.from_address(info.value).value)
    if not same_bits(download(work, ws + SENTINEL)[ws:], np.full(SENTINEL, T.NAN)):
        detail.append("the sentinel behind the work buffer changed")
    for p in (A, work, info):
        shim.hipFree(p)
    seen.update(status=st, work=ws, exact=not detail, detail=detail + bad)
    return seen


def table(results):
    out = ["%-58s %-62s %5s %3s %3s  %s" % ("row", "launches of the family", "GEMMs", "Cin", "K2", "why")]
    for c in T.CASES:
        r = results[c.id]
        text = " + ".join("%s x %d" % (k.replace("_kernel", ""), v) for k, v in r["kernels"].items())
        out.append("%-58s %-62s %5d %3d %3d  %s" % (c.id, text, r["gemms"], r["cin"], r["paired"], c.why))
    return "\n".join(out)


def main(argv):
    want_table = "--table" in argv
    paths = [a for a in argv if not a.startswith("--")]
    only = os.environ.get("SHIM_FILTER", "")
    results = {}
    shim.shim_set_compute(1)
    for c in T.CASES:
        if only and only not in c.id:
            continue
        try:
            results[c.id] = run_plan(c) if c.entry == "plan" else run_dpotrf(c)
        except Exception as e:      # a refused call or a crash of the host side is a finding of that row
            results[c.id] = {"kernels": {}, "panel_grids": [], "gemm_names": {}, "gemms": -1, "cin": -1, "ks": [], "ksplit": 1, "paired": -1, "status": -1, "exact": False,
                             "detail": ["exception: %r" % (e,)]}
        if only:
            print(c.id, json.dumps(results[c.id]), "| expected", c.kernels, c.gemms, c.cin, c.k2)
    shim.shim_set_compute(0)
    out = {"registered": registered(), "unmodelled": int(shim.shim_unmodelled()), "cases": results}
    if paths:
        json.dump(out, open(paths[0], "w"), indent=1)
    if want_table and not only:
        print(table(results))
    print("%d rows, %d findings" % (len(results), sum(1 for r in results.values() if r["exact"] is False or r["status"] != 0 or r["detail"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
