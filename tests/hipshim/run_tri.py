"""TEST INFRASTRUCTURE: every row of tests/tri_cases.py through the library's own object files on the recording stand-in.

    python tests/hipshim/run_tri.py out.json          # what tests/test_tri_cases.py starts
    python tests/hipshim/run_tri.py --table           # the row -> kernel table (profiles/r16_tri_exact.txt)

Per row: the status of cap_dtrtri / cap_dtrsm / cap_dpotrs / cap_dpotri, the launches it made (the stand-in's `K` trace lines: the names
among leaf_trtri_kernel / potrs_subst_kernel<NR> / potrs_nan_kernel / dlauum_nt_kernel in order with their grids, the number of dgemm_*
and scale_kernel launches) and, in compute mode, whether the CPU models' result equals the exact reference bit for bit (-0.0 = +0.0) with
every NaN of the buffers where it was - `work` is all NaN with a NaN sentinel behind it, so a model that reads scratch nobody wrote
shows.  TRTRI, TRSM and POTRI rows run in compute mode; POTRS rows run in trace mode (names and grids only: potrs_subst_kernel has no CPU
model).  Also lists every registered kernel name of the family and runs the refusals.  Its own process (no torch)."""
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
from tests import tri_cases as T     # noqa: E402
from tests.blas3_cases import place, same_bits, describe_mismatch   # noqa: E402

L, shim = rs.L, rs.shim
shim.shim_set_compute.argtypes = [C.c_int]
shim.shim_unmodelled.restype = C.c_longlong
shim.shim_kernel_names.restype, shim.shim_kernel_names.argtypes = C.c_longlong, [C.c_char_p, C.c_longlong]

FAMILY = ("leaf_trtri_kernel", "potrs_subst_kernel", "potrs_nan_kernel", "dlauum_nt_kernel")
LISTED = ("leaf_trtri_kernel", "potrs_subst_kernel", "potrs_nan_kernel")          # the completeness check of tests/test_tri_cases.py
SENTINEL = 4096


def registered():
    return sorted({short(n) for n in text_of(shim.shim_kernel_names).split() if any(w in n for w in LISTED)})


def upload(flat):
    p = rs.dmalloc(8 * flat.size)
    np.ctypeslib.as_array((C.c_double * flat.size).from_address(p.value))[:] = flat
    return p


def download(p, size):
    return np.ctypeslib.as_array((C.c_double * size).from_address(p.value)).copy()


def launches():
    path = os.path.join(rs.build_shim.OUT, "trace_tri_%d.txt" % os.getpid())
    shim.shim_dump(path.encode())
    lines = open(path).read().splitlines()
    os.unlink(path)
    bad = [l for l in lines if l.split()[0] in ("OOB", "ORPHAN", "BADLAUNCH", "UNMODELLED", "BADFREE")]
    k = [l.split() for l in lines if l.startswith("K ")]
    return {"kernels": [short(x[2]) for x in k if any(w in x[2] for w in FAMILY)],
            "grids": [int(x[3]) for x in k if any(w in x[2] for w in FAMILY)],
            "gemms": sum(1 for x in k if "dgemm_" in x[2]),
            "scales": sum(1 for x in k if "scale_kernel" in x[2] and "unscale" not in x[2]),
            "ops": sum(1 for l in lines if l.split()[0] in ("K", "COPY", "COPY2D", "SET"))}, bad


def run_case(c, compute):
    shim.shim_reset()
    ld = T.lds(c)
    ws = T.work_size(L, c)
    detail = []
    if compute:
        ops = T.operands(c)
        host = {"T": place(T.stored(ops["T"]), ld["T"])}
        if "B" in ops:
            host["B"] = place(ops["B"], ld["B"])
        dev = {name: upload(flat) for name, flat in host.items()}
        work = upload(np.full(c.woff + ws + SENTINEL, T.NAN))
    else:
        cols = c.other if c.op == "potrs" else c.n
        dev = {"T": rs.dmalloc(8 * ld["T"] * c.n), "B": rs.dmalloc(8 * ld["B"] * cols)}
        work = rs.dmalloc(8 * (c.woff + ws + SENTINEL))
    st = T.call(L, c, dev["T"], dev.get("B"), C.c_void_p(work.value + 8 * c.woff), ld)
    seen, bad = launches()
    if compute:
        out = "T" if c.op in ("trtri", "potri") else "B"
        want = dict(host)
        want[out] = place(T.reference(c, ops), ld[out])
        for name in host:
            got = T.positive_zero(download(dev[name], host[name].size)) if name == out else download(dev[name], host[name].size)
            exp = T.positive_zero(want[name]) if name == out else want[name]
            if not same_bits(got, exp):
                detail.append("%s: %s" % (name, describe_mismatch(got, exp, ld[name])))
        if not same_bits(download(work, c.woff + ws + SENTINEL)[c.woff + ws:], np.full(SENTINEL, T.NAN)):
            detail.append("the sentinel behind the work buffer changed")
    for p in list(dev.values()) + [work]:
        shim.hipFree(p)
    seen.update(status=int(st), work=ws, exact=(not detail) if compute else None, detail=detail + bad)
    return seen


def run_refusals():
    n, ld = T.REFUSAL_N, T.REFUSAL_N + 2
    out = []
    for entry, what, want in T.REFUSALS:
        shim.shim_reset()
        a, b, work = upload(np.full(ld * n, T.NAN)), upload(np.full(ld * n, T.NAN)), upload(np.full(1 << 16, T.NAN))
        st = T.refusal_call(L, entry, what, a, b, work)
        seen, bad = launches()
        untouched = all(same_bits(download(p, size), np.full(size, T.NAN)) for p, size in ((a, ld * n), (b, ld * n), (work, 1 << 16)))
        for p in (a, b, work):
            shim.hipFree(p)
        out.append({"entry": entry, "what": what, "status": int(st), "want": want, "launches": seen["ops"], "untouched": untouched, "detail": bad})
    return out


def table(results):
    out = ["%-38s %-62s %5s %6s  %s" % ("row", "launches of the family (in order; grids)", "GEMMs", "scales", "why")]
    for c in T.CASES:
        r = results[c.id]
        runs, names = [], r["kernels"]
        for i, (k, g) in enumerate(zip(names, r["grids"])):          # "name x count" for runs of equal launches
            if runs and runs[-1][0] == k and (runs[-1][1] == g or "subst" not in k):
                runs[-1][2] += 1
            else:
                runs.append([k, g, 1])
        text = " + ".join("%s%s%s" % (k, "[%d]" % g if "subst" in k or "lauum" in k else "", " x %d" % cnt if cnt > 1 else "") for k, g, cnt in runs)
        out.append("%-38s %-62s %5d %6d  %s" % (c.id, text, r["gemms"], r["scales"], c.why))
    return "\n".join(out)


def main(argv):
    want_table = "--table" in argv
    paths = [a for a in argv if not a.startswith("--")]
    only = os.environ.get("SHIM_FILTER", "")
    results = {}
    for c in T.CASES:
        if only and only not in c.id:
            continue
        compute = c.op != "potrs"
        shim.shim_set_compute(1 if compute else 0)
        try:
            results[c.id] = run_case(c, compute)
        except Exception as e:      # a refused call or a crash of the host side is a finding of that row
            results[c.id] = {"kernels": [], "grids": [], "gemms": -1, "scales": -1, "ops": -1, "status": -1, "work": -1, "exact": False, "detail": ["exception: %r" % (e,)]}
    shim.shim_set_compute(0)
    out = {"registered": registered(), "unmodelled": int(shim.shim_unmodelled()), "cases": results, "refusals": run_refusals()}
    if paths:
        json.dump(out, open(paths[0], "w"), indent=1)
    if want_table and not only:
        print(table(results))
    bad = sum(1 for r in results.values() if r["exact"] is False or r["status"] != 0 or r["detail"])
    bad += sum(1 for r in out["refusals"] if r["status"] != r["want"] or r["launches"] or not r["untouched"])
    print("%d rows, %d refusals, %d findings" % (len(results), len(out["refusals"]), bad))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
