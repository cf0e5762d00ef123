"""TEST INFRASTRUCTURE: every row of tests/blas3_cases.py through the library's own object files on the recording stand-in.

    python tests/hipshim/run_blas3.py out.json          # what tests/test_blas3_paths.py starts
    python tests/hipshim/run_blas3.py --table           # the case -> kernel instance table (profiles/r11_blas3_paths.txt)

Per row and per (alpha, beta): the device names of the GEMM-family kernels the call launched (the stand-in's `K` trace lines; template
instances have different names), the run-time modes of the tile-kernel launches (GemmArgs fields, logged by the CPU models) and, in
compute mode, whether the CPU models' result equals the exact reference bit for bit with every NaN of the buffers where it was.  The
large-pitch rows run in trace mode: the kernel's name only, no byte of their 4.3 GB operands is touched.  Also lists every kernel name
the object files registered.  Its own process (no torch)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import run_scenarios as rs          # noqa: E402  (builds and loads the libraries, installs the access hook)
from tests import blas3_cases as T   # noqa: E402

L, shim = rs.L, rs.shim
shim.shim_set_compute.argtypes = [C.c_int]
shim.shim_unmodelled.restype = C.c_longlong
for f in (shim.shim_kernel_names, shim.shim_gemm_modes):
    f.restype, f.argtypes = C.c_longlong, [C.c_char_p, C.c_longlong]

FAMILY = ("dgemm_", "scale_kernel", "splitk_reduce_kernel")


def short(mangled):
    """_ZN12_GLOBAL__N_112dgemm_kernelILb1ELb1ELi0ELi0EEEvNS_8GemmArgsE -> dgemm_kernel<1,1,0,0> (bool and int template arguments only)"""
    pos = 3 if mangled.startswith("_ZN") else 2 if mangled.startswith("_Z") else len(mangled)
    while True:                                    # the length-prefixed identifiers of the (nested) name, one after the other
        m = re.match(r"\d+", mangled[pos:])
        if not m:
            break
        ident = mangled[pos + m.end():pos + m.end() + int(m.group())]
        pos += m.end() + len(ident)
        if ident.endswith("kernel"):
            t = re.match(r"I((?:L[ib]n?\d+E)+)E", mangled[pos:])
            return ident if not t else "%s<%s>" % (ident, ",".join(a.replace("n", "-") for a in re.findall(r"L[ib](n?\d+)E", t.group(1))))
    return mangled


def text_of(fn):
    buf = C.create_string_buffer(1 << 20)
    assert int(fn(buf, len(buf))) <= len(buf)
    return buf.value.decode()


def registered():
    return sorted({short(n) for n in text_of(shim.shim_kernel_names).split() if any(w in n for w in FAMILY)})


def upload(flat):
    p = rs.dmalloc(8 * flat.size)
    np.ctypeslib.as_array((C.c_double * flat.size).from_address(p.value))[:] = flat
    return p


def download(p, size):
    return np.ctypeslib.as_array((C.c_double * size).from_address(p.value)).copy()


def at(p, off):
    return C.c_void_p(p.value + 8 * off)


def call(c, alpha, beta, ptr, ld):
    """the C ABI call of a row on device pointers ptr[name] (already offset) -> status"""
    if c.op == "gemm":
        return L.cap_dgemm(T.CAP_TRANS[c.form[0]], T.CAP_TRANS[c.form[1]], c.m, c.n, c.k, alpha, ptr["A"], ld["A"], ptr["B"], ld["B"], beta, ptr["C"], ld["C"], None)
    if c.op == "syrk":
        return L.cap_dsyrk(1 if c.form[0] == "U" else 0, T.CAP_TRANS[c.form[1]], c.n, c.k, alpha, ptr["A"], ld["A"], beta, ptr["C"], ld["C"], None)
    side = 0 if c.form[0] == "L" else 1
    work = rs.dmalloc(8 * max(int(L.cap_dtrmm_work_size(side, c.m, c.n)), 2))
    st = L.cap_dtrmm(side, 1, T.CAP_TRANS[c.form[1]], 0, c.m, c.n, alpha, ptr["T"], ld["T"], ptr["B"], ld["B"], work, None)
    shim.hipFree(work)
    return st


def launches():
    """short names of the GEMM-family launches of the trace so far, and the trace lines that are findings by themselves"""
    path = os.path.join(rs.build_shim.OUT, "trace_blas3_%d.txt" % os.getpid())
    shim.shim_dump(path.encode())
    lines = open(path).read().splitlines()
    os.unlink(path)
    bad = [l for l in lines if l.split()[0] in ("OOB", "ORPHAN", "BADLAUNCH", "UNMODELLED", "BADFREE")]
    return [short(l.split()[2]) for l in lines if l.startswith("K ") and any(w in l.split()[2] for w in FAMILY)], bad


def run_case(c, seed):
    ops = T.operands(c, seed)
    ld = T.lds(c)
    offs = dict(zip(("T", "B") if c.op == "trmm" else ("A", "B"), c.offs))
    out_name = "B" if c.op == "trmm" else "C"
    runs = []
    for alpha, beta in c.ab:
        shim.shim_reset(); text_of(shim.shim_gemm_modes)
        host = {name: T.place(T.initial_output(c, ops, beta) if name == out_name else mat, ld[name], offs.get(name, 0)) for name, mat in ops.items()}
        dev = {name: upload(flat) for name, flat in host.items()}
        st = call(c, alpha, beta, {name: at(p, offs.get(name, 0)) for name, p in dev.items()}, ld)
        kernels, bad = launches()
        modes = [dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in l.split()) for l in text_of(shim.shim_gemm_modes).splitlines()]
        want = dict(host)
        want[out_name] = T.place(T.exact_reference(c, ops, alpha, beta), ld[out_name], offs.get(out_name, 0))
        detail = ["%s: %s" % (name, T.describe_mismatch(download(dev[name], host[name].size), want[name], ld[name], offs.get(name, 0)))
                  for name in host if not T.same_bits(download(dev[name], host[name].size), want[name])]
        for p in dev.values():
            shim.hipFree(p)
        runs.append({"alpha": alpha, "beta": beta, "status": int(st), "kernels": kernels, "modes": modes, "exact": not detail, "detail": detail + bad})
    return runs


def run_big(c):
    """trace mode: which instance a large-pitch row launches (the 4.3 GB operand is an untouched mapping)"""
    runs = []
    ld = {"A": T.BIG_K, "B": T.BIG_K, "C": c.m}
    ld[c.which] = c.ld
    for alpha, beta in c.ab:
        shim.shim_reset()
        dev = {"A": rs.dmalloc(8 * c.m * ld["A"]), "B": rs.dmalloc(8 * c.n * ld["B"]), "C": rs.dmalloc(8 * c.m * c.n)}
        st = call(c, alpha, beta, dev, ld)
        kernels, bad = launches()
        for p in dev.values():
            shim.hipFree(p)
        runs.append({"alpha": alpha, "beta": beta, "status": int(st), "kernels": kernels, "modes": [], "exact": None, "detail": bad})
    return runs


def table(results):
    """one line per row: what it launches"""
    out = ["%-34s %-55s %-16s %s" % ("case", "kernel instances (launch order)", "modes", "why")]
    for c in T.CASES + T.BIG_CASES:
        r = results[c.id][0]
        m = r["modes"][0] if r["modes"] else {}
        modes = " ".join(w for w in ("ksplit=%d" % m["ksplit"] if m.get("ksplit", 1) > 1 else "", "band=%dx%d" % (m["stm"], m["stn"]) if m and m["stm"] != m["stn"] else "",
                                      "etri=%d" % m["etri"] if m.get("etri") else "") if w)
        out.append("%-34s %-55s %-16s %s" % (c.id, " + ".join(r["kernels"]), modes, c.why))
    return "\n".join(out)


def main(argv):
    want_table = "--table" in argv
    paths = [a for a in argv if not a.startswith("--")]
    only = os.environ.get("SHIM_FILTER", "")
    results = {}
    shim.shim_set_compute(1)
    for i, c in enumerate(T.CASES):
        if only and only not in c.id:
            continue
        try:
            results[c.id] = run_case(c, i)
        except Exception as e:      # a refused call or a crash of the host side is a finding of that row
            results[c.id] = [{"alpha": None, "beta": None, "status": -1, "kernels": [], "modes": [], "exact": False, "detail": ["exception: %r" % (e,)]}]
    shim.shim_set_compute(0)
    for c in T.BIG_CASES:
        if only and only not in c.id:
            continue
        results[c.id] = run_big(c)
    out = {"registered": registered(), "unmodelled": int(shim.shim_unmodelled()), "cases": results}
    if paths:
        json.dump(out, open(paths[0], "w"), indent=1)
    if want_table and not only:
        print(table(results))
    bad = sum(1 for r in results.values() for x in r if x["exact"] is False or x["status"] != 0)
    print("%d rows, %d calls, %d not exact" % (len(results), sum(len(r) for r in results.values()), bad))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
