"""TEST INFRASTRUCTURE: the rows of tests/cqr256_cases.py through the library's own launchers on the recording stand-in.

    python tests/hipshim/run_cqr256.py out.json          # what tests/test_cqr256_cases.py starts

Per row: the status of cap_dgram256 / cap_dqrapply256, the grid of every launch the call made (the stand-in's `K` trace lines) and whether the CPU
kernel models' result equals the exact reference bit for bit with every NaN of the buffers where it was.  The CPU models are plain
loops: they check the table, the reference helpers and the launchers' arithmetic before a GPU sees them, not the kernels' LDS rings.
The rows above MAX_COMPUTE_M run in trace mode (grids only, no byte touched).  Every refusal row must return CAP_ERR_UNSUPPORTED without
a launch.  Its own process (no torch)."""
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
from tests import cqr256_cases as T   # noqa: E402
from tests.blas3_cases import NAN, describe_mismatch, same_bits   # noqa: E402

L, shim = rs.L, rs.shim
shim.shim_set_compute.argtypes = [C.c_int]
N = T.N
MAX_COMPUTE_M = 20000
ALL_PADS_M = 2048
TAIL = 64


def upload(arr):
    flat = np.ascontiguousarray(arr, dtype=np.float64).ravel()
    p = rs.dmalloc(8 * flat.size)
    np.ctypeslib.as_array((C.c_double * flat.size).from_address(p.value))[:] = flat
    return p


def download(p, shape):
    size = int(np.prod(shape))
    return np.ctypeslib.as_array((C.c_double * size).from_address(p.value)).copy().reshape(shape)


def launches():
    """(kernel name, grid x) of the launches of the trace so far, and the trace lines that are findings by themselves"""
    path = os.path.join(rs.build_shim.OUT, "trace_cqr256_%d.txt" % os.getpid())
    shim.shim_dump(path.encode())
    lines = open(path).read().splitlines()
    os.unlink(path)
    bad = [l for l in lines if l.split()[0] in ("OOB", "ORPHAN", "BADLAUNCH", "UNMODELLED", "BADFREE")]
    return [l.split() for l in lines if l.startswith("K ")], bad


def grid_of(kline, name):
    """grid x of the launch of `name` among the K lines ("K stream name gx gy gz bx ...")"""
    hit = [k for k in kline if name in k[2]]
    assert len(hit) == 1, (name, kline)
    return int(hit[0][3])


def run_gram(m, cap, compute):
    res = []
    ws = int(L.cap_dgram256_work_size(m))
    full = compute and m <= ALL_PADS_M          # (the CPU models are plain loops: the taller rows run one padded geometry)
    for pq in T.GRAM_LDQ_PADS if full else (2,):
        for pg in T.GRAM_LDG_PADS if full else (3,):
            shim.shim_reset()
            ldq, ldg = m + pq, N + pg
            detail = []
            if compute:
                qhost = T.place_cols(T.panel(m), ldq)
                q, g, work = upload(qhost), upload(np.full((N, ldg), NAN)), upload(np.full(ws + TAIL, NAN))
            else:
                q, g, work = rs.dmalloc(8 * N * ldq), rs.dmalloc(8 * N * ldg), rs.dmalloc(8 * (ws + TAIL))
            st = L.cap_dgram256(m, q, ldq, g, ldg, work, cap, None)
            k, bad = launches()
            if compute:
                got, want = download(g, (N, ldg)), T.place_cols(T.gram_reference(m), ldg)
                if not same_bits(got, want):
                    detail.append("G: " + describe_mismatch(got, want, ldg))
                if not same_bits(download(q, (N, ldq)), qhost):
                    detail.append("Q changed")
                if not same_bits(download(work, (ws + TAIL,))[ws:], np.full(TAIL, NAN)):
                    detail.append("the sentinel behind the work buffer changed")
            for p in (q, g, work):
                shim.hipFree(p)
            res.append({"ldq": ldq, "ldg": ldg, "status": int(st), "work": ws, "slabs": grid_of(k, "gram256_kernel") if st == 0 else None,
                        "reduce_grid": grid_of(k, "gram256_reduce_kernel") if st == 0 else None, "launches": len(k), "exact": (not detail) if compute else None,
                        "detail": detail + bad})
    return res


def run_apply(m, cap, compute, ri):
    res = []
    ldin, ldout = m + 2, m + 6
    for inplace in (False, True):
        shim.shim_reset()
        detail = []
        if compute:
            want = T.apply_reference(T.panel(m), ri)
            qhost = T.place_cols(T.panel(m), ldin)
            qin, rid = upload(qhost), upload(ri)
            qout = qin if inplace else upload(np.full((N, ldout), NAN))
        else:
            qin, rid = rs.dmalloc(8 * N * ldin), rs.dmalloc(8 * N * N)
            qout = qin if inplace else rs.dmalloc(8 * N * ldout)
        ldo = ldin if inplace else ldout
        st = L.cap_dqrapply256(m, qin, ldin, rid, qout, ldo, cap, None)
        k, bad = launches()
        if compute:
            got, exp = download(qout, (N, ldo)), T.place_cols(want, ldo)
            if not same_bits(got, exp):
                detail.append("Qout: " + describe_mismatch(got, exp, ldo))
            if not inplace and not same_bits(download(qin, (N, ldin)), qhost):
                detail.append("Qin changed")
            if not same_bits(download(rid, (N, N)), ri):
                detail.append("Ri changed")
        for p in {qin.value: qin, rid.value: rid, qout.value: qout}.values():
            shim.hipFree(p)
        res.append({"inplace": inplace, "status": int(st), "grid": grid_of(k, "qrapply256_kernel") if st == 0 else None, "launches": len(k),
                    "exact": (not detail) if compute else None, "detail": detail + bad})
    return res


def main(argv):
    out = {"gram": {}, "apply": {}, "apply_nan": {}, "apply_block": {}, "refusals": []}
    for m, cap, _ in T.GRAM_CASES:
        compute = m <= MAX_COMPUTE_M
        shim.shim_set_compute(1 if compute else 0)
        out["gram"]["%d-%d" % (m, cap)] = run_gram(m, cap, compute)
    for m, cap, _ in T.APPLY_CASES:
        compute = m <= MAX_COMPUTE_M
        shim.shim_set_compute(1 if compute else 0)
        out["apply"]["%d-%d" % (m, cap)] = run_apply(m, cap, compute, T.ri_dense(m + cap))
        if compute:
            out["apply_nan"]["%d-%d" % (m, cap)] = run_apply(m, cap, True, T.ri_dense(m + cap, below=NAN))
    shim.shim_set_compute(1)
    for br, bc in T.APPLY_BLOCKS:
        out["apply_block"]["%d-%d" % (br, bc)] = run_apply(T.APPLY_BLOCK_M, T.APPLY_BLOCK_CAP, True, T.ri_block(br, bc, 16 * br + bc))
    shim.shim_set_compute(0)
    for entry, over, why in T.REFUSALS:
        shim.shim_reset()
        st = T.refusal_call(L, entry, over, ptr=C.c_void_p)
        k, bad = launches()
        out["refusals"].append({"entry": entry, "why": why, "status": int(st), "launches": len(k), "detail": bad})
    out["work_sizes"] = {str(m): int(L.cap_dgram256_work_size(m)) for m in (-16, 0, 16, 1023, 1024, 14848, 131072, 131088, 1 << 21)}
    if argv:
        json.dump(out, open(argv[0], "w"), indent=1)
    bad = sum(1 for sec in ("gram", "apply", "apply_nan", "apply_block") for r in out[sec].values() for x in r if x["exact"] is False or x["status"] != 0 or x["detail"])
    bad += sum(1 for r in out["refusals"] if r["status"] != T.UNSUPPORTED or r["launches"])
    print("%d gram rows, %d apply rows, %d refusals, %d findings" % (len(out["gram"]), len(out["apply"]), len(out["refusals"]), bad))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
