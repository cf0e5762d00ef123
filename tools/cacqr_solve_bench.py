"""Time the least-squares solve on a CholeskyQR2 factorization at m = 2^21, n = 256 (default), nrhs = 1, 8, 16:

    tall_tn     cap_dgemm_tall_tn on the plan's Q: the slab kernel + its reduction (csrc/cqr_solve.hip), with the achieved bytes per second
                ((m n + m nrhs) 8 B over the time) beside a device-to-device copy of Q's bytes timed in the same run
    solve       the whole cap_cacqr_solve (Q^T B, then the substitution on R with the cached block inverses)
    old_route   what a caller had to do before: cap_dgemm(TRANS, NOTRANS, n, nrhs, m) on the plan's Q, then cap_dtrsm
    factor      cap_cacqr_factor itself, for the solve's share of a factor-plus-solve

The three routes of one nrhs alternate inside one loop; median / min ms over --reps calls after one warm-up round, device events on the stream.
The last section measures the chunking crossover: nrhs = 32 ... 128 as ceil(nrhs / 16) passes of the slab kernel against one tile product.
One JSON line per measurement.  A fresh process, one GPU:

    timeout -k 10 600 python tools/cacqr_solve_bench.py [--m 2097152] [--n 256] [--nrhs 1,8,16] [--reps 9]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402

LEFT, UPPER, NOTRANS, TRANS = 0, 1, 0, 1


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def alternate(s, routes, reps):
    ts = {k: [] for k in routes}
    for rep in range(reps + 1):                            # the first round is the warm-up
        for k, fn in routes.items():
            t = timed(s, fn)
            if rep:
                ts[k].append(t)
    return {k: stats(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 21)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--nrhs", default="1,8,16")
    ap.add_argument("--crossover", default="32,48,64,128")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    assert a.reps >= 7
    m, n = a.m, a.n
    torch.cuda.set_device(0)
    L = _lib.lib()
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    lda = m + (m & 1)
    A = torch.empty(n, lda, dtype=torch.float64, device="cuda")
    _lib.check(L.cap_fill_random(A.data_ptr(), lda, m, n, 0, 0, 1, 1, 0, sp), "fill")
    h = C.c_void_p()
    _lib.check(L.cap_cacqr_plan_create(C.byref(h), m, n, 2, None), "plan")
    factor = lambda: _lib.check(L.cap_cacqr_factor(h, A.data_ptr(), lda, sp), "factor")  # noqa: E731
    factor()
    info = C.c_int64(0)
    _lib.check_info(L.cap_cacqr_info(h, sp, C.byref(info)), "info")
    assert info.value == 0, info.value
    ldq, ldr = C.c_int64(0), C.c_int64(0)
    Q = L.cap_cacqr_Q_ptr(h, C.byref(ldq))
    R = L.cap_cacqr_R_ptr(h, C.byref(ldr))
    ldq, ldr = ldq.value, ldr.value
    # ---- the yardstick of this run: a device-to-device copy of Q's bytes
    D = torch.empty_like(A)
    cp = alternate(s, {"copy": lambda: D.copy_(A)}, a.reps)["copy"]
    qbytes = 8.0 * m * n
    print(json.dumps({"m": m, "n": n, "route": "copy_of_Q_bytes", **cp, "TB_per_s_read_plus_write": round(2 * qbytes / (cp["median_ms"] * 1e-3) / 1e12, 3),
                      "TB_per_s_read_only": round(qbytes / (cp["median_ms"] * 1e-3) / 1e12, 3)}), flush=True)
    del D
    fac = alternate(s, {"factor": factor}, a.reps)["factor"]
    print(json.dumps({"m": m, "n": n, "route": "factor(num_iter=2)", **fac}), flush=True)
    # ---- the three routes
    maxr = max([int(x) for x in a.nrhs.split(",")] + [int(x) for x in a.crossover.split(",") if x])
    g = torch.Generator(device="cuda"); g.manual_seed(9)
    B = torch.randn(maxr, lda, dtype=torch.float64, device="cuda", generator=g)
    work = torch.empty(max(int(L.cap_dgemm_tall_tn_work_size(m, n, 16)), 2), dtype=torch.float64, device="cuda")
    for nrhs in [int(x) for x in a.nrhs.split(",")]:
        Z = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda")
        X = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda")
        Xo = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda")
        tw = torch.empty(max(int(L.cap_dtrsm_work_size(LEFT, n, nrhs)), 2), dtype=torch.float64, device="cuda")

        def old():
            _lib.check(L.cap_dgemm(TRANS, NOTRANS, n, nrhs, m, 1.0, Q, ldq, B.data_ptr(), lda, 0.0, Xo.data_ptr(), n, sp), "dgemm")
            _lib.check(L.cap_dtrsm(LEFT, UPPER, NOTRANS, n, nrhs, 1.0, R, ldr, Xo.data_ptr(), n, tw.data_ptr(), sp), "dtrsm")

        routes = {
            "tall_tn": lambda: _lib.check(L.cap_dgemm_tall_tn(m, n, nrhs, Q, ldq, B.data_ptr(), lda, Z.data_ptr(), n, work.data_ptr(), sp), "tall_tn"),
            "solve": lambda: _lib.check(L.cap_cacqr_solve(h, B.data_ptr(), lda, nrhs, X.data_ptr(), n, sp), "solve"),
            "old_route": old,
        }
        st = alternate(s, routes, a.reps)
        byts = 8.0 * (m * n + m * nrhs)
        print(json.dumps({"m": m, "n": n, "nrhs": nrhs, "route": "tall_tn", **st["tall_tn"],
                          "TB_per_s((mn+m*nrhs)*8)": round(byts / (st["tall_tn"]["median_ms"] * 1e-3) / 1e12, 3),
                          "of_copy_rate(read+write)": round(byts / (st["tall_tn"]["median_ms"] * 1e-3) / (2 * qbytes / (cp["median_ms"] * 1e-3)), 3)}), flush=True)
        print(json.dumps({"m": m, "n": n, "nrhs": nrhs, "route": "solve", **st["solve"],
                          "share_of_factor_plus_solve": round(st["solve"]["median_ms"] / (st["solve"]["median_ms"] + fac["median_ms"]), 4)}), flush=True)
        print(json.dumps({"m": m, "n": n, "nrhs": nrhs, "route": "old_route", **st["old_route"]}), flush=True)
        diff = (torch.linalg.norm(X - Xo) / torch.linalg.norm(Xo)).item()
        print(json.dumps({"m": m, "n": n, "nrhs": nrhs, "solve_over_old_route": round(st["solve"]["median_ms"] / st["old_route"]["median_ms"], 4),
                          "required": "< 1, and <= 0.6 at nrhs = 8", "routes_differ_normwise": diff}), flush=True)
    # ---- chunking crossover: passes of the slab kernel (16 right-hand sides each) against ONE tile product
    for nrhs in [int(x) for x in a.crossover.split(",") if x]:
        Z1 = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda")
        Z2 = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda")

        def chunks():
            for c0 in range(0, nrhs, 16):
                c = min(16, nrhs - c0)
                _lib.check(L.cap_dgemm_tall_tn(m, n, c, Q, ldq, B.data_ptr() + 8 * c0 * lda, lda, Z1.data_ptr() + 8 * c0 * n, n, work.data_ptr(), sp), "tall_tn")

        tile = lambda: _lib.check(L.cap_dgemm(TRANS, NOTRANS, n, nrhs, m, 1.0, Q, ldq, B.data_ptr(), lda, 0.0, Z2.data_ptr(), n, sp), "dgemm")  # noqa: E731
        st = alternate(s, {"chunks": chunks, "tile": tile}, a.reps)
        diff = (torch.linalg.norm(Z1 - Z2) / torch.linalg.norm(Z2)).item()
        print(json.dumps({"m": m, "n": n, "nrhs": nrhs, "route": "crossover", "slab_kernel_passes": (nrhs + 15) // 16, "passes_ms": st["chunks"],
                          "tile_product_ms": st["tile"], "passes_over_tile": round(st["chunks"]["median_ms"] / st["tile"]["median_ms"], 3),
                          "routes_differ_normwise": diff}), flush=True)
    L.cap_cacqr_plan_destroy(h)


if __name__ == "__main__":
    main()
