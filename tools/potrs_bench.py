"""Time the fp64 Cholesky solve A X = B at N = 65536 (default) for a few right-hand side counts:

    kernel   cap_cholinv_solve, option "solve_kernel" = 1 (nrhs <= 16: one launch per substitution, potrs.hip)
    blocked  cap_cholinv_solve, option "solve_kernel" = 0 (cap_dtrsm's blocked substitution with the plan's cached block inverses)
    dtrsm2   the route before cap_cholinv_solve existed: cap_dtrsm (LEFT, UPPER, TRANS) then (NOTRANS) on cap_cholinv_R_ptr

and prints one JSON line per (route, nrhs): median / min ms over --reps solves after one warm-up, the backward error of the last X,
and the solve's bytes (two passes over R's upper triangle) per second against the 6.3 TB/s HBM rate MI355X_MICROARCH.md calls achievable.
The first solve after a factor call also inverts R's diagonal blocks; it is reported separately ("first_ms").  One process, one GPU:

    timeout -k 10 600 python tools/potrs_bench.py [--n 65536] [--nrhs 1,8,16,64] [--reps 5] [--routes kernel,blocked,dtrsm2]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--nrhs", default="1,8,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", default="kernel,blocked,dtrsm2")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    n = a.n
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    A = torch.empty(n, n, dtype=torch.float64, device="cuda")
    _lib.check(L.cap_fill_symmetric(A.data_ptr(), n, n, 0, 0, 1, 1, sp), "fill")
    h = C.c_void_p()
    _lib.check(L.cap_cholinv_plan_create(C.byref(h), n, -1, 1, -2, b"U", None), "plan")
    _lib.check(L.cap_cholinv_factor(h, A.data_ptr(), n, sp), "factor")
    info = C.c_int64(0)
    _lib.check_info(L.cap_cholinv_info(h, sp, C.byref(info)), "info")
    assert info.value == 0, info.value
    ldr = C.c_int64(0)
    R = L.cap_cholinv_R_ptr(h, C.byref(ldr))
    tri_bytes = 8.0 * n * (n + 1) / 2
    for nrhs in [int(x) for x in a.nrhs.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(nrhs)
        B = torch.rand(nrhs, n, dtype=torch.float64, device="cuda", generator=g) - 0.5
        X = torch.empty_like(B)
        for route in a.routes.split(","):
            if route == "dtrsm2":
                work = torch.empty(L.cap_dtrsm_work_size(0, n, nrhs), dtype=torch.float64, device="cuda")

                def run():
                    X.copy_(B)
                    _lib.check(L.cap_dtrsm(0, 1, 1, n, nrhs, 1.0, R, ldr.value, X.data_ptr(), n, work.data_ptr(), sp), "dtrsm T")
                    _lib.check(L.cap_dtrsm(0, 1, 0, n, nrhs, 1.0, R, ldr.value, X.data_ptr(), n, work.data_ptr(), sp), "dtrsm N")
            else:
                _lib.check(L.cap_cholinv_set_option(h, b"solve_kernel", 1 if route == "kernel" else 0), "option")
                _lib.check(L.cap_cholinv_factor(h, A.data_ptr(), n, sp), "factor")     # new generation: the first solve inverts

                def run():
                    _lib.check(L.cap_cholinv_solve(h, B.data_ptr(), n, X.data_ptr(), n, nrhs, sp), "solve")
            times = []
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                run()
                e1.record(s)
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            first, rest = times[0], sorted(times[1:])
            med = rest[len(rest) // 2]
            # backward error ||B - A X||_F / (||A||_F ||X||_F) (cap_fill_symmetric fills both triangles)
            Xt = X.t()
            AX = A @ Xt
            berr = (torch.linalg.norm(B.t() - AX) / (torch.linalg.norm(A) * torch.linalg.norm(Xt))).item()
            tbs = 2 * tri_bytes / (med * 1e-3) / 1e12
            print(json.dumps({"n": n, "nrhs": nrhs, "route": route, "median_ms": round(med, 3), "min_ms": round(rest[0], 3),
                              "first_ms": round(first, 3), "TBps": round(tbs, 3), "of_6.3TBps": round(tbs / HBM_TBS, 3),
                              "byte_floor_ms": round(2 * tri_bytes / (HBM_TBS * 1e12) * 1e3, 3), "backward_error": berr}), flush=True)
            del AX
    print(json.dumps({"solve_fallbacks": int(L.cap_solve_fallbacks())}))
    L.cap_cholinv_plan_destroy(h)


if __name__ == "__main__":
    main()
