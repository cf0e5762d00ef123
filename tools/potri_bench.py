"""Time the fp64 SPD inverse A^-1 = R^-1 R^-T and the log-determinant at N = 16384 and 32768 (default):

    lauum         cap_dlauum on the plan's resident R^-1 (complete_inv = 1): the triangular product alone, n^3 / 3 flops
    syrk_nt       cap_dsyrk(UPPER, NOTRANS, n, n, 1, Rinv, ldi, 0, C, ldc): the only route to the same result before cap_dlauum existed
                  (register-staged NT kernel, dense K: n^3 flops).  The two are timed alternately and their results compared.
    inverse_ci1   cap_cholinv_inverse on a complete_inv = 1 plan, fill = 0 / 1
    inverse_ci-1  cap_cholinv_inverse on a complete_inv = -1 plan, fill = 0 / 1: the first call after a factor call (copies and inverts R)
                  and the later ones (the cached inverse)
    logdet        cap_cholinv_logdet

and prints one JSON line per measurement: median / min ms over --reps calls after one warm-up (device events on the stream), and for
lauum (n^3 / 3) / time as a fraction of the 78.6 TF fp64 MFMA peak.  One process, one GPU:

    timeout -k 10 900 python tools/potri_bench.py [--n 16384,32768] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402

PEAK_TF = 78.6


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    for n in [int(x) for x in a.n.split(",")]:
        A = torch.empty(n, n, dtype=torch.float64, device="cuda")
        _lib.check(L.cap_fill_symmetric(A.data_ptr(), n, n, 0, 0, 1, 1, sp), "fill")
        C1 = torch.zeros(n, n, dtype=torch.float64, device="cuda")
        C2 = torch.zeros(n, n, dtype=torch.float64, device="cuda")
        # ---- the product alone, against the SYRK route, on the resident R^-1 of a complete_inv = 1 plan
        h = C.c_void_p()
        _lib.check(L.cap_cholinv_plan_create(C.byref(h), n, 1, 1, -2, b"U", None), "plan")
        _lib.check(L.cap_cholinv_factor(h, A.data_ptr(), n, sp), "factor")
        info = C.c_int64(0)
        _lib.check_info(L.cap_cholinv_info(h, sp, C.byref(info)), "info")
        assert info.value == 0, info.value
        ldi = C.c_int64(0)
        Ri = L.cap_cholinv_Rinv_ptr(h, C.byref(ldi))
        routes = {
            "lauum": lambda: _lib.check(L.cap_dlauum(1, n, Ri, ldi.value, C1.data_ptr(), n, sp), "lauum"),
            "syrk_nt": lambda: _lib.check(L.cap_dsyrk(1, 0, n, n, 1.0, Ri, ldi.value, 0.0, C2.data_ptr(), n, sp), "syrk"),
        }
        ts = {k: [] for k in routes}
        for rep in range(a.reps + 1):                      # alternating; the first round is the warm-up
            for k, fn in routes.items():
                t = timed(s, fn)
                if rep:
                    ts[k].append(t)
        diff = (torch.linalg.norm(torch.tril(C1 - C2)) / torch.linalg.norm(torch.tril(C2))).item()   # buffers are [col, row]: tril = upper triangle
        for k in routes:
            st = stats(ts[k])
            tf = (n ** 3 / 3.0) / (st["median_ms"] * 1e-3) / 1e12
            print(json.dumps({"n": n, "route": k, **st, "useful_TF(n^3/3)": round(tf, 2), "of_78.6TF": round(tf / PEAK_TF, 3)}), flush=True)
        print(json.dumps({"n": n, "lauum_over_syrk_nt": round(stats(ts["lauum"])["median_ms"] / stats(ts["syrk_nt"])["median_ms"], 4),
                          "required": "<= 0.5", "routes_differ_normwise": diff}), flush=True)
        del C2
        # ---- the plan calls
        ld_dev = torch.zeros(1, dtype=torch.float64, device="cuda")
        for ci in (1, -1):
            if ci != 1:
                L.cap_cholinv_plan_destroy(h)
                h = C.c_void_p()
                _lib.check(L.cap_cholinv_plan_create(C.byref(h), n, ci, 1, -2, b"U", None), "plan")
            for fill in (0, 1):
                _lib.check(L.cap_cholinv_factor(h, A.data_ptr(), n, sp), "factor")      # new generation: the first call inverts (ci = -1)
                call = lambda: _lib.check(L.cap_cholinv_inverse(h, C1.data_ptr(), n, fill, sp), "inverse")  # noqa: E731
                first = timed(s, call)
                later = [timed(s, call) for _ in range(a.reps)]
                print(json.dumps({"n": n, "route": "inverse_ci%d" % ci, "fill": fill, "first_ms": round(first, 3), **stats(later)}), flush=True)
            if ci == -1:
                E = A @ C1                                 # C1: fill = 1, symmetric
                E.diagonal().sub_(1.0)
                res = (torch.linalg.norm(E) / (torch.linalg.norm(A) * torch.linalg.norm(C1))).item()
                del E
                print(json.dumps({"n": n, "route": "inverse_ci-1", "residual |A X - I| / (|A| |X|)": res}), flush=True)
            call = lambda: _lib.check(L.cap_cholinv_logdet(h, ld_dev.data_ptr(), sp), "logdet")  # noqa: E731
            timed(s, call)
            print(json.dumps({"n": n, "route": "logdet_ci%d" % ci, **stats([timed(s, call) for _ in range(a.reps)]), "logdet": ld_dev.item()}), flush=True)
        L.cap_cholinv_plan_destroy(h)
        del A, C1


if __name__ == "__main__":
    main()
