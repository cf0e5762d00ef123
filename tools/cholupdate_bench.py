"""Time the rank-k update / downdate of the resident fp64 Cholesky factor (cap_cholinv_update) against a new factorization:

    one   option "chud_kernel" = 1: one launch per pass of 16 columns of V (+ its recovery launch), csrc/cholupdate.hip
    step  option "chud_kernel" = 0: two launches per 64-row block step, the same item code

For every n and k, one repetition is: cap_cholinv_factor(A), then with each driver an update by V and the downdate by the same V (which
returns to the factor of A), every call between two stream events.  Reported per (n, k, sign): the median over --reps repetitions after
one warm-up repetition, the ratio to the factor call's median of the same repetitions, and the bytes of the sweep - n (n + 1) / 2
elements read and written (16 B) per pass - per second as a share of the device-to-device copy rate measured in the same run (a copy of
the triangle's bytes, read + write counted).  A = the diagonally dominant test matrix of cap_fill_symmetric, V uniform in [-0.1, 0.1).
One process, one GPU; prints the table of profiles/r12_cholupdate.txt:

    timeout -k 10 900 python tools/cholupdate_bench.py [--n 4096,16384,32768] [--k 1,16,64] [--reps 9]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,16384,32768")
    ap.add_argument("--k", default="1,16,64")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    s = torch.cuda.current_stream()
    sp = s.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    fb0 = int(L.cap_update_fallbacks())
    print("     n    k  sign   factor ms    one ms  (x factor, of copy)    step ms  (x factor, of copy)   copy TB/s   backward error")
    for n in [int(x) for x in a.n.split(",")]:
        A = torch.empty(n, n, dtype=torch.float64, device="cuda")
        _lib.check(L.cap_fill_symmetric(A.data_ptr(), n, n, 0, 0, 1, 1, sp), "fill")
        h = C.c_void_p()
        _lib.check(L.cap_cholinv_plan_create(C.byref(h), n, -1, 1, -2, b"U", None), "plan")
        tri_elems = n * (n + 1) // 2
        src = torch.empty(tri_elems, dtype=torch.float64, device="cuda").normal_()
        dst = torch.empty_like(src)
        copy_ms = median([timed(lambda: dst.copy_(src)) for _ in range(a.reps + 1)][1:])
        copy_tbs = 16.0 * tri_elems / (copy_ms * 1e-3) / 1e12
        del src, dst
        for k in [int(x) for x in a.k.split(",")]:
            g = torch.Generator(device="cuda").manual_seed(1000 + k)
            V = (torch.rand(k, n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1) * 0.1      # buffer [col, row]
            passes = (k + 15) // 16
            t = {"factor": [], (1, 1): [], (1, -1): [], (0, 1): [], (0, -1): []}
            for rep in range(a.reps + 1):
                t["factor"].append(timed(lambda: _lib.check(L.cap_cholinv_factor(h, A.data_ptr(), n, sp), "factor")))
                for drv in (1, 0):
                    _lib.check(L.cap_cholinv_set_option(h, b"chud_kernel", drv), "option")
                    for sign in (1, -1):
                        t[(drv, sign)].append(timed(lambda: _lib.check(L.cap_cholinv_update(h, sign, V.data_ptr(), n, k, sp), "update")))
            info = C.c_int64(0)
            _lib.check_info(L.cap_cholinv_info(h, sp, C.byref(info)), "info")
            assert info.value == 0, info.value
            # after the last downdate R is the factor of A again: |R^T R - A|_F / |A|_F
            R = torch.empty(n, n, dtype=torch.float64, device="cuda")
            _lib.check(L.cap_cholinv_get_R(h, R.data_ptr(), n, sp), "get_R")
            E = R @ R.t()                       # buffer [col, row] holds R^T: R^T R
            E -= A
            berr = (torch.linalg.norm(E) / torch.linalg.norm(A)).item()
            del R, E
            fm = median(t["factor"][1:])
            for sign in (1, -1):
                cells = []
                for drv in (1, 0):
                    m = median(t[(drv, sign)][1:])
                    tbs = passes * 16.0 * tri_elems / (m * 1e-3) / 1e12
                    cells.append("%9.3f  (%6.4f, %5.3f)     " % (m, m / fm, tbs / copy_tbs))
                print("%6d %4d   %+d   %9.3f %s %9.3f    %.2e" % (n, k, sign, fm, "".join(cells), copy_tbs, berr), flush=True)
        L.cap_cholinv_plan_destroy(h)
        del A
    print("fallbacks during the run: %d" % (int(L.cap_update_fallbacks()) - fb0))


if __name__ == "__main__":
    main()
