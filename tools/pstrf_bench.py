"""Time the pivoted Cholesky factorization cap_dpstrf (csrc/pstrf.hip) truncated at r steps, beside cap_cholinv_factor of the same matrix:

For every n, A = the diagonally dominant test matrix of cap_fill_symmetric (full rank: no call stops before its cap).  Per (n, r) the
median over --reps calls after one warm-up call, every call between two stream events; the bytes of the model - step j streams the j x n
factor so far, 8 n j bytes, 4 n r^2 in all (the row and the column of A and the row written per step are left out) - per second and as a
share of the 6.3 TB/s a device copy reaches on this part; and the time per step: the whole call over r, and the launch floor, the slope
between r = 8 and r = 40 (steps whose columns are a few entries long).  One process, one GPU; prints the table of
profiles/r13_pstrf.txt:

    timeout -k 10 900 python tools/pstrf_bench.py [--n 16384,65536] [--r 256,1024] [--reps 5]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402

COPY_TBS = 6.3


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,65536")
    ap.add_argument("--r", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-factor", action="store_true", help="leave cap_cholinv_factor out (it needs a second n x n matrix)")
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

    print("     n     r    pstrf ms   us/step   model TB/s  (of %.1f)   rank info   trace left / trace A   factor ms   pstrf / factor" % COPY_TBS)
    for n in [int(x) for x in a.n.split(",")]:
        A = torch.empty(n, n, dtype=torch.float64, device="cuda")
        _lib.check(L.cap_fill_symmetric(A.data_ptr(), n, n, 0, 0, 1, 1, sp), "fill")
        trace = float(torch.diagonal(A).sum().item())
        fm = float("nan")
        if not a.no_factor:
            h = C.c_void_p()
            _lib.check(L.cap_cholinv_plan_create(C.byref(h), n, -1, 1, -2, b"U", None), "plan")
            fm = median([timed(lambda: _lib.check(L.cap_cholinv_factor(h, A.data_ptr(), n, sp), "factor")) for _ in range(a.reps + 1)][1:])
            L.cap_cholinv_plan_destroy(h)
        piv = torch.empty(n, dtype=torch.int64, device="cuda")
        rank = torch.zeros(1, dtype=torch.int64, device="cuda")
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        resid = torch.zeros(1, dtype=torch.float64, device="cuda")

        def run(r):
            R = torch.empty(n, max(r, 1), dtype=torch.float64, device="cuda")         # buffer [col, row], ldr = r
            work = torch.empty(max(int(L.cap_dpstrf_work_size(n, r)), 2), dtype=torch.float64, device="cuda")
            call = lambda: _lib.check(L.cap_dpstrf(1, n, r, -1.0, A.data_ptr(), n, R.data_ptr(), max(r, 1), piv.data_ptr(), rank.data_ptr(),
                                                   resid.data_ptr(), info.data_ptr(), work.data_ptr(), sp), "pstrf")
            return median([timed(call) for _ in range(a.reps + 1)][1:])

        t8, t40 = run(8), run(40)
        floor_us = (t40 - t8) / 32 * 1e3
        for r in [int(x) for x in a.r.split(",")]:
            m = run(r)
            tbs = 4.0 * n * r * r / (m * 1e-3) / 1e12
            print("%6d %5d  %10.3f  %8.2f   %10.3f  (%5.3f)   %6d %4d   %20.3e  %10.3f   %14.4f"
                  % (n, r, m, m / r * 1e3, tbs, tbs / COPY_TBS, int(rank.item()), int(info.item()), float(resid.item()) / trace, fm, m / fm), flush=True)
        print("%6d launch floor: %.2f us per step (calls of 8 and 40 steps: %.3f and %.3f ms)" % (n, floor_us, t8, t40), flush=True)
        del A


if __name__ == "__main__":
    main()
