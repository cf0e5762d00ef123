"""Time the thin symmetric product, the 1-norm, the condition estimate and the error bounds at N = 16384, 32768, 65536 (default), all in
one run on one GPU, and print one JSON line per measurement (median / min ms over --reps calls after a warm-up, device events):

    copy          a device-to-device copy of 4 GiB: bytes read + bytes written per second, the rate the others are set against
    symm_thin     cap_dsymm_thin (alpha = -1, beta = 1: the residual B - A X) at nrhs 1 / 4 / 16, and cap_dlansy: ms, bytes of the
                  upper triangle per second, and that rate as a fraction of the copy rate of this run
    factor        cap_cholinv_factor (complete_inv = -1)
    solve         cap_cholinv_solve at nrhs 1 / 8 / 16
    rcond         cap_cholinv_rcond given A (the norm included), the number of solves the estimator took, and its time in units of
                  one single-column solve - (solves taken + 1) is what the design promises, 11 would mean the skip word does not work
    error_bounds  cap_cholinv_error_bounds at nrhs 1 / 8 / 16, berr alone and ferr + berr, against the solve of the same nrhs

    timeout -k 10 900 python tools/poerr_bench.py [--n 16384,32768,65536] [--reps 5] > profiles/r14_poerr.txt
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def med(s, fn, reps):
    timed(s, fn)
    ts = sorted(timed(s, fn) for _ in range(reps))
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768,65536")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    # ---- the copy rate of this run
    nb = 4 << 30
    src = torch.empty(nb // 8, dtype=torch.float64, device="cuda").fill_(1.0)
    dst = torch.empty_like(src)
    st = med(s, lambda: dst.copy_(src), a.reps)
    copy_rate = 2 * nb / (st["median_ms"] * 1e-3)
    print(json.dumps({"route": "copy", "bytes": nb, **st, "read_plus_write_TB/s": round(copy_rate / 1e12, 3)}), flush=True)
    del src, dst
    for n in [int(x) for x in a.n.split(",")]:
        A = torch.empty(n, n, dtype=torch.float64, device="cuda")
        _lib.check(L.cap_fill_symmetric(A.data_ptr(), n, n, 0, 0, 1, 1, sp), "fill")
        tri = n * (n + 1) // 2 * 8
        X = torch.rand(16, n, dtype=torch.float64, device="cuda") - 0.5
        B = torch.rand(16, n, dtype=torch.float64, device="cuda") - 0.5
        Y = torch.empty(16, n, dtype=torch.float64, device="cuda")
        work = torch.empty(L.cap_dsymm_thin_work_size(n, 16), dtype=torch.float64, device="cuda")
        for nrhs in (1, 4, 16):
            st = med(s, lambda: _lib.check(L.cap_dsymm_thin(1, 0, n, nrhs, -1.0, A.data_ptr(), n, X.data_ptr(), n, 1.0, B.data_ptr(), n,
                                                            Y.data_ptr(), n, work.data_ptr(), sp), "symm_thin"), a.reps)
            rate = tri / (st["median_ms"] * 1e-3)
            print(json.dumps({"n": n, "route": "symm_thin", "nrhs": nrhs, **st, "triangle_TB/s": round(rate / 1e12, 3),
                              "of_copy_rate": round(rate / copy_rate, 3)}), flush=True)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        lw = torch.empty(L.cap_dlansy_work_size(n), dtype=torch.float64, device="cuda")
        st = med(s, lambda: _lib.check(L.cap_dlansy(ord('1'), 1, n, A.data_ptr(), n, out.data_ptr(), lw.data_ptr(), sp), "lansy"), a.reps)
        rate = tri / (st["median_ms"] * 1e-3)
        print(json.dumps({"n": n, "route": "lansy", **st, "triangle_TB/s": round(rate / 1e12, 3), "of_copy_rate": round(rate / copy_rate, 3),
                          "norm1": out.item()}), flush=True)
        del work, lw
        # ---- the plan
        h = C.c_void_p()
        _lib.check(L.cap_cholinv_plan_create(C.byref(h), n, -1, 1, -2, b"U", None), "plan")
        st = med(s, lambda: _lib.check(L.cap_cholinv_factor(h, A.data_ptr(), n, sp), "factor"), 2)
        factor_ms = st["median_ms"]
        print(json.dumps({"n": n, "route": "factor", **st}), flush=True)
        info = C.c_int64(0)
        _lib.check_info(L.cap_cholinv_info(h, sp, C.byref(info)), "info")
        assert info.value == 0, info.value
        solve_ms = {}
        for nrhs in (1, 8, 16):
            st = med(s, lambda: _lib.check(L.cap_cholinv_solve(h, B.data_ptr(), n, Y.data_ptr(), n, nrhs, sp), "solve"), a.reps)
            solve_ms[nrhs] = st["median_ms"]
            print(json.dumps({"n": n, "route": "solve", "nrhs": nrhs, **st}), flush=True)
        rc = torch.zeros(1, dtype=torch.float64, device="cuda")
        st = med(s, lambda: _lib.check(L.cap_cholinv_rcond(h, A.data_ptr(), n, None, rc.data_ptr(), sp), "rcond"), a.reps)
        solves = L.cap_pocon_last_solves()
        print(json.dumps({"n": n, "route": "rcond", **st, "rcond": rc.item(), "solves_taken": solves,
                          "in_single_column_solves": round(st["median_ms"] / solve_ms[1], 2), "expected_about": solves + 1,
                          "of_factor": round(st["median_ms"] / factor_ms, 4)}), flush=True)
        fe = torch.zeros(16, dtype=torch.float64, device="cuda")
        be = torch.zeros(16, dtype=torch.float64, device="cuda")
        for nrhs in (1, 8, 16):
            _lib.check(L.cap_cholinv_solve(h, B.data_ptr(), n, Y.data_ptr(), n, nrhs, sp), "solve")
            sb = med(s, lambda: _lib.check(L.cap_cholinv_error_bounds(h, A.data_ptr(), n, B.data_ptr(), n, Y.data_ptr(), n, nrhs, None,
                                                                      be.data_ptr(), sp), "berr"), a.reps)
            sf = med(s, lambda: _lib.check(L.cap_cholinv_error_bounds(h, A.data_ptr(), n, B.data_ptr(), n, Y.data_ptr(), n, nrhs, fe.data_ptr(),
                                                                      be.data_ptr(), sp), "bounds"), a.reps)
            print(json.dumps({"n": n, "route": "error_bounds", "nrhs": nrhs, "berr_only": sb, "ferr_and_berr": sf,
                              "solves_taken": L.cap_pocon_last_solves(), "in_solves_of_this_nrhs": round(sf["median_ms"] / solve_ms[nrhs], 2),
                              "max_berr": be[:nrhs].max().item(), "max_ferr": fe[:nrhs].max().item()}), flush=True)
        L.cap_cholinv_plan_destroy(h)
        del A, X, B, Y


if __name__ == "__main__":
    main()
