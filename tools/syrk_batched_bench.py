"""Time the batched symmetric rank-k products into the factor layout (cap_dsyrk_batched / cap_dsyrk_vbatched, csrc/syrk_batched.hip).

One run; every item is a window between two stream events that holds `inner` back-to-back calls (the per-call time is window / inner), the
items of a row alternating in one process, median of --reps windows after one warm-up round, fastest and slowest beside it.
  1. FIXED SIZE: n in 8 .. 256, k in 1, 16, 64, 1024, at 1024 blocks and at 65536 (n <= 32) / 16384 (n = 64) / 4096 (n > 64) blocks (halved
     until V holds at most 2^30 elements): the call with V in either layout (beta = 0, fill = 0) and with fill = 1, against
       (a) torch.bmm on the same operands (both triangles, C = V^T V in torch's reading),
       (b) a device-to-device copy of V plus as many doubles as C's triangles hold - the traffic the call cannot avoid.
     TFLOP/s on the n (n + 1) k useful flops, as a fraction of the fp64 MFMA peak (78.6 TFLOP/s), and the fraction of the copy rate.
  2. THE MIXED BLOCK-JACOBI BATCH of tools/potrf_vbatched_bench.py (80 % n <= 16, 20 % n in 100..200; 4096 blocks) through a plan against one
     fixed-size call per distinct size on pre-gathered sub-batches (the gather is not counted).
  3. FORM AND FACTOR AGAINST UPDATE: A_i + V_i V_i^T by cap_dsyrk_batched (beta = 1) followed by cap_dpotrf_batched_blocked, against
     cap_dcholupdate_batched on the resident factor, k in 1, 4, 16 - the figure behind the "forming not counted" of the update rows.  The
     window of the first holds a restoring copy of A in front of every pair; the copy alone is timed beside it and subtracted.
  4. with --parent-lib: cap_dpotrf_batched_blocked and cap_dtrsm_batched of this build and of another build of the library (the parent
     commit's), alternating in this process at 1024 blocks - the existing entries must not have moved.
The time of these kernels does not depend on the data.  Writes the table to --out and prints it:

    timeout -k 10 900 python tools/syrk_batched_bench.py [--reps 9] [--out profiles/r25_syrk_batched.txt] [--parent-lib path/to/libcapital_amd.so]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from capital_amd import _lib, build  # noqa: E402

OUT = [None]
T_, N_ = 1, 0
PEAK = 78.6e12                                  # fp64 matrix peak of the MI355X, FLOP/s
V_CAP = 1 << 30


def say(line=""):
    print(line, flush=True)
    if OUT[0]:
        OUT[0].write(line + "\n")
        OUT[0].flush()


def stats(x):
    x = sorted(x[1:])                       # the first round is the warm-up
    return x[len(x) // 2], x[0], x[-1]


class Timer:
    def __init__(self):
        self.s = torch.cuda.current_stream()

    def __call__(self, fn, inner=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.s)
        for _ in range(inner):
            fn()
        e1.record(self.s)
        e1.synchronize()
        return e0.elapsed_time(e1) / inner


def big_batch(n):
    return 65536 if n <= 32 else 16384 if n == 64 else 4096


def group1(L, a, T, sp):
    say("1. fixed size, beta = 0; per-call times in ms, median [fastest slowest] for the NOTRANS call, medians for the rest; (a) torch.bmm, (b) "
        "device-to-device copy of V plus the triangles' worth of doubles")
    say("%4s %5s %6s  %-30s %9s %9s %9s %9s  %8s %8s %8s %8s %7s" % (
        "n", "k", "blocks", "cap_dsyrk_batched N", "T", "N fill=1", "(a)", "(b)", "(a)/N", "T/N", "(b)/N", "TFLOP/s", "% peak"))
    losses = []
    for n in a.sizes:
        for k in a.ks:
            done = set()
            for batch in (1024, big_batch(n)):
                while batch * n * k > V_CAP:
                    batch //= 2
                if batch in done:
                    continue
                done.add(batch)
                V = torch.rand(batch, k, n, dtype=torch.float64, device="cuda") - 0.5          # NOTRANS: n x k column-major blocks, ldv = n
                Vt = V.transpose(1, 2).contiguous()                                             # TRANS: k x n column-major blocks, ldv = k
                Cm = torch.zeros(batch, n, n, dtype=torch.float64, device="cuda")
                Vc, tri, tric = torch.empty_like(V), torch.zeros(batch * n * (n + 1) // 2, dtype=torch.float64, device="cuda"), None
                tric = torch.empty_like(tri)
                flops = float(batch) * n * (n + 1) * k
                inner = a.inner if flops < 2e10 else 2

                def syrk(trans, fill):
                    if trans:
                        _lib.check(L.cap_dsyrk_batched(1, T_, n, k, 1.0, Vt.data_ptr(), k, n * k, 0.0, Cm.data_ptr(), n, n * n, None, fill, batch, sp))
                    else:
                        _lib.check(L.cap_dsyrk_batched(1, N_, n, k, 1.0, V.data_ptr(), n, n * k, 0.0, Cm.data_ptr(), n, n * n, None, fill, batch, sp))

                def copy():
                    Vc.copy_(V)
                    tric.copy_(tri)
                t = {x: [] for x in ("n", "t", "f", "a", "c")}
                for rep in range(a.reps + 1):
                    for key, fn in (("n", lambda: syrk(0, 0)), ("t", lambda: syrk(1, 0)), ("f", lambda: syrk(0, 1)),
                                    ("a", lambda: torch.bmm(Vt, V, out=Cm)), ("c", copy)):
                        t[key].append(T(fn, inner))
                sn, st, sf, sa, sc = (stats(t[x]) for x in ("n", "t", "f", "a", "c"))
                tf = flops / (sn[0] * 1e-3) / 1e12
                say("%4d %5d %6d  %9.4f [%8.4f %8.4f] %9.4f %9.4f %9.4f %9.4f  %8.2f %8.2f %8.2f %8.3f %7.2f" % (
                    n, k, batch, sn[0], sn[1], sn[2], st[0], sf[0], sa[0], sc[0], sa[0] / sn[0], st[0] / sn[0], sc[0] / sn[0], tf, 100 * tf * 1e12 / PEAK))
                if sn[0] > sa[0] + max(sn[2] - sn[1], sa[2] - sa[1]):
                    losses.append((n, k, batch, round(sn[0] / sa[0], 2)))
                del V, Vt, Cm, Vc, tri, tric
                torch.cuda.empty_cache()
    say("rows where the NOTRANS call is slower than torch.bmm by more than the row's own spread (n, k, blocks, call / bmm): %s" % (losses if losses else "none"))
    say()


def group2(L, a, T, sp):
    rng = np.random.default_rng([22, 4096, 2])                                  # mixed_sizes("block-Jacobi mix", 4096) of tools/potrf_vbatched_bench.py
    small = rng.random(4096) < 0.8
    sizes = np.where(small, rng.integers(1, 17, size=4096), rng.integers(100, 201, size=4096))
    batch = len(sizes)
    arr = (C.c_int64 * batch)(*[int(x) for x in sizes])
    plan = C.c_void_p()
    _lib.check(L.cap_vbatch_plan_create(batch, arr, None, None, C.byref(plan)), "cap_vbatch_plan_create")
    launches, rows, total = int(L.cap_vbatch_plan_info(plan, 4)), int(sizes.sum()), int((sizes * sizes).sum())
    A = torch.zeros(total, dtype=torch.float64, device="cuda")
    distinct = [int(x) for x in np.unique(sizes)]
    say("2. block-Jacobi mix, %d blocks (%d rows, %d distinct sizes, %.1f MB of blocks, %d launches per plan call); per-call times in ms, median "
        "[fastest slowest]; the fixed-size route: one call per distinct size on pre-gathered sub-batches" % (batch, rows, len(distinct), total * 8 / 1e6, launches))
    for k in (4, 64):
        V = torch.rand(k, rows, dtype=torch.float64, device="cuda") - 0.5
        sub = []
        for n in distinct:
            b = int((sizes == n).sum())
            sub.append((n, b, torch.rand(b, k, n, dtype=torch.float64, device="cuda") - 0.5, torch.zeros(b, n, n, dtype=torch.float64, device="cuda")))

        def per_size():
            for n, b, v, c in sub:
                _lib.check(L.cap_dsyrk_batched(1, N_, n, k, 1.0, v.data_ptr(), n, n * k, 0.0, c.data_ptr(), n, n * n, None, 0, b, sp))
        t = {"plan": [], "sizes": []}
        for rep in range(a.reps + 1):
            t["plan"].append(T(lambda: _lib.check(L.cap_dsyrk_vbatched(plan, 1, N_, k, 1.0, V.data_ptr(), rows, 0.0, A.data_ptr(), None, 0, sp)), a.inner))
            t["sizes"].append(T(per_size, 2))
        p, s = stats(t["plan"]), stats(t["sizes"])
        say("   k %3d  cap_dsyrk_vbatched %9.4f [%8.4f %8.4f]   one call per size %9.4f [%8.4f %8.4f]   per size / plan %.1f" % (
            k, p[0], p[1], p[2], s[0], s[1], s[2], s[0] / p[0]))
    say()
    L.cap_vbatch_plan_destroy(plan)


def group3(L, a, T, sp):
    say("3. A + V V^T formed by cap_dsyrk_batched (beta = 1) and factored by cap_dpotrf_batched_blocked against cap_dcholupdate_batched on the resident "
        "factor; per-call times in ms, medians; form + factor = (copy, syrk, potrf) - (copy)")
    say("%4s %3s %6s  %9s %9s %9s %9s  %s" % ("n", "k", "blocks", "syrk", "syrk+potrf", "update", "copy", "(syrk + potrf) / update"))
    for n in a.sizes:
        for batch in (1024, big_batch(n)):
            g = torch.Generator(device="cuda").manual_seed(n)
            X = torch.rand(batch, n, n, dtype=torch.float64, device="cuda", generator=g) - 0.5
            A0 = torch.bmm(X, X.transpose(1, 2)) + n * torch.eye(n, dtype=torch.float64, device="cuda")
            del X
            A, R = A0.clone(), A0.clone()
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            _lib.check(L.cap_dpotrf_batched_blocked(1, n, R.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
            R0 = R.clone()
            for k in (1, 4, 16):
                V = (torch.rand(batch, k, n, dtype=torch.float64, device="cuda") - 0.5) * 0.1

                def syrk():
                    _lib.check(L.cap_dsyrk_batched(1, N_, n, k, 1.0, V.data_ptr(), n, n * k, 1.0, A.data_ptr(), n, n * n, None, 0, batch, sp))

                def both():
                    A.copy_(A0)
                    syrk()
                    _lib.check(L.cap_dpotrf_batched_blocked(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))

                def update():
                    _lib.check(L.cap_dcholupdate_batched(1, 1, n, k, R.data_ptr(), n, n * n, V.data_ptr(), n, n * k, batch, info.data_ptr(), sp))
                t = {x: [] for x in ("s", "b", "u", "c")}
                for rep in range(a.reps + 1):
                    A.copy_(A0)
                    R.copy_(R0)
                    for key, fn in (("s", syrk), ("b", both), ("u", update), ("c", lambda: A.copy_(A0))):
                        t[key].append(T(fn, a.inner))
                s, b, u, c = (stats(t[x])[0] for x in ("s", "b", "u", "c"))
                say("%4d %3d %6d  %9.4f %9.4f %9.4f %9.4f  %.2f" % (n, k, batch, s, b - c, u, c, (b - c) / u))
            assert not info.cpu().numpy().any()
            del A0, A, R, R0
            torch.cuda.empty_cache()
    say()


def group4(L, a, T, sp, path):
    P = C.CDLL(path)
    for name in ("cap_dpotrf_batched_blocked", "cap_dtrsm_batched"):
        sig = _lib.SIGNATURES[name]
        getattr(P, name).restype, getattr(P, name).argtypes = sig[0], sig[1]
    say("4. cap_dpotrf_batched_blocked and cap_dtrsm_batched (trans, 16 right-hand sides) of this build and of the parent commit's build, alternating "
        "in this process; 1024 blocks, per-call times in ms, median [fastest slowest]")
    say("%4s %-6s  %-30s %-30s %8s %s" % ("n", "entry", "this build", "parent build", "this/par", "within the spread"))
    moved = []
    for n in a.sizes:
        batch, nrhs = 1024, 16
        g = torch.Generator(device="cuda").manual_seed(n)
        X = torch.rand(batch, n, n, dtype=torch.float64, device="cuda", generator=g) - 0.5
        A0 = torch.bmm(X, X.transpose(1, 2)) + n * torch.eye(n, dtype=torch.float64, device="cuda")
        A = A0.clone()
        info = torch.zeros(batch, dtype=torch.int32, device="cuda")
        B = torch.rand(batch, nrhs, n, dtype=torch.float64, device="cuda") - 0.5
        _lib.check(L.cap_dpotrf_batched_blocked(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
        R = A.clone()
        for entry in ("potrf", "trsm"):
            t = {"new": [], "old": []}
            for rep in range(a.reps + 1):
                for key, lib in (("new", L), ("old", P)):
                    if entry == "potrf":
                        def fn():
                            A.copy_(A0)
                            _lib.check(lib.cap_dpotrf_batched_blocked(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
                    else:
                        def fn():
                            _lib.check(lib.cap_dtrsm_batched(1, T_, n, nrhs, R.data_ptr(), n, n * n, B.data_ptr(), n, n * nrhs, batch, info.data_ptr(), None, 0, sp))
                    t[key].append(T(fn, a.inner))
            x, y = stats(t["new"]), stats(t["old"])
            ok = abs(x[0] - y[0]) <= max(x[2] - x[1], y[2] - y[1])
            if not ok:
                moved.append((n, entry))
            say("%4d %-6s  %9.4f [%8.4f %8.4f] %9.4f [%8.4f %8.4f] %8.3f %s" % (n, entry, x[0], x[1], x[2], y[0], y[1], y[2], x[0] / y[0], "yes" if ok else "NO"))
    say("the existing entries within the run's own spread of the parent's time at every row: %s (potrf's windows include the restoring copy)" % (
        "yes" if not moved else "NO - %s" % moved))
    say()


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for name, v in sorted(build.kernel_resources().items()):
        if "syrk_" in name and "batched" in name:
            say("  %-74s VGPRs %3s  AGPRs %3s  scratch %s  LDS %6s B  waves/SIMD %s" % (
                name, v.get("VGPRs"), v.get("AGPRs"), v.get("ScratchSize"), v.get("LDS Size"), v.get("Occupancy")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sizes", default="8,16,32,64,96,128,192,256")
    ap.add_argument("--ks", default="1,16,64,1024")
    ap.add_argument("--groups", default="1,2,3,4")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_syrk_batched.txt"))
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    a.ks = [int(x) for x in a.ks.split(",")]
    groups = a.groups.split(",")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT[0] = open(a.out, "w")
    L = _lib.lib()
    T = Timer()
    sp = T.s.cuda_stream
    say("Batched symmetric rank-k products into the factor layout (cap_dsyrk_batched / cap_dsyrk_vbatched, csrc/syrk_batched.hip) - round 25")
    say("tools/syrk_batched_bench.py on one %s, torch %s, ONE run, %d windows of %d calls (2 for the heaviest rows) after a warm-up round, every window "
        "between two stream events" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.inner))
    say()
    if "1" in groups:
        group1(L, a, T, sp)
    if "2" in groups:
        group2(L, a, T, sp)
    if "3" in groups:
        group3(L, a, T, sp)
    if "4" in groups and a.parent_lib:
        group4(L, a, T, sp, a.parent_lib)
    resources()
    OUT[0].close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
