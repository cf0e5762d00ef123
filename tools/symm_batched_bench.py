"""Time the batched symmetric products and the diagnostics built on them (cap_dsymm_batched, cap_dlansy_batched, cap_dpocon_batched,
cap_dpoerr_batched and the _vbatched forms, csrc/symm_batched.hip).

One run; every item is a window between two stream events that holds `inner` back-to-back calls (the per-call time is window / inner), the
items of a row alternating in one process, median of --reps windows after one warm-up round, fastest and slowest beside it.
  1. SYMM at nrhs = 1 and 16 and NORM1, n in 8 .. 256, at 1024 blocks and at 65536 (n <= 32) / 16384 (n = 64) / 4096 (n > 64) blocks, against
       (a) torch.bmm on full symmetric copies of the blocks (both triangles),
       (b) a device-to-device copy of the batch's bytes (batch n n doubles) - the traffic a pass over A cannot avoid.
  2. RCOND against the cap_dpotri_batched call it contains, against torch.linalg.cond(., 1) on full copies, and against the host loop over
     cap_dlansy + cap_dpocon (timed on --loop-blocks blocks and scaled to the batch: the loop's time is proportional to its length).
  3. ERROR_BOUNDS at nrhs = 1 and 16 (ferr and berr; berr alone) against the cap_dpotrs_batched_blocked call it judges.
  4. THE MIXED BLOCK-JACOBI BATCH of tools/potrf_vbatched_bench.py (80 % n <= 16, 20 % n in 100..200; 4096 blocks) through a plan: symm, norm1,
     rcond and error_bounds at nrhs = 1.
  5. with --parent-lib: cap_dpotri_batched, cap_dpotrs_batched_blocked and cap_dsyrk_batched of this build and of another build of the
     library (the parent commit's), alternating in this process at 1024 blocks - the existing entries must not have moved.
The time of these kernels does not depend on the data.  Writes the table to --out and prints it:

    timeout -k 10 900 python tools/symm_batched_bench.py [--reps 9] [--out profiles/r26_symm_batched.txt] [--parent-lib path/to/libcapital_amd.so]
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
ONE = ord('1')


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


def spd(batch, n):
    g = torch.Generator(device="cuda").manual_seed(n)
    X = torch.rand(batch, n, n, dtype=torch.float64, device="cuda", generator=g) - 0.5
    return torch.bmm(X, X.transpose(1, 2)) + n * torch.eye(n, dtype=torch.float64, device="cuda")


def run(items, a, T, inner):
    t = {k: [] for k, _ in items}
    for rep in range(a.reps + 1):
        for k, fn in items:
            t[k].append(T(fn, inner))
    return {k: stats(v) for k, v in t.items()}


def group1(L, a, T, sp):
    say("1. symm (alpha = 1, beta = 0) at nrhs = 1 and 16, and norm1; per-call times in ms, median [fastest slowest] for the calls, medians for "
        "(a) torch.bmm on full symmetric copies and (b) the device-to-device copy of the batch's bytes")
    say("%4s %6s  %-30s %9s %7s  %-30s %9s %7s  %-30s %9s %7s" % ("n", "blocks", "symm nrhs 1", "(a)", "(a)/it", "symm nrhs 16", "(a)", "(a)/it",
                                                                 "norm1", "(b)", "(b)/it"))
    losses = []
    for n in a.sizes:
        for batch in (1024, big_batch(n)):
            A = spd(batch, n)
            Ac = torch.empty_like(A)
            X = {k: torch.rand(batch, k, n, dtype=torch.float64, device="cuda") - 0.5 for k in (1, 16)}
            Y = {k: torch.empty_like(X[k]) for k in (1, 16)}
            Xt = {k: X[k].transpose(1, 2).contiguous() for k in (1, 16)}
            Yt = {k: torch.empty_like(Xt[k]) for k in (1, 16)}
            out = torch.zeros(batch, dtype=torch.float64, device="cuda")
            inner = a.inner if batch * n * n < (1 << 26) else 2

            def symm(k):
                _lib.check(L.cap_dsymm_batched(1, 0, n, k, 1.0, A.data_ptr(), n, n * n, X[k].data_ptr(), n, n * k, 0.0, None, n, n * k, Y[k].data_ptr(), n,
                                               n * k, batch, sp))
            r = run((("s1", lambda: symm(1)), ("b1", lambda: torch.bmm(A, Xt[1], out=Yt[1])), ("s16", lambda: symm(16)),
                     ("b16", lambda: torch.bmm(A, Xt[16], out=Yt[16])),
                     ("nm", lambda: _lib.check(L.cap_dlansy_batched(ONE, 1, n, A.data_ptr(), n, n * n, batch, out.data_ptr(), sp))),
                     ("cp", lambda: Ac.copy_(A))), a, T, inner)
            f = lambda s: "%9.4f [%8.4f %8.4f]" % s
            say("%4d %6d  %s %9.4f %7.2f  %s %9.4f %7.2f  %s %9.4f %7.2f" % (
                n, batch, f(r["s1"]), r["b1"][0], r["b1"][0] / r["s1"][0], f(r["s16"]), r["b16"][0], r["b16"][0] / r["s16"][0], f(r["nm"]), r["cp"][0],
                r["cp"][0] / r["nm"][0]))
            for key, ref, what in (("s1", "b1", "symm nrhs 1 / bmm"), ("s16", "b16", "symm nrhs 16 / bmm"), ("nm", "cp", "norm1 / copy")):
                if r[key][0] > r[ref][0] + max(r[key][2] - r[key][1], r[ref][2] - r[ref][1]):
                    losses.append((n, batch, what, round(r[key][0] / r[ref][0], 2)))
            del A, Ac, X, Y, Xt, Yt
            torch.cuda.empty_cache()
    say("rows that LOSE by more than the row's own spread (n, blocks, what, ratio): %s" % (losses if losses else "none"))
    say()


def group2(L, a, T, sp):
    say("2. rcond (cap_dlansy_batched beforehand, not counted) against the potri call it contains, torch.linalg.cond(., 1) on full copies, and the "
        "host loop over cap_dlansy + cap_dpocon (timed on %d blocks, scaled to the batch); per-call times in ms" % a.loop_blocks)
    say("%4s %6s  %-30s %9s %9s %11s  %9s %9s %9s" % ("n", "blocks", "rcond", "potri", "cond_1", "loop", "rcond/potri", "cond_1/rcond", "loop/rcond"))
    failed = []
    for n in a.sizes:
        for batch in (1024, big_batch(n)):
            A = spd(batch, n)
            R, Rc = A.clone(), torch.empty_like(A)
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            an, rc = torch.zeros(batch, dtype=torch.float64, device="cuda"), torch.zeros(batch, dtype=torch.float64, device="cuda")
            _lib.check(L.cap_dlansy_batched(ONE, 1, n, A.data_ptr(), n, n * n, batch, an.data_ptr(), sp))
            _lib.check(L.cap_dpotrf_batched_blocked(1, n, R.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
            work = torch.empty(max(int(L.cap_dpocon_batched_work_size(n, batch)), 1), dtype=torch.float64, device="cuda")
            inner = a.inner if batch * n * n < (1 << 26) else 2
            lb = min(a.loop_blocks, batch)
            w1 = torch.empty(int(L.cap_dlansy_work_size(n)) + int(L.cap_dpocon_work_size(n)) + 8, dtype=torch.float64, device="cuda")

            def potri():
                Rc.copy_(R)
                _lib.check(L.cap_dpotri_batched(1, n, Rc.data_ptr(), n, n * n, batch, info.data_ptr(), 0, sp))

            def loop():
                for i in range(lb):
                    _lib.check(L.cap_dlansy(ONE, 1, n, A.data_ptr() + 8 * i * n * n, n, an.data_ptr() + 8 * i, w1.data_ptr(), sp))
                    _lib.check(L.cap_dpocon(1, n, R.data_ptr() + 8 * i * n * n, n, an.data_ptr() + 8 * i, rc.data_ptr() + 8 * i, w1.data_ptr(), sp))
            items = [("rc", lambda: _lib.check(L.cap_dpocon_batched(1, n, R.data_ptr(), n, n * n, batch, an.data_ptr(), info.data_ptr(), rc.data_ptr(),
                                                                    work.data_ptr(), sp))),
                     ("pi", potri), ("cp", lambda: Rc.copy_(R))]
            try:                                                                 # (torch's batched LU can refuse a shape: the row then says so)
                torch.linalg.cond(A, 1)
                items.append(("tc", lambda: torch.linalg.cond(A, 1)))
            except RuntimeError as e:
                failed.append((n, batch, str(e).split("\n")[0][:120]))
            r = run(items, a, T, inner)
            r.setdefault("tc", (float("nan"),) * 3)
            lt = stats([T(loop, 1) for _ in range(4)])[0] * batch / lb
            pi = r["pi"][0] - r["cp"][0]
            say("%4d %6d  %9.4f [%8.4f %8.4f] %9.4f %9.4f %11.2f  %9.2f %9.2f %9.1f" % (
                n, batch, r["rc"][0], r["rc"][1], r["rc"][2], pi, r["tc"][0], lt, r["rc"][0] / pi, r["tc"][0] / r["rc"][0], lt / r["rc"][0]))
            del A, R, Rc, work
            torch.cuda.empty_cache()
    say("(potri = (copy, potri) - (copy): the batched inverse is in place, so its window holds a restoring copy)")
    if failed:
        say("torch.linalg.cond(., 1) raised at (n, blocks, message): %s" % failed)
    say()


def group3(L, a, T, sp):
    say("3. error_bounds against the potrs it judges; per-call times in ms, median [fastest slowest] for ferr + berr, medians for the rest")
    say("%4s %4s %6s  %-30s %9s %9s  %9s %9s" % ("n", "nrhs", "blocks", "ferr + berr", "berr alone", "potrs", "both/potrs", "berr/potrs"))
    for n in a.sizes:
        for batch in (1024, big_batch(n)):
            A = spd(batch, n)
            R = A.clone()
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            _lib.check(L.cap_dpotrf_batched_blocked(1, n, R.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
            inner = a.inner if batch * n * n < (1 << 26) else 2
            for k in (1, 16):
                B = torch.rand(batch, k, n, dtype=torch.float64, device="cuda") - 0.5
                X = B.clone()
                _lib.check(L.cap_dpotrs_batched_blocked(1, n, k, R.data_ptr(), n, n * n, X.data_ptr(), n, n * k, batch, info.data_ptr(), sp))
                Xs = X.clone()
                fe, be = torch.zeros(batch * k, dtype=torch.float64, device="cuda"), torch.zeros(batch * k, dtype=torch.float64, device="cuda")
                work = torch.empty(max(int(L.cap_dpoerr_batched_work_size(n, k, batch)), 1), dtype=torch.float64, device="cuda")

                def bounds(want):
                    _lib.check(L.cap_dpoerr_batched(1, n, k, A.data_ptr(), n, n * n, R.data_ptr(), n, n * n, B.data_ptr(), n, n * k, X.data_ptr(), n, n * k,
                                                    batch, info.data_ptr(), fe.data_ptr() if want else None, be.data_ptr(), k, work.data_ptr(), sp))
                r = run((("fb", lambda: bounds(1)), ("b", lambda: bounds(0)),
                         ("ps", lambda: _lib.check(L.cap_dpotrs_batched_blocked(1, n, k, R.data_ptr(), n, n * n, Xs.data_ptr(), n, n * k, batch,
                                                                                info.data_ptr(), sp)))), a, T, inner)
                say("%4d %4d %6d  %9.4f [%8.4f %8.4f] %9.4f %9.4f  %9.2f %9.2f" % (n, k, batch, r["fb"][0], r["fb"][1], r["fb"][2], r["b"][0], r["ps"][0],
                                                                                 r["fb"][0] / r["ps"][0], r["b"][0] / r["ps"][0]))
                del B, X, Xs, work
            del A, R
            torch.cuda.empty_cache()
    say()


def group4(L, a, T, sp):
    rng = np.random.default_rng([22, 4096, 2])                                  # mixed_sizes("block-Jacobi mix", 4096) of tools/potrf_vbatched_bench.py
    small = rng.random(4096) < 0.8
    sizes = np.where(small, rng.integers(1, 17, size=4096), rng.integers(100, 201, size=4096))
    batch = len(sizes)
    arr = (C.c_int64 * batch)(*[int(x) for x in sizes])
    plan = C.c_void_p()
    _lib.check(L.cap_vbatch_plan_create(batch, arr, None, None, C.byref(plan)), "cap_vbatch_plan_create")
    launches, rows, total = int(L.cap_vbatch_plan_info(plan, 4)), int(sizes.sum()), int((sizes * sizes).sum())
    A = torch.zeros(total, dtype=torch.float64, device="cuda")
    at = 0
    for n in sizes:                                                              # diagonally dominant blocks: SPD, the factor exists
        n = int(n)
        A[at:at + n * n].view(n, n).copy_(torch.eye(n, dtype=torch.float64, device="cuda") * (n + 1.0) + 0.5)
        at += n * n
    R = A.clone()
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    _lib.check(L.cap_dpotrf_vbatched(plan, 1, R.data_ptr(), info.data_ptr(), None, sp))
    B = torch.rand(rows, dtype=torch.float64, device="cuda") - 0.5
    X, Y = B.clone(), torch.empty_like(B)
    _lib.check(L.cap_dpotrs_vbatched(plan, 1, 1, R.data_ptr(), X.data_ptr(), rows, info.data_ptr(), sp))
    Xs = X.clone()
    an, rc, fe, be = (torch.zeros(batch, dtype=torch.float64, device="cuda") for _ in range(4))
    work = torch.empty(int(L.cap_dpoerr_vbatched_work_size(plan, 1)), dtype=torch.float64, device="cuda")
    Rc = torch.empty_like(R)
    say("4. block-Jacobi mix, %d blocks (%d rows, %.1f MB of blocks, %d launches per plan call of the older entries); nrhs = 1; per-call times in ms, "
        "median [fastest slowest]" % (batch, rows, total * 8 / 1e6, launches))

    def potri():
        Rc.copy_(R)
        _lib.check(L.cap_dpotri_vbatched(plan, 1, Rc.data_ptr(), info.data_ptr(), 0, sp))
    r = run((("symm", lambda: _lib.check(L.cap_dsymm_vbatched(plan, 1, 0, 1, 1.0, A.data_ptr(), X.data_ptr(), rows, 0.0, None, rows, Y.data_ptr(), rows, sp))),
             ("norm1", lambda: _lib.check(L.cap_dlansy_vbatched(plan, ONE, 1, A.data_ptr(), an.data_ptr(), sp))),
             ("rcond", lambda: _lib.check(L.cap_dpocon_vbatched(plan, 1, R.data_ptr(), an.data_ptr(), info.data_ptr(), rc.data_ptr(), work.data_ptr(), sp))),
             ("error_bounds", lambda: _lib.check(L.cap_dpoerr_vbatched(plan, 1, 1, A.data_ptr(), R.data_ptr(), B.data_ptr(), rows, X.data_ptr(), rows,
                                                                       info.data_ptr(), fe.data_ptr(), be.data_ptr(), 1, work.data_ptr(), sp))),
             ("berr alone", lambda: _lib.check(L.cap_dpoerr_vbatched(plan, 1, 1, A.data_ptr(), R.data_ptr(), B.data_ptr(), rows, X.data_ptr(), rows,
                                                                     info.data_ptr(), None, be.data_ptr(), 1, None, sp))),
             ("potrs", lambda: _lib.check(L.cap_dpotrs_vbatched(plan, 1, 1, R.data_ptr(), Xs.data_ptr(), rows, info.data_ptr(), sp))),
             ("copy + potri", potri), ("copy", lambda: Rc.copy_(R))), a, T, a.inner)
    for k, v in r.items():
        say("   %-14s %9.4f [%8.4f %8.4f]" % (k, v[0], v[1], v[2]))
    say()
    L.cap_vbatch_plan_destroy(plan)


def group5(L, a, T, sp, path):
    P = C.CDLL(path)
    for name in ("cap_dpotri_batched", "cap_dpotrs_batched_blocked", "cap_dsyrk_batched"):
        sig = _lib.SIGNATURES[name]
        getattr(P, name).restype, getattr(P, name).argtypes = sig[0], sig[1]
    say("5. cap_dpotri_batched, cap_dpotrs_batched_blocked (16 right-hand sides) and cap_dsyrk_batched (k = 16) of this build and of the parent "
        "commit's build, alternating in this process; 1024 blocks, per-call times in ms, median [fastest slowest]")
    say("%4s %-6s  %-30s %-30s %8s %s" % ("n", "entry", "this build", "parent build", "this/par", "within the spread"))
    moved = []
    for n in a.sizes:
        batch, k = 1024, 16
        A0 = spd(batch, n)
        R = A0.clone()
        info = torch.zeros(batch, dtype=torch.int32, device="cuda")
        _lib.check(L.cap_dpotrf_batched_blocked(1, n, R.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
        Rc = R.clone()
        B = torch.rand(batch, k, n, dtype=torch.float64, device="cuda") - 0.5
        for entry in ("potri", "potrs", "syrk"):
            t = {"new": [], "old": []}
            for rep in range(a.reps + 1):
                for key, lib in (("new", L), ("old", P)):
                    if entry == "potri":
                        def fn():
                            Rc.copy_(R)
                            _lib.check(lib.cap_dpotri_batched(1, n, Rc.data_ptr(), n, n * n, batch, info.data_ptr(), 0, sp))
                    elif entry == "potrs":
                        def fn():
                            _lib.check(lib.cap_dpotrs_batched_blocked(1, n, k, R.data_ptr(), n, n * n, B.data_ptr(), n, n * k, batch, info.data_ptr(), sp))
                    else:
                        def fn():
                            _lib.check(lib.cap_dsyrk_batched(1, 0, n, k, 1.0, B.data_ptr(), n, n * k, 0.0, Rc.data_ptr(), n, n * n, None, 0, batch, sp))
                    t[key].append(T(fn, a.inner))
            x, y = stats(t["new"]), stats(t["old"])
            ok = abs(x[0] - y[0]) <= max(x[2] - x[1], y[2] - y[1])
            if not ok:
                moved.append((n, entry, round(x[0] / y[0], 3)))
            say("%4d %-6s  %9.4f [%8.4f %8.4f] %9.4f [%8.4f %8.4f] %8.3f %s" % (n, entry, x[0], x[1], x[2], y[0], y[1], y[2], x[0] / y[0], "yes" if ok else "NO"))
    say("the existing entries within the run's own spread of the parent's time at every row: %s (potri's windows include the restoring copy)" % (
        "yes" if not moved else "NO - %s" % moved))
    say()


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for name, v in sorted(build.kernel_resources().items()):
        if "symm_" in name and ("batched" in name or "copy_upper" in name or "rcond" in name):
            say("  %-74s VGPRs %3s  AGPRs %3s  scratch %s  LDS %6s B  waves/SIMD %s" % (
                name, v.get("VGPRs"), v.get("AGPRs"), v.get("ScratchSize"), v.get("LDS Size"), v.get("Occupancy")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sizes", default="8,16,32,64,96,128,192,256")
    ap.add_argument("--groups", default="1,2,3,4,5")
    ap.add_argument("--loop-blocks", type=int, default=32)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_symm_batched.txt"))
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    groups = a.groups.split(",")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT[0] = open(a.out, "w")
    L = _lib.lib()
    T = Timer()
    sp = T.s.cuda_stream
    say("Batched symmetric products, 1-norms, exact rcond and solve error bounds (csrc/symm_batched.hip) - round 26")
    say("tools/symm_batched_bench.py on one %s, torch %s, ONE run, %d windows of %d calls (2 for the heaviest rows) after a warm-up round, every window "
        "between two stream events" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.inner))
    say()
    if "1" in groups:
        group1(L, a, T, sp)
    if "2" in groups:
        group2(L, a, T, sp)
    if "3" in groups:
        group3(L, a, T, sp)
    if "4" in groups:
        group4(L, a, T, sp)
    if "5" in groups and a.parent_lib:
        group5(L, a, T, sp, a.parent_lib)
    resources()
    OUT[0].close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
