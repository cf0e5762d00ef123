"""Time the batched triangular solves and products on Cholesky factors (cap_dtrsm_batched / cap_dtrmm_batched and their plan forms,
csrc/trsm_batched.hip).

One run; every item is a window between two stream events that holds `inner` back-to-back calls (the per-call time is window / inner), the
items of a row alternating in one process, median of --reps windows after one warm-up round, fastest and slowest beside it.  B is restored
from a copy in front of every window (not counted), so no item sees another one's values.
  1. FIXED SIZE: n in 8 .. 256, nrhs in 1, 16, at 1024 blocks and at 65536 (n <= 32) / 16384 (n = 64) / 4096 (n > 64) blocks, both trans
     values: trsm, trsm with sumsq, trmm, against
       (a) cap_dpotrs_batched_blocked on the same operands - the route a caller had to take (both substitutions),
       (b) torch.linalg.solve_triangular on the same factors, and for the products torch.matmul with torch.tril,
       (c) a device-to-device copy of R plus B.
     A row where trsm is slower than (a) by more than the run's own spread of that row (slowest - fastest window) is listed at the end.
  2. THE MIXED BLOCK-JACOBI BATCH of tools/potrf_vbatched_bench.py (80 % n <= 16, 20 % n in 100..200; 4096 blocks) through a plan:
     cap_dtrsm_vbatched (both trans values, with and without sumsq) and cap_dtrmm_vbatched against cap_dpotrs_vbatched.
  3. with --parent-lib: cap_dpotrs_batched_blocked of this build and of another build of the library (the parent commit's), alternating
     in this process on the operands of section 1 at 1024 blocks - the existing entry must not have moved.
The factors are random upper triangles with n + 1 on the diagonal; the time of these kernels does not depend on the data.  Writes the table
to --out and prints it:

    timeout -k 10 900 python tools/trsm_batched_bench.py [--reps 9] [--out profiles/r24_trsm_batched.txt] [--parent-lib path/to/libcapital_amd.so]
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


def factors(batch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    R = torch.rand(batch, n, n, dtype=torch.float64, device="cuda", generator=g) - 0.5
    R.diagonal(dim1=1, dim2=2).fill_(float(n + 1))
    return R


def big_batch(n):
    return 65536 if n <= 32 else 16384 if n == 64 else 4096


def group1(L, a, T, sp):
    say("1. fixed size; per-call times in ms, median [fastest slowest] for trsm, medians for the rest; (a) cap_dpotrs_batched_blocked, (b) "
        "torch.linalg.solve_triangular / torch.matmul(tril), (c) device-to-device copy of R plus B")
    say("%4s %4s %6s %2s  %-30s %9s %9s %9s %9s %9s %9s  %8s %8s %8s" % (
        "n", "nrhs", "blocks", "op", "cap_dtrsm_batched", "+sumsq", "trmm", "(a)", "(b)solve", "(b)mm", "(c)", "(a)/trsm", "(b)/trsm", "trsm/(c)"))
    slower = []
    for n in a.sizes:
        for batch in (1024, big_batch(n)):
            R = factors(batch, n, n)                 # torch reads block i as L = R_i^T (lower)
            Rc = torch.empty_like(R)
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            for nrhs in (1, 16):
                B0 = torch.rand(batch, nrhs, n, dtype=torch.float64, device="cuda") - 0.5
                B, Bc = B0.clone(), torch.empty_like(B0)
                Bt = B0.transpose(1, 2).contiguous()          # (batch, n, nrhs) for torch
                q = torch.zeros(batch, nrhs, dtype=torch.float64, device="cuda")
                inner = a.inner
                tin = max(1, inner // 4)
                for trans in (T_, N_):
                    Lt = R if trans else R.transpose(1, 2)

                    def trsm(qq=None):
                        _lib.check(L.cap_dtrsm_batched(1, trans, n, nrhs, R.data_ptr(), n, n * n, B.data_ptr(), n, n * nrhs, batch, info.data_ptr(),
                                                       qq, nrhs, sp))

                    def trmm():
                        _lib.check(L.cap_dtrmm_batched(1, trans, n, nrhs, R.data_ptr(), n, n * n, B.data_ptr(), n, n * nrhs, batch, info.data_ptr(), sp))

                    def potrs():
                        _lib.check(L.cap_dpotrs_batched_blocked(1, n, nrhs, R.data_ptr(), n, n * n, B.data_ptr(), n, n * nrhs, batch, info.data_ptr(), sp))

                    def copy():
                        Rc.copy_(R)
                        Bc.copy_(B0)
                    t = {x: [] for x in ("s", "q", "m", "a", "bs", "bm", "c")}
                    for rep in range(a.reps + 1):
                        for key, fn, inn in (("s", trsm, inner), ("q", lambda: trsm(q.data_ptr()), inner), ("m", trmm, inner), ("a", potrs, inner),
                                             ("bs", lambda: torch.linalg.solve_triangular(Lt, Bt, upper=not trans), tin),
                                             ("bm", lambda: torch.matmul(torch.tril(Lt) if trans else torch.triu(Lt), Bt), tin), ("c", copy, inner)):
                            B.copy_(B0)
                            t[key].append(T(fn, inn))
                    s, sq, m, pa, bs, bm, c = (stats(t[k]) for k in ("s", "q", "m", "a", "bs", "bm", "c"))
                    say("%4d %4d %6d %2s  %9.4f [%8.4f %8.4f] %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f  %8.2f %8.2f %8.2f" % (
                        n, nrhs, batch, "T" if trans else "N", s[0], s[1], s[2], sq[0], m[0], pa[0], bs[0], bm[0], c[0], pa[0] / s[0], bs[0] / s[0],
                        s[0] / c[0]))
                    spread = max(s[2] - s[1], pa[2] - pa[1])
                    if s[0] > pa[0] + spread:
                        slower.append((n, nrhs, batch, "T" if trans else "N", round(s[0] / pa[0], 3)))
                del B0, B, Bc, Bt, q
            del R, Rc
            torch.cuda.empty_cache()
    say("rows where trsm is slower than potrs (a) by more than the row's own spread: %s" % (slower if slower else "none"))
    say()
    return slower


def group2(L, a, T, sp):
    rng = np.random.default_rng([22, 4096, 2])                                  # mixed_sizes("block-Jacobi mix", 4096) of tools/potrf_vbatched_bench.py
    small = rng.random(4096) < 0.8
    sizes = np.where(small, rng.integers(1, 17, size=4096), rng.integers(100, 201, size=4096))
    batch = len(sizes)
    arr = (C.c_int64 * batch)(*[int(x) for x in sizes])
    plan = C.c_void_p()
    _lib.check(L.cap_vbatch_plan_create(batch, arr, None, None, C.byref(plan)), "cap_vbatch_plan_create")
    launches, rows, total = int(L.cap_vbatch_plan_info(plan, 4)), int(sizes.sum()), int((sizes * sizes).sum())
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(total, dtype=torch.float64, device="cuda", generator=g) - 0.5
    off = np.concatenate([[0], np.cumsum(sizes * sizes)[:-1]])
    for n in np.unique(sizes):                                                  # n + 1 on every diagonal
        idx = torch.from_numpy(off[sizes == n]).cuda()
        A[(idx[:, None] + torch.arange(int(n), device="cuda")[None, :] * (int(n) + 1)).reshape(-1)] = float(n + 1)
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    say("2. block-Jacobi mix, %d blocks (%d rows, %.1f MB of factors, %d launches per call); per-call times in ms, median [fastest slowest]" % (
        batch, rows, total * 8 / 1e6, launches))
    for nrhs in (1, 16):
        B0 = torch.rand(nrhs, rows, dtype=torch.float64, device="cuda") - 0.5
        B = B0.clone()
        q = torch.zeros(batch, nrhs, dtype=torch.float64, device="cuda")
        items = [("cap_dpotrs_vbatched", lambda: L.cap_dpotrs_vbatched(plan, 1, nrhs, A.data_ptr(), B.data_ptr(), rows, info.data_ptr(), sp))]
        for trans in (T_, N_):
            tag = "T" if trans else "N"
            items.append(("cap_dtrsm_vbatched %s" % tag, lambda trans=trans: L.cap_dtrsm_vbatched(plan, 1, trans, nrhs, A.data_ptr(), B.data_ptr(), rows,
                                                                                                   info.data_ptr(), None, 0, sp)))
            items.append(("cap_dtrsm_vbatched %s + sumsq" % tag, lambda trans=trans: L.cap_dtrsm_vbatched(plan, 1, trans, nrhs, A.data_ptr(), B.data_ptr(),
                                                                                                           rows, info.data_ptr(), q.data_ptr(), nrhs, sp)))
            items.append(("cap_dtrmm_vbatched %s" % tag, lambda trans=trans: L.cap_dtrmm_vbatched(plan, 1, trans, nrhs, A.data_ptr(), B.data_ptr(), rows,
                                                                                                   info.data_ptr(), sp)))
        t = {name: [] for name, _ in items}
        for rep in range(a.reps + 1):
            for name, fn in items:
                B.copy_(B0)
                t[name].append(T(lambda: _lib.check(fn()), a.inner))
        base = stats(t["cap_dpotrs_vbatched"])[0]
        for name, _ in items:
            s = stats(t[name])
            say("   nrhs %2d  %-32s %9.4f [%8.4f %8.4f]   potrs / this %.2f" % (nrhs, name, s[0], s[1], s[2], base / s[0]))
    say()
    L.cap_vbatch_plan_destroy(plan)


def group3(L, a, T, sp, path):
    P = C.CDLL(path)
    sig = _lib.SIGNATURES["cap_dpotrs_batched_blocked"]
    P.cap_dpotrs_batched_blocked.restype, P.cap_dpotrs_batched_blocked.argtypes = sig[0], sig[1]
    say("3. cap_dpotrs_batched_blocked of this build and of the parent commit's build, alternating in this process; 1024 blocks, per-call times in ms, "
        "median [fastest slowest]")
    say("%4s %4s  %-30s %-30s %8s %s" % ("n", "nrhs", "this build", "parent build", "this/par", "within the spread"))
    moved = []
    for n in a.sizes:
        batch = 1024
        R = factors(batch, n, n)
        info = torch.zeros(batch, dtype=torch.int32, device="cuda")
        for nrhs in (1, 16):
            B0 = torch.rand(batch, nrhs, n, dtype=torch.float64, device="cuda") - 0.5
            B = B0.clone()
            t = {"new": [], "old": []}
            for rep in range(a.reps + 1):
                for key, lib in (("new", L), ("old", P)):
                    B.copy_(B0)
                    t[key].append(T(lambda: _lib.check(lib.cap_dpotrs_batched_blocked(1, n, nrhs, R.data_ptr(), n, n * n, B.data_ptr(), n, n * nrhs, batch,
                                                                                     info.data_ptr(), sp)), a.inner))
            x, y = stats(t["new"]), stats(t["old"])
            ok = abs(x[0] - y[0]) <= max(x[2] - x[1], y[2] - y[1])
            if not ok:
                moved.append((n, nrhs))
            say("%4d %4d  %9.4f [%8.4f %8.4f] %9.4f [%8.4f %8.4f] %8.3f %s" % (n, nrhs, x[0], x[1], x[2], y[0], y[1], y[2], x[0] / y[0], "yes" if ok else "NO"))
    say("the existing entry within the run's own spread of the parent's time at every row: %s" % ("yes" if not moved else "NO - %s" % moved))
    say()


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for name, v in sorted(build.kernel_resources().items()):
        if "tri_" in name and "batched" in name and "potri" not in name:
            say("  %-74s VGPRs %3s  AGPRs %3s  scratch %s  LDS %6s B  waves/SIMD %s" % (
                name, v.get("VGPRs"), v.get("AGPRs"), v.get("ScratchSize"), v.get("LDS Size"), v.get("Occupancy")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sizes", default="8,16,32,64,96,128,192,256")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_trsm_batched.txt"))
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT[0] = open(a.out, "w")
    L = _lib.lib()
    T = Timer()
    sp = T.s.cuda_stream
    say("Batched triangular solves and products on Cholesky factors (cap_dtrsm_batched / cap_dtrmm_batched / cap_dtrsm_vbatched / cap_dtrmm_vbatched, "
        "csrc/trsm_batched.hip) - round 24")
    say("tools/trsm_batched_bench.py on one %s, torch %s, ONE run, %d windows of %d calls after a warm-up round, every window between two "
        "stream events" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.inner))
    say()
    group1(L, a, T, sp)
    group2(L, a, T, sp)
    if a.parent_lib:
        group3(L, a, T, sp, a.parent_lib)
    resources()
    OUT[0].close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
