"""Time the batched pivoted Cholesky factorization (cap_dpstrf_batched, cap_dpstrf_vbatched, csrc/pstrf_batched.hip).

One run; every item is a window between two stream events that holds `inner` back-to-back calls (the per-call time is window / inner), the
items of a row alternating in one process, median of --reps windows after one warm-up round, fastest and slowest beside it.
  1. PSTRF at n = 8 / 16 / 32 / 64, at 1024 blocks and at 65536 (n <= 32) / 16384 (n = 64) blocks, on three kinds of blocks - full rank
     (`dominant`), rank n / 4 stopped by the tolerance (`gram`), full rank capped at max_rank = n / 4 (`capped`) - against
       (a) cap_dpotrf_batched on the same batch (a restoring copy in its window, subtracted): the pivoted call does the same n^3 / 6
           multiply-adds at full rank plus one cross-lane exchange per product.  No threshold is set; the rows it LOSES are named.
       (b) the host loop over cap_dpstrf (timed on --loop-blocks blocks and scaled to the batch: the loop's time is proportional to its length).
  2. A BLOCK-JACOBI-STYLE MIX within n <= 64 (80 % n <= 16, 20 % n in 33 .. 64; 4096 blocks) through a plan against one fixed-size call per
     occurring size on the same blocks.
  3. with --parent-lib: cap_dpotrf_batched of this build and of another build of the library (the parent commit's), alternating in this
     process at 1024 blocks - the existing entry must not have moved.
The time of the pivoted kernel DOES depend on the data (the rank), hence the three kinds.  Writes the table to --out and prints it:

    timeout -k 10 900 python tools/pstrf_batched_bench.py [--reps 9] [--out profiles/r27_pstrf_batched.txt] [--parent-lib path/to/libcapital_amd.so]
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
    return 65536 if n <= 32 else 16384


def blocks(kind, batch, n):
    """dominant: G G^T / 2n + diag in [1, 3] (full rank); gram: G G^T with G n x n / 4 (rank n / 4)"""
    g = torch.Generator(device="cuda").manual_seed(n)
    k = n if kind == "dominant" else max(n // 4, 1)
    X = torch.randn(batch, n, k, dtype=torch.float64, device="cuda", generator=g)
    A = torch.bmm(X, X.transpose(1, 2))
    if kind == "dominant":
        A = A / (2 * n) + torch.diag_embed(1.0 + 2.0 * torch.rand(batch, n, dtype=torch.float64, device="cuda", generator=g))
    return A.contiguous()


def run(items, a, T, inner):
    t = {k: [] for k, _ in items}
    for rep in range(a.reps + 1):
        for k, fn in items:
            t[k].append(T(fn, inner))
    return {k: stats(v) for k, v in t.items()}


class Outputs:
    def __init__(self, batch, n):
        z = lambda dt, m: torch.zeros(max(m, 1), dtype=dt, device="cuda")
        self.R, self.piv = z(torch.float64, batch * n * n), z(torch.int64, batch * n)
        self.rank, self.info, self.resid = z(torch.int32, batch), z(torch.int32, batch), z(torch.float64, batch)


def group1(L, a, T, sp):
    say("1. pstrf on full-rank blocks (dominant), on rank-n/4 blocks stopped by the default tolerance (gram) and on full-rank blocks capped at "
        "max_rank = n/4 (capped); per-call times in ms, median [fastest slowest]; potrf = cap_dpotrf_batched on the dominant batch (restoring "
        "copy subtracted), loop = the host loop over cap_dpstrf on %d dominant blocks scaled to the batch" % a.loop_blocks)
    say("%4s %6s  %-30s %-30s %-30s %9s %11s  %11s %11s %10s" % ("n", "blocks", "dominant", "gram", "capped", "potrf", "loop", "dominant/potrf",
                                                                "gram/potrf", "loop/dominant"))
    losses, ranks = [], []
    for n in a.sizes:
        for batch in (1024, big_batch(n)):
            A, Gm = blocks("dominant", batch, n), blocks("gram", batch, n)
            Ac = torch.empty_like(A)
            o = Outputs(batch, n)
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            inner = a.inner if batch * n * n < (1 << 26) else 2
            cap = max(n // 4, 1)

            def pstrf(M, mr):
                _lib.check(L.cap_dpstrf_batched(1, n, mr, -1.0, M.data_ptr(), n, n * n, o.R.data_ptr(), max(mr, 1), mr * n, o.piv.data_ptr(),
                                                o.rank.data_ptr(), o.resid.data_ptr(), None, o.info.data_ptr(), batch, sp))

            def potrf():
                Ac.copy_(A)
                _lib.check(L.cap_dpotrf_batched(1, n, Ac.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
            pstrf(Gm, n)
            gr = o.rank.clone()
            pstrf(A, n)
            ranks.append((n, batch, int(o.rank.min()), int(o.rank.max()), int(gr.min()), int(gr.max())))
            lb = min(a.loop_blocks, batch)
            w1 = torch.empty(int(L.cap_dpstrf_work_size(n, n)) + 8, dtype=torch.float64, device="cuda")
            rank1 = torch.zeros(lb, dtype=torch.int64, device="cuda")

            def loop():
                for i in range(lb):
                    _lib.check(L.cap_dpstrf(1, n, n, -1.0, A.data_ptr() + 8 * i * n * n, n, o.R.data_ptr() + 8 * i * n * n, n, o.piv.data_ptr() + 8 * i * n,
                                            rank1.data_ptr() + 8 * i, o.resid.data_ptr() + 8 * i, o.info.data_ptr() + 4 * i, w1.data_ptr(), sp))
            r = run((("dom", lambda: pstrf(A, n)), ("gram", lambda: pstrf(Gm, n)), ("cap", lambda: pstrf(A, cap)), ("pf", potrf),
                     ("cp", lambda: Ac.copy_(A))), a, T, inner)
            lt = stats([T(loop, 1) for _ in range(4)])[0] * batch / lb
            pf = r["pf"][0] - r["cp"][0]
            f = lambda s: "%9.4f [%8.4f %8.4f]" % s
            say("%4d %6d  %s %s %s %9.4f %11.2f  %11.2f %11.2f %10.1f" % (n, batch, f(r["dom"]), f(r["gram"]), f(r["cap"]), pf, lt, r["dom"][0] / pf,
                                                                          r["gram"][0] / pf, lt / r["dom"][0]))
            spread = max(r["dom"][2] - r["dom"][1], r["pf"][2] - r["pf"][1])
            for key, what in (("dom", "dominant"), ("gram", "gram"), ("cap", "capped")):
                if r[key][0] > pf + spread:
                    losses.append((n, batch, what, round(r[key][0] / pf, 2)))
            del A, Gm, Ac, o
            torch.cuda.empty_cache()
    say("rows where the pivoted call LOSES to potrf by more than the row's own spread (n, blocks, kind, ratio): %s" % (losses if losses else "none"))
    say("ranks found (n, blocks, dominant min, max, gram min, max): %s" % ranks)
    say()


def group2(L, a, T, sp):
    rng = np.random.default_rng([27, 4096, 2])
    small = rng.random(4096) < 0.8
    sizes = np.where(small, rng.integers(1, 17, size=4096), rng.integers(33, 65, size=4096))
    batch = len(sizes)
    arr = (C.c_int64 * batch)(*[int(x) for x in sizes])
    plan = C.c_void_p()
    _lib.check(L.cap_vbatch_plan_create(batch, arr, None, None, C.byref(plan)), "cap_vbatch_plan_create")
    launches, rows, total = int(L.cap_vbatch_plan_info(plan, 4)), int(sizes.sum()), int((sizes * sizes).sum())
    A = torch.zeros(total, dtype=torch.float64, device="cuda")
    per = {}                                                                     # the same blocks grouped by size for the fixed-size calls
    at = 0
    g = torch.Generator(device="cuda").manual_seed(27)
    for n in sizes:
        n = int(n)
        X = torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g)
        M = X @ X.T / (2 * n) + torch.diag(1.0 + 2.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=g))
        A[at:at + n * n].view(n, n).copy_(M)
        per.setdefault(n, []).append(M)
        at += n * n
    per = {n: torch.stack(v).contiguous() for n, v in per.items()}
    R = torch.zeros_like(A)
    piv = torch.zeros(rows, dtype=torch.int64, device="cuda")
    rank, info = torch.zeros(batch, dtype=torch.int32, device="cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")
    resid = torch.zeros(batch, dtype=torch.float64, device="cuda")
    outs = {n: Outputs(v.shape[0], n) for n, v in per.items()}
    say("2. block-Jacobi-style mix within n <= 64, %d full-rank blocks (%d rows, %.1f MB of blocks): the plan call (%d launches) against one "
        "fixed-size call per occurring size (%d launches) on the same blocks; per-call times in ms, median [fastest slowest]"
        % (batch, rows, total * 8 / 1e6, launches, len(per)))

    def fixed():
        for n, M in per.items():
            o = outs[n]
            _lib.check(L.cap_dpstrf_batched(1, n, n, -1.0, M.data_ptr(), n, n * n, o.R.data_ptr(), n, n * n, o.piv.data_ptr(), o.rank.data_ptr(),
                                            o.resid.data_ptr(), None, o.info.data_ptr(), M.shape[0], sp))
    r = run((("plan", lambda: _lib.check(L.cap_dpstrf_vbatched(plan, 1, 64, -1.0, A.data_ptr(), R.data_ptr(), piv.data_ptr(), rank.data_ptr(),
                                                              resid.data_ptr(), None, info.data_ptr(), sp))),
             ("per size", fixed)), a, T, a.inner)
    for k, v in r.items():
        say("   %-10s %9.4f [%8.4f %8.4f]" % (k, v[0], v[1], v[2]))
    say("   per size / plan %.2f" % (r["per size"][0] / r["plan"][0]))
    say()
    L.cap_vbatch_plan_destroy(plan)


def group3(L, a, T, sp, path):
    P = C.CDLL(path)
    sig = _lib.SIGNATURES["cap_dpotrf_batched"]
    P.cap_dpotrf_batched.restype, P.cap_dpotrf_batched.argtypes = sig[0], sig[1]
    say("3. cap_dpotrf_batched of this build and of the parent commit's build, alternating in this process; 1024 blocks, per-call times in ms "
        "(the window holds a restoring copy), median [fastest slowest]")
    say("%4s  %-30s %-30s %8s %s" % ("n", "this build", "parent build", "this/par", "within the spread"))
    moved = []
    for n in a.sizes:
        batch = 1024
        A = blocks("dominant", batch, n)
        Ac = torch.empty_like(A)
        info = torch.zeros(batch, dtype=torch.int32, device="cuda")
        t = {"new": [], "old": []}
        for rep in range(a.reps + 1):
            for key, lib in (("new", L), ("old", P)):
                def fn():
                    Ac.copy_(A)
                    _lib.check(lib.cap_dpotrf_batched(1, n, Ac.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))
                t[key].append(T(fn, a.inner))
        x, y = stats(t["new"]), stats(t["old"])
        ok = abs(x[0] - y[0]) <= max(x[2] - x[1], y[2] - y[1])
        if not ok:
            moved.append((n, round(x[0] / y[0], 3)))
        say("%4d  %9.4f [%8.4f %8.4f] %9.4f [%8.4f %8.4f] %8.3f %s" % (n, x[0], x[1], x[2], y[0], y[1], y[2], x[0] / y[0], "yes" if ok else "NO"))
    say("potrf within the run's own spread of the parent's time at every row: %s" % ("yes" if not moved else "NO - %s" % moved))
    say()


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for name, v in sorted(build.kernel_resources().items()):
        if "pstrf_batched_kernel" in name or "pstrf_vbatched_kernel" in name:
            say("  %-70s VGPRs %3s  scratch %s  LDS %6s B  waves/SIMD %s" % (name, v.get("VGPRs"), v.get("ScratchSize"), v.get("LDS Size"),
                                                                           v.get("Occupancy")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sizes", default="8,16,32,64")
    ap.add_argument("--groups", default="1,2,3")
    ap.add_argument("--loop-blocks", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_pstrf_batched.txt"))
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    groups = a.groups.split(",")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT[0] = open(a.out, "w")
    L = _lib.lib()
    T = Timer()
    sp = T.s.cuda_stream
    say("Batched pivoted Cholesky for semidefinite blocks, n <= 64 (csrc/pstrf_batched.hip) - round 27")
    say("tools/pstrf_batched_bench.py on one %s, torch %s, ONE run, %d windows of %d calls (2 for the heaviest rows) after a warm-up round, every window "
        "between two stream events" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.inner))
    say()
    if "1" in groups:
        group1(L, a, T, sp)
    if "2" in groups:
        group2(L, a, T, sp)
    if "3" in groups and a.parent_lib:
        group3(L, a, T, sp, a.parent_lib)
    elif "3" in groups:
        say("3. cap_dpotrf_batched against the parent commit's build: not measured (no --parent-lib given)")
        say()
    resources()
    OUT[0].close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
