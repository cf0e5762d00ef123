"""Time the batched rank-k update of Cholesky factors (cap_dcholupdate_batched / cap_dcholupdate_vbatched, csrc/cholupdate_batched.hip).

One run; every item is a window between two stream events that holds `inner` back-to-back calls (the per-call time is window / inner), the
items of a row alternating in one process, median of --reps windows after one warm-up round, fastest and slowest beside it.
  1. FIXED SIZE: n in 8 .. 256, k in 1, 4, 16, at 1024 blocks and at 65536 (n <= 32) / 16384 (n = 64) / 4096 (n > 64) blocks, against
       (a) the loop over cap_dcholupdate on the same blocks (1024 blocks only; one window around the whole loop),
       (b) the route the update replaces when the matrices are at hand: cap_dpotrf_batched[_blocked] of pre-formed SPD blocks - FORMING
           A + V V^T IS NOT COUNTED,
       (c) a device-to-device copy of the batch of factors.
  2. THE MIXED BLOCK-JACOBI BATCH of tools/potrf_vbatched_bench.py (80 % n <= 16, 20 % n in 100..200; 4096 blocks) through a plan against
     one fixed-size call per distinct size on sub-batches gathered beforehand (the gather is not counted).
The factors are random upper triangles with n + 1 on the diagonal, V uniform in [-0.05, 0.05): the update (sign = +1) can be repeated in
place, and the time of these kernels does not depend on the data.  Writes the table to --out and prints it:

    timeout -k 10 900 python tools/cholupdate_batched_bench.py [--reps 9] [--out profiles/r23_cholupdate_batched.txt]
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


def factors(batch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    R = torch.rand(batch, n, n, dtype=torch.float64, device="cuda", generator=g) - 0.5
    R.diagonal(dim1=1, dim2=2).fill_(float(n + 1))
    return R


def big_batch(n):
    return 65536 if n <= 32 else 16384 if n == 64 else 4096


def group1(L, a, T, sp):
    say("1. fixed size, sign = +1; per-call times in ms, median [fastest slowest]; (a) loop over cap_dcholupdate, (b) potrf of pre-formed blocks "
        "(forming not counted), (c) device-to-device copy of the factors")
    say("%4s %3s %6s  %-30s %10s %10s %10s  %8s %8s %8s" % ("n", "k", "blocks", "cap_dcholupdate_batched", "(a)", "(b)", "(c)", "(a)/upd", "(b)/upd", "upd/(c)"))
    lost = []
    for n in a.sizes:
        fac = L.cap_dpotrf_batched if n <= 64 else L.cap_dpotrf_batched_blocked
        for batch in (1024, big_batch(n)):
            R0 = factors(batch, n, n)
            R, Rc = R0.clone(), torch.empty_like(R0)
            inner = a.inner
            nb = max(1, min(inner, (1 << 30) // (R0.numel() * 8)))
            S0 = R0 + R0.transpose(1, 2)                                       # symmetric, diagonally dominant: the blocks of route (b)
            S = [S0.clone() for _ in range(nb)]
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            work = torch.empty(max(L.cap_dcholupdate_work_size(n, 16), 1), dtype=torch.float64, device="cuda")
            one = torch.zeros(1, dtype=torch.int32, device="cuda")
            for k in (1, 4, 16):
                V = (torch.rand(batch, k, n, dtype=torch.float64, device="cuda") - 0.5) * 0.1
                t = {x: [] for x in "uabc"}

                def upd():
                    _lib.check(L.cap_dcholupdate_batched(1, 1, n, k, R.data_ptr(), n, n * n, V.data_ptr(), n, n * k, batch, info.data_ptr(), sp))

                def loop():
                    for i in range(batch):
                        _lib.check(L.cap_dcholupdate(1, 1, n, k, R.data_ptr() + 8 * i * n * n, n, V.data_ptr() + 8 * i * n * k, n, one.data_ptr(),
                                                     work.data_ptr(), sp))
                for rep in range(a.reps + 1):
                    R.copy_(R0)
                    t["u"].append(T(upd, inner))
                    if batch == 1024:
                        R.copy_(R0)
                        t["a"].append(T(loop))
                    for s in S:
                        s.copy_(S0)
                    it = iter(S)
                    t["b"].append(T(lambda: _lib.check(fac(1, n, next(it).data_ptr(), n, n * n, batch, info.data_ptr(), None, sp)), nb))
                    t["c"].append(T(lambda: Rc.copy_(R0), inner))
                u, b, c = stats(t["u"]), stats(t["b"])[0], stats(t["c"])[0]
                la = stats(t["a"])[0] if t["a"] else float("nan")
                say("%4d %3d %6d  %9.4f [%8.4f %8.4f] %10.4f %10.4f %10.4f  %8.1f %8.2f %8.2f" % (n, k, batch, u[0], u[1], u[2], la, b, c, la / u[0], b / u[0], u[0] / c))
                if batch == 1024 and not u[0] < la:
                    lost.append((n, k))
            assert not int(info.abs().max().item()), "an update or a factorization reported a failure"
            del R0, R, Rc, S0, S
            torch.cuda.empty_cache()
    say("at 1024 blocks the call is faster than loop (a) at every (n, k): %s" % ("yes" if not lost else "NO - slower at %s" % lost))
    say()
    return lost


def group2(L, a, T, sp):
    rng = np.random.default_rng([22, 4096, 2])                                  # mixed_sizes("block-Jacobi mix", 4096) of tools/potrf_vbatched_bench.py
    small = rng.random(4096) < 0.8
    sizes = np.where(small, rng.integers(1, 17, size=4096), rng.integers(100, 201, size=4096))
    k, batch = 4, len(sizes)
    arr = (C.c_int64 * batch)(*[int(x) for x in sizes])
    plan = C.c_void_p()
    _lib.check(L.cap_vbatch_plan_create(batch, arr, None, None, C.byref(plan)), "cap_vbatch_plan_create")
    launches, rows, total = int(L.cap_vbatch_plan_info(plan, 4)), int(sizes.sum()), int((sizes * sizes).sum())
    g = torch.Generator(device="cuda").manual_seed(5)
    A0 = torch.rand(total, dtype=torch.float64, device="cuda", generator=g) - 0.5
    off = np.concatenate([[0], np.cumsum(sizes * sizes)[:-1]])
    for n in np.unique(sizes):                                                  # n + 1 on every diagonal
        idx = torch.from_numpy(off[sizes == n]).cuda()
        A0[(idx[:, None] + torch.arange(int(n), device="cuda")[None, :] * (int(n) + 1)).reshape(-1)] = float(n + 1)
    A = A0.clone()
    V = (torch.rand(k, rows, dtype=torch.float64, device="cuda") - 0.5) * 0.1
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    groups = []
    for n in np.unique(sizes):
        n, cnt = int(n), int((sizes == n).sum())
        groups.append((n, cnt, factors(cnt, n, n), (torch.rand(cnt, k, n, dtype=torch.float64, device="cuda") - 0.5) * 0.1,
                       torch.zeros(cnt, dtype=torch.int32, device="cuda")))

    def each():
        for n, cnt, Rg, Vg, ig in groups:
            _lib.check(L.cap_dcholupdate_batched(1, 1, n, k, Rg.data_ptr(), n, n * n, Vg.data_ptr(), n, n * k, cnt, ig.data_ptr(), sp))
    tv, tf = [], []
    for rep in range(a.reps + 1):
        A.copy_(A0)
        tv.append(T(lambda: _lib.check(L.cap_dcholupdate_vbatched(plan, 1, 1, k, A.data_ptr(), V.data_ptr(), rows, info.data_ptr(), sp)), a.inner))
        tf.append(T(each, a.inner))
    v, f = stats(tv), stats(tf)
    say("2. block-Jacobi mix, %d blocks (%d rows, %.1f MB of factors, %d distinct sizes), k = %d; per-call times in ms, median [fastest slowest]" % (
        batch, rows, total * 8 / 1e6, len(groups), k))
    say("   plan (%d launches)                  %9.4f [%8.4f %8.4f]" % (launches, v[0], v[1], v[2]))
    say("   one fixed-size call per size (%3d)  %9.4f [%8.4f %8.4f]   fixed / plan %.2f" % (len(groups), f[0], f[1], f[2], f[0] / v[0]))
    say()
    L.cap_vbatch_plan_destroy(plan)


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for name, v in sorted(build.kernel_resources().items()):
        if "chud_" in name and "batched" in name:
            say("  %-74s VGPRs %3s  AGPRs %3s  scratch %s  LDS %6s B  waves/SIMD %s" % (
                name, v.get("VGPRs"), v.get("AGPRs"), v.get("ScratchSize"), v.get("LDS Size"), v.get("Occupancy")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sizes", default="8,16,32,64,96,128,192,256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_cholupdate_batched.txt"))
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT[0] = open(a.out, "w")
    L = _lib.lib()
    T = Timer()
    sp = T.s.cuda_stream
    say("Batched rank-k update of Cholesky factors (cap_dcholupdate_batched / cap_dcholupdate_vbatched, csrc/cholupdate_batched.hip) - round 23")
    say("tools/cholupdate_batched_bench.py on one %s, torch %s, ONE run, %d windows of %d calls after a warm-up round, every window between two "
        "stream events" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.inner))
    say()
    lost = group1(L, a, T, sp)
    group2(L, a, T, sp)
    resources()
    OUT[0].close()
    return 1 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
