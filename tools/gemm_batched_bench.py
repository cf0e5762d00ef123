"""Time the batched general products (cap_dgemm_batched, cap_dgemm_vbatched_inner, cap_dgemm_vbatched_combine, csrc/gemm_batched.hip).

One run, one process; every item is a window between two stream events that holds `inner` back-to-back calls (the per-call time is
window / inner), the items of a row alternating, median of --reps windows after one warm-up round, fastest and slowest beside it.
  1. FIXED SIZE against torch.baddbmm (beta = 0) at the same shapes: squares m = n = k = 8 .. 256 at 1024 blocks and at the large batches
     of the other profiles (65536 for n <= 32, 16384 for 64, 4096 above), and the shapes (p, q, n) = (1, 1, n), (16, 16, n): contractions
     X^T y over n rows - and (n, 16, k = 64): a block times 16 vectors.  No threshold is set; the rows it LOSES are named.
  2. THE BLOCK-JACOBI MIX (80 % n <= 16, 20 % n in 100 .. 200; 4096 blocks) through `inner` (p = q = 16) and `combine` (nrhs = 16, k = 16)
     against one fixed-size call per distinct size on the same data and against torch.bmm on blocks padded to n_max.
  3. with --parent-lib: cap_dsyrk_batched and cap_dsymm_batched of this build and of another build of the library (the parent commit's),
     alternating in this process at 1024 blocks on rows of profiles/r25 and r26 - nothing of theirs was rebuilt; the ratio is reported
     whatever it is.
Writes the table to --out and prints it:

    timeout -k 10 900 python tools/gemm_batched_bench.py [--reps 9] [--out profiles/r28_gemm_batched.txt] [--parent-lib path/to/libcapital_amd.so]
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


def run(items, a, T, inner):
    t = {k: [] for k, _ in items}
    for rep in range(a.reps + 1):
        for k, fn in items:
            t[k].append(T(fn, inner))
    return {k: stats(v) for k, v in t.items()}


def big_batch(n):
    return 65536 if n <= 32 else 16384 if n <= 64 else 4096


def rnd(*shape):
    return torch.randn(*shape, dtype=torch.float64, device="cuda")


def fmt(s):
    return "%9.4f [%8.4f %8.4f]" % s


def group1(L, a, T, sp):
    say("1. fixed size, alpha = 1, beta = 0: C_i (m x n) = A_i^T B_i with A_i k x m and B_i k x n column-major (CAP_TRANS, CAP_NOTRANS) for the "
        "contractions, A_i B_i (CAP_NOTRANS, CAP_NOTRANS) for the squares and the block-times-vectors rows; torch = torch.baddbmm(beta = 0) on the "
        "same memory; per-call times in ms, median [fastest slowest]")
    say("%-16s %4s %4s %4s %6s  %-30s %-30s %9s %8s" % ("shape", "m", "n", "k", "blocks", "cap_dgemm_batched", "torch.baddbmm", "torch/it", "TFLOP/s"))
    losses = []
    rows = []
    for n in a.sizes:
        for batch in (1024, big_batch(n)):
            rows.append(("square", n, n, n, batch, 0))
    for n in a.sizes:
        rows.append(("(1, 1, n)", 1, 1, n, big_batch(n), 1))
        rows.append(("(16, 16, n)", 16, 16, n, big_batch(n), 1))
        rows.append(("(n, 16, k = 64)", n, 16, 64, big_batch(n), 0))
    for what, m, n, k, batch, ta in rows:
        # torch's row-major (batch, r, c) is our column-major c x r with ld = c
        Am = rnd(batch, m, k) if ta else rnd(batch, k, m)          # ta: A_i stored k x m column-major = torch (batch, m, k)
        Bm = rnd(batch, n, k)                                      # B_i k x n column-major = torch (batch, n, k)
        Cm = torch.zeros(batch, n, m, dtype=torch.float64, device="cuda")      # C_i m x n column-major = torch (batch, n, m)
        inner = a.inner if batch * max(m * n, m * k, n * k) < (1 << 26) else 2
        lda = k if ta else m

        def ours():
            _lib.check(L.cap_dgemm_batched(1 if ta else 0, 0, m, n, k, 1.0, Am.data_ptr(), lda, m * k, Bm.data_ptr(), k, n * k, 0.0, Cm.data_ptr(), m,
                                           m * n, batch, sp))
        At = Am.transpose(1, 2) if ta else Am                      # op(A)^T as torch reads it: the row-major C^T = B^T op(A)^T

        def theirs():
            torch.baddbmm(Cm, Bm, At, beta=0.0, alpha=1.0, out=Cm)
        ours()
        ref = Cm.clone()
        theirs()
        err = float((Cm - ref).abs().max() / (ref.abs().max() + 1e-300))
        assert err < 1e-10, (what, m, n, k, err)
        r = run((("it", ours), ("torch", theirs)), a, T, inner)
        tf = 2.0 * m * n * k * batch / (r["it"][0] * 1e-3) / 1e12
        say("%-16s %4d %4d %4d %6d  %s %s %9.2f %8.3f" % (what, m, n, k, batch, fmt(r["it"]), fmt(r["torch"]), r["torch"][0] / r["it"][0], tf))
        spread = max(r["it"][2] - r["it"][1], r["torch"][2] - r["torch"][1])
        if r["it"][0] > r["torch"][0] + spread:
            losses.append((what, m, n, k, batch, round(r["it"][0] / r["torch"][0], 2)))
        del Am, Bm, Cm, ref
        torch.cuda.empty_cache()
    say("rows where cap_dgemm_batched LOSES to torch.baddbmm by more than the row's own spread (shape, m, n, k, blocks, ratio): %s"
        % (losses if losses else "none"))
    say()


def group2(L, a, T, sp):
    rng = np.random.default_rng([22, 4096, 2])                                  # mixed_sizes("block-Jacobi mix", 4096) of tools/potrf_vbatched_bench.py
    small = rng.random(4096) < 0.8
    sizes = np.where(small, rng.integers(1, 17, size=4096), rng.integers(100, 201, size=4096))
    batch, rows, nmax = len(sizes), int(sizes.sum()), int(sizes.max())
    arr = (C.c_int64 * batch)(*[int(x) for x in sizes])
    plan = C.c_void_p()
    _lib.check(L.cap_vbatch_plan_create(batch, arr, None, None, C.byref(plan)), "cap_vbatch_plan_create")
    launches = int(L.cap_vbatch_plan_info(plan, 4))
    p = q = k = 16
    X, Y = rnd(p, rows), rnd(q, rows)                           # stacked: column-major rows x p, ld = rows
    G = torch.zeros(batch, q, p, dtype=torch.float64, device="cuda")            # G_i p x q column-major
    V = rnd(k, rows)
    Z = rnd(batch, q, k)                                        # Z_i k x nrhs column-major
    Cs = torch.zeros(q, rows, dtype=torch.float64, device="cuda")
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    per = {}
    for i, n in enumerate(sizes):
        per.setdefault(int(n), []).append(i)
    # the same data grouped by size for the fixed-size calls, and padded to n_max for torch.bmm
    Xs, Ys, Vs, Zs, Gs, Os = {}, {}, {}, {}, {}, {}
    Xp, Yp = torch.zeros(batch, p, nmax, dtype=torch.float64, device="cuda"), torch.zeros(batch, q, nmax, dtype=torch.float64, device="cuda")
    Vp = torch.zeros(batch, k, nmax, dtype=torch.float64, device="cuda")
    for n, idx in per.items():
        cols = torch.as_tensor(np.concatenate([np.arange(off[i], off[i] + n) for i in idx]), device="cuda")
        Xs[n] = X[:, cols].reshape(p, len(idx), n).permute(1, 0, 2).contiguous()        # (b, p, n): X_i n x p column-major
        Ys[n] = Y[:, cols].reshape(q, len(idx), n).permute(1, 0, 2).contiguous()
        Vs[n] = V[:, cols].reshape(k, len(idx), n).permute(1, 0, 2).contiguous()        # (b, k, n): V_i n x k column-major
        Zs[n] = Z[torch.as_tensor(idx, device="cuda")].contiguous()
        Gs[n] = torch.zeros(len(idx), q, p, dtype=torch.float64, device="cuda")
        Os[n] = torch.zeros(len(idx), q, n, dtype=torch.float64, device="cuda")
        ii = torch.as_tensor(idx, device="cuda")
        Xp[ii, :, :n], Yp[ii, :, :n], Vp[ii, :, :n] = Xs[n], Ys[n], Vs[n]
    Gp = torch.zeros(batch, q, p, dtype=torch.float64, device="cuda")
    Op = torch.zeros(batch, q, nmax, dtype=torch.float64, device="cuda")
    say("2. block-Jacobi mix, %d blocks (%d rows, %d distinct sizes, n_max = %d, %d launches per `combine` call, 1 per `inner` call); p = q = nrhs = k = 16; "
        "per-call times in ms, median [fastest slowest]; per size = one cap_dgemm_batched call per distinct size on the same data, padded = "
        "torch.bmm on blocks padded to n_max" % (batch, rows, len(per), nmax, launches))

    def inner_plan():
        _lib.check(L.cap_dgemm_vbatched_inner(plan, p, q, 1.0, X.data_ptr(), rows, Y.data_ptr(), rows, 0.0, G.data_ptr(), p, p * q, sp))

    def inner_fixed():
        for n in per:
            _lib.check(L.cap_dgemm_batched(1, 0, p, q, n, 1.0, Xs[n].data_ptr(), n, n * p, Ys[n].data_ptr(), n, n * q, 0.0, Gs[n].data_ptr(), p, p * q,
                                           len(per[n]), sp))

    def inner_torch():
        torch.bmm(Yp, Xp.transpose(1, 2), out=Gp)

    def combine_plan():
        _lib.check(L.cap_dgemm_vbatched_combine(plan, q, k, 1.0, V.data_ptr(), rows, Z.data_ptr(), k, k * q, 0.0, Cs.data_ptr(), rows, sp))

    def combine_fixed():
        for n in per:
            _lib.check(L.cap_dgemm_batched(0, 0, n, q, k, 1.0, Vs[n].data_ptr(), n, n * k, Zs[n].data_ptr(), k, k * q, 0.0, Os[n].data_ptr(), n, n * q,
                                           len(per[n]), sp))

    def combine_torch():
        torch.bmm(Z, Vp, out=Op)
    inner_plan(); inner_fixed(); inner_torch(); combine_plan(); combine_fixed(); combine_torch()
    for n, idx in per.items():                                   # the three routes agree
        ii = torch.as_tensor(idx, device="cuda")
        assert torch.equal(G[ii], Gs[n]) and float((Gp[ii] - Gs[n]).abs().max()) < 1e-9
        cols = torch.as_tensor(np.concatenate([np.arange(off[i], off[i] + n) for i in idx]), device="cuda")
        assert torch.equal(Cs[:, cols].reshape(q, len(idx), n).permute(1, 0, 2), Os[n]) and float((Op[ii, :, :n] - Os[n]).abs().max()) < 1e-9
    r = run((("inner", inner_plan), ("inner per size", inner_fixed), ("inner padded", inner_torch), ("combine", combine_plan),
             ("combine per size", combine_fixed), ("combine padded", combine_torch)), a, T, a.inner)
    for key, v in r.items():
        say("   %-18s %s" % (key, fmt(v)))
    say("   inner: per size / plan %.2f, padded torch.bmm / plan %.2f;  combine: per size / plan %.2f, padded torch.bmm / plan %.2f"
        % (r["inner per size"][0] / r["inner"][0], r["inner padded"][0] / r["inner"][0], r["combine per size"][0] / r["combine"][0],
           r["combine padded"][0] / r["combine"][0]))
    say()
    L.cap_vbatch_plan_destroy(plan)


def group3(L, a, T, sp, path):
    P = C.CDLL(path)
    for name in ("cap_dsyrk_batched", "cap_dsymm_batched"):
        sig = _lib.SIGNATURES[name]
        getattr(P, name).restype, getattr(P, name).argtypes = sig[0], sig[1]
    say("3. cap_dsyrk_batched (k = 64, CAP_NOTRANS, beta = 0) and cap_dsymm_batched (nrhs = 16, beta = 0) of this build and of the parent commit's "
        "build, alternating in this process; 1024 blocks, per-call times in ms, median [fastest slowest]")
    say("%-6s %4s  %-30s %-30s %8s %s" % ("entry", "n", "this build", "parent build", "this/par", "within the spread"))
    moved = []
    for n in a.sizes:
        batch, k, nrhs = 1024, 64, 16
        V, Cm = rnd(batch, k, n), torch.zeros(batch, n, n, dtype=torch.float64, device="cuda")
        A, X, Y = rnd(batch, n, n), rnd(batch, nrhs, n), torch.zeros(batch, nrhs, n, dtype=torch.float64, device="cuda")
        calls = {"syrk": lambda lib: _lib.check(lib.cap_dsyrk_batched(1, 0, n, k, 1.0, V.data_ptr(), n, n * k, 0.0, Cm.data_ptr(), n, n * n, None, 0, batch, sp)),
                 "symm": lambda lib: _lib.check(lib.cap_dsymm_batched(1, 0, n, nrhs, 1.0, A.data_ptr(), n, n * n, X.data_ptr(), n, n * nrhs, 0.0, None, n, 0,
                                                                      Y.data_ptr(), n, n * nrhs, batch, sp))}
        for entry, call in calls.items():
            t = {"new": [], "old": []}
            for rep in range(a.reps + 1):
                for key, lib in (("new", L), ("old", P)):
                    t[key].append(T(lambda: call(lib), a.inner))
            x, y = stats(t["new"]), stats(t["old"])
            ok = abs(x[0] - y[0]) <= max(x[2] - x[1], y[2] - y[1])
            if not ok:
                moved.append((entry, n, round(x[0] / y[0], 3)))
            say("%-6s %4d  %s %s %8.3f %s" % (entry, n, fmt(x), fmt(y), x[0] / y[0], "yes" if ok else "NO"))
    say("syrk and symm within the run's own spread of the parent's time at every row: %s" % ("yes" if not moved else "NO - %s" % moved))
    say()


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for name, v in sorted(build.kernel_resources().items()):
        if "gemm_batched_kernel" in name or "gemm_batched_blocked_kernel" in name:
            say("  %-70s VGPRs %3s  AGPRs %3s  scratch %s  waves/SIMD %s" % (name, v.get("VGPRs"), v.get("AGPRs"), v.get("ScratchSize"), v.get("Occupancy")))
    say("device text md5 (unchanged by this round: neither file was edited, no header of theirs changed): syrk_batched.hip %s  symm_batched.hip %s"
        % (build.device_text_md5("syrk_batched.hip"), build.device_text_md5("symm_batched.hip")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sizes", default="8,16,32,64,96,128,192,256")
    ap.add_argument("--groups", default="1,2,3")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_gemm_batched.txt"))
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    groups = a.groups.split(",")
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT[0] = open(a.out, "w")
    L = _lib.lib()
    T = Timer()
    sp = T.s.cuda_stream
    say("Batched general products on the block layouts (csrc/gemm_batched.hip) - round 28")
    say("tools/gemm_batched_bench.py on one %s, torch %s, ONE run, %d windows of %d calls (2 for the heaviest rows) after a warm-up round, every window "
        "between two stream events" % (torch.cuda.get_device_name(0), torch.__version__, a.reps, a.inner))
    say()
    if "1" in groups:
        group1(L, a, T, sp)
    if "2" in groups:
        group2(L, a, T, sp)
    if "3" in groups and a.parent_lib:
        group3(L, a, T, sp, a.parent_lib)
    elif "3" in groups:
        say("3. cap_dsyrk_batched / cap_dsymm_batched against the parent commit's build: not measured (no --parent-lib given)")
        say()
    resources()
    OUT[0].close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
