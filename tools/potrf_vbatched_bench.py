"""Time the variable-size batched Cholesky (cap_dpotrf_vbatched / cap_dpotrs_vbatched / cap_dpotri_vbatched, csrc/potrf_vbatched.hip).

One run, every item between two stream events, the items of a row alternating in one process, median of --reps after one warm-up round (with
the fastest and slowest repetition of the fixed-size entry beside it: its run-to-run spread); the inputs are restored outside the timed
window.  Three groups, for factor, solve (--nrhs right-hand sides) and inverse (fill = 0) each:

  1. ALL SIZES EQUAL: 4096 blocks of n = 8, 32, 64, 128, 256 through a plan against the fixed-size entry on the same data.
  2. MIXED BATCHES: n uniform in 1..64, uniform in 1..256, and a block-Jacobi-like mix (80 % n <= 16, 20 % n in 100..200), 4096 and 65536
     blocks (a row that does not fit the memory is reported as such), against
       (a) the route the plan replaces: one fixed-size call per distinct size on sub-batches gathered beforehand - the time of the gather
           and of the scatter back is reported separately, it is not part of (a);
       (b) padding every block to n_max with an identity (one fixed-size call at n_max).
  3. THE FIXED-SIZE ENTRIES against another build of the library (--parent-lib: the parent commit's libcapital_amd.so), the same data,
     alternating - their kernels are built from the bodies that moved into csrc/batched_*.h.

Blocks are diagonally dominant (uniform off-diagonal entries, n + 1 on the diagonal): the time of these kernels does not depend on the data.
Writes the table to --out (default profiles/r22_potrf_vbatched.txt) and prints it:

    timeout -k 10 1100 python tools/potrf_vbatched_bench.py [--reps 9] [--groups 1,2,3] [--parent-lib PATH]
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

OUT = [None]                                # the open --out file: every line goes there as it is printed


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

    def __call__(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.s)
        fn()
        e1.record(self.s)
        e1.synchronize()
        return e0.elapsed_time(e1)


def make_plan(L, sizes):
    arr = (C.c_int64 * max(len(sizes), 1))(*[int(x) for x in sizes])
    p = C.c_void_p()
    _lib.check(L.cap_vbatch_plan_create(len(sizes), arr, None, None, C.byref(p)), "cap_vbatch_plan_create")
    return p


def flat_spd(sizes, seed):
    """the packed flat buffer of diagonally dominant blocks, its offsets (NumPy) and the indices of the diagonals"""
    n = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(n * n)[:-1]])
    total = int((n * n).sum())
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.rand(total, dtype=torch.float64, device="cuda", generator=g) - 0.5
    nd, offd = torch.from_numpy(n).cuda(), torch.from_numpy(off).cuda()
    j = torch.arange(int(n.sum()), device="cuda") - torch.repeat_interleave(torch.cumsum(nd, 0) - nd, nd)
    diag = torch.repeat_interleave(offd, nd) + j * (torch.repeat_interleave(nd, nd) + 1)
    A[diag] = (torch.repeat_interleave(nd, nd) + 1).to(torch.float64)
    return A, off


def fixed_fns(L, n):
    return ((L.cap_dpotrf_batched if n <= 64 else L.cap_dpotrf_batched_blocked), (L.cap_dpotrs_batched if n <= 64 else L.cap_dpotrs_batched_blocked),
            L.cap_dpotri_batched)


def row(name, cols):
    say("%-34s " % name + " ".join(cols))


def fmt(t):
    return "%9.4f [%8.4f %8.4f]" % t


def group1(L, a, T, sp):
    say("1. all sizes equal, 4096 blocks: the plan against the fixed-size entry on the same data; median [fastest slowest] in ms")
    say("%-34s %-28s %-28s %s" % ("", "fixed-size entry", "plan", "plan / fixed (medians)"))
    batch = 4096
    for n in (8, 32, 64, 128, 256):
        A0, _ = flat_spd([n] * batch, n)
        plan = make_plan(L, [n] * batch)
        fac, sol, inv = fixed_fns(L, n)
        A, B0 = torch.empty_like(A0), torch.randn(a.nrhs, n * batch, dtype=torch.float64, device="cuda")
        B, info = torch.empty_like(B0), torch.zeros(batch, dtype=torch.int32, device="cuda")
        Bf0 = B0.reshape(a.nrhs, batch, n).transpose(0, 1).contiguous()      # the fixed-size layout: block i's n x nrhs right-hand sides together
        Bf = torch.empty_like(Bf0)
        t = {k: [] for k in ("ff", "fv", "sf", "sv", "if", "iv")}
        for rep in range(a.reps + 1):
            A.copy_(A0)
            t["ff"].append(T(lambda: _lib.check(fac(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))))
            R = A.clone()
            A.copy_(A0)
            t["fv"].append(T(lambda: _lib.check(L.cap_dpotrf_vbatched(plan, 1, A.data_ptr(), info.data_ptr(), None, sp))))
            assert torch.equal(A.view(torch.int64), R.view(torch.int64)), "factor bits differ"
            Bf.copy_(Bf0); B.copy_(B0)
            t["sf"].append(T(lambda: _lib.check(sol(1, n, a.nrhs, R.data_ptr(), n, n * n, Bf.data_ptr(), n, n * a.nrhs, batch, info.data_ptr(), sp))))
            t["sv"].append(T(lambda: _lib.check(L.cap_dpotrs_vbatched(plan, 1, a.nrhs, R.data_ptr(), B.data_ptr(), n * batch, info.data_ptr(), sp))))
            assert torch.equal(B.reshape(a.nrhs, batch, n).transpose(0, 1).contiguous().view(torch.int64), Bf.view(torch.int64)), "solve bits differ"
            A.copy_(R)
            t["if"].append(T(lambda: _lib.check(inv(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), 0, sp))))
            X = A.clone()
            A.copy_(R)
            t["iv"].append(T(lambda: _lib.check(L.cap_dpotri_vbatched(plan, 1, A.data_ptr(), info.data_ptr(), 0, sp))))
            assert torch.equal(A.view(torch.int64), X.view(torch.int64)), "inverse bits differ"
        for op, kf, kv in (("factor", "ff", "fv"), ("solve nrhs %d" % a.nrhs, "sf", "sv"), ("inverse", "if", "iv")):
            f, v = stats(t[kf]), stats(t[kv])
            row("n %3d  %s" % (n, op), [fmt(f), fmt(v), "%8.3f" % (v[0] / f[0])])
        L.cap_vbatch_plan_destroy(plan)
        del A0, A, B0, B, Bf0, Bf
    say()


MIXES = ("uniform 1..64", "uniform 1..256", "block-Jacobi mix")


def mixed_sizes(kind, batch):
    rng = np.random.default_rng([22, batch, MIXES.index(kind)])
    if kind == "uniform 1..64":
        return rng.integers(1, 65, size=batch)
    if kind == "uniform 1..256":
        return rng.integers(1, 257, size=batch)
    small = rng.random(batch) < 0.8
    return np.where(small, rng.integers(1, 17, size=batch), rng.integers(100, 201, size=batch))


def group2(L, a, T, sp):
    say("2. mixed batches: the plan against (a) one fixed-size call per distinct size on gathered sub-batches and (b) padding to n_max; ms")
    say("%-34s %9s %9s %9s %9s %9s %9s   %s" % ("", "plan", "(a)", "gather", "(b)", "(a)/plan", "(b)/plan", "launches plan / (a)"))
    for kind in MIXES:
        for batch in (4096, 65536):
            try:
                mixed_row(L, a, T, sp, kind, batch)
            except torch.cuda.OutOfMemoryError:
                say("%-34s does not fit the device memory" % ("%s, %d blocks" % (kind, batch)))
            torch.cuda.empty_cache()
    say()


def mixed_row(L, a, T, sp, kind, batch):
    sizes = mixed_sizes(kind, batch)
    nmax = int(sizes.max())
    A0, off = flat_spd(sizes, batch)
    plan = make_plan(L, sizes)
    launches = int(L.cap_vbatch_plan_info(plan, 4))
    rows = int(sizes.sum())
    row_off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    A = torch.empty_like(A0)
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    B0 = torch.randn(a.nrhs, rows, dtype=torch.float64, device="cuda")
    B = torch.empty_like(B0)
    # (a): per distinct size the block indices; the gather makes (count, n, n) sub-batches, the scatter puts them back
    groups = [(int(n), torch.from_numpy(np.nonzero(sizes == n)[0]).cuda()) for n in np.unique(sizes)]
    offd, rowd = torch.from_numpy(off).cuda(), torch.from_numpy(row_off).cuda()

    def gather(src):
        return [src[(offd[idx][:, None] + torch.arange(n * n, device="cuda")[None, :])] for n, idx in groups]

    def scatter(dst, subs):
        for (n, idx), sub in zip(groups, subs):
            dst[(offd[idx][:, None] + torch.arange(n * n, device="cuda")[None, :])] = sub

    def gather_b(src):
        return [src[:, (rowd[idx][:, None] + torch.arange(n, device="cuda")[None, :])].permute(1, 0, 2).contiguous() for n, idx in groups]

    infos = [torch.zeros(len(idx), dtype=torch.int32, device="cuda") for _, idx in groups]

    def each(which, subs, bsubs=None):
        for k, ((n, idx), sub) in enumerate(zip(groups, subs)):
            fac, sol, inv = fixed_fns(L, n)
            cnt = len(idx)
            if which == 0:
                _lib.check(fac(1, n, sub.data_ptr(), n, n * n, cnt, infos[k].data_ptr(), None, sp))
            elif which == 1:
                _lib.check(sol(1, n, a.nrhs, sub.data_ptr(), n, n * n, bsubs[k].data_ptr(), n, n * a.nrhs, cnt, infos[k].data_ptr(), sp))
            else:
                _lib.check(inv(1, n, sub.data_ptr(), n, n * n, cnt, infos[k].data_ptr(), 0, sp))

    # (b): (batch, nmax, nmax) with the block in the leading corner and ones on the rest of the diagonal
    def padded(subs):
        P = torch.zeros(batch, nmax, nmax, dtype=torch.float64, device="cuda")
        P.diagonal(dim1=1, dim2=2).fill_(1.0)
        for (n, idx), sub in zip(groups, subs):
            P[idx, :n, :n] = sub.reshape(len(idx), n, n)
        return P

    facm, solm, invm = fixed_fns(L, nmax)
    infop = torch.zeros(batch, dtype=torch.int32, device="cuda")
    t = {k: [] for k in ("fv", "fa", "fg", "fb", "sv", "sa", "sg", "sb", "iv", "ia", "ig", "ib")}
    do_b = True
    for rep in range(a.reps + 1):
        A.copy_(A0)
        t["fv"].append(T(lambda: _lib.check(L.cap_dpotrf_vbatched(plan, 1, A.data_ptr(), info.data_ptr(), None, sp))))
        box = {}
        g1 = T(lambda: box.__setitem__("s", gather(A0)))
        subs = box.pop("s")
        t["fa"].append(T(lambda: each(0, subs)))
        A.copy_(A0)
        t["fg"].append(g1 + T(lambda: scatter(A, subs)))
        R = A                                       # the factors, scattered back: the plan's input for the solve and the inverse
        if rep == 0:
            chk = A0.clone()
            _lib.check(L.cap_dpotrf_vbatched(plan, 1, chk.data_ptr(), info.data_ptr(), None, sp))
            assert torch.equal(torch.nan_to_num(chk).view(torch.int64), torch.nan_to_num(R).view(torch.int64)), "the two routes factor differently"
            del chk
        B.copy_(B0)
        t["sv"].append(T(lambda: _lib.check(L.cap_dpotrs_vbatched(plan, 1, a.nrhs, R.data_ptr(), B.data_ptr(), rows, info.data_ptr(), sp))))
        g1 = T(lambda: box.__setitem__("b", gather_b(B0)))
        bsubs = box.pop("b")
        t["sa"].append(T(lambda: each(1, subs, bsubs)))
        t["sg"].append(g1)
        if do_b:
            try:
                P = padded(subs)
                Bp = torch.zeros(batch, a.nrhs, nmax, dtype=torch.float64, device="cuda")
                t["sb"].append(T(lambda: _lib.check(solm(1, nmax, a.nrhs, P.data_ptr(), nmax, nmax * nmax, Bp.data_ptr(), nmax, nmax * a.nrhs, batch,
                                                         infop.data_ptr(), sp))))
                t["ib"].append(T(lambda: _lib.check(invm(1, nmax, P.data_ptr(), nmax, nmax * nmax, batch, infop.data_ptr(), 0, sp))))
                del P, Bp
                P = padded(gather(A0))
                t["fb"].append(T(lambda: _lib.check(facm(1, nmax, P.data_ptr(), nmax, nmax * nmax, batch, infop.data_ptr(), None, sp))))
                del P
            except torch.cuda.OutOfMemoryError:
                do_b = False
                torch.cuda.empty_cache()
        X = R.clone()
        t["iv"].append(T(lambda: _lib.check(L.cap_dpotri_vbatched(plan, 1, X.data_ptr(), info.data_ptr(), 0, sp))))
        t["ia"].append(T(lambda: each(2, subs)))
        t["ig"].append(t["fg"][-1])
        del subs, bsubs, X
    name = "%s, %d blocks" % (kind, batch)
    for op, k in (("factor", "f"), ("solve nrhs %d" % a.nrhs, "s"), ("inverse", "i")):
        v, ra, g = stats(t[k + "v"])[0], stats(t[k + "a"])[0], stats(t[k + "g"])[0]
        rb = stats(t[k + "b"])[0] if do_b and len(t[k + "b"]) > 1 else float("nan")
        row("%s" % name if op == "factor" else "", ["%-14s" % op, "%9.4f %9.4f %9.4f %9.4f %9.2f %9.2f   %d / %d" % (v, ra, g, rb, ra / v, rb / v, launches, len(groups))])
    say("%-34s   (%d rows, n_max %d, %.1f MB of blocks, %d distinct sizes%s)" % ("", rows, nmax, A0.numel() * 8 / 1e6, len(groups),
                                                                            "" if do_b else "; (b) does not fit the device memory"))
    L.cap_vbatch_plan_destroy(plan)


def group3(L, a, T, sp):
    if not a.parent_lib:
        say("3. the fixed-size entries against the parent commit: not run (no --parent-lib)")
        say()
        return
    old = C.CDLL(a.parent_lib, mode=C.RTLD_LOCAL)
    for name in ("cap_dpotrf_batched", "cap_dpotrs_batched", "cap_dpotrf_batched_blocked", "cap_dpotrs_batched_blocked", "cap_dpotri_batched"):
        f = getattr(old, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    say("3. the fixed-size entries, 4096 blocks: this build against the parent commit's library, the same data, alternating; median [fastest slowest] in ms")
    say("%-34s %-28s %-28s %s" % ("", "parent commit", "this build", "this / parent (medians)"))
    batch = 4096
    for n in (8, 32, 64, 128, 192, 256):
        A0, _ = flat_spd([n] * batch, n)
        A, info = torch.empty_like(A0), torch.zeros(batch, dtype=torch.int32, device="cuda")
        B0 = torch.randn(batch, a.nrhs, n, dtype=torch.float64, device="cuda")
        B = torch.empty_like(B0)
        t = {k: [] for k in ("fo", "fn", "so", "sn", "io", "in")}
        for rep in range(a.reps + 1):
            outs = []
            for tag, lib in (("o", old), ("n", L)):
                fac, sol, inv = fixed_fns(lib, n)
                A.copy_(A0)
                t["f" + tag].append(T(lambda: _lib.check(fac(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp))))
                R = A.clone()
                B.copy_(B0)
                t["s" + tag].append(T(lambda: _lib.check(sol(1, n, a.nrhs, R.data_ptr(), n, n * n, B.data_ptr(), n, n * a.nrhs, batch, info.data_ptr(), sp))))
                t["i" + tag].append(T(lambda: _lib.check(inv(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), 0, sp))))
                outs.append((R, B.clone(), A.clone()))
            assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(*outs)), "the two builds differ in bits"
        for op, k in (("factor", "f"), ("solve nrhs %d" % a.nrhs, "s"), ("inverse", "i")):
            o, nw = stats(t[k + "o"]), stats(t[k + "n"])
            row("n %3d  %s" % (n, op), [fmt(o), fmt(nw), "%8.3f" % (nw[0] / o[0])])
    say()


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for k, v in sorted(build.kernel_resources().items()):
        if "vbatched" in k:
            say("  %-72s VGPRs %3s  AGPRs %3s  scratch %s  LDS %6s B  waves/SIMD %s" % (
                k, v.get("VGPRs"), v.get("AGPRs"), v.get("ScratchSize"), v.get("LDS Size"), v.get("Occupancy")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nrhs", type=int, default=4)
    ap.add_argument("--groups", default="1,2,3")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_potrf_vbatched.txt"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT[0] = open(a.out, "w")
    L = _lib.lib()
    T = Timer()
    sp = T.s.cuda_stream
    say("Variable-size batched Cholesky (cap_dpotrf_vbatched / cap_dpotrs_vbatched / cap_dpotri_vbatched, csrc/potrf_vbatched.hip) - round 22")
    say("tools/potrf_vbatched_bench.py on one %s, torch %s, ONE run, %d repetitions after a warm-up round, every item between two stream events"
        % (torch.cuda.get_device_name(0), torch.__version__, a.reps))
    say()
    todo = a.groups.split(",")
    for g in todo:                          # in the order given
        {"1": group1, "2": group2, "3": group3}[g](L, a, T, sp)
    resources()
    OUT[0].close()


if __name__ == "__main__":
    main()
