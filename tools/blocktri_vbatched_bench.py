"""Time the ragged block-tridiagonal entries (batched.VarChains: cap_dpotrf_blocktri_vbatched, cap_dpotrs_blocktri_vbatched,
cap_dpotri_blocktri_vbatched, csrc/blocktri_vbatched.hip) against the routes a caller had before them, in the same run.

One run, one process; every item is a window between two stream events, the items of a row alternating, median of --reps windows after
one warm-up round, fastest and slowest beside it.  Per shape (n, T_max, chains) and length distribution - uniform on [T_max / 2, T_max],
log-uniform on [1, T_max], "mostly short" (95 % at T_max / 16, the rest at T_max) -
  * the plan: one launch on the ragged storage;
  * PADDING every chain to T_max with identity diagonal blocks and zero couplings through the fixed-size entries (exact; it costs
    T_max / mean(T) times the memory, traffic and sequential positions - the figure printed beside the ratio is what a perfect ragged
    implementation could gain);
  * ONE FIXED-SIZE CALL PER DISTINCT LENGTH on gathered copies (the gather is not counted).
Then all lengths equal (the plan against the fixed-size entry on the same data: what the record lookup and the activity predicates cost,
per NP) and the few-long-chains corner (64 chains around 10000 positions, n = 8: microseconds per position).
The calls work in place, so every window of the factor and the inverse starts with a restoring copy; its own time is reported (the
floor) and is part of every figure of that row, ours and the other routes' alike.
With --parent-lib: the six entries (factor, solve, inverse; fixed size and on a plan) of this build and of another build of the library
(the parent commit's) through the C ABI, alternating in this process on the "all lengths equal" shapes; per row the ratio this / parent
without the restoring copy, held against 1 + max(0.02, the parent's own spread (slowest - fastest) / median in this run).
--sections picks what is run.  Writes the table to --out and prints it:

    timeout -k 10 900 python tools/blocktri_vbatched_bench.py [--reps 9] [--out profiles/r31_blocktri_vbatched.txt]
                                                              [--sections ragged,equal,long,parent] [--parent-lib path/to/libcapital_amd.so]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from capital_amd import _lib, batched, build  # noqa: E402
from tools.blocktri_bench import fmt, run  # noqa: E402

SHAPES = ((8, 256, 4096), (16, 128, 4096), (32, 64, 2048), (64, 32, 1024))
EQUAL = ((8, 256, 1024), (16, 128, 1024), (32, 64, 1024), (64, 32, 1024))
NRHS = 8
OUT = [None]


def say(line=""):
    print(line, flush=True)
    if OUT[0]:
        OUT[0].write(line + "\n")
        OUT[0].flush()


def lengths_of(kind, tmax, batch, rng):
    if kind == "uniform":
        return rng.integers(tmax // 2, tmax + 1, size=batch)
    if kind == "log-uniform":
        return np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(tmax + 1), size=batch))).astype(np.int64), 1, tmax)
    t = np.full(batch, max(tmax // 16, 1), dtype=np.int64)
    t[rng.random(batch) >= 0.95] = tmax
    return t


def slots_of(n, slots, seed):
    """diagonally dominant blocks in every slot: D (slots, n, n) symmetric, E (slots, n, n)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    E = torch.rand(slots, n, n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    S = torch.rand(slots, n, n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    D = 0.5 * (S + S.transpose(-1, -2)) + (3.0 * n + 1.5) * torch.eye(n, dtype=torch.float64, device="cuda")
    return D, E


def three(tag, factor, solve, inverse, restore, restore_b, reps):
    """(factor + copy, solve, inverse + copy) medians of one route; the factor is left in place for the solve and the inverse"""
    r = run([(tag + " factor + copy", lambda: (restore(), factor()))], reps)
    restore(); factor(); keep = restore.snapshot()
    r.update(run([(tag + " solve (%d right-hand sides) + copy" % NRHS, lambda: (restore_b(), solve()))], reps))
    r.update(run([(tag + " inverse + copy", lambda: (keep(), inverse()))], reps))
    return r


class Store:
    """tensors that are restored from their originals in front of a window"""

    def __init__(self, *tensors):
        self.live = tensors
        self.orig = [t.clone() for t in tensors]

    def __call__(self):
        for t, o in zip(self.live, self.orig):
            t.copy_(o)

    def snapshot(self):
        return Store(*self.live)


def ragged_section(n, tmax, batch, kind, reps, rng):
    T = lengths_of(kind, tmax, batch, rng)
    rows = int(T.sum())
    vc = batched.VarChains([int(t) for t in T])
    D, E = slots_of(n, vc.slots, n * 1000 + tmax)
    B = torch.rand(NRHS, rows * n, dtype=torch.float64, device="cuda")
    say("n = %d, T_max = %d, %d chains, %s: mean T = %.1f, T_max / mean(T) = %.2f, %d distinct lengths; ragged D and E hold %.3f GB, padded %.3f GB"
        % (n, tmax, batch, kind, T.mean(), tmax / T.mean(), len(set(T.tolist())), 2 * D.numel() * 8 / 1e9, 2 * batch * tmax * n * n * 8 / 1e9))
    res = {}
    sd, sb = Store(D, E), Store(B)
    res.update(run([("copy of the ragged D and E (floor)", sd)], reps))
    res.update(three("plan:", lambda: vc.potrf(D, E), lambda: vc.potrs(D, E, B), lambda: vc.potri(D, E), sd, sb, reps))
    # padding to T_max: identity diagonal blocks, zero couplings
    first = torch.tensor(vc.first, device="cuda")
    Tt = torch.from_numpy(T).cuda()
    pos = torch.arange(tmax, device="cuda")
    on = pos[None, :] < Tt[:, None]
    src = (first[:, None] + pos[None, :]).clamp_(max=vc.slots - 1)
    Dp = torch.where(on[:, :, None, None], D[src], torch.eye(n, dtype=torch.float64, device="cuda"))
    Ep = torch.where((pos[None, :] + 1 < Tt[:, None])[:, :, None, None], E[src], torch.zeros((), dtype=torch.float64, device="cuda"))[:, :tmax - 1].contiguous()
    Bp = torch.rand(batch, NRHS, tmax * n, dtype=torch.float64, device="cuda")
    sp, sbp = Store(Dp, Ep), Store(Bp)
    res.update(run([("copy of the padded D and E", sp)], reps))
    res.update(three("padded:", lambda: batched.blocktri_potrf(Dp, Ep), lambda: batched.blocktri_potrs(Dp, Ep, Bp), lambda: batched.blocktri_potri(Dp, Ep),
                     sp, sbp, reps))
    del Dp, Ep, Bp, sp, sbp
    # one fixed-size call per distinct length, on gathered copies
    groups = []
    for t in sorted(set(T.tolist())):
        idx = torch.from_numpy(np.nonzero(T == t)[0]).cuda()
        s = first[idx][:, None] + torch.arange(t, device="cuda")[None, :]
        groups.append((D[s].contiguous(), E[s][:, :t - 1].contiguous() if t > 1 else None, torch.rand(len(idx), NRHS, t * n, dtype=torch.float64, device="cuda")))
    sg = Store(*[x for g in groups for x in g[:2] if x is not None])
    sbg = Store(*[g[2] for g in groups])
    res.update(run([("copy of the gathered D and E", sg)], reps))
    res.update(three("per length (%d calls):" % len(groups), lambda: [batched.blocktri_potrf(d, e) for d, e, _ in groups],
                     lambda: [batched.blocktri_potrs(d, e, b) for d, e, b in groups], lambda: [batched.blocktri_potri(d, e) for d, e, _ in groups], sg, sbg, reps))
    for k, v in res.items():
        say("  %-58s %s" % (k, fmt(v)))
    fl = {"plan:": res["copy of the ragged D and E (floor)"][0], "padded:": res["copy of the padded D and E"][0],
          "per length": res["copy of the gathered D and E"][0]}
    for op in ("factor", "inverse"):
        t = {tag: [v[0] for k, v in res.items() if k.startswith(tag) and " %s " % op in k][0] - f for tag, f in fl.items()}
        say("  %s without its copy: plan %.3f ms, padded %.3f ms (padded / plan = %.2f of a possible %.2f), per length %.3f ms (per length / plan = %.2f)"
            % (op, t["plan:"], t["padded:"], t["padded:"] / t["plan:"], tmax / T.mean(), t["per length"], t["per length"] / t["plan:"]))
    say()
    del groups, sg, sbg, D, E, B, sd, sb
    torch.cuda.empty_cache()


def equal_section(n, T, batch, reps):
    vc = batched.VarChains([T] * batch)
    D, E = slots_of(n, vc.slots, n * 1000 + T)
    B = torch.rand(NRHS, batch * T * n, dtype=torch.float64, device="cuda")
    D4, E4 = D.unflatten(0, (batch, T)), E.unflatten(0, (batch, T))[:, :T - 1]
    B3 = torch.rand(batch, NRHS, T * n, dtype=torch.float64, device="cuda")
    sd, sb = Store(D, E), Store(B, B3)
    r = run([("copy (floor)", sd)], reps)
    r.update(run([("plan: factor + copy", lambda: (sd(), vc.potrf(D, E))), ("fixed: factor + copy", lambda: (sd(), batched.blocktri_potrf(D4, E4)))], reps))
    sd(); vc.potrf(D, E); keep = sd.snapshot()
    r.update(run([("plan: solve + copy", lambda: (sb(), vc.potrs(D, E, B))), ("fixed: solve + copy", lambda: (sb(), batched.blocktri_potrs(D4, E4, B3)))], reps))
    r.update(run([("plan: inverse + copy", lambda: (keep(), vc.potri(D, E))), ("fixed: inverse + copy", lambda: (keep(), batched.blocktri_potri(D4, E4)))], reps))
    say("n = %d (NP = %d), T = %d, %d chains, all lengths equal" % (n, 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64, T, batch))
    for k, v in r.items():
        say("  %-58s %s" % (k, fmt(v)))
    fl = r["copy (floor)"][0]
    say("  plan / fixed without the copy: factor %.3f, inverse %.3f; with its copy of B: solve %.3f"
        % ((r["plan: factor + copy"][0] - fl) / (r["fixed: factor + copy"][0] - fl), (r["plan: inverse + copy"][0] - fl) / (r["fixed: inverse + copy"][0] - fl),
           r["plan: solve + copy"][0] / r["fixed: solve + copy"][0]))
    say()
    del D, E, B, B3, sd, sb, keep
    torch.cuda.empty_cache()


def long_section(reps, rng):
    n, batch = 8, 64
    T = rng.integers(9000, 11001, size=batch)
    vc = batched.VarChains([int(t) for t in T])
    D, E = slots_of(n, vc.slots, 4242)
    B = torch.rand(NRHS, vc.rows * n, dtype=torch.float64, device="cuda")
    sd, sb = Store(D, E), Store(B)
    r = run([("copy (floor)", sd), ("plan: factor + copy", lambda: (sd(), vc.potrf(D, E)))], reps)
    sd(); vc.potrf(D, E); keep = sd.snapshot()
    r.update(run([("plan: solve + copy", lambda: (sb(), vc.potrs(D, E, B))), ("plan: inverse + copy", lambda: (keep(), vc.potri(D, E)))], reps))
    say("n = 8, 64 chains of 9000 .. 11000 positions (T_max = %d, mean %.0f): eight wavefronts on the whole chip" % (T.max(), T.mean()))
    for k, v in r.items():
        say("  %-58s %s" % (k, fmt(v)))
    fl = r["copy (floor)"][0]
    say("  microseconds per position of the longest chain: factor %.3f, solve (both sweeps, %d right-hand sides) %.3f, inverse %.3f"
        % (1e3 * (r["plan: factor + copy"][0] - fl) / T.max(), NRHS, 1e3 * r["plan: solve + copy"][0] / T.max(), 1e3 * (r["plan: inverse + copy"][0] - fl) / T.max()))
    say()


ENTRIES = ("cap_dpotrf_blocktri_batched", "cap_dpotrs_blocktri_batched", "cap_dpotri_blocktri_batched", "cap_blocktri_plan_create",
           "cap_blocktri_plan_destroy", "cap_dpotrf_blocktri_vbatched", "cap_dpotrs_blocktri_vbatched", "cap_dpotri_blocktri_vbatched")


def parent_section(n, T, batch, reps, libs):
    """the six entries of both libraries on one set of buffers (a plan of each library's own); False when a row does not hold"""
    D, E = slots_of(n, batch * T, n * 1000 + T)                # slot c T + i: block i of chain c; the last E slot of a chain is not addressed
    B = torch.rand(NRHS, batch * T * n, dtype=torch.float64, device="cuda")
    B3 = torch.rand(batch, NRHS, T * n, dtype=torch.float64, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    d, e, b, b3, ip, nn, chain = D.data_ptr(), E.data_ptr(), B.data_ptr(), B3.data_ptr(), info.data_ptr(), n * n, T * n * n
    plans = {}
    for tag, lib in libs.items():
        plans[tag] = C.c_void_p()
        _lib.check(lib.cap_blocktri_plan_create(batch, (C.c_int64 * batch)(*([T] * batch)), None, C.byref(plans[tag])), "cap_blocktri_plan_create")
    calls = {
        "fixed factor": lambda lib, p: lib.cap_dpotrf_blocktri_batched(1, n, T, d, n, nn, chain, e, n, nn, chain, ip, None, batch, sp),
        "plan  factor": lambda lib, p: lib.cap_dpotrf_blocktri_vbatched(p, 1, n, d, n, nn, e, n, nn, ip, None, sp),
        "fixed solve": lambda lib, p: lib.cap_dpotrs_blocktri_batched(1, 0, n, T, NRHS, d, n, nn, chain, e, n, nn, chain, b3, T * n, NRHS * T * n, None, batch, sp),
        "plan  solve": lambda lib, p: lib.cap_dpotrs_blocktri_vbatched(p, 1, 0, n, NRHS, d, n, nn, e, n, nn, b, batch * T * n, None, sp),
        "fixed inverse": lambda lib, p: lib.cap_dpotri_blocktri_batched(1, 0, n, T, d, n, nn, chain, e, n, nn, chain, None, batch, sp),
        "plan  inverse": lambda lib, p: lib.cap_dpotri_blocktri_vbatched(p, 1, 0, n, d, n, nn, e, n, nn, None, sp),
    }
    sd, sb = Store(D, E), Store(B, B3)
    sd(); _lib.check(calls["fixed factor"](libs["this"], None)); keep = sd.snapshot()      # the factor, for the solve and the inverse
    say("n = %d (NP = %d), T = %d, %d chains: this build and the parent's, alternating" % (n, 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64, T, batch))
    say("  %-14s %-32s %-32s %-32s %8s %8s %s" % ("entry", "this + copy", "parent + copy", "copy (floor)", "this/par", "1 + s", "holds"))
    good = True
    for name, call in calls.items():
        restore = sb if "solve" in name else sd if "factor" in name else keep
        r = run([("floor", restore)] + [(tag, lambda lib=lib, tag=tag: (restore(), _lib.check(call(lib, plans[tag])))) for tag, lib in libs.items()], reps)
        x, y, fl = r["this"], r["parent"], r["floor"]
        ratio, bound = (x[0] - fl[0]) / (y[0] - fl[0]), 1.0 + max(0.02, (y[2] - y[1]) / y[0])
        good = good and ratio <= bound
        say("  %-14s %s %s %s %8.3f %8.3f %s" % (name, fmt(x), fmt(y), fmt(fl), ratio, bound, "yes" if ratio <= bound else "NO"))
    say()
    for tag, lib in libs.items():
        lib.cap_blocktri_plan_destroy(plans[tag])
    del D, E, B, B3, sd, sb, keep
    torch.cuda.empty_cache()
    return good


def resources():
    say("kernel resources (the compiler's remarks of this build):")
    for name, v in sorted(build.kernel_resources().items()):
        if "blocktri_" in name:
            say("  %-84s VGPRs %3s  AGPRs %3s  LDS %6s  scratch %s  spilled %s  waves/SIMD %s"
                % (name, v.get("VGPRs"), v.get("AGPRs"), v.get("LDS Size"), v.get("ScratchSize"), v.get("VGPRs Spill"), v.get("Occupancy")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sections", default="ragged,equal,long,parent")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--title", default="Ragged block-tridiagonal chains on a plan (csrc/blocktri_vbatched.hip) - round 31")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_blocktri_vbatched.txt"))
    a = ap.parse_args()
    build.build(verbose=False)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    OUT[0] = open(a.out, "w")
    sections = a.sections.split(",")
    say(a.title)
    say("tools/blocktri_vbatched_bench.py on one %s, torch %s, ONE run, median [fastest slowest] of %d windows after a warm-up round, times in ms per call"
        % (torch.cuda.get_device_name(0), torch.__version__, a.reps))
    say("device text (md5 of the gfx950 .text of the last build): " + ", ".join("%s %s" % (s, build.device_text_md5(s)) for s in (
        "blocktri_batched.hip", "blocktri_potri_batched.hip", "blocktri_vbatched.hip")))
    say()
    rng = np.random.default_rng(31)
    for (n, tmax, batch) in SHAPES if "ragged" in sections else ():
        for kind in ("uniform", "log-uniform", "mostly short"):
            ragged_section(n, tmax, batch, kind, a.reps, rng)
    for (n, T, batch) in EQUAL if "equal" in sections else ():
        equal_section(n, T, batch, a.reps)
    if "long" in sections:
        long_section(a.reps, rng)
    if "parent" in sections and a.parent_lib:
        libs = {"this": _lib.lib(), "parent": C.CDLL(a.parent_lib)}
        for name in ENTRIES:
            getattr(libs["parent"], name).restype, getattr(libs["parent"], name).argtypes = _lib.SIGNATURES[name]
        held = [parent_section(n, T, batch, a.reps, libs) for (n, T, batch) in EQUAL]
        say("every row within 1 + max(0.02, the parent's own spread) of the parent's time: %s" % ("yes" if all(held) else "NO"))
        say()
        resources()
    elif "parent" in sections:
        say("this build against the parent commit's: not measured (no --parent-lib given)")
    OUT[0].close()


if __name__ == "__main__":
    main()
