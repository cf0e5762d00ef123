"""Time the batched block-tridiagonal Cholesky (cap_dpotrf_blocktri_batched, cap_dpotrs_blocktri_batched, csrc/blocktri_batched.hip).

One run, one process; every item is a window between two stream events, the items of a row alternating, median of --reps windows after
one warm-up round, fastest and slowest beside it.  Shapes (n, T, batch): (8, 1024, 1024), (16, 256, 4096), (32, 128, 1024),
(64, 64, 1024) and (8, 10000, 64) - a few long chains, the corner that is expected to be bound by latency.  The factor and the solve
(nrhs = 1 and 16) against
  * the host-driven composition of the existing entries in the same run (the route this replaces: potrf + trsm + syrk per position,
    trsm + gemm per position and sweep) - its kernels are the parent commit's, their device text is unchanged;
  * torch.linalg.cholesky + torch.cholesky_solve on the assembled dense matrices where T n <= 2048 (on as many chains as fit 2 GiB);
  * a device-to-device copy of D and E, the memory floor of the factor.
The factor works in place, so every window starts with a restoring copy of D and E (the floor's copy): the copy's own time is reported
and is part of every factor figure, ours and the composition's alike.  Writes the table to --out and prints it:

    timeout -k 10 900 python tools/blocktri_bench.py [--reps 9] [--out profiles/r29_blocktri_batched.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from capital_amd import batched, build  # noqa: E402

SHAPES = ((8, 1024, 1024), (16, 256, 4096), (32, 128, 1024), (64, 64, 1024), (8, 10000, 64))
OUT = [None]


def say(line=""):
    print(line, flush=True)
    if OUT[0]:
        OUT[0].write(line + "\n")
        OUT[0].flush()


def stats(x):
    x = sorted(x[1:])                       # the first round is the warm-up
    return x[len(x) // 2], x[0], x[-1]


def timed(fn):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def run(items, reps):
    t = {k: [] for k, _ in items}
    for _ in range(reps + 1):
        for k, fn in items:
            t[k].append(timed(fn))
    return {k: stats(v) for k, v in t.items()}


def fmt(s):
    return "%10.3f [%9.3f %9.3f]" % s


def chains(n, T, batch):
    """diagonally dominant chains: D (batch, T, n, n) symmetric, E (batch, T - 1, n, n)"""
    g = torch.Generator(device="cuda").manual_seed(n * 1000 + T)
    E = torch.rand(batch, T - 1, n, n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    S = torch.rand(batch, T, n, n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1
    D = 0.5 * (S + S.transpose(-1, -2)) + (3.0 * n + 1.5) * torch.eye(n, dtype=torch.float64, device="cuda")
    return D, E


def compose_factor(D, E):
    T = D.shape[1]
    for i in range(T):
        info = batched.potrf(D[:, i])
        if i + 1 < T:
            batched.schur(D[:, i], E[:, i], D[:, i + 1], info)


def compose_solve(D, E, B, tmp):
    T, n = D.shape[1], D.shape[2]
    seg = lambda i: B[:, :, i * n:(i + 1) * n]
    for i in range(T):
        batched.trsm(D[:, i], seg(i), trans=True)
        if i + 1 < T:
            tmp.copy_(seg(i))
            batched.gemm(tmp, E[:, i], C=seg(i + 1), transb=True, alpha=-1.0, beta=1.0)
    for i in range(T - 1, -1, -1):
        if i + 1 < T:
            tmp.copy_(seg(i + 1))
            batched.gemm(tmp, E[:, i], C=seg(i), alpha=-1.0, beta=1.0)
        batched.trsm(D[:, i], seg(i), trans=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_blocktri_batched.txt"))
    ap.add_argument("--compose-max-launches", type=int, default=40000, help="rows whose composition needs more launches per call run it with fewer reps")
    a = ap.parse_args()
    build.build(verbose=False)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    OUT[0] = open(a.out, "w")
    say("Batched block-tridiagonal Cholesky (csrc/blocktri_batched.hip) - round 29")
    say("tools/blocktri_bench.py on one %s, torch %s, ONE run, median [fastest slowest] of %d windows after a warm-up round, times in ms per call"
        % (torch.cuda.get_device_name(0), torch.__version__, a.reps))
    say("device text (md5 of the gfx950 .text of the last build): " + ", ".join("%s %s" % (s, build.device_text_md5(s)) for s in (
        "potrf_batched.hip", "trsm_batched.hip", "syrk_batched.hip", "gemm_batched.hip", "potrf_vbatched.hip", "blocktri_batched.hip")))
    say()
    for (n, T, batch) in SHAPES:
        D0, E0 = chains(n, T, batch)
        D, E = D0.clone(), E0.clone()
        gb = (D0.numel() + E0.numel()) * 8 / 1e9
        say("n = %d, T = %d, batch = %d: D and E hold %.3f GB" % (n, T, batch, gb))

        def restore():
            D.copy_(D0)
            E.copy_(E0)
        reps_c = a.reps if 3 * T <= a.compose_max_launches // 10 else 2
        items = [("copy of D and E (floor)", restore), ("blocktri_potrf + copy", lambda: (restore(), batched.blocktri_potrf(D, E)))]
        r = run(items, a.reps)
        rc = run([("composition + copy (%d launches)" % (3 * T - 2), lambda: (restore(), compose_factor(D, E)))], reps_c)
        r.update(rc)
        restore()
        info = batched.blocktri_potrf(D, E)
        assert not bool(info.any())
        Dc, Ec = D0.clone(), E0.clone()
        compose_factor(Dc, Ec)
        same = torch.equal(torch.tril(D), torch.tril(Dc)) and torch.equal(E, Ec)
        for k, v in r.items():
            say("  factor  %-44s %s" % (k, fmt(v)))
        fl, it, co = r["copy of D and E (floor)"][0], r["blocktri_potrf + copy"][0], [v for k, v in r.items() if k.startswith("composition")][0][0]
        say("  factor  without the copy: blocktri_potrf %.3f ms = %.2f x the copy; composition %.3f ms; composition / blocktri_potrf = %.2f; bits equal: %s"
            % (it - fl, (it - fl) / fl, co - fl, (co - fl) / max(it - fl, 1e-9), same))
        dense = None
        if T * n <= 2048:
            nb = max(1, min(batch, int(2e9 // (8 * (T * n) ** 2))))
            A = torch.zeros(nb, T * n, T * n, dtype=torch.float64, device="cuda")
            for i in range(T):
                A[:, i * n:(i + 1) * n, i * n:(i + 1) * n] = D0[:nb, i]
                if i + 1 < T:
                    A[:, (i + 1) * n:(i + 2) * n, i * n:(i + 1) * n] = E0[:nb, i]
                    A[:, i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = E0[:nb, i].transpose(-1, -2)
            rd = run([("torch.linalg.cholesky, dense, %d chains" % nb, lambda: torch.linalg.cholesky(A))], min(a.reps, 3))
            for k, v in rd.items():
                say("  factor  %-44s %s   (x %d / %d = %.3f ms for the batch)" % (k, fmt(v), batch, nb, v[0] * batch / nb))
            dense = (A, torch.linalg.cholesky(A), nb)
        for nrhs in (1, 16):
            B0 = torch.rand(batch, nrhs, T * n, dtype=torch.float64, device="cuda") * 2 - 1
            B = B0.clone()
            tmp = torch.empty(batch, nrhs, n, dtype=torch.float64, device="cuda")
            items = [("copy of B", lambda: B.copy_(B0)), ("blocktri_potrs + copy", lambda: (B.copy_(B0), batched.blocktri_potrs(D, E, B)))]
            r = run(items, a.reps)
            r.update(run([("composition + copy (%d launches)" % (6 * T - 4), lambda: (B.copy_(B0), compose_solve(D, E, B, tmp)))], reps_c))
            B.copy_(B0)
            batched.blocktri_potrs(D, E, B)
            Bc = B0.clone()
            compose_solve(D, E, Bc, tmp)
            same = torch.equal(B, Bc)
            for k, v in r.items():
                say("  solve nrhs = %-2d  %-36s %s" % (nrhs, k, fmt(v)))
            fl, it, co = r["copy of B"][0], r["blocktri_potrs + copy"][0], [v for k, v in r.items() if k.startswith("composition")][0][0]
            say("  solve nrhs = %-2d  without the copy: blocktri_potrs %.3f ms; composition %.3f ms; composition / blocktri_potrs = %.2f; bits equal: %s"
                % (nrhs, it - fl, co - fl, (co - fl) / max(it - fl, 1e-9), same))
            if dense is not None:
                A, Lc, nb = dense
                Bd = B0[:nb].transpose(-1, -2).contiguous()
                rd = run([("torch.cholesky_solve, dense, %d chains" % nb, lambda: torch.cholesky_solve(Bd, Lc))], min(a.reps, 3))
                for k, v in rd.items():
                    say("  solve nrhs = %-2d  %-36s %s   (x %d / %d = %.3f ms for the batch)" % (nrhs, k, fmt(v), batch, nb, v[0] * batch / nb))
            del B0, B, tmp
        del dense, D0, E0, D, E
        torch.cuda.empty_cache()
        say()
    OUT[0].close()


if __name__ == "__main__":
    main()
