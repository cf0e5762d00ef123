"""Time the batched block-tridiagonal selected inverse (cap_dpotri_blocktri_batched, csrc/blocktri_potri_batched.hip).

One run, one process; every item is a window between two stream events, the items of a row alternating, median of --reps windows after
one warm-up round, fastest and slowest beside it.  The shapes (n, T, batch) of tools/blocktri_bench.py - (8, 1024, 1024),
(16, 256, 4096), (32, 128, 1024), (64, 64, 1024), (8, 10000, 64) - and (8, 256, 1024), the one whose T n = 2048 lets the dense route run.
blocktri_potri on the factors blocktri_potrf left, against
  * the host-driven composition of the fixed-size entries in the same run (the route this replaces: trsm + potri + two gemm and the
    copies and the mirror they need, per position);
  * blocktri_potrs on T n identity right-hand sides where T n <= 2048 (the whole inverse, on as many chains as fit 2 GiB);
  * a device-to-device copy of D and E, the memory floor.
The call works in place, so every window starts with a restoring copy of the factor (the floor's copy): its own time is reported and
is part of every figure, ours and the composition's alike.  Writes the table to --out and prints it:

    timeout -k 10 900 python tools/blocktri_potri_bench.py [--reps 9] [--out profiles/r30_blocktri_potri.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from capital_amd import batched, build  # noqa: E402
from tools.blocktri_bench import SHAPES, chains, fmt, run  # noqa: E402

SHAPES = SHAPES + ((8, 256, 1024),)
OUT = [None]


def say(line=""):
    print(line, flush=True)
    if OUT[0]:
        OUT[0].write(line + "\n")
        OUT[0].flush()


def compose(D, E):
    """positions descending: G = trsm; P = potri (mirrored); C = -G Sigma_next; Sigma = P - C G^T, the lower triangle of torch's reading mirrored"""
    T = D.shape[1]
    sig = None
    for i in range(T - 1, -1, -1):
        if i + 1 < T:
            batched.trsm(D[:, i], E[:, i], trans=False)
        batched.potri(D[:, i], symmetric=True)
        if i + 1 < T:
            Gt = E[:, i].clone()
            batched.gemm(sig, Gt, C=E[:, i], alpha=-1.0, beta=0.0)
            batched.gemm(Gt, E[:, i], C=D[:, i], transa=True, alpha=-1.0, beta=1.0)
        sig = torch.tril(D[:, i]) + torch.tril(D[:, i], -1).transpose(-1, -2)
        D[:, i].copy_(sig)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_blocktri_potri.txt"))
    ap.add_argument("--compose-max-positions", type=int, default=1500, help="rows with longer chains run the composition with fewer reps")
    a = ap.parse_args()
    build.build(verbose=False)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    OUT[0] = open(a.out, "w")
    say("Batched block-tridiagonal selected inverse (csrc/blocktri_potri_batched.hip) - round 30")
    say("tools/blocktri_potri_bench.py on one %s, torch %s, ONE run, median [fastest slowest] of %d windows after a warm-up round, times in ms per call"
        % (torch.cuda.get_device_name(0), torch.__version__, a.reps))
    say("device text (md5 of the gfx950 .text of the last build): " + ", ".join("%s %s" % (s, build.device_text_md5(s)) for s in (
        "potrf_batched.hip", "trsm_batched.hip", "syrk_batched.hip", "gemm_batched.hip", "potri_batched.hip", "potrf_vbatched.hip", "blocktri_batched.hip",
        "blocktri_potri_batched.hip")))
    say()
    for (n, T, batch) in SHAPES:
        D0, E0 = chains(n, T, batch)
        assert not bool(batched.blocktri_potrf(D0, E0).any())              # D0, E0: the factor
        D, E = D0.clone(), E0.clone()
        say("n = %d, T = %d, batch = %d: D and E hold %.3f GB" % (n, T, batch, (D0.numel() + E0.numel()) * 8 / 1e9))

        def restore():
            D.copy_(D0)
            E.copy_(E0)
        reps_c = a.reps if T <= a.compose_max_positions else 2
        r = run([("copy of D and E (floor)", restore), ("blocktri_potri + copy", lambda: (restore(), batched.blocktri_potri(D, E))),
                 ("blocktri_potri(symmetric) + copy", lambda: (restore(), batched.blocktri_potri(D, E, symmetric=True)))], a.reps)
        r.update(run([("composition + copy (%d positions)" % T, lambda: (restore(), compose(D, E)))], reps_c))
        restore()
        batched.blocktri_potri(D, E, symmetric=True)
        Dc, Ec = D0.clone(), E0.clone()
        compose(Dc, Ec)
        same = torch.equal(D, Dc) and torch.equal(E, Ec)
        for k, v in r.items():
            say("  %-46s %s" % (k, fmt(v)))
        fl, it, co = r["copy of D and E (floor)"][0], r["blocktri_potri + copy"][0], [v for k, v in r.items() if k.startswith("composition")][0][0]
        say("  without the copy: blocktri_potri %.3f ms = %.2f x the copy; composition %.3f ms; composition / blocktri_potri = %.2f; bits equal: %s"
            % (it - fl, (it - fl) / fl, co - fl, (co - fl) / max(it - fl, 1e-9), same))
        if T * n <= 2048:
            nb = max(1, min(batch, int(2e9 // (8 * (T * n) ** 2))))
            eye = torch.eye(T * n, dtype=torch.float64, device="cuda").expand(nb, T * n, T * n)
            B = eye.contiguous()
            rd = run([("blocktri_potrs on %d identity columns, %d chains" % (T * n, nb), lambda: (B.copy_(eye), batched.blocktri_potrs(D0[:nb], E0[:nb], B)))],
                     min(a.reps, 3))
            rc = run([("  its copy of the identity", lambda: B.copy_(eye))], min(a.reps, 3))
            for k, v in list(rd.items()) + list(rc.items()):
                say("  %-46s %s   (x %d / %d = %.3f ms for the batch)" % (k, fmt(v), batch, nb, v[0] * batch / nb))
            del B, eye
        del D0, E0, D, E, Dc, Ec
        torch.cuda.empty_cache()
        say()
    OUT[0].close()


if __name__ == "__main__":
    main()
