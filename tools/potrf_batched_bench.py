"""Time the batched Cholesky factor and solve (cap_dpotrf_batched / cap_dpotrs_batched, csrc/potrf_batched.hip) on many small SPD blocks.

Per n in {8, 16, 32, 64} and per batch (1024 and a large one: 2^16 for n <= 32, 2^14 for n = 64) three things alternate in one process, every
one between two stream events, median of --reps after one warm-up round:
  (a) the two new calls: the factor of the whole batch (input restored outside the timed window), then the solve with one right-hand side;
  (b) the only route there was before: a loop of cap_dpotrf + cap_dpotrs over the first 1024 blocks;
  (c) a device-to-device copy of the batch's 8 n^2 batch bytes - it reads and writes as many bytes as the factor has to (16 n^2 batch), so
      (c) / factor time is the factor's share of the copy rate of that run.
torch.linalg.cholesky of the same batch is timed as an outside reference where it runs on the device.  Prints the table of
profiles/r17_potrf_batched.txt:

    timeout -k 10 600 python tools/potrf_batched_bench.py [--n 8,16,32,64] [--reps 9]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402

LOOP_BLOCKS = 1024


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="8,16,32,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-torch", action="store_true", help="leave torch.linalg.cholesky out")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    print("device: %s, torch %s, %d reps (median), times in ms" % (torch.cuda.get_device_name(0), torch.__version__, a.reps))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    print("   n   batch   factor    solve1   (a)=f+s   (b) loop of %d   (a)/(b)     copy   copy TB/s   factor TB/s   factor/copy   torch.linalg.cholesky"
          % LOOP_BLOCKS)
    for n in [int(x) for x in a.n.split(",")]:
        for batch in (1024, 1 << 16 if n <= 32 else 1 << 14):
            g = torch.Generator(device="cuda").manual_seed(n)
            M = torch.randn(batch, n, n, dtype=torch.float64, device="cuda", generator=g)
            A0 = torch.matmul(M, M.transpose(1, 2)) + n * torch.eye(n, dtype=torch.float64, device="cuda")
            del M
            A, A2 = torch.empty_like(A0), torch.empty_like(A0)
            B0 = torch.randn(batch, n, dtype=torch.float64, device="cuda", generator=g)
            B = torch.empty_like(B0)
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            work = torch.empty(max(int(L.cap_dpotrf_work_size(n)), int(L.cap_dpotrs_work_size(n, 1)), 2), dtype=torch.float64, device="cuda")
            info1 = torch.zeros(1, dtype=torch.int32, device="cuda")
            nb = n * n * 8
            do_loop = batch == 1024

            def factor():
                _lib.check(L.cap_dpotrf_batched(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp), "potrf_batched")

            def solve():
                _lib.check(L.cap_dpotrs_batched(1, n, 1, A.data_ptr(), n, n * n, B.data_ptr(), n, n, batch, info.data_ptr(), sp), "potrs_batched")

            def loop():
                for i in range(LOOP_BLOCKS):
                    _lib.check(L.cap_dpotrf(1, n, A.data_ptr() + i * nb, n, info1.data_ptr(), work.data_ptr(), sp), "potrf")
                    _lib.check(L.cap_dpotrs(1, n, 1, A.data_ptr() + i * nb, n, B.data_ptr() + i * n * 8, n, work.data_ptr(), sp), "potrs")

            tf, ts, tl, tc = [], [], [], []
            for rep in range(a.reps + 1):
                A.copy_(A0); B.copy_(B0)
                tf.append(timed(factor))
                ts.append(timed(solve))
                if rep == 0:
                    assert int(info.abs().max().item()) == 0
                    X = B.clone()
                if do_loop:
                    A.copy_(A0); B.copy_(B0)
                    tl.append(timed(loop))
                    if rep == 0:      # both routes solve the same systems
                        err = float((B[:LOOP_BLOCKS] - X[:LOOP_BLOCKS]).abs().max().item())
                        assert err < 1e-9, err
                tc.append(timed(lambda: A2.copy_(A0)))
            f, so, c = median(tf[1:]), median(ts[1:]), median(tc[1:])
            lo = median(tl[1:]) if do_loop else float("nan")
            tt = "not run"
            if not a.no_torch:
                try:
                    tq = [timed(lambda: torch.linalg.cholesky(A0)) for _ in range(4)]
                    tt = "%.3f" % median(tq[1:])
                except Exception as e:      # no device path in this build
                    tt = "does not run here (%s)" % type(e).__name__
            byt = 16.0 * n * n * batch
            print("%4d %7d %8.4f %8.4f %9.4f %16s %9s %8.4f %10.3f %12.3f %12.3f   %s"
                  % (n, batch, f, so, f + so, "%.3f" % lo if do_loop else "-", "%.5f" % ((f + so) / lo) if do_loop else "-", c,
                     byt / (c * 1e-3) / 1e12, byt / (f * 1e-3) / 1e12, c / f, tt), flush=True)
            del A0, A, A2


if __name__ == "__main__":
    main()
