"""Time the batched Cholesky factor and solve for blocks of 65 .. 256 rows (cap_dpotrf_batched_blocked / cap_dpotrs_batched_blocked,
csrc/potrf_batched_blocked.hip).

Per n in {96, 128, 192, 256} and per batch (1024 and 4096, which fills the chip several times over) these alternate in one process, every
one between two stream events, median of --reps after one warm-up round:
  (a) the two new calls: the factor of the whole batch (input restored outside the timed window), the solve with one right-hand side, and
      the solve with 16 right-hand sides;
  (b) at batch 1024 the only route there was before: a loop of cap_dpotrf + cap_dpotrs (one right-hand side) over the same 1024 blocks;
  (c) a device-to-device copy of the batch's 8 n^2 batch bytes.
torch.linalg.cholesky of the same batch is timed as an outside reference where it runs on the device.  TFLOP/s counts n^3 / 3 per block; the
peak it is set against is the 78.6 TFLOP/s of the fp64 MFMA.  Prints the table of profiles/r18_potrf_batched_blocked.txt:

    timeout -k 10 600 python tools/potrf_batched_blocked_bench.py [--n 96,128,192,256] [--reps 9]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402

LOOP_BLOCKS = 1024
BIG_BATCH = 4096
PEAK_TF = 78.6
NRHS = 16


def median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="96,128,192,256")
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

    print("   n   batch   factor    solve1   solve16   (a)=f+s1   (b) loop of %d   (a)/(b)   factor TF/s   of peak     copy   factor/copy   torch.linalg.cholesky"
          % LOOP_BLOCKS)
    for n in [int(x) for x in a.n.split(",")]:
        for batch in (LOOP_BLOCKS, BIG_BATCH):
            g = torch.Generator(device="cuda").manual_seed(n)
            M = torch.randn(batch, n, n, dtype=torch.float64, device="cuda", generator=g)
            A0 = torch.matmul(M, M.transpose(1, 2)) + n * torch.eye(n, dtype=torch.float64, device="cuda")
            del M
            A, A2 = torch.empty_like(A0), torch.empty_like(A0)
            B0 = torch.randn(batch, NRHS, n, dtype=torch.float64, device="cuda", generator=g)
            B = torch.empty_like(B0)
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            work = torch.empty(max(int(L.cap_dpotrf_work_size(n)), int(L.cap_dpotrs_work_size(n, 1)), 2), dtype=torch.float64, device="cuda")
            info1 = torch.zeros(1, dtype=torch.int32, device="cuda")
            nb = n * n * 8
            do_loop = batch == LOOP_BLOCKS

            def factor():
                _lib.check(L.cap_dpotrf_batched_blocked(1, n, A.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp), "potrf_batched_blocked")

            def solve(nrhs):
                _lib.check(L.cap_dpotrs_batched_blocked(1, n, nrhs, A.data_ptr(), n, n * n, B.data_ptr(), n, n * NRHS, batch, info.data_ptr(), sp),
                           "potrs_batched_blocked")

            def loop():
                for i in range(LOOP_BLOCKS):
                    _lib.check(L.cap_dpotrf(1, n, A.data_ptr() + i * nb, n, info1.data_ptr(), work.data_ptr(), sp), "potrf")
                    _lib.check(L.cap_dpotrs(1, n, 1, A.data_ptr() + i * nb, n, B.data_ptr() + i * n * NRHS * 8, n, work.data_ptr(), sp), "potrs")

            tf, ts, ts16, tl, tc = [], [], [], [], []
            for rep in range(a.reps + 1):
                A.copy_(A0); B.copy_(B0)
                tf.append(timed(factor))
                ts.append(timed(lambda: solve(1)))
                if rep == 0:
                    assert int(info.abs().max().item()) == 0
                    X = B[:, 0].clone()
                B.copy_(B0)
                ts16.append(timed(lambda: solve(NRHS)))
                if rep == 0:          # a column's bits do not depend on how many travel with it
                    assert torch.equal(B[:, 0], X)
                if do_loop:
                    A.copy_(A0); B.copy_(B0)
                    tl.append(timed(loop))
                    if rep == 0:      # both routes solve the same systems
                        err = float((B[:, 0] - X).abs().max().item())
                        assert err < 1e-9, err
                tc.append(timed(lambda: A2.copy_(A0)))
            f, so, s16, c = median(tf[1:]), median(ts[1:]), median(ts16[1:]), median(tc[1:])
            lo = median(tl[1:]) if do_loop else float("nan")
            tt = "not run"
            if not a.no_torch:
                try:
                    tq = [timed(lambda: torch.linalg.cholesky(A0)) for _ in range(4)]
                    tt = "%.3f" % median(tq[1:])
                except Exception as e:      # no device path in this build
                    tt = "does not run here (%s)" % type(e).__name__
            tf_s = batch * n ** 3 / 3.0 / (f * 1e-3) / 1e12
            print("%4d %7d %8.4f %8.4f %9.4f %10.4f %16s %9s %13.3f %8.1f%% %8.4f %13.3f   %s"
                  % (n, batch, f, so, s16, f + so, "%.3f" % lo if do_loop else "-", "%.5f" % ((f + so) / lo) if do_loop else "-", tf_s,
                     100.0 * tf_s / PEAK_TF, c, c / f, tt), flush=True)
            del A0, A, A2


if __name__ == "__main__":
    main()
