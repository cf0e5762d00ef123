"""Time the batched SPD inverse and triangular inverse (cap_dpotri_batched / cap_dtrtri_batched, csrc/potri_batched.hip).

Per n in {8, 16, 32, 64, 96, 128, 192, 256} and per batch (1024 and the large one of the factor's profiles: 2^16 for n <= 32, 2^14 for n = 64,
4096 above) these alternate in one process, every one between two stream events, median of --reps after one warm-up round; the factors are
restored outside the timed window:
  potri   cap_dpotri_batched with info, fill = 0 and fill = 1;
  trtri   cap_dtrtri_batched alone;
  (a)     the route potri replaces: cap_dpotrs_batched[_blocked] with info on a batch of identity matrices (2 n^3 flops per block
          instead of 2 n^3 / 3, a second batch-sized buffer);
  (b)     at batch 1024: a loop of cap_dpotri over the same 1024 blocks;
  (c)     torch.cholesky_inverse of the same factors (torch's row-major reading: L = R^T);
  copy    a device-to-device copy of the batch's 8 n^2 batch bytes.
GFLOP/s counts 2 n^3 / 3 per block.  Prints the table of profiles/r21_potri_batched.txt:

    timeout -k 10 900 python tools/potri_batched_bench.py [--n 8,16,32,64,96,128,192,256] [--reps 9]
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


def big_batch(n):
    return 1 << 16 if n <= 32 else 1 << 14 if n <= 64 else 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="8,16,32,64,96,128,192,256")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-torch", action="store_true", help="leave torch.cholesky_inverse out")
    ap.add_argument("--no-loop", action="store_true", help="leave the loop over cap_dpotri out")
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

    print("   n   batch    potri   potri fill    trtri   (a) potrs on I   potri/(a)   (b) loop of %d   potri/(b)   (c) torch   potri GF/s     copy   potri/copy"
          % LOOP_BLOCKS)
    for n in [int(x) for x in a.n.split(",")]:
        for batch in (LOOP_BLOCKS, big_batch(n)):
            g = torch.Generator(device="cuda").manual_seed(n)
            M = torch.randn(batch, n, n, dtype=torch.float64, device="cuda", generator=g)
            R0 = torch.matmul(M, M.transpose(1, 2)) + n * torch.eye(n, dtype=torch.float64, device="cuda")
            del M
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            fac = L.cap_dpotrf_batched if n <= 64 else L.cap_dpotrf_batched_blocked
            sol = L.cap_dpotrs_batched if n <= 64 else L.cap_dpotrs_batched_blocked
            _lib.check(fac(1, n, R0.data_ptr(), n, n * n, batch, info.data_ptr(), None, sp), "potrf_batched")
            assert int(info.abs().max().item()) == 0
            R, R2 = torch.empty_like(R0), torch.empty_like(R0)
            eye = torch.eye(n, dtype=torch.float64, device="cuda").repeat(batch, 1, 1)
            X = torch.empty_like(eye)
            work = torch.empty(max(int(L.cap_dpotri_work_size(n)), 2), dtype=torch.float64, device="cuda")
            nb = n * n * 8
            do_loop = batch == LOOP_BLOCKS and not a.no_loop

            def potri(fill):
                _lib.check(L.cap_dpotri_batched(1, n, R.data_ptr(), n, n * n, batch, info.data_ptr(), fill, sp), "potri_batched")

            def trtri():
                _lib.check(L.cap_dtrtri_batched(1, n, R.data_ptr(), n, n * n, batch, info.data_ptr(), sp), "trtri_batched")

            def route_a():
                _lib.check(sol(1, n, n, R.data_ptr(), n, n * n, X.data_ptr(), n, n * n, batch, info.data_ptr(), sp), "potrs_batched")

            def loop():
                for i in range(LOOP_BLOCKS):
                    _lib.check(L.cap_dpotri(1, n, R.data_ptr() + i * nb, n, work.data_ptr(), sp), "potri")

            tp, tpf, tt, ta, tl, tc = [], [], [], [], [], []
            for rep in range(a.reps + 1):
                R.copy_(R0)
                tp.append(timed(lambda: potri(0)))
                if rep == 0:
                    ref = R.clone()
                R.copy_(R0)
                tpf.append(timed(lambda: potri(1)))
                if rep == 0:          # fill = 1: the same upper triangle (the column-major upper triangle is torch's lower one) and its mirror
                    assert torch.equal(torch.tril(R), torch.tril(ref)) and torch.equal(R, R.transpose(1, 2))
                R.copy_(R0)
                tt.append(timed(trtri))
                R.copy_(R0); X.copy_(eye)
                ta.append(timed(route_a))
                if rep == 0:          # both routes invert the same matrices
                    err = float((torch.tril(X) - torch.tril(ref)).abs().max().item() / ref.abs().max().item())
                    assert err < 1e-9, err
                if do_loop:
                    R.copy_(R0)
                    tl.append(timed(loop))
                    if rep == 0:
                        err = float((torch.tril(R) - torch.tril(ref)).abs().max().item() / ref.abs().max().item())
                        assert err < 1e-9, err
                tc.append(timed(lambda: R2.copy_(R0)))
            p, pf, t, ra, c = median(tp[1:]), median(tpf[1:]), median(tt[1:]), median(ta[1:]), median(tc[1:])
            lo = median(tl[1:]) if do_loop else float("nan")
            tq = "not run"
            if not a.no_torch:
                try:
                    Lt = torch.tril(R0)           # torch's reading of the same memory: L = R^T
                    q = [timed(lambda: torch.cholesky_inverse(Lt)) for _ in range(4)]
                    tq = "%.3f" % median(q[1:])
                    del Lt
                except Exception as e:      # no device path in this build
                    tq = "does not run here (%s)" % type(e).__name__
            gf = batch * 2.0 * n ** 3 / 3.0 / (p * 1e-3) / 1e9
            print("%4d %7d %8.4f %12.4f %8.4f %16.4f %11.3f %16s %11s %11s %12.1f %8.4f %12.2f"
                  % (n, batch, p, pf, t, ra, p / ra, "%.3f" % lo if do_loop else "-", "%.5f" % (p / lo) if do_loop else "-", tq, gf, c, p / c), flush=True)
            del R0, R, R2, eye, X


if __name__ == "__main__":
    main()
