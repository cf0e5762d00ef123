"""Timing of qrapply256 alone at 2^21 rows, out of place and in place (median and minimum of five launches on fresh data), through the
kernel-level entry cap_dqrapply256.  Correctness is tests/test_gpu_cqr256_exact.py (exact integer results, every grid shape)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from capital_amd import _lib
L = _lib.lib()
n = 256
st = torch.cuda.current_stream().cuda_stream
torch.manual_seed(1)
Ri = torch.triu(torch.randn(n, n, dtype=torch.float64, device="cuda")).t().contiguous()   # column-major upper
m = 1 << 21
Q = torch.randn(n, m, dtype=torch.float64, device="cuda"); Qo = torch.empty_like(Q)


def run(out):
    _lib.check(L.cap_dqrapply256(m, Q.data_ptr(), m, Ri.data_ptr(), out.data_ptr(), m, 0, st), "cap_dqrapply256")


for name, out in (("out-of-place", Qo), ("in-place", Q)):
    Q.normal_()
    run(out); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        Q.normal_()
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record(); run(out); e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    t = sorted(ts)[2]
    print("qrapply256 %s diag=%s: %.3f ms (min %.3f)  (%.0f GB/s r+w, %.1f TF useful)" % (name, os.environ.get("CAP_CQR_DIAG", "0"), t, min(ts), 16.0 * m * n / t / 1e6, m * n * (n + 16.0) / t / 1e9))
