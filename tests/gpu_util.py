"""Helpers for the -m gpu parity tests: the HIP path (through the C ABI) vs the CPU oracle."""
import numpy as np
import torch

DEV = "cuda:0"


def to_dev(a, ld=None):
    """numpy (rows, cols) -> column-major device buffer with leading dimension ld; returns (buf, view[row, col])."""
    a = np.asarray(a, dtype=np.float64)
    rows, cols = a.shape
    ld = ld or rows
    buf = torch.full((cols, ld), float("nan"), dtype=torch.float64, device=DEV)
    buf[:, :rows] = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)
    return buf, buf[:, :rows].t()


SENTINEL = 4096


class NanWork:
    """device scratch the way the exact-result suites hand it over: exactly `size` doubles, all NaN, with a sentinel of SENTINEL doubles
    (NaNs with a payload of their own each) behind it.  A read of scratch the call never wrote shows as NaN in its result, a write past the
    stated size in check()."""

    def __init__(self, size):
        self.size = int(size)
        bits = np.int64(0x7ff8000000000000) | np.arange(1, self.size + SENTINEL + 1, dtype=np.int64)
        self.host = bits.view(np.float64).copy()
        self.buf = torch.from_numpy(self.host.copy()).to(DEV)

    def data_ptr(self):
        return self.buf.data_ptr()

    def check(self, what="the call"):
        torch.cuda.synchronize()
        tail = self.buf[self.size:].cpu().numpy()
        assert tail.size == SENTINEL and np.array_equal(tail.view(np.int64), self.host[self.size:].view(np.int64)), \
            "%s wrote behind the %d doubles of scratch it asked for" % (what, self.size)


def to_host(view):
    return view.detach().cpu().numpy().copy()


def relerr(x, ref):
    d = np.linalg.norm(np.asarray(x) - np.asarray(ref))
    n = np.linalg.norm(ref)
    return d / n if n > 0 else d
