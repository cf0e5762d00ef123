"""Digest of cap_dcholupdate's output bits: python tools/cholupdate_digest.py

For every shape of tests/test_gpu_cholupdate.py's OPERATOR_CASES the factor of cm.spd(n) is updated with cm.thin(n, k) and downdated again
through cap_dcholupdate (the one-launch driver); the sha256 of the two results' bytes and info words is printed per shape, then one digest
over all of them.  Two trees whose last lines agree write the same bits for these inputs - the check behind "moving the row steps of
csrc/cholupdate.hip into csrc/chud_step.h changed nothing" (profiles/r23_cholupdate_batched.txt)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from capital_amd import _lib  # noqa: E402
from tests import cholupdate_model as cm  # noqa: E402

CASES = [(1, 1), (1, 17), (2, 5), (2, 40), (63, 16), (63, 1), (64, 17), (64, 5), (65, 40), (65, 16), (127, 1), (127, 17),
         (128, 5), (128, 40), (129, 17), (129, 16), (300, 1), (300, 40), (517, 5), (517, 40)]


def main():
    L = _lib.lib()
    dev = "cuda:0"
    total = hashlib.sha256()
    for n, k in CASES:
        A, V = cm.spd(n, 10 + n), cm.thin(n, k, 100 + n)
        R = torch.from_numpy(np.ascontiguousarray(np.linalg.cholesky(A))).to(dev)       # row-major L = column-major R
        Vd = torch.from_numpy(np.ascontiguousarray(V.T)).to(dev)                        # column-major V
        work = torch.empty(max(L.cap_dcholupdate_work_size(n, k), 1), dtype=torch.float64, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        h = hashlib.sha256()
        for sign in (1, -1):
            st = L.cap_dcholupdate(1, sign, n, k, R.data_ptr(), n, Vd.data_ptr(), n, info.data_ptr(), work.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
            assert st == 0, st
            torch.cuda.synchronize()
            h.update(torch.tril(R).cpu().numpy().tobytes())
            h.update(info.cpu().numpy().tobytes())
        print("n=%4d k=%3d %s" % (n, k, h.hexdigest()[:32]))
        total.update(h.digest())
    print("cap_dcholupdate digest over %d shapes: %s" % (len(CASES), total.hexdigest()))


if __name__ == "__main__":
    main()
