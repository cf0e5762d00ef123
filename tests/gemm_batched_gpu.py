"""TEST INFRASTRUCTURE of tests/test_gpu_gemm_batched.py and tests/test_gpu_gemm_vbatched.py: the three C ABI entries of
csrc/gemm_batched.hip on flat NaN buffers (trsm_batched_gpu.Flat and Plan).  Every buffer of a call starts as NaN everywhere - the pad
rows, the gaps between blocks, a guard behind the last element, and with beta == 0 the old blocks of C too - and every call checks that
what it must not touch kept every bit and that A and B (X, Y, V, Z) kept theirs."""
import numpy as np
import torch

from tests import trsm_batched_gpu as G
from tests import vbatched_cases as VC

DEV, NOTRANS, TRANS, OK = G.DEV, G.NOTRANS, G.TRANS, G.OK
lib, stream, same = G.lib, G.stream, G.same


def flat(mats, layout):
    rows, cols = mats[0].shape
    ld = max(rows + layout[0], 1)
    return G.Flat(mats, ld, ld * cols + layout[1], False)


def run(ta, tb, As, Bs, Cs, alpha, beta, la=(0, 0), lb=(0, 0), lc=(0, 0), null_ab=False):
    """cap_dgemm_batched on the batch.  As, Bs: the mathematical op(A) (m x k) and op(B) (k x n), handed over in the layouts ta / tb name;
    Cs: the m x n C_old, or None (beta == 0: the whole buffer is NaN).  -> list of m x n results."""
    L = lib()
    batch, (m, k), n = len(As), As[0].shape, Bs[0].shape[1]
    Af, Bf = flat([a.T if ta else a for a in As], la), flat([b.T if tb else b for b in Bs], lb)
    Cf = flat([np.full((m, n), np.nan) for _ in As] if Cs is None else Cs, lc)
    st = L.cap_dgemm_batched(ta, tb, m, n, k, alpha, None if null_ab else Af.ptr(), Af.ld, Af.stride, None if null_ab else Bf.ptr(), Bf.ld,
                             Bf.stride, beta, Cf.ptr(), Cf.ld, Cf.stride, batch, stream())
    torch.cuda.synchronize()
    assert st == OK, st
    assert Af.unchanged() and Bf.unchanged(), "A or B was written"
    out, host = Cf.all()
    assert same(host[~Cf.touched], Cf.host0[~Cf.touched]), "C: an element outside the m x n rectangles was written"
    return out


def real(m, n, k, seed):
    """random real op(A) (m x k), op(B) (k x n), C_old (m x n): full 53-bit mantissas"""
    rng = np.random.default_rng([433, m, n, k, seed])
    return rng.standard_normal((m, k)), rng.standard_normal((k, n)), rng.standard_normal((m, n))


class Plan(G.Plan):
    """cap_dgemm_vbatched_inner / _combine on a vbatched_cases.Layout (only its sizes and row offsets matter: neither entry takes the flat
    tensor); the stacked operands lie in buffers of distinct NaNs with ld = rows + 2 / rows + 3"""

    def stack(self, mats, cols, pad, salt):
        """the stacked (rows x cols) matrix whose block i is mats[i] (n_i x cols), ld = rows + pad"""
        lay = self.lay
        ld = lay.rows + pad
        buf = VC.nan_pattern(ld * max(cols, 1) + 8, salt=salt)
        for i, M in enumerate(mats):
            n, r0 = int(lay.sizes[i]), int(lay.row_off[i])
            for c in range(cols):
                buf[c * ld + r0:c * ld + r0 + n] = M[:, c]
        return buf, ld

    def unstack(self, buf, ld, cols):
        lay = self.lay
        return [np.stack([buf[c * ld + int(lay.row_off[i]):c * ld + int(lay.row_off[i]) + int(lay.sizes[i])] for c in range(cols)], axis=1)
                if cols else np.zeros((int(lay.sizes[i]), 0)) for i in range(lay.batch)]

    def inner(self, Xs, Ys, Gs, alpha, beta, pad_g=(1, 3)):
        """Xs[i]: n_i x m, Ys[i]: n_i x n, Gs[i]: m x n or Gs None (beta == 0: NaN) -> list of m x n results, one per block of the batch,
        the empty ones included"""
        L, lay = lib(), self.lay
        m, n = Xs[0].shape[1], Ys[0].shape[1]
        X0, ldx = self.stack(Xs, m, 2, 11)
        Y0, ldy = self.stack(Ys, n, 3, 12)
        Gf = flat([np.full((m, n), np.nan) for _ in Xs] if Gs is None else Gs, pad_g)
        Xd, Yd = torch.from_numpy(X0.copy()).to(DEV), torch.from_numpy(Y0.copy()).to(DEV)
        st = L.cap_dgemm_vbatched_inner(self.plan, m, n, alpha, Xd.data_ptr(), ldx, Yd.data_ptr(), ldy, beta, Gf.ptr(), Gf.ld, Gf.stride, stream())
        torch.cuda.synchronize()
        assert st == OK, st
        assert VC.same_bits(Xd.cpu().numpy(), X0) and VC.same_bits(Yd.cpu().numpy(), Y0), "X or Y was written"
        out, host = Gf.all()
        assert same(host[~Gf.touched], Gf.host0[~Gf.touched]), "G: an element between or behind the blocks was written"
        return out

    def combine(self, Vs, Zs, Cs, alpha, beta, pad_z=(1, 3)):
        """Vs[i]: n_i x k, Zs[i]: k x nrhs, Cs[i]: n_i x nrhs or Cs None (beta == 0: NaN) -> list of n_i x nrhs results.  Every word of C
        outside the blocks' rows (the pad rows behind sum n_i, the guard) keeps its bits."""
        L, lay = lib(), self.lay
        k, nrhs = Zs[0].shape
        V0, ldv = self.stack(Vs, k, 2, 13)
        if Cs is None:
            ldc = lay.rows + 3
            C0 = VC.nan_pattern(ldc * max(nrhs, 1) + 8, salt=14)
        else:
            C0, ldc = self.stack(Cs, nrhs, 3, 14)
        Zf = flat(Zs, pad_z)
        Vd, Cd = torch.from_numpy(V0.copy()).to(DEV), torch.from_numpy(C0.copy()).to(DEV)
        st = L.cap_dgemm_vbatched_combine(self.plan, nrhs, k, alpha, Vd.data_ptr(), ldv, Zf.ptr(), Zf.ld, Zf.stride, beta, Cd.data_ptr(), ldc, stream())
        torch.cuda.synchronize()
        assert st == OK, st
        assert VC.same_bits(Vd.cpu().numpy(), V0) and Zf.unchanged(), "V or Z was written"
        Ch = Cd.cpu().numpy()
        keep = np.ones(Ch.shape, dtype=bool)
        for c in range(nrhs):
            keep[c * ldc:c * ldc + lay.rows] = False
        assert np.array_equal(Ch.view(np.int64)[keep], C0.view(np.int64)[keep]), "C: a row that belongs to no block was written"
        return self.unstack(Ch, ldc, nrhs)
