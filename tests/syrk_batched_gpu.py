"""TEST INFRASTRUCTURE of tests/test_gpu_syrk_batched.py and tests/test_gpu_syrk_vbatched.py: the two C ABI entries on flat NaN buffers
(trsm_batched_gpu.Flat and Plan).  Every buffer of a call starts as NaN everywhere - the strictly lower triangles, the pad rows, the gaps
between blocks, a guard behind the last element, and with beta == 0 the old upper triangles too - and every call checks that what it must
not touch is still NaN, that V kept every bit, and that with fill = 1 the strictly lower triangle is the bit-identical mirror."""
import numpy as np
import torch

from tests import trsm_batched_gpu as G
from tests import vbatched_cases as VC

DEV, NOTRANS, TRANS, UPPER, OK = G.DEV, G.NOTRANS, G.TRANS, G.UPPER, G.OK
lib, stream, same, gamma = G.lib, G.stream, G.same, G.gamma


def shapes(n, k, trans, layout_c, layout_v):
    """(ldc, stride_c, ldv, stride_v)"""
    ldc = max(n + layout_c[0], 1)
    rows, cols = (k, n) if trans else (n, k)
    ldv = max(rows + layout_v[0], 1)
    return ldc, ldc * n + layout_c[1], ldv, ldv * cols + layout_v[1]


def lower_nan(M):
    M = np.array(M, dtype=np.float64)
    M[np.tril_indices(M.shape[0], -1)] = np.nan
    return M


def run(trans, Vs, Cs, alpha, beta, lam=None, fill=0, layout_c=(0, 0), layout_v=(0, 0), null_v=False):
    """cap_dsyrk_batched on the batch.  Vs: the mathematical n x k matrices (C = alpha V V^T + ...), handed over in the layout `trans` names;
    Cs: n x n matrices whose upper triangles are C_old, or None (beta == 0: the whole buffer is NaN); lam: per-block shifts or None.
    -> list of n x n results: the upper triangle, and the lower one with fill (else zeros)."""
    L = lib()
    batch, (n, k) = len(Vs), Vs[0].shape
    ldc, sc, ldv, sv = shapes(n, k, trans, layout_c, layout_v)
    old = [np.full((n, n), np.nan) if Cs is None else lower_nan(c) for c in Cs or Vs]
    Cf = G.Flat(old, ldc, sc, not fill)
    Vf = G.Flat([v.T if trans else v for v in Vs], ldv, sv, False)
    sh = None if lam is None else torch.tensor(np.asarray(lam, dtype=np.float64), device=DEV)
    st = L.cap_dsyrk_batched(UPPER, trans, n, k, alpha, None if null_v else Vf.ptr(), ldv, sv, beta, Cf.ptr(), ldc, sc,
                             None if sh is None else sh.data_ptr(), fill, batch, stream())
    torch.cuda.synchronize()
    assert st == OK, st
    assert Vf.unchanged(), "V was written"
    out, host = Cf.all()
    assert np.isnan(host[~Cf.touched]).all(), "C: an element outside the %s was written" % ("windows" if fill else "upper triangles")
    if sh is not None:
        assert same(sh.cpu().numpy(), np.asarray(lam, dtype=np.float64))
    for m in out:
        if fill:
            assert same(np.tril(m, -1), np.triu(m, 1).T), "the lower triangle is not the mirror of the upper one"
    return out


def check_exact(out, want, fill):
    for i, (m, e) in enumerate(zip(out, want)):
        assert same(np.triu(m), np.triu(e)), "block %d" % i
        if fill:
            assert same(m, e), "block %d (mirror)" % i


class Plan(G.Plan):
    """cap_dsyrk_vbatched on a vbatched_cases.Layout: C in the layout's flat buffer, V stacked (NOTRANS: rows x k, ldv = rows + 2; TRANS:
    k x rows, ldv = k + 1) in a buffer of distinct NaNs"""

    def stacked_v(self, Vs, k, trans):
        lay = self.lay
        ldv = (k + 1) if trans else (lay.rows + 2)
        buf = VC.nan_pattern(ldv * (lay.rows if trans else k) + 8, salt=6)
        for i, v in enumerate(Vs):
            n, r0 = int(lay.sizes[i]), int(lay.row_off[i])
            for j in range(n):
                for q in range(k):
                    buf[q + (r0 + j) * ldv if trans else (r0 + j) + q * ldv] = v[j, q]
        return buf, ldv

    def run(self, trans, Vs, Cs, k, alpha, beta, lam=None, fill=0):
        """-> list of per-block results (None for empty blocks).  Asserts CAP_OK, V and shift bit for bit unchanged, every word of C outside
        the blocks' upper triangles (windows with fill) unchanged."""
        L, lay = lib(), self.lay
        if Cs is None:
            C0 = VC.nan_pattern(lay.total + VC.GUARD)
        else:
            C0 = lay.buffer([None if c is None else np.triu(c) for c in Cs])
        V0, ldv = self.stacked_v(Vs, k, trans)
        Cd, Vd = torch.from_numpy(C0.copy()).to(DEV), torch.from_numpy(V0.copy()).to(DEV)
        sh = None if lam is None else torch.tensor(np.asarray(lam, dtype=np.float64), device=DEV)
        st = L.cap_dsyrk_vbatched(self.plan, UPPER, trans, k, alpha, Vd.data_ptr(), ldv, beta, Cd.data_ptr(), None if sh is None else sh.data_ptr(),
                                  fill, stream())
        torch.cuda.synchronize()
        assert st == OK, st
        assert VC.same_bits(Vd.cpu().numpy(), V0), "V was written"
        Ch = Cd.cpu().numpy()
        keep = ~lay.written("window" if fill else "upper")
        assert np.array_equal(Ch.view(np.int64)[keep], C0.view(np.int64)[keep]), "C: a word outside the blocks was written"
        out = []
        for i in range(lay.batch):
            if not lay.sizes[i]:
                out.append(None)
                continue
            m = lay.block(Ch, i)
            if fill:
                assert same(np.tril(m, -1), np.triu(m, 1).T), "block %d: the lower triangle is not the mirror" % i
            else:
                m = np.triu(m)
            out.append(m)
        return out


def real(n, k, seed):
    """random real V (n x k), C_old (symmetric) and a shift: full 53-bit mantissas"""
    rng = np.random.default_rng([577, n, k, seed])
    V = rng.standard_normal((n, k))
    C = rng.standard_normal((n, n))
    return V, C + C.T, float(rng.standard_normal())
