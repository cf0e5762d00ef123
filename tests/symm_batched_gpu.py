"""TEST INFRASTRUCTURE of tests/test_gpu_symm_batched.py, tests/test_gpu_symm_vbatched.py and tests/test_gpu_symm_batched_stream.py: the
eight C ABI entries of csrc/symm_batched.hip on flat NaN buffers (trsm_batched_gpu.Flat and Plan).  Every buffer of a call starts as NaN
everywhere outside what the call may read - the strictly lower triangles, the pad rows, the gaps between blocks, a guard behind the last
element, with beta == 0 the whole of B, the whole of Y - and every call checks that what it must not touch kept every bit and that its
inputs were not written."""
import numpy as np
import torch

from tests import trsm_batched_gpu as G
from tests import vbatched_cases as VC

DEV, UPPER, OK = G.DEV, G.UPPER, G.OK
lib, stream, same = G.lib, G.stream, G.same
NAN_BITS = np.int64(0x7ff8000000000000)


def flat(mats, layout, tri=False):
    rows, cols = mats[0].shape
    ld = max(rows + layout[0], 1)
    return G.Flat(mats, ld, ld * cols + layout[1], tri)


def vec(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def ptr(t):
    return None if t is None else (t.ptr() if isinstance(t, G.Flat) else t.data_ptr())


def symm(As, Xs, Bs, alpha, beta, absolute=0, la=(0, 0), lx=(0, 0), inplace=False, null_ax=False):
    """cap_dsymm_batched -> list of n x nrhs results.  As: symmetric matrices (only their upper triangles are laid in); Bs None: B is
    NULL with beta == 0, a buffer of NaN otherwise expected (beta == 0 hands over NaN blocks to show that B is not read)."""
    L = lib()
    batch, (n, nrhs) = len(Xs), Xs[0].shape
    Af, Xf = flat(As, la, True), flat(Xs, lx)
    nanb = [np.full((n, nrhs), np.nan) for _ in Xs]
    Bf = flat(nanb if beta == 0.0 else Bs, lx)
    Yf = Bf if inplace else flat(nanb, (lx[0] + 1, lx[1] + 2))
    st = L.cap_dsymm_batched(UPPER, absolute, n, nrhs, alpha, None if null_ax else Af.ptr(), Af.ld, Af.stride, None if null_ax else Xf.ptr(),
                             Xf.ld, Xf.stride, beta, Bf.ptr(), Bf.ld, Bf.stride, Yf.ptr(), Yf.ld, Yf.stride, batch, stream())
    torch.cuda.synchronize()
    assert st == OK, st
    assert Af.unchanged() and Xf.unchanged(), "A or X was written"
    if not inplace:
        assert Bf.unchanged(), "B was written"
    out, host = Yf.all()
    assert np.isnan(host[~Yf.touched]).all(), "Y: an element outside the windows was written"
    return out


def norm(As, la=(0, 0), upper=None):
    """cap_dlansy_batched -> (batch,) array.  upper: the triangles to lay in where they are not those of As (NaN probes)"""
    L = lib()
    n = As[0].shape[0]
    Af = flat(As if upper is None else upper, la, True)
    out = vec(np.full(len(As) + 2, np.nan))
    st = L.cap_dlansy_batched(ord('1'), UPPER, n, Af.ptr(), Af.ld, Af.stride, len(As), out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert st == OK, st
    assert Af.unchanged()
    o = out.cpu().numpy()
    assert np.isnan(o[len(As):]).all()
    return o[:len(As)]


def potri(Rs):
    """cap_dpotri_batched on a copy of the factors -> list of symmetric inverses (the mirror of the computed upper triangle)"""
    L = lib()
    n = Rs[0].shape[0]
    Rf = flat(Rs, (0, 0), True)
    assert L.cap_dpotri_batched(UPPER, n, Rf.ptr(), Rf.ld, Rf.stride, len(Rs), None, 0, stream()) == OK
    torch.cuda.synchronize()
    from tests.symm_batched_cases import sym
    return [sym(m) for m in Rf.all()[0]]


def rcond(Rs, anorm, info=None, lr=(0, 0)):
    """cap_dpocon_batched -> (batch,) array; R unchanged bit for bit, anorm and info too"""
    L = lib()
    batch, n = len(Rs), Rs[0].shape[0]
    Rf = flat(Rs, lr, True)
    an, inf = vec(anorm), vec(info, np.int32)
    out = vec(np.full(batch + 2, np.nan))
    work = vec(np.full(int(L.cap_dpocon_batched_work_size(n, batch)) + 4, np.nan))
    st = L.cap_dpocon_batched(UPPER, n, Rf.ptr(), Rf.ld, Rf.stride, batch, an.data_ptr(), ptr(inf), out.data_ptr(), work.data_ptr(), stream())
    torch.cuda.synchronize()
    assert st == OK, st
    assert Rf.unchanged(), "R was written"
    assert same(an.cpu().numpy(), np.asarray(anorm, dtype=np.float64))
    assert np.isnan(work.cpu().numpy()[-4:]).all(), "work: written behind its stated size"
    o = out.cpu().numpy()
    assert np.isnan(o[batch:]).all()
    return o[:batch]


def poerr(As, Rs, Bs, Xs, info=None, want_ferr=True, want_berr=True, la=(0, 0), lx=(0, 0), pad=0):
    """cap_dpoerr_batched -> (ferr, berr), (batch, nrhs) arrays or None; lde = nrhs + pad; A, R, B, X unchanged bit for bit"""
    L = lib()
    batch, (n, nrhs) = len(Xs), Xs[0].shape
    Af, Rf, Bf, Xf = flat(As, la, True), flat(Rs, (la[1] % 4, la[0]), True), flat(Bs, lx), flat(Xs, (lx[0] + 2, lx[1] + 1))
    lde = nrhs + pad
    fe = vec(np.full(batch * lde + 2, np.nan)) if want_ferr else None
    be = vec(np.full(batch * lde + 2, np.nan)) if want_berr else None
    work = vec(np.full(int(L.cap_dpoerr_batched_work_size(n, nrhs, batch)) + 4, np.nan)) if want_ferr else None
    inf = vec(info, np.int32)
    st = L.cap_dpoerr_batched(UPPER, n, nrhs, Af.ptr(), Af.ld, Af.stride, Rf.ptr(), Rf.ld, Rf.stride, Bf.ptr(), Bf.ld, Bf.stride, Xf.ptr(), Xf.ld,
                              Xf.stride, batch, ptr(inf), ptr(fe), ptr(be), lde, ptr(work), stream())
    torch.cuda.synchronize()
    assert st == OK, st
    assert Af.unchanged() and Rf.unchanged() and Bf.unchanged() and Xf.unchanged(), "an input was written"
    if work is not None:
        assert np.isnan(work.cpu().numpy()[-4:]).all(), "work: written behind its stated size"
    res = []
    for t in (fe, be):
        if t is None:
            res.append(None)
            continue
        h = t.cpu().numpy()
        m = h[:batch * lde].reshape(batch, lde)
        assert np.isnan(h[batch * lde:]).all() and np.isnan(m[:, nrhs:]).all(), "ferr / berr: written outside batch x nrhs"
        res.append(m[:, :nrhs].copy())
    return res[0], res[1]


class Plan(G.Plan):
    """the four _vbatched entries on a vbatched_cases.Layout: A / R in the layout's flat buffer, X / B / Y stacked (ld = rows + 2) in
    buffers of distinct NaNs"""

    def live(self):
        return [i for i in range(self.lay.batch) if self.lay.sizes[i]]

    def unstack(self, buf, ld, nrhs):
        lay, out = self.lay, []
        for i in range(lay.batch):
            n, r0 = int(lay.sizes[i]), int(lay.row_off[i])
            out.append(None if not n else np.array([buf[k * ld + r0:k * ld + r0 + n] for k in range(nrhs)]).reshape(nrhs, n).T.copy())
        return out

    def pad_untouched(self, before, after, ld, nrhs):
        pad = np.ones(before.shape, dtype=bool)
        for k in range(nrhs):
            pad[k * ld:k * ld + self.lay.rows] = False
        return np.array_equal(before.view(np.int64)[pad], after.view(np.int64)[pad])

    def mats(self, Ms):
        return self.lay.buffer([None if m is None else np.triu(m) for m in Ms])

    def symm(self, As, Xs, Bs, nrhs, alpha, beta, absolute=0, inplace=False):
        L, lay = lib(), self.lay
        A0 = self.mats(As)
        X0, ldx = self.stacked(Xs, nrhs)
        B0, ldb = self.stacked(Bs if beta != 0.0 else [None if x is None else np.full(x.shape, np.nan) for x in Xs], nrhs)
        Y0 = VC.nan_pattern(B0.size, salt=9)
        Ad, Xd, Bd, Yd = (vec(t) for t in (A0, X0, B0, Y0))
        if inplace:
            Yd, Y0 = Bd, B0
        st = L.cap_dsymm_vbatched(self.plan, UPPER, absolute, nrhs, alpha, Ad.data_ptr(), Xd.data_ptr(), ldx, beta, Bd.data_ptr(), ldb,
                                  Yd.data_ptr(), ldb, stream())
        torch.cuda.synchronize()
        assert st == OK, st
        assert VC.same_bits(Ad.cpu().numpy(), A0) and VC.same_bits(Xd.cpu().numpy(), X0), "A or X was written"
        if not inplace:
            assert VC.same_bits(Bd.cpu().numpy(), B0), "B was written"
        Yh = Yd.cpu().numpy()
        assert self.pad_untouched(Y0, Yh, ldb, nrhs), "Y: a pad row was written"
        return self.unstack(Yh, ldb, nrhs)

    def norm(self, As):
        L, lay = lib(), self.lay
        A0 = self.mats(As)
        Ad, out = vec(A0), vec(np.full(lay.batch + 2, -7.5))
        st = L.cap_dlansy_vbatched(self.plan, ord('O'), UPPER, Ad.data_ptr(), out.data_ptr(), stream())
        torch.cuda.synchronize()
        assert st == OK, st
        assert VC.same_bits(Ad.cpu().numpy(), A0)
        o = out.cpu().numpy()
        assert all(o[i] == -7.5 for i in range(lay.batch + 2) if i >= lay.batch or not lay.sizes[i]), "an entry of an empty block was written"
        return o[:lay.batch]

    def rcond(self, Rs, anorm, info=None):
        L, lay = lib(), self.lay
        R0 = self.mats(Rs)
        Rd, an, inf, out = vec(R0), vec(anorm), vec(info, np.int32), vec(np.full(lay.batch + 2, -7.5))
        work = vec(np.full(int(L.cap_dpocon_vbatched_work_size(self.plan)) + 4, np.nan))
        st = L.cap_dpocon_vbatched(self.plan, UPPER, Rd.data_ptr(), an.data_ptr(), ptr(inf), out.data_ptr(), work.data_ptr(), stream())
        torch.cuda.synchronize()
        assert st == OK, st
        assert VC.same_bits(Rd.cpu().numpy(), R0), "R was written"
        assert np.isnan(work.cpu().numpy()[-4:]).all()
        o = out.cpu().numpy()
        assert all(o[i] == -7.5 for i in range(lay.batch + 2) if i >= lay.batch or not lay.sizes[i]), "an entry of an empty block was written"
        return o[:lay.batch]

    def poerr(self, As, Rs, Bs, Xs, nrhs, info=None, want_ferr=True):
        L, lay = lib(), self.lay
        A0, R0 = self.mats(As), self.mats(Rs)
        B0, ldb = self.stacked(Bs, nrhs)
        X0, ldx = self.stacked(Xs, nrhs)
        Ad, Rd, Bd, Xd, inf = vec(A0), vec(R0), vec(B0), vec(X0), vec(info, np.int32)
        lde = nrhs + 1
        fe = vec(np.full(lay.batch * lde + 2, -7.5)) if want_ferr else None
        be = vec(np.full(lay.batch * lde + 2, -7.5))
        work = vec(np.full(int(L.cap_dpoerr_vbatched_work_size(self.plan, nrhs)) + 4, np.nan)) if want_ferr else None
        st = L.cap_dpoerr_vbatched(self.plan, UPPER, nrhs, Ad.data_ptr(), Rd.data_ptr(), Bd.data_ptr(), ldb, Xd.data_ptr(), ldx, ptr(inf), ptr(fe),
                                   be.data_ptr(), lde, ptr(work), stream())
        torch.cuda.synchronize()
        assert st == OK, st
        for d, h in ((Ad, A0), (Rd, R0), (Bd, B0), (Xd, X0)):
            assert VC.same_bits(d.cpu().numpy(), h), "an input was written"
        if work is not None:
            assert np.isnan(work.cpu().numpy()[-4:]).all()
        res = []
        for t in (fe, be):
            if t is None:
                res.append(None)
                continue
            h = t.cpu().numpy()
            m = h[:lay.batch * lde].reshape(lay.batch, lde)
            assert (h[lay.batch * lde:] == -7.5).all() and (m[:, nrhs:] == -7.5).all()
            assert all((m[i] == -7.5).all() for i in range(lay.batch) if not lay.sizes[i]), "a row of an empty block was written"
            res.append(m[:, :nrhs].copy())
        return res[0], res[1]


def factor(As):
    """upper factors of SPD blocks by cap_dpotrf_batched_blocked (trsm_batched_gpu.factor)"""
    return G.factor(As)
