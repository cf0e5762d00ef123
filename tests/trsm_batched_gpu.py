"""TEST INFRASTRUCTURE of tests/test_gpu_trsm_batched.py and tests/test_gpu_trsm_vbatched.py: the four C ABI entries (and cap_dpotrs_*,
cap_dpotrf_batched_blocked for comparison) on flat NaN buffers.  Every buffer of a call starts as NaN everywhere - the strictly lower
triangles, the pad rows, the gaps between blocks and columns, a guard behind the last element - and every call checks that what it must
not touch is still NaN (R: that no bit of the whole buffer changed)."""
import ctypes as C

import numpy as np
import torch

from tests import vbatched_cases as V

DEV = "cuda:0"
GUARD = 16
NOTRANS, TRANS, UPPER, OK = 0, 1, 1, 0
U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


def lib():
    from capital_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


class Flat:
    """`batch` column-major rows x cols windows, window i at i * stride with leading dimension ld, in a flat NaN buffer with a NaN guard
    behind the last one; tri: only the elements with row <= col are laid in (the rest of the window stays NaN)"""

    def __init__(self, mats, ld, stride, tri):
        rows, cols = mats[0].shape
        self.rows, self.cols, self.ld, self.stride, self.batch = rows, cols, ld, stride, len(mats)
        size = stride * (len(mats) - 1) + ld * cols + GUARD
        host = np.full(size, np.nan)
        r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        mask = (r <= c) if tri else (r >= 0)
        self.r, self.c = r[mask], c[mask]
        self.touched = np.zeros(size, dtype=bool)
        for i, M in enumerate(mats):
            host[self.index(i)] = np.asarray(M, dtype=np.float64)[self.r, self.c]
            self.touched[self.index(i)] = True
        self.host0 = host
        self.dev = torch.from_numpy(host.copy()).to(DEV)

    def index(self, i):
        return i * self.stride + self.r + self.c * self.ld

    def ptr(self):
        return self.dev.data_ptr()

    def all(self):
        host = self.dev.cpu().numpy()
        out = []
        for i in range(self.batch):
            m = np.zeros((self.rows, self.cols))
            m[self.r, self.c] = host[self.index(i)]
            out.append(m)
        return out, host

    def unchanged(self):
        return same(self.dev.cpu().numpy(), self.host0)


def shape_of(n, nrhs, layout):
    """(ldr, stride_r, ldb, stride_b) of a layout (ld - n, stride - ld cols)"""
    dl, ds = layout
    ldr, ldb = max(n + dl, 1), max(n + dl, 1)
    return ldr, ldr * n + ds, ldb, ldb * nrhs + ds


def run(entry, trans, Rs, Bs, layout=(0, 0), info=None, sumsq=False):
    """entry = 'trsm' | 'trmm' | 'potrs' on the batch (Rs upper triangles, Bs n x nrhs) -> (list of results, q (batch, nrhs) or None).
    Asserts CAP_OK, that R kept every bit, and that everything outside the n x nrhs windows of B and the batch x nrhs window of sumsq is
    still NaN."""
    L = lib()
    n, nrhs, batch = Rs[0].shape[0], Bs[0].shape[1], len(Rs)
    ldr, sr, ldb, sb = shape_of(n, nrhs, layout)
    Rf, Bf = Flat([np.triu(r) for r in Rs], ldr, sr, True), Flat(Bs, ldb, sb, False)
    inf = None if info is None else torch.tensor(info, dtype=torch.int32, device=DEV)
    ip = None if inf is None else inf.data_ptr()
    ldq = nrhs + layout[0]
    q = torch.full((batch * ldq + GUARD,), float("nan"), dtype=torch.float64, device=DEV) if sumsq else None
    if entry == "trsm":
        st = L.cap_dtrsm_batched(UPPER, trans, n, nrhs, Rf.ptr(), ldr, sr, Bf.ptr(), ldb, sb, batch, ip, q.data_ptr() if sumsq else None, ldq, stream())
    elif entry == "trmm":
        st = L.cap_dtrmm_batched(UPPER, trans, n, nrhs, Rf.ptr(), ldr, sr, Bf.ptr(), ldb, sb, batch, ip, stream())
    else:
        st = L.cap_dpotrs_batched_blocked(UPPER, n, nrhs, Rf.ptr(), ldr, sr, Bf.ptr(), ldb, sb, batch, ip, stream())
    torch.cuda.synchronize()
    assert st == OK, st
    assert Rf.unchanged(), "R was written"
    out, host = Bf.all()
    assert np.isnan(host[~Bf.touched]).all(), "B: an element outside the n x nrhs windows was written"
    if inf is not None:
        assert np.array_equal(inf.cpu().numpy(), np.asarray(info, dtype=np.int32))
    qh = None
    if sumsq:
        qa = q.cpu().numpy()
        qh = qa[:batch * ldq].reshape(batch, ldq)[:, :nrhs].copy()
        pad = np.ones(qa.shape, dtype=bool)
        for i in range(batch):
            pad[i * ldq:i * ldq + nrhs] = False
        assert np.isnan(qa[pad]).all(), "sumsq: a word outside the batch x nrhs window was written"
    return out, qh


def factor(As):
    """cap_dpotrf_batched_blocked on the SPD blocks -> list of upper factors (strictly lower triangles zero)"""
    L = lib()
    n = As[0].shape[0]
    Af = Flat([np.triu(a) for a in As], n, n * n, True)
    info = torch.full((len(As),), 7, dtype=torch.int32, device=DEV)
    assert L.cap_dpotrf_batched_blocked(UPPER, n, Af.ptr(), n, n * n, len(As), info.data_ptr(), None, stream()) == OK
    torch.cuda.synchronize()
    assert not info.cpu().numpy().any()
    return Af.all()[0]


def triangle(n, seed):
    """a well-conditioned random upper triangle with a positive diagonal (not rounded to anything: full 53-bit mantissas)"""
    rng = np.random.default_rng([911, n, seed])
    return np.triu(rng.standard_normal((n, n)) / np.sqrt(n), 1) + np.diag(1.0 + rng.random(n))


def arr64(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*[int(x) for x in a])


class Plan:
    """a cap_vbatch_plan on a vbatched_cases.Layout, with the stacked right-hand sides in a NaN buffer (ldb = rows + 2)"""

    def __init__(self, sizes, kind):
        self.lay = V.Layout(sizes, kind)
        self.plan = C.c_void_p()
        lay = self.lay
        assert lib().cap_vbatch_plan_create(lay.batch, arr64(lay.sizes), arr64(lay.ld_arg), arr64(lay.off_arg), C.byref(self.plan)) == OK

    def close(self):
        lib().cap_vbatch_plan_destroy(self.plan)

    def stacked(self, Bs, nrhs):
        """flat host buffer of the stacked B (distinct NaNs, then the blocks' rows), ldb"""
        lay = self.lay
        ldb = lay.rows + 2
        buf = V.nan_pattern(ldb * nrhs + 8, salt=5)
        for i, b in enumerate(Bs):
            if lay.sizes[i]:
                for k in range(nrhs):
                    at = k * ldb + int(lay.row_off[i])
                    buf[at:at + int(lay.sizes[i])] = b[:, k]
        return buf, ldb

    def run(self, entry, trans, Rs, Bs, nrhs, info=None, sumsq=False):
        """-> (list of per-block results (None for empty blocks), q (batch, nrhs) or None); asserts CAP_OK, R bit for bit unchanged, the pad
        rows of B and the sumsq words of empty blocks untouched"""
        L, lay = lib(), self.lay
        R0 = lay.buffer([None if r is None else np.triu(r) for r in Rs])
        B0, ldb = self.stacked(Bs, nrhs)
        Rd, Bd = torch.from_numpy(R0.copy()).to(DEV), torch.from_numpy(B0.copy()).to(DEV)
        inf = None if info is None else torch.tensor(info, dtype=torch.int32, device=DEV)
        ip = None if inf is None else inf.data_ptr()
        ldq = nrhs + 1
        q = torch.from_numpy(V.nan_pattern(lay.batch * ldq + GUARD, salt=9)).to(DEV) if sumsq else None
        if entry == "trsm":
            st = L.cap_dtrsm_vbatched(self.plan, UPPER, trans, nrhs, Rd.data_ptr(), Bd.data_ptr(), ldb, ip, q.data_ptr() if sumsq else None, ldq, stream())
        elif entry == "trmm":
            st = L.cap_dtrmm_vbatched(self.plan, UPPER, trans, nrhs, Rd.data_ptr(), Bd.data_ptr(), ldb, ip, stream())
        else:
            st = L.cap_dpotrs_vbatched(self.plan, UPPER, nrhs, Rd.data_ptr(), Bd.data_ptr(), ldb, ip, stream())
        torch.cuda.synchronize()
        assert st == OK, st
        assert V.same_bits(Rd.cpu().numpy(), R0), "R was written"
        Bh = Bd.cpu().numpy()
        keep = np.ones(Bh.shape, dtype=bool)
        out = []
        for i in range(lay.batch):
            k = int(lay.sizes[i])
            if not k:
                out.append(None)
                continue
            cols = [Bh[c * ldb + int(lay.row_off[i]):c * ldb + int(lay.row_off[i]) + k] for c in range(nrhs)]
            out.append(np.stack(cols, axis=1))
        for c in range(nrhs):
            keep[c * ldb:c * ldb + lay.rows] = False
        assert np.array_equal(Bh.view(np.int64)[keep], B0.view(np.int64)[keep]), "B: a pad element was written"
        qh = None
        if sumsq:
            qa, q0 = q.cpu().numpy(), V.nan_pattern(lay.batch * ldq + GUARD, salt=9)
            qh = qa[:lay.batch * ldq].reshape(lay.batch, ldq)[:, :nrhs].copy()
            keep = np.ones(qa.shape, dtype=bool)
            for i in range(lay.batch):
                if lay.sizes[i]:
                    keep[i * ldq:i * ldq + nrhs] = False
            assert np.array_equal(qa.view(np.int64)[keep], q0.view(np.int64)[keep]), "sumsq: a word of an empty block or of the padding was written"
        return out, qh
