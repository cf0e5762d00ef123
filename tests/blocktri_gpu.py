"""TEST INFRASTRUCTURE of tests/test_gpu_blocktri_batched.py: batched.blocktri_potrf / blocktri_potrs (cap_dpotrf_blocktri_batched,
cap_dpotrs_blocktri_batched, csrc/blocktri_batched.hip) and the host-driven COMPOSITION of the existing entries they replace, both on
strided views of flat NaN buffers.  Every buffer starts as NaN everywhere - what torch reads as the strictly upper triangles of D, the pad
rows, the gaps between blocks and chains, a guard behind every tensor - and after every call whatever the call must not touch is
asserted to be NaN still; the solve is asserted to leave every bit of D and E alone.

Conventions: tests/blocktri_cases.py (mathematical, column-major reading: D_i symmetric, Bc_i = A[i, i + 1]).  In torch's reading
D[c, i] holds D_i in its lower triangle, E[c, i] = Bc_i^T = A[i + 1, i], B[c, k] is right-hand side k of chain c."""
import numpy as np
import torch

from tests import blocktri_cases as BC

DEV = "cuda:0"
GUARD = 16


def same(a, b):
    """bit for bit, NaN equal to NaN by position"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def _flat(shape, strides):
    """a flat NaN host tensor that holds `shape` under `strides` plus a guard, its strided view and the mask of the view's elements"""
    size = sum((d - 1) * s for d, s in zip(shape, strides)) + 1 + GUARD if all(d > 0 for d in shape) else GUARD
    flat = torch.full((size,), float("nan"), dtype=torch.float64)
    mask = torch.zeros(size, dtype=torch.bool)
    return flat, mask


class Chains:
    """one batch of chains of a row of the table in its layout, on the device"""

    def __init__(self, row, D, Bc, rhs=None, lay=None):
        self.row = row
        n, T, batch, nrhs, _ = row
        if rhs is not None:
            nrhs = rhs.shape[2]
        ldd, step_d, stride_d, lde, step_e, stride_e, ldb, stride_b = lay if lay is not None else BC.layout((n, T, batch, nrhs, row[4]))
        self.n, self.T, self.batch, self.nrhs = n, T, batch, nrhs
        self.shapes = {"D": ((batch, T, n, n), (stride_d, step_d, ldd, 1)), "E": ((batch, T - 1, n, n), (stride_e, step_e, lde, 1)),
                       "B": ((batch, nrhs, T * n), (stride_b, ldb, 1))}
        self.flat, self.mask = {}, {}
        low = torch.tril(torch.ones(n, n, dtype=torch.bool))
        for name, src in (("D", torch.from_numpy(np.ascontiguousarray(D, dtype=np.float64))),
                          ("E", torch.from_numpy(np.ascontiguousarray(np.swapaxes(Bc, -1, -2), dtype=np.float64))),
                          ("B", None if rhs is None else torch.from_numpy(np.ascontiguousarray(np.swapaxes(rhs, -1, -2), dtype=np.float64)))):
            shape, strides = self.shapes[name]
            if src is None or (name == "E" and T == 1):
                continue
            flat, mask = _flat(shape, strides)
            fv, mv = flat.as_strided(shape, strides), mask.as_strided(shape, strides)
            if name == "D":
                fv[..., low] = src[..., low]
                mv[..., low] = True
            else:
                fv.copy_(src)
                mv.fill_(True)
            self.flat[name], self.mask[name] = flat.to(DEV), mask.numpy()
        self.host0 = {k: v.cpu().numpy() for k, v in self.flat.items()}

    def view(self, name):
        if name not in self.flat:
            return None
        return self.flat[name].as_strided(*self.shapes[name])

    def clone(self):
        import copy
        c = copy.copy(self)
        c.flat = {k: v.clone() for k, v in self.flat.items()}
        return c

    def host(self, name):
        """the view on the host; D with what torch reads as the strictly upper triangle set to zero"""
        if name not in self.flat:
            return None
        v = self.view(name).cpu().numpy().copy()
        return np.tril(v) if name == "D" else v

    def guards_intact(self, names):
        for name in names:
            if name in self.flat:
                h = self.flat[name].cpu().numpy()
                assert np.isnan(h[~self.mask[name]]).all(), "%s: a word outside the blocks was written" % name

    def unchanged_since(self, before, names):
        for name in names:
            if name in self.flat:
                assert np.array_equal(self.flat[name].cpu().numpy().view(np.int64), before[name].view(np.int64)), "%s was written" % name

    def snapshot(self):
        return {k: v.cpu().numpy() for k, v in self.flat.items()}

    # ------------------------------------------------------------------------------------------ the new entries
    def factor(self):
        from capital_amd import batched
        info, ld = batched.blocktri_potrf(self.view("D"), self.view("E"), logdet=True)
        torch.cuda.synchronize()
        self.guards_intact(("D", "E"))
        return info, ld

    def solve(self, info=None, half=None):
        from capital_amd import batched
        before = self.snapshot()
        out = batched.blocktri_potrs(self.view("D"), self.view("E"), self.view("B"), info=info, half=half)
        torch.cuda.synchronize()
        assert out.data_ptr() == self.view("B").data_ptr()
        self.guards_intact(("B",))
        self.unchanged_since(before, ("D", "E"))

    # ------------------------------------------------------------------------------------------ the route they replace
    def compose_factor(self):
        """for i: info_i, ld_i = potrf(D[:, i]); schur(D[:, i], E[:, i], D[:, i + 1], info_i) -> (info, logdet) of the chains"""
        from capital_amd import batched
        D, E = self.view("D"), self.view("E")
        info = torch.zeros(self.batch, dtype=torch.int32, device=DEV)
        ld = torch.zeros(self.batch, dtype=torch.float64, device=DEV)
        for i in range(self.T):
            info_i, ld_i = batched.potrf(D[:, i], logdet=True)
            info = torch.where((info == 0) & (info_i != 0), info_i + i * self.n, info)
            ld += ld_i
            if i + 1 < self.T:
                batched.schur(D[:, i], E[:, i], D[:, i + 1], info_i)
        torch.cuda.synchronize()
        self.guards_intact(("D", "E"))
        return info, ld

    def compose_solve(self, info=None, half=None):
        """forward: trsm(trans) on segment i, gemm into segment i + 1; backward: gemm into segment i, trsm(notrans) - on a copy of the
        input segment, which gemm's overlap rule asks for (a copy changes no bit)"""
        from capital_amd import batched
        D, E, B, n = self.view("D"), self.view("E"), self.view("B"), self.n
        seg = lambda i: B[:, :, i * n:(i + 1) * n]
        if half in (None, "forward"):
            for i in range(self.T):
                batched.trsm(D[:, i], seg(i), trans=True, info=info)
                if i + 1 < self.T:
                    batched.gemm(seg(i).contiguous(), E[:, i], C=seg(i + 1), transb=True, alpha=-1.0, beta=1.0)
        if half in (None, "backward"):
            for i in range(self.T - 1, -1, -1):
                if i + 1 < self.T:
                    batched.gemm(seg(i + 1).contiguous(), E[:, i], C=seg(i), alpha=-1.0, beta=1.0)
                batched.trsm(D[:, i], seg(i), trans=False, info=info)
        torch.cuda.synchronize()
        self.guards_intact(("B",))
