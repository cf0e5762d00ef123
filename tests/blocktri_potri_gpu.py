"""TEST INFRASTRUCTURE of tests/test_gpu_blocktri_potri.py: batched.blocktri_potri (cap_dpotri_blocktri_batched,
csrc/blocktri_potri_batched.hip) and the host-driven COMPOSITION of the fixed-size entries it replaces, on the NaN-guarded strided
buffers of tests/blocktri_gpu.py: what torch reads as the strictly upper triangles of D (unless the call fills them), the pad rows, the
gaps between blocks and chains and a guard behind every tensor start as NaN and must still be NaN after the call.

Conventions: tests/blocktri_potri_cases.py (mathematical, column-major reading).  In torch's reading D[c, i] holds U_i^T in its lower
triangle and afterwards Sigma_(i,i) there; E[c, i] holds W_i^T and afterwards C_i^T = Sigma[block i + 1, block i]."""
import numpy as np
import torch

from tests import blocktri_gpu as G

DEV = G.DEV
same = G.same


def sw(a):
    return np.swapaxes(a, -1, -2)


class Factors(G.Chains):
    """chains that hold a FACTOR: U (batch, T, n, n) upper and W (batch, T - 1, n, n) of a row (n, T, batch, fill, layout)"""

    def __init__(self, row, U, W, lay=None):
        n, T, batch, fill, name = row
        super().__init__((n, T, batch, 1, name), sw(np.array(U, dtype=np.float64)), np.array(W, dtype=np.float64), lay=lay)
        self.fill = bool(fill)
        if self.fill:                              # the call may write the whole D blocks
            torch.from_numpy(self.mask["D"]).as_strided(*self.shapes["D"]).fill_(True)

    def full(self, name):
        """the view on the host, untouched"""
        return self.view(name).cpu().numpy().copy() if name in self.flat else None

    def potri(self, info=None):
        from capital_amd import batched
        out = batched.blocktri_potri(self.view("D"), self.view("E"), info=info, symmetric=self.fill)
        torch.cuda.synchronize()
        assert out[0].data_ptr() == self.view("D").data_ptr() and (out[1] is None) == (self.T == 1)
        self.guards_intact(("D", "E"))
        return self

    def compose(self, info=None):
        """positions descending: trsm(trans=False) -> G; potri(symmetric=True) -> P; gemm(-1, 0) with the mirrored Sigma_(i+1,i+1) -> C;
        gemm(-1, 1) of C and G into P, of which torch's LOWER triangle (the upper one of the column-major block) counts.  Returns
        (Sd, Sc) in torch's reading on the host: Sd full blocks, the mirror of that triangle."""
        from capital_amd import batched
        D, E, T = self.view("D"), self.view("E"), self.T
        sig, Sd, Sc = None, [None] * T, [None] * max(T - 1, 0)
        for i in range(T - 1, -1, -1):
            if i + 1 < T:
                batched.trsm(D[:, i], E[:, i], trans=False, info=info)
            batched.potri(D[:, i], info=info, symmetric=True)
            if i + 1 < T:
                Gt = E[:, i].clone()               # gemm's overlap rule asks for a copy (.contiguous() returns a block of one element itself)
                batched.gemm(sig, Gt, C=E[:, i], alpha=-1.0, beta=0.0)
                batched.gemm(Gt, E[:, i], C=D[:, i], transa=True, alpha=-1.0, beta=1.0)
                Sc[i] = E[:, i].cpu().numpy().copy()
            low = torch.tril(D[:, i])
            sig = (low + torch.tril(D[:, i], -1).transpose(-1, -2)).contiguous()
            Sd[i] = sig.cpu().numpy().copy()
        torch.cuda.synchronize()
        return np.stack(Sd, axis=1), (np.stack(Sc, axis=1) if T > 1 else None)

    def result(self):
        """(Sd, Sc) in torch's reading as the call left them: Sd[c, i] the lower triangle (zeros above) or, with fill, the whole block"""
        Dh = self.full("D")
        return (Dh if self.fill else np.tril(Dh)), self.full("E")


def from_device_factor(row, seed=0):
    """a random chain of the row factored by blocktri_potrf on the device: (U, W, info) on the host, column-major reading"""
    from tests import blocktri_cases as BC
    n, T, batch, _, lay = row
    D, Bc, _ = BC.random_chain((n, T, batch, 1, lay), seed)
    c = G.Chains((n, T, batch, 1, "packed"), D, Bc)
    info, _ = c.factor()
    U = sw(c.host("D"))
    W = sw(c.host("E")) if T > 1 else np.zeros((batch, 0, n, n))
    return U, W, info
