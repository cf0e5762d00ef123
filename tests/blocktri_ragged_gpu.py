"""TEST INFRASTRUCTURE of tests/test_gpu_blocktri_ragged.py: one row of tests/blocktri_ragged_cases.py on the device, as batched.VarChains
sees it - D and E two strided views of ONE shape (slots, n, n) of flat buffers, B the stacked right-hand sides - and the route the plan is
held to: ONE FIXED-SIZE CALL PER CHAIN (batched.blocktri_potrf / blocktri_potrs / blocktri_potri with batch = 1) on views of a CLONE.
Every buffer starts as a pattern of DISTINCT NaNs - what torch reads as the strictly upper triangles of D, the pad rows, the gaps between
slots, the slots no chain owns, every chain's unused slot of E, a guard behind every tensor - so comparing the WHOLE flat buffers bit for
bit checks the bit contract and that nothing else was written in one go: the fixed-size calls touch their own chain alone.

Conventions: tests/blocktri_cases.py.  In torch's reading D[s] holds D_i in its lower triangle, E[s] = Bc_i^T, B[k] is right-hand side k."""
import copy

import numpy as np
import torch

from tests import blocktri_ragged_cases as RC
from tests import vbatched_cases as V

DEV = "cuda:0"
GUARD = 16


def bits(t):
    return t.cpu().numpy().view(np.int64)


class Ragged:
    def __init__(self, row, family="exact", batch_order=None, fail=None):
        """batch_order: a permutation - chain k of this object is chain batch_order[k] of the row (same data, other company and places).
        fail: (chain, position) - that diagonal block gets a negative second (or only) diagonal entry"""
        from capital_amd import batched
        n, lengths, mode, nrhs, _ = row
        perm = list(range(len(lengths))) if batch_order is None else list(batch_order)
        self.source = perm
        lengths = tuple(lengths[c] for c in perm)
        self.row = (n, lengths) + tuple(row[2:])
        self.n, self.lengths, self.nrhs = n, lengths, nrhs
        self.first, self.rows_at, self.slots, self.eslots, self.rows = RC.geometry(self.row)
        ld, step, ldb = RC.layout(self.row)
        self.plan = batched.VarChains(lengths, RC.first_slots(lengths, mode))
        assert (self.plan.slots, self.plan.eslots, self.plan.rows) == (self.slots, self.eslots, self.rows)
        slots = max(self.slots, 1)
        self.shapes = {"D": ((slots, n, n), (step, ld, 1)), "E": ((slots, n, n), (step, ld, 1)), "B": ((nrhs, self.rows * n), (ldb, 1))}
        self.flat, self.exact = {}, []
        low = torch.tril(torch.ones(n, n, dtype=torch.bool))
        host = {}
        for salt, name in enumerate(("D", "E", "B")):
            shape, strides = self.shapes[name]
            size = sum((d - 1) * s for d, s in zip(shape, strides)) + 1 + GUARD if all(d > 0 for d in shape) else GUARD
            host[name] = torch.from_numpy(V.nan_pattern(size, salt=salt + 1))
        Dv, Ev, Bv = (host[k].as_strided(*self.shapes[k]) for k in ("D", "E", "B"))
        for k, c in enumerate(perm):
            T = lengths[k]
            if family == "exact":
                Dc, Bc, X, rhs, U, W, logdet = RC.exact_chain(row, c)
                self.exact.append((U, W, X, logdet))
            else:
                Dc, Bc, rhs = RC.random_chain(row, c)
            Dc = np.array(Dc, dtype=np.float64)
            if fail is not None and fail[0] == k:
                Dc[fail[1], min(1, n - 1), min(1, n - 1)] = -4.0
            for i in range(T):
                Dv[self.first[k] + i][low] = torch.from_numpy(Dc[i])[low]
                if i + 1 < T:
                    Ev[self.first[k] + i].copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(Bc[i], dtype=np.float64).T)))
            if T:
                Bv[:, self.rows_at[k] * n:(self.rows_at[k] + T) * n] = torch.from_numpy(np.ascontiguousarray(np.asarray(rhs, dtype=np.float64).T))
        self.flat = {k: v.to(DEV) for k, v in host.items()}
        self.rhs0 = self.flat["B"].clone()

    def view(self, name):
        return self.flat[name].as_strided(*self.shapes[name])

    def clone(self):
        c = copy.copy(self)
        c.flat = {k: v.clone() for k, v in self.flat.items()}
        return c

    def reset_rhs(self):
        self.flat["B"] = self.rhs0.clone()

    def same_as(self, other, names):
        for name in names:
            assert np.array_equal(bits(self.flat[name]), bits(other.flat[name])), "%s differs from the fixed-size route (or a word outside the chains was written)" % name

    # ------------------------------------------------------------------------------------------ the plan
    def factor(self):
        info, ld = self.plan.potrf(self.view("D"), self.view("E") if self.eslots else None, logdet=True)
        torch.cuda.synchronize()
        return info.cpu().numpy(), ld.cpu().numpy()

    def solve(self, info=None, half=None):
        self.plan.potrs(self.view("D"), self.view("E") if self.eslots else None, self.view("B"), info=info, half=half)
        torch.cuda.synchronize()

    def inverse(self, info=None, symmetric=False):
        self.plan.potri(self.view("D"), self.view("E") if self.eslots else None, info=info, symmetric=symmetric)
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------ one fixed-size call per chain
    def _chain_views(self, k):
        T, f, n = self.lengths[k], self.first[k], self.n
        D = self.view("D")[f:f + T].unsqueeze(0)
        E = self.view("E")[f:f + T - 1].unsqueeze(0) if T > 1 else None
        B = self.view("B")[:, self.rows_at[k] * n:(self.rows_at[k] + T) * n].unsqueeze(0)
        return D, E, B

    def fixed_factor(self):
        from capital_amd import batched
        info = np.zeros(len(self.lengths), dtype=np.int32)
        ld = np.zeros(len(self.lengths), dtype=np.float64)
        for k, T in enumerate(self.lengths):
            if T:
                D, E, _ = self._chain_views(k)
                i, l = batched.blocktri_potrf(D, E, logdet=True)
                info[k], ld[k] = int(i.cpu()[0]), float(l.cpu()[0])
        torch.cuda.synchronize()
        return info, ld

    def fixed_solve(self, info=None, half=None):
        from capital_amd import batched
        for k, T in enumerate(self.lengths):
            if T:
                D, E, B = self._chain_views(k)
                batched.blocktri_potrs(D, E, B, info=None if info is None else info[k:k + 1].contiguous(), half=half)
        torch.cuda.synchronize()

    def fixed_inverse(self, info=None, symmetric=False):
        from capital_amd import batched
        for k, T in enumerate(self.lengths):
            if T:
                D, E, _ = self._chain_views(k)
                batched.blocktri_potri(D, E, info=None if info is None else info[k:k + 1].contiguous(), symmetric=symmetric)
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------ a chain's own words, for company independence
    def chain_bits(self, k):
        """the bits of everything chain k owns: its D blocks (lower triangles in torch's reading), its E blocks, its right-hand sides"""
        T, f, n = self.lengths[k], self.first[k], self.n
        D = np.tril(self.view("D")[f:f + T].cpu().numpy())
        E = self.view("E")[f:f + max(T - 1, 0)].cpu().numpy()
        B = self.view("B")[:, self.rows_at[k] * n:(self.rows_at[k] + T) * n].cpu().numpy()
        return [np.ascontiguousarray(x).view(np.int64) for x in (D, E, B)]
