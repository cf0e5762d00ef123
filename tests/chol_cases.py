"""One case table for the fp64 Cholesky factorization - cap_cholinv_factor (complete_inv = -1 / 0 / 1: the blocked right-looking sweep,
its strip buffers, paired far update, fused first-step copy, column-split look-ahead, the one-launch and the stepwise diagonal-block chain,
the inverse tree, the plain recursion) and cap_dpotrf (the same sweep in place on caller memory) - shared by tests/test_chol_cases.py (no
GPU: every row through the library's own object files on the recording stand-in) and tests/test_gpu_chol_exact.py (-m gpu: the same rows
on the device, bit for bit).  NumPy only, nothing of torch or the GPU is imported here.

EXACT RESULTS.  R = diag(d) (I + N) is the F1 "three classes" family of tests/tri_cases.py with a positive diagonal (d_i from {1/2, 1, 2,
4}, N from {+-1, +-2}, N^3 = 0) and A = R^T R.  The pivots of A are d_i^2, from {1/4, 1, 4, 16}: leaf.hip takes 1 / sqrt(pivot) from
v_rsq_f64 and two Newton steps, which the device returns exactly for these four values (the probe of tests/test_gpu_chol_exact.py
measures that and stays in the suite; on an MI355X all four are exact, so the diagonal is not restricted).  Everything else the
factorization does only multiplies and adds: the sweep, the explicit inverses of the diagonal blocks, the block-row products
Dinv^T A_row, the Schur updates in any order and pairing and the inverse tree form dyadic rationals far below 2^53, so R and
R^-1 = (I - N + N^2) diag(d)^-1 must come out bit for bit, whatever the schedule.

THE PREMISE IS ASSERTED, NOT ASSUMED (bounds()).  With S = 2 |R|^T |R| (the stored A plus everything any Schur update can have taken
from it or still has to), all of these must be < 2^53:
  * every partial sum of a Schur update, in any order or pairing: S_ij, 2 fraction bits;
  * every partial sum of a block-row solve Dinv^T A_row: with the comparison inverse M^-1 = (I + |N| + |N|^2) |D|^-1 >= |R^-1| of the
    panel's diagonal block, (M^-T S)_ij on the panel's rows, 5 fraction bits - for every panel width the row uses (the 64-wide steps
    inside a diagonal block, the leaf size of the recursion, the panel width nb and the halves of the recursion are all diagonal
    blocks of the same triangular M, whose inverse restricted to a diagonal block is that block's inverse);
  * the inverse tree, the in-block merges and the leaf's inverse: |R^-1| |R| |R^-1|, 5 fraction bits, as in tests/tri_cases.py.
A row that fails is a bad row, not a reason to loosen anything.

REFERENCES.  R itself; R^-1 from the closed form (tri_cases.family asserts R Rinv == I == Rinv R elementwise); for complete_inv = 0 the
root block Rinv[:n >> split, n >> split:] is exactly zero unless the root is itself a base case (root_is_base, the rule of cholinv.hpp:93
that tests/test_gpu_cholinv.py checks against the oracle's pattern; tests/test_chol_cases.py does the same for this table).  At n <= 40
tests/test_chol_cases.py recomputes factor and inverse from the stored A with fractions.Fraction.

A row names what it must launch: `kernels`, the number of launches per kernel of the factor's own family (leaf_cholinv_kernel,
panel64_solve_update_kernel, chain64_coop_kernel, trinv_merge_kernel<RBW>), `gemms`, the number of dgemm_* launches, `cin`, how many of
them read their C input from A (the fused first-step copy), `k2`, how many are paired far updates (K = 2 NB), and `why`.

The option sets and shapes of the sweep rows are those of tests/test_gpu_cholinv.py, not its rows verbatim: every plan here has
bc_mult_dim = -2 (the existing inverse-tree test uses -3 at n = 3072 and 4096; nb is set explicitly there, so the schedule is the same),
complete_inv / split cycle over the knob sets, and lda alternates between n, n + 2 and n + 3.

cap_dpotrf: its `outer` = 2 nb, `tail` and `depth2` defaults start at n >= 8192 and n >= 24576, out of reach at test shapes; the plan
rows run the same code (right_looking) with those knobs through cap_cholinv_set_option."""
import collections
import functools

import numpy as np

from tests import tri_cases as TC
from tests.tri_cases import NAN, LIMIT, positive_zero, stored   # noqa: F401  (re-exported for the two test files)

LEAF = "leaf_cholinv_kernel"
PANEL = "panel64_solve_update_kernel"
CHAIN = "chain64_coop_kernel"
FAMILY = (LEAF, PANEL, CHAIN, "trinv_merge_kernel")
LEAF_MAX = 64
BC = -2                 # bc_mult_dim of every plan row (the knob tests/test_gpu_cholinv.py uses): the root is partitioned from n = 2 on
PROBE_PIVOTS = (0.25, 1.0, 4.0, 16.0)          # d^2 for d in tri_cases.DIAG
# every key of cap_cholinv_set_option that changes the schedule of a single-GPU factor call
SCHEDULE_KEYS = ("nb", "leaf", "lookahead", "outer", "tail", "depth2", "pair_rest", "inner_la", "occ1_m", "fastdiag", "use_sb", "inv_fast",
                 "inv_overlap", "inv_start_m", "reserve", "reserve_m", "fuse_copy", "chain_coop", "serial_m")


def MERGE(rbw):
    return "trinv_merge_kernel<%d>" % rbw


class Case(TC.Case):
    """a row: entry (plan / dpotrf), n, ci (complete_inv), split, opts (the cap_cholinv_set_option calls, in order), pad (lda - n), second
    (factor a second exact matrix on the same plan and compare that one), pivot (None, or the 0-based pivot made exactly -1), kernels,
    gemms, cin, k2, why"""

    @property
    def id(self):
        s = "%s-n%d" % (self.entry, self.n)
        if self.entry == "plan":
            s += "-ci%d-s%d" % (self.ci, self.split)
        s += "".join("-%s%d" % (k, v) for k, v in self.opts)
        s += "-pad%d" % self.pad
        if self.second:
            s += "-second"
        if self.pivot is not None:
            s += "-pivot%d" % self.pivot
        return s

    @property
    def opt(self):
        return dict(self.opts)


# ------------------------------------------------------------------------------------------------- what the host side is expected to do
def default_nb(n, bc=BC):
    nb = 512 if n >= 8192 else 256
    if bc < 0:
        b = 1
        for _ in range(-bc):
            if b < n:
                b *= 2
        b = max(1, min(n, b))
        hint = ((n // b) // 128) * 128
        nb = min(nb, hint) if hint >= 128 else min(nb, 128)
    return nb


def root_is_base(n, split, bc=BC):
    """the root is itself a base case (cholinv.hpp:93): complete_inv = 0 then gives the full inverse"""
    b = 1
    if bc < 0:
        for _ in range(-bc):
            if b < n:
                b *= 2
    else:
        for _ in range(bc):
            b //= 2
    b = max(1, min(n, b))
    return n <= n // b or (n >> split) < split


def knobs(c):
    """the schedule parameters a row ends up with: the defaults of its entry, then its options"""
    n = c.n
    if c.entry == "dpotrf":
        nb = min(default_nb(n, 0), (max(n, 1) + 63) // 64 * 64)
        return dict(nb=nb, leaf=LEAF_MAX, lookahead=int(n >= 4096), outer=2 * nb if n >= 8192 else nb, tail=n // 8 if n >= 8192 else 0, depth2=int(n >= 24576),
                    pair_rest=1, inner_la=0, occ1_m=16384, fastdiag=1, use_sb=0, inv_fast=1, inv_overlap=1, inv_start_m=max(16384, n // 2), reserve=0,
                    reserve_m=0, fuse_copy=0, chain_coop=32, serial_m=0)
    nb = default_nb(n)
    k = dict(nb=nb, leaf=LEAF_MAX, lookahead=1, outer=2 * nb if n >= 8192 else nb, tail=n // 8 if n >= 8192 else 0, depth2=int(n >= 24576), pair_rest=1,
             inner_la=0, occ1_m=16384, fastdiag=1, use_sb=1, inv_fast=1, inv_overlap=1, inv_start_m=max(16384, n // 2), reserve=0, reserve_m=0, fuse_copy=1,
             chain_coop=32, serial_m=0)
    k.update(c.opt)
    return k


def pick_split(n, leaf):
    return TC.pick_split(n, leaf)


def _rec(n, leaf, k, g, root_n1=0, root_skip=False):
    """rec_cholinv on an n x n block: leaves and products (4 per partition; 2 at a root whose inverse block stays empty)"""
    if n <= leaf and not root_n1:
        k[LEAF] += 1
        return g
    n1 = root_n1 if 0 < root_n1 < n else pick_split(n, leaf)
    g = _rec(n1, leaf, k, g)
    g = _rec(n - n1, leaf, k, g)
    return g + (2 if root_skip else 4)


def _diag_block(jb, kn, k, g):
    """panel_chain on a jb-wide diagonal block"""
    if kn["fastdiag"] and jb % 64 == 0 and 128 <= jb <= 1024 and jb & (jb - 1) == 0 and kn["leaf"] == LEAF_MAX:
        nblk, merged = jb // 64, 0
        if kn["chain_coop"] >= 2 and nblk >= 4:
            k[CHAIN] += 2                                  # the launch and its recovery launch (two workgroups that return at once)
            merged = min(256, jb // 2)
        else:
            k[LEAF] += 1
            k[PANEL] += nblk - 1
        h = 64
        while h < jb:
            if h > merged:
                if h <= 256:
                    k[MERGE(h // 64)] += 1
                else:
                    g += 2 * (jb // (2 * h))
            h *= 2
        return g
    return _rec(jb, kn["leaf"], k, g)


def strip_bounds(n, kn):
    nb = kn["nb"]
    NB = max(nb, kn["outer"] // nb * nb)
    bnd = [0]
    while bnd[-1] < n:
        bnd.append(min(n, bnd[-1] + (NB if n - bnd[-1] > kn["tail"] else nb)))
    return bnd, NB


def _strip(J0, rows, n, kn, k, g):
    """factor_strip: per nb-wide panel the diagonal block, the block-row solve and the update of the strip's own rows"""
    nb, Jend = kn["nb"], J0 + rows
    for j0 in range(J0, Jend, nb):
        jb = min(nb, Jend - j0)
        g = _diag_block(jb, kn, k, g)
        j1 = j0 + jb
        g += int(n - j1 > 0) + int(Jend - j1 > 0 and n - j1 > 0)
    return g


def expected_launches(c):
    """-> (Counter of the family's launches, dgemm launches, of them with Cin, of them paired) of a row's FIRST factor call"""
    kn, n = knobs(c), c.n
    k, g, cin, k2 = collections.Counter(), 0, 0, 0
    nb = kn["nb"]
    inverse = False
    if c.entry == "plan" and c.ci >= 0:
        base = root_is_base(n, c.split)
        if kn["inv_fast"] and n >= 2 * nb and kn["leaf"] == LEAF_MAX:
            inverse = True
        else:
            n1 = 0 if base else n >> c.split
            return k, _rec(n, kn["leaf"], k, 0, root_n1=n1, root_skip=(not base and c.ci == 0 and 0 < n1 < n)), 0, 0
    bnd, NB = strip_bounds(n, kn)
    nstrip = len(bnd) - 1
    la = bool(kn["lookahead"]) and nstrip > 2
    split_path = bool(kn["inner_la"]) and kn["serial_m"] == 0 and kn["reserve"] == 0 and NB // nb <= 8 and not inverse
    lda = n + c.pad
    fuse = (c.entry == "plan" and la and not split_path and bool(kn["fuse_copy"]) and n % 128 == 0 and nb % 128 == 0 and lda % 2 == 0
            and n - bnd[1] > kn["serial_m"])
    if not la:
        for s in range(nstrip):
            g = _strip(bnd[s], bnd[s + 1] - bnd[s], n, kn, k, g)
            g += int(n - bnd[s + 1] > 0)
    elif split_path:
        B = lambda i: bnd[min(i, nstrip)]                   # noqa: E731
        upd = lambda r0, r1, c0, c1: int(r1 > r0 and c1 > c0)   # noqa: E731
        g = _strip(0, bnd[1], n, kn, k, g)
        for s in range(nstrip - 1):
            J1, J2, Jc, Jn = bnd[s + 1], bnd[s + 2], B(s + 3), B(s + 4)
            g += upd(J1, J2, J1, Jc)
            for j0 in range(J1, J2, nb):
                jb = min(nb, J2 - j0)
                j1 = j0 + jb
                g = _diag_block(jb, kn, k, g)
                g += int(Jc - j1 > 0) + upd(j1, J2, j1, Jc)
            if Jc < n:
                g += upd(J1, J2, Jc, Jn) + upd(J1, J2, Jn, n)
                for j0 in range(J1, J2, nb):
                    j1 = j0 + min(nb, J2 - j0)
                    g += int(Jn - Jc > 0) + int(n - Jn > 0)
                    if j1 < J2:
                        g += upd(j1, J2, Jc, Jn) + upd(j1, J2, Jn, n)
            m2 = n - J2
            if m2 > 0:
                rows2 = bnd[s + 3] - bnd[s + 2] if s + 3 <= nstrip else m2
                g += 2 if kn["depth2"] and rows2 < m2 else 1
    else:
        tail_res = kn["reserve"] > 0 and kn["reserve_m"] > 0
        ksw = nstrip
        for s in range(1, nstrip):
            if n - bnd[s + 1] <= kn["serial_m"]:
                ksw = s
                break
        g = _strip(0, bnd[1], n, kn, k, g)
        deferred = deferred_cin = False
        for s in range(nstrip):
            rows, m = bnd[s + 1] - bnd[s], n - bnd[s + 1]
            if m <= 0:
                break
            if s >= ksw:
                for q in range(s, nstrip):
                    if q > s:
                        g = _strip(bnd[q], bnd[q + 1] - bnd[q], n, kn, k, g)
                    g += int(n - bnd[q + 1] > 0)
                break
            fz = int(fuse and s == 0)                        # step 0 of the fused form: every update of the step reads its C input from A
            rows1 = bnd[s + 2] - bnd[s + 1]
            g, cin = g + 1, cin + fz                         # the update of strip s + 1's rows
            g = _strip(bnd[s + 1], rows1, n, kn, k, g)
            m2 = m - rows1
            if m2 <= 0:
                continue
            rows2 = bnd[s + 3] - bnd[s + 2] if s + 3 <= nstrip else m2
            if not (kn["depth2"] and rows2 < m2):
                g, cin = g + 1, cin + fz                     # the whole rest in one update
                continue
            g, cin = g + 1, cin + fz                         # head: strip s + 2's rows
            if deferred:                                     # the paired far update: its C input is A's if the deferring step was step 0
                g, cin, k2, deferred = g + 1, cin + deferred_cin, k2 + 1, False
            else:
                g, cin = g + 1, cin + fz                     # a second head (strip s + 3's rows, the rest deferred) or the rest
                if kn["pair_rest"] and s % 2 == 0 and s + 4 < nstrip and s + 1 < ksw and rows == NB and rows1 == NB and not tail_res:
                    deferred, deferred_cin = True, fz
    if inverse:                                              # one node per partition of the panels, two products each; an empty root block has none
        np_ = -(-n // nb)
        n1 = n >> c.split
        skip = not root_is_base(n, c.split) and 0 < n1 < n and n1 % nb == 0 and c.ci == 0
        g += 2 * (np_ - 1 - int(skip))
    return k, g, cin, k2


# ----------------------------------------------------------------------------------------------------------------------------- the rows
KNOB_N = 1536
KNOB_SETS = [{"lookahead": 0}, {"lookahead": 1, "nb": 128}, {"nb": 256}, {"nb": 512, "leaf": 32}, {"leaf": 16},
             {"nb": 128, "outer": 512, "tail": 256}, {"nb": 128, "outer": 256, "depth2": 1},
             {"nb": 128, "outer": 256, "tail": 512, "depth2": 1}, {"nb": 256, "reserve": 8}, {"nb": 512, "fastdiag": 1}, {"nb": 256, "fastdiag": 1, "lookahead": 0},
             {"nb": 128, "fastdiag": 1, "outer": 256},
             {"nb": 128, "outer": 256, "inner_la": 1}, {"nb": 128, "outer": 512, "tail": 512, "depth2": 1, "inner_la": 1},
             {"nb": 256, "outer": 256, "inner_la": 1}, {"nb": 128, "outer": 1024, "inner_la": 1},
             {"nb": 128, "outer": 256, "occ1_m": 0}, {"nb": 128, "outer": 256, "occ1_m": 1024},
             {"nb": 128, "outer": 256, "occ1_m": 4096, "inner_la": 1},
             {"nb": 128, "outer": 256, "use_sb": 0}, {"nb": 128, "outer": 512, "tail": 512, "depth2": 1, "use_sb": 0},
             {"nb": 128, "outer": 128, "use_sb": 1}, {"nb": 256, "outer": 512, "tail": 0, "use_sb": 1},
             {"nb": 128, "outer": 256, "fuse_copy": 0}, {"nb": 128, "outer": 256, "depth2": 1, "fuse_copy": 1},
             {"nb": 256, "outer": 256, "use_sb": 0, "fuse_copy": 1},
             {"nb": 128, "outer": 256, "reserve": 8, "reserve_m": 768}]          # tests/test_gpu_cholinv.py::test_schedule_knobs_do_not_change_the_answer
PAIRED = [(2048, -1, {"nb": 128, "outer": 256, "depth2": 1}, "8 strips: pairs (0,1) (2,3); the last steps run unpaired"),
          (2304, -1, {"nb": 128, "outer": 256, "depth2": 1}, "9 strips"),
          (1280, -1, {"nb": 128, "outer": 256, "depth2": 1}, "5 strips: exactly one pair"),
          (1024, -1, {"nb": 128, "outer": 256, "depth2": 1}, "4 strips: no step may defer (no strip k + 4)"),
          (3072, -1, {"nb": 128, "outer": 512, "tail": 1024, "depth2": 1}, "nb-wide strips in the tail: pairing stops there"),
          (2048, -1, {"nb": 128, "outer": 256, "depth2": 1, "use_sb": 0}, "operands inside R: the pair is two adjacent row blocks"),
          (2048, -1, {"nb": 128, "outer": 256, "depth2": 1, "fuse_copy": 0}, "pairs without the fused copy"),
          (2560, 1, {"nb": 128, "outer": 256, "depth2": 1}, "the inverse tree rides on the paired sweep"),
          (2176, -1, {"nb": 128, "outer": 256, "depth2": 1}, "ragged last strip")]      # ...::test_paired_far_update_against_the_unpaired_schedule
TREE = [(2048, 0, 2, {}, "root partition n >> 2 = 512 on a panel boundary: unbalanced tree, root node skipped"),
        (2048, 1, 2, {}, "the same tree with its root"),
        (1536, 1, 1, {"nb": 256}, "6 panels: non-power-of-two tree"),
        (1792, 0, 1, {"nb": 256}, "7 panels, root partition 896 inside a panel: full tree, root block emptied afterwards"),
        (1100, 1, 1, {"nb": 128}, "ragged last panel (76 columns)"),
        (1100, 0, 1, {"nb": 256}, "ragged last panel, root partition inside a panel"),
        (2048, 1, 1, {"nb": 128, "outer": 256, "tail": 512, "depth2": 1}, "tree behind two-level blocking"),
        (4096, 0, 1, {"nb": 512}, "8 panels of 512"),
        (1536, 1, 1, {"nb": 256, "lookahead": 0}, "tree behind the sweep without look-ahead"),
        (3072, 1, 1, {"nb": 256, "inv_overlap": 0}, "tree after the join"),
        (3072, 1, 1, {"nb": 256, "inv_start_m": 0}, "overlapped mode that never starts early = flush at the end"),
        (3072, 0, 1, {"nb": 256, "inv_start_m": 1 << 30}, "tree enqueued from the first panel on"),
        (3072, 1, 1, {"nb": 256, "use_sb": 0}, "without strip buffers: the tree's events come from the panel stream"),
        (1100, 0, 1, {"nb": 128, "use_sb": 0}, "ragged, without strip buffers"),
        (3072, 1, 1, {"nb": 256, "inv_fast": 0}, "the plain recursion on the whole matrix"),
        (1100, 0, 1, {"nb": 128, "inv_fast": 0}, "the plain recursion, ragged, empty root block")]   # ...::test_inverse_tree_on_blocked_factorization
COOP_G = (0, 2, 3, 7, 32, 200)
PIVOT_N, PIVOT_NB = 512, 256


def _row(entry, n, why, ci=-1, split=1, opts=(), pad=0, second=False, pivot=None):
    opts = tuple(opts.items()) if isinstance(opts, dict) else tuple(opts)
    c = Case(entry=entry, n=n, ci=ci, split=split, opts=opts, pad=pad, second=second, pivot=pivot, why=why, kernels=None, gemms=0, cin=0, k2=0)
    k, g, cin, k2 = expected_launches(c)
    c.update(kernels=dict(sorted(k.items())), gemms=g, cin=cin, k2=k2)
    return c


def _leaf_rows():
    rows = []
    for i, n in enumerate((1, 2, 15, 16, 17, 33, 64)):
        why = "one leaf, padded to %d" % TC.leaf_padding(n)
        rows.append(_row("plan", n, why + "; R only", ci=-1, pad=(0, 2, 3)[i % 3]))
        rows.append(_row("plan", n, why + ("; root partition %d + %d, padded to %s" % (n >> 1, n - (n >> 1), "/".join(
            str(p) for p in sorted({TC.leaf_padding(n >> 1), TC.leaf_padding(n - (n >> 1))}))) if n > 1 else "; the root is a base case"), ci=1, pad=(2, 3, 0)[i % 3]))
        rows.append(_row("dpotrf", n, why, pad=(3, 0, 2)[i % 3]))
    rows.append(_row("plan", 64, "leaf = 16: recursion down to 16-wide leaves", ci=-1, opts={"leaf": 16}))
    rows.append(_row("plan", 64, "leaf = 32, empty root block", ci=0, opts={"leaf": 32}))
    rows.append(_row("plan", 33, "leaf = 16: leaves of 16 and 17 -> 16 + 1", ci=1, opts={"leaf": 16}, pad=3))
    return rows


def _block_rows():
    """one diagonal block (complete_inv = -1, n = nb: R alone is visible) and two of them under one tree node (complete_inv = 1, n = 2 nb: the
    diagonal blocks of R^-1 are the chain's own inverses, written in place)"""
    rows = []
    for nb in (128, 256, 512, 1024):
        for ci, n in ((-1, nb), (1, 2 * nb)):
            if n > 1024 and ci == 1 and nb == 1024:
                n = 2048
            rows.append(_row("plan", n, "fastdiag off: rec_cholinv + leaf_cholinv_kernel on the %d-wide block" % nb, ci=ci, opts={"nb": nb, "fastdiag": 0}))
            for G in COOP_G:
                nblk = nb // 64
                chain = G >= 2 and nblk >= 4
                why = ("one-launch chain of %d blocks, G = %d" % (nblk, G)) if chain else "stepwise folded chain of %d blocks (G = %d)" % (nblk, G)
                if ci == 1 and not (nb in (256, 1024) or G in (0, 32)):
                    continue                              # (the R + R^-1 form at every width for the two chains, at every G for two widths)
                rows.append(_row("plan", n, why, ci=ci, opts={"nb": nb, "fastdiag": 1, "chain_coop": G}))
    for n in (65, 100, 130, 200, 300):
        rows.append(_row("plan", n, "ragged or non-power-of-two block: rec_cholinv + leaves", ci=-1, opts={"nb": (n + 63) // 64 * 64}, pad=(0, 3)[n % 2]))
        rows.append(_row("plan", n, "the plain recursion with the root partition %d + %d" % (n >> 1, n - (n >> 1)), ci=1, pad=(2, 0)[n % 2]))
    return rows


def _sweep_rows():
    rows = []
    for i, o in enumerate(KNOB_SETS):
        ci, split = (-1, 0, 1)[i % 3], 1 + (i // 3) % 2
        rows.append(_row("plan", KNOB_N, "schedule knobs", ci=ci, split=split, opts=o, pad=(0, 2)[i % 2]))
    for n, ci, o, why in PAIRED:                                 # (lda = n + 2 = ldr + 2: the fused copy's C input has a pitch of its own)
        for pr in (0, 1):
            rows.append(_row("plan", n, why, ci=ci, opts=dict(o, pair_rest=pr), pad=2 * pr))
    for i, (n, ci, split, o, why) in enumerate(TREE):            # (an odd lda turns the fused copy off: expected_launches follows)
        rows.append(_row("plan", n, why, ci=ci, split=split, opts=o, pad=(0, 2, 0, 3)[i % 4]))
    for fc in (0, 1):
        for sb in (0, 1):
            rows.append(_row("plan", 1024, "fused first-step copy %s, strip buffers %s" % (("off", "on")[fc], ("off", "on")[sb]), ci=(1, -1)[fc ^ sb],
                             opts={"nb": 128, "outer": 128, "fuse_copy": fc, "use_sb": sb}, pad=2))
    rows.append(_row("plan", 1536, "serial tail: from 512 columns left on nothing is overlapped", ci=-1, opts={"nb": 128, "outer": 256, "serial_m": 512}))
    seen = set()                                              # (an option set of one list may be a row of another)
    return [c for c in rows if not (c.id in seen or seen.add(c.id))]


def _dpotrf_rows():
    rows = []
    for n in (1, 64, 65, 129, 640, 1100, 2304, 4096):
        kn = knobs(Case(entry="dpotrf", n=n, opts=()))
        why = "%d panel%s of %d%s" % (-(-n // kn["nb"]), "" if n <= kn["nb"] else "s", kn["nb"], ", look-ahead" if kn["lookahead"] else "")
        for pad in ((2,) if n == 4096 else (3,) if n == 2304 else (0, 2, 3)):
            if n in (1, 64) and pad == 3:
                continue                                  # (the leaf rows above hold them)
            rows.append(_row("dpotrf", n, why, pad=pad))
    return rows


def _reuse_rows():
    return [_row("plan", 1536, "a second exact matrix on the same plan: stale strip buffers, stale counters", ci=1, opts={"nb": 128, "outer": 256, "depth2": 1}, second=True),
            _row("plan", 1024, "a second exact matrix through the one-launch chain's counters and backup", ci=-1, opts={"nb": 256, "use_sb": 0}, second=True),
            _row("plan", 300, "a second exact matrix through the plain recursion", ci=0, second=True)]


def _pivot_rows():
    rows = []
    for r in (0, 63, 64, PIVOT_NB - 1, PIVOT_NB, PIVOT_N - 1):
        for G in (0, 32):
            rows.append(_row("plan", PIVOT_N, "pivot %d exactly -1 on the %s chain: info = %d" % (r, "one-launch" if G else "stepwise", r + 1), ci=1,
                             opts={"nb": PIVOT_NB, "chain_coop": G}, pivot=r))
    return rows


LEAF_CASES = _leaf_rows()
BLOCK_CASES = _block_rows()
SWEEP_CASES = _sweep_rows()
DPOTRF_CASES = _dpotrf_rows()
REUSE_CASES = _reuse_rows()
PIVOT_CASES = _pivot_rows()
EXACT_CASES = LEAF_CASES + BLOCK_CASES + SWEEP_CASES + DPOTRF_CASES + REUSE_CASES
CASES = EXACT_CASES + PIVOT_CASES


# ------------------------------------------------------------------------------------------------------------------------ the operands
@functools.lru_cache(maxsize=12)
def factor_pair(n, second=False):
    """(R, Rinv, N, d) exact; `second`: the same diagonal with N negated - another member of the family, R2 = 2 diag(d) - R"""
    R, Rinv, N, d = TC.family("F1", n, False)
    if second:
        N = -N
        R = d[:, None] * (np.eye(n) + N)
        Rinv = (np.eye(n) - N + TC._square_of_n(N, TC.classes(n))) / d[None, :]
        TC._check_inverse(R, Rinv)
        for a in (R, Rinv, N):
            a.setflags(write=False)
    return R, Rinv, N, d


@functools.lru_cache(maxsize=12)
def spd(n, second=False):
    """A = R^T R as a float64 product (exact: every partial sum is below (|R|^T |R|)_ij, which bounds() keeps far under 2^53)"""
    R = factor_pair(n, second)[0]
    A = R.T @ R
    assert np.abs(R).T.dot(np.abs(R)).max() * 4 < LIMIT and np.array_equal(A, A.T)
    A.setflags(write=False)
    return A


def operand(c, second=False):
    """the stored A of a row: NaN in the strictly lower triangle; `pivot` lowers one diagonal element so that this pivot is exactly -1"""
    A = stored(spd(c.n, second))
    if c.pivot is not None:
        d = factor_pair(c.n, second)[3]
        A[c.pivot, c.pivot] -= d[c.pivot] ** 2 + 1.0
    return A


def references(c, second=False):
    """(R, Rinv or None) a row's plan must hand out (full matrices, zero below the diagonal; cap_dpotrf: see dpotrf_reference)"""
    R, Rinv, _, _ = factor_pair(c.n, second)
    if c.entry != "plan" or c.ci < 0:
        return R, None
    if c.ci == 0 and not root_is_base(c.n, c.split):
        n1 = c.n >> c.split
        if 0 < n1 < c.n:
            Rinv = Rinv.copy()
            Rinv[:n1, n1:] = 0.0
    return R, Rinv


def dpotrf_reference(c):
    """cap_dpotrf works in place: R in the upper triangle, the NaNs of the lower triangle where they were"""
    return stored(factor_pair(c.n)[0])


# ---------------------------------------------------------------------------------------------------------- the premise of exactness
def panel_widths(c):
    """every width of a diagonal block whose explicit inverse multiplies a block row on a row's route"""
    kn = knobs(c)
    w = {min(64, c.n), min(kn["leaf"], c.n), min(kn["nb"], c.n)}
    n = c.n
    while n > kn["leaf"]:                                   # the halves of the recursion (whole matrix or one ragged panel)
        n = max(pick_split(n, kn["leaf"]), n - pick_split(n, kn["leaf"]))
        w.add(n)
    if c.entry == "plan" and c.ci >= 0:
        w.add(max(c.n >> c.split, 1))
        w.add(c.n)                                          # (covers every partition of the recursion: the comparison solve on the whole matrix)
    return sorted(w)


@functools.lru_cache(maxsize=4)
def _bound_parts(n, second):
    R, Rinv, N, d = factor_pair(n, second)
    aR = np.abs(R)
    S = 2.0 * (aR.T @ aR)
    Mi = TC._comparison(N, d)
    assert np.all(Mi >= np.abs(Rinv))
    return S, Mi, (np.abs(Rinv) @ aR @ np.abs(Rinv)).max()


@functools.lru_cache(maxsize=None)
def _solve_bound(n, second, w):
    S, Mi, _ = _bound_parts(n, second)
    worst = 0.0
    for o in range(0, n, w):
        worst = max(worst, (Mi[o:o + w, o:o + w].T @ S[o:o + w, o:]).max())
    return worst


def bounds(c, second=False):
    """{name: bound x 2^fraction bits} of everything a row's route forms; all must be < 2^53"""
    S, _, inv = _bound_parts(c.n, second)
    out = {"Schur updates 2 |R|^T |R| x 2^2": S.max() * 4}
    for w in panel_widths(c):
        out["block-row solve, width %d: M^-T 2 |R|^T |R| x 2^5" % w] = _solve_bound(c.n, second, w) * 32
    out["inverses |Rinv||R||Rinv| x 2^5"] = inv * 32
    return out


def check_premise(c):
    b = bounds(c)
    if c.second:
        b.update({"second: " + k: v for k, v in bounds(c, True).items()})
    for name, v in b.items():
        assert np.isfinite(v) and v < LIMIT, "%s: %s = 2^%.1f is not below 2^53" % (c.id, name, np.log2(v))
    return b


# --------------------------------------------------------------------------------------------------------------------------- the calls
UPPER = 1
OK, ERR_NOT_SPD = 0, 3


def create_plan(L, c):
    """a row's plan with its options set -> the plan handle (ctypes.c_void_p)"""
    import ctypes as C
    plan = C.c_void_p()
    st = L.cap_cholinv_plan_create(C.byref(plan), c.n, c.ci, c.split, BC, b"U", None)
    assert st == 0, (c.id, "cap_cholinv_plan_create", st)
    for k, v in c.opts:
        st = L.cap_cholinv_set_option(plan, k.encode(), v)
        assert st == 0, (c.id, "cap_cholinv_set_option", k, v, st)
    return plan


def plan_info(L, plan, stream=None):
    import ctypes as C
    info = C.c_int64(-1)
    st = L.cap_cholinv_info(plan, stream, C.byref(info))
    assert st == (OK if info.value == 0 else ERR_NOT_SPD), ("cap_cholinv_info", st, info.value)
    return int(info.value)
