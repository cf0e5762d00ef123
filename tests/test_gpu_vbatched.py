"""-m gpu: the variable-size batched Cholesky (cap_vbatch_plan_*, cap_dpotrf_vbatched, cap_dpotrs_vbatched, cap_dpotri_vbatched,
csrc/potrf_vbatched.hip) through the C ABI and capital_amd.batched.VarBatch.

Every flat buffer starts as NaNs with a payload of their own per element (tests/vbatched_cases.py): strictly lower triangles, padding rows,
gaps and a guard behind the buffer; whatever a call must not write is compared as int64 afterwards.  info and logdet start as sentinels: the
words of empty blocks must keep them.

What is exact:
 * the operand families F1 / F2 / F2i of tests/potri_batched_cases.py: A_i = T_i^T T_i must factor into exactly T_i and invert into exactly
   triu(T_i^-1 T_i^-T), compared as bits after -0 -> +0 (the convention of tests/test_gpu_potri_batched.py);
 * THE BIT CONTRACT on random SPD blocks: every block's factor, info, logdet, solutions and inverse are, as int64, what the FIXED-SIZE entries
   (cap_dpotrf_batched_blocked, cap_dpotrs_batched_blocked, cap_dpotri_batched) write for that block alone with n = n_i and batch = 1.
What is bounded, by bounds the fixed-size tests already use:
 * logdet of the exact families against 2 K log 2 (K = sum log2 t_jj, an integer): gamma_{n+2} 2 sum |log t_jj|, the bound of
   tests/test_gpu_potrf_batched_blocked.check_logdet (a logarithm within one ulp, n - 1 additions) - and bit for bit against the fixed-size entry;
 * the solve's componentwise residual |B - A X| <= gamma_{3n+4} |R|^T |R| |X| (solve_residual_ok of the same file)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import potri_batched_cases as P  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import vbatched_cases as V  # noqa: E402
from tests.gpu_util import DEV  # noqa: E402
from tests.test_gpu_potrf_batched_blocked import gamma, solve_residual_ok  # noqa: E402
from tests.test_gpu_potrf_batched_blocked import random_spd as well_conditioned  # noqa: E402
from tests.tri_cases import positive_zero  # noqa: E402

UPPER = 1
LD = np.longdouble
NRHS = (1, 3, 16, 17, 33)
INFO_SENTINEL, LOGDET_SENTINEL = -7, 123.5


@pytest.fixture(scope="module")
def L():
    from capital_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def exact_bits(a):
    return bits(positive_zero(a))


class Plan:
    """a layout of tests/vbatched_cases.py with its cap_vbatch_plan"""

    def __init__(self, L, sizes, kind):
        self.L, self.lay = L, V.Layout(sizes, kind)
        lay = self.lay
        arr = lambda a: None if a is None else (C.c_int64 * max(len(a), 1))(*[int(x) for x in a])
        self.handle = C.c_void_p()
        assert L.cap_vbatch_plan_create(lay.batch, arr(lay.sizes), arr(lay.ld_arg), arr(lay.off_arg), C.byref(self.handle)) == 0
        assert L.cap_vbatch_plan_info(self.handle, 1) == lay.total and L.cap_vbatch_plan_info(self.handle, 2) == lay.rows

    def __del__(self):
        if getattr(self, "handle", None):
            self.L.cap_vbatch_plan_destroy(self.handle)
            self.handle = None

    # every call: enqueue on the current stream; the caller synchronises by reading back
    def outputs(self, logdet=True):
        """info and logdet, filled with their sentinels on the CURRENT stream"""
        info = torch.full((max(self.lay.batch, 1),), INFO_SENTINEL, dtype=torch.int32, device=DEV)
        return info, (torch.full((max(self.lay.batch, 1),), LOGDET_SENTINEL, dtype=torch.float64, device=DEV) if logdet else None)

    def potrf(self, A, logdet=True, s=None, out=None):
        """out: outputs() made (and finished) beforehand - needed when s is not the stream the sentinels are filled on"""
        info, ld = out if out is not None else self.outputs(logdet)
        assert self.L.cap_dpotrf_vbatched(self.handle, UPPER, A.data_ptr(), info.data_ptr(), ld.data_ptr() if logdet else None,
                                          stream() if s is None else s) == 0
        return info, ld

    def potrs(self, R, B, nrhs, ldb, info=None, s=None):
        assert self.L.cap_dpotrs_vbatched(self.handle, UPPER, nrhs, R.data_ptr(), B.data_ptr(), ldb, info.data_ptr() if info is not None else None,
                                          stream() if s is None else s) == 0

    def potri(self, R, info=None, fill=0, s=None):
        assert self.L.cap_dpotri_vbatched(self.handle, UPPER, R.data_ptr(), info.data_ptr() if info is not None else None, fill,
                                          stream() if s is None else s) == 0

    def upper(self, host, i):
        idx, _ = self.lay.index(i, "upper")
        return host[idx]

    def live(self):
        return [i for i in range(self.lay.batch) if self.lay.sizes[i]]

    def check_sentinels(self, info, logdet=None):
        empty = [i for i in range(self.lay.batch) if not self.lay.sizes[i]]
        assert all(info[i] == INFO_SENTINEL for i in empty)
        if logdet is not None:
            assert all(logdet[i] == LOGDET_SENTINEL for i in empty)


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def untouched(before, after, may_write, what):
    keep = ~may_write
    bad = np.nonzero(bits(before)[keep] != bits(after)[keep])[0]
    assert bad.size == 0, "%s: %d elements outside the written set changed, the first at %d" % (what, bad.size, np.nonzero(keep)[0][bad[0]])


def rhs_buffer(rows, nrhs, ldb, Bfull):
    """stacked right-hand sides, column-major with ld ldb, NaN pattern in the padding rows and behind"""
    buf = V.nan_pattern(ldb * max(nrhs, 1) + V.GUARD, salt=7)
    mask = np.zeros(buf.shape, dtype=bool)
    for j in range(nrhs):
        buf[j * ldb:j * ldb + rows] = Bfull[:, j]
        mask[j * ldb:j * ldb + rows] = True
    return buf, mask


def stacked_rhs(rows, seed=0):
    return np.random.default_rng([99, rows, seed]).standard_normal((max(rows, 1), max(NRHS)))[:rows]


# --------------------------------------------------------------------------------------------------- the fixed-size entries, block by block
def fixed_reference(L, sizes, mats, Bfull):
    """per non-empty block i, from the fixed-size entries with n = n_i and batch = 1 on a packed copy of the block (NaN strictly lower
    triangle): {"R", "info", "logdet", "X": {nrhs: n x nrhs}, "inv0", "inv1"} - R / inv0 as the n (n + 1) / 2 upper elements in the
    order of Layout.index(i, "upper") (that of np.triu_indices), inv1 as the n x n window [r, c]; the solve and the inverse get the factor's info"""
    row_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    todo = []
    for i, n in enumerate(sizes):
        if not n:
            continue
        a = np.full((n, n), np.nan)
        iu = np.triu_indices(n)
        a[iu] = np.asarray(mats[i])[iu]
        R = dev(a.T.ravel())                                   # column-major: element (r, c) at r + c n
        info = torch.full((1,), INFO_SENTINEL, dtype=torch.int32, device=DEV)
        ld = torch.full((1,), LOGDET_SENTINEL, dtype=torch.float64, device=DEV)
        assert L.cap_dpotrf_batched_blocked(UPPER, n, R.data_ptr(), n, n * n, 1, info.data_ptr(), ld.data_ptr(), stream()) == 0
        up = info.data_ptr()
        X = {}
        for nrhs in NRHS:
            b = dev(Bfull[row_off[i]:row_off[i] + n, :nrhs].T.ravel())
            assert L.cap_dpotrs_batched_blocked(UPPER, n, nrhs, R.data_ptr(), n, n * n, b.data_ptr(), n, n * nrhs, 1, up, stream()) == 0
            X[nrhs] = b
        inv = [R.clone(), R.clone()]
        for fill in (0, 1):
            assert L.cap_dpotri_batched(UPPER, n, inv[fill].data_ptr(), n, n * n, 1, up, fill, stream()) == 0
        todo.append((i, n, R, info, ld, X, inv))
    torch.cuda.synchronize()
    out = {}
    for i, n, R, info, ld, X, inv in todo:
        iu = np.triu_indices(n)
        cm = lambda t: t.cpu().numpy().reshape(n, n).T         # [r, c]
        out[i] = {"R": cm(R)[iu], "info": int(info.item()), "logdet": ld.cpu().numpy().copy(), "inv0": cm(inv[0])[iu], "inv1": cm(inv[1]),
                  "X": {k: v.cpu().numpy().reshape(k, n).T for k, v in X.items()}}
    return out


@functools.lru_cache(maxsize=None)
def random_case(name, kappa):
    """(sizes, mats, Bfull) of a list with random SPD blocks - host data, shared and never modified"""
    sizes = V.LISTS[name]
    mats = V.random_blocks(sizes, kappa)
    for m in mats:
        if m is not None:
            m.setflags(write=False)
    B = stacked_rhs(int(np.sum(sizes)), seed=int(np.log10(kappa)))
    B.setflags(write=False)
    return sizes, mats, B


_FIXED = {}


def fixed_for(L, name, kappa):
    """the fixed-size reference of random_case(name, kappa): computed once, shared by the tests that need it"""
    if (name, kappa) not in _FIXED:
        sizes, mats, B = random_case(name, kappa)
        _FIXED[(name, kappa)] = fixed_reference(L, sizes, mats, B)
    return _FIXED[(name, kappa)]


def run_all(L, sizes, mats, Bfull, kind, info_override=None, want=("factor", "solve", "inverse")):
    """factor, solve (every nrhs of NRHS, ldb = rows + 2) and inverse (fill 0 and 1) of one batch in one layout; everything a call must not
    write is checked here.  info_override(info tensor) -> the info (tensor or None) the solve and the inverse get.
    -> {"R": host buffer, "info", "logdet", "X": {nrhs: rows x nrhs}, "inv0": host buffer, "inv1": host buffer, "plan"}"""
    pl = Plan(L, sizes, kind)
    lay = pl.lay
    before = lay.buffer(mats)
    A = dev(before)
    info, logdet = pl.potrf(A)
    R = A.cpu().numpy()
    untouched(before, R, lay.written("upper"), "potrf %s" % kind)
    out = {"R": R, "info": info.cpu().numpy(), "logdet": logdet.cpu().numpy(), "plan": pl, "X": {}}
    pl.check_sentinels(out["info"], out["logdet"])
    use = info if info_override is None else info_override(info)
    if "solve" in want:
        ldb = lay.rows + 2
        for nrhs in NRHS:
            b0, mask = rhs_buffer(lay.rows, nrhs, ldb, Bfull)
            Bd = dev(b0)
            pl.potrs(A, Bd, nrhs, ldb, use)
            b1 = Bd.cpu().numpy()
            untouched(b0, b1, mask, "potrs nrhs %d" % nrhs)
            out["X"][nrhs] = np.stack([b1[j * ldb:j * ldb + lay.rows] for j in range(nrhs)], axis=1) if lay.rows else np.zeros((0, nrhs))
        assert np.array_equal(bits(A.cpu().numpy()), bits(R)), "potrs wrote its factor"
    if "inverse" in want:
        for fill in (0, 1):
            Ai = dev(R)
            pl.potri(Ai, use, fill)
            got = Ai.cpu().numpy()
            untouched(R, got, lay.written("window" if fill else "upper"), "potri fill %d" % fill)
            out["inv%d" % fill] = got
    return out


def assert_matches_fixed(res, ref, what, parts=("factor", "solve", "inverse")):
    pl = res["plan"]
    lay = pl.lay
    for i in pl.live():
        n, r = int(lay.sizes[i]), ref[i]
        tag = "%s block %d (n = %d)" % (what, i, n)
        assert np.array_equal(bits(pl.upper(res["R"], i)), bits(r["R"])), tag + ": factor"
        assert res["info"][i] == r["info"], tag + ": info %d != %d" % (res["info"][i], r["info"])
        assert np.array_equal(bits(res["logdet"][i:i + 1]), bits(r["logdet"])), tag + ": logdet"
        if "solve" in parts:
            for nrhs, X in res["X"].items():
                mine = X[lay.row_off[i]:lay.row_off[i] + n]
                assert np.array_equal(bits(mine), bits(r["X"][nrhs])), tag + ": solve with nrhs %d" % nrhs
        if "inverse" in parts:
            assert np.array_equal(bits(pl.upper(res["inv0"], i)), bits(r["inv0"])), tag + ": inverse"
            assert np.array_equal(bits(lay.block(res["inv1"], i)), bits(r["inv1"])), tag + ": inverse with fill"


# ------------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("kind", V.LAYOUTS)
@pytest.mark.parametrize("name", sorted(V.LISTS))
@pytest.mark.parametrize("fam", V.FAMILIES)
def test_exact_factor_and_inverse(L, fam, name, kind):
    """1. A_i = T_i^T T_i: potrf leaves exactly T_i, info 0, logdet within the fixed-size tests' bound of the exact 2 K log 2; potri leaves
    exactly triu(T_i^-1 T_i^-T), with fill = 1 the mirrored block; every NaN that is not written is still the same NaN"""
    sizes = V.LISTS[name]
    blocks = V.exact_blocks(fam, sizes)
    pl = Plan(L, sizes, kind)
    lay = pl.lay
    before = lay.buffer([None if b is None else b[0].T @ b[0] for b in blocks])
    A = dev(before)
    info, logdet = pl.potrf(A)
    R = A.cpu().numpy()
    info, logdet = info.cpu().numpy(), logdet.cpu().numpy()
    untouched(before, R, lay.written("upper"), "potrf")
    pl.check_sentinels(info, logdet)
    for i in pl.live():
        T, _, Cm = blocks[i]
        iu = np.triu_indices(int(sizes[i]))
        assert np.array_equal(exact_bits(pl.upper(R, i)), exact_bits(T[iu])), "block %d (n = %d): the factor is not T" % (i, sizes[i])
        assert info[i] == 0
        want, scale = V.exact_logdet(T)
        err = abs(LD(logdet[i]) - want)
        assert err <= gamma(int(sizes[i]) + 2) * scale, "block %d: logdet %r, exact %r" % (i, logdet[i], want)
    pl.potri(A, dev(info))
    X = A.cpu().numpy()
    untouched(R, X, lay.written("upper"), "potri")
    for i in pl.live():
        iu = np.triu_indices(int(sizes[i]))
        assert np.array_equal(exact_bits(pl.upper(X, i)), exact_bits(blocks[i][2][iu])), "block %d (n = %d): the inverse" % (i, sizes[i])
    before = lay.buffer([None if b is None else b[0] for b in blocks])
    A = dev(before)
    pl.potri(A, None, 1)
    X = A.cpu().numpy()
    untouched(before, X, lay.written("window"), "potri fill = 1")
    for i in pl.live():
        n = int(sizes[i])
        got = lay.block(X, i)
        iu, il = np.triu_indices(n), np.tril_indices(n, -1)
        assert np.array_equal(exact_bits(got[iu]), exact_bits(blocks[i][2][iu])), "block %d (n = %d): the inverse with fill" % (i, n)
        assert np.array_equal(bits(got[il]), bits(got.T[il])), "block %d: not mirrored bit for bit" % i


@pytest.mark.parametrize("kappa", P.KAPPAS)
@pytest.mark.parametrize("name", ("EVERY", "WAVES", "EDGES"))
def test_bit_equality_with_the_fixed_size_entries(L, name, kappa):
    """2. random SPD blocks: factor, info, logdet, solve with nrhs = 1, 3, 16, 17, 33 at ldb = rows + 2 and inverse with fill 0 and 1
    equal, as bits, what the fixed-size entry gives for each block alone; in two layouts per case (all four over the cases)"""
    sizes, mats, B = random_case(name, kappa)
    ref = fixed_for(L, name, kappa)
    assert all(r["info"] == 0 for r in ref.values())
    k = ("EVERY", "WAVES", "EDGES").index(name) + P.KAPPAS.index(kappa)
    for kind in (V.LAYOUTS[k % 4], V.LAYOUTS[(k + 2) % 4]):
        assert_matches_fixed(run_all(L, sizes, mats, B, kind), ref, "%s kappa %g %s" % (name, kappa, kind))


@pytest.mark.parametrize("name", ("EVERY", "WAVES", "EDGES"))
def test_order_and_company_independence(L, name):
    """3. the batch in another order (other waves, other neighbours, other class lists), the plan rebuilt: every block's bits, info and logdet
    follow the permutation - checked against the fixed-size reference of the unpermuted batch, block by block"""
    kappa = 1e6
    sizes, mats, B = random_case(name, kappa)
    ref = fixed_for(L, name, kappa)
    row_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    for seed in (1, 2):
        perm = np.random.default_rng([33, seed]).permutation(len(sizes))
        psizes = tuple(int(sizes[j]) for j in perm)
        pmats = [mats[j] for j in perm]
        pB = np.concatenate([B[row_off[j]:row_off[j] + sizes[j]] for j in perm], axis=0) if len(B) else B
        pref = {k: ref[int(j)] for k, j in enumerate(perm) if sizes[j]}
        assert_matches_fixed(run_all(L, psizes, pmats, pB, V.LAYOUTS[seed]), pref, "%s permutation %d" % (name, seed))


def _failing(name):
    """{block: (row p (0-based), bad value)} - neighbours inside one wave, first / middle / last row, a NaN pivot, and for the blocked path
    rows in the second diagonal block"""
    if name == "WAVES":       # the sorted NP = 8 list starts with the blocks of n = 5: 0, 4, 8, ... share the first wave
        return {0: (0, -1.0), 4: (2, 0.0), 8: (4, np.nan), 1: (5, -2.0), 70: (4, np.nan), 71: (100, -1.0)}
    return {0: (0, np.nan), 1: (32, -1.0), 2: (64, 0.0), 3: (70, -3.0), 4: (0, -1.0), 5: (191, np.nan), 13: (192, -1.0), 7: (16, 0.0), 8: (63, -1.0)}


@pytest.mark.parametrize("name", ("WAVES", "EDGES"))
def test_failed_blocks(L, name):
    """4. a pivot that is not > 0 (negative, zero, NaN) in some blocks: info is the 1-based row, NaN from that row of R on and nowhere else,
    logdet NaN; every other block - the neighbours in the same wave too - is bit-identical to the run without the failure; potrs and
    potri with that info write NaN for exactly those blocks; a hand-set info flags good factors without reading them, info = NULL
    treats every block as good.  All of it equal to the fixed-size entries on the same blocks."""
    sizes, clean, B = random_case(name, 1e1)
    fail = _failing(name)
    mats = [None if m is None else m.copy() for m in clean]
    for b, (p, v) in fail.items():
        assert p < sizes[b]
        mats[b][p, p] = v
    good_ref = fixed_for(L, name, 1e1)
    ref = fixed_reference(L, sizes, mats, B)
    res = run_all(L, sizes, mats, B, "ld+3")
    assert_matches_fixed(res, ref, name + " with failures")
    pl = res["plan"]
    lay = pl.lay
    for i in pl.live():
        n = int(sizes[i])
        iu = np.triu_indices(n)
        Rm = np.full((n, n), 0.0)
        Rm[iu] = pl.upper(res["R"], i)
        rows = slice(lay.row_off[i], lay.row_off[i] + n)
        if i in fail:
            p = fail[i][0]
            assert res["info"][i] == p + 1 and np.isnan(res["logdet"][i])
            assert np.isnan(Rm[iu][iu[0] >= p]).all() and not np.isnan(Rm[iu][iu[0] < p]).any()
            gi = np.triu_indices(n)
            assert np.array_equal(bits(Rm[gi][gi[0] < p]), bits(good_ref[i]["R"][gi[0] < p])), "rows in front of the failure changed"
            assert all(np.isnan(X[rows]).all() for X in res["X"].values())
            assert np.isnan(pl.upper(res["inv0"], i)).all() and np.isnan(lay.block(res["inv1"], i)).all()
        else:                  # as if nothing had failed anywhere
            assert res["info"][i] == 0
            assert np.array_equal(bits(pl.upper(res["R"], i)), bits(good_ref[i]["R"])), "block %d changed with a neighbour's failure" % i
            assert np.array_equal(bits(res["logdet"][i:i + 1]), bits(good_ref[i]["logdet"]))
            assert all(np.array_equal(bits(X[rows]), bits(good_ref[i]["X"][k])) for k, X in res["X"].items())
            assert np.array_equal(bits(pl.upper(res["inv0"], i)), bits(good_ref[i]["inv0"]))
            assert np.array_equal(bits(lay.block(res["inv1"], i)), bits(good_ref[i]["inv1"]))
    # good factors with a hand-set info: NaN exactly there; then info = NULL on factors of which some failed: computed, not flagged
    hand = np.zeros(len(sizes), dtype=np.int32)
    hand[list(fail)] = 7
    res = run_all(L, sizes, clean, B, "gaps", info_override=lambda info: dev(hand))
    for i in res["plan"].live():
        rows = slice(res["plan"].lay.row_off[i], res["plan"].lay.row_off[i] + sizes[i])
        if i in fail:
            assert all(np.isnan(X[rows]).all() for X in res["X"].values()) and np.isnan(res["plan"].upper(res["inv0"], i)).all()
            assert np.isnan(res["plan"].lay.block(res["inv1"], i)).all()
        else:
            assert all(np.array_equal(bits(X[rows]), bits(good_ref[i]["X"][k])) for k, X in res["X"].items())
            assert np.array_equal(bits(res["plan"].upper(res["inv0"], i)), bits(good_ref[i]["inv0"]))
    res = run_all(L, sizes, clean, B, "reverse", info_override=lambda info: None)
    assert_matches_fixed(res, good_ref, name + " info = NULL")


def test_solve_residuals(L):
    """5. EVERY with the well-conditioned random blocks of the fixed-size tests: the componentwise residual of every block and right-hand side
    within gamma_{3n+4} |R|^T |R| |X| (the bound of tests/test_gpu_potrf_batched_blocked.py); numpy.linalg.solve on the same blocks is
    printed beside it - what is attainable"""
    sizes = V.EVERY
    rng = np.random.default_rng(5)
    mats = [well_conditioned(rng, n, 1)[0] if n else None for n in sizes]
    B = stacked_rhs(int(np.sum(sizes)), seed=5)
    res = run_all(L, sizes, mats, B, "gaps", want=("factor", "solve"))
    pl = res["plan"]
    assert not res["info"][pl.live()].any()
    for i in pl.live():
        n = int(sizes[i])
        iu = np.triu_indices(n)
        R = np.zeros((n, n))
        R[iu] = pl.upper(res["R"], i)
        rows = slice(pl.lay.row_off[i], pl.lay.row_off[i] + n)
        X = res["X"][33][rows]
        solve_residual_ok(mats[i], R, X, B[rows, :33], tag="block %d" % i)
        Xn = np.linalg.solve(mats[i], B[rows, :33])
        bound = gamma(3 * n + 4) * ((np.abs(R).T @ np.abs(R)).astype(LD) @ np.abs(Xn).astype(LD))
        rn = np.abs(B[rows, :33].astype(LD) - mats[i].astype(LD) @ Xn.astype(LD))
        print("block %d n %d: numpy.linalg.solve residual / bound = %.3f" % (i, n, float(np.max(rn[bound > 0] / bound[bound > 0]))))


@pytest.mark.parametrize("n", sorted(V.LONE))
def test_lone_blocks(L, n):
    """6a. a plan of one block, at the ends of both kernel paths"""
    sizes = V.LONE[n]
    mats = V.random_blocks(sizes, 1e6)
    B = stacked_rhs(n, seed=n)
    ref = fixed_reference(L, sizes, mats, B)
    for kind in ("packed", "ld+3"):
        assert_matches_fixed(run_all(L, sizes, mats, B, kind), ref, "lone %d %s" % (n, kind))


def test_degenerate_batches(L):
    """6b. a batch of zeros only and an empty batch: nothing is written, NULL pointers are fine; nrhs = 0 writes nothing; a plan used twice
    with different data"""
    for sizes in ((0, 0, 0), ()):
        pl = Plan(L, sizes, "packed")
        assert L.cap_vbatch_plan_info(pl.handle, 4) == 0
        assert L.cap_dpotrf_vbatched(pl.handle, UPPER, None, None, None, stream()) == 0
        assert L.cap_dpotrs_vbatched(pl.handle, UPPER, 3, None, None, 0, None, stream()) == 0
        assert L.cap_dpotri_vbatched(pl.handle, UPPER, None, None, 1, stream()) == 0
        guard = dev(V.nan_pattern(8))
        info, logdet = pl.potrf(guard)
        pl.potrs(guard, guard, 2, 1, info)
        pl.potri(guard, info, 1)
        assert np.array_equal(bits(guard.cpu().numpy()), bits(V.nan_pattern(8)))
        assert (info.cpu().numpy() == INFO_SENTINEL).all() and (logdet.cpu().numpy() == LOGDET_SENTINEL).all()
    sizes, mats, B = random_case("EDGES", 1e1)
    ref = fixed_for(L, "EDGES", 1e1)
    pl = Plan(L, sizes, "packed")
    A = dev(pl.lay.buffer(mats))
    info, _ = pl.potrf(A)
    b0 = V.nan_pattern(pl.lay.rows + 8)
    Bd = dev(b0)
    pl.potrs(A, Bd, 0, pl.lay.rows, info)
    assert np.array_equal(bits(Bd.cpu().numpy()), bits(b0))
    # the same plan, other data
    mats2 = [m * 4.0 for m in mats]
    A2 = dev(pl.lay.buffer(mats2))
    info2, ld2 = pl.potrf(A2)
    R1, R2 = A.cpu().numpy(), A2.cpu().numpy()
    for i in pl.live():
        assert np.array_equal(bits(pl.upper(R1, i)), bits(ref[i]["R"]))
        assert np.array_equal(bits(pl.upper(R2, i)), bits(2.0 * ref[i]["R"]))      # a power-of-two scaling is exact in every step
    assert not info2.cpu().numpy().any()


def test_one_plan_on_two_streams(L):
    """6c. one plan used from two non-blocking streams at once on two buffers: both results equal the serial run"""
    sizes, mats, B = random_case("EVERY", 1e1)
    ref = fixed_for(L, "EVERY", 1e1)
    pl = Plan(L, sizes, "ld+3")
    lay = pl.lay
    host = lay.buffer(mats)
    ldb = lay.rows
    b0, _ = rhs_buffer(lay.rows, 17, ldb, B)
    env = SO.Env(2)                        # two caller streams, asserted non-blocking
    streams = env.streams
    torch.cuda.synchronize()
    outs = []
    for s in streams:
        with torch.cuda.stream(s):
            A, Bd = dev(host), dev(b0)
            outs.append((A, Bd))
    pre = [pl.outputs() for _ in streams]  # the sentinels are in place before anything is enqueued on the caller streams
    torch.cuda.synchronize()
    results = []
    for rep in range(3):                   # interleaved: factor on both, then solve on both, then inverse on both
        for s, (A, Bd) in zip(streams, outs):
            h = s.cuda_stream
            if rep == 0:
                results.append(pl.potrf(A, s=h, out=pre[streams.index(s)]))
            elif rep == 1:
                pl.potrs(A, Bd, 17, ldb, results[streams.index(s)][0], s=h)
            else:
                Ai = torch.empty_like(A)
                with torch.cuda.stream(s):
                    Ai.copy_(A)
                pl.potri(Ai, results[streams.index(s)][0], 1, s=h)
                results.append(Ai)
    torch.cuda.synchronize()
    for k, (A, Bd) in enumerate(outs):
        res = {"plan": pl, "R": A.cpu().numpy(), "info": results[k][0].cpu().numpy(), "logdet": results[k][1].cpu().numpy(),
               "X": {17: np.stack([Bd.cpu().numpy()[j * ldb:j * ldb + lay.rows] for j in range(17)], axis=1)},
               "inv1": results[2 + k].cpu().numpy()}
        res["inv0"] = res["inv1"]          # (the upper triangle of the filled inverse is the inverse)
        assert_matches_fixed(res, ref, "stream %d" % k, parts=("factor", "solve"))
        for i in pl.live():
            assert np.array_equal(bits(lay.block(res["inv1"], i)), bits(ref[i]["inv1"]))
    env.close()


def test_python_layer(L):
    """VarBatch: pack / block in torch's reading, potrf / potrs / potri against torch on well-conditioned blocks, and the bits of the C entry"""
    from capital_amd import batched
    sizes = (3, 0, 70, 9, 64, 130)
    rng = np.random.default_rng(11)
    mats = [well_conditioned(rng, n, 1)[0] if n else np.zeros((0, 0)) for n in sizes]
    vb = batched.VarBatch(sizes, ld=[n + 1 for n in sizes])
    A = vb.pack([torch.from_numpy(m) for m in mats])
    assert A.is_cuda and A.numel() == vb.total
    for i, m in enumerate(mats):
        assert np.array_equal(vb.block(A, i).cpu().numpy(), m)
    info, logdet = vb.potrf(A, logdet=True)
    assert not info.cpu().numpy().any() and logdet.cpu().numpy()[1] == 0.0
    ref = fixed_reference(L, sizes, mats, stacked_rhs(sum(sizes), seed=1))
    B = torch.from_numpy(stacked_rhs(sum(sizes), seed=1)[:, :5].T.copy()).to(DEV)      # (nrhs, rows)
    Bin = B.clone()
    assert vb.potrs(A, B, info) is B
    one = Bin[0].clone()
    vb.potrs(A, one)
    assert torch.equal(one, B[0])
    for i, n in enumerate(sizes):
        if not n:
            continue
        Lt = np.tril(vb.block(A, i).cpu().numpy())
        want = torch.linalg.cholesky(torch.from_numpy(mats[i])).numpy()
        assert np.allclose(Lt, want, rtol=0, atol=n * gamma(n + 2) * np.abs(want).max() * 8)
        assert np.array_equal(bits(vb.block(A, i).cpu().numpy().T[np.triu_indices(n)]), bits(ref[i]["R"]))      # torch's lower triangle is R^T
        rows = slice(vb.row_offsets[i], vb.row_offsets[i] + n)
        assert np.array_equal(bits(B.cpu().numpy()[:3, rows].T), bits(ref[i]["X"][3]))
        assert np.array_equal(bits(logdet.cpu().numpy()[i:i + 1]), bits(ref[i]["logdet"]))
    assert vb.potri(A, info, symmetric=True) is A
    for i, n in enumerate(sizes):
        if n:
            got = vb.block(A, i).cpu().numpy()
            assert np.array_equal(bits(got), bits(got.T)) and np.array_equal(bits(got.T), bits(ref[i]["inv1"]))
