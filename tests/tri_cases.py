"""One case table for the triangular inverse and solve paths - cap_dtrtri (rec_trtri + leaf_trtri_kernel), cap_dtrsm (cap_trsm_prepare +
cap_trsm_apply), cap_dpotrs (potrs_subst_kernel<1|2|4|8|16> and the blocked route above 16 right-hand sides) and cap_dpotri (TRTRI +
cap_dlauum) - shared by tests/test_tri_cases.py (no GPU: every row through the library's own object files on the recording stand-in) and
tests/test_gpu_tri_exact.py (-m gpu: the same rows on the device, bit for bit).  NumPy only, nothing of torch or the GPU is imported here.

EXACT RESULTS.  leaf_trtri_kernel forms the reciprocals of the diagonal with a true division and everything after that only multiplies and
adds, so with a power-of-two diagonal every value these routes form is a dyadic rational; while the magnitudes (times 2^fraction bits)
stay below 2^53, any summation order and any FMA contraction is exact and a float64 NumPy product of the exact operands IS the result.
All operands are upper triangular, every strictly lower element of a stored operand is NaN.

  F1 "three classes"    class(i) = 2 - ((n - 1 - i) mod 3); N[i, j] from {+-1, +-2} where i < j and class(i) < class(j), else 0;
                        T = diag(d) (I + N), d_i from {1/2, 1, 2, 4} (random signs for TRTRI / TRSM, positive for POTRS / POTRI).
                        N^3 = 0, so T^-1 = (I - N + N^2) diag(d)^-1 exactly.  About a third of every off-diagonal 16 x 16 tile of T and of
                        T^-1 is nonzero; the classes count from the END so that the one-column last block of n = 128 k + 1 is not empty.
                        Three classes, not four: with four the POTRS bound below passes 2^53 at n = 2304.
  F2 "dense"            T = diag(d) S1 C S2, C the all-ones upper triangle, S1 / S2 random +-1 diagonals: every upper element nonzero,
                        T^-1 = S2 C^-1 S1 diag(d)^-1 bidiagonal.
  F2' "bidiagonal"      the inverse of an F2 matrix used as T: a bidiagonal T whose inverse has every upper element nonzero.
  right-hand sides      integers of {+-1, +-2, +-3}; alpha from {1, -1, 2, -1/2}.

THE PREMISE IS ASSERTED, NOT ASSUMED (bounds()).  Every partial sum of a product sum_k a_ik b_kj, in ANY order, is bounded by the entry
(|A| |B|)_ij - never more than (number of terms) x max|A| x max|B|, and sharp enough to admit n = 4224.  For every row:
  * inverse routes (rec_trtri on the matrix or on the diagonal blocks of a substitution; the 16-blocked leaf inside): every intermediate
    is a sub-block of T, of T^-1, of T12 T22^-1 or of T11^-1 (T12 T22^-1), all bounded by sub-blocks of |T^-1| |T| |T^-1| (and the
    leaf's substitution sums by |T| |T^-1|), with 5 fraction bits;
  * substitutions (F1 only), in any block order and width: with the comparison matrix M = |D| (I - |N|), M^-1 = (I + |N| + |N|^2) |D|^-1
    >= |T^-1| elementwise, the solution Xc = M^-1 |alpha B| of the comparison system bounds every block solution by induction over the
    blocks, every partial sum of a block-inverse product by Xc, and every partial sum S_i and right-hand side B_i - S_i by
    |alpha B| + |strict upper T| Xc.  POTRS chains two of them (5 fraction bits at the end);
  * the triangular product of POTRI: |T^-1| |T^-1|^T, 4 fraction bits.
All of them must be < 2^53.  A row that fails is a bad row, not a reason to loosen anything.

REFERENCES.  T^-1 from the closed forms above; the module asserts T @ Tinv == I and Tinv @ T == I elementwise.  alpha op(T)^-1 B,
alpha B op(T)^-1, T^-1 T^-T B and triu(T^-1 T^-T) are float64 products of these exact operands under the bounds above; at n <= 40
tests/test_tri_cases.py recomputes all of them with fractions.Fraction.

A row names what it must launch: `kernels`, the launches in order among leaf_trtri_kernel / potrs_subst_kernel<NR> / potrs_nan_kernel /
dlauum_nt_kernel, `gemms`, the number of dgemm_* product launches, and `scales`, the scale_kernel launches (alpha != 1 in TRSM)."""
import functools

import numpy as np

NAN = np.float64("nan")
RHS_VALUES = np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])
ALPHAS = (1.0, -1.0, 2.0, -0.5)
DIAG = np.array([0.5, 1.0, 2.0, 4.0])
LEAF = "leaf_trtri_kernel"
LAUUM = "dlauum_nt_kernel"
LEAF_MAX = 64
POTRS_BLOCK = 128
LIMIT = 2.0 ** 53


def SUBST(nr):
    return "potrs_subst_kernel<%d>" % nr


class Case(dict):
    """a row: op (trtri / trsm / potrs / potri), fam (F1 / F2 / F2i), n (the triangle), other (right-hand sides / the other extent of B),
    form (side + trans of TRSM), alpha, pads (rows between T / B and their leading dimensions), woff (elements the work pointer is moved
    off its 16-byte alignment), kernels, gemms, scales, why"""
    __getattr__ = dict.__getitem__

    @property
    def id(self):
        s = "%s-%s-n%d" % (self.op, self.fam, self.n)
        if self.op == "trsm":
            s += "-%s-x%d-a%g" % (self.form, self.other, self.alpha)
        if self.op == "potrs":
            s += "-r%d" % self.other
        s += "-pad%d" % self.pads[0] + ("_%d" % self.pads[1] if self.op in ("trsm", "potrs") else "")
        return s + ("-woff%d" % self.woff if self.woff else "")

    @property
    def signed(self):
        return self.op in ("trtri", "trsm")


# ------------------------------------------------------------------------------------------------- what the host side is expected to do
def pick_split(n, leaf=LEAF_MAX):
    """rec_trtri's partition: half of n rounded down to a multiple of 128 (n >= 512) or of the leaf, else min(leaf, n - 1)"""
    q = 128 if n >= 512 else leaf
    h = (n // 2) // q * q
    return h if h > 0 else min(leaf, n - 1)


def leaf_sizes(n):
    """the sizes of the leaf_trtri_kernel launches of rec_trtri(n), in launch order"""
    if n <= LEAF_MAX:
        return [n]
    h = pick_split(n)
    return leaf_sizes(h) + leaf_sizes(n - h)


def leaf_padding(n):
    return 16 if n <= 16 else 32 if n <= 32 else 64


def trsm_block(td):
    """block width of the blocked substitution: round_up(td, 2) below 128, 128 up to 511, 256 from 512, 512 from 2048"""
    return min(512 if td >= 2048 else 256 if td >= 512 else 128, (max(td, 1) + 1) // 2 * 2)


def blocks(n, tb):
    return [min(tb, n - o) for o in range(0, n, tb)]


def _prepare(n, tb):
    """(leaf launches, GEMM launches) of cap_trsm_prepare: every diagonal block inverted by rec_trtri"""
    leaves = [len(leaf_sizes(w)) for w in blocks(n, tb)]
    return sum(leaves), sum(2 * (l - 1) for l in leaves)


def expected_launches(op, n, other=0, alpha=1.0, woff=0):
    if op == "trtri":
        l = len(leaf_sizes(n))
        return [LEAF] * l, 2 * (l - 1), 0
    if op == "trsm":
        tb = trsm_block(n)
        l, g = _prepare(n, tb)
        nblk = len(blocks(n, tb))
        return [LEAF] * l, g + nblk + (nblk - 1), int(alpha != 1.0)
    if op == "potrs":
        if other <= 16:
            l, g = _prepare(n, POTRS_BLOCK)
            nr = 1 if other <= 1 else 2 if other <= 2 else 4 if other <= 4 else 8 if other <= 8 else 16
            return [LEAF] * l + [SUBST(nr)] * 4, g, 0
        tb = trsm_block(n)
        l, g = _prepare(n, tb)
        nblk = len(blocks(n, tb))
        return [LEAF] * l, g + 2 * (nblk + nblk - 1), 0
    assert op == "potri"
    l = len(leaf_sizes(n))
    g = 2 * (l - 1)
    if woff & 1:                          # the inverse is not 16-byte aligned: cap_dlauum's copy route, one dense product
        return [LEAF] * l, g + 1, 0
    n0, r = n // 128 * 128, n % 128
    return [LEAF] * l + ([LAUUM] if n0 else []), g + ((3 if n0 else 1) if r else 0), 0


# ----------------------------------------------------------------------------------------------------------------------------- the rows
TRTRI_N = (1, 2, 15, 16, 17, 33, 64, 65, 100, 127, 128, 129, 200, 255, 256, 300, 511, 512, 513, 640, 777, 1000, 1152, 2304)
TRTRI_F2_N = (65, 129, 300, 513, 1000)
TRSM_TD = (1, 2, 7, 100, 127, 128, 129, 300, 511, 512, 640, 1000, 2047, 2048, 2176)
TRSM_OTHER = (1, 5, 16, 130, 520)
TRSM_FORMS = ("LN", "LT", "RN", "RT")
TRSM_PADS = ((0, 0), (2, 2), (3, 1), (1, 3))            # ldt, ldb: tight, even, odd
POTRS_N = (1, 2, 64, 127, 128, 129, 255, 256, 300, 640, 1000, 1153, 2304, 4224)
POTRS_NRHS = (1, 2, 3, 4, 5, 8, 9, 16)
POTRS_ALL_NRHS_N = (129, 300, 1153)
POTRS_BLOCKED = ((300, 128), (1000, 256), (2176, 512))  # n, the block width it takes
POTRS_BLOCKED_NRHS = (17, 40, 130)
POTRI_N = (1, 100, 128, 129, 640, 1155)


def _row(op, fam, n, why, other=0, form="", alpha=1.0, pads=(0, 0), woff=0):
    kernels, gemms, scales = expected_launches(op, n, other, alpha, woff)
    return Case(op=op, fam=fam, n=n, other=other, form=form, alpha=alpha, pads=pads, woff=woff, kernels=kernels, gemms=gemms, scales=scales, why=why)


def _trtri_rows():
    rows = []
    for n in TRTRI_N:
        sizes = leaf_sizes(n)
        why = "%d lea%s, padded to %s" % (len(sizes), "f" if len(sizes) == 1 else "ves", "/".join(str(p) for p in sorted({leaf_padding(s) for s in sizes})))
        if n > LEAF_MAX:
            why += "; root split %d + %d" % (pick_split(n), n - pick_split(n))
        for pad in ((3,) if n == 2304 else (0, 2, 3)):          # lda = n, n + 2, n + 3 (odd for the even n); the largest size once
            rows.append(_row("trtri", "F1", n, why, pads=(pad, 0)))
    for i, n in enumerate(TRTRI_F2_N):
        rows.append(_row("trtri", "F2", n, "dense T, bidiagonal inverse: one wrong row or column anywhere", pads=((2, 3, 0)[i % 3], 0)))
        rows.append(_row("trtri", "F2i", n, "bidiagonal T, dense inverse", pads=((3, 0, 2)[i % 3], 0)))
    return rows


def _trsm_rows():
    rows = []
    for ti, td in enumerate(TRSM_TD):
        tb = trsm_block(td)
        bl = blocks(td, tb)
        shape = "one block of %d" % bl[0] if len(bl) == 1 else "%d blocks of %d%s" % (len(bl), tb, "" if bl[-1] == tb else ", ragged last block of %d" % bl[-1])
        for fi, form in enumerate(TRSM_FORMS):
            r = 4 * ti + fi
            rows.append(_row("trsm", "F1", td, shape, other=TRSM_OTHER[(ti + 2 * fi) % 5], form=form, alpha=ALPHAS[(ti + fi) % 4], pads=TRSM_PADS[(r + r // 4) % 4]))
    return rows


def _potrs_rows():
    rows, pads = [], ((0, 0), (2, 2), (1, 3), (3, 1))
    k = 0
    for i, n in enumerate(POTRS_N):
        bl = blocks(n, POTRS_BLOCK)
        items = len(bl) * (len(bl) + 1) // 2
        why = "one launch per substitution: %d block%s = %d item%s%s" % (len(bl), "" if len(bl) == 1 else "s", items, "" if items == 1 else "s",
                                                                        "" if bl[-1] == POTRS_BLOCK else ", last block %d" % bl[-1])
        if n == 4224:
            counts = (5,)                 # more items than workgroups: workgroups claim several tickets; the largest size once
        elif n in POTRS_ALL_NRHS_N:
            counts = POTRS_NRHS
        else:
            counts = (POTRS_NRHS[(3 * i) % 8], POTRS_NRHS[(3 * i + 5) % 8])
        for nrhs in counts:
            rows.append(_row("potrs", "F1", n, why, other=nrhs, pads=pads[k % 4]))
            k += 1
    for n, tb in POTRS_BLOCKED:
        for nrhs in POTRS_BLOCKED_NRHS:
            rows.append(_row("potrs", "F1", n, "blocked route, block width %d" % tb, other=nrhs, pads=pads[1 + k % 3]))
            k += 1
    return rows


def _potri_rows():
    rows = []
    for n in POTRI_N:
        n0, r = n // 128 * 128, n % 128
        why = ("staircase kernel on %d" % n0 if n0 else "no whole tile") + (", border of %d" % r if r else "")
        rows.append(_row("potri", "F1", n, why + "; even lda", pads=(2 - n % 2, 0)))
        rows.append(_row("potri", "F1", n, why + "; odd lda", pads=(1 + n % 2, 0)))
    # cap_dpotri inverts into its own scratch with an even leading dimension, so no lda reaches cap_dlauum's copy route; a work pointer
    # that is only 8-byte aligned does
    rows.append(_row("potri", "F1", 129, "work 8-byte aligned only: cap_dlauum's copy route", pads=(1, 0), woff=1))
    return rows


TRTRI_CASES = _trtri_rows()
TRSM_CASES = _trsm_rows()
POTRS_CASES = _potrs_rows()
POTRI_CASES = _potri_rows()
CASES = TRTRI_CASES + TRSM_CASES + POTRS_CASES + POTRI_CASES
SEED = {c.id: 7000 + i for i, c in enumerate(CASES)}
RECOVERY_CASE = next(c for c in POTRS_CASES if c.n == 1153 and c.other == 5)
AGREEMENT_CASE = next(c for c in POTRS_CASES if c.n == 300 and c.other == 9)


# ------------------------------------------------------------------------------------------------------------------------ the operands
def classes(n):
    return 2 - ((n - 1 - np.arange(n)) % 3)


def _square_of_n(N, cls):
    """N @ N for the three-class N: only (class 0, class 2) entries, through class 1"""
    c0, c1, c2 = (np.flatnonzero(cls == k) for k in range(3))
    N2 = np.zeros_like(N)
    if c0.size and c1.size and c2.size:
        N2[np.ix_(c0, c2)] = N[np.ix_(c0, c1)] @ N[np.ix_(c1, c2)]
    return N2


@functools.lru_cache(maxsize=8)
def family(fam, n, signed):
    """(T, Tinv, N or None, d) of a family at size n, exact, without the NaN triangle; cached: the arrays are shared, never written"""
    rng = np.random.default_rng([{"F1": 1, "F2": 2, "F2i": 2}[fam], n, int(signed)])
    d = DIAG[rng.integers(0, 4, size=n)]
    if signed:
        d = d * rng.choice([-1.0, 1.0], size=n)
    if fam == "F1":
        cls = classes(n)
        allowed = np.triu(cls[:, None] < cls[None, :], 1)
        N = np.where(allowed, rng.choice([-2.0, -1.0, 1.0, 2.0], size=(n, n)), 0.0)
        T = d[:, None] * (np.eye(n) + N)
        Tinv = (np.eye(n) - N + _square_of_n(N, cls)) / d[None, :]
        if n <= 300:
            assert not np.any(N @ N @ N) and np.array_equal(N @ N, _square_of_n(N, cls)), "N^3 = 0, and N^2 by classes"
    else:
        s1, s2 = rng.choice([-1.0, 1.0], size=n), rng.choice([-1.0, 1.0], size=n)
        N = None
        T = (d * s1)[:, None] * np.triu(np.ones((n, n))) * s2[None, :]
        Tinv = s2[:, None] * (np.eye(n) - np.eye(n, k=1)) * (s1 / d)[None, :]
        if fam == "F2i":
            T, Tinv = Tinv, T
    for a in (T, Tinv, d) + ((N,) if N is not None else ()):
        a.setflags(write=False)
    if n <= 2304:                         # (n = 4224: by diagonal blocks, as the solve uses them - _check_blocks)
        _check_inverse(T, Tinv)
    return T, Tinv, N, d


def _check_inverse(T, Tinv):
    n = T.shape[0]
    assert np.abs(T).dot(np.abs(Tinv)).max() * 8 < LIMIT          # (the float64 products below are exact)
    assert np.array_equal(T @ Tinv, np.eye(n)) and np.array_equal(Tinv @ T, np.eye(n)), "T Tinv == I == Tinv T"
    assert not np.any(np.tril(T, -1)) and not np.any(np.tril(Tinv, -1)) and np.all(np.diagonal(T) != 0)


def stored(T):
    """the operand as a caller stores it: NaN in the strictly lower triangle"""
    S = T.copy()
    S[np.tril_indices(T.shape[0], -1)] = NAN
    return S


def rhs(c):
    """the integer right-hand sides of a row: n x other (LEFT, POTRS) or other x n (RIGHT)"""
    rng = np.random.default_rng(SEED.get(c.id, 6999))          # (rows outside the table: the helpers' own tests)
    shape = (c.other, c.n) if c.op == "trsm" and c.form[0] == "R" else (c.n, c.other)
    return RHS_VALUES[rng.integers(0, len(RHS_VALUES), size=shape)]


def operands(c):
    """{"T": exact T, "Tinv", "B" (if any)} of a row"""
    T, Tinv, _, _ = family(c.fam, c.n, c.signed)
    ops = {"T": T, "Tinv": Tinv}
    if c.op in ("trsm", "potrs"):
        ops["B"] = rhs(c)
    return ops


def lds(c):
    ld = {"T": max(c.n, 1) + c.pads[0]}
    if c.op in ("trsm", "potrs"):
        rows = c.other if c.op == "trsm" and c.form[0] == "R" else c.n
        ld["B"] = max(rows, 1) + c.pads[1]
    return ld


# ---------------------------------------------------------------------------------------------------------------------- the references
def reference(c, ops):
    """the matrix the call must leave in its output (A for TRTRI / POTRI with NaN below the diagonal, B for TRSM / POTRS)"""
    T, Tinv = ops["T"], ops["Tinv"]
    if c.op == "trtri":
        return stored(Tinv)
    if c.op == "potri":
        return stored(np.triu(Tinv @ Tinv.T))
    B = ops["B"]
    if c.op == "potrs":
        return Tinv @ (Tinv.T @ B)
    op = Tinv.T if c.form[1] == "T" else Tinv
    return c.alpha * (op @ B if c.form[0] == "L" else B @ op)


def positive_zero(a):
    """-0.0 -> +0.0 (an alpha = -1 product of exact zeros is legitimately -0.0), nothing else changes: NaNs keep their bits"""
    a = np.array(a, dtype=np.float64, copy=True)
    a[a == 0.0] = 0.0
    return a


# ---------------------------------------------------------------------------------------------------------- the premise of exactness
def _inverse_route_bound(T, Tinv, tb):
    """max entry of |Tinv| |T| |Tinv| (and of |T| |Tinv|, |Tinv| |T|) over the diagonal blocks of width tb that a route inverts"""
    worst = 0.0
    n = T.shape[0]
    for o in range(0, n, tb):
        t, ti = np.abs(T[o:o + tb, o:o + tb]), np.abs(Tinv[o:o + tb, o:o + tb])
        tti = t @ ti
        worst = max(worst, tti.max(), (ti @ t).max(), (ti @ tti).max())
    return worst


def _check_blocks(T, Tinv, tb):
    """T^-1's diagonal blocks invert T's: what a block substitution relies on (used where the whole matrix is too large to multiply twice)"""
    for o in range(0, T.shape[0], tb):
        _check_inverse(T[o:o + tb, o:o + tb], Tinv[o:o + tb, o:o + tb])


def _comparison(N, d):
    """M^-1 = (I + |N| + |N|^2) |D|^-1 of the comparison matrix M = |D| (I - |N|)"""
    n = d.size
    aN = np.abs(N)
    return (np.eye(n) + aN + _square_of_n(aN, classes(n))) / np.abs(d)[None, :]


def _substitution_bound(Mi, Tsu, B, trans):
    """(bound on every intermediate of a block substitution with op(T) on right-hand sides of magnitude B, the comparison solution)"""
    if trans:
        Mi, Tsu = Mi.T, Tsu.T
    Xc = Mi @ B
    return max(Xc.max(), (B + Tsu @ Xc).max()), Xc


def bounds(c):
    """{name: bound x 2^fraction bits} of every product the route of a row forms; all must be < 2^53"""
    T, Tinv, N, d = family(c.fam, c.n, c.signed)
    out = {}
    if c.op in ("trtri", "potri"):
        out["inverse |Tinv||T||Tinv| x 2^5"] = _inverse_route_bound(T, Tinv, max(c.n, 1)) * 32
        if c.op == "potri":
            out["product |Tinv||Tinv|^T x 2^4"] = (np.abs(Tinv) @ np.abs(Tinv).T).max() * 16
        return out
    assert c.fam == "F1", "the comparison-matrix argument is about F1"
    tb = POTRS_BLOCK if c.op == "potrs" and c.other <= 16 else trsm_block(c.n)
    out["block inverses |Tinv||T||Tinv| x 2^5"] = _inverse_route_bound(T, Tinv, tb) * 32
    Mi, Tsu = _comparison(N, d), np.abs(np.triu(T, 1))
    assert np.all(Mi >= np.abs(Tinv))
    B = np.abs(rhs(c))
    if c.op == "trsm":
        if c.form[0] == "R":              # X op(T) = alpha B  <=>  op(T)^T X^T = alpha B^T
            b, _ = _substitution_bound(Mi, Tsu, abs(c.alpha) * B.T, c.form[1] == "N")
        else:
            b, _ = _substitution_bound(Mi, Tsu, abs(c.alpha) * B, c.form[1] == "T")
        out["substitution (comparison matrix) x 2^4"] = b * 16          # alpha B: 1 bit, T^-1: 2, T X: 1
        return out
    bf, Yc = _substitution_bound(Mi, Tsu, B, True)
    bb, _ = _substitution_bound(Mi, Tsu, Yc, False)
    out["two substitutions (comparison matrix) x 2^5"] = max(bf, bb) * 32   # Y: 2 bits, X: 4, R X: 5
    return out


def check_premise(c):
    """the exactness premise of a row (and, where family() could not afford it, that the diagonal blocks of T^-1 invert those of T)"""
    b = bounds(c)
    for name, v in b.items():
        assert np.isfinite(v) and v < LIMIT, "%s: %s = 2^%.1f is not below 2^53" % (c.id, name, np.log2(v))
    if c.n > 2304:
        T, Tinv, _, _ = family(c.fam, c.n, c.signed)
        _check_blocks(T, Tinv, POTRS_BLOCK)
    return b


# ------------------------------------------------------------------------------------------------- refusals (no launch, nothing touched)
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 4
LOWER, UPPER = 0, 1
# (entry, what is wrong, expected status); the callers fill in valid values for everything that is not named
REFUSALS = [
    ("trtri", "lower", ERR_UNSUPPORTED), ("trtri", "n<0", ERR_ARG), ("trtri", "ld<n", ERR_ARG), ("trtri", "A=NULL", ERR_ARG), ("trtri", "work=NULL", ERR_ARG),
    ("trsm", "lower", ERR_UNSUPPORTED), ("trsm", "m<0", ERR_ARG), ("trsm", "n<0", ERR_ARG), ("trsm", "ldt<td", ERR_ARG), ("trsm", "ldb<m", ERR_ARG),
    ("trsm", "T=NULL", ERR_ARG), ("trsm", "B=NULL", ERR_ARG), ("trsm", "work=NULL", ERR_ARG),
    ("potrs", "lower", ERR_UNSUPPORTED), ("potrs", "n<0", ERR_ARG), ("potrs", "nrhs<0", ERR_ARG), ("potrs", "ldr<n", ERR_ARG), ("potrs", "ldb<n", ERR_ARG),
    ("potrs", "R=NULL", ERR_ARG), ("potrs", "B=NULL", ERR_ARG), ("potrs", "work=NULL", ERR_ARG),
    ("potri", "lower", ERR_UNSUPPORTED), ("potri", "n<0", ERR_ARG), ("potri", "ld<n", ERR_ARG), ("potri", "A=NULL", ERR_ARG), ("potri", "work=NULL", ERR_ARG),
]
REFUSAL_N, REFUSAL_NRHS = 40, 3


def refusal_call(L, entry, what, a, b, work, stream=None):
    """one refused call: `a` the triangle (ld n + 2), `b` the right-hand sides (ld n + 2), `work` - device addresses (int); -> status"""
    n, r, ld = REFUSAL_N, REFUSAL_NRHS, REFUSAL_N + 2
    uplo = LOWER if what == "lower" else UPPER
    null = lambda p, name: None if what == name + "=NULL" else p          # noqa: E731
    if entry in ("trtri", "potri"):
        f = L.cap_dtrtri if entry == "trtri" else L.cap_dpotri
        return f(uplo, -1 if what == "n<0" else n, null(a, "A"), n - 1 if what == "ld<n" else ld, null(work, "work"), stream)
    if entry == "trsm":
        return L.cap_dtrsm(0, uplo, 0, -1 if what == "m<0" else n, -1 if what == "n<0" else r, 2.0, null(a, "T"), n - 1 if what == "ldt<td" else ld,
                           null(b, "B"), n - 1 if what == "ldb<m" else ld, null(work, "work"), stream)
    return L.cap_dpotrs(uplo, -1 if what == "n<0" else n, -1 if what == "nrhs<0" else r, null(a, "R"), n - 1 if what == "ldr<n" else ld,
                        null(b, "B"), n - 1 if what == "ldb<n" else ld, null(work, "work"), stream)


# --------------------------------------------------------------------------------------------------------------------------- the calls
def work_size(L, c):
    if c.op == "trtri":
        return int(L.cap_dtrtri_work_size(c.n))
    if c.op == "potri":
        return int(L.cap_dpotri_work_size(c.n))
    if c.op == "potrs":
        return int(L.cap_dpotrs_work_size(c.n, c.other))
    side = 0 if c.form[0] == "L" else 1
    m, n = (c.n, c.other) if side == 0 else (c.other, c.n)
    return int(L.cap_dtrsm_work_size(side, m, n))


def call(L, c, t, b, work, ld, stream=None):
    """the C ABI call of a row on device addresses (int) -> status"""
    if c.op == "trtri":
        return L.cap_dtrtri(UPPER, c.n, t, ld["T"], work, stream)
    if c.op == "potri":
        return L.cap_dpotri(UPPER, c.n, t, ld["T"], work, stream)
    if c.op == "potrs":
        return L.cap_dpotrs(UPPER, c.n, c.other, t, ld["T"], b, ld["B"], work, stream)
    side = 0 if c.form[0] == "L" else 1
    m, n = (c.n, c.other) if side == 0 else (c.other, c.n)
    return L.cap_dtrsm(side, UPPER, 1 if c.form[1] == "T" else 0, m, n, c.alpha, t, ld["T"], b, ld["B"], work, stream)
