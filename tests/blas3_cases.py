"""One case table for the fp64 GEMM / SYRK / TRMM kernel paths of csrc/gemm.hip, shared by tests/test_blas3_paths.py (no GPU: every row is
driven through the library's own object files on the recording stand-in, which shows the kernel instance each row launches) and
tests/test_gpu_blas3_exact.py (-m gpu: the same rows on the device).  Plain data and NumPy helpers, nothing of the GPU is imported here.

EXACT RESULTS.  Every operand entry is a nonzero integer of {+-1, +-2, +-3}, alpha and beta come from {-1, 1, 2, 0.5, -3, 0} and k <= 6000:
every partial sum of a product, in ANY order, is an integer of magnitude <= 9 * 6000 = 5.4e4, alpha = 0.5 makes it a half-integer, beta * C
adds at most 9 - all exactly representable far below 2^53.  A float64 NumPy product of the same arrays therefore IS the result, whatever
order a kernel sums in, and the device must reproduce it bit for bit: the comparisons are on view(int64), there is no tolerance anywhere.
exact_reference() asserts the premise (|ref| < 2^53) instead of assuming it.

FORBIDDEN REGIONS ARE NaN.  The rows of every buffer between the matrix and its leading dimension, the strictly lower triangle of a TRMM
operand, the triangle of a SYRK C the call must not touch and, for beta == 0, the whole of C hold NaNs; the comparison covers the whole
buffer, so a NaN that moved, vanished or leaked into a result is a failure like a wrong element.

A row names the kernel instance(s) it must launch, in launch order, as `name<template arguments>`:
    dgemm_small_kernel<TA,TB>   dgemm_kernel<A_KC,B_KC,EDGE,TAG>   dgemm_tn_dma_kernel<TAG,A_MC,DIAG,BUF,SKIP>
    dgemm_tn_skinny_kernel<F32>   dgemm_nn_skinny_kernel<F32>   scale_kernel   splitk_reduce_kernel
and the run-time modes that do not show in the name: split-K (`ksplit`) and the XCD band mapping of the products with a triangular
operand (`band` = (stm, stn), the supertile shape; None = square supertiles)."""
import numpy as np

VALUES = np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])
SCALARS = (-1.0, 1.0, 2.0, 0.5, -3.0, 0.0)
NAN = np.float64("nan")

SCALE = "scale_kernel"
REDUCE = "splitk_reduce_kernel"
TN_SKINNY = "dgemm_tn_skinny_kernel<0>"
NN_SKINNY = "dgemm_nn_skinny_kernel<0>"


def SMALL(ta, tb):
    return "dgemm_small_kernel<%d,%d>" % (ta, tb)


def GEN(a_kc, b_kc, edge):
    """the register-staged tile kernel: operand A / B K-contiguous, EDGE 0 aligned / 1 ragged vector loads / 2 scalar loads"""
    return "dgemm_kernel<%d,%d,%d,0>" % (a_kc, b_kc, edge)


def DMA(a_mc, buf, skip):
    """the LDS-DMA tile kernel: A M-contiguous (the NN form), buffer-addressed DMA, 16 x 16 block skipping"""
    return "dgemm_tn_dma_kernel<0,%d,0,%d,%d>" % (a_mc, buf, skip)


FORMS = ("TN", "NN", "TT", "NT")          # (ta, tb) = (1, 0), (0, 0), (1, 1), (0, 1) - the order of test_gpu_operators.py


def generic(edge, split=False):
    """all four transposes on dgemm_kernel (a_kc = ta, b_kc = not tb)"""
    tail = [REDUCE] if split else []
    return {"TN": [GEN(1, 1, edge)] + tail, "NN": [GEN(0, 1, edge)] + tail, "TT": [GEN(1, 0, edge)] + tail, "NT": [GEN(0, 0, edge)] + tail}


# aligned shapes: TN and NN have LDS-DMA kernels, the forms with a transposed B stay on the register-staged kernel
ALIGNED = {"TN": [DMA(0, 1, 0)], "NN": [DMA(1, 0, 0)], "TT": [GEN(1, 0, 0)], "NT": [GEN(0, 0, 0)]}
# ... under split-K only TN keeps its LDS-DMA kernel (the NN one has no split-K epilogue)
ALIGNED_SPLIT = {"TN": [DMA(0, 1, 0), REDUCE], "NN": [GEN(0, 1, 0), REDUCE], "TT": [GEN(1, 0, 0), REDUCE], "NT": [GEN(0, 0, 0), REDUCE]}

GEMM_AB = ((-1.0, 1.0), (2.0, 0.0), (0.5, -3.0))      # beta == 1: the atomic epilogue of the LDS-DMA kernels on the device
SYRK_AB = ((-1.0, 1.0), (1.0, 0.0), (0.5, -3.0))
TRMM_ALPHA = (1.0, -1.0, 0.5)


class Case(dict):
    """a row: op, form, m, n, k, pads (rows between a matrix and its leading dimension: A / T, B, C), offs (element offset of the A and the B
    pointer inside their buffers), ab [(alpha, beta)], kernels [instances in launch order], ksplit, band, why"""
    __getattr__ = dict.__getitem__

    @property
    def id(self):
        if "which" in self:
            return "%s-%s-%dx%dx%d-ld%s%d" % (self.op, self.form, self.m, self.n, self.k, self.which, self.ld)
        extra = "".join("-%s%d" % (w, v) for w, v in (("pad", max(self.pads)), ("offA", self.offs[0]), ("offB", self.offs[1])) if v)
        return "%s-%s-%dx%dx%d%s" % (self.op, self.form, self.m, self.n, self.k, extra)


def _gemm_rows():
    rows = []
    small = {"TN": [SMALL(1, 0)], "NN": [SMALL(0, 0)], "TT": [SMALL(1, 1)], "NT": [SMALL(0, 1)]}

    def add(m, n, k, kernels, why, pads=(0, 0, 0), offs=(0, 0), forms=FORMS, ab=GEMM_AB):
        for f in forms:
            rows.append(Case(op="gemm", form=f, m=m, n=n, k=k, pads=pads, offs=offs, ab=ab, kernels=list(kernels[f]), ksplit=REDUCE in kernels[f],
                             band=None, why=why))

    # the latency kernel of the little products (m, n <= 512, k <= 1024, m n <= 65536): 64 x 64 tiles, three of them ragged, three K chunks
    add(129, 257, 130, small, "small kernel, odd everything", pads=(1, 1, 1))
    # aligned interior, odd and even numbers of K tiles (1, 3, 4): the software pipeline's prologue, loop and tail
    add(384, 256, 16, ALIGNED, "aligned, one K tile", pads=(0, 0, 2))
    add(384, 256, 48, ALIGNED, "aligned, three K tiles")
    add(256, 384, 64, ALIGNED, "aligned, four K tiles", pads=(2, 2, 2))
    # EDGE == 1: every leading dimension, k and the outer extents even, extents ragged
    add(258, 386, 66, generic(1), "ragged, vector loads", pads=(2, 2, 2))
    add(130, 600, 34, generic(1), "ragged, vector loads, n > 512")
    # EDGE == 2: odd geometry / a pointer that is only 8-byte aligned
    add(257, 385, 65, generic(2), "odd extents and leading dimensions, scalar loads", pads=(2, 2, 2))
    add(256, 384, 64, generic(2), "aligned extents, A pointer 8-byte aligned only", offs=(1, 0))
    add(256, 384, 64, generic(2), "aligned extents, B pointer 8-byte aligned only", offs=(0, 1))
    # partial supertiles (2 x 2 tiles): 5 x 3 tiles; one row / one column of C
    add(640, 384, 32, ALIGNED, "5 x 3 tiles, partial supertiles")
    add(1, 600, 17, generic(2), "one row of C", pads=(1, 1, 1))
    add(600, 1, 17, generic(2), "one column of C", pads=(1, 1, 1))
    # split-K: fewer than 128 tiles and k >= 4096
    add(256, 256, 4096, ALIGNED_SPLIT, "split-K, equal slices")
    add(256, 256, 5008, ALIGNED_SPLIT, "split-K, last slice shorter than kchunk")
    add(130, 258, 4100, generic(1, split=True), "split-K on the ragged vector path", pads=(2, 2, 2))
    add(129, 257, 4099, generic(2, split=True), "split-K on the scalar path", pads=(2, 2, 2))
    # degenerate: C = beta C
    add(300, 300, 0, {"NN": [SCALE]}, "k == 0", forms=("NN",), ab=((2.0, 0.0), (2.0, -3.0)), pads=(0, 0, 1))
    add(300, 300, 8, {"NN": [SCALE]}, "alpha == 0", forms=("NN",), ab=((0.0, 0.0), (0.0, -3.0)), pads=(0, 0, 1))
    # a few right-hand sides against a big operand (m >= 1024, n <= 8, B not transposed, k % 8 == 0; TN: m % 16 == 0, NN: m % 64 == 0);
    # a transposed B never qualifies and takes the tile kernels (an odd ldb = n + pad: scalar loads)
    add(2048, 8, 1024, {"TN": [TN_SKINNY], "NN": [NN_SKINNY], "TT": [GEN(1, 0, 1)], "NT": [GEN(0, 0, 1)]}, "skinny")
    add(1088, 3, 4104, {"TN": [TN_SKINNY], "NN": [NN_SKINNY], "TT": [GEN(1, 0, 2), REDUCE], "NT": [GEN(0, 0, 2), REDUCE]}, "skinny, padded", pads=(2, 2, 2))
    add(4160, 5, 1000, {"TN": [TN_SKINNY], "NN": [NN_SKINNY], "TT": [GEN(1, 0, 2)], "NT": [GEN(0, 0, 2)]}, "skinny")
    add(1024, 1, 64, {"TN": [TN_SKINNY], "NN": [NN_SKINNY], "TT": [GEN(1, 0, 2)], "NT": [GEN(0, 0, 2)]}, "skinny, one right-hand side")
    add(1024, 8, 8, {"TN": [TN_SKINNY], "NN": [NN_SKINNY], "TT": [GEN(1, 0, 1)], "NT": [GEN(0, 0, 1)]}, "skinny, smallest k")
    add(1024, 8, 12, generic(1), "the skinny launcher declines k % 8 != 0")
    add(1032, 4, 16, generic(1), "the skinny launcher declines m % 16 != 0 (TN) and m % 64 != 0 (NN)")
    return rows


def _syrk_rows():
    rows = []

    def add(n, k, upper_trans, lower_trans, notrans, why, pad=0):
        for uplo in ("U", "L"):
            for trans in ("T", "N"):
                kernels = list(notrans if trans == "N" else (upper_trans if uplo == "U" else lower_trans))
                rows.append(Case(op="syrk", form=uplo + trans, m=n, n=n, k=k, pads=(pad, 0, pad), offs=(0, 0), ab=SYRK_AB, kernels=kernels,
                                 ksplit=REDUCE in kernels, band=None, why=why))

    # Trans is the TN form (LDS-DMA when aligned; upper with <= 8 tile rows: the instance that skips the dead 16 x 16 blocks of the diagonal
    # tiles), NoTrans the NT form (register-staged).  Square tile spaces: the supertile triangle is enumerated.
    add(130, 512, [SMALL(1, 0)], [SMALL(1, 0)], [SMALL(0, 1)], "small kernel under a triangle mask", pad=1)
    add(384, 16, [DMA(0, 1, 1)], [DMA(0, 1, 0)], [GEN(0, 0, 0)], "3 tile rows: skipping instance for upper", pad=2)
    add(384, 80, [DMA(0, 1, 1)], [DMA(0, 1, 0)], [GEN(0, 0, 0)], "3 tile rows, five K tiles")
    add(1152, 32, [DMA(0, 1, 0)], [DMA(0, 1, 0)], [GEN(0, 0, 0)], "9 tile rows: no skipping; 5 x 5 supertile triangle, ragged last supertile")
    add(770, 34, [GEN(1, 1, 1)], [GEN(1, 1, 1)], [GEN(0, 0, 1)], "ragged, vector loads", pad=2)
    add(1000, 77, [GEN(1, 1, 2)], [GEN(1, 1, 2)], [GEN(0, 0, 2)], "odd k, scalar loads")
    add(256, 6000, [DMA(0, 1, 1), REDUCE], [DMA(0, 1, 0), REDUCE], [GEN(0, 0, 0), REDUCE], "split-K under a triangle mask")
    return rows


def _trmm_rows():
    rows = []
    # (side, trans) -> hint tag of the launcher: LT 16 (aupt), LN 32 (aupn), RN 8 (bupper), RT 0 (none).  B := alpha op(T) B or alpha B op(T).

    def add(m, n, lt, ln, rn, rt, why, band_ln=None, band_rn=None, pad=2):
        for form, kernels, band in (("LT", lt, None), ("LN", ln, band_ln), ("RN", rn, band_rn), ("RT", rt, None)):
            td = m if form[0] == "L" else n
            rows.append(Case(op="trmm", form=form, m=m, n=n, k=td, pads=(pad, pad, 0), offs=(0, 0), ab=tuple((a, 0.0) for a in TRMM_ALPHA),
                             kernels=[kernels], ksplit=False, band=band, why=why))

    HINTED = dict(lt=DMA(0, 1, 1), ln=DMA(1, 0, 1), rn=DMA(1, 0, 1), rt=GEN(0, 0, 0))
    # band mapping (supertiles of 8 x 8 tiles and at least 64 tiles): LN walks bands of tile columns, RN bands of tile rows
    add(1024, 1024, why="8 x 8 tiles: band mapping for LN and RN", band_ln=(8, 1), band_rn=(1, 8), **HINTED)
    add(1152, 1024, why="9 x 8 tiles: band mapping, 8 does not divide the tile count", band_ln=(9, 1), band_rn=(1, 8), **HINTED)
    add(1024, 1152, why="8 x 9 tiles: band mapping, 8 does not divide the tile count", band_ln=(8, 1), band_rn=(1, 9), **HINTED)
    add(640, 384, why="hinted, below the band threshold", **HINTED)
    # ragged shapes fall to dgemm_kernel, which ignores the hints (the copied triangle carries explicit zeros)
    add(1000, 700, GEN(1, 1, 1), GEN(0, 1, 1), GEN(0, 1, 1), GEN(0, 0, 1), "even triangle, ragged: vector loads")
    add(1001, 333, GEN(1, 1, 2), GEN(0, 1, 2), GEN(0, 1, 2), GEN(0, 0, 2), "odd triangle: scalar loads", pad=1)
    add(333, 1001, GEN(1, 1, 2), GEN(0, 1, 2), GEN(0, 1, 2), GEN(0, 0, 2), "odd triangle: scalar loads", pad=1)
    return rows


GEMM_CASES = _gemm_rows()
SYRK_CASES = _syrk_rows()
TRMM_CASES = _trmm_rows()
CASES = GEMM_CASES + SYRK_CASES + TRMM_CASES

# Large pitch: C[128 x 128] = alpha A^T B + beta C, k = 1040 (beyond the small kernel), one operand with a leading dimension at the limit of
# the buffer-addressed LDS-DMA: usebuf needs 128 * ld * 8 + k * 8 < 0xfffffff0 for both operands.  About 4.3 GB of address space per case,
# of which only the k leading rows of each of the 128 columns are ever read.
BIG_M, BIG_K = 128, 1040
BIG_LIMIT = 0xfffffff0
BIG_LD_LAST = ((BIG_LIMIT - 1 - BIG_K * 8) // (128 * 8)) & ~1          # the largest even ld that still fits: the last legal buffer offset
BIG_LD_FIRST = BIG_LD_LAST + 2                                          # the smallest even ld that does not: the BUF == false instance
assert 128 * BIG_LD_LAST * 8 + BIG_K * 8 < BIG_LIMIT <= 128 * BIG_LD_FIRST * 8 + BIG_K * 8
BIG_CASES = [Case(op="gemm", form="TN", m=BIG_M, n=BIG_M, k=BIG_K, which=which, ld=ld, pads=(0, 0, 0), offs=(0, 0), ab=GEMM_AB, kernels=[DMA(0, buf, 0)], ksplit=False,
                  band=None, why="large pitch on %s, %s" % (which, "last legal buffer offset" if buf else "64-bit addresses"))
             for which in ("A", "B") for ld, buf in ((BIG_LD_LAST, 1), (BIG_LD_FIRST, 0))]
# ... and the one instance only a SYRK with such a pitch reaches: block skipping (upper, one tile row) without the buffer-addressed DMA
BIG_CASES.append(Case(op="syrk", form="UT", m=BIG_M, n=BIG_M, k=BIG_K, which="A", ld=BIG_LD_FIRST, pads=(0, 0, 0), offs=(0, 0), ab=SYRK_AB, kernels=[DMA(0, 0, 1)],
                      ksplit=False, band=None, why="large pitch under an upper mask: skipping instance on 64-bit addresses"))


# ------------------------------------------------------------------------------------------------------------------ operands and references
def ints(rng, shape):
    """nonzero integers of {+-1, +-2, +-3} as float64"""
    return VALUES[rng.integers(0, len(VALUES), size=shape)]


def operand_shapes(c):
    """stored (rows, cols) of the operands of a row, in call order"""
    if c.op == "gemm":
        return {"A": (c.k, c.m) if c.form[0] == "T" else (c.m, c.k), "B": (c.n, c.k) if c.form[1] == "T" else (c.k, c.n), "C": (c.m, c.n)}
    if c.op == "syrk":
        return {"A": (c.k, c.n) if c.form[1] == "T" else (c.n, c.k), "C": (c.n, c.n)}
    return {"T": (c.k, c.k), "B": (c.m, c.n)}


def operands(c, seed):
    """fresh logical operands of a row; T of a TRMM row is returned WITH its NaN lower triangle (as stored)"""
    rng = np.random.default_rng(seed)
    ops = {name: ints(rng, shape) for name, shape in operand_shapes(c).items()}
    if c.op == "trmm":
        ops["T"][np.tril_indices(c.k, -1)] = NAN
    return ops


def exact_reference(c, ops, alpha, beta):
    """the matrix the call must leave in its output (C, or B for TRMM), NaN where the call must not write"""
    assert alpha in SCALARS and beta in SCALARS and c.k <= 6000
    if c.op == "gemm":
        a = ops["A"].T if c.form[0] == "T" else ops["A"]
        b = ops["B"].T if c.form[1] == "T" else ops["B"]
        prod, c0, keep = a @ b, ops["C"], None
    elif c.op == "syrk":
        a = ops["A"].T if c.form[1] == "T" else ops["A"]
        prod, c0 = a @ a.T, ops["C"]
        keep = np.tril(np.ones((c.n, c.n), dtype=bool), -1) if c.form[0] == "U" else np.triu(np.ones((c.n, c.n), dtype=bool), 1)
    else:
        t = np.triu(np.nan_to_num(ops["T"], nan=0.0))
        assert np.count_nonzero(np.triu(t)) == c.k * (c.k + 1) // 2, "no zero in the stored triangle"
        t = t.T if c.form[1] == "T" else t
        prod, c0, keep = (t @ ops["B"] if c.form[0] == "L" else ops["B"] @ t), None, None
    ref = alpha * prod if alpha != 0.0 else np.zeros_like(prod)          # (BLAS: alpha == 0 does not reference the product - no -0.0 from it)
    if beta != 0.0:
        ref = ref + beta * c0
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() < 2.0 ** 53 and np.array_equal(ref * 2.0, np.rint(ref * 2.0)), "the premise of exactness"
    if keep is not None:
        ref[keep] = NAN
    return ref


def initial_output(c, ops, beta):
    """what the output buffer's matrix holds before the call: all NaN for beta == 0 (BLAS: C is not read), else the integers with NaN in the
    triangle a SYRK must not touch; B itself for TRMM"""
    if c.op == "trmm":
        return ops["B"].copy()
    c0 = ops["C"].copy()
    if beta == 0.0:
        c0[:] = NAN
    elif c.op == "syrk":
        c0[np.tril_indices(c.n, -1) if c.form[0] == "U" else np.triu_indices(c.n, 1)] = NAN
    return c0


def lds(c):
    """leading dimensions of the stored operands: rows + pad (at least 1)"""
    sh = operand_shapes(c)
    pads = dict(zip(("T", "B", "C") if c.op == "trmm" else ("A", "B", "C"), c.pads))
    return {name: max(rows, 1) + pads[name] for name, (rows, _) in sh.items()}


def place(mat, ld, off=0):
    """column-major image of `mat` with leading dimension ld behind `off` leading elements; everything that is not the matrix is NaN"""
    rows, cols = mat.shape
    flat = np.full(off + ld * max(cols, 1), NAN)
    flat[off:off + ld * cols].reshape(cols, ld)[:, :rows] = mat.T
    return flat


def same_bits(got, want):
    """bit-for-bit equality of two float64 arrays (NaN patterns included)"""
    got = np.ascontiguousarray(got, dtype=np.float64); want = np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def describe_mismatch(got, want, ld, off=0):
    """which elements differ: count and the bounding rows / columns (identifies the tile, the 16 x 16 block and, by the size of the error, the K step)"""
    g = np.ascontiguousarray(got, dtype=np.float64).view(np.int64); w = np.ascontiguousarray(want, dtype=np.float64).view(np.int64)
    if g.shape != w.shape:
        return "shapes differ: %s / %s" % (g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return "equal"
    if bad[0] < off:
        return "the %d elements in front of the pointer changed" % off
    r, col = (bad - off) % ld, (bad - off) // ld
    i = bad[0]
    return "%d elements differ, rows %d..%d, columns %d..%d; first at (%d, %d): got %r, expected %r" % (
        bad.size, r.min(), r.max(), col.min(), col.max(), r[0], col[0], float(np.asarray(got).ravel()[i]), float(np.asarray(want).ravel()[i]))


CAP_TRANS = {"N": 0, "T": 1}
