"""Size lists, layouts and operands for the variable-size batched Cholesky (cap_vbatch_plan_*, cap_dpotrf_vbatched, cap_dpotrs_vbatched,
cap_dpotri_vbatched), shared by tests/test_vbatched_cases.py, tests/test_vbatched_abi.py (no GPU) and tests/test_gpu_vbatched*.py (-m gpu).
NumPy only, nothing of torch or the GPU is imported here.

SIZE LISTS are built from potri_batched_cases.SMALL_N / LARGE_N, the sizes at which the exact families F1 / F2 / F2i are known to satisfy
their exactness premise (block() asserts it per block).  LAYOUTS: how the blocks lie in the flat buffer.  A layout is (ld, offsets, total)
plus what is handed to cap_vbatch_plan_create (None where the plan's default is the layout).

THE FLAT BUFFER of a test starts as NaNs with a payload of their own per element; the upper triangles (or, for fill = 1, the windows with
NaN strictly lower triangles) of the blocks are laid into it, a guard of NaNs follows the last block.  `written` masks say which elements
a call may write; everything else is compared as int64 afterwards."""
import numpy as np

from tests import potri_batched_cases as P

CLASS_NAMES = ("NP8", "NP16", "NP32", "NP64", "NBLK2", "NBLK3", "NBLK4")
CLASS_MAX = (8, 16, 32, 64, 128, 192, 256)
GUARD = 16


def class_of(n):
    assert 1 <= n <= 256
    return next(c for c, m in enumerate(CLASS_MAX) if n <= m)


def _every():
    sizes = list(P.SMALL_N) + list(P.LARGE_N) + [0, 0]
    np.random.default_rng(2201).shuffle(sizes)
    return tuple(int(x) for x in sizes)


EVERY = _every()
WAVES = tuple((5, 6, 7, 8)[i % 4] for i in range(70)) + (9, 200)
LONE = {n: (n,) for n in (1, 64, 65, 256)}
ONE_CLASS = (130,) * 5
EDGES = tuple(n for _ in range(3) for n in (33, 64, 65, 128, 129, 192, 193))
LISTS = {"EVERY": EVERY, "WAVES": WAVES, "ONE_CLASS": ONE_CLASS, "EDGES": EDGES}
LISTS.update({"LONE%d" % n: s for n, s in LONE.items()})
LAYOUTS = ("packed", "ld+3", "gaps", "reverse")
FAMILIES = P.FAMILIES


def expected_lists(sizes):
    """the seven class lists a plan must hold: the block indices of each class, stably sorted by n"""
    out = [[] for _ in CLASS_MAX]
    for i, n in enumerate(sizes):
        if n > 0:
            out[class_of(n)].append(i)
    return [sorted(l, key=lambda i: sizes[i]) for l in out]           # sorted() is stable


class Layout:
    """ld, offsets (NumPy int64, batch order), total = elements spanned; ld_arg / off_arg: what cap_vbatch_plan_create gets (None = NULL)"""

    def __init__(self, sizes, kind):
        n = np.asarray(sizes, dtype=np.int64)
        self.sizes, self.kind, self.batch = n, kind, len(n)
        if kind == "packed":
            self.ld = np.maximum(n, 1)
            self.ld_arg = self.off_arg = None
        elif kind == "ld+3":
            self.ld = n + 3
            self.ld_arg, self.off_arg = self.ld, None
        elif kind == "gaps":
            self.ld = np.maximum(n, 1)
            self.ld_arg = None
        elif kind == "reverse":
            self.ld = n + 1
            self.ld_arg = self.ld
        else:
            raise ValueError(kind)
        span = self.ld * n
        if kind == "gaps":
            self.off = np.concatenate([[0], np.cumsum(span + 5)[:-1]]).astype(np.int64) + 2
            self.off_arg = self.off
        elif kind == "reverse":             # block 0 lies last
            rev = np.concatenate([[0], np.cumsum(span[::-1])[:-1]]).astype(np.int64)
            self.off = rev[::-1].copy()
            self.off_arg = self.off
        else:
            self.off = np.concatenate([[0], np.cumsum(span)[:-1]]).astype(np.int64) if len(n) else np.zeros(0, dtype=np.int64)
        ends = [int(o + (k - 1) * l + k) for o, l, k in zip(self.off, self.ld, n) if k > 0]
        self.total = max(ends) if ends else 0
        self.rows = int(n.sum())
        self.row_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if len(n) else np.zeros(0, dtype=np.int64)

    def index(self, i, which):
        """flat indices of block i's elements: which = 'upper' (r <= c), 'lower' (r > c) or 'window'; in the order of np.nonzero of the mask"""
        k = int(self.sizes[i])
        r, c = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
        m = {"upper": r <= c, "lower": r > c, "window": r >= 0}[which]
        return (int(self.off[i]) + r[m] + c[m] * int(self.ld[i])).astype(np.int64), (r[m], c[m])

    def buffer(self, mats):
        """the flat buffer (total + GUARD doubles): distinct NaNs everywhere, then the upper triangle of mats[i] as block i"""
        buf = nan_pattern(self.total + GUARD)
        for i, M in enumerate(mats):
            if self.sizes[i] == 0:
                continue
            idx, (r, c) = self.index(i, "upper")
            buf[idx] = np.asarray(M, dtype=np.float64)[r, c]
        return buf

    def written(self, which):
        """boolean mask over total + GUARD: the elements of all blocks' upper triangles / windows"""
        m = np.zeros(self.total + GUARD, dtype=bool)
        for i in range(self.batch):
            if self.sizes[i]:
                m[self.index(i, which)[0]] = True
        return m

    def block(self, buf, i):
        """block i of a flat buffer as an n x n matrix [r, c] (the column-major reading)"""
        k = int(self.sizes[i])
        idx, (r, c) = self.index(i, "window")
        out = np.empty((k, k))
        out[r, c] = buf[idx]
        return out


def nan_pattern(count, salt=0):
    bits = np.int64(0x7ff8000000000000) | (np.arange(1, count + 1, dtype=np.int64) + np.int64(salt << 32))
    return bits.view(np.float64).copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def exact_blocks(fam, sizes):
    """[(T, Tinv, C) or None for an empty block] - potri_batched_cases.block with positive diagonals (premise asserted there); blocks of one
    size differ (five operands per size and family, dealt by position)"""
    return [P.block(fam, int(n), False, i % 5) if n else None for i, n in enumerate(sizes)]


def exact_logdet(T):
    """(log det (T^T T), sum |2 log t_jj|) with t_jj powers of two: 2 K log 2 with the integer K = sum log2 t_jj, in np.longdouble"""
    k = np.log2(np.diagonal(T))
    assert np.array_equal(k, np.round(k))
    ln2 = np.log(np.longdouble(2))
    return 2 * np.longdouble(k.sum()) * ln2, 2 * np.longdouble(np.abs(k).sum()) * ln2


def random_blocks(sizes, kappa):
    """one random SPD block per entry (potri_batched_cases.random_spd, seeded by position), None for an empty one"""
    return [P.random_spd(int(n), kappa, 1, seed=i)[0] if n else None for i, n in enumerate(sizes)]
