"""Case tables for the two n = 256 CholeskyQR kernels of csrc/cqr_kernels.hip, driven on their own through cap_dgram256 and
cap_dqrapply256.  Shared by tests/test_cqr256_cases.py (no GPU: the tables reach every class of the kernels' partitions, and every row
runs through the library's own launchers on the recording stand-in) and tests/test_gpu_cqr256_exact.py (-m gpu: the same rows on the
device).  Plain data and NumPy helpers, nothing of the GPU is imported here.

EXACT RESULTS.  Every operand entry is an integer of {+-1, +-2, +-3} (Ri: 0 where the operand must be zero), m <= 131088 and the
contraction of the apply has 256 terms: every partial sum of G = Q^T Q, in ANY order and split over any number of slabs, is an integer of
magnitude <= 9 * 131088 = 1.2e6, every partial sum of Qout = Qin Ri one of magnitude <= 9 * 256 - exact doubles.  The float64 NumPy product
IS the result and the device must reproduce it bit for bit (a sum that comes out zero is +0.0 on both sides: accumulators start at +0.0
and round-to-nearest never turns x + (-x) or +0.0 + (-0.0) into -0.0); the references assert the premise instead of assuming it.

WHAT A CASE MUST REACH is decided by how the launchers split the rows, mirrored here (gram_partition, apply_partition):

  gram256     nslab = max(1, min(max_wgs, CUs, m / 512)) workgroups own chunk = round_up(ceil(m / nslab), 16) rows each, that is
              max(0, min(chunk, m - b chunk)) / 16 K tiles for workgroup b, staged through a 4-stage LDS ring that is primed with three
              tiles (clamped to the last one: 1, 2 and 3 K tiles are all-prologue, 4 and 5 the first refills, the ring wraps at 4);
              gram256_reduce adds the nslab slabs in four interleaved groups, 16-strided while z + 12 < nslab, then one by one.
  qrapply256  ntiles = m / 128 row tiles, G = min(max_wgs, CUs, ntiles) workgroups, workgroup b walks the max(0, min(per, ntiles - b per))
              tiles from b per on, per = ceil(ntiles / G): the K loop runs on across row tiles through a 4-stage and a 3-stage ring, so
              the B ring is back in phase 0 only at the fourth tile, and the first tile's wait differs from every later one.

max_wgs (0 = none) is what lets a row give ONE workgroup five row tiles at m = 640 and makes the rows independent of the CU count."""
import functools

import numpy as np

from tests.blas3_cases import NAN, ints

N = 256
CUS = 256                       # the device the tables are laid out for (MI355X); the GPU tests are exact on any CU count
UNSUPPORTED = 4                 # CAP_ERR_UNSUPPORTED


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


def cap_of(x, cap):
    return min(x, cap) if cap > 0 else x


def gram_partition(m, cap=0, cus=CUS):
    """K tiles (16 rows) of every workgroup of gram256_kernel, in blockIdx order"""
    nslab = max(1, cap_of(min(cus, m // 512), cap))
    chunk = round_up(ceil_div(m, nslab), 16)
    return [max(0, min(chunk, m - b * chunk)) // 16 for b in range(nslab)]


def gram_work_size(m, cus=CUS):
    """cap_dgram256_work_size: the uncapped slab count"""
    return max(1, min(cus, m // 512)) * N * N if m > 0 else 0


def apply_partition(m, cap=0, cus=CUS):
    """row tiles (128 rows) of every workgroup of qrapply256_kernel, in blockIdx order"""
    ntiles = m // 128
    grid = cap_of(min(cus, ntiles), cap)
    per = ceil_div(ntiles, grid)
    return [max(0, min(per, ntiles - b * per)) for b in range(grid)]


# ------------------------------------------------------------------------------------------------------------------ the tables: (m, max_wgs, why)
GRAM_CASES = (
    (16, 0, "1 K tile: the three prologue requests all clamp to tile 0"),
    (32, 0, "2 K tiles: prologue clamped once, both refills clamped"),
    (48, 0, "3 K tiles: the prologue exactly, every refill clamped"),
    (64, 0, "4 K tiles: the first real refill, into the fourth stage"),
    (80, 0, "5 K tiles: the ring wraps, tile 4 lands in stage 0"),
    (144, 0, "9 K tiles: the ring wraps twice"),
    (512, 0, "32 K tiles: the smallest full slab"),
    (1040, 0, "2 unequal slabs: 528 + 512 rows"),
    (1536, 0, "3 slabs: the remainder loop of the reduce, one group idle"),
    (2048, 0, "4 slabs: one slab per group"),
    (2048, 1, "capped to one workgroup: 128 K tiles, 32 wraps"),
    (2048, 3, "capped to 3 unequal slabs: 688 + 688 + 672 rows"),
    (2560, 0, "5 slabs: group 0 adds two"),
    (6144, 0, "12 slabs: the last count without the 16-strided loop"),
    (6656, 0, "13 slabs: group 0 enters the 16-strided loop, the others do not"),
    (8192, 0, "16 slabs: every group in the 16-strided loop, no remainder"),
    (8704, 0, "17 slabs: 16-strided loop and remainder in group 0"),
    (14848, 0, "29 slabs: group 0 twice through the 16-strided loop, the others once + remainder"),
    (17424, 0, "34 slabs of 528 rows, the last one EMPTY: its zero slab must still be written"),
    (131072, 0, "one full slab per CU"),
    (131088, 0, "256 slabs of 528 rows: 248 full, one short (9 K tiles), seven empty"),
)
GRAM_LDQ_PADS = (0, 2, 6)
GRAM_LDG_PADS = (0, 3)

APPLY_CASES = (
    (128, 0, "one row tile"),
    (256, 0, "two workgroups, one tile each"),
    (256, 1, "2 tiles in one workgroup: the K loop runs across a row-tile boundary"),
    (384, 1, "3 tiles: the B ring (3 stages) at phases 0, 1, 2"),
    (512, 1, "4 tiles: the B ring back at phase 0"),
    (640, 1, "5 tiles"),
    (640, 4, "5 tiles on a grid of 4: 2 + 2 + 1 + a workgroup with none"),
    (896, 2, "7 tiles on 2: 4 + a short last workgroup of 3"),
    (1152, 2, "9 tiles on 2: 5 + 4"),
    (1664, 3, "13 tiles on 3: 5 + 5 + 3"),
    (32896, 0, "uncapped, CUs + 1 tiles: two per workgroup, one short, the upper half of the grid idle"),
)
# a single nonzero 16 x 16 block (r, c), r <= c, of Ri: only block column c of the result is nonzero, and it is Qin's block column r times the
# block - a K tile consumed at the wrong step or a block column stored from the wrong accumulator moves a visibly wrong block
APPLY_BLOCKS = ((0, 0), (0, 1), (0, 15), (1, 14), (7, 8), (8, 8), (14, 15), (15, 15))
APPLY_BLOCK_M, APPLY_BLOCK_CAP = 384, 1          # three tiles in one workgroup: every phase of the B ring sees the block

LIMIT = 0xfffffff0
GRAM_LD_LAST = ((LIMIT - 1) // (128 * 8)) & ~1                   # 128 ld 8 < 0xfffffff0: the offsets of the 128 columns of a half
GRAM_LD_FIRST = GRAM_LD_LAST + 2
APPLY_LD_LAST = ((LIMIT - 1 - 1024) // (15 * 8)) & ~1            # 15 ld 8 + 1024 < 0xfffffff0: 15 columns of a tile + the lane offset
APPLY_LD_FIRST = APPLY_LD_LAST + 2
BIG_GRAM_M = 128
assert 128 * GRAM_LD_LAST * 8 < LIMIT <= 128 * GRAM_LD_FIRST * 8 and 15 * APPLY_LD_LAST * 8 + 1024 < LIMIT <= 15 * APPLY_LD_FIRST * 8 + 1024

# Refusals: (entry, overrides of the accepted base call, why).  Base calls: m = 1024, every leading dimension minimal, every pointer aligned.
# `off_*` are BYTE offsets added to a pointer, `null` names a pointer passed as NULL.
GRAM_BASE = dict(m=1024, ldq=1024, ldg=256, cap=0, off_q=0, null=None)
APPLY_BASE = dict(m=1024, ldin=1024, ldout=1024, cap=0, off_qin=0, off_ri=0, null=None)
REFUSALS = (
    ("gram", dict(m=0), "m = 0"),
    ("gram", dict(m=-16), "m < 0"),
    ("gram", dict(m=1032, ldq=1032), "m % 16 != 0"),
    ("gram", dict(ldq=1025), "odd ldq"),
    ("gram", dict(ldq=1022), "ldq < m"),
    ("gram", dict(ldg=254), "ldg < 256"),
    ("gram", dict(ldg=255), "ldg < 256 (odd)"),
    ("gram", dict(off_q=8), "Q 8 bytes off 16-byte alignment"),
    ("gram", dict(m=128, ldq=GRAM_LD_FIRST), "128 ldq 8 >= 0xfffffff0"),
    ("gram", dict(m=128, ldq=GRAM_LD_FIRST + 2), "128 ldq 8 >= 0xfffffff0"),
    ("gram", dict(cap=-1), "negative max_wgs"),
    ("gram", dict(null="q"), "NULL Q"),
    ("gram", dict(null="g"), "NULL G"),
    ("gram", dict(null="work"), "NULL work"),
    ("apply", dict(m=0), "m = 0"),
    ("apply", dict(m=-128), "m < 0"),
    ("apply", dict(m=1040, ldin=1040, ldout=1040), "m % 128 != 0 (a multiple of 16)"),
    ("apply", dict(ldin=1025), "odd ldin"),
    ("apply", dict(ldin=1022), "ldin < m"),
    ("apply", dict(ldout=1022), "ldout < m"),
    ("apply", dict(off_qin=8), "Qin 8 bytes off 16-byte alignment"),
    ("apply", dict(off_ri=8), "Ri 8 bytes off 16-byte alignment"),
    ("apply", dict(m=128, ldin=APPLY_LD_FIRST), "ldin beyond the 32-bit offsets of a tile"),
    ("apply", dict(m=128, ldin=APPLY_LD_FIRST + 2), "ldin beyond the 32-bit offsets of a tile"),
    ("apply", dict(m=128, ldout=APPLY_LD_FIRST), "ldout beyond the 32-bit offsets of a tile"),
    ("apply", dict(m=128, ldout=APPLY_LD_FIRST + 2), "ldout beyond the 32-bit offsets of a tile"),
    ("apply", dict(m=128, ldin=1 << 29, ldout=1 << 29), "ld * 8 does not fit 32 bits at all"),
    ("apply", dict(cap=-1), "negative max_wgs"),
    ("apply", dict(null="qin"), "NULL Qin"),
    ("apply", dict(null="ri"), "NULL Ri"),
    ("apply", dict(null="qout"), "NULL Qout"),
)
FAKE = 0x40000000               # an aligned address that is never dereferenced: a refusal returns before any launch


def refusal_call(L, entry, over, ptr=lambda a: a):
    """issue the refused call of a REFUSALS row on fake pointers -> status"""
    a = dict(GRAM_BASE if entry == "gram" else APPLY_BASE)
    a.update(over)

    def p(name, off=0):
        return None if a["null"] == name else ptr(FAKE + off)
    if entry == "gram":
        return L.cap_dgram256(a["m"], p("q", a["off_q"]), a["ldq"], p("g"), a["ldg"], p("work"), a["cap"], None)
    return L.cap_dqrapply256(a["m"], p("qin", a["off_qin"]), a["ldin"], p("ri", a["off_ri"]), p("qout"), a["ldout"], a["cap"], None)


# ------------------------------------------------------------------------------------------------------------------ operands and references
@functools.lru_cache(maxsize=None)
def panel(m, seed=0):
    """the m x 256 panel as its column-major image without padding: array [256][m] of nonzero integers (read-only, shared)"""
    q = ints(np.random.default_rng(1000 * seed + m), (N, m))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def gram_reference(m):
    """the 256 x 256 square G must hold, as its column-major image [col][row]: Q^T Q on and above the diagonal, +0.0 below"""
    q = panel(m)
    g = q @ q.T
    assert np.abs(g).max() <= 9 * m < 2.0 ** 53 and np.array_equal(g, np.rint(g)), "the premise of exactness"
    g = np.tril(g)                              # image [col][row]: row <= col is the LOWER triangle of the image
    g.setflags(write=False)
    return g


def place_cols(mat, ld):
    """column-major buffer [cols][ld] of the image mat [cols][rows]; pad rows NaN"""
    buf = np.full((mat.shape[0], ld), NAN)
    buf[:, :mat.shape[1]] = mat
    return buf


def ri_dense(seed, below=0.0):
    """Ri as its column-major image [col][row] (ld 256): nonzero integers on and above the diagonal, 0.0 strictly below it inside the
    16 x 16 diagonal blocks, `below` (0.0 or NaN) in every 16 x 16 block below the block diagonal"""
    rng = np.random.default_rng(7000 + seed)
    r = np.triu(ints(rng, (N, N)))              # r[row][col]
    blk = np.arange(N) // 16
    r[blk[:, None] > blk[None, :]] = below
    return np.ascontiguousarray(r.T)


def ri_block(br, bc, seed):
    """Ri with the single nonzero 16 x 16 block (br, bc), br <= bc (upper triangular inside a diagonal block), as its image [col][row]"""
    assert br <= bc
    rng = np.random.default_rng(8000 + seed)
    r = np.zeros((N, N))
    r[16 * br:16 * br + 16, 16 * bc:16 * bc + 16] = ints(rng, (16, 16))
    return np.ascontiguousarray(np.triu(r).T)


def apply_reference(q, ri):
    """image [256][m] of Qin Ri for the images q [256][m] and ri [col][row]; NaN blocks of ri (never read) count as zero"""
    r = np.nan_to_num(ri, nan=0.0)
    assert np.count_nonzero(np.triu(r, 1)) == 0, "Ri must be upper triangular (its image lower)"
    out = r @ q + 0.0
    assert np.abs(out).max() <= 9 * N and np.array_equal(out, np.rint(out)), "the premise of exactness"
    return out
