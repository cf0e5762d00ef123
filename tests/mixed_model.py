"""Rounding model of the mixed-precision factor (csrc/mixed.hip, cap_mpchol_factor) in NumPy: the arithmetic, not the schedule.

    R32 = fp32(triu(A));  nb = the largest power of two <= min(n, 1024) (the last panel may be shorter);  for every panel k:
      diagonal block   fp64 Cholesky R_kk of fp64(R32[kk]) and its inverse Dinv;  R32[kk] = fp32(R_kk)
      block row        solve3 (default): Dinv -> fp32 -> bf16 hi / lo,  row -> bf16 hi / lo  (lo = bf16(x - hi)),
                         S = hi^T hi + hi^T lo + lo^T hi  summed exactly, rounded once to fp32
                       solve3 off: S = fp32(Dinv^T fp64(row))
                       R32[row] = S;  panel P = bf16(S) (round to nearest even: the device's (__bf16)(float) cast)
      trailing update  C32 = fp32(C32 - P^T P), upper triangle, the sum exact (fp64 sums of exact bf16 products)

The schedule options (strip, split, pair_rest, the update kernel) only regroup the fp32 sums of the updates, so every one of them
must agree with this model to fp32-accumulation level.  `rounding=False` turns every rounding off: plain fp64 blocked Cholesky.
`perturb` plants ONE defect (the teeth of tests/test_mixed_model.py):
    ("trunc",)              bf16 conversions truncate instead of rounding to nearest even
    ("no_lohi",)            the lo(Dinv)^T hi(row) term of the split row solve is dropped
    ("skip_tile", k, i, j)  the 256 x 256 tile (i, j) (global tile indices) of panel k's update is not applied
    ("stale_panel", k)      panel k's update uses panel k - 1's bf16 operand (a stale pair buffer)
`matmul` replaces the fp64 products (the GPU tests pass an fp64 GEMM on the device: the same exact-to-fp64 sums, faster).
This module imports NumPy only."""
import numpy as np

TILE = 256


def panel_width(n):
    nb = 1024
    while nb > n:
        nb //= 2
    return nb


def bf16_bits(x, trunc=False):
    """uint16 bf16 encodings of the float32 array x: round to nearest even (NaN -> the canonical quiet NaN 0x7fc0), or truncation"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    if trunc:
        return (u >> 16).astype(np.uint16)
    r = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def bf16(x, trunc=False):
    """float32 values of bf16(x) for the float32 array x"""
    return (bf16_bits(x, trunc).astype(np.uint32) << 16).view(np.float32)


def _split(x, trunc=False):
    hi = bf16(x, trunc)
    return hi, bf16(x - hi, trunc)          # x - hi is exact in fp32


def factor(a, rounding=True, solve3=True, perturb=None, panels_of=None, matmul=np.matmul):
    """the fp32 factor R32 (upper, float64 array of the fp32 values; float64 throughout when rounding is off) of the SPD matrix a.

    panels_of: a factor computed elsewhere (a GPU's R32).  The trailing updates then subtract ITS bf16 panels, bf16(its block rows),
    instead of the model's own: every panel of the result is the model's arithmetic applied to the history that factor really had.
    Without it one panel that rounds to the other side of a bf16 boundary (fp32 sums in another order) changes every update behind
    it by a bf16 ulp, and those flips cascade from panel to panel; with it the comparison sees the fp32 sums alone."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    nb = panel_width(n)
    kind = perturb[0] if perturb else None
    trunc = kind == "trunc"
    f32 = (lambda x: x.astype(np.float32).astype(np.float64)) if rounding else (lambda x: x)
    c = f32(np.triu(a))
    prev_p = None
    for k, j0 in enumerate(range(0, n, nb)):
        j1 = min(n, j0 + nb)
        d = np.triu(c[j0:j1, j0:j1])
        rkk = np.linalg.cholesky(d + np.triu(d, 1).T).T
        c[j0:j1, j0:j1] = f32(rkk)
        if j1 == n:
            break
        dinv = np.linalg.inv(rkk)
        dinv = np.triu(dinv)
        row = c[j0:j1, j1:]
        if not rounding:
            s = matmul(dinv.T, row)
            p = s
        else:
            if solve3 and j1 - j0 == nb:
                dh, dl = _split(dinv.astype(np.float32), trunc)
                rh, rl = _split(row.astype(np.float32), trunc)
                dh, dl, rh, rl = (v.astype(np.float64) for v in (dh, dl, rh, rl))
                s = matmul(dh.T, rh) + matmul(dh.T, rl)
                if kind != "no_lohi":
                    s += matmul(dl.T, rh)
            else:
                s = matmul(dinv.T, row)
            s = f32(s)
            p = bf16(s.astype(np.float32), trunc).astype(np.float64)
        c[j0:j1, j1:] = s
        pu = p
        if panels_of is not None:
            pu = bf16(np.asarray(panels_of[j0:j1, j1:], dtype=np.float32)).astype(np.float64)
        if kind == "stale_panel" and perturb[1] == k and prev_p is not None:
            pu = prev_p[:, nb:]                              # the previous panel's rows at these columns
        prev_p = p
        upd = matmul(pu.T, pu)
        if kind == "skip_tile" and perturb[1] == k:
            i0, c0 = perturb[2] * TILE - j1, perturb[3] * TILE - j1
            upd[max(i0, 0):i0 + TILE, max(c0, 0):c0 + TILE] = 0.0
        c[j1:, j1:] = f32(c[j1:, j1:] - upd)
    return np.triu(c)


def tile_errors(x, ref, tile=TILE):
    """per tile x tile block of the upper triangle: ||x - ref||_F / ||ref||_F of that block (blocks with ||ref|| == 0 use 1)"""
    n = ref.shape[0]
    t = -(-n // tile)
    pad = t * tile - n
    d = np.pad(np.triu(x - ref), ((0, pad), (0, pad))).reshape(t, tile, t, tile)
    r = np.pad(np.triu(ref), ((0, pad), (0, pad))).reshape(t, tile, t, tile)
    dn = np.sqrt((d * d).sum(axis=(1, 3)))
    rn = np.sqrt((r * r).sum(axis=(1, 3)))
    return np.where(rn > 0, dn / np.where(rn > 0, rn, 1.0), dn)


U32 = 2.0 ** -24


def tolerances(n):
    """(normwise, per-tile) bounds of ||R32 - factor(a, panels_of=R32)|| / ||factor(...)|| for a factor whose updates sum in fp32.

    With the history fixed (panels_of) what is left is the order of the fp32 sums: an update of K terms accumulated in fp32 (the
    MFMA chain, then one add into C; the strips, the pairs and the split schedule regroup these) is off the exact sum by a random walk of
    ~ sqrt(K / 16) fp32 roundings of the partial sums; over the panels of an n x n factor K adds up to n, and the diagonal-block
    Cholesky and the row solve pass the error of C on with the condition of the diagonal block (sqrt(kappa(A)) <= 15 for the test
    inputs).  u32 sqrt(n / 16) * 15 ~ u32 sqrt(n) * 4: the normwise bound.  A tile of 256 x 256 carries as few as 256 (n / 256)
    elements of the ragged diagonal, so its ratio scatters more: four times the normwise bound.  Measured on the MI355X (n = 640 ..
    9216, every input kind and schedule option of tests/test_gpu_mixed.py): at most 7.6e-7 normwise (bound 2.3e-5 at n = 9216) and
    5.2e-6 per tile (n = 5248, kappa ~ 200; bound 6.9e-5)."""
    t = 4.0 * U32 * n ** 0.5
    return t, 4.0 * t
