"""TEST INFRASTRUCTURE: the table of the ragged block-tridiagonal tests (cap_blocktri_plan, cap_dpotrf_blocktri_vbatched,
cap_dpotrs_blocktri_vbatched, cap_dpotri_blocktri_vbatched, csrc/blocktri_vbatched.hip).  No GPU, no torch: NumPy only.

A ROW is (n, lengths, first-mode, nrhs, layout).  Chain c of a row is chain 0 of tests/blocktri_cases.py's row (n, T_c, 1, nrhs, layout)
with seed c (exact_chain / random_chain): the exactness premise is the one tests/test_blocktri_cases.py proves per chain.
n takes both edges of every NP = 8 / 16 / 32 / 64.  For NP < 64 there is a wavefront whose G = 64 / NP chains all differ in length and
include T = 0, 1 and 2 as far as G allows (G = 2 holds two of them, the third opens the next wavefront), with the longest chain not first
in batch order; batches that are no multiple of G (a ragged last wavefront); a chain of 1 position beside one of 257; NP = 64 rows such
as (2, 1, 3, 0); rows with all lengths equal.  first-modes: "default" (first = None: back to back in batch order), "gaps" (unowned slots
between the chains), "reversed" (stored in reverse batch order).  nrhs = 1, 3, 17, 70.  Layouts: packed / a leading dimension above n /
a step with a gap / ldb above n ROWS."""
import numpy as np

from tests import blocktri_cases as BC

FIRST_MODES = ("default", "gaps", "reversed")
LAYOUTS = ("packed", "ld", "gaps", "ldb")

ROWS = (
    (8, (3, 0, 1, 2, 5, 4, 7, 6), "default", 3, "packed"),          # one wavefront at NP = 8, all lengths differ, the longest not first
    (3, (2, 5, 1, 0, 3, 4, 7, 6, 2, 1, 3), "gaps", 1, "ld"),        # a ragged second wavefront
    (1, (1, 2, 0, 3, 4, 5, 6, 8, 1), "reversed", 17, "gaps"),
    (8, (1, 257), "default", 3, "gaps"),                            # 1 beside 257
    (9, (2, 0, 1, 3), "reversed", 70, "ldb"),                       # one wavefront at NP = 16
    (16, (1, 4, 2, 0, 3), "gaps", 17, "packed"),
    (17, (1, 2, 0), "default", 3, "ld"),                            # NP = 32: (2, 1) share a wavefront, (0, dead) the next
    (32, (3, 5, 2), "gaps", 1, "gaps"),
    (33, (2, 1, 3, 0), "default", 17, "packed"),                    # NP = 64
    (63, (1, 3), "reversed", 3, "ld"),
    (64, (2, 1, 3, 0), "gaps", 1, "ldb"),
    (8, (3,) * 9, "default", 3, "packed"),                          # all equal
    (64, (2, 2), "default", 1, "packed"),
)
STREAM_ROWS = (ROWS[0], ROWS[3], ROWS[10])   # mixed lengths at NP = 8, 1 beside 257, NP = 64


def rows():
    return list(ROWS)


def padded(n):
    return BC.padded(n)


def first_slots(lengths, mode):
    """the first slot of every chain, or None for the plan's default"""
    if mode == "default":
        return None
    out, at = [0] * len(lengths), 0
    order = range(len(lengths)) if mode == "gaps" else reversed(range(len(lengths)))
    for c in order:
        if mode == "gaps":
            at += c % 3 + 1
        out[c] = at
        at += lengths[c]
    return out


def geometry(row):
    """first (always a list), row offsets, slots, eslots, rows of the stacked system"""
    _, lengths, mode, _, _ = row
    first = first_slots(lengths, mode)
    prefix = [int(x) for x in np.concatenate([[0], np.cumsum(lengths)])]
    if first is None:
        first = prefix[:-1]
    slots = max([f + t for f, t in zip(first, lengths) if t > 0], default=0)
    eslots = max([f + t - 1 for f, t in zip(first, lengths) if t > 1], default=0)
    return first, prefix[:-1], slots, eslots, prefix[-1]


def layout(row):
    """(ld, step, ldb) in elements: D and E share ld and step"""
    n, lengths, _, nrhs, lay = row
    ld = n + 3 if lay == "ld" else n + 1 if lay == "ldb" else n
    step = ld * n + (5 if lay == "gaps" else 0)
    ldb = sum(lengths) * n + (4 if lay == "ldb" else 0)
    return ld, step, ldb


def order(lengths):
    """the plan's list: stable by T descending"""
    return sorted(range(len(lengths)), key=lambda c: -lengths[c])


def chain_row(row, c):
    n, lengths, _, nrhs, lay = row
    return (n, lengths[c], 1, nrhs, lay)


def exact_chain(row, c):
    """chain c: D (T, n, n) full symmetric, Bc (T - 1, n, n), X (T n, nrhs), RHS, U, W, logdet"""
    D, Bc, X, rhs, U, W, logdet = BC.exact_chain(chain_row(row, c), seed=c)
    return D[0], Bc[0], X[0], rhs[0], U[0], W[0], float(logdet[0])


def random_chain(row, c):
    D, Bc, rhs = BC.random_chain(chain_row(row, c), seed=c)
    return D[0], Bc[0], rhs[0]
