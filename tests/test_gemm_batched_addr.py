"""CPU-only: the address arithmetic of the batched general products (capital_amd/csrc/gemm_batched_addr.h) swept lane by lane by a
stand-alone C++ program (tests/gemm_batched_addr_sweep.cpp, built here with g++ and the address and undefined-behaviour sanitizers) over
every row of tests/gemm_batched_cases.py: every wavefront and workgroup the three entries launch for the fixed-size rows and for the plan
rows (the wavefronts of `inner` in batch order with their mixed contraction lengths, those of `combine` in class order with their mixed
row counts, the dead groups at the tail of a grid).  Every addressed offset must lie inside its operand's m x k, k x n or m x n extent and
the addressed set of C must be exactly the rectangle, every element once.  The kernels call the very functions swept here."""
import os
import subprocess

import pytest

from tests import gemm_batched_cases as GC
from tests import vbatched_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_batched_addr_sweep.cpp")
INC = os.path.join(ROOT, "capital_amd", "csrc")


def padded(n):
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


def line(group, NP, n, akc, bkc, lda, ldb, ldc, blocks):
    return "%d %d %d %d %d %d %d %d %d " % (group, NP, n, akc, bkc, lda, ldb, ldc, len(blocks)) + " ".join("%d %d" % b for b in blocks)


def waves(blocks, G):
    """the blocks of a grid, G to a wavefront, the last one filled with dead groups"""
    blocks = list(blocks) + [(0, 0)] * (-len(blocks) % G)
    return [blocks[i:i + G] for i in range(0, len(blocks), G)]


def fixed_lines():
    out = []
    for (m, n, k, batch, ta, tb, ab, la, lb, lc) in GC.exact_rows():
        lda, ldb, ldc = max((k if ta else m) + la[0], 1), max((n if tb else k) + lb[0], 1), max(m + lc[0], 1)
        keff = 0 if ab[0] == 0.0 else k
        if max(m, n) > 64:
            out.append(line(1, 64, n, ta, 1 - tb, lda, ldb, ldc, [(m, keff)]))
            continue
        NP = padded(max(m, n))
        G = 64 // NP
        for w in {tuple(w) for w in waves([(m, keff)] * min(batch, 2 * G + 1), G)}:       # a full wavefront and the ragged last one
            out.append(line(0, NP, n, ta, 1 - tb, lda, ldb, ldc, w))
    return out


def plan_lines():
    out = []
    for (entry, name, kind, (a, b), ab) in GC.plan_rows():
        sizes = GC.PLAN_LISTS[name]
        rows = sum(sizes)
        on = ab[0] != 0.0
        if entry == "inner":                         # G_i (a x b) = X_i^T Y_i, contraction over the n_i rows; every block in batch order
            if not a or not b:
                continue
            blocks = [(a, s if on else 0) for s in sizes]
            if max(a, b) > 64:
                out += [line(1, 64, b, 1, 1, rows + 2, rows + 3, a + 1, [blk]) for blk in sorted(set(blocks))]
            else:
                NP = padded(max(a, b))
                out += [line(0, NP, b, 1, 1, rows + 2, rows + 3, a + 1, w) for w in waves(blocks, 64 // NP)]
        else:                                        # C_i (n_i x nrhs) = V_i (n_i x k) Z_i (k x nrhs), one launch per class
            nrhs, k = a, b if on else 0
            if not nrhs:
                continue
            for cls, lst in enumerate(VC.expected_lists(sizes)):
                blocks = [(sizes[i], k) for i in lst]
                if not blocks:
                    continue
                if cls >= 4:
                    out += [line(1, 64, nrhs, 0, 1, rows + 2, max(k, 1) + 1, rows + 1, [blk]) for blk in sorted(set(blocks))]
                else:
                    NP = 8 << cls
                    out += [line(0, NP, nrhs, 0, 1, rows + 2, max(k, 1) + 1, rows + 1, w) for w in waves(blocks, 64 // NP)]
    return out


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_addr") / "sweep")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I" + INC, SRC,
                    "-o", exe], check=True, cwd=ROOT)

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        return p.returncode, p.stdout
    return run


def test_every_fixed_size_row_stays_inside_its_operands(sweep):
    lines = fixed_lines()
    assert len(lines) >= len(GC.exact_rows())
    assert any(l.startswith("1 ") for l in lines) and {l.split()[1] for l in lines if l.startswith("0 ")} == {"8", "16", "32", "64"}
    code, out = sweep(lines)
    assert code == 0 and out.split()[0] == "ok" and int(out.split()[1]) == len(lines), out[-2000:]
    assert int(out.split()[2]) > 0 and int(out.split()[3]) > 0


def test_every_plan_row_stays_inside_its_operands(sweep):
    lines = plan_lines()
    assert any(l.startswith("1 ") for l in lines) and any(l.startswith("0 ") for l in lines)
    code, out = sweep(lines)
    assert code == 0 and out.split()[0] == "ok" and int(out.split()[1]) == len(lines), out[-2000:]


def test_the_sweep_finds_a_load_one_slab_past_an_operand(sweep):
    """the check checks: a line that claims a leading dimension below the stored extent, and a block taller than its wavefront's NP"""
    code, out = sweep([line(0, 16, 9, 0, 1, 8, 5, 9, [(9, 5)] * 4)])
    assert code == 1 and "op(A)" in out, out
    code, out = sweep([line(0, 8, 3, 0, 1, 20, 5, 20, [(9, 5)] * 8)])
    assert code == 1 and "not a launch" in out, out
