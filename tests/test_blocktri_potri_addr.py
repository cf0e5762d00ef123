"""CPU-only: the address arithmetic of the batched block-tridiagonal selected inverse (the accessors blocktri_potri_batched.hip takes from
capital_amd/csrc/blocktri_addr.h) swept workgroup by workgroup and lane by lane by a stand-alone C++ program
(tests/blocktri_potri_addr_sweep.cpp, built here with g++ and the address and undefined-behaviour sanitizers, run as a child process)
over every row of tests/blocktri_potri_cases.py.  Every global offset must lie inside its block, nothing may be addressed at position -1
or T, no E at all with T = 1, the dead lane groups at the tail of a grid nothing; the written set must be exactly the D triangles - the
whole D blocks with fill - plus the E blocks, each element once; every LDS offset must lie inside its area and every word of an MFMA
operand below n must have been written before the products read it.  The kernel calls the very functions swept here and forms no
address any other way."""
import os
import subprocess

import pytest

from tests import blocktri_cases as BC
from tests import blocktri_potri_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "blocktri_potri_addr_sweep.cpp")
INC = os.path.join(ROOT, "capital_amd", "csrc")


def line(row, eblocks=None, dfirst=0, **over):
    n, T, batch, fill, _ = row
    names = ("ldd", "step_d", "stride_d", "lde", "step_e", "stride_e")
    lay = dict(zip(names, IC.layout(row)))
    lay.update(over)
    return " ".join(str(v) for v in (n, T, batch, fill) + tuple(lay[k] for k in names) + (T - 1 if eblocks is None else eblocks, dfirst))


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blocktri_potri_addr") / "sweep")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I" + INC, SRC,
                    "-o", exe], check=True, cwd=ROOT)

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        return p.returncode, p.stdout
    return run


def test_every_row_stays_inside_its_blocks_and_writes_exactly_what_it_should(sweep):
    rows = IC.rows()
    assert {BC.padded(r[0]) for r in rows} == {8, 16, 32, 64} and {r[1] for r in rows} >= {1, 2, 3, 5, 257} and {r[3] for r in rows} == {0, 1}
    assert any(r[2] % (64 // BC.padded(r[0])) for r in rows if BC.padded(r[0]) < 64)      # dead lane groups at the tail of a grid
    lines = [line(r) for r in rows] + [line(r[:3] + (1 - r[3],) + r[4:]) for r in rows if r[1] <= 5]      # every row with the other fill too
    code, out = sweep(lines)
    assert code == 0 and out.split()[0] == "ok" and int(out.split()[1]) == len(lines), out[-2000:]
    assert int(out.split()[2]) > 0 and int(out.split()[3]) > 0


def test_the_sweep_finds_the_planted_defects(sweep):
    """the check checks: an E operand one block shorter than the chain (the kernel then addresses a coupling block the chain does not have),
    a leading dimension below n, and a D operand that starts one position late (the walk then addresses a predecessor at that chain's
    first position)."""
    for row in ((9, 3, 5, 0, "packed"), (8, 2, 9, 1, "gaps"), (64, 5, 1, 1, "ld"), (33, 3, 3, 0, "ldb")):
        code, out = sweep([line(row)])
        assert code == 0, out
        code, out = sweep([line(row, eblocks=row[1] - 2)])
        assert code == 1 and ": E: " in out, out
        code, out = sweep([line(row, dfirst=1)])
        assert code == 1 and ": D: position outside the chain" in out, out
    code, out = sweep([line((9, 3, 5, 0, "packed"), ldd=8)])
    assert code == 1 and "D: leading dimension below n" in out, out
    code, out = sweep([line((9, 3, 5, 1, "packed"), lde=8)])
    assert code == 1 and "E: leading dimension below n" in out, out
