"""CPU-only: the address arithmetic of the batched block-tridiagonal Cholesky (capital_amd/csrc/blocktri_addr.h) swept workgroup by
workgroup and lane by lane by a stand-alone C++ program (tests/blocktri_addr_sweep.cpp, built here with g++ and the address and
undefined-behaviour sanitizers) over every row of tests/blocktri_cases.py: the factor and the solve with half = 0, 1, 2.  Every offset
must lie inside its block's extent, position T - 1 must address no E block and no successor, T = 1 no E at all, the dead lane groups at
the tail of a grid nothing, and the written set must be exactly the triangles, the E blocks and the right-hand-side segments, each
element once per step.  The kernels call the very functions swept here and form no address any other way."""
import os
import subprocess

import pytest

from tests import blocktri_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "blocktri_addr_sweep.cpp")
INC = os.path.join(ROOT, "capital_amd", "csrc")


def line(row, eblocks=None, **over):
    n, T, batch, nrhs, _ = row
    names = ("ldd", "step_d", "stride_d", "lde", "step_e", "stride_e", "ldb", "stride_b")
    lay = dict(zip(names, BC.layout(row)))
    lay.update(over)
    return " ".join(str(v) for v in (n, T, batch, nrhs) + tuple(lay[k] for k in names) + (T - 1 if eblocks is None else eblocks,))


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blocktri_addr") / "sweep")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I" + INC, SRC,
                    "-o", exe], check=True, cwd=ROOT)

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        return p.returncode, p.stdout
    return run


def test_every_row_stays_inside_its_blocks_and_writes_exactly_what_it_should(sweep):
    rows = BC.rows()
    assert {BC.padded(r[0]) for r in rows} == {8, 16, 32, 64} and {r[1] for r in rows} >= {1, 2, 3, 5, 257}
    assert any(r[2] % (64 // BC.padded(r[0])) for r in rows if BC.padded(r[0]) < 64)      # dead lane groups at the tail of a grid
    assert any(r[3] > 64 for r in rows) and {r[4] for r in rows} == set(BC.LAYOUTS)
    lines = [line(r) for r in rows]
    code, out = sweep(lines)
    assert code == 0 and out.split()[0] == "ok" and int(out.split()[1]) == len(lines), out[-2000:]
    assert int(out.split()[2]) > 0 and int(out.split()[3]) > 0


def test_the_sweep_finds_a_coupling_block_at_the_last_position_and_a_short_leading_dimension(sweep):
    """the check checks: two planted lines.  An E operand one block shorter than the chain (the kernel then addresses a coupling block at
    that chain's last position), and a leading dimension below n."""
    for row in ((9, 3, 5, 3, "packed"), (8, 2, 9, 1, "gaps"), (64, 5, 1, 17, "ld")):
        code, out = sweep([line(row, eblocks=row[1] - 2)])
        assert code == 1 and ": E: " in out, out
        code, out = sweep([line(row)])
        assert code == 0, out
    code, out = sweep([line((9, 3, 5, 3, "packed"), ldd=8)])
    assert code == 1 and "D: leading dimension below n" in out, out
    code, out = sweep([line((9, 3, 5, 3, "packed"), lde=8)])
    assert code == 1 and "E: leading dimension below n" in out, out
    code, out = sweep([line((9, 3, 5, 3, "packed"), ldb=26)])
    assert code == 1 and "B: leading dimension below T n" in out, out
