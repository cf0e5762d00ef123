"""CPU-only: the address arithmetic of the ragged block-tridiagonal kernels (capital_amd/csrc/blocktri_addr.h on bt_chain_plan chains) swept
workgroup by workgroup and lane by lane by a stand-alone C++ program (tests/blocktri_ragged_addr_sweep.cpp, built here with g++ and the
address and undefined-behaviour sanitizers) over every row of tests/blocktri_ragged_cases.py, on the plan's sorted order: the factor, the
solve with half = 0, 1, 2 and the selected inverse with fill = 0, 1.  Every offset must lie inside the addressed chain's OWN slots of D
and its own T_c - 1 coupling slots of E, the last E slot of a chain is never addressed, an ended chain, a T = 0 chain and a dead lane
group address nothing, the written set is exactly the triangles (full blocks under fill), the E blocks and the right-hand-side segments,
each element once per step, and every exchange-area word below n that a product reads was written for that position.  The kernels call
the very functions swept here and form no address any other way."""
import os
import subprocess

import pytest

from tests import blocktri_ragged_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "blocktri_ragged_addr_sweep.cpp")
INC = os.path.join(ROOT, "capital_amd", "csrc")


def line(row, overstate=None, eslots=None, **over):
    """one launch; overstate: the chain whose plan length is one above what its operands hold"""
    n, lengths, _, nrhs, _ = row
    lengths = list(lengths)
    real = list(lengths)
    if overstate is not None:
        lengths[overstate] += 1
    first, _, _, es, _ = RC.geometry((n, tuple(lengths)) + tuple(row[2:]))
    ld, step, ldb = RC.layout((n, tuple(lengths)) + tuple(row[2:]))
    lay = dict(ldd=ld, step_d=step, lde=ld, step_e=step, ldb=ldb)
    lay.update(over)
    head = [n, nrhs, lay["ldd"], lay["step_d"], lay["lde"], lay["step_e"], lay["ldb"], es if eslots is None else eslots, len(lengths)]
    for T, f, R in zip(lengths, first, real):
        head += [T, f, R]
    return " ".join(str(v) for v in head)


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blocktri_ragged_addr") / "sweep")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I" + INC, SRC,
                    "-o", exe], check=True, cwd=ROOT)

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        return p.returncode, p.stdout
    return run


def test_every_row_stays_inside_its_own_chains_and_writes_exactly_what_it_should(sweep):
    rows = RC.rows()
    assert {RC.padded(r[0]) for r in rows} == {8, 16, 32, 64} and {r[2] for r in rows} == set(RC.FIRST_MODES)
    assert any(0 in r[1] for r in rows) and any(len(r[1]) % (64 // RC.padded(r[0])) for r in rows if RC.padded(r[0]) < 64)
    lines = [line(r) for r in rows]
    code, out = sweep(lines)
    assert code == 0 and out.split()[0] == "ok" and int(out.split()[1]) == len(lines), out[-2000:]
    assert int(out.split()[2]) > 0 and int(out.split()[3]) > 0


def test_the_sweep_rejects_its_planted_defects(sweep):
    """the check checks.  A chain whose length is overstated by one against its operands (the kernel walks one position past the
    chain's own slots - into its neighbour's, or behind the operand); an E operand one slot short at the end; a leading dimension
    below n; ldb below n ROWS."""
    for row, c in ((RC.ROWS[0], 2), (RC.ROWS[0], 6), (RC.ROWS[4], 1), (RC.ROWS[8], 3), (RC.ROWS[10], 0)):
        code, out = sweep([line(row, overstate=c)])
        assert code == 1 and ("own slots" in out or "own rows" in out), out
        code, out = sweep([line(row)])
        assert code == 0, out
    for row in (RC.ROWS[0], RC.ROWS[4], RC.ROWS[10]):
        es = RC.geometry(row)[3]
        code, out = sweep([line(row, eslots=es - 1)])
        assert code == 1 and ": E: a slot beyond the operand" in out, out
    row = RC.ROWS[4]
    n = row[0]
    code, out = sweep([line(row, ldd=n - 1)])
    assert code == 1 and "D: leading dimension below n" in out, out
    code, out = sweep([line(row, lde=n - 1)])
    assert code == 1 and "E: leading dimension below n" in out, out
    code, out = sweep([line(row, ldb=n * sum(row[1]) - 1)])
    assert code == 1 and "B: leading dimension below n ROWS" in out, out
