"""The case tables of tests/cqr256_cases.py reach what they claim (no GPU).

Two things are asserted:

  * coverage, on the Python mirror of the launchers' row partitions (cqr256_cases.gram_partition / apply_partition, for the 256 CUs of
    the MI355X): every class of K tiles per workgroup, of slab counts in the reduce, of row tiles per workgroup and of grids that the
    kernels distinguish has a row - nothing is left to luck, and a row that is edited away fails here;
  * the mirror is the launchers': every row is driven through cap_dgram256 / cap_dqrapply256 of the product's own object files on the
    recording stand-in (tests/hipshim/run_cqr256.py, one child process), the grids it launches are the mirror's, the CPU kernel models'
    results equal the exact references bit for bit with every NaN where it was (which checks the table and the reference helpers before a
    GPU sees them), and every refusal row returns CAP_ERR_UNSUPPORTED without a single launch."""
import json
import os
import subprocess
import sys

import pytest

from tests import cqr256_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gram_parts():
    return {(m, cap): T.gram_partition(m, cap) for m, cap, _ in T.GRAM_CASES}


def _apply_parts():
    return {(m, cap): T.apply_partition(m, cap) for m, cap, _ in T.APPLY_CASES}


def test_gram_rows_cover_every_class():
    parts = _gram_parts()
    per_wg = {k for p in parts.values() for k in p}
    small = {k for (m, cap), p in parts.items() if m <= 2048 for k in p}
    assert {1, 2, 3, 4, 5} <= small                                  # the three-deep prologue with clamped refills, the first ring wrap
    assert any(k >= 9 for k in small)                                # two wraps
    assert 0 in per_wg                                               # a workgroup without rows
    assert parts[(17424, 0)] == [33] * 33 + [0]                      # ... the smallest such m: 34 slabs of 528 rows, the last one empty
    assert all(T.gram_partition(m)[-1] > 0 for m in range(16, 17424, 16))
    assert any(len(set(p)) > 1 and min(p) > 0 for p in parts.values())          # unequal slabs, all of them at work
    assert all(16 * sum(p) == m for (m, cap), p in parts.items())    # every row belongs to exactly one slab
    slabs = {len(p) for p in parts.values()}
    assert {1, 3, 4, 5, 12, 13, 16, 17, 29} <= slabs                 # remainder loop only (<= 12), first entry into the 16-strided loop, both
    assert parts[(131072, 0)] == [32] * T.CUS                        # one slab per CU
    assert parts[(131088, 0)] == [33] * 248 + [9] + [0] * 7          # 256 slabs: one short, several empty
    # what the loops of gram256_reduce_kernel do per slab count, group by group: (16-strided trips, remainder trips)
    def trips(nslab, grp):
        z, strided, rem = grp, 0, 0
        while z + 12 < nslab:
            strided += 1; z += 16
        while z < nslab:
            rem += 1; z += 4
        return strided, rem
    seen = {trips(n, g) for n in slabs for g in range(4)}
    assert {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, 0)} <= seen
    assert any(trips(n, 0)[0] and not trips(n, 3)[0] for n in slabs)             # groups of one launch on different sides of the threshold
    # capped grids: the cap is what the partition says it is
    assert len(parts[(2048, 1)]) == 1 and parts[(2048, 1)] == [128] and parts[(2048, 3)] == [43, 43, 42]


def test_apply_rows_cover_every_class():
    parts = _apply_parts()
    one_wg = {p[0] for p in parts.values() if len(p) == 1}
    assert {1, 2, 3, 4, 5} <= one_wg                                 # the B ring returns to phase 0 at the fourth tile; u0 == 0 waits differ
    assert any(0 < p[-1] < p[0] for p in parts.values())             # a short last workgroup
    assert any(0 in p for p in parts.values())                       # workgroups without tiles
    assert any(0 in p for (m, cap), p in parts.items() if m <= 2048)
    assert parts[(640, 1)] == [5] and parts[(896, 2)] == [4, 3] and parts[(1152, 2)] == [5, 4] and parts[(1664, 3)] == [5, 5, 3]
    assert {1, 2, 3} <= {len(p) for (m, cap), p in parts.items() if cap}
    assert parts[(32896, 0)] == [2] * 128 + [1] + [0] * 127          # uncapped, ntiles = CUs + 1
    assert all(128 * sum(p) == m for (m, cap), p in parts.items())
    assert all(r <= c for r, c in T.APPLY_BLOCKS) and {(0, 0), (0, 15), (7, 8), (15, 15)} <= set(T.APPLY_BLOCKS)


def test_tables_stay_inside_the_exactness_argument():
    assert len({(m, cap) for m, cap, _ in T.GRAM_CASES}) == len(T.GRAM_CASES) and len({(m, cap) for m, cap, _ in T.APPLY_CASES}) == len(T.APPLY_CASES)
    assert all(m % 16 == 0 and 0 < m <= 131088 for m, _, _ in T.GRAM_CASES) and all(m % 128 == 0 and 0 < m <= 131088 for m, _, _ in T.APPLY_CASES)
    assert T.GRAM_LD_LAST == 4194302 and T.APPLY_LD_LAST == 35791384
    # the bounds come from the kernels' offsets: 127 columns + a chunk of rows (gram256), 15 columns + a lane offset below 1024 + 8 bytes (qrapply256)
    assert 127 * T.GRAM_LD_LAST * 8 + T.GRAM_LD_LAST * 8 < 0xfffffff0 and 15 * T.APPLY_LD_LAST * 8 + 888 + 128 + 8 < 0xffffffff
    q = T.panel(48)
    assert q.shape == (256, 48) and set(abs(q).ravel()) <= {1.0, 2.0, 3.0}
    ri = T.ri_dense(3, below=T.NAN)
    assert all((ri[c, r] == ri[c, r]) == (r // 16 <= c // 16) and (ri[c, r] != 0.0) == (r <= c or r // 16 > c // 16) for c in range(0, 256, 5) for r in range(256))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    from capital_amd import build
    build.build(verbose=False)
    out = str(tmp_path_factory.mktemp("cqr256") / "cqr256.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hipshim", "run_cqr256.py"), out], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.load(open(out))


@pytest.mark.parametrize("m,cap", [(m, cap) for m, cap, _ in T.GRAM_CASES])
def test_gram_row_on_the_stand_in(shim, m, cap):
    runs = shim["gram"]["%d-%d" % (m, cap)]
    assert len(runs) == (len(T.GRAM_LDQ_PADS) * len(T.GRAM_LDG_PADS) if m <= 2048 else 1)
    for r in runs:
        assert r["status"] == 0 and not r["detail"], r
        assert r["launches"] == 2 and r["slabs"] == len(T.gram_partition(m, cap)) and r["reduce_grid"] == 256, r
        assert r["work"] == T.gram_work_size(m) >= r["slabs"] * 65536
        assert r["exact"] is (True if m <= 20000 else None), r


@pytest.mark.parametrize("m,cap", [(m, cap) for m, cap, _ in T.APPLY_CASES])
def test_apply_row_on_the_stand_in(shim, m, cap):
    for sec in ("apply", "apply_nan") if m <= 20000 else ("apply",):
        runs = shim[sec]["%d-%d" % (m, cap)]
        assert [r["inplace"] for r in runs] == [False, True]
        for r in runs:
            assert r["status"] == 0 and not r["detail"], (sec, r)
            assert r["launches"] == 1 and r["grid"] == len(T.apply_partition(m, cap)), (sec, r)
            assert r["exact"] is (True if m <= 20000 else None), (sec, r)


def test_single_block_rows_on_the_stand_in(shim):
    assert sorted(shim["apply_block"]) == sorted("%d-%d" % b for b in T.APPLY_BLOCKS)
    for runs in shim["apply_block"].values():
        for r in runs:
            assert r["status"] == 0 and r["exact"] is True and not r["detail"] and r["grid"] == T.APPLY_BLOCK_CAP, r


def test_refusals_launch_nothing(shim):
    assert len(shim["refusals"]) == len(T.REFUSALS)
    for r in shim["refusals"]:
        assert r["status"] == T.UNSUPPORTED and r["launches"] == 0 and not r["detail"], r
    whys = " ".join(w for _, _, w in T.REFUSALS)
    for need in ("m = 0", "m % 16", "m % 128", "odd ldq", "odd ldin", "ldq < m", "ldin < m", "ldout < m", "ldg < 256", "Q 8 bytes", "Qin 8 bytes", "Ri 8 bytes",
                 "128 ldq 8 >= 0xfffffff0", "ldin beyond", "ldout beyond"):
        assert need in whys, need
    over = [o for e, o, _ in T.REFUSALS if e == "apply"]
    assert any(o.get("ldin") == T.APPLY_LD_FIRST for o in over) and any(o.get("ldin") == T.APPLY_LD_FIRST + 2 for o in over)
    assert any(o.get("ldout") == T.APPLY_LD_FIRST for o in over) and any(o.get("ldout") == T.APPLY_LD_FIRST + 2 for o in over)


def test_work_sizes(shim):
    assert {int(m): w for m, w in shim["work_sizes"].items()} == {m: T.gram_work_size(m) for m in (-16, 0, 16, 1023, 1024, 14848, 131072, 131088, 1 << 21)}
