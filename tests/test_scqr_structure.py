"""CPU-only: the schedule of a shifted CholeskyQR factor call (num_iter 3 and 4) on the recording HIP / RCCL stand-in (tests/hipshim): every
launch and collective of two factor calls replayed with vector clocks - no data race between the conditioning launches and the sweep around
them, nothing out of bounds, the ranks' collectives matching - and the launch counts of the last call: num_iter - 2 launches of each conditioning
kernel, the global row count set and summed by the FIRST call only."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import run_scenarios as rs
shapes = ((8192, 256), (5000, 37))                     # gram256 / qrapply256, and the generic path with ragged m
for us in (0, 1):
    for (m, n) in shapes:
        for iters in (2, 3, 4):
            for P in (1, 2):
                for p in range(P):
                    rs.scenario("scqr m=%d n=%d iter=%d P=%d rank=%d" % (m, n, iters, P, p), us, "scqr m=%d n=%d iter=%d P=%d" % (m, n, iters, P), p, P)(
                        lambda r, a=(m, n, iters, P, p): rs.cacqr_case(r, *a))
json.dump(rs.RESULTS, open(sys.argv[2], "w"))
"""


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    lib = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
    if not os.path.exists(lib):
        from capital_amd import build
        build.build(verbose=False)
    out = str(tmp_path_factory.mktemp("scqr") / "results.json")
    r = subprocess.run([sys.executable, "-c", DRIVER, os.path.join(ROOT, "tests", "hipshim"), out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.load(open(out))


def test_no_findings(results):
    assert len(results) == 2 * 2 * 3 * (1 + 2 + 1)                  # one per rank, one joint replay per two-rank configuration
    bad = [(x["name"], x["findings"][:3]) for x in results if x["findings"]]
    assert not bad, bad
    assert all(x["stats"].get("oob", 0) == 0 for x in results)


def test_conditioning_launches_per_factor_call(results):
    seen = 0
    for x in results:
        if "joint replay" in x["name"]:
            continue
        iters = int(x["name"].split("iter=")[1].split()[0])
        hist = x["stats"]["factor_kernels"]                          # the launches of the LAST factor call, by mangled kernel name
        count = lambda key: sum(v for k, v in hist.items() if key in k)   # noqa: E731
        for key in ("scqr_scales_kernel", "scqr_equilibrate_kernel", "scqr_unscale_kernel"):
            assert count(key) == max(iters - 2, 0), (x["name"], key, hist)
        assert count("scqr_rows_kernel") == 0, (x["name"], hist)    # the row count belongs to the plan: set by its first call
        seen += 1
    assert seen == 2 * 2 * 3 * 3
