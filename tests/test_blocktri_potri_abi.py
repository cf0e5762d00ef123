"""CPU-only: argument handling of the batched block-tridiagonal selected inverse (cap_dpotri_blocktri_batched) - the argument rules of
include/capital_amd.h in their stated order, every case decided before the library touches a device - the header / ctypes agreement,
the Python and engine names and refusals, and the compiler's resource remarks of the four kernel instances.  The last test drives the
entry through the recording stand-in of tests/hipshim in a process of its own (this file run as a script): exactly one launch per call
and nothing else (no allocation, memset, copy or synchronisation), every launch annotated, no finding, nothing for an empty call, and
the access notes cover EXACTLY what tests/test_blocktri_potri_addr.py's sweep says the kernel touches: the upper triangles of the D blocks
(the whole blocks with fill), the E blocks and info."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
LOWER, UPPER = 0, 1
OK, ARG, HIP, UNSUPPORTED = 0, 1, 2, 4
NAME = "cap_dpotri_blocktri_batched"
TRACE = ((1, 1, 3, 0), (8, 3, 17, 1), (9, 2, 5, 0), (33, 5, 3, 1), (64, 3, 2, 0))      # n, T, batch, fill
LDS = {8: 11264, 16: 22016, 32: 43520, 64: 86528}          # bytes: 64 / NP images + two exchange areas (the kernel file's head)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


PD, PE, PI = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 30)   # never dereferenced


def call(L):
    def potri(uplo=UPPER, fill=0, n=9, T=3, D=PD, ldd=9, step_d=81, stride_d=243, E=PE, lde=9, step_e=81, stride_e=162, info=PI, batch=5):
        return L.cap_dpotri_blocktri_batched(uplo, fill, n, T, D, ldd, step_d, stride_d, E, lde, step_e, stride_e, info, batch, None)
    return potri


def test_arguments_are_checked_in_the_documented_order(L):
    f = call(L)
    b = dict(n=65, ldd=65, lde=65, step_d=65 * 65, step_e=65 * 65, stride_d=3 * 65 * 65, stride_e=2 * 65 * 65)
    # 1. negative sizes - before everything else
    assert f(n=-1) == ARG and f(T=-1) == ARG and f(batch=-1) == ARG and f(n=-1, uplo=LOWER) == ARG and f(batch=-1, D=None) == ARG and f(n=-1, fill=2) == ARG
    # 2. NULL pointers with work to do; E only when T > 1; info may be NULL
    assert f(D=None) == ARG and f(E=None) == ARG and f(D=None, uplo=LOWER) == ARG and f(D=None, fill=2) == ARG and f(D=None, **b) == ARG
    assert f(D=None, batch=0) == OK and f(D=None, E=None, n=0, ldd=0, lde=0) == OK and f(D=None, E=None, T=0) == OK
    assert f(info=None, batch=0) == OK
    # 3. the layout, in 128-bit arithmetic
    assert f(ldd=8) == ARG and f(lde=8) == ARG and f(step_d=80) == ARG and f(step_e=80) == ARG and f(stride_d=242) == ARG and f(stride_e=161) == ARG
    assert f(ldd=8, uplo=LOWER) == ARG and f(ldd=8, fill=2) == ARG and f(ldd=64, **{k: v for k, v in b.items() if k != "ldd"}) == ARG
    assert f(stride_d=-1) == ARG and f(step_d=-1) == ARG and f(stride_d=0) == ARG
    assert f(ldd=1 << 40, step_d=1 << 62, stride_d=0) == ARG                      # 3 x 2^62 does not wrap
    assert f(T=2, stride_e=80) == ARG and f(T=2, stride_e=81, step_e=0, uplo=LOWER) == UNSUPPORTED          # one E block per chain: no step
    assert f(T=1, E=None, lde=0, step_e=0, stride_e=0, stride_d=80) == ARG        # one block per chain: E is not looked at
    # 4. fill after the layout, before uplo
    assert f(fill=2) == ARG and f(fill=-1) == ARG and f(fill=2, uplo=LOWER) == ARG and f(fill=2, **b) == ARG and f(fill=2, batch=0) == ARG
    # 5. uplo, 6. n, 7. T n, 8. the grid - in that order
    assert f(uplo=LOWER) == UNSUPPORTED and f(uplo=LOWER, **b) == UNSUPPORTED and f(**b) == UNSUPPORTED and f(batch=0, **b) == UNSUPPORTED
    long = dict(n=64, T=1 << 25, ldd=64, lde=64, step_d=4096, step_e=4096, batch=1, stride_d=0, stride_e=0)
    assert f(**long) == UNSUPPORTED and f(uplo=LOWER, **long) == UNSUPPORTED and f(**dict(long, ldd=63)) == ARG
    wide = dict(n=8, T=1, ldd=8, step_d=64, stride_d=64, E=None, lde=8, step_e=64, stride_e=64, batch=1 << 34)
    assert f(**wide) == UNSUPPORTED
    # 9. nothing to do: no launch, whatever the pointers
    assert f(batch=0, D=None, E=None, info=None) == OK and f(n=0, D=None, E=None, info=None, ldd=0, lde=0) == OK and f(T=0, D=None, E=None) == OK


def test_header_declares_the_symbol_with_the_ctypes_signature(L):
    from capital_amd import _lib
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as fh:
        header = fh.read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    m = re.search(r"^int %s\(([^;]*)\);" % NAME, header, re.M)
    assert m, NAME + " is not declared"
    want = []
    for a in m.group(1).replace("\n", " ").split(","):
        a = a.strip()
        want.append(C.c_void_p if "*" in a else kinds[a.replace("const ", "").split()[0]])
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and list(args) == want, (args, want)
    assert getattr(L, NAME).argtypes == want
    section = header[header.index("csrc/blocktri_potri_batched.hip"):m.start()]
    assert header.index("csrc/blocktri_potri_batched.hip") > header.index("int cap_dpotrs_blocktri_batched(")        # a section of its own, after
    for s in ("THE BIT CONTRACT IS A COMPOSITION", "CONSEQUENCES", "Argument rules, in this order", "ONE launch per call", "Position 0 has no predecessor",
              "fma(beta, p, t)", "ONLY THE", "2^31 - 1", "P_i - C_i G_i^T", "clone"):
        assert s in section, s
    with open(os.path.join(ROOT, "capital_amd", "csrc", "blocktri_potri_batched.hip")) as fh:
        head = fh.read().split("#include", 1)[0]
    for s in ("THE ARITHMETIC IS A COMPOSITION", "HOW THE BLOCKS TRAVEL", "blocktri_addr.h", "out of scope", "pb_backward_step", "pi_invert",
              "pi_product_rows", "hipFuncSetAttribute", "ONE wavefront per CU", "84.5 KiB"):
        assert s in head, s


def test_python_layer_names_and_refusals():
    import torch
    from capital_amd import _lib, batched, lapack
    fn = lapack.engine._potri_blocktri_batched
    assert callable(fn) and "64" in fn.__doc__
    doc = batched.blocktri_potri.__doc__
    assert "torch.linalg.inv" in doc and "Sigma[block i + 1, block i]" in doc and "lower triangle" in doc.lower() and "clone" in doc
    assert "blocktri_potri" in batched.__doc__
    assert len({int(m) for m in lapack.Method}) == len(list(lapack.Method))
    col = lapack.ArgPack_potri_blocktri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    row = lapack.ArgPack_potri_blocktri_batched(lapack.Order.AlapackRowMajor, lapack.UpLo.AlapackUpper)
    assert col.method == lapack.Method.AlapackPotriBlocktriBatched
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        fn(None, None, 4, 2, 4, 16, 32, 4, 16, 16, 1, None, row)
    with pytest.raises(_lib.CapitalError, match="64"):
        fn(None, None, 65, 2, 65, 65 * 65, 2 * 65 * 65, 65, 65 * 65, 65 * 65, 1, None, col)
    D, E = torch.zeros(2, 3, 4, 4, dtype=torch.float64), torch.zeros(2, 2, 4, 4, dtype=torch.float64)
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        batched.blocktri_potri(D, E)
    with pytest.raises(_lib.CapitalError):
        batched.blocktri_potri(None, None)


def test_every_kernel_instance_lives_in_registers_and_states_its_lds(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR at NP = 8, 16, 32, 64; the LDS is dynamic (no static
    allocation) and its size is what the kernel file's head states"""
    from capital_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if re.search(r"\d+blocktri_potri_kernelI", k)}
    assert len(res) == 4, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
        assert int(v["LDS Size"]) == 0, (k, v)
    assert "blocktri_potri_kernel" in build.NO_SCRATCH
    for NP, want in LDS.items():                   # 8 bytes x (64 / NP images of NP / 2 lines of NP + 2 doubles + 2 areas of NP lines of 68 doubles)
        assert 8 * ((64 // NP) * (NP // 2) * (NP + 2) + 2 * NP * 68) == want
    assert LDS[32] <= 64 * 1024 < LDS[64] <= 160 * 1024 and 160 * 1024 // LDS[64] == 1


def test_one_annotated_launch_per_call_on_the_recording_stand_in(tmp_path):
    from capital_amd import build
    build.build(verbose=False)
    out = tmp_path / "trace.json"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    res = json.load(open(out))
    assert len(res) == 2 * len(TRACE)
    for x in res:
        assert not x["findings"], (x["name"], x["findings"][:4])
        assert x["stats"]["kernels"] == x["expected"] and not x["stats"].get("unannotated"), (x["name"], x["stats"], x["expected"])
        assert x["stats"]["oob"] == 0 and x["stats"].get("races", 0) == 0
        assert all(k.startswith("K ") and "blocktri_potri" in k for k in x["launches"]), x["launches"]
        for name, lines in x["per_call"]:
            assert len(lines) == 1 and lines[0].startswith("K "), (x["name"], name, lines)       # one launch and nothing else
        assert x["empty_calls"] == []
        assert x["coverage"] == [], x["coverage"][:4]


def _trace_main(out_path):
    """runs in a process of its own (no torch: the stand-in takes the place of the HIP runtime)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipshim"))
    sys.path.insert(0, ROOT)
    import run_scenarios as S
    from tests import blocktri_potri_cases as IC
    from tests.test_blocktri_abi import _marks, _noted
    results = []
    for user_stream in (0, 1):
        tag = " [user stream]" if user_stream else " [NULL stream]"
        for (n, T, batch, fill) in TRACE:
            ldd, step_d, stride_d, lde, step_e, stride_e = IC.layout((n, T, batch, fill, "gaps"))
            r = S.Run("blocktri potri %d x %d%s" % (n, T, tag), user_stream)
            # the buffers end with the last element the kernel may touch: a note that reaches further is out of bounds
            dsz = (batch - 1) * stride_d + (T - 1) * step_d + (n - 1) * ldd + n
            esz = (batch - 1) * stride_e + (T - 2) * step_e + (n - 1) * lde + n if T > 1 else 1
            Dd, Ed, Id = S.dmalloc(8 * dsz), S.dmalloc(8 * esz), S.dmalloc(4 * batch)
            E = Ed if T > 1 else None
            calls = [("potri", S.L.cap_dpotri_blocktri_batched, UPPER, fill, n, T, Dd, ldd, step_d, stride_d, E, lde, step_e, stride_e, Id, batch, r.stream),
                     ("potri no info", S.L.cap_dpotri_blocktri_batched, UPPER, 1 - fill, n, T, Dd, ldd, step_d, stride_d, E, lde, step_e, stride_e, None,
                      batch, r.stream)]
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty batch=0", S.L.cap_dpotri_blocktri_batched, UPPER, fill, n, T, None, ldd, step_d, stride_d, None, lde, step_e, stride_e, None, 0,
                       r.stream),
                      ("empty T=0", S.L.cap_dpotri_blocktri_batched, UPPER, fill, n, 0, Dd, ldd, step_d, stride_d, E, lde, step_e, stride_e, Id, batch,
                       r.stream)):
                S.ok(r.call(*c), c[0])
            res = r.finish()
            res["expected"] = len(calls)
            res["launches"] = [l for l in r.lines if l.startswith("K ")]
            res["per_call"], res["empty_calls"], notes = _marks(r)
            # what the sweep says is touched, in bytes from the start of each buffer
            tri = {8 * (c * stride_d + i * step_d + a + b * ldd) for c in range(batch) for i in range(T) for b in range(n) for a in range(b + 1)}
            blk = {8 * (c * stride_d + i * step_d + a + b * ldd) for c in range(batch) for i in range(T) for b in range(n) for a in range(n)}
            full = {8 * (c * stride_e + i * step_e + a + b * lde) for c in range(batch) for i in range(T - 1) for b in range(n) for a in range(n)}
            cov = []
            for what, lines in notes:
                if what.startswith("empty"):
                    if lines:
                        cov.append((what, "notes for an empty call"))
                    continue
                rd, wr = _noted(lines)
                got = {"rd": sorted(sorted(v) for v in rd.values()), "wr": sorted(sorted(v) for v in wr.values())}
                f = fill if what == "potri" else 1 - fill
                d = sorted(blk if f else tri)          # the D blocks are noted as cap_dpotri_batched notes its block: read and written
                e = [sorted(full)] if T > 1 else []
                want_rd = [d] + e + ([list(range(0, 4 * batch, 4))] if what == "potri" else [])
                want_wr = [d] + e
                if got["rd"] != sorted(want_rd) or got["wr"] != sorted(want_wr):
                    cov.append((what, [len(v) for v in got["rd"]], [len(v) for v in want_rd], [len(v) for v in got["wr"]], [len(v) for v in want_wr]))
            res["coverage"] = cov
            for q in (Dd, Ed, Id):
                S.shim.hipFree(q)
            results.append(res)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
