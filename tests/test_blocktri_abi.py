"""CPU-only: argument handling of the batched block-tridiagonal Cholesky (cap_dpotrf_blocktri_batched, cap_dpotrs_blocktri_batched) - the
argument rules of include/capital_amd.h in their stated order, every case decided before the library touches a device - the header /
ctypes agreement, the Python and engine names and refusals, and the compiler's resource remarks of the eight kernel instances.  The last
test drives both entries through the recording stand-in of tests/hipshim in a process of its own (this file run as a script): exactly
one launch per call and nothing else (no allocation, memset, copy or synchronisation), every launch annotated, no finding, nothing for
an empty call, and the access notes cover EXACTLY what tests/test_blocktri_addr.py's sweep says the kernels touch: the upper triangles
of the D blocks, the E blocks, the right-hand-side segments, info and logdet."""
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
NAMES = ("cap_dpotrf_blocktri_batched", "cap_dpotrs_blocktri_batched")
TRACE = ((1, 1, 3, 1), (8, 3, 17, 3), (9, 2, 5, 70), (33, 5, 3, 16), (64, 3, 2, 17))      # n, T, batch, nrhs


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


PD, PE, PB, PI = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28), C.c_void_p(1 << 30)   # never dereferenced


def calls(L):
    def factor(uplo=UPPER, n=9, T=3, D=PD, ldd=9, step_d=81, stride_d=243, E=PE, lde=9, step_e=81, stride_e=162, info=PI, logdet=None, batch=5):
        return L.cap_dpotrf_blocktri_batched(uplo, n, T, D, ldd, step_d, stride_d, E, lde, step_e, stride_e, info, logdet, batch, None)

    def solve(uplo=UPPER, half=0, n=9, T=3, nrhs=4, D=PD, ldd=9, step_d=81, stride_d=243, E=PE, lde=9, step_e=81, stride_e=162, B=PB, ldb=27,
              stride_b=108, info=None, batch=5):
        return L.cap_dpotrs_blocktri_batched(uplo, half, n, T, nrhs, D, ldd, step_d, stride_d, E, lde, step_e, stride_e, B, ldb, stride_b, info, batch,
                                             None)
    return factor, solve


def test_arguments_are_checked_in_the_documented_order(L):
    factor, solve = calls(L)
    big = dict(n=65, ldd=65, lde=65, step_d=65 * 65, step_e=65 * 65, stride_d=3 * 65 * 65, stride_e=2 * 65 * 65)
    bigs = dict(big, ldb=195, stride_b=4 * 195)
    for f, b in ((factor, big), (solve, bigs)):
        # 1. negative sizes - before everything else
        assert f(n=-1) == ARG and f(T=-1) == ARG and f(batch=-1) == ARG and f(n=-1, uplo=LOWER) == ARG and f(batch=-1, D=None) == ARG
        # 2. NULL pointers with work to do; E only when T > 1
        assert f(D=None) == ARG and f(E=None) == ARG and f(D=None, uplo=LOWER) == ARG and f(D=None, **b) == ARG
        assert f(D=None, batch=0) == OK and f(D=None, E=None, n=0, ldd=0, lde=0) == OK and f(D=None, E=None, T=0) == OK
        # 3. the layout, in 128-bit arithmetic
        assert f(ldd=8) == ARG and f(lde=8) == ARG and f(step_d=80) == ARG and f(step_e=80) == ARG and f(stride_d=242) == ARG and f(stride_e=161) == ARG
        assert f(ldd=8, uplo=LOWER) == ARG and f(ldd=64, **{k: v for k, v in b.items() if k != "ldd"}) == ARG
        assert f(stride_d=-1) == ARG and f(step_d=-1) == ARG and f(stride_d=0) == ARG
        assert f(ldd=1 << 40, step_d=1 << 62, stride_d=0) == ARG                  # 3 x 2^62 does not wrap
        assert f(T=2, stride_e=80) == ARG and f(T=2, stride_e=81, step_e=0, uplo=LOWER) == UNSUPPORTED      # one E block per chain: no step
        # 5. uplo, 6. n, 7. T n, 8. the grid - in that order
        assert f(uplo=LOWER) == UNSUPPORTED and f(uplo=LOWER, **b) == UNSUPPORTED and f(**b) == UNSUPPORTED and f(batch=0, **b) == UNSUPPORTED
    assert factor(info=None) == ARG and factor(info=None, batch=0) == OK
    assert solve(nrhs=-1) == ARG and solve(B=None) == ARG and solve(B=None, nrhs=0) == OK and solve(ldb=26) == ARG and solve(stride_b=107) == ARG
    # one block per chain: E holds nothing and is not looked at; the stride rule falls back to one block
    assert factor(T=1, E=None, lde=0, step_e=0, stride_e=0, stride_d=80) == ARG
    # 4. half after the layout, before uplo
    assert solve(half=3) == ARG and solve(half=-1) == ARG and solve(half=3, ldb=26) == ARG and solve(half=3, uplo=LOWER) == ARG and solve(half=3, **bigs) == ARG
    # 7. T n > 2^31 - 1 (far apart operands, one chain)
    long = dict(n=64, T=1 << 25, ldd=64, lde=64, step_d=4096, step_e=4096, batch=1, stride_d=0, stride_e=0)
    assert factor(**long) == UNSUPPORTED and solve(ldb=1 << 31, stride_b=0, **long) == UNSUPPORTED
    assert factor(uplo=LOWER, **long) == UNSUPPORTED and factor(**dict(long, ldd=63)) == ARG
    # 8. the grid: 2^31 workgroups of eight chains
    wide = dict(n=8, T=1, ldd=8, step_d=64, stride_d=64, E=None, lde=8, step_e=64, stride_e=64, batch=1 << 34)
    assert factor(**wide) == UNSUPPORTED and solve(ldb=8, stride_b=32, **wide) == UNSUPPORTED
    # 9. nothing to do: no launch, whatever the pointers
    assert factor(batch=0, D=None, E=None, info=None) == OK and factor(n=0, D=None, E=None, info=None, ldd=0, lde=0) == OK
    assert solve(nrhs=0, D=None, E=None, B=None) == OK and solve(T=0, D=None, E=None, B=None, ldb=0) == OK


def test_header_declares_the_symbols_with_the_ctypes_signatures(L):
    from capital_amd import _lib
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in NAMES:
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name + " is not declared"
        want = []
        for a in m.group(1).replace("\n", " ").split(","):
            a = a.strip()
            want.append(C.c_void_p if "*" in a else kinds[a.replace("const ", "").split()[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and list(args) == want, (name, args, want)
        assert getattr(L, name).argtypes == want
    section = header[header.index("csrc/blocktri_batched.hip"):]
    for s in ("THE BIT CONTRACT IS A COMPOSITION", "CONSEQUENCES", "Argument rules, in this order", "ONE launch per call", "Position T - 1", "half = 1",
              "fma(beta, d, t)", "2^31 - 1"):
        assert s in section, s
    with open(os.path.join(ROOT, "capital_amd", "csrc", "blocktri_batched.hip")) as f:
        head = f.read().split("#include", 1)[0]
    for s in ("THE ARITHMETIC IS A COMPOSITION", "HOW THE BLOCKS TRAVEL", "blocktri_addr.h", "out of scope", "pb_factor_step", "pb_forward_step"):
        assert s in head, s


def test_python_layer_names_and_refusals():
    import torch
    from capital_amd import _lib, batched, lapack
    for fn in (lapack.engine._potrf_blocktri_batched, lapack.engine._potrs_blocktri_batched):
        assert callable(fn) and "64" in fn.__doc__
    for fn in (batched.blocktri_potrf, batched.blocktri_potrs):
        assert callable(fn) and "torch.linalg.cholesky" in fn.__doc__ and "L_(i+1, i)" in fn.__doc__ and "lower triangle" in fn.__doc__.lower()
    assert "blocktri_potrf" in batched.__doc__
    assert len({int(m) for m in lapack.Method}) == len(list(lapack.Method))
    col = lapack.ArgPack_potrf_blocktri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    row = lapack.ArgPack_potrf_blocktri_batched(lapack.Order.AlapackRowMajor, lapack.UpLo.AlapackUpper)
    srow = lapack.ArgPack_potrs_blocktri_batched(lapack.Order.AlapackRowMajor, lapack.UpLo.AlapackUpper)
    scol = lapack.ArgPack_potrs_blocktri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper, half=2)
    assert scol.half == 2 and srow.half == 0
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        lapack.engine._potrf_blocktri_batched(None, None, 4, 2, 4, 16, 32, 4, 16, 16, 1, row)
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        lapack.engine._potrs_blocktri_batched(None, None, None, 4, 2, 1, 4, 16, 32, 4, 16, 16, 8, 8, 1, None, srow)
    with pytest.raises(_lib.CapitalError, match="64"):
        lapack.engine._potrf_blocktri_batched(None, None, 65, 2, 65, 65 * 65, 2 * 65 * 65, 65, 65 * 65, 65 * 65, 1, col)
    with pytest.raises(_lib.CapitalError, match="64"):
        lapack.engine._potrs_blocktri_batched(None, None, None, 65, 2, 1, 65, 65 * 65, 2 * 65 * 65, 65, 65 * 65, 65 * 65, 130, 130, 1, None, scol)
    D, E, B = torch.zeros(2, 3, 4, 4, dtype=torch.float64), torch.zeros(2, 2, 4, 4, dtype=torch.float64), torch.zeros(2, 12, dtype=torch.float64)
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        batched.blocktri_potrf(D, E)
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        batched.blocktri_potrs(D, E, B)
    with pytest.raises(_lib.CapitalError, match="half"):
        batched.blocktri_potrs(D, E, B, half="both")
    for bad in (lambda: batched.blocktri_potrf(None, None), lambda: batched.blocktri_potrs(None, None, None)):
        with pytest.raises(_lib.CapitalError):
            bad()


def test_every_kernel_instance_lives_in_registers(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR, for the factor and the solve at NP = 8, 16, 32, 64"""
    from capital_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if re.search(r"\d+blocktri_potr[fs]_kernelI", k)}
    assert len(res) == 8, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
        assert int(v["LDS Size"]) <= 64 * 1024, (k, v)
    for name in ("blocktri_potrf_kernel", "blocktri_potrs_kernel"):
        assert name in build.NO_SCRATCH


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
        assert all(k.startswith("K ") and "blocktri_potr" in k for k in x["launches"]), x["launches"]
        for name, lines in x["per_call"]:
            assert len(lines) == 1 and lines[0].startswith("K "), (x["name"], name, lines)       # one launch and nothing else
        assert x["empty_calls"] == []
        assert x["coverage"] == [], x["coverage"][:4]


def _marks(r):
    per, cur, empties, notes = [], None, [], []
    for l in r.lines:
        if l.startswith("MARK begin "):
            cur = (l[len("MARK begin "):], [], [])
        elif l.startswith("MARK end "):
            (empties if cur[0].startswith("empty") else per).append(cur[:2])
            notes.append((cur[0], cur[2]))
            cur = None
        elif cur is not None and l.startswith("A "):
            cur[2].append([int(v) for v in l.split()[1:9]])
        elif cur is not None and not l.startswith("ACC "):
            cur[1].append(l)
    return per, [e for e in empties if e[1]], notes


def _noted(notes):
    """{(alloc, mode-writes?)}: the bytes the notes of one call cover, per allocation: (read set, written set)"""
    rd, wr = {}, {}
    for mode, alloc, off, pitch, rb, cols, tri, elem in notes:
        for j in range(cols):
            s = off + j * pitch
            e = s + (min((j + 1) * elem, rb) if tri == 1 else rb)
            span = set(range(s, e, elem))
            if mode & 1:
                rd.setdefault(alloc, set()).update(span)
            if mode & 2:
                wr.setdefault(alloc, set()).update(span)
    return rd, wr


def _trace_main(out_path):
    """runs in a process of its own (no torch: the stand-in takes the place of the HIP runtime)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipshim"))
    sys.path.insert(0, ROOT)
    import run_scenarios as S
    from tests import blocktri_cases as BC
    results = []
    for user_stream in (0, 1):
        tag = " [user stream]" if user_stream else " [NULL stream]"
        for (n, T, batch, nrhs) in TRACE:
            row = (n, T, batch, nrhs, "gaps")
            ldd, step_d, stride_d, lde, step_e, stride_e, ldb, stride_b = BC.layout(row)
            r = S.Run("blocktri %d x %d%s" % (n, T, tag), user_stream)
            # the buffers end with the last element the kernels may touch: a note that reaches further is out of bounds
            dsz = (batch - 1) * stride_d + (T - 1) * step_d + (n - 1) * ldd + n
            esz = (batch - 1) * stride_e + (T - 2) * step_e + (n - 1) * lde + n if T > 1 else 1
            bsz = (batch - 1) * stride_b + (nrhs - 1) * ldb + T * n
            Dd, Ed, Bd, Id, Ld = S.dmalloc(8 * dsz), S.dmalloc(8 * esz), S.dmalloc(8 * bsz), S.dmalloc(4 * batch), S.dmalloc(8 * batch)
            E = Ed if T > 1 else None
            calls = [("factor", S.L.cap_dpotrf_blocktri_batched, UPPER, n, T, Dd, ldd, step_d, stride_d, E, lde, step_e, stride_e, Id, Ld, batch, r.stream),
                     ("factor no logdet", S.L.cap_dpotrf_blocktri_batched, UPPER, n, T, Dd, ldd, step_d, stride_d, E, lde, step_e, stride_e, Id, None, batch,
                      r.stream)]
            for half in (0, 1, 2):
                calls.append(("solve half=%d" % half, S.L.cap_dpotrs_blocktri_batched, UPPER, half, n, T, nrhs, Dd, ldd, step_d, stride_d, E, lde, step_e,
                              stride_e, Bd, ldb, stride_b, Id if half else None, batch, r.stream))
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty batch=0", S.L.cap_dpotrf_blocktri_batched, UPPER, n, T, None, ldd, step_d, stride_d, None, lde, step_e, stride_e, None, None, 0,
                       r.stream),
                      ("empty nrhs=0", S.L.cap_dpotrs_blocktri_batched, UPPER, 0, n, T, 0, Dd, ldd, step_d, stride_d, E, lde, step_e, stride_e, None, ldb,
                       stride_b, None, batch, r.stream)):
                S.ok(r.call(*c), c[0])
            res = r.finish()
            res["expected"] = len(calls)
            res["launches"] = [l for l in r.lines if l.startswith("K ")]
            res["per_call"], res["empty_calls"], notes = _marks(r)
            # what the sweep says is touched, in bytes from the start of each buffer
            tri = {8 * (c * stride_d + i * step_d + a + b * ldd) for c in range(batch) for i in range(T) for b in range(n) for a in range(b + 1)}
            full = {8 * (c * stride_e + i * step_e + a + b * lde) for c in range(batch) for i in range(T - 1) for b in range(n) for a in range(n)}
            rhs = {8 * (c * stride_b + k * ldb + a) for c in range(batch) for k in range(nrhs) for a in range(T * n)}
            cov = []
            for what, lines in notes:
                if what.startswith("empty"):
                    if lines:
                        cov.append((what, "notes for an empty call"))
                    continue
                rd, wr = _noted(lines)
                sets = sorted(set(rd) | set(wr))
                got = {"rd": sorted(sorted(v) for v in rd.values()), "wr": sorted(sorted(v) for v in wr.values())}
                if what.startswith("factor"):
                    want_rd = [sorted(tri)] + ([sorted(full)] if T > 1 else [])
                    want_wr = want_rd + [list(range(0, 4 * batch, 4))] + ([list(range(0, 8 * batch, 8))] if "no logdet" not in what else [])
                else:
                    want_rd = [sorted(tri)] + ([sorted(full)] if T > 1 else []) + [sorted(rhs)] + ([list(range(0, 4 * batch, 4))] if "half=0" not in what else [])
                    want_wr = [sorted(rhs)]
                if got["rd"] != sorted(want_rd) or got["wr"] != sorted(want_wr):
                    cov.append((what, len(sets), [len(v) for v in got["rd"]], [len(v) for v in want_rd], [len(v) for v in got["wr"]], [len(v) for v in want_wr]))
            res["coverage"] = cov
            for q in (Dd, Ed, Bd, Id, Ld):
                S.shim.hipFree(q)
            results.append(res)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
