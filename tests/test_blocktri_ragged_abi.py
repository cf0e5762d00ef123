"""CPU-only: argument handling of the ragged block-tridiagonal entries (cap_blocktri_plan_*, cap_dpotrf_blocktri_vbatched,
cap_dpotrs_blocktri_vbatched, cap_dpotri_blocktri_vbatched) - the plan and entry rules of include/capital_amd.h in their stated order,
with pointers that are never dereferenced - _info and _order (T descending, stable), the header / ctypes agreement, the Python and engine
names and refusals, and the compiler's resource remarks of the twelve kernel instances.  The last test drives the three entries through
the recording stand-in of tests/hipshim in a process of its own (this file run as a script): exactly one annotated launch per call and
nothing else, nothing for an empty call, and the access notes cover EXACTLY what tests/test_blocktri_ragged_addr.py's sweep says the
kernels touch: the plan's records and list, the upper triangles (full blocks under fill) of the owned D slots, the owned coupling slots
of E, the right-hand-side segments, and the info / logdet entries of the chains that have a position."""
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
BATCH, SLOTS, ESLOTS, ROWS, TMAX = range(5)
NAMES = ("cap_blocktri_plan_create", "cap_blocktri_plan_destroy", "cap_blocktri_plan_order", "cap_dpotrf_blocktri_vbatched",
         "cap_dpotrs_blocktri_vbatched", "cap_dpotri_blocktri_vbatched")
TRACE = (0, 1, 4, 8, 10)                 # rows of tests/blocktri_ragged_cases.py: NP = 8 (two of them), 16, 64 (two of them)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


PD, PE, PB, PI = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28), C.c_void_p(1 << 30)   # never dereferenced


def arr(seq):
    return (C.c_int64 * max(len(seq), 1))(*seq)


def make(L, T, first=None, status=OK):
    p = C.c_void_p()
    st = L.cap_blocktri_plan_create(len(T), arr(T), arr(first) if first is not None else None, C.byref(p))
    assert st == status, (st, status, T, first)
    assert bool(p) == (status == OK)
    return p


def test_plan_rules_info_and_order(L):
    p = C.c_void_p()
    # 1.
    assert L.cap_blocktri_plan_create(1, arr([1]), None, None) == ARG
    assert L.cap_blocktri_plan_create(-1, arr([1]), None, C.byref(p)) == ARG and not p
    assert L.cap_blocktri_plan_create(2, None, None, C.byref(p)) == ARG and not p
    assert L.cap_blocktri_plan_create(-1, None, None, None) == ARG
    # 2. negative entries - before the overlap
    make(L, [3, -1], status=ARG)
    make(L, [3, 2], [0, -1], status=ARG)
    make(L, [3, -1], [0, 0], status=ARG)
    # 3. slot ranges that meet, whatever the batch order; empty chains meet nobody
    make(L, [3, 2], [0, 2], status=ARG)
    make(L, [2, 3], [2, 0], status=ARG)
    make(L, [3, 3], [5, 5], status=ARG)
    # 4. sums beyond int64
    make(L, [1 << 62, 1 << 62], status=ARG)
    make(L, [2], [(1 << 63) - 2], status=ARG)
    for T, first, want in (([3, 0, 2], [0, 1, 3], (3, 5, 4, 5, 3)), ([3, 0, 1, 2, 5, 4, 7, 6], None, (8, 28, 27, 28, 7)), ([], None, (0, 0, 0, 0, 0)),
                           ([0, 0], [9, 9], (2, 0, 0, 0, 0)), ([1, 1, 1], [4, 0, 2], (3, 5, 0, 3, 1)), ([2, 1], [5, 0], (2, 7, 6, 3, 2))):
        q = make(L, T, first)
        assert tuple(L.cap_blocktri_plan_info(q, w) for w in range(5)) == want, (T, first)
        assert L.cap_blocktri_plan_info(q, 5) == -1 and L.cap_blocktri_plan_info(q, -1) == -1
        order = arr([0] * len(T))
        assert L.cap_blocktri_plan_order(q, order, len(T)) == OK
        assert list(order)[:len(T)] == sorted(range(len(T)), key=lambda c: -T[c])       # T descending, stable
        assert L.cap_blocktri_plan_order(q, None, 1) == ARG and L.cap_blocktri_plan_order(q, order, -1) == ARG
        assert L.cap_blocktri_plan_order(q, None, 0) == OK
        assert L.cap_blocktri_plan_destroy(q) == OK
    assert L.cap_blocktri_plan_info(None, BATCH) == -1 and L.cap_blocktri_plan_destroy(None) == OK and L.cap_blocktri_plan_order(None, None, 0) == ARG
    from tests import blocktri_ragged_cases as RC
    for row in RC.rows():
        q = make(L, list(row[1]), RC.first_slots(row[1], row[2]))
        first, _, slots, eslots, rows = RC.geometry(row)
        assert tuple(L.cap_blocktri_plan_info(q, w) for w in range(5)) == (len(row[1]), slots, eslots, rows, max(row[1]))
        order = arr([0] * len(row[1]))
        assert L.cap_blocktri_plan_order(q, order, len(row[1])) == OK and list(order) == RC.order(row[1])
        L.cap_blocktri_plan_destroy(q)


def calls(L, plan):
    def factor(p=plan, uplo=UPPER, n=9, D=PD, ldd=9, step_d=81, E=PE, lde=9, step_e=81, info=PI, logdet=None):
        return L.cap_dpotrf_blocktri_vbatched(p, uplo, n, D, ldd, step_d, E, lde, step_e, info, logdet, None)

    def solve(p=plan, uplo=UPPER, half=0, n=9, nrhs=4, D=PD, ldd=9, step_d=81, E=PE, lde=9, step_e=81, B=PB, ldb=54, info=None):
        return L.cap_dpotrs_blocktri_vbatched(p, uplo, half, n, nrhs, D, ldd, step_d, E, lde, step_e, B, ldb, info, None)

    def inverse(p=plan, uplo=UPPER, fill=0, n=9, D=PD, ldd=9, step_d=81, E=PE, lde=9, step_e=81, info=None):
        return L.cap_dpotri_blocktri_vbatched(p, uplo, fill, n, D, ldd, step_d, E, lde, step_e, info, None)
    return factor, solve, inverse


def test_entry_arguments_are_checked_in_the_documented_order(L):
    """a process without a device makes plans that describe only: every rule up to 9 is decided without one, rule 10 says so"""
    plan = make(L, [3, 0, 1, 2])                    # ROWS = 6, SLOTS = 6, ESLOTS = 5
    empty, zeros, single = make(L, []), make(L, [0, 0]), make(L, [1, 0, 1])
    last = HIP if not _has_device() else None       # with work to do and every rule passed
    factor, solve, inverse = calls(L, plan)
    big = dict(n=65, ldd=65, lde=65, step_d=65 * 65, step_e=65 * 65)
    for f, b in ((factor, big), (solve, dict(big, ldb=6 * 65)), (inverse, big)):
        # 1.
        assert f(p=None) == ARG and f(n=-1) == ARG and f(n=-1, uplo=LOWER) == ARG and f(p=None, D=None) == ARG
        # 2. NULL pointers with something to launch; E only while some chain has T > 1
        assert f(D=None) == ARG and f(E=None) == ARG and f(D=None, uplo=LOWER) == ARG and f(D=None, **b) == ARG
        assert f(p=empty, D=None, E=None) == OK and f(p=zeros, D=None, E=None) == OK and f(n=0, D=None, E=None, ldd=0, lde=0) == OK
        if last is not None:
            assert f(p=single, E=None, lde=0, step_e=0) == last
        # 3. the layout, in 128-bit arithmetic
        assert f(ldd=8) == ARG and f(lde=8) == ARG and f(step_d=80) == ARG and f(step_e=80) == ARG and f(step_d=-1) == ARG
        assert f(ldd=8, uplo=LOWER) == ARG and f(ldd=64, **{k: v for k, v in b.items() if k != "ldd"}) == ARG
        assert f(ldd=1 << 62, lde=1 << 62, step_d=1 << 62, step_e=1 << 62) == ARG                # 9 x 2^62 does not wrap
        assert f(p=single, lde=0, step_e=0, uplo=LOWER) == UNSUPPORTED          # no chain has two positions: E is not looked at
        assert f(p=single, ldd=8) == ARG
        # 5. uplo, 6. n - in that order
        assert f(uplo=LOWER) == UNSUPPORTED and f(uplo=LOWER, **b) == UNSUPPORTED and f(**b) == UNSUPPORTED and f(p=empty, **b) == UNSUPPORTED
        # 10. a plan without a device
        if last is not None:
            assert f() == last
    assert factor(info=None) == ARG and factor(info=None, p=zeros) == OK
    assert solve(nrhs=-1) == ARG and solve(B=None) == ARG and solve(B=None, nrhs=0) == OK and solve(ldb=53) == ARG and solve(ldb=53, nrhs=0) == ARG
    # 4. half / fill after the layout, before uplo
    assert solve(half=3) == ARG and solve(half=-1) == ARG and solve(half=3, ldb=53) == ARG and solve(half=3, uplo=LOWER) == ARG
    assert inverse(fill=2) == ARG and inverse(fill=-1) == ARG and inverse(fill=2, uplo=LOWER) == ARG and inverse(fill=2, **big) == ARG
    # 7. n TMAX > 2^31 - 1
    long = make(L, [1 << 25, 3])
    kw = dict(p=long, n=64, ldd=64, lde=64, step_d=4096, step_e=4096)
    assert factor(**kw) == UNSUPPORTED and inverse(**kw) == UNSUPPORTED and solve(ldb=64 * ((1 << 25) + 3), **kw) == UNSUPPORTED
    assert factor(uplo=LOWER, **kw) == UNSUPPORTED and factor(**dict(kw, ldd=63)) == ARG
    assert solve(ldb=64 * ((1 << 25) + 3) - 1, **kw) == ARG
    # 9. nothing to do: no launch, whatever the pointers
    assert factor(p=empty, D=None, E=None, info=None) == OK and solve(nrhs=0, D=None, E=None, B=None) == OK
    assert inverse(n=0, D=None, E=None, ldd=0, lde=0) == OK and solve(p=zeros, D=None, E=None, B=None, ldb=0) == OK
    for q in (plan, empty, zeros, single, long):
        L.cap_blocktri_plan_destroy(q)


def _has_device():
    import torch
    return torch.cuda.is_available()


def test_header_declares_the_symbols_with_the_ctypes_signatures(L):
    from capital_amd import _lib
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in NAMES + ("cap_blocktri_plan_info",):
        m = re.search(r"^(int|int64_t)\s+%s\(([^;]*)\);" % name, header, re.M)
        assert m, name + " is not declared"
        want = []
        for a in m.group(2).replace("\n", " ").split(","):
            a = a.strip()
            if a.endswith("**") or "** " in a:
                want.append(C.POINTER(C.c_void_p))
            elif "int64_t*" in a:
                want.append(C.POINTER(C.c_int64))
            else:
                want.append(C.c_void_p if "*" in a else kinds[a.replace("const ", "").split()[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)] and list(args) == want, (name, args, want)
        assert getattr(L, name).argtypes == want
    assert re.search(r"CAP_BLOCKTRI_BATCH = 0, CAP_BLOCKTRI_SLOTS = 1, CAP_BLOCKTRI_ESLOTS = 2, CAP_BLOCKTRI_ROWS = 3, CAP_BLOCKTRI_TMAX = 4", header)
    section = header[header.index("csrc/blocktri_vbatched.hip"):]
    for s in ("bit for bit", "MAY SYNCHRONISE", "Argument rules, in this order", "ONE launch per call", "STABLY BY T DESCENDING", "never addressed",
              "NOT written", "2^31 - 1", "without a device"):
        assert s in section, s
    with open(os.path.join(ROOT, "capital_amd", "csrc", "blocktri_vbatched.hip")) as f:
        head = f.read().split("#include", 1)[0]
    for s in ("THE BIT CONTRACT", "WHO IS ALIVE AT A STEP", "blocktri_addr.h", "SELECTION", "pb_factor_step", "pi_invert"):
        assert s in head, s


def test_python_layer_names_and_refusals():
    import torch
    from capital_amd import _lib, batched, lapack
    for fn in (lapack.engine._potrf_blocktri_vbatched, lapack.engine._potrs_blocktri_vbatched, lapack.engine._potri_blocktri_vbatched):
        assert callable(fn) and "one launch" in fn.__doc__ and "_vbatched" in fn.__doc__
    for fn in (batched.VarChains.potrf, batched.VarChains.potrs, batched.VarChains.potri):
        assert "ONE launch" in fn.__doc__ and "alone" in fn.__doc__
    assert "BIT FOR BIT" in batched.VarChains.__doc__ and "Never touched" in batched.VarChains.__doc__ and "VarChains" in batched.__doc__
    row = lapack.ArgPack_potrf_blocktri_batched(lapack.Order.AlapackRowMajor, lapack.UpLo.AlapackUpper)
    col = lapack.ArgPack_potrf_blocktri_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        lapack.engine._potrf_blocktri_vbatched(None, None, None, 4, 4, 16, 4, 16, 1, row)
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        lapack.engine._potrs_blocktri_vbatched(None, None, None, None, 4, 1, 4, 16, 4, 16, 8, 1, None, row)
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        lapack.engine._potri_blocktri_vbatched(None, None, None, 4, 4, 16, 4, 16, 1, None, row)
    with pytest.raises(_lib.CapitalError, match="64"):
        lapack.engine._potrf_blocktri_vbatched(None, None, None, 65, 65, 65 * 65, 65, 65 * 65, 1, col)
    with pytest.raises(_lib.CapitalError, match="64"):
        lapack.engine._potri_blocktri_vbatched(None, None, None, 65, 65, 65 * 65, 65, 65 * 65, 1, None, col)
    for bad in (lambda: batched.VarChains([3, -1]), lambda: batched.VarChains([3, 2], [0, 2]), lambda: batched.VarChains([3, 2], [0])):
        with pytest.raises(_lib.CapitalError):
            bad()
    vc = batched.VarChains([3, 0, 1, 2], [4, 0, 0, 1])
    assert (vc.lengths, vc.first, vc.row_offsets) == ((3, 0, 1, 2), (4, 0, 0, 1), (0, 3, 3, 4))
    assert (vc.slots, vc.eslots, vc.rows, vc.tmax, vc.order, vc.batch) == (7, 6, 6, 3, (0, 3, 2, 1), 4)
    assert batched.VarChains([2, 1]).first == (0, 2)
    D, E, B = torch.zeros(7, 4, 4, dtype=torch.float64), torch.zeros(7, 4, 4, dtype=torch.float64), torch.zeros(24, dtype=torch.float64)
    assert tuple(vc.chain(D, 0).shape) == (3, 4, 4) and vc.chain(D, 0).data_ptr() == D[4].data_ptr() and vc.chain(D, 1).shape[0] == 0
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        vc.potrf(D, E)
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        vc.potrs(D, E, B)
    with pytest.raises(_lib.CapitalError, match="no CPU path"):
        vc.potri(D, E)
    with pytest.raises(_lib.CapitalError, match="half"):
        vc.potrs(D, E, B, half="both")
    with pytest.raises(_lib.CapitalError):
        vc.pack([(D[:3], E[:2])])


def test_every_kernel_instance_lives_in_registers(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR for the twelve instances; the factor and the solve
    within 64 KiB of static LDS, the inverse dynamic; no instance below the occupancy class of its fixed-size twin"""
    from capital_amd import build
    all_res = build.kernel_resources()
    res = {k: v for k, v in all_res.items() if re.search(r"\d+blocktri_vpotr[fsi]_kernelI", k)}
    assert len(res) == 12, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
        if "vpotri" in k:
            assert int(v["LDS Size"]) == 0, (k, v)                 # dynamic: 8 (G image + 2 areas + table) <= 84.75 KiB, asked for at the launch
        else:
            assert 0 < int(v["LDS Size"]) <= 64 * 1024, (k, v)
        m = re.search(r"\d+blocktri_v(potr[fsi])_kernelILi(\d+)E", k)
        twin = [w for q, w in all_res.items() if re.search(r"\d+blocktri_%s_kernelILi%sE" % (m.group(1), m.group(2)), q)]
        assert len(twin) == 1 and int(v["Occupancy"]) >= int(twin[0]["Occupancy"]), (k, v["Occupancy"], twin)
    for name in ("blocktri_vpotrf_kernel", "blocktri_vpotrs_kernel", "blocktri_vpotri_kernel"):
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
        assert all(k.startswith("K ") and "blocktri_vpotr" in k for k in x["launches"]), x["launches"]
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
    from tests import blocktri_ragged_cases as RC
    results = []
    for user_stream in (0, 1):
        tag = " [user stream]" if user_stream else " [NULL stream]"
        for k in TRACE:
            row = RC.ROWS[k]
            n, lengths, mode, nrhs, _ = row
            batch = len(lengths)
            first, rows_at, slots, eslots, rows = RC.geometry(row)
            ld, step, ldb = RC.layout(row)
            plan = C.c_void_p()
            fs = RC.first_slots(lengths, mode)
            S.ok(S.L.cap_blocktri_plan_create(batch, arr(list(lengths)), arr(fs) if fs is not None else None, C.byref(plan)), "plan")
            r = S.Run("ragged blocktri row %d%s" % (k, tag), user_stream)
            # the buffers end with the last element the kernels may touch: a note that reaches further is out of bounds
            dsz = (slots - 1) * step + (n - 1) * ld + n
            esz = (eslots - 1) * step + (n - 1) * ld + n if eslots else 1
            bsz = (nrhs - 1) * ldb + rows * n
            Dd, Ed, Bd, Id, Ld = S.dmalloc(8 * dsz), S.dmalloc(8 * esz), S.dmalloc(8 * bsz), S.dmalloc(4 * batch), S.dmalloc(8 * batch)
            E = Ed if eslots else None
            calls = [("factor", S.L.cap_dpotrf_blocktri_vbatched, plan, UPPER, n, Dd, ld, step, E, ld, step, Id, Ld, r.stream),
                     ("factor no logdet", S.L.cap_dpotrf_blocktri_vbatched, plan, UPPER, n, Dd, ld, step, E, ld, step, Id, None, r.stream)]
            for half in (0, 1, 2):
                calls.append(("solve half=%d" % half, S.L.cap_dpotrs_blocktri_vbatched, plan, UPPER, half, n, nrhs, Dd, ld, step, E, ld, step, Bd, ldb,
                              Id if half else None, r.stream))
            for fill in (0, 1):
                calls.append(("inverse fill=%d" % fill, S.L.cap_dpotri_blocktri_vbatched, plan, UPPER, fill, n, Dd, ld, step, E, ld, step,
                              Id if fill else None, r.stream))
            for c in calls:
                S.ok(r.call(*c), c[0])
            for c in (("empty n=0", S.L.cap_dpotrf_blocktri_vbatched, plan, UPPER, 0, None, 0, 0, None, 0, 0, None, None, r.stream),
                      ("empty nrhs=0", S.L.cap_dpotrs_blocktri_vbatched, plan, UPPER, 0, n, 0, Dd, ld, step, E, ld, step, None, ldb, None, r.stream)):
                S.ok(r.call(*c), c[0])
            res = r.finish()
            res["expected"] = len(calls)
            res["launches"] = [l for l in r.lines if l.startswith("K ")]
            res["per_call"], res["empty_calls"], notes = _marks(r)
            # what the sweep says is touched, in bytes from the start of each buffer
            own = [(first[c] + i, i + 1 < lengths[c]) for c in range(batch) for i in range(lengths[c])]
            tri = {8 * (s * step + a + b * ld) for s, _ in own for b in range(n) for a in range(b + 1)}
            blk = {8 * (s * step + a + b * ld) for s, _ in own for b in range(n) for a in range(n)}
            cpl = {8 * (s * step + a + b * ld) for s, nxt in own if nxt for b in range(n) for a in range(n)}
            rhs = {8 * (kk * ldb + (rows_at[c] + i) * n + a) for c in range(batch) for i in range(lengths[c]) for kk in range(nrhs) for a in range(n)}
            live = [c for c in range(batch) if lengths[c] > 0]
            plan_rd = [list(range(0, 24 * batch, 8)), list(range(0, 8 * batch, 8))]
            i4, l8 = [4 * c for c in live], [8 * c for c in live]
            e_rd = [sorted(cpl)] if cpl else []
            cov = []
            for what, lines in notes:
                if what.startswith("empty"):
                    if lines:
                        cov.append((what, "notes for an empty call"))
                    continue
                rd, wr = _noted(lines)
                got = {"rd": sorted(sorted(v) for v in rd.values()), "wr": sorted(sorted(v) for v in wr.values())}
                if what.startswith("factor"):
                    want_rd = plan_rd + [sorted(tri)] + e_rd
                    want_wr = [sorted(tri)] + e_rd + [i4] + ([l8] if "no logdet" not in what else [])
                elif what.startswith("solve"):
                    want_rd = plan_rd + [sorted(tri)] + e_rd + [sorted(rhs)] + ([i4] if "half=0" not in what else [])
                    want_wr = [sorted(rhs)]
                else:
                    d = blk if "fill=1" in what else tri
                    want_rd = plan_rd + [sorted(d)] + e_rd + ([i4] if "fill=1" in what else [])
                    want_wr = [sorted(d)] + e_rd
                if got["rd"] != sorted(want_rd) or got["wr"] != sorted(want_wr):
                    cov.append((what, [len(v) for v in got["rd"]], [len(v) for v in want_rd], [len(v) for v in got["wr"]], [len(v) for v in want_wr]))
            res["coverage"] = cov
            for q in (Dd, Ed, Bd, Id, Ld):
                S.shim.hipFree(q)
            S.L.cap_blocktri_plan_destroy(plan)
            results.append(res)
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
