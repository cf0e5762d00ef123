"""CPU-only: argument handling of the batched pivoted Cholesky factorization (cap_dpstrf_batched, cap_dpstrf_vbatched,
csrc/pstrf_batched.hip) - the argument rules of include/capital_amd.h in their order, every case decided before the library touches a
device - the header / ctypes agreement, the Python names and refusals, and the compiler's resource remarks of every new kernel instance.
The last test drives the entries through the recording stand-in of tests/hipshim in a process of its own (this file run as a script):
ONE launch for the fixed-size call, one per occurring size class on a plan, none for an empty call or a refused one, every launch
annotated, no finding."""
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
NAN = float("nan")
TRACE_N = (1, 8, 9, 33, 64)
TRACE_LISTS = {"EVERY": tuple((7 * i) % 65 for i in range(65)), "WAVES": tuple((5, 6, 7, 8)[i % 4] for i in range(70)) + (9, 40),
               "ONE_CLASS": (20,) * 5, "LONE1": (1,)}
NAMES = ("cap_dpstrf_batched", "cap_dpstrf_vbatched")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        from capital_amd import build
        build.build(verbose=False)
    from capital_amd import _lib
    return _lib.lib()


A_ = C.c_void_p(1 << 20)                 # never dereferenced: every call below returns before any device work
R_ = C.c_void_p(1 << 24)
P_ = C.c_void_p(1 << 28)
K_ = C.c_void_p(1 << 32)
O_ = C.c_void_p(1 << 36)


def arr(a):
    return None if a is None else (C.c_int64 * max(len(a), 1))(*a)


def test_fixed_size_arguments_are_checked_in_the_documented_order(L):
    def call(uplo=UPPER, n=10, max_rank=4, tol=-1.0, A=A_, lda=10, stride_a=100, R=R_, ldr=4, stride_r=40, piv=P_, rank=K_, resid=O_, logdet=None,
             info=None, batch=5):
        return L.cap_dpstrf_batched(uplo, n, max_rank, tol, A, lda, stride_a, R, ldr, stride_r, piv, rank, resid, logdet, info, batch, None)
    big = dict(n=65, max_rank=65, lda=65, stride_a=65 * 65, ldr=65, stride_r=65 * 65)
    # 1. negative sizes, max_rank > n, a NaN tol - in front of everything else
    for kw in (dict(n=-1, max_rank=0), dict(batch=-1), dict(max_rank=-1), dict(max_rank=11), dict(tol=NAN), dict(n=0, max_rank=1)):
        assert call(uplo=LOWER, **kw) == ARG and call(A=None, **kw) == ARG, kw
    assert call(tol=NAN, **big) == ARG and call(batch=0, tol=NAN) == ARG
    # 2. NULL pointers with work to do, leading dimensions and strides
    for kw in (dict(A=None), dict(piv=None), dict(rank=None), dict(R=None), dict(lda=9), dict(stride_a=99), dict(ldr=3), dict(stride_r=39),
               dict(stride_a=-1), dict(lda=12, stride_a=119), dict(ldr=6, stride_r=59)):
        assert call(uplo=LOWER, **kw) == ARG, kw
        assert call(**dict(big, **{k: (v if v is None else 64) for k, v in kw.items()})) == ARG, kw
    assert call(R=None, max_rank=0, ldr=0, stride_r=0, uplo=LOWER) == UNSUPPORTED          # nothing of R is addressed
    assert call(resid=None, logdet=None, info=None, uplo=LOWER) == UNSUPPORTED              # optional outputs
    assert call(stride_a=0, stride_r=0, batch=1, uplo=LOWER) == UNSUPPORTED                 # one block needs no stride
    assert call(A=None, R=None, piv=None, rank=None, batch=0) == OK and call(A=None, R=None, piv=None, rank=None, n=0, max_rank=0, lda=0) == OK
    assert call(lda=9, batch=0) == ARG and call(ldr=3, batch=0) == ARG                      # the operand rule does not wait for work
    assert call(n=1 << 30, max_rank=1, lda=1 << 40, stride_a=1 << 62, ldr=1, stride_r=1 << 29) == ARG      # the clipped product
    # 3. LOWER comes before the size limit and the empty case
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=7, n=0, max_rank=0) == UNSUPPORTED and call(uplo=LOWER, batch=0) == UNSUPPORTED
    # 4. n > 64, the grid
    assert call(**big) == UNSUPPORTED and call(batch=0, **big) == UNSUPPORTED and call(uplo=LOWER, **big) == UNSUPPORTED
    n64 = dict(n=64, max_rank=64, lda=64, stride_a=64 * 64, ldr=64, stride_r=64 * 64)
    assert call(batch=1 << 31, **n64) == UNSUPPORTED and call(batch=(1 << 34), n=8, max_rank=8, lda=8, stride_a=64, ldr=8, stride_r=64) == UNSUPPORTED
    # 5. nothing to do
    assert call(n=0, max_rank=0) == OK and call(batch=0) == OK and call(batch=0, **n64) == OK
    for sz in (1, 8, 9, 64):
        kw = dict(n=sz, max_rank=sz, lda=sz, stride_a=sz * sz, ldr=sz, stride_r=sz * sz)
        assert call(batch=0, **kw) == OK and call(**dict(kw, lda=sz - 1)) == ARG and call(uplo=LOWER, **kw) == UNSUPPORTED


def create(L, n):
    p = C.c_void_p()
    assert L.cap_vbatch_plan_create(len(n), arr(n), None, None, C.byref(p)) == OK
    return p


def test_plan_entry_arguments_are_checked_in_the_documented_order(L):
    """no call here reaches a launch: in a process without a device the accepted calls on a non-empty plan end in CAP_ERR_HIP"""
    p, p65, p0, p1 = create(L, [5, 0, 64]), create(L, [5, 65]), create(L, [0, 0, 0]), create(L, [])

    def call(p=p, uplo=UPPER, max_rank=4, tol=-1.0, A=A_, R=R_, piv=P_, rank=K_, resid=O_, logdet=None, info=None):
        return L.cap_dpstrf_vbatched(p, uplo, max_rank, tol, A, R, piv, rank, resid, logdet, info, None)
    assert call(p=None, uplo=LOWER) == ARG and call(max_rank=-1, uplo=LOWER) == ARG and call(tol=NAN, p=p65) == ARG and call(tol=NAN, p=p0) == ARG
    for kw in (dict(A=None), dict(piv=None), dict(rank=None), dict(R=None)):
        assert call(uplo=LOWER, **kw) == ARG and call(p=p65, **kw) == ARG, kw
    assert call(R=None, max_rank=0, uplo=LOWER) == UNSUPPORTED
    assert call(uplo=LOWER) == UNSUPPORTED and call(uplo=LOWER, p=p65) == UNSUPPORTED and call(uplo=LOWER, p=p0) == UNSUPPORTED
    assert call(p=p65) == UNSUPPORTED and call(p=p65, max_rank=0, R=None) == UNSUPPORTED
    for q in (p0, p1):
        assert call(p=q, A=None, R=None, piv=None, rank=None, resid=None) == OK
    assert call(max_rank=1 << 40, uplo=LOWER) == UNSUPPORTED                               # a cap above every n_i is legal
    import torch
    if not torch.cuda.is_available():
        assert call() == HIP and call(max_rank=1 << 40) == HIP and call(max_rank=0, R=None) == HIP      # a plan made without a device
    for q in (p, p65, p0, p1):
        L.cap_vbatch_plan_destroy(q)


def test_header_declares_the_symbols_with_the_ctypes_signatures(L):
    from capital_amd import _lib
    with open(os.path.join(ROOT, "include", "capital_amd.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name in NAMES:
        m = re.search(r"^(int|int64_t) %s\(([^;]*)\);" % name, header, re.M)
        assert m, name + " is not declared"
        want = []
        for a in m.group(2).replace("\n", " ").split(","):
            a = a.strip()
            want.append(C.c_void_p if "*" in a else kinds[a.replace("const ", "").split()[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)] and list(args) == want, (name, args, want)
        assert getattr(L, name).argtypes == want
    section = header[header.index("csrc/pstrf_batched.hip"):]
    for s in ("THE BIT CONTRACT", "PLAN = FIXED", "THE STATED RECURRENCE", "R MUST NOT OVERLAP A", "Argument rules, in this order", "ONE launch",
              "fma(-W[i, p], W[i, c], t)", "is NOT the info"):
        assert s in section, s
    assert header.index("csrc/symm_batched.hip") < header.index("csrc/pstrf_batched.hip")
    with open(os.path.join(ROOT, "capital_amd", "csrc", "pstrf_batched.hip")) as f:
        head = f.read().split("#include", 1)[0]
    for s in ("THE BIT CONTRACT", "STOPPING", "wave-uniform", "fma(-w_i[p], w_i[c], t)"):
        assert s in head, s


def test_python_layer_names_and_refusals():
    import torch
    from capital_amd import _lib, batched, lapack
    for fn in (lapack.engine._pstrf_batched, lapack.engine._pstrf_vbatched):
        assert callable(fn) and "64" in fn.__doc__ and "factor_pivoted" in fn.__doc__
    for fn in (batched.pstrf, batched.VarBatch.pstrf):
        assert callable(fn) and "LOWER" in fn.__doc__ and "(info == 2).int()" in fn.__doc__ and "factor_pivoted" in fn.__doc__
    assert callable(batched.permute) and callable(batched.VarBatch.permute)
    assert len({int(m) for m in lapack.Method}) == len(list(lapack.Method))
    row = lapack.ArgPack_pstrf_batched(lapack.Order.AlapackRowMajor, lapack.UpLo.AlapackUpper)
    with pytest.raises(_lib.CapitalError, match="AlapackColumnMajor"):
        lapack.engine._pstrf_batched(None, None, None, 4, 4, 4, 16, 4, 16, 1, -1.0, row)
    col = lapack.ArgPack_pstrf_batched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    with pytest.raises(_lib.CapitalError, match="factor_pivoted"):
        lapack.engine._pstrf_batched(None, None, None, 65, 65, 65, 65 * 65, 65, 65 * 65, 1, -1.0, col)
    vcol = lapack.ArgPack_pstrf_vbatched(lapack.Order.AlapackColumnMajor, lapack.UpLo.AlapackUpper)
    with pytest.raises(_lib.CapitalError, match="factor_pivoted"):
        lapack.engine._pstrf_vbatched(None, None, None, None, 70, 65, 65, 2, -1.0, vcol)
    a = torch.zeros(3, 10, 10, dtype=torch.float64)
    vb = batched.VarBatch([3, 5])
    with pytest.raises(_lib.CapitalError, match="^A must"):                   # no CPU path
        batched.pstrf(a)
    with pytest.raises(_lib.CapitalError, match="factor_pivoted"):
        batched.VarBatch([3, 65]).pstrf(torch.zeros(3 * 3 + 65 * 65, dtype=torch.float64))
    for bad in (lambda: batched.pstrf(None), lambda: batched.pstrf(a.to(torch.float32)), lambda: vb.pstrf(torch.zeros(34, dtype=torch.float64)),
                lambda: vb.pstrf(None), lambda: batched.permute(a, None), lambda: batched.permute(a[:, 0], torch.zeros(3, 9, dtype=torch.int64)),
                lambda: vb.permute(torch.zeros(7, dtype=torch.float64), torch.zeros(8, dtype=torch.int64))):
        with pytest.raises(_lib.CapitalError):
            bad()
    piv = torch.tensor([[2, 0, 1], [0, 1, 2]])                                # permute is torch only: it runs wherever its tensors live
    b = torch.tensor([[10.0, 20.0, 30.0], [1.0, 2.0, 3.0]], dtype=torch.float64)
    f = batched.permute(b, piv)
    assert f.tolist() == [[30.0, 10.0, 20.0], [1.0, 2.0, 3.0]] and torch.equal(batched.permute(f, piv, inverse=True), b)
    b3 = torch.stack([b, -b], dim=1)
    assert torch.equal(batched.permute(batched.permute(b3, piv), piv, inverse=True), b3) and torch.equal(batched.permute(b3, piv)[:, 1], -f)
    sp = torch.tensor([2, 0, 1, 4, 3, 2, 1, 0])
    s = torch.arange(8.0, dtype=torch.float64)
    g = vb.permute(s, sp)
    assert g.tolist() == [2.0, 0.0, 1.0, 7.0, 6.0, 5.0, 4.0, 3.0] and torch.equal(vb.permute(g, sp, inverse=True), s)


def test_every_new_kernel_instance_keeps_its_column_in_registers(L):
    """the compiler's resource remarks of the last build: no scratch, no spilled VGPR - 4 NP x (fixed size, plan)"""
    from capital_amd import build
    res = {k: v for k, v in build.kernel_resources().items() if re.search(r"\d+pstrf_v?batched_kernelI", k)}
    assert len(res) == 4 * 2, sorted(res)
    for k, v in res.items():
        assert int(v["ScratchSize"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
    for name in ("pstrf_batched_kernel", "pstrf_vbatched_kernel"):
        assert name in build.NO_SCRATCH


def test_the_stated_launch_counts_on_the_recording_stand_in(tmp_path):
    """the fixed-size entry at n = 1, 8, 9, 33, 64, the plan entry on four size lists; the caller on the NULL stream and on a stream of its own"""
    from capital_amd import build
    build.build(verbose=False)
    out = tmp_path / "trace.json"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    res = json.load(open(out))
    assert len(res) == 2 * (len(TRACE_N) + len(TRACE_LISTS))
    for x in res:
        assert not x["findings"], (x["name"], x["findings"][:4])
        assert x["stats"]["kernels"] == x["expected"] and not x["stats"].get("unannotated"), (x["name"], x["stats"], x["expected"])
        assert x["stats"]["oob"] == 0 and x["stats"].get("races", 0) == 0
        assert all(k.startswith("K ") and "pstrf_" in k and "batched_kernel" in k for k in x["launches"]), x["launches"]
        for (name, lines), want in zip(x["per_call"], x["per_launches"]):
            assert len(lines) == want and all(l.startswith("K ") for l in lines), (x["name"], name, lines, want)   # launches and nothing else
        assert len(x["per_call"]) == len(x["per_launches"])
        assert x["empty_calls"] == []


def _marks(r):
    per, cur, empties = [], None, []
    for l in r.lines:                  # what the trace holds between the marks of one call
        if l.startswith("MARK begin "):
            cur = (l[len("MARK begin "):], [])
        elif l.startswith("MARK end "):
            (empties if cur[0].startswith(("empty", "refused")) else per).append(cur)
            cur = None
        elif cur is not None and not l.startswith(("ACC ", "A ")):
            cur[1].append(l)
    return per, [e for e in empties if e[1]]


def _trace_main(out_path):
    """runs in a process of its own (no torch: the stand-in takes the place of the HIP runtime)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipshim"))
    sys.path.insert(0, ROOT)
    import run_scenarios as S
    from tests import vbatched_cases as VC
    lib = S.L
    results = []

    def finish(r, want, bufs):
        out = r.finish()
        out["expected"], out["per_launches"] = sum(want), want
        out["launches"] = [l for l in r.lines if l.startswith("K ")]
        out["per_call"], out["empty_calls"] = _marks(r)
        for q in bufs:
            S.shim.hipFree(q)
        results.append(out)

    for user_stream in (0, 1):
        tag = " [user stream]" if user_stream else " [NULL stream]"
        for n in TRACE_N:
            r = S.Run("pstrf batched n=%d%s" % (n, tag), user_stream)
            batch, lda = 37, n + 1
            sa = lda * n + 3
            Ad, Rd = S.dmalloc(8 * sa * batch), S.dmalloc(8 * ((n + 2) * n + 5) * batch)
            piv, rank, resid, logdet, info = (S.dmalloc(8 * batch * (n + 1)) for _ in range(5))
            want = []
            for mr in sorted({n, n // 2, 0}):
                ldr = mr + 2
                S.ok(r.call("dpstrf_batched max_rank=%d" % mr, lib.cap_dpstrf_batched, 1, n, mr, -1.0, Ad, lda, sa, Rd, ldr, ldr * n + 5, piv, rank, resid,
                            logdet, info, batch, r.stream), "cap_dpstrf_batched")
                want.append(1)
            S.ok(r.call("dpstrf_batched rank alone", lib.cap_dpstrf_batched, 1, n, n, 0.5, Ad, lda, sa, Rd, n, n * n, piv, rank, None, None, None, batch,
                        r.stream), "cap_dpstrf_batched")
            S.ok(r.call("dpstrf_batched one block", lib.cap_dpstrf_batched, 1, n, n, -1.0, Ad, n, 0, Rd, n, 0, piv, rank, resid, None, info, 1, r.stream),
                 "cap_dpstrf_batched")
            S.ok(r.call("dpstrf_batched no R", lib.cap_dpstrf_batched, 1, n, 0, -1.0, Ad, n, n * n, None, 0, 0, piv, rank, resid, None, info, batch,
                        r.stream), "cap_dpstrf_batched")
            want += [1, 1, 1]
            for c in (("empty batch=0", lib.cap_dpstrf_batched, 1, n, n, -1.0, None, n, 0, None, n, 0, None, None, None, None, None, 0),
                      ("empty n=0", lib.cap_dpstrf_batched, 1, 0, 0, -1.0, None, 0, 0, None, 0, 0, None, None, None, None, None, batch)):
                S.ok(r.call(c[0], c[1], *c[2:], r.stream), c[0])
            for c, st in ((("refused n=65", lib.cap_dpstrf_batched, 1, 65, 65, -1.0, Ad, 65, 65 * 65, Rd, 65, 65 * 65, piv, rank, resid, logdet, info, 1), 4),
                          (("refused lower", lib.cap_dpstrf_batched, 0, n, n, -1.0, Ad, lda, sa, Rd, n, n * n, piv, rank, resid, logdet, info, batch), 4),
                          (("refused max_rank", lib.cap_dpstrf_batched, 1, n, n + 1, -1.0, Ad, lda, sa, Rd, n + 1, (n + 1) * n, piv, rank, resid, logdet,
                            info, batch), 1)):
                assert r.call(c[0], c[1], *c[2:], r.stream) == st, c[0]
            finish(r, want, (Ad, Rd, piv, rank, resid, logdet, info))
        for name, sizes in TRACE_LISTS.items():
            lay = VC.Layout(sizes, "gaps")
            plan, empty, big = C.c_void_p(), C.c_void_p(), C.c_void_p()
            S.ok(lib.cap_vbatch_plan_create(lay.batch, arr(list(lay.sizes)), None, arr(list(lay.off_arg)), C.byref(plan)), "cap_vbatch_plan_create")
            S.ok(lib.cap_vbatch_plan_create(3, arr([0, 0, 0]), None, None, C.byref(empty)), "cap_vbatch_plan_create")
            S.ok(lib.cap_vbatch_plan_create(2, arr([8, 65]), None, None, C.byref(big)), "cap_vbatch_plan_create")
            r = S.Run("pstrf vbatched %s%s" % (name, tag), user_stream)
            Ad, Rd = S.dmalloc(8 * max(lay.total, 65 * 65 + 64)), S.dmalloc(8 * max(lay.total, 65 * 65 + 64))
            piv, rank, resid, logdet, info = (S.dmalloc(8 * (lay.rows + lay.batch + 80)) for _ in range(5))
            classes = int(lib.cap_vbatch_plan_info(plan, 4))
            assert classes >= 1 and classes == len({VC.class_of(n) for n in sizes if n})
            want = []
            for mr in (64, 3, 0):
                S.ok(r.call("dpstrf_vbatched max_rank=%d" % mr, lib.cap_dpstrf_vbatched, plan, 1, mr, -1.0, Ad, Rd, piv, rank, resid, logdet, info,
                            r.stream), "cap_dpstrf_vbatched")
                want.append(classes)
            S.ok(r.call("dpstrf_vbatched rank alone", lib.cap_dpstrf_vbatched, plan, 1, 1 << 40, 0.25, Ad, Rd, piv, rank, None, None, None, r.stream),
                 "cap_dpstrf_vbatched")
            S.ok(r.call("dpstrf_vbatched no R", lib.cap_dpstrf_vbatched, plan, 1, 0, -1.0, Ad, None, piv, rank, resid, None, info, r.stream),
                 "cap_dpstrf_vbatched")
            want += [classes, classes]
            S.ok(r.call("empty plan", lib.cap_dpstrf_vbatched, empty, 1, 4, -1.0, None, None, None, None, None, None, None, r.stream), "empty plan")
            assert r.call("refused block of 65", lib.cap_dpstrf_vbatched, big, 1, 4, -1.0, Ad, Rd, piv, rank, resid, logdet, info, r.stream) == 4
            assert r.call("refused lower", lib.cap_dpstrf_vbatched, plan, 0, 4, -1.0, Ad, Rd, piv, rank, resid, logdet, info, r.stream) == 4
            finish(r, want, (Ad, Rd, piv, rank, resid, logdet, info))
            for q in (plan, empty, big):
                S.ok(lib.cap_vbatch_plan_destroy(q), "cap_vbatch_plan_destroy")
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    _trace_main(sys.argv[1])
