"""Shifted CholeskyQR3 (cap_cacqr_plan_create with num_iter 3 / 4) on one GPU, a fresh process:

    time     cap_cacqr_factor at m x n (default 2^21 x 256, generator matrix) for the num_iter values of --iters, alternating inside one loop:
             median / min / max ms over --reps (>= 10) calls after one warm-up round, device events on the stream; with num_iter 2 in the list
             the ratios t(k) / t(2) and the cost of a shifted sweep against an unshifted one ((t(3) - t(2)) / (t(2) / 2)).
             --lib PATH times another build of the library (the parent commit's, num_iter 2 only: the yardstick of the same session)
    hash     sha256 of the bytes of R and Q for num_iter 1 and 2 at --m x --n (generator matrix): equal across two builds = bit-identical
    reach    per m of --reach-m at n = 256: A = U diag(logspace(0, -log10 kappa, n)) V^T for kappa = 1e8 ... 1e16 (U: the Q of CholeskyQR2 of a
             random matrix, orthonormal to 1e-15; V: Householder Q of a random n x n), factored with num_iter 2, 3 and 4; a decade counts as
             handled when info == 0, ||QR - A||_F / ||A||_F < 1e-13 and ||Q^T Q - I||_F / n < 1e-15 (torch fp64 products)
    trace    --trace K: nothing but 5 factor calls with num_iter K, for `rocprofv3 --kernel-trace --stats -- python tools/scqr_bench.py --trace 3`

One JSON line per measurement.

    timeout -k 10 600 python tools/scqr_bench.py [--m 2097152] [--n 256] [--iters 2,3,4] [--reps 11] [--hash] [--reach] [--lib PATH]
"""
import argparse
import ctypes as C
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def load(path):
    """the handful of entries this tool needs, bound by hand: --lib may name a build that lacks the newer ones"""
    L = C.CDLL(path, mode=C.RTLD_LOCAL)
    ptr, i64, cint = C.c_void_p, C.c_int64, C.c_int
    for name, res, args in (("cap_cacqr_plan_create", cint, [C.POINTER(ptr), i64, i64, cint, ptr]), ("cap_cacqr_plan_destroy", cint, [ptr]),
                            ("cap_cacqr_factor", cint, [ptr, ptr, i64, ptr]), ("cap_cacqr_info", cint, [ptr, ptr, C.POINTER(i64)]),
                            ("cap_cacqr_Q_ptr", ptr, [ptr, C.POINTER(i64)]), ("cap_cacqr_R_ptr", ptr, [ptr, C.POINTER(i64)]),
                            ("cap_fill_random", cint, [ptr, i64, i64, i64, i64, i64, i64, i64, i64, ptr]),
                            ("cap_copy_window", cint, [ptr, cint, i64, i64, i64, ptr, cint, i64, i64, i64, i64, i64, cint, cint, ptr])):
        f = getattr(L, name); f.restype = res; f.argtypes = args
    return L


def ok(st, what):
    if st != 0:
        raise RuntimeError("%s failed: status %d" % (what, st))


class Plan:
    def __init__(self, L, m, n, it):
        self.L, self.m, self.n, self.it, self.h = L, m, n, it, C.c_void_p()
        ok(L.cap_cacqr_plan_create(C.byref(self.h), m, n, it, None), "cap_cacqr_plan_create(num_iter=%d)" % it)

    def factor(self, A, lda, sp):
        ok(self.L.cap_cacqr_factor(self.h, A.data_ptr(), lda, sp), "cap_cacqr_factor")

    def info(self, sp):
        v = C.c_int64(0)
        st = self.L.cap_cacqr_info(self.h, sp, C.byref(v))
        if st not in (0, 3):
            ok(st, "cap_cacqr_info")
        return v.value

    def QR(self, sp):
        """copies of Q (n x m, row j = column j) and R (n x n) as torch tensors"""
        ldq, ldr = C.c_int64(0), C.c_int64(0)
        q = self.L.cap_cacqr_Q_ptr(self.h, C.byref(ldq)); r = self.L.cap_cacqr_R_ptr(self.h, C.byref(ldr))
        Q = torch.empty(self.n, self.m, dtype=torch.float64, device="cuda"); R = torch.empty(self.n, self.n, dtype=torch.float64, device="cuda")
        ok(self.L.cap_copy_window(q, 0, ldq.value, 0, 0, Q.data_ptr(), 0, self.m, 0, 0, self.m, self.n, 0, 0, sp), "copy Q")
        ok(self.L.cap_copy_window(r, 0, ldr.value, 0, 0, R.data_ptr(), 0, self.n, 0, 0, self.n, self.n, 0, 0, sp), "copy R")
        return Q, R

    def close(self):
        self.L.cap_cacqr_plan_destroy(self.h)


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def generator_matrix(L, m, n, sp):
    lda = m + (m & 1)
    A = torch.empty(n, lda, dtype=torch.float64, device="cuda")
    ok(L.cap_fill_random(A.data_ptr(), lda, m, n, 0, 0, 1, 1, 0, sp), "cap_fill_random")
    return A, lda


def run_time(L, a, s, tag):
    sp = s.cuda_stream
    A, lda = generator_matrix(L, a.m, a.n, sp)
    iters = [int(x) for x in a.iters.split(",")]
    plans = {it: Plan(L, a.m, a.n, it) for it in iters}
    ts = {it: [] for it in iters}
    for rep in range(a.reps + 1):                          # the first round is the warm-up
        for it in iters:
            t = timed(s, lambda: plans[it].factor(A, lda, sp))
            if rep:
                ts[it].append(t)
    st = {it: stats(v) for it, v in ts.items()}
    for it in iters:
        assert plans[it].info(sp) == 0
        print(json.dumps({"lib": tag, "m": a.m, "n": a.n, "route": "factor(num_iter=%d)" % it, "reps": a.reps, **st[it]}), flush=True)
    if 2 in st:
        t2 = st[2]["median_ms"]
        out = {"lib": tag, "m": a.m, "n": a.n}
        for it in iters:
            if it > 2:
                out["t(%d)/t(2)" % it] = round(st[it]["median_ms"] / t2, 4)
                out["shifted_sweep_over_unshifted(num_iter=%d)" % it] = round((st[it]["median_ms"] - t2) / (it - 2) / (t2 / 2), 4)
        if len(out) > 3:
            out["expected"] = "t(3)/t(2) ~ 1.5, t(4)/t(2) ~ 2: a shifted sweep costs one sweep"
            print(json.dumps(out), flush=True)
    for p in plans.values():
        p.close()


def run_hash(L, a, s, tag):
    sp = s.cuda_stream
    A, lda = generator_matrix(L, a.m, a.n, sp)
    for it in (1, 2):
        p = Plan(L, a.m, a.n, it)
        p.factor(A, lda, sp)
        assert p.info(sp) == 0
        Q, R = p.QR(sp)
        torch.cuda.synchronize()
        print(json.dumps({"lib": tag, "m": a.m, "n": a.n, "num_iter": it, "sha256_R": hashlib.sha256(R.cpu().numpy().tobytes()).hexdigest(),
                          "sha256_Q": hashlib.sha256(Q.cpu().numpy().tobytes()).hexdigest()}), flush=True)
        p.close()


def run_reach(L, a, s):
    sp = s.cuda_stream
    n = 256
    g = torch.Generator(device="cuda"); g.manual_seed(10)
    v, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=torch.Generator().manual_seed(11)))
    v = v.cuda()
    for m in [int(x) for x in a.reach_m.split(",")]:
        X = torch.randn(n, m, dtype=torch.float64, device="cuda", generator=g)            # column-major m x n, ld = m
        p2 = Plan(L, m, n, 2)
        p2.factor(X, m, sp)
        assert p2.info(sp) == 0
        U, _ = p2.QR(sp)
        p2.close()
        del X
        plans = {it: Plan(L, m, n, it) for it in (2, 3, 4)}
        best = {2: None, 3: None, 4: None}
        for e in range(8, 17):
            sig = torch.logspace(0, -e, n, dtype=torch.float64, device="cuda")
            A = (v * sig) @ U                                                              # (U diag(sig) V^T)^T: n x m, rows = columns of A
            na = torch.linalg.norm(A).item()
            row = {"m": m, "n": n, "kappa": "1e%d" % e}
            for it in (2, 3, 4):
                plans[it].factor(A, m, sp)
                info = plans[it].info(sp)
                res = orth = float("nan")
                if info == 0:
                    Q, R = plans[it].QR(sp)
                    res = (torch.linalg.norm(R @ Q - A) / na).item()                       # both tensors hold the transposes: (Q R)^T = R^T Q^T
                    orth = (torch.linalg.norm(Q @ Q.t() - torch.eye(n, dtype=torch.float64, device="cuda")) / n).item()
                    del Q, R
                good = info == 0 and res < 1e-13 and orth < 1e-15
                row["num_iter=%d" % it] = {"info": info, "residual": res, "orthogonality": orth, "handled": good}
                if good and (best[it] is None or best[it] == e - 1):
                    best[it] = e
            print(json.dumps(row), flush=True)
            del A
        print(json.dumps({"m": m, "n": n, "largest_kappa_handled_without_a_gap_from_1e8": {("num_iter=%d" % it): (("1e%d" % best[it]) if best[it] else None)
                                                                                       for it in (2, 3, 4)}}), flush=True)
        for p in plans.values():
            p.close()
        del U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 21)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", default="2,3,4")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--lib", default=os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so"))
    ap.add_argument("--hash", action="store_true")
    ap.add_argument("--reach", action="store_true")
    ap.add_argument("--reach-m", default="8192,65536,2097152")
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    assert a.reps >= 10
    torch.cuda.set_device(0)
    L = load(a.lib)
    tag = os.path.relpath(os.path.abspath(a.lib), ROOT)
    s = torch.cuda.current_stream()
    if a.trace:
        A, lda = generator_matrix(L, a.m, a.n, s.cuda_stream)
        p = Plan(L, a.m, a.n, a.trace)
        for _ in range(5):
            p.factor(A, lda, s.cuda_stream)
        assert p.info(s.cuda_stream) == 0
        p.close()
    elif a.hash:
        run_hash(L, a, s, tag)
    elif a.reach:
        run_reach(L, a, s)
    else:
        run_time(L, a, s, tag)


if __name__ == "__main__":
    main()
