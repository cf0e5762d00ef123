#!/usr/bin/env python3
"""bench.py - fp64 Cholesky TFLOP/s on MI355X (BASELINE.json metric), one process per GPU.

    python bench.py --gpus 1 --steps 3 --warmup 1            # N = 65536 on one GPU
    python bench.py --full                                    # ... plus the checks, rooflines, CPU baseline and extra_configs below
    python bench.py --dump-outputs out                        # ... plus out/R.npy: a fixed sample of the last step's factor
    python bench.py --gpus 8 --steps 3 --warmup 1            # starts its own 8 ranks (one per GPU, RCCL) and relays rank 0's line
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
           --master-port 29501 bench.py --gpus 8 --steps 3 --warmup 1      # the same under an external launcher
    python bench.py --workload cacqr                          # CholeskyQR2 2^21 x 256 per GPU (BASELINE config 4 shape)
    python bench.py --workload mixed                          # bf16 MFMA factor + fp64 refinement, 1 GPU (BASELINE config 5's method)

A "step" = one warm `factor` call on a resident synthetic matrix (the reference's own generators,
structure.hpp:68-129, computed on the GPU), timed like bench/cholesky/cholinv.cpp:44-60:
barrier + sync, K calls, sync + barrier, max over ranks.
  cholesky: TFLOP/s := (N^3/3) / seconds-per-factor, N = 65536 for every GPU count ("strong" scaling).
  cacqr   : TFLOP/s := 4 m n^2 / seconds, m = 2^21 rows PER GPU ("weak" scaling), n = 256.

A plain run sets up, warms up, times the steps, writes the last step's outputs if --dump-outputs DIR is given, and prints the
JSON line (a non-zero `info` still fails it).  With --full the JSON line also carries
  config.residual - the reference validator's metric (test/cholesky/validate.hpp:33-46) of the LAST timed result,
                 computed after the timed region, plus an independent probe check (torch fp64 matmul);
                 a non-zero `info` or a residual above tolerance makes the run FAIL (value null, exit code 1),
  roofline     - the dominant kernel measured live with HIP events on its launch stream (separate profiled call),
  cpu_baseline - the REAL reference (oracle/_ref, MPICH + MKL, 8 ranks = its own 2x2x2 grid) or, if
                 that binary is unavailable, the NumPy port, timed on the host cores on a bounded sample,
  extra_configs - (1 GPU, cholesky) BASELINE configs[1] (N = 32768) and the reference-semantics mode
                 (complete_inv = 0: R and R^-1) timed the same way, fewer steps.
"""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TF = 78.6      # MI355X dense fp64 MFMA peak; measured 77.7 (tools/mfma_f64_probe2)
HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s measured streaming copy)
RES_TOL = 1e-14               # ||A - R^T R||_F / ||A||_F (BASELINE.md section 4 parity gate)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0, help="timed steps (default: 3 factorizations; 20 for the 10 ms CholeskyQR2 step)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="cholesky", choices=["cholesky", "cacqr", "mixed", "summa"])
    ap.add_argument("--n", "--size", dest="n", type=int, default=65536,
                    help="matrix dimension (BASELINE metric: 65536); use --size under torch.distributed.run, whose own parser trips over --n")
    ap.add_argument("--nb", type=int, default=0, help="panel width override (0 = library default)")
    ap.add_argument("--outer", type=int, default=0, help="outer strip height NB override (0 = library default)")
    ap.add_argument("--tail", type=int, default=-1, help="trailing size below which strips are nb wide (-1 = default)")
    ap.add_argument("--depth2", type=int, default=-1, help="look-ahead depth 2 (split bulk updates): 1/0, -1 = library default")
    ap.add_argument("--reserve", type=int, default=-1, help="CUs reserved for the panel chain (-1 = library default)")
    ap.add_argument("--occ1-m", type=int, default=-1, help="columns left below which bulk updates run one workgroup per CU (-1 = library default 16384, 0 = never)")
    ap.add_argument("--inner-la", type=int, default=-1, help="column-split look-ahead 1/0 (-1 = library default: off)")
    ap.add_argument("--serial-m", type=int, default=-1, help="remaining rows below which chain and bulk update are not overlapped (-1 = default)")
    ap.add_argument("--strip", type=int, default=0, help="multi-GPU: block rows per strip (0 = library default)")
    ap.add_argument("--dist-mode", default="auto", choices=["auto", "safe", "overlap", "ipc"],
                    help="multi-GPU: safe = one communicator + one communication stream; overlap = small messages on their own "
                         "communicator/stream; ipc = overlap with the strip exchange as IPC peer copies; auto = safe first (warm-up + "
                         "residual check + timing), then overlap, then ipc, each under a host watchdog - the best completed mode is "
                         "reported (fallback to it if a later mode makes no progress)")
    ap.add_argument("--exchange", default="rccl", choices=["rccl", "ipc"], help="multi-GPU strip exchange: RCCL all-gather or IPC peer copies")
    ap.add_argument("--grid-rows", default="auto",
                    help="multi-GPU: process rows Pr of the Pr x Pc block-cyclic layout (1 = block columns only); auto (default) = the 1 x P modes "
                         "first, then - where P = 2 x Pc with 2 | Pc (4, 8 GPUs) - the 2 x (P/2) layout, all under the same watchdog in ONE "
                         "invocation: every layout / mode is listed in config.modes, the best completed one is reported")
    ap.add_argument("--watchdog-s", type=float, default=0.0, help="multi-GPU: seconds without completion before a step counts as hung (0 = auto)")
    ap.add_argument("--complete-inv", type=int, default=-1,
                    help="-1 blocked Cholesky (headline), 0/1 reference cholinv semantics (R and R^-1)")
    ap.add_argument("--qr-rows", type=int, default=1 << 21, help="cacqr: rows per GPU")
    ap.add_argument("--qr-cols", type=int, default=256, help="cacqr: columns")
    ap.add_argument("--replay-rank", type=int, default=None,
                    help="PROJECTION, not a multi-GPU measurement: replay rank r (-1: every rank) of the --of P rank 1 x P schedule on THIS GPU "
                         "(tools/replay.py: the peers' data comes out of a finished factor behind a link model) and print the per-rank timeline")
    ap.add_argument("--of", type=int, default=8, help="--replay-rank: ranks of the replayed schedule")
    ap.add_argument("--link-gbps", type=float, default=100.0, help="--replay-rank: modelled bandwidth per xGMI link")
    ap.add_argument("--lat-us", type=float, default=10.0, help="--replay-rank: modelled latency per collective")
    ap.add_argument("--channels", type=int, default=0, help="--replay-rank: workgroups a collective's stand-in kernel occupies for its modelled time (the CU share of an "
                                                             "RCCL kernel; 0: none, like the IPC / copy-engine exchange)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the extra_configs runs")
    ap.add_argument("--no-check", action="store_true", help="skip the residual checks (profiling runs)")
    ap.add_argument("--cpu-n", type=int, default=16384, help="bounded CPU-baseline sample size")
    ap.add_argument("--cpu-budget-s", type=float, default=100.0, help="seconds of host time the CPU baseline may take")
    ap.add_argument("--check", action="store_true", help="(kept for compatibility: --full computes the residual)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: residual checks, rooflines, the CPU baseline and "
                         "extra_configs (without it a run sets up, warms up, times the steps and prints the result line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed as DIR/<name>.npy (float64; an output of more than "
                         "%d entries as a fixed, seeded sample of them); one GPU" % DUMP_SAMPLE)
    args = ap.parse_args()
    if args.steps <= 0:
        args.steps = 20 if args.workload == "cacqr" else (5 if args.workload == "summa" else 3)      # a CholeskyQR2 step is 10 ms: average over more of them
    if not args.full:
        args.no_cpu_baseline = args.no_extra = args.no_check = True
    if args.dump_outputs and (args.gpus != 1 or args.replay_rank is not None):
        ap.error("--dump-outputs runs on one GPU, without --replay-rank")
    return args


DUMP_SAMPLE = 1 << 21         # entries written of a larger output: 16 MB of float64, 4 outputs at most per workload


def sample_positions(rows, cols, upper):
    """The (row, col) positions --dump-outputs writes of a rows x cols output: all of them up to DUMP_SAMPLE entries, else
    DUMP_SAMPLE positions drawn with a fixed seed (in the upper triangle for a triangular factor)."""
    import numpy as np
    if rows * cols <= DUMP_SAMPLE:
        r, c = np.divmod(np.arange(rows * cols), cols)
        return (r[r <= c], c[r <= c]) if upper else (r, c)
    rng = np.random.default_rng(20261015)
    r, c = rng.integers(0, rows, DUMP_SAMPLE), rng.integers(0, cols, DUMP_SAMPLE)
    return (np.minimum(r, c), np.maximum(r, c)) if upper else (r, c)


def dump_outputs(args, outputs):
    """--dump-outputs: outputs = [(name, [row, col] device view, upper triangular?)] -> DIR/<name>.npy, float64, one value per
    position of sample_positions (the whole output, row-major, when it is small enough)."""
    if not args.dump_outputs:
        return
    import numpy as np
    import torch
    os.makedirs(args.dump_outputs, exist_ok=True)
    for name, view, upper in outputs:
        r, c = (torch.from_numpy(x).to(view.device) for x in sample_positions(view.shape[0], view.shape[1], upper))
        np.save(os.path.join(args.dump_outputs, name + ".npy"), view[r, c].to(torch.float64).cpu().numpy())


def _largest_cube(limit):
    c = 1
    while (c + 1) ** 3 <= limit:
        c += 1
    return c ** 3


def cpu_baseline(cpu_n, budget_s=100.0):
    """Reference CPU/MPI path on the host cores (protocol bench/cholesky/cholinv.cpp:44-60), bounded to about `budget_s` seconds.

    The REAL reference (oracle/_ref); MKL with 1 thread per rank and, hybrid, 8 / 16 threads per rank.  What the budget is spent on (round-3 measurements on the GPU box's
    256-core EPYC: upstream's own 2 x 2 x 2 grid wins; 64 ranks and one rank x 128 MKL threads are 2-4x SLOWER):
      c1     BASELINE configs[0], the plumbing case: 1 rank, N = 2048, bcMult = 0, the bench's default policy; its residual is
             the number SURVEY App. A pins (1.70e-16);
      8 ranks, bcMult = -3 (the winner of every sweep so far) at N = cpu_n / 2 with 1, 8 and 16 MKL threads per rank (8 / 64 / 128
             host cores), the best of the three at N = cpu_n (8 x 1: about 7 s per factor at 16384; a run = generation + warm-up +
             timed factor + the validator's own SUMMA product, i.e. several factor times), the one-thread grid at N = cpu_n as well
             when time is left, then bcMult = -2 at N = cpu_n / 2 for the record; the first MPI start of a fresh box (15 - 25 s of paging) is
             absorbed by c1;
      one documented run each of the 64-rank (4 x 4 x 4) grid and of 1 rank x all cores inside MKL (GNU threading layer), at
             N = cpu_n / 4 so that they stay cheap - scaling evidence, never the reported value unless they win.
    `value` is the figure of the LARGEST N that completed (TFLOP/s on N^3/3, best knobs at that N); every run is in `runs`."""
    exe = os.path.join(ROOT, "oracle", "_ref", "cholinv_ref")
    mpiexec = "/opt/conda/bin/mpiexec"
    ncores = os.cpu_count() or 1
    host = "%d host cores" % ncores
    try:
        model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")]
        if model:
            host += " (%s)" % model[0]
    except Exception:
        pass
    t_start = time.time()
    runs = []

    def run_ref(ranks, nn, bc, threads, timeout, policy=1, keep=True):
        env = dict(os.environ, MKL_NUM_THREADS=str(threads), OMP_NUM_THREADS=str(threads))
        if threads > 1:
            env["MKL_THREADING_LAYER"] = "GNU"        # the default Intel-OpenMP layer gives wrong answers here
        t0 = time.time()
        try:
            out = subprocess.run([mpiexec, "-n", str(ranks), exe, str(nn), "0", "1", str(bc), "0", "0", str(policy), "-", "1"],
                                 env=env, capture_output=True, text=True, timeout=max(5.0, timeout)).stdout
        except Exception:
            return None
        m = re.search(r"time=([\d.eE+-]+) residual=([\d.eE+-]+)", out)
        if not m:
            return None
        t, res = float(m.group(1)), float(m.group(2))
        r = {"ranks": ranks, "threads_per_rank": threads, "cores": ranks * threads, "n": nn, "bcMult": bc, "seconds": t,
             "tflops": nn ** 3 / 3.0 / t / 1e12, "residual": res, "wall_s": time.time() - t0}
        if res < 1e-14:
            if keep:
                runs.append(r)
            return r
        return None

    if os.path.exists(exe) and os.path.exists(mpiexec):
        left = lambda: budget_s - (time.time() - t_start)
        half_n = max(1024, cpu_n // 2)
        # configs[0]: the reference's own CPU-runnable case (1 rank, N = 2048, bcMult = 0, Serialize + NoReplication = the bench default)
        # (the first MPI start on a fresh box pages the binaries in: 15 - 25 s; it is absorbed here, by the smallest run)
        c1r = run_ref(1, 2048, 0, 1, 45.0, policy=0, keep=False)
        def c1_of(r):
            return ({"n": 2048, "ranks": 1, "bcMult": 0, "seconds": r["seconds"], "tflops": r["tflops"], "residual": r["residual"],
                     "what": "BASELINE configs[0]: N=2048 fp64 cholinv, 1 MPI rank, reference CPU BLAS path (MKL, 1 thread)"} if r else None)
        c1 = c1_of(c1r)
        if ncores >= 8:
            # order of importance: upstream's own 8-rank grid (2 x 2 x 2, the only valid multi-rank grid among 2 / 4 / 8) with bcMult = -3
            # (the winner of every sweep so far) at N / 2 - one MKL thread per rank, then HYBRID: 8 ranks x {8, 16} MKL threads (GNU
            # threading layer; bench/set_critter_env.sh:3-18 is the upstream script that sets the per-rank thread count) - then the best
            # of those at N, then the one-thread grid at N for continuity with earlier rounds, then the second bcMult for the record
            first = run_ref(8, half_n, -3, 1, min(left(), 0.3 * budget_s)) if left() > 10 else None
            if first is None and left() > 10:
                first = run_ref(8, half_n, -2, 1, min(left(), 0.25 * budget_s))
            cands = [first] if first else []
            if first is not None:
                for th in (8, 16):
                    if ncores >= 8 * th and left() > 25:
                        r = run_ref(8, half_n, first["bcMult"], th, min(left() - 20, 0.2 * budget_s))
                        if r:
                            cands.append(r)
            if cands and left() > 20:
                b0 = max(cands, key=lambda r: r["tflops"])
                big = run_ref(8, cpu_n, b0["bcMult"], b0["threads_per_rank"], left() - 4)   # 8 x 1: about 7 s per factor at N = 16384, several per run
                if big is not None and b0["threads_per_rank"] > 1 and left() > 45:
                    run_ref(8, cpu_n, first["bcMult"], 1, left() - 4)
            if first is not None and first["bcMult"] == -3 and left() > 15:
                run_ref(8, half_n, -2, 1, min(left() - 2, 0.2 * budget_s))
        quarter_n = max(1024, cpu_n // 4)
        if ncores >= 64 and left() > 12:
            run_ref(64, quarter_n, -2, 1, min(left() - 2, 20.0))
        if ncores >= 16 and left() > 8:
            run_ref(1, quarter_n, -2, min(ncores, 128), min(left() - 1, 20.0))
        if not runs and left() > 5:      # fewer than 8 cores: whatever the host has
            run_ref(1, min(cpu_n, 4096), -2, 1, left())
        if c1 is None and left() > 6:    # (a cold start that outlasted its limit: the plumbing run once more, warm)
            c1 = c1_of(run_ref(1, 2048, 0, 1, min(left(), 20.0), policy=0, keep=False))
        if runs:
            nmax = max(r["n"] for r in runs)
            b = max((r for r in runs if r["n"] == nmax), key=lambda r: r["tflops"])
            out = {"value": b["tflops"], "unit": "TFLOP/s", "cores": b["cores"], "kind": "reference", "host": host,
                   "sample": "N=%d (bounded sample of the N=65536 workload; the largest N of %d runs in %.0f s, all listed in `runs`): upstream "
                             "cholinv on %d MPI rank(s) x %d MKL thread(s), Serialize+ReplicateCommComp, bcMult=%d, complete_inv=0, %.3f s/factor, "
                             "residual %.2e" % (b["n"], len(runs), time.time() - t_start, b["ranks"], b["threads_per_rank"], b["bcMult"],
                                                b["seconds"], b["residual"]),
                   "runs": runs}
            if c1:
                out["c1"] = c1
            return out
    # fallback: the NumPy/LAPACK port of the same factorization on all host cores
    import numpy as np
    from oracle import capital_oracle as orc
    n = min(cpu_n, 8192)
    a = orc.symmetric_global(n, True)
    t0 = time.time(); r = np.linalg.cholesky(a); t = time.time() - t0
    return {"value": n ** 3 / 3.0 / t / 1e12, "unit": "TFLOP/s", "cores": os.cpu_count(), "kind": "port", "host": host,
            "sample": "N=%d numpy.linalg.cholesky (OpenBLAS, all host threads), %.3f s" % (n, t)}


def reference_on_operators(n=8192, iters=3, limit_s=90.0, libdirs=None, extra_env=None):
    """Part of the cpu_baseline leg (the only part of this file that may execute anything under oracle/): the comparator - the REAL reference,
    unmodified - once more with libcapital_amd_cblas.so (include/capital_amd_cblas.h) in MKL's place: its own cholinv::factor
    on one rank (MPI singleton), every BLAS / LAPACK call staged through HBM onto this library's operators - a PCIe-INCLUSIVE figure, reported
    inside `cpu_baseline` for the record and never part of `value`.  oracle/_ref/cholinv_cap is the checker's build of the reference
    (oracle/ref/build_ref.py); it is timed here the way cpu_baseline times the MKL build.  Never raises, never hangs (own process group,
    killed at `limit_s`)."""
    import signal
    label = ("the reference itself (unmodified sources, bench/cholesky/cholinv.cpp:39-60's protocol) with libcapital_amd_cblas.so in MKL's place: "
             "1 rank, N=%d, complete_inv=0, bcMult=-2; every BLAS / LAPACK call crosses PCIe twice" % n)
    exe = os.path.join(ROOT, "oracle", "_ref", "cholinv_cap")
    if not os.path.exists(exe):
        return {"workload": label, "value": None, "error": "oracle/_ref/cholinv_cap not built here (needs /root/reference at build time)"}
    env = dict(os.environ, CAPCB_REPORT="1", OMP_NUM_THREADS="1")
    env.pop("LD_PRELOAD", None)
    env["LD_LIBRARY_PATH"] = ":".join(["/usr/lib/x86_64-linux-gnu"] + (libdirs or [os.path.join(ROOT, "capital_amd", "lib"), "/opt/rocm/lib"]))
    env.update(extra_env or {})
    t0 = time.time()
    p = subprocess.Popen([exe, str(n), "0", "1", "-2", "0", "0", "0", "-", str(iters)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, start_new_session=True)
    try:
        so, se = p.communicate(timeout=limit_s)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except OSError:
            pass
        p.communicate()
        return {"workload": label, "value": None, "error": "no result within %.0f s" % limit_s}
    mt, mr = re.search(r"time=([\d.eE+-]+)", so), re.search(r"residual=([\d.eE+-]+)", so)
    ms = re.search(r"(\d+) calls served, (\d+) bytes host -> device, (\d+) bytes device -> host", se)
    if p.returncode != 0 or not mt or not mr:
        return {"workload": label, "value": None, "error": ("exit code %d: " % p.returncode) + (se or so)[-300:]}
    sec = float(mt.group(1))
    e = {"workload": label, "n": n, "value": n ** 3 / 3.0 / sec / 1e12, "unit": "TFLOP/s (N^3/3), PCIe-inclusive", "ms_per_step": sec * 1e3, "steps": iters,
         "residual": float(mr.group(1)), "residual_kind": "the reference's own validator (test/cholesky/validate.hpp:33-46)", "wall_s": time.time() - t0}
    if ms:   # whole process: generation, warm-up, `iters` timed factors and the validator's products
        e["blas_lapack_calls_served"] = int(ms.group(1)); e["bytes_host_to_device"] = int(ms.group(2)); e["bytes_device_to_host"] = int(ms.group(3))
        mi = re.search(r"([\d.]+) ms inside the entry points", se)
        if mi:   # (whole process too) - what is NOT inside them is the reference's own host code: serialize / swap / zero-fill loops on one core
            e["ms_inside_blas_lapack_entry_points_whole_process"] = float(mi.group(1))
    return e


def cpu_baseline_cacqr(m, n):
    """CholeskyQR2 on the host cores: the REAL reference's cacqr (1D grid, 8 ranks) on a bounded sample of the rows."""
    exe = os.path.join(ROOT, "oracle", "_ref", "cacqr_ref")
    mpiexec = "/opt/conda/bin/mpiexec"
    ms = min(m, 1 << 18)
    if os.path.exists(exe) and os.path.exists(mpiexec):
        env = dict(os.environ, MKL_NUM_THREADS="1", OMP_NUM_THREADS="1")
        try:
            # oracle/ref/drv_cacqr.cpp argv: variant(2 = CholeskyQR2) M N c complete_inv split bcMult dump iters
            out = subprocess.run([mpiexec, "-n", "8", exe, "2", str(ms), str(n), "1", "1", "1", "0", "-", "3"], env=env,
                                 capture_output=True, text=True, timeout=300).stdout
            mt = re.search(r"time=([\d.eE+-]+)", out)
            if mt:
                t = float(mt.group(1))
                return {"value": 4.0 * ms * n * n / t / 1e12, "unit": "TFLOP/s", "cores": 8, "kind": "reference",
                        "sample": "%dx%d (bounded sample of the rows): upstream cacqr 1D grid, 8 MPI ranks, MKL 1 thread/rank, "
                                  "CholeskyQR2, %.3f s" % (ms, n, t)}
        except Exception:
            pass
    import numpy as np
    from oracle import capital_oracle as orc
    a = np.random.default_rng(0).random((ms, n))
    t0 = time.time(); orc.cacqr_1d([a], 2); t = time.time() - t0
    return {"value": 4.0 * ms * n * n / t / 1e12, "unit": "TFLOP/s", "cores": os.cpu_count(), "kind": "port",
            "sample": "%dx%d NumPy port of CholeskyQR2 (OpenBLAS, all host threads), %.3f s" % (ms, n, t)}


def traffic_from_profile(n, args):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of THIS command
    (profiles/rNN_traffic_bench_n65536.json, produced by tools/prof_round.sh + tools/make_traffic_json.py: FETCH_SIZE and WRITE_SIZE in
    separate runs, FETCH_SIZE doubled per the gfx950 correction).  Counters cannot be collected inside the timed run; the
    number is only reported for the exact configuration AND kernel build it was measured on (same source, or same machine code of
    gemm.hip's kernels), newest round first, else null."""
    import glob
    import hashlib
    try:
        src = b"".join(open(os.path.join(ROOT, "capital_amd", "csrc", f), "rb").read() for f in ("gemm.hip", "tile_dma.h"))
        sha = hashlib.sha256(src).hexdigest()[:16]
        # the identity that matters is the kernel's MACHINE CODE: host-only edits of gemm.hip (a scratch-buffer release, the access
        # notes of the schedule checker) change the source hash and not one instruction (capital_amd/build.py device_text_md5)
        from capital_amd import build as _b
        text = _b.device_text_md5("gemm.hip")
        for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic_bench_n65536.json")), reverse=True):
            d = json.load(open(path))
            if (d["config"]["n"] == n and d["config"]["complete_inv"] == args.complete_inv and not (args.nb or args.outer or args.tail >= 0)
                    and (d.get("kernel_src_sha16") == sha or (text is not None and d.get("kernel_text_md5") == text))):
                return d["traffic_bytes_per_launch"]
    except Exception:
        pass
    return None


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(args, argv=None):
    """Re-run this file as N ranks: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port <free> bench.py <the same arguments>` - one process per GPU (RCCL), or per rank on cuda:0 under
    CAPITAL_BENCH_EMULATE=1.  stdout / stderr are inherited, so rank 0's one JSON line is this process's JSON line; the exit
    code is the launcher's.  Never returns without a JSON line: a box with fewer GPUs than ranks gets one with value null."""
    argv = list(sys.argv[1:] if argv is None else argv)
    fixed = []
    for a in argv:                         # torch.distributed.run's own parser trips over "--n": hand the size over as --size
        if a == "--n":
            a = "--size"
        elif a.startswith("--n="):
            a = "--size=" + a[4:]
        fixed.append(a)
    emulate = os.environ.get("CAPITAL_BENCH_EMULATE") == "1"
    if not emulate:
        try:
            import torch
            have = torch.cuda.device_count()
        except Exception:
            have = 0
        if have < args.gpus:
            print(json.dumps({"metric": args.workload, "value": None, "unit": "TFLOP/s", "n_gpus": args.gpus, "steps": args.steps,
                              "warmup": args.warmup, "higher_is_better": True,
                              "error": "--gpus %d but this box shows %d GPU(s)" % (args.gpus, have)}), flush=True)
            return 1
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + fixed
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("OMP_NUM_THREADS", "1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL and the IPC strip exchange need it on this driver
    print("[bench] starting %d ranks: %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    import torch
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (the reference's protocol is one binary under
        # `mpirun -n P`, bench/cholesky/cholinv.cpp:44-60) and relay rank 0's JSON line and the exit code
        sys.exit(self_launch(args))
    if args.gpus != world:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: launch as many ranks as GPUs" % (args.gpus, world))
    # CAPITAL_BENCH_EMULATE=1 (tests only): all ranks share cuda:0 and talk through gloo + the host-staged communicator,
    # which exercises this file's N > 1 path on a 1-GPU box; the product path is RCCL, one GPU per rank.
    emulate = os.environ.get("CAPITAL_BENCH_EMULATE") == "1"
    torch.cuda.set_device(0 if emulate else local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if emulate:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    from capital_amd import _lib
    L = _lib.lib()     # fails loudly if the HIP library is missing
    import ctypes as C

    if args.replay_rank is not None:
        # one rank's real schedule at full speed on the one GPU there is; everything it prints is labelled a projection
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import replay
        ranks = None if args.replay_rank < 0 else [args.replay_rank]
        if str(args.grid_rows) not in ("auto", "1"):
            Pr = int(args.grid_rows)
            res = replay.run2d(args.n, Pr, args.of // Pr, ranks, 512, args.steps or 3, args.warmup, args.link_gbps, args.lat_us, 500, 300, args.occ1_m if args.occ1_m >= 0 else None)
            print(json.dumps({
                "metric": "PROJECTED fp64 Cholesky TFLOP/s on %d MI355X, %s block-cyclic plan (max over the replayed ranks of N^3/3 per second of one rank's schedule on ONE GPU; "
                          "peers' data from a finished factor behind a link model) - not a multi-GPU measurement" % (args.of, res["grid"]),
                "value": res["projected_tf_whole_job"], "unit": "TFLOP/s", "n_gpus": 1, "projection_of_gpus": args.of, "steps": args.steps or 3, "warmup": args.warmup,
                "ms_per_step": res["projected_ms_max_over_ranks"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                "config": {"workload": "N=%d fp64 Cholesky, rank(s) %s of the %s block-cyclic plan replayed on one GPU (tools/replay.py run2d)" % (args.n, "all" if ranks is None else ranks, res["grid"]),
                           "link_GBps_per_link": args.link_gbps, "lat_us": args.lat_us, "projected_frac_of_node_fp64_mfma_peak": res["projected_frac_of_P_gpu_peak"],
                           "projected_speedup_vs_1gpu": res["projected_speedup_vs_1gpu"], "single_gpu_tf_same_box": res["single_gpu_tf"]},
                "ranks": res["ranks"]}))
            return
        res = replay.run(args.n, args.of, ranks, 512, args.steps or 3, args.warmup, args.link_gbps, args.lat_us, "auto",
                         args.occ1_m if args.occ1_m >= 0 else None, args.strip or None, channels=args.channels)
        print(json.dumps({
            "metric": "PROJECTED fp64 Cholesky TFLOP/s on %d MI355X (max over the replayed ranks of N^3/3 per second of one rank's schedule on ONE GPU; "
                      "peers' data from a finished factor behind a link model) - not a multi-GPU measurement" % args.of,
            "value": res["projected_tf_whole_job"], "unit": "TFLOP/s", "n_gpus": 1, "projection_of_gpus": args.of, "steps": args.steps or 3, "warmup": args.warmup,
            "ms_per_step": res["projected_ms_max_over_ranks"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "N=%d fp64 Cholesky, rank(s) %s of the 1 x %d block-column-cyclic plan replayed on one GPU (tools/replay.py)" % (
                args.n, "all" if ranks is None else ranks, args.of), "link_GBps_per_link": args.link_gbps, "lat_us": args.lat_us, "collective_kernel_workgroups": args.channels,
                "projected_frac_of_node_fp64_mfma_peak": res["projected_frac_of_P_gpu_peak"], "projected_speedup_vs_1gpu": res["projected_speedup_vs_1gpu"],
                "single_gpu_tf_same_box": res["single_gpu_tf"]},
            "ranks": res["ranks"]}))
        return

    # N > 1: the control plane (barriers, max over ranks) runs over a gloo group on the HOST and GPU completion is POLLED, so a
    # collective that never completes (first contact with multi-rank RCCL) cannot block the bench: after `watchdog_s` without
    # completion every rank reports, rank 0 prints a JSON line with value null + the error, and the processes leave without
    # touching the GPU again.  Used by every multi-GPU workload that has no mode ladder of its own (CholeskyQR2, mixed precision).
    ctl = dist.new_group(backend="gloo") if (dist is not None and not emulate) else None

    def ctl_max(x):
        if dist is None:
            return float(x)
        t = torch.tensor([float(x)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=ctl)
        return float(t.item())

    def wait_gpu(limit_s):
        if dist is None:
            torch.cuda.synchronize()
            return True
        ev = torch.cuda.Event(); ev.record()
        t0 = time.perf_counter()
        while not ev.query():
            if time.perf_counter() - t0 > limit_s:
                return False
            time.sleep(2e-4)
        return True

    def hang_exit(what):
        print("[bench rank %d] %s made no progress within the watchdog limit" % (rank, what), file=sys.stderr, flush=True)
        if rank == 0:
            print(json.dumps({"metric": args.workload, "value": None, "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                              "higher_is_better": True, "error": "%s made no progress within %.0f s (host watchdog): a collective did not "
                              "complete" % (what, watchdog_limit), "fallback": True}), flush=True)
        sys.stdout.flush(); sys.stderr.flush()
        time.sleep(1.0)
        os._exit(1)

    watchdog_limit = args.watchdog_s or 120.0

    def barrier(what="step"):
        if ctl_max(0.0 if wait_gpu(watchdog_limit) else 1.0):
            hang_exit(what)
        if dist is not None:
            dist.barrier(group=ctl)

    def timed(run, steps, warmup):
        for _ in range(warmup):
            run()
        barrier("warm-up")
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        barrier("timed region")
        dt = time.perf_counter() - t0
        return ctl_max(dt) / steps

    def allreduce_sum(t):
        if dist is None:
            return t
        if emulate:
            h = t.cpu(); dist.all_reduce(h); return h.to(t.device)
        dist.all_reduce(t)
        return t

    if args.workload == "cacqr":
        out, ok = bench_cacqr(args, torch, L, C, rank, world, dist, emulate, timed, allreduce_sum)
    elif args.workload == "mixed":
        out, ok = bench_mixed(args, torch, L, C, rank, world, timed)
    elif args.workload == "summa":
        if world != 1:
            raise SystemExit("bench.py --workload summa runs on one GPU (the multi-rank driver is tools/summa_bench.py / examples/summa_driver.c)")
        out, ok = bench_summa(args, torch, L, C, rank, world, timed)
    else:
        out, ok = bench_cholesky(args, torch, L, C, rank, world, dist, emulate, timed, allreduce_sum)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if not ok:
        sys.exit(1)


def _librccl_path():
    try:
        libs = sorted({l.split()[-1] for l in open("/proc/self/maps") if "librccl" in l})
        return libs[0] if libs else None
    except Exception:
        return None


def bench_cholesky(args, torch, L, C, rank, world, dist, emulate, timed, allreduce_sum):
    from capital_amd import _lib, cholinv, validate
    from capital_amd.matrix import matrix
    n = args.n

    def single_gpu_case(nn, complete_inv, steps, warmup, opts=True):
        A = matrix(nn, nn, 1, 1)
        A.distribute_symmetric(0, 0, 1, 1, 0, True)
        pack = cholinv.info(complete_inv, 1, -5, 'U')      # bcMult -5: base-case hint N/32 >= 512 -> the library's 512-wide panels
        if opts:
            for key, v in (("nb", args.nb), ("outer", args.outer)):
                if v:
                    pack.set_option(key, v)
            for key, v in (("tail", args.tail), ("reserve", args.reserve), ("depth2", args.depth2), ("serial_m", args.serial_m),
                           ("occ1_m", args.occ1_m), ("inner_la", args.inner_la)):
                if v >= 0:
                    pack.set_option(key, v)
        sec = timed(lambda: cholinv.factor(A, pack, None), steps, warmup)
        return A, pack, sec

    diag = {}
    if world == 1:
        A, pack, sec = single_gpu_case(n, args.complete_inv, args.steps, args.warmup)
        info = pack.last_info()
        parallelism = "1 GPU"
        if args.dump_outputs:
            outs = [("R", cholinv.construct_R(pack))] + ([("Rinv", cholinv.construct_Rinv(pack))] if args.complete_inv >= 0 else [])
            dump_outputs(args, [(name, M.view(), True) for name, M in outs])
            del outs
            torch.cuda.empty_cache()
    else:
        ctx, sec, info, diag = multi_gpu_case(args, torch, L, C, rank, world, dist, emulate, allreduce_sum)
        parallelism = diag.pop("parallelism")

    tflops = (n ** 3 / 3.0 / sec / 1e12) if sec else None
    out = {"metric": "fp64 Cholesky TFLOP/s (N^3/3 per wall-second of one warm factor call), N=%d" % n,
           "value": tflops, "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": sec * 1e3 if sec else None, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f64", "data": "synthetic",
           "config": {"workload": "N=%d fp64 Cholesky A=R^T R, upstream distribute_symmetric(diag-dominant) input generated on "
                                  "the GPU, resident in HBM; complete_inv=%d" % (n, args.complete_inv),
                      "parallelism": parallelism, "info": int(info),
                      "pct_of_fp64_mfma_peak_per_gpu": (100.0 * tflops / (FP64_MFMA_PEAK_TF * world)) if tflops else None}}
    out["config"].update(diag)
    ok = int(info) == 0 and sec is not None

    # ---- parity of the result the timed loop left behind (outside the timed region)
    if not args.no_check and sec is not None:
        if world == 1:
            res = validate.cholesky.residual(A, pack)
            R = cholinv.construct_R(pack)
            probe = validate.cholesky.probe(A.view(), R.view())
            del R
        else:
            res = None
            probe = ctx.probe(allreduce_sum)
        out["config"]["residual"] = res if res is not None else probe
        out["config"]["residual_kind"] = ("||R^T R - A||_F/||A||_F over the upper triangle (test/cholesky/validate.hpp:33-46)"
                                          if res is not None else "probe")
        out["config"]["probe_residual"] = probe    # ||(R^T R - A) X||_F / ||A X||_F, X = 8 random vectors, torch fp64 matmul
        ok = ok and (res is None or (res == res and res <= RES_TOL)) and probe == probe and probe <= 1e-13
        torch.cuda.empty_cache()

    if args.full and rank == 0 and world == 1 and args.complete_inv < 0:
        # roofline of the dominant kernel, measured live (HIP events on its launch stream) on one more factor call
        pack.set_option("profile", 1)
        cholinv.factor(A, pack, None); torch.cuda.synchronize()
        nl, ms, fl = C.c_int64(0), C.c_double(0), C.c_double(0)
        _lib.check(L.cap_cholinv_profile(pack._plan, C.byref(nl), C.byref(ms), C.byref(fl)))
        pack.set_option("profile", 0)
        if nl.value:
            ach = fl.value / (ms.value * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": "dgemm_tn_dma_kernel<1> (trailing-update DSYRK, upper tiles)",
                               "achieved": ach, "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": ach / FP64_MFMA_PEAK_TF,
                               "launches": nl.value, "avg_launch_ms": ms.value / nl.value,
                               "algorithmic_flops_per_launch_avg": fl.value / nl.value, "traffic": traffic_from_profile(n, args)}
    if args.full and world > 1 and sec is not None:
        r = ctx.roofline(L, C)
        if rank == 0 and r:
            out["roofline"] = r

    # ---- the other configurations the judge asked to see in a driver-run record (1 GPU, default run only)
    if rank == 0 and world == 1 and not args.no_extra and args.complete_inv < 0 and n == 65536:
        del A, pack
        torch.cuda.empty_cache()
        extra = []
        for (nn, ci, steps2, label) in (
                (32768, -1, 3, "BASELINE configs[1]: N=32768 blocked Cholesky"),
                (32768, 0, 3, "reference semantics (cholinv.hpp:85-165): R and R^-1, complete_inv=0, N=32768"),
                (32768, 1, 3, "reference semantics: R and the full R^-1, complete_inv=1, N=32768"),
                (65536, 0, 2, "reference semantics at the headline size (what bench/cholesky/cholinv.cpp:39-53 runs): R and R^-1, "
                              "complete_inv=0, N=65536")):
            A2, p2, s2 = single_gpu_case(nn, ci, steps2, 1, opts=False)
            i2 = p2.last_info()
            r2 = validate.cholesky.residual(A2, p2) if not args.no_check else None
            tf = nn ** 3 / 3.0 / s2 / 1e12
            e = {"workload": label, "n": nn, "complete_inv": ci, "value": tf, "unit": "TFLOP/s (N^3/3)", "ms_per_step": s2 * 1e3,
                 "steps": steps2, "pct_of_fp64_mfma_peak": 100.0 * tf / FP64_MFMA_PEAK_TF, "info": int(i2), "residual": r2}
            if ci >= 0:   # true flops: N^3/3 (factor) + 2 (N/2)^3/3 (the two diagonal blocks of R^-1, split = 1) or + N^3/3 (all of R^-1)
                true_tf = (nn ** 3 / 3.0 + (nn ** 3 / 12.0 if ci == 0 else nn ** 3 / 3.0)) / s2 / 1e12
                e["true_flops_tflops"] = true_tf; e["true_flops_frac_of_peak"] = true_tf / FP64_MFMA_PEAK_TF
                if not args.no_check:
                    # the OTHER half of the reference's output: R^-1 checked where it is timed (torch fp64 matmul, per filled block) +
                    # the structure of the root block (exactly empty for complete_inv = 0, cholinv.hpp:147; filled for 1)
                    torch.cuda.empty_cache()
                    R2 = cholinv.construct_R(p2); Ri2 = cholinv.construct_Rinv(p2)
                    pr, nz = validate.cholesky.rinv_probe(R2.view(), Ri2.view(), ci, 1)
                    del R2, Ri2
                    e["rinv_probe"] = pr; e["rinv_root_block_nonzeros"] = nz
                    e["rinv_probe_kind"] = ("max over the filled diagonal blocks of ||R (R^-1 X) - X||_F/||X||_F, 8 vectors, torch fp64 matmul; "
                                            "root block Rinv[0:n/2, n/2:n] must be exactly zero for complete_inv=0, non-zero for 1")
                    ok = ok and validate.cholesky.rinv_ok(pr, nz, ci, nn, 1)
            extra.append(e)
            ok = ok and int(i2) == 0 and (r2 is None or r2 <= RES_TOL)
            del A2, p2
            torch.cuda.empty_cache()
        # BASELINE configs[3] (per-GPU shape) and configs[4]'s method on one GPU, each with its own roofline and residual
        class _Sub:
            pass
        # Each of them runs in a process of its own (this script with --workload): a workload that allocates its ~ 100 GB after another one of
        # the same process has freed as much runs 2 - 10 % slower whichever comes second (measured both ways, profiles/r06_experiments.md
        # section 11: the mixed factorization 156 ms here against 134 ms alone) - the figure wanted is the workload's own.  In-process fallback
        # if the child cannot be run (or CAPITAL_BENCH_INPROC=1).
        def run_child(wl, steps):
            cmd = [sys.executable, os.path.abspath(__file__), "--workload", wl, "--steps", str(steps), "--warmup", "1", "--full", "--no-extra"]
            if wl != "cacqr" or args.no_cpu_baseline:
                cmd.append("--no-cpu-baseline")
            if args.no_check:
                cmd.append("--no-check")
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if not lines:
                raise RuntimeError("no result line from %s (rc %d): %s" % (" ".join(cmd[1:]), r.returncode, r.stderr[-300:]))
            o = json.loads(lines[-1])
            o["process"] = "own process (python bench.py --workload %s)" % wl
            return o, r.returncode == 0
        for wl in ("cacqr", "mixed", "summa"):
            sub = _Sub(); sub.__dict__.update(vars(args))
            sub.no_cpu_baseline = True; sub.warmup = 1
            if not os.environ.get("CAPITAL_BENCH_INPROC"):
                try:
                    torch.cuda.empty_cache()
                    o2, k2 = run_child(wl, {"cacqr": 20, "summa": 5}.get(wl, 2))
                    extra.append({"workload": o2.get("metric"), "value": o2.get("value"), "unit": o2.get("unit"), "ms_per_step": o2.get("ms_per_step"),
                                  "steps": o2.get("steps"), "dtype": o2.get("dtype"), "config": o2.get("config"), "roofline": o2.get("roofline"),
                                  "cpu_baseline": o2.get("cpu_baseline"), "error": o2.get("error"), "process": o2.get("process")})
                    ok = ok and k2
                    continue
                except Exception as ex:      # fall through to the in-process run
                    sys.stderr.write("bench.py: extra %s in its own process failed (%r); running it in-process\n" % (wl, ex))
            try:
                if wl == "cacqr":
                    sub.steps = 20
                    sub.no_cpu_baseline = args.no_cpu_baseline      # config 4's CPU comparator (the real reference's cacqr on 8 ranks, bounded sample) rides along
                    o2, k2 = bench_cacqr(sub, torch, L, C, rank, world, dist, emulate, timed, allreduce_sum)
                elif wl == "summa":
                    sub.steps = 5
                    o2, k2 = bench_summa(sub, torch, L, C, rank, world, timed)
                else:
                    sub.steps = 2
                    o2, k2 = bench_mixed(sub, torch, L, C, rank, world, timed)
            except Exception as ex:      # an extra must not take the headline down with it; it is reported as failed
                o2, k2 = {"metric": wl, "value": None, "error": repr(ex)}, False
            extra.append({"workload": o2.get("metric"), "value": o2.get("value"), "unit": o2.get("unit"), "ms_per_step": o2.get("ms_per_step"),
                          "steps": o2.get("steps"), "dtype": o2.get("dtype"), "config": o2.get("config"), "roofline": o2.get("roofline"),
                          "cpu_baseline": o2.get("cpu_baseline"), "error": o2.get("error")})
            ok = ok and k2
            torch.cuda.empty_cache()
        out["extra_configs"] = extra
    if rank == 0 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.cpu_n, args.cpu_budget_s)
        if world == 1 and args.complete_inv < 0 and n == 65536:
            # the same comparator (the checker's build of the reference, oracle/_ref) once more with its BLAS / LAPACK calls served by this
            # library through PCIe: part of the baseline leg, informational, cannot change `value` or its gate
            try:
                out["cpu_baseline"]["reference_with_offloaded_blas"] = reference_on_operators()
            except Exception as ex:
                out["cpu_baseline"]["reference_with_offloaded_blas"] = {"value": None, "error": repr(ex)}
    if not ok:
        out["value"] = None
        out["error"] = "factorization failed its parity gate (info != 0 or residual above %g)" % RES_TOL if sec is not None else \
                       "no mode of the multi-GPU schedule completed (see config.watchdog)"
    return out, ok


def multi_gpu_case(args, torch, L, C, rank, world, dist, emulate, allreduce_sum):
    """N > 1: the distributed schedule (csrc/dist.hip) with self-diagnosis.  Returns (ctx, seconds per factor or None, info, diag).

    First contact with real multi-rank RCCL must yield a number, not a hang:
      1. safe mode (one communicator, one communication stream, collectives in program order): warm-up, residual check, timing;
      2. overlapped mode under a HOST watchdog: completion is polled (event query), never waited for; if a step makes no
         progress within the limit, every rank prints how far its event chain got (cap_dist_progress) and the safe-mode
         figure is reported with "fallback": true.  The control plane (barriers, max over ranks) runs over gloo on the host
         so a stuck GPU queue cannot block it."""
    import ctypes
    from capital_amd import _lib, dist_cholesky
    n = args.n
    ctl = None if emulate else dist.new_group(backend="gloo")

    def ctl_barrier():
        dist.barrier(group=ctl)

    def ctl_max(x):
        t = torch.tensor([float(x)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=ctl)
        return float(t.item())

    auto_grid = str(args.grid_rows) == "auto"
    layouts = [1] if auto_grid else [int(args.grid_rows)]
    if auto_grid and world >= 4 and world % 2 == 0 and (world // 2) % 2 == 0:
        layouts.append(2)                # 2 x 2, 2 x 4: the north star's 2D block-cyclic layout, measured next to 1 x P in the same run

    def make_ctx(gr):
        row = col = None
        if emulate:
            from tests.host_staged import HostStagedComm, grid_groups
            c = HostStagedComm()
            if gr > 1:
                row, col = grid_groups(gr, HostStagedComm)
        else:
            c = dist_cholesky.RcclComm()
        cx = dist_cholesky.setup(n, nb=args.nb or 0, comm=c, grid_rows=gr, row=row, col=col)
        if gr == 1:
            if args.strip:
                cx.set_option("strip", args.strip)
            if args.depth2 >= 0:
                cx.set_option("depth2", args.depth2)
            if args.exchange == "ipc":
                cx.set_option("ipc", 1)
        return c, cx

    comm, ctx = make_ctx(layouts[0])
    nr, rk, dev = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(L.cap_comm_query(comm.handle, C.byref(nr), C.byref(rk), C.byref(dev)))
    diag = {"n_ranks_seen": nr.value, "rank_seen": rk.value, "device": dev.value, "librccl": _librccl_path(),
            "comm_backend": {0: "self", 1: "rccl", 2: "host-staged (emulation)"}[int(L.cap_comm_backend(comm.handle))],
            "exchange": args.exchange}
    seen = ctl_max(-nr.value)            # every rank must see the same communicator size
    if int(-seen) != world or nr.value != world:
        diag["error"] = "communicator reports %d ranks, launcher %d" % (nr.value, world)

    def wait_gpu(limit_s):
        """Completion of everything enqueued on the current stream (the factor joins its helper streams into it), polled."""
        ev = torch.cuda.Event(); ev.record()
        t0 = time.perf_counter()
        while not ev.query():
            if time.perf_counter() - t0 > limit_s:
                return False
            time.sleep(2e-4)
        return True

    def progress(cx, is2d):
        if is2d:
            return {}
        out9 = (ctypes.c_int64 * 9)()
        L.cap_dist_progress(cx.plan, out9)
        v = list(out9)
        return {"fact": v[0], "msg": v[1], "rowdone": v[2], "solved": v[3], "gather": v[4], "head2": v[5], "rest": v[6],
                "block_rows": v[7], "strips": v[8]}

    def timed_watch(cx, steps, warmup, limit_s):
        """barrier + sync | K factor calls | sync + barrier, max over ranks - with the syncs polled; None when a rank hangs."""
        for _ in range(warmup):
            cx.factor()
        hung = ctl_max(0.0 if wait_gpu(limit_s * max(warmup, 1)) else 1.0)
        if hung:
            return None
        ctl_barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            cx.factor()
        okw = wait_gpu(limit_s * steps)
        if ctl_max(0.0 if okw else 1.0):
            return None
        torch.cuda.synchronize()
        ctl_barrier()
        return ctl_max(time.perf_counter() - t0) / steps

    limit = args.watchdog_s or max(60.0, 20.0 * (n / 65536.0) ** 3 * 4.0)
    results, wd, ctxs = {}, {}, {}
    stop = False
    for gr in layouts:
        is2d = gr > 1
        if gr != layouts[0]:
            _, ctx = make_ctx(gr)
        if is2d:
            modes = ["2d"]
        else:
            modes = {"auto": ["safe", "overlap", "ipc"], "safe": ["safe"], "overlap": ["overlap"], "ipc": ["ipc"]}[args.dist_mode]
            if args.exchange == "ipc":
                modes = [m for m in modes if m != "ipc"] or ["ipc"]         # every mode already runs on the IPC exchange
        for mode in modes:
            key = mode if not is2d else "%dx%d" % (gr, world // gr)
            if not is2d:
                ctx.set_option("safe", 1 if mode == "safe" else 0)
                if mode == "ipc":                                          # overlapped schedule, strip exchange by IPC peer copies (SDMA)
                    ctx.set_option("ipc", 1)
            sec = timed_watch(ctx, args.steps, max(args.warmup, 1), limit)
            if sec is None:
                wd[key] = {"hung": True, "limit_s": limit, "progress_rank%d" % rank: progress(ctx, is2d)}
                print("[bench rank %d] %s made no progress within %.0f s: %s" % (rank, key, limit, json.dumps(wd[key])), file=sys.stderr, flush=True)
                stop = True
                break                        # the GPU queues are stuck: nothing further can run in this process
            info = ctx.last_info()
            probe = ctx.probe(allreduce_sum) if not args.no_check else 0.0
            results[key] = {"sec": sec, "info": int(info), "probe": probe, "tflops": n ** 3 / 3.0 / sec / 1e12,
                            "layout": "%dx%d block-cyclic (nb=%d)" % (gr, world // gr, ctx.nb)}
            ctxs[key] = (ctx, mode, is2d)
            if not is2d and (mode == "ipc" or args.exchange == "ipc"):
                results[key]["ipc_active"] = int(ctx.get_option("ipc_active"))    # 0: a peer could not be mapped, the run used RCCL
            if is2d:
                results[key]["launches_per_factor_rank0"] = ctx.launch_counts()
            if int(info) != 0 or not (probe <= 1e-13):
                stop = True
                break
        if stop:
            break
    diag["modes"] = {m: dict({"tflops": r["tflops"], "ms_per_step": r["sec"] * 1e3, "info": r["info"], "probe_residual": r["probe"], "layout": r["layout"]},
                             **{k: r[k] for k in ("ipc_active", "launches_per_factor_rank0") if k in r}) for m, r in results.items()}
    if wd:
        diag["watchdog"] = wd
    good = {m: r for m, r in results.items() if r["info"] == 0 and r["probe"] <= 1e-13}
    first_gr = layouts[0]
    diag["parallelism"] = "%dx%d block-cyclic (nb=%d), RCCL over xGMI" % (first_gr, world // first_gr, ctx.nb)
    diag["grid"] = "%dx%d" % (first_gr, world // first_gr)
    if not good:
        if wd:
            _emit_and_exit_on_hang(args, rank, n, world, diag, None)
        return ctx, None, (list(results.values())[0]["info"] if results else -1), diag
    best = min(good, key=lambda m: good[m]["sec"])
    bctx, bmode, b2d = ctxs[best]
    diag["mode"] = best
    diag["fallback"] = bool(wd)
    diag["parallelism"] = good[best]["layout"] + ", RCCL over xGMI"
    diag["grid"] = good[best]["layout"].split()[0]
    if wd:
        # a mode hung: its kernels still occupy the queues, so nothing more can be measured or checked in this process -
        # report the mode that completed, and leave without touching the GPU again
        _emit_and_exit_on_hang(args, rank, n, world, diag, good[best])
    if b2d:
        diag["launches_per_factor_rank0"] = good[best]["launches_per_factor_rank0"]
    if list(results)[-1] != best and not b2d:        # leave the plan holding the result (and the mode, for the profiled call) of the reported mode
        bctx.set_option("safe", 1 if bmode == "safe" else 0)
        bctx.set_option("ipc", 1 if (bmode == "ipc" or args.exchange == "ipc") else 0)
        bctx.factor(); torch.cuda.synchronize()
    elif list(results)[-1] != best:
        bctx.factor(); torch.cuda.synchronize()
    return bctx, good[best]["sec"], good[best]["info"], diag


def _emit_and_exit_on_hang(args, rank, n, world, diag, res):
    if rank == 0:
        par = diag.pop("parallelism", "")
        out = {"metric": "fp64 Cholesky TFLOP/s (N^3/3 per wall-second of one warm factor call), N=%d" % n,
               "value": res["tflops"] if res else None, "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": res["sec"] * 1e3 if res else None, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
               "dtype": "f64", "data": "synthetic", "fallback": True,
               "config": dict({"workload": "N=%d fp64 Cholesky A=R^T R, upstream distribute_symmetric(diag-dominant) input generated on the "
                                           "GPU, resident in HBM; complete_inv=-1" % n, "parallelism": par,
                               "info": res["info"] if res else -1, "residual": res["probe"] if res else None, "residual_kind": "probe",
                               "pct_of_fp64_mfma_peak_per_gpu": 100.0 * res["tflops"] / (FP64_MFMA_PEAK_TF * world) if res else None}, **diag)}
        if not res:
            out["error"] = "no mode of the multi-GPU schedule completed (see config.watchdog)"
        print(json.dumps(out), flush=True)
    sys.stdout.flush(); sys.stderr.flush()
    time.sleep(1.0)
    os._exit(0 if res else 1)


BF16_MFMA_PEAK_TF = 2500.0    # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md; the 5 PF headline figure includes 2:1 sparsity)


def bench_mixed(args, torch, L, C, rank, world, timed):
    """Mixed-precision Cholesky solve on ONE GPU: a step = bf16-MFMA factorization + fp64 iterative refinement of 8 right-hand
    sides to fp64 accuracy; value = fp64-equivalent TFLOP/s (N^3/3 per second of factor + solve)."""
    if world != 1:
        return bench_mixed_dist(args, torch, L, C, rank, world, timed)
    from capital_amd import blas, cholinv, mixed
    from capital_amd.matrix import matrix
    n, nrhs = args.n, 8
    A = matrix(n, n, 1, 1); A.distribute_symmetric(0, 0, 1, 1, 0, True)
    B = matrix(nrhs, n, 1, 1); B.distribute_random(0, 0, 1, 1, 7)
    p = mixed.plan(n, nrhs)
    res = {}

    def step():
        p.factor(A)
        res["x"] = p.solve(A, B, max_iter=30, tol=1e-15)
    sec = timed(step, args.steps, args.warmup)
    X, sweeps, relres = res["x"]
    info = p.last_info()
    dump_outputs(args, [("X", X.view(), False)])
    tf_only = timed(lambda: p.factor(A), 2, 0)
    tflops = n ** 3 / 3.0 / sec / 1e12
    # check 1: ||A X - B||_F / ||B||_F recomputed with torch's fp64 matmul (rocBLAS), not this library's kernels.  A plain K = N
    # product sums N / 4 MFMA accumulations in a chain: its own rounding error is ~5e-15 of ||B|| at N = 65536 (rocBLAS and this
    # library's tile kernel share the MT128x128x16 / MI16x16x4 summation order - their results agreed bit for bit in round 2), so
    # the same norm is also taken from 1024-column partial products summed by torch's cascade summation (independent_residual_
    # chunked): that one can see the accuracy the refinement reaches with its compensated residual kernel (gemm.hip, skinny TN).
    r = A.view() @ X.view() - B.view()
    bn = float(B.view().norm())
    indep = float(r.norm() / bn)
    parts = torch.stack([A.view()[:, c0:c0 + 1024] @ X.view()[c0:c0 + 1024] for c0 in range(0, n, 1024)])
    indep_chunked = float((parts.sum(0) - B.view()).norm() / bn)
    Xp = X.view().clone(); Xp[0, 0] *= (1.0 + 1e-8)
    indep_perturbed = float((A.view() @ Xp - B.view()).norm() / bn)
    del r, Xp, parts
    # check 2: the same system through the fp64 path of this library (blocked Cholesky + two blocked TRSMs): a different algorithm
    x_diff = None
    if not args.no_check:
        pack = cholinv.info(-1, 1, -5, 'U'); cholinv.factor(A, pack, None)
        R = cholinv.construct_R(pack)
        Xf = matrix(nrhs, n, 1, 1); Xf.view().copy_(B.view())
        for trans in (1, 0):
            blas.engine._trsm(R.data(), Xf.data(), n, nrhs, R.ld(), Xf.ld(),
                              blas.ArgPack_trmm(blas.Order.AblasColumnMajor, blas.Side.AblasLeft, blas.UpLo.AblasUpper, blas.Transpose(trans),
                                                blas.Diag.AblasNonUnit, 1.0))
        x_diff = float((X.view() - Xf.view()).norm() / Xf.view().norm())
        del pack, R, Xf
        torch.cuda.empty_cache()
    ok = (int(info) == 0 and relres == relres and relres <= 1e-14 and indep <= 1e-13 and indep_chunked <= 1e-14 and indep_perturbed > 10 * indep
          and (x_diff is None or x_diff <= 1e-12))
    # roofline of the dominant kernel (bf16 trailing update), measured live with HIP events on its launch stream
    nl, ms, fl, by = p.profile_update(A)
    roof = {"bound": "hbm", "kernel": "bf16_tn3x_kernel (csrc/bf16_tn3.hip; trailing update C32 -= S16^T S16: fp32 C read-modify-write, K/4 flop per byte)",
            "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None}
    if nl:
        gbs, tf16 = by / (ms * 1e-3) / 1e9, fl / (ms * 1e-3) / 1e12
        intensity, ridge = fl / by, BF16_MFMA_PEAK_TF * 1e12 / (HBM_PEAK_GBS * 1e9)
        hbm = {"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}
        mfma = {"achieved": tf16, "peak": BF16_MFMA_PEAK_TF, "unit": "TFLOP/s (bf16, dense)", "frac": tf16 / BF16_MFMA_PEAK_TF}
        # the roof that binds is the one the kernel's algorithmic intensity puts it under (K = 2048 strips: 512 flop/B > ridge 312)
        roof.update(mfma if intensity > ridge else hbm)
        roof.update({"bound": "mfma" if intensity > ridge else "hbm", "launches": nl, "avg_launch_ms": ms / nl,
                     "algorithmic_bytes_per_launch_avg": by / nl, "algorithmic_flops_per_launch_avg": fl / nl,
                     "flop_per_byte": intensity, "ridge_flop_per_byte": ridge, "hbm": hbm, "mfma": mfma})
    out = {"metric": "fp64-equivalent Cholesky-solve TFLOP/s (N^3/3 per wall-second of bf16-MFMA factor + fp64 refinement), N=%d" % n,
           "value": tflops if ok else None, "unit": "TFLOP/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": sec * 1e3,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "bf16 MFMA (fp32 accumulate) factor, f64 refinement",
           "data": "synthetic",
           "config": {"workload": "N=%d mixed-precision Cholesky solve, %d right-hand sides, upstream distribute_symmetric input resident in HBM" % (n, nrhs),
                      "parallelism": "1 GPU", "info": int(info), "refinement_sweeps": int(sweeps), "residual": relres,
                      "residual_kind": "||B - A X||_F/||B||_F (fp64, library kernels)", "independent_residual": indep,
                      "independent_residual_kind": "same norm with torch fp64 matmul (rocBLAS, one K = N product: its summation chain rounds at "
                                                   "~5e-15); _chunked: 1024-column partial products + cascade sum; after scaling X[0,0] by "
                                                   "1+1e-8 the plain norm reads independent_residual_perturbed",
                      "independent_residual_chunked": indep_chunked, "independent_residual_perturbed": indep_perturbed,
                      "x_vs_fp64_path": x_diff, "factor_ms": tf_only * 1e3, "factor_fp64_equiv_tflops": n ** 3 / 3.0 / tf_only / 1e12},
           "roofline": roof}
    if not ok:
        out["error"] = "mixed-precision solve failed its parity gate"
    p.close()
    if not getattr(args, "no_cpu_baseline", False):
        out["cpu_baseline"] = cpu_baseline(args.cpu_n, args.cpu_budget_s)     # the reference has no solve path: its fp64 factor is the comparator
    return out, ok


def bench_mixed_dist(args, torch, L, C, rank, world, timed):
    """BASELINE config 5 as stated (N = 131072 on 8 GPUs with `--size 131072`): the mixed-precision solve on the 1 x P
    block-column-cyclic layout (csrc/dist_mixed.hip): bf16-MFMA factorization with all-gathered bf16 panels + distributed fp64
    refinement of 8 right-hand sides.  value = fp64-equivalent TFLOP/s of the whole job (N^3/3 per second of factor + solve)."""
    import torch.distributed as dist
    from capital_amd import _lib, dist_cholesky, mixed
    from capital_amd.matrix import matrix
    emulate = os.environ.get("CAPITAL_BENCH_EMULATE") == "1"
    n, nrhs = args.n, 8
    if emulate:
        from tests.host_staged import HostStagedComm
        comm = HostStagedComm()
    else:
        comm = dist_cholesky.RcclComm()
    nb = args.nb or 1024
    p = mixed.dist_plan(n, comm, nb=nb, nrhs_max=nrhs)
    lc = p.local_cols
    Al = torch.zeros(max(lc, 1), n, dtype=torch.float64, device="cuda")
    _lib.check(L.cap_fill_symmetric_bc(Al.data_ptr(), n, n, nb, world, rank, 1, None), "cap_fill_symmetric_bc")
    B = matrix(nrhs, n, 1, 1); B.distribute_random(0, 0, 1, 1, 7)          # the same right-hand sides on every rank
    res = {}

    def step():
        p.factor(Al)
        res["x"] = p.solve(Al, B, max_iter=30, tol=1e-15)
    sec = timed(step, args.steps, args.warmup)
    X, sweeps, relres = res["x"]
    info = p.last_info()
    tf_only = timed(lambda: p.factor(Al), 2, 0)
    # independent check with torch's fp64 matmul over my rows of A X (A is symmetric: rows = my block columns), summed over the ranks
    cols = torch.from_numpy(dist_cholesky.global_cols_of_rank(n, nb, world, rank)).cuda()
    num = torch.zeros(2, dtype=torch.float64, device="cuda")
    if lc:
        r_my = Al[:lc] @ X.view() - B.view()[cols]
        num[0] = (r_my * r_my).sum(); num[1] = (B.view()[cols] ** 2).sum()
    if emulate:
        h = num.cpu(); dist.all_reduce(h); num = h
    else:
        dist.all_reduce(num)
    indep = float(torch.sqrt(num[0] / num[1]))
    ok = int(info) == 0 and relres == relres and relres <= 1e-14 and indep <= 1e-13
    tflops = n ** 3 / 3.0 / sec / 1e12
    out = {"metric": "fp64-equivalent Cholesky-solve TFLOP/s (N^3/3 per wall-second of bf16-MFMA factor + fp64 refinement), N=%d" % n,
           "value": tflops if ok else None, "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": sec * 1e3,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "bf16 MFMA (fp32 accumulate) factor, f64 refinement",
           "data": "synthetic",
           "config": {"workload": "N=%d mixed-precision Cholesky solve, %d right-hand sides, upstream distribute_symmetric input generated on the "
                                  "GPUs in the block-column-cyclic layout, resident in HBM" % (n, nrhs),
                      "parallelism": "1x%d block-cyclic columns (nb=%d): bf16 panels all-gathered, distributed refinement; RCCL over xGMI" % (world, nb),
                      "info": int(info), "refinement_sweeps": int(sweeps), "residual": relres,
                      "residual_kind": "||B - A X||_F/||B||_F (fp64, library kernels)", "independent_residual": indep,
                      "factor_ms": tf_only * 1e3, "factor_fp64_equiv_tflops": n ** 3 / 3.0 / tf_only / 1e12},
           "roofline": {"bound": "hbm", "kernel": "bf16_tn_kernel (staircase form, gathered bf16 A operand)", "achieved": None, "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": None, "traffic": None}}
    if not ok:
        out["error"] = "distributed mixed-precision solve failed its parity gate"
    p.close()
    if rank == 0 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.cpu_n, args.cpu_budget_s)     # the reference has no solve path: its fp64 factor is the comparator
    return out, ok


def bench_summa(args, torch, L, C, rank, world, timed):
    """SUMMA on one GPU (d = c = 1: the carrier's plan, streams and events around the local MFMA products) - the reference's
    bench/matmult/summa_gemm.cpp:7-55 protocol (warm call, timed calls) for its GEMM overload (NoTrans x NoTrans, the only form that
    bench runs), the SYRK overload in its Trans form (C = A^T A, summa.hpp:98-161: the TN product of the Cholesky update) and a tall-K
    GEMM, each with its own roofline and a check against torch's fp64 matmul on a probe."""
    from capital_amd import blas, summa, topo
    from capital_amd.matrix import matrix
    T = topo.square(1, 0, 4)
    forms, ok = [], True
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    steps = args.steps or 5
    for (name, kind, M, N, K) in (("GEMM NN 8192^3", "gemm", 8192, 8192, 8192), ("SYRK Trans (TN) n=8192 k=8192", "syrk", 8192, 8192, 8192),
                                  ("GEMM NN tall-K 4096 x 4096 x 65536", "gemm", 4096, 4096, 65536)):
        if kind == "gemm":
            A = matrix(K, M, 1, 1); B = matrix(N, K, 1, 1); Cm = matrix(N, M, 1, 1)
            A.distribute_random(0, 0, 1, 1, 0); B.distribute_random(0, 0, 1, 1, 1000)
            pack = blas.ArgPack_gemm(blas.Order.AblasColumnMajor, blas.Transpose.AblasNoTrans, blas.Transpose.AblasNoTrans, 1.0, 0.0)
            run = lambda: summa.invoke(A, B, Cm, T, pack)
            flops = 2.0 * M * N * K
        else:
            A = matrix(N, K, 1, 1); Cm = matrix(N, N, 1, 1)            # A: K x N, C = A^T A (upper)
            A.distribute_random(0, 0, 1, 1, 0)
            pack = blas.ArgPack_syrk(blas.Order.AblasColumnMajor, blas.UpLo.AblasUpper, blas.Transpose.AblasTrans, 1.0, 0.0)
            run = lambda: summa.invoke(A, Cm, T, pack)
            flops = 1.0 * N * (N + 1) * K
        sec = timed(run, steps, args.warmup)
        dump_outputs(args, [("C_%s_%dx%dx%d" % (kind, M, N, K), Cm.view(), kind == "syrk")])
        tf = flops / sec / 1e12
        err = None
        if not args.no_check:
            # probe: a 256 x 256 block of C (inside the upper triangle for SYRK) against torch's fp64 matmul of the operand slices
            r0, c0 = 128, N - 512
            Cv = Cm.view()[r0:r0 + 256, c0:c0 + 256]
            if kind == "gemm":
                ref = A.view()[r0:r0 + 256, :] @ B.view()[:, c0:c0 + 256]
            else:
                ref = A.view()[:, r0:r0 + 256].t() @ A.view()[:, c0:c0 + 256]
            err = float((Cv - ref).norm() / ref.norm())
            ok = ok and err == err and err <= 1e-13
        extra_f = {} if kind == "gemm" else {"executed_tflops": 2.0 * N * N * K / sec / 1e12,
                                             "note": "like upstream's SYRK overload (summa.hpp:98-161) the carrier forms the full product A^T A: 2 n^2 k flops are executed, "
                                                     "n (n + 1) k are counted in `value`"}
        forms.append({"form": name, "M": M, "N": N, "K": K, "value": tf, **extra_f, "unit": "TFLOP/s", "ms_per_step": sec * 1e3, "steps": steps, "probe_rel_err": err,
                      "roofline": {"bound": "mfma", "kernel": "dgemm_tn_dma_kernel (%s)" % ("A_MC: M-contiguous A" if kind == "gemm" else "K-contiguous operands, upper tiles"),
                                   "achieved": tf, "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": tf / FP64_MFMA_PEAK_TF, "traffic": None,
                                   "algorithmic_flops_per_step": flops}})
        del A, Cm
        if kind == "gemm": del B
        summa.release(T)
        torch.cuda.empty_cache()
    T.close()
    best = forms[0]
    out = {"metric": "fp64 SUMMA GEMM TFLOP/s (2 M N K per wall-second of one warm summa::invoke, bench/matmult/summa_gemm.cpp:39-52), 8192^3 on 1 GPU",
           "value": best["value"], "unit": "TFLOP/s", "n_gpus": world, "steps": steps, "warmup": args.warmup, "ms_per_step": best["ms_per_step"],
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "SUMMA (matmult::summa::invoke) on the 1 x 1 x 1 grid: GEMM NN 8192^3 (headline of this line), SYRK Trans 8192 x 8192 x 8192, "
                                  "GEMM NN 4096 x 4096 x 65536; upstream distribute_random operands generated on the GPU", "forms": forms},
           "roofline": best["roofline"]}
    if not ok:
        out["value"] = None; out["error"] = "a SUMMA form failed its probe against torch's fp64 matmul"
    return out, ok


def bench_cacqr(args, torch, L, C, rank, world, dist, emulate, timed, allreduce_sum):
    """CholeskyQR2 on the 1D grid (c = 1, d = world): m rows per GPU (row-cyclic), n columns; one Gram all-reduce per sweep."""
    from capital_amd import _lib, cacqr, cholinv, validate, dist_cholesky
    from capital_amd.matrix import matrix
    m, n = args.qr_rows, args.qr_cols

    class Topo:
        pass
    topo = None
    if world > 1:
        if emulate:
            from tests.host_staged import HostStagedComm      # tests only (CAPITAL_BENCH_EMULATE=1)
            comm = HostStagedComm()
        else:
            comm = dist_cholesky.RcclComm()
        topo = Topo(); topo.c, topo.d, topo.x, topo.y, topo.z = 1, world, 0, rank, 0
        topo.rank, topo.size, topo.world = rank, world, comm.handle
    A = matrix(n, m * world, 1, world)
    A.distribute_random(0, rank, 1, world, rank)            # key = rank / c (bench/qr/cacqr.cpp:34)
    pack = cacqr.info(2, cholinv.info(1, 1, 0, 'U'))
    sec = timed(lambda: cacqr.factor(A, pack, topo), args.steps, args.warmup)
    info = pack.last_info()
    if args.dump_outputs:
        Q, R = cacqr.construct_Q(pack), cacqr.construct_R(pack)
        dump_outputs(args, [("Q", Q.view(), False), ("R", R.view(), True)])
        del Q, R
    flops = 4.0 * m * world * n * n
    abytes = 6.0 * 8 * m * n                                 # per GPU: 2 sweeps x (read A for the Gram + read A, write Q)
    tflops = flops / sec / 1e12
    out = {"metric": "fp64 CholeskyQR2 TFLOP/s (4 m n^2 per wall-second of one warm factor call), %d x %d per GPU" % (m, n),
           "value": tflops, "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": sec * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f64", "data": "synthetic",
           "config": {"workload": "CholeskyQR2 (cacqr 1D, num_iter=2) of a %d x %d matrix, %d rows per GPU row-cyclic, upstream "
                                  "distribute_random input generated on the GPU, resident in HBM" % (m * world, n, m),
                      "parallelism": "1D row-cyclic over %d GPU(s), Gram all-reduce on RCCL" % world, "info": int(info),
                      "pct_of_fp64_mfma_peak_per_gpu": 100.0 * tflops / (FP64_MFMA_PEAK_TF * world),
                      "algorithmic_GBps_per_gpu": abytes / sec / 1e9}}
    ok = int(info) == 0
    if not args.no_check:
        res = validate.qr.residual(A, pack, topo); orth = validate.qr.orthogonality(A, pack, topo)
        out["config"]["residual"] = res; out["config"]["orthogonality"] = orth
        ok = ok and res == res and res <= 1e-13 and orth <= 1e-15
    if rank == 0:
        # per-GPU roofline of the whole factor call.  The four passes (2 sweeps x Gram + Q R^-1) need 4 m n^2 flops = 7.0 ms
        # of fp64 MFMA at n = 256 against 6*8*m*n bytes = 3.2 ms of HBM: the binding roof is MFMA; the HBM fraction is kept
        # beside it
        kern = ("gram256_kernel + qrapply256_kernel (csrc/cqr_kernels.hip)" if n == 256 and m % 128 == 0
                else "split-K DSYRK + streaming Q R^-1 on dgemm_tn_dma_kernel")
        out["roofline"] = {"bound": "mfma", "kernel": "cacqr sweeps: %s, whole factor call" % kern,
                           "achieved": tflops / world, "peak": FP64_MFMA_PEAK_TF, "unit": "TFLOP/s",
                           "frac": tflops / world / FP64_MFMA_PEAK_TF, "traffic": None,
                           "hbm_frac": abytes / sec / 1e9 / HBM_PEAK_GBS, "algorithmic_GBps": abytes / sec / 1e9,
                           "algorithmic_bytes_per_step": abytes, "algorithmic_flops_per_step_per_gpu": flops / world}
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_cacqr(m, n)
    if not ok:
        out["value"] = None
        out["error"] = "CholeskyQR2 failed its parity gate"
    return out, ok


if __name__ == "__main__":
    main()
