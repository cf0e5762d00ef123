"""Multi-rank coverage.
 not gpu : world_size-2/3 gloo runs of the block-cyclic index logic + ragged gather assembly (CPU only)
 gpu     : the real schedule (csrc/dist.hip, HIP kernels) with 1, 2 and 4 ranks sharing cuda:0 through the
           host-staged gloo communicator; result vs oracle.  The RCCL path differs only in the three
           collectives (cap_comm_*), exercised at P = 1 here and at P = 2/4/8 by the driver's scaling run."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# BLAS pool size of a worker process: the workers pin themselves to ONE thread (tests/dist_worker.py) except rank 0, whose oracle
# checks (a NumPy Cholesky and an R^T R product per case - 40 s at n = 8192 on one thread) may use the pool
_WORKER_THREADS = str(max(1, min(16, (os.cpu_count() or 1) // 2)))


def _launch(nproc, mode, n, nb, port, extra=()):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker.py"), "--mode", mode, "--size", str(n),
           "--nb", str(nb)] + [str(x) for x in extra]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS=_WORKER_THREADS)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        # keep the complete output of a failing multi-rank run (the assertion message only shows its tail)
        d = os.path.join(ROOT, "gpurun_out")
        try:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "dist_fail_%s_%d_%d.log" % (mode, nproc, port)), "w") as f:
                f.write(" ".join(cmd) + "\n---- stdout\n" + r.stdout + "\n---- stderr\n" + r.stderr)
        except OSError:
            pass
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# One launch per rank count.  A torch.distributed.run start costs 5 - 10 s per rank set on the GPU box (python + torch import per
# rank, rendezvous) - two thirds of the suite's wall time in round 4 - while a case itself runs for a second or two.  Every
# multi-rank GPU case of this module is therefore registered at collection time (tests/conftest.py, only the SELECTED tests) and the
# first test of a rank count runs ALL registered cases of that count inside one launch (tests/dist_worker.py --cases); the others
# read their own segment of that output.  A case that fails ends its launch (a failed rank leaves its peers inside a collective);
# the cases behind it are then run one launch each, so every test still reports its own result.  CAPITAL_TEST_NOBATCH=1 = one
# launch per test as before.
_REGISTERED = {}          # nproc -> {case id: argv}
_RESULTS = {}             # case id -> result


class _Result:
    def __init__(self, returncode, stdout, stderr=""):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr


def _argv(mode, n, nb, extra):
    return ["--mode", mode, "--size", str(n), "--nb", str(nb)] + [str(x) for x in extra]


def _case_id(nproc, mode, n, nb, extra):
    return "p%d %s" % (nproc, " ".join(_argv(mode, n, nb, extra)))


def register_case(nproc, mode, n, nb, extra=()):
    _REGISTERED.setdefault(int(nproc), {})[_case_id(nproc, mode, n, nb, extra)] = _argv(mode, n, nb, extra)


def _run_batch(nproc):
    import json
    import tempfile
    todo = [(cid, argv) for cid, argv in _REGISTERED.get(nproc, {}).items() if cid not in _RESULTS]
    if not todo:
        return
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump([{"id": cid, "argv": argv} for cid, argv in todo], f)
    worker = [os.path.join(ROOT, "tests", "dist_worker.py"), "--cases", f.name]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(29500 + nproc)] + worker
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS=_WORKER_THREADS)
    timeout = 120 + 60 * len(todo)
    try:
        if nproc >= _MAX_GPU_PROCS:
            rc, out, err = _spawn_ranks(nproc, worker, 29500 + nproc, env, timeout)
        else:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
            out, err, rc = r.stdout, r.stderr, r.returncode
    except subprocess.TimeoutExpired as e:
        out = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = "batch launch timed out"; rc = -9
    finally:
        os.unlink(f.name)
    seg, cur = {}, None
    for line in out.splitlines():
        if line.startswith("CASE-BEGIN "):
            cur = line[len("CASE-BEGIN "):]; seg[cur] = {"lines": [], "ended": False}
        elif line.startswith("CASE-END ") and cur is not None:
            seg[cur]["ended"] = True
        elif cur is not None:
            seg[cur]["lines"].append(line)
    for cid, _ in todo:
        if cid in seg and seg[cid]["ended"]:
            _RESULTS[cid] = _Result(0, "\n".join(seg[cid]["lines"]))
        elif cid in seg:                      # the case the launch died in
            _RESULTS[cid] = _Result(rc or 1, "\n".join(seg[cid]["lines"]), err[-3000:])
            try:
                d = os.path.join(ROOT, "gpurun_out"); os.makedirs(d, exist_ok=True)
                with open(os.path.join(d, "dist_fail_batch_p%d.log" % nproc), "w") as g:
                    g.write(" ".join(cmd) + "\n---- stdout\n" + out + "\n---- stderr\n" + err)
            except OSError:
                pass
        # (cases behind a failed one: no entry - run alone on demand)
    return err


# At most 16 processes may hold the GPU at once.  A torch.distributed.run agent initialises the HIP runtime itself (its launch
# config asks torch.cuda.is_available()), and so does this pytest process once a GPU test has run in it.  A launch of 16 ranks
# therefore starts its ranks directly (_spawn_ranks) and runs at collection time, before any test has touched the GPU
# (run_wide_batches, called by tests/conftest.py).
_MAX_GPU_PROCS = 16


def _spawn_ranks(nproc, worker, port, env, timeout):
    """The ranks of one launch as plain child processes with the environment torch.distributed.run would give them; like the
    launcher, the first rank that fails ends the others.  Returns (returncode, stdout of rank 0 followed by the others', stderr)."""
    import tempfile
    import time
    logs = [(tempfile.TemporaryFile("w+"), tempfile.TemporaryFile("w+")) for _ in range(nproc)]
    procs = [subprocess.Popen([sys.executable] + worker, stdout=o, stderr=e, text=True,
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(nproc), LOCAL_WORLD_SIZE=str(nproc),
                                       MASTER_PORT=str(port)))
             for r, (o, e) in enumerate(logs)]
    deadline, timed_out = time.monotonic() + timeout, False
    while any(p.poll() is None for p in procs):
        timed_out = time.monotonic() > deadline
        if any(p.returncode for p in procs) or timed_out:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            break
        time.sleep(0.2)
    for p in procs:
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill(); p.wait()
    rc = -9 if timed_out else next((p.returncode for p in procs if p.returncode), 0)
    text = []
    for o, e in logs:
        o.seek(0); e.seek(0)
        text.append((o.read(), e.read()))
        o.close(); e.close()
    err = "".join(e for _, e in text) + ("\nbatch launch timed out" if timed_out else "")
    return rc, "".join(o for o, _ in text), err


def run_wide_batches():
    """Run every registered case of 16 or more ranks now (tests/conftest.py calls this once the tests are collected): one launch per
    rank count, and after a case that failed one more launch for the cases behind it, so that each has a result before any test runs."""
    for nproc in sorted(p for p in _REGISTERED if p >= _MAX_GPU_PROCS):
        while True:
            todo = [cid for cid in _REGISTERED[nproc] if cid not in _RESULTS]
            if not todo:
                break
            err = _run_batch(nproc)
            if todo[0] not in _RESULTS:                 # the launch ended before its first case began
                for cid in todo:
                    _RESULTS[cid] = _Result(1, "", err[-3000:])


def _case(nproc, mode, n, nb, extra=(), port=29700):
    cid = _case_id(nproc, mode, n, nb, extra)
    if int(nproc) >= _MAX_GPU_PROCS:
        return _RESULTS.get(cid) or _Result(1, "", "a case of %d ranks runs at collection time only (run_wide_batches)" % nproc)
    if os.environ.get("CAPITAL_TEST_NOBATCH") != "1" and cid in _REGISTERED.get(int(nproc), {}):
        if cid not in _RESULTS:
            _run_batch(int(nproc))
        if cid in _RESULTS:
            return _RESULTS[cid]
    return _launch(nproc, mode, n, nb, port + int(nproc), extra)


@pytest.mark.parametrize("nproc,n,nb", [(2, 1024, 128), (3, 1000, 100), (2, 640, 256)])
def test_block_cyclic_index_logic_gloo(nproc, n, nb):
    r = _launch(nproc, "index", n, nb, 29611 + nproc)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "INDEX-OK" in r.stdout


def test_topo_coords_match_reference_formulas():
    """cap_topo_coords (pure, no GPU) against the rank -> (x, y, z) maps of topology.h:44-50,75-83."""
    so = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    import ctypes as C
    from capital_amd import _lib
    L = _lib.lib()
    for kind, size, c in [(0, 8, 2), (0, 1, 1), (0, 4, 1), (0, 27, 3), (0, 16, 1), (1, 8, 1), (1, 8, 2), (1, 16, 2), (1, 4, 1)]:
        for rank in range(size):
            d, x, y, z = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            assert L.cap_topo_coords(kind, rank, size, c, C.byref(d), C.byref(x), C.byref(y), C.byref(z)) == 0
            if kind == 0:
                dd = int(round((size / c) ** 0.5)); top = dd * c
                want = (dd, (rank % top) // c, rank // top, rank % c)
            else:
                want = (size // (c * c), (rank % (c * c)) // c, rank // (c * c), rank % c)
            assert (d.value, x.value, y.value, z.value) == want
    d = C.c_int()
    assert L.cap_topo_coords(0, 0, 6, 1, C.byref(d), C.byref(d), C.byref(d), C.byref(d)) != 0      # 6 is no d*d*c grid


def test_index_helpers_match_library_when_built():
    """The pure-Python maps agree with the C helpers the schedule uses (cap_bc_*); skipped if the .so is absent."""
    so = os.path.join(ROOT, "capital_amd", "lib", "libcapital_amd.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    from capital_amd import _lib, dist_cholesky as dc
    L = _lib.lib()
    for (n, nb, P) in [(4096, 512, 8), (1024, 128, 3), (65536, 512, 8), (2048, 256, 1), (1000, 128, 3), (2049, 256, 4)]:
        nblk = (n + nb - 1) // nb
        tot = 0
        for p in range(P):
            assert L.cap_bc_num_local_cols(n, nb, P, p) == dc.global_cols_of_rank(n, nb, P, p).size
            tot += dc.global_cols_of_rank(n, nb, P, p).size
        assert tot == n
        for J in range(0, nblk, 3):
            assert L.cap_bc_owner(J, P) == dc.owner(J, P) and L.cap_bc_local_block(J, P) == dc.local_block(J, P)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,n,nb", [(1, 1024, 128), (2, 1024, 128), (4, 2048, 128), (3, 1536, 256), (2, 2048, 512),
                                        (8, 8192, 512)])   # the driver's 8-GPU shape: P = 8, nb = 512 (2 block columns per rank)
def test_multirank_schedule_on_one_gpu(nproc, n, nb):
    r = _case(nproc, "gpu", n, nb)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DIST-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,n,nb,extra", [
    (3, 1000, 128, ()),                                   # ragged N: identity-padded last block (policy.h:196 `span`)
    (2, 2047, 256, ()), (4, 2049, 128, ()),               # the reference's own odd sizes (matrix.hpp:8-11)
    (2, 2048, 128, ("--strip", 1, "--depth2", 0)),        # schedule knobs change the association order only
    (4, 4096, 128, ("--strip", 2, "--depth2", 1)),
    (2, 2048, 256, ("--seam", 1)),                        # through cholinv::factor(A, pack, topo)
    (4, 4096, 128, ("--safe", 1)),                        # one communicator, one communication stream: collectives in program order
    (3, 1000, 128, ("--safe", 1, "--strip", 1)),
    (8, 8192, 512, ("--safe", 1)),
    # strip exchange by IPC peer copies (hipIpcOpenMemHandle of the peers' gathered-strip buffers, pushes on per-peer copy
    # streams, two 8-byte all-reduces as barriers) instead of the all-gather collective
    (2, 2048, 128, ("--ipc", 1)), (4, 4096, 128, ("--ipc", 1, "--safe", 1)), (3, 1000, 128, ("--ipc", 1)), (8, 8192, 512, ("--ipc", 1)),
    (4, 4096, 128, ("--ipc", 1, "--jitter", 200)),
])
def test_multirank_schedule_variants(nproc, n, nb, extra):
    r = _case(nproc, "gpu", n, nb, extra)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DIST-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,n,nb,jitter", [(2, 4096, 128, 300), (4, 4096, 128, 200), (3, 3072, 256, 500)])
def test_multirank_schedule_under_random_stream_delays(nproc, n, nb, jitter):
    """Event-edge stress: every launch group of the four streams is preceded by a spin kernel of random length (different
    per rank), and the host-staged collectives only wait for their own stream - a missing dependency between the panel /
    msg / comm / main streams changes R."""
    r = _case(nproc, "gpu", n, nb, ("--jitter", jitter))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DIST-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,n,nb,extra", [
    (4, 1024, 128, ("--ci", 1)),                                  # R and R^-1 on P > 1 (cholinv.hpp:85-165 semantics)
    (4, 1024, 128, ("--ci", 0)),                                  # root partition 512 on a block boundary: columns >= 512 stop at block row 4
    (3, 1024, 128, ("--ci", 0, "--split", 2)),                    # n >> 2 = 256
    (3, 1000, 128, ("--ci", 0)),                                  # ragged N, root partition 500 inside a block: cleared afterwards
    (2, 1536, 256, ("--ci", 1, "--safe", 1)),
    (8, 4096, 512, ("--ci", 1)),
    (2, 2048, 256, ("--ci", 1, "--seam", 1)),                     # through cholinv::factor / construct_Rinv with a multi-rank topo
    (1, 1024, 128, ("--ci", 0)),
    # the streamed inverse under random per-stream delays (its steps run on their own stream behind "block row k is solved"), with the
    # IPC strip exchange, and with more steps
    (4, 2048, 128, ("--ci", 1, "--jitter", 300)), (3, 1536, 128, ("--ci", 0, "--jitter", 200)), (4, 2048, 128, ("--ci", 1, "--ipc", 1)),
    (2, 4096, 128, ("--ci", 1)), (8, 8192, 512, ("--ci", 0, "--safe", 1)),
])
def test_distributed_inverse_matches_oracle(nproc, n, nb, extra):
    r = _case(nproc, "gpu", n, nb, extra)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DIST-OK" in r.stdout and "DISTINV-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cholinv_p8_n128_ci1_s1_bc-2.npz", "cholinv_p8_n192_ci0_s1_bc-3.npz", "cholinv_p8_n250_ci1_s1_bc-2.npz"])
def test_distributed_factors_match_the_8rank_reference_dumps(name):
    """The REAL reference on 8 MPI ranks (2 x 2 x 2 grid, element-cyclic) and this library on 8 ranks (1 x 8 block columns):
    same input, same knobs -> the gathered R and R^-1 agree, including which part of R^-1 stays empty."""
    r = _case(8, "gpu", 128, 128, ("--golden", name))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DIST-OK" in r.stdout and "DISTINV-OK" in r.stdout and "golden=ok" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,pr,n,nb", [
    (4, 2, 2048, 128),        # 2 x 2
    (8, 2, 4096, 128),        # 2 x 4: the node's 8 GPUs, two A-operand contributors per process row
    (8, 2, 8192, 512),        # 2 x 4 at the driver's block size
    (4, 2, 1000, 128),        # ragged N: identity-padded last block
    (8, 2, 2049, 256),
    (4, 1, 2048, 128),        # 1 x 4 through the 2D code: every column contributes to the A operand (cross-check of dist.hip)
    (2, 1, 1536, 256),
    (4, 4, 1536, 128),        # 4 x 1 is refused (Pr must divide Pc) - see below; 4 = 2 x 2 only
    (16, 4, 4096, 128),       # 4 x 4
    (1, 1, 1024, 128),
])
def test_2d_block_cyclic_schedule_on_one_gpu(nproc, pr, n, nb):
    """The Pr x Pc block-cyclic plan (csrc/dist2d.hip) with all ranks sharing cuda:0: generator, factor, construct_R and the
    distributed probe against the oracle; row / column communicators are host-staged gloo groups."""
    if nproc // pr % pr:
        # not a supported grid: the plan must refuse it (status, no hang)
        r = _case(nproc, "gpu2d", n, nb, ("--pr", pr, "--expect-fail", "cap_dist2d_plan_create"))
        assert r.returncode == 0 and "REFUSED-OK" in r.stdout, (r.stdout[-3000:] + r.stderr[-3000:])
        return
    r = _case(nproc, "gpu2d", n, nb, ("--pr", pr))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DIST2D-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,pr,n,nb,extra", [
    (4, 2, 4096, 128, ("--strip", 1, "--depth2", 0)),          # the round-3 schedule: one block row per update, look-ahead 1
    (4, 2, 4096, 128, ("--strip", 2, "--depth2", 0)),
    (8, 2, 4096, 128, ("--strip", 2, "--depth2", 1)),          # 2 x 4, strips of two block rows that live on different process rows
    (8, 2, 2049, 256, ("--strip", 2, "--depth2", 1)),          # ragged n, odd number of block rows (the last strip is one row)
    (16, 4, 4096, 128, ("--strip", 2,)),                       # 4 x 4
    (4, 1, 2048, 128, ("--strip", 2,)), (1, 1, 2048, 128, ("--strip", 2,)),
    (8, 2, 4096, 128, ("--safe", 1)),                          # one communicator family, collectives in program order
    (4, 2, 2048, 128, ("--ci", 1)), (8, 2, 2048, 128, ("--ci", 0)), (8, 2, 1000, 128, ("--ci", 0)),     # R^-1 streamed on the 2D grid
    (4, 2, 1024, 128, ("--ci", 0, "--split", 2)), (8, 2, 4096, 256, ("--ci", 1, "--safe", 1)), (1, 1, 1024, 128, ("--ci", 1)),
    (16, 4, 2048, 128, ("--ci", 1)),
    # both operand moves (solved row down the process columns, strip pieces along the process rows) as IPC peer copies
    (4, 2, 2048, 128, ("--ipc", 1)), (8, 2, 4096, 128, ("--ipc", 1)), (8, 2, 2049, 256, ("--ipc", 1, "--ci", 1)), (16, 4, 2048, 128, ("--ipc", 1)),
    (4, 1, 2048, 128, ("--ipc", 1)),
])
def test_2d_block_cyclic_schedule_options(nproc, pr, n, nb, extra):
    """The Pr x Pc plan at parity with the 1 x P plan: strips of two block rows (K = 2 nb updates), look-ahead depth 2, safe mode,
    R^-1 (complete_inv = 0 / 1) streamed with the sweep - against the oracle."""
    r = _case(nproc, "gpu2d", n, nb, ("--pr", pr) + tuple(extra))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DIST2D-OK" in r.stdout, r.stdout[-2000:]
    if "--ci" in extra:
        assert "DIST2DINV-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,n,nb", [(2, 1024, 128), (4, 2048, 256), (3, 1536, 128), (1, 1024, 256), (8, 8192, 512), (4, 1280, 256), (2, 1152, 256)])
@pytest.mark.parametrize("hard", [0, 1])
def test_distributed_mixed_precision_solve(nproc, n, nb, hard):
    """BASELINE config 5's method on P ranks sharing cuda:0: bf16-MFMA factorization on block columns (bf16 panels all-gathered,
    staircase bf16 update) + distributed fp64 refinement; X against numpy's fp64 solve, the fp32 factor against the fp64 one and
    against the one-rank factor of the same arithmetic (fp32 rounding level); hard = an input that is not diagonally dominant."""
    r = _case(nproc, "mixed", n, nb, ("--hard", hard))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DMP-OK" in r.stdout, r.stdout[-2000:]
    if "DMP-FLAKE" in r.stdout:
        # the worker's one-rank cross-check read a factor that was still being computed (seen once in round 5, see the comment in
        # tests/dist_worker.py and DESIGN.md section 9); the repeated read / factor agreed, so the case counts - but not silently
        import warnings
        warnings.warn("one-rank cross-check of the distributed mixed-precision factor had to be repeated:\n" +
                      "\n".join(l for l in r.stdout.splitlines() if "DMP-FLAKE" in l)[:2000])


@pytest.mark.gpu
def test_real_rccl_communicator_size1_runs_every_collective():
    """A REAL RCCL communicator (ncclCommInitRank, size 1) on this box's GPU: the distributed Cholesky schedule and
    CholeskyQR2 run their broadcast / all-gather / all-reduce through ncclBroadcast / ncclAllGather / ncclAllReduce, plus
    ncclCommSplit sub-communicators of the grid bundle."""
    import ctypes as C
    import torch
    from capital_amd import _lib, cacqr, cholinv, validate, dist_cholesky as dc
    from capital_amd.matrix import matrix
    L = _lib.lib()
    comm = dc.RcclComm(force_rccl=True)
    assert L.cap_comm_backend(comm.handle) == 1 and L.cap_comm_size(comm.handle) == 1
    # raw collectives
    x = torch.arange(1000, dtype=torch.float64, device="cuda")
    y = torch.zeros(1000, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.cap_comm_allreduce_sum(comm.handle, x.data_ptr(), 1000, s))
    _lib.check(L.cap_comm_bcast(comm.handle, x.data_ptr(), 1000, 0, s))
    _lib.check(L.cap_comm_allgather(comm.handle, x.data_ptr(), y.data_ptr(), 1000, s))
    _lib.check(L.cap_comm_reduce_sum(comm.handle, x.data_ptr(), 1000, 0, s))
    _lib.check(L.cap_comm_barrier(comm.handle, s))
    assert torch.equal(x.cpu(), torch.arange(1000, dtype=torch.float64)) and torch.equal(x, y)
    # sub-communicators + grid bundle through ncclCommSplit
    t = C.c_void_p()
    _lib.check(L.cap_topo_create(C.byref(t), 0, comm.handle, 1, 0, 0), "cap_topo_create")
    for which in (1, 2, 3, 4):
        sub = L.cap_topo_comm(t, which)
        assert sub and L.cap_comm_size(sub) == 1 and L.cap_comm_backend(sub) == 1
        _lib.check(L.cap_comm_allreduce_sum(sub, x.data_ptr(), 1000, s))
    torch.cuda.synchronize()
    assert [L.cap_topo_get(t, f) for f in range(7)] == [0, 1, 1, 1, 0, 0, 0]
    L.cap_topo_destroy(t)
    # SUMMA and the grid CholeskyQR path over size-1 RCCL sub-communicators (ncclCommSplit)
    from capital_amd import blas, summa, topo as tp
    Tq = tp.square(1, 0, 2, force_rccl=True)
    assert L.cap_comm_backend(Tq.row) == 1 and L.cap_comm_backend(Tq.depth) == 1
    Am = matrix(384, 512, 1, 1); Bm = matrix(256, 384, 1, 1); Cm = matrix(256, 512, 1, 1)
    Am.distribute_random(0, 0, 1, 1, 1); Bm.distribute_random(0, 0, 1, 1, 2)
    summa.invoke(Am, Bm, Cm, Tq, blas.ArgPack_gemm(blas.Order.AblasColumnMajor, blas.Transpose.AblasNoTrans, blas.Transpose.AblasNoTrans, 1.0, 0.0))
    assert np.linalg.norm(Cm.to_numpy() - Am.to_numpy() @ Bm.to_numpy()) / np.linalg.norm(Cm.to_numpy()) < 1e-14
    summa.release(Tq); Tq.close()
    # the distributed Cholesky schedule over it (also ragged N)
    for n, nb in ((4096, 512), (3000, 256)):
        ctx = dc.Context(n, nb, comm)
        ctx.fill_symmetric(True)
        ctx.factor()
        assert ctx.last_info() == 0
        R1 = ctx.local_R()
        A = matrix(n, n, 1, 1); A.distribute_symmetric(0, 0, 1, 1, 0, True)
        pack = cholinv.info(-1, 1, -3, 'U'); cholinv.factor(A, pack, None)
        R2 = cholinv.construct_R(pack).to_numpy()
        assert np.linalg.norm(R1 - R2) / np.linalg.norm(R2) < 1e-14
        ctx.close()
    # CholeskyQR2 with the Gram all-reduce on RCCL
    class Topo:
        pass
    topo = Topo(); topo.c, topo.d, topo.x, topo.y, topo.z, topo.rank, topo.size, topo.world = 1, 1, 0, 0, 0, 0, 1, comm.handle
    Q = matrix(64, 8192, 1, 1); Q.distribute_random(0, 0, 1, 1, 0)
    qp = cacqr.info(2, cholinv.info(1, 1, 0, 'U'))
    cacqr.factor(Q, qp, topo)
    assert validate.qr.residual(Q, qp, topo) < 1e-13 and validate.qr.orthogonality(Q, qp, topo) < 1e-15
    comm.close()


@pytest.mark.gpu
def test_single_rank_dist_path_matches_single_gpu_plan():
    """P = 1 through the RCCL-less self communicator: same R as the single-GPU plan, at a larger size."""
    import torch
    from capital_amd import cholinv, dist_cholesky as dc
    from capital_amd.matrix import matrix
    n, nb = 4096, 512
    ctx = dc.setup(n, nb)
    ctx.factor()
    assert ctx.last_info() == 0
    R1 = ctx.local_R()
    A = matrix(n, n, 1, 1); A.distribute_symmetric(0, 0, 1, 1, 0, True)
    pack = cholinv.info(-1, 1, -3, 'U'); cholinv.factor(A, pack, None)
    R2 = cholinv.construct_R(pack).to_numpy()
    assert np.linalg.norm(R1 - R2) / np.linalg.norm(R2) < 1e-14
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,m,n", [(2, 4096, 64), (4, 10000, 48), (3, 6000, 128)])
def test_multirank_cacqr_on_one_gpu(nproc, m, n):
    """CholeskyQR2 1D: row-cyclic pieces on several ranks, Gram all-reduce through the (host-staged) communicator."""
    r = _case(nproc, "cacqr", m, n)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "CACQR-OK" in r.stdout, r.stdout[-2000:]


def _bench_self_launched(nproc, extra, timeout=900):
    """`python bench.py --gpus N ...` WITHOUT a launcher: bench.py starts its own N ranks (torch.distributed.run, free port) and relays
    rank 0's JSON line - the form the driver uses.  CAPITAL_BENCH_EMULATE=1: all ranks on cuda:0, gloo + host-staged collectives."""
    import json
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "1", "--warmup", "1", "--full"] + list(extra)
    env = dict(os.environ, CAPITAL_BENCH_EMULATE="1", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_multi_gpu_self_launch_emulated():
    """bench.py --gpus 2 end to end with no torchrun around it (rank bootstrap, timing reduce, JSON) - the numbers are meaningless
    on a shared GPU, the contract fields are checked: both ranks seen by the communicator, the mode ladder, the roofline of rank 0's
    share of the trailing update, the CPU comparator (the REAL reference, bounded)."""
    d = _bench_self_launched(2, ("--size", "4096", "--cpu-n", "1024", "--cpu-budget-s", "40"))
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["unit"] == "TFLOP/s" and d["value"] > 0
    assert d["config"]["info"] == 0 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["config"]["n_ranks_seen"] == 2 and set(d["config"]["modes"]) == {"safe", "overlap", "ipc"}
    assert d["roofline"]["bound"] == "mfma" and d["roofline"]["launches"] > 0 and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["cores"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,extra,key", [
    (4, ("--size", "4096", "--nb", "256", "--grid-rows", "2", "--no-cpu-baseline"), "2x2"),             # the Pr x Pc plan through bench.py
    (2, ("--size", "2048", "--nb", "256", "--workload", "mixed", "--cpu-n", "1024", "--cpu-budget-s", "40"), "mixed"),   # config 5's method on P ranks
    (2, ("--size", "4096", "--nb", "256", "--dist-mode", "auto", "--exchange", "rccl", "--no-cpu-baseline"), "auto"),   # safe, overlap and ipc modes in turn
    (4, ("--size", "4096", "--nb", "256", "--no-cpu-baseline"), "layouts"),                             # default --grid-rows auto: 1 x 4 modes, then 2 x 2
    (2, ("--workload", "cacqr", "--qr-rows", "8192", "--qr-cols", "64"), "cacqr"),                      # CholeskyQR2 under the polled watchdog
])
def test_bench_multi_gpu_variants_emulated(nproc, extra, key):
    d = _bench_self_launched(nproc, extra)
    assert d["n_gpus"] == nproc and d["value"] > 0 and d["config"]["info"] == 0
    if key == "layouts":
        assert set(d["config"]["modes"]) == {"safe", "overlap", "ipc", "2x2"}, d["config"]["modes"]
        assert all(m["info"] == 0 and m["probe_residual"] <= 1e-13 for m in d["config"]["modes"].values())
        assert d["config"]["mode"] in d["config"]["modes"] and d["config"]["fallback"] is False
    if key == "cacqr":
        assert d["scaling"] == "weak" and d["config"]["residual"] <= 1e-13
        assert d["roofline"]["frac"] > 0 and d["cpu_baseline"]["value"] > 0
    if key == "2x2":
        assert d["config"]["grid"] == "2x2" and d["config"]["n_ranks_seen"] == 4 and d["config"]["launches_per_factor_rank0"]["collectives"] > 0
    if key == "auto":
        assert set(d["config"]["modes"]) == {"safe", "overlap", "ipc"} and d["config"]["modes"]["ipc"]["ipc_active"] == 1
        assert d["config"]["fallback"] is False and d["config"]["mode"] in ("safe", "overlap", "ipc")
    if key == "mixed":
        assert d["config"]["residual"] <= 1e-14 and d["config"]["independent_residual"] <= 1e-13
        assert "roofline" in d and d["cpu_baseline"]["value"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,c,M,N,K,chunks", [(4, 1, 512, 384, 640, 0), (4, 1, 300, 200, 250, 3), (8, 2, 512, 512, 512, 2), (8, 2, 300, 210, 250, 3),
                                                   (1, 1, 256, 256, 256, 2), (9, 1, 300, 300, 300, 2)])
def test_summa_gemm_on_process_grids(nproc, c, M, N, K, chunks):
    """matmult::summa GEMM on d x d x c grids sharing one GPU (host-staged row / column / depth communicators): 2 x 2 x 1
    (2D SUMMA, 2 steps), 2 x 2 x 2 (the reference's own 3D cube, one step per layer + depth all-reduce), 3 x 3 x 1, ragged
    cyclic pieces, chunked B broadcasts overlapped with the local GEMMs."""
    r = _case(nproc, "summa", M, N, ("--c", c, "--k", K, "--chunks", chunks))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "SUMMA-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,c,m,n", [(8, 2, 4096, 64), (4, 1, 3000, 48), (16, 2, 6000, 96), (8, 2, 1001, 32), (8, 2, 256, 16),
                                         (8, 1, 256, 16)])
def test_cacqr_3d_and_tunable_grid(nproc, c, m, n):
    """CholeskyQR2 on c x d x c grids: 2 x 2 x 2 (sweep_3d), 1 x 4 x 1 (degenerates to 1D), 2 x 4 x 2 (sweep_tune), ragged rows;
    256 x 16 on 2 x 2 x 2 and 1 x 8 x 1 are also compared with the real reference's 8-rank dumps (tests/golden/cacqr2_p8_*)."""
    r = _case(nproc, "cacqr3d", m, n, ("--c", c))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "CACQR3D-OK" in r.stdout, r.stdout[-2000:]
    if m == 256:
        assert "golden=ok" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,c,pr,n,nb", [
    (8, 2, 1, 1024, 128),        # the reference's 2 x 2 x 2 grid -> 1 x 8 block columns
    (8, 2, 2, 1024, 128),        # ... -> 2 x 4 block-cyclic (cap_dist2d_*)
    (4, 1, 1, 1000, 128),        # 2 x 2 x 1, ragged n (padded pieces, partial last block)
    (4, 1, 2, 777, 256),         # -> 2 x 2, odd n
    (9, 1, 3, 1100, 128),        # 3 x 3 x 1 -> 3 x 3
    (8, 2, 1, 250, 128),         # fewer blocks than ranks: most ranks hold nothing on the block-cyclic side
    (1, 1, 1, 512, 128),
])
def test_distributed_redistribution_cyclic_block_cyclic(nproc, c, pr, n, nb):
    """Element-cyclic d x d x c pieces <-> Pr x Pc block-cyclic pieces by ONE all-to-all (csrc/redist.hip): both directions
    bit-exact against NumPy index arithmetic; the replicas share the supply (destination t reads layer t mod c)."""
    r = _case(nproc, "redist", n, nb, ("--c", c, "--pr", pr))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "REDIST-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,pr", [("cyclic", 1), ("cyclic2d", 2)])
@pytest.mark.parametrize("name", ["cholinv_p8_n128_ci1_s1_bc-2.npz", "cholinv_p8_n192_ci0_s1_bc-3.npz", "cholinv_p8_n250_ci1_s1_bc-2.npz"])
def test_reference_layout_end_to_end_against_the_8rank_piece_dumps(mode, pr, name):
    """A caller holding the reference's element-cyclic pieces on 8 ranks (2 x 2 x 2): factor, construct_R, construct_Rinv speak
    that layout end to end (1 x 8 behind cholinv::factor; 2 x 4 through redistribute + cap_dist2d) - every rank's piece is
    compared with the piece the REAL reference left on the same rank."""
    r = _case(8, mode, 128, 128, ("--golden", name, "--pr", pr))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "CYCLIC-OK" in r.stdout and "golden=ok" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cholinv_grid8_n256_ci0_s1_bc0.npz", "cholinv_grid8_n251_ci0_s1_bc-2.npz"])
def test_reference_layout_follows_the_grids_base_case_rule_and_root_partition(name):
    """Upstream's base-case dimension starts at c d (cholinv.hpp:15-18) and its root partition is taken on the LOCAL dimension (:107):
    with complete_inv = 0 and bc_mult_dim = 0 the 2 x 2 x 2 grid leaves Rinv[0:128, 128:256] empty where one process would invert the
    whole base case, and n = 251 is cut at 126, not 125.  Every rank's pieces against the REAL reference's (round 5: found on the CPU by
    tests/hipshim/run_compute.py, which runs these two dumps as well)."""
    r = _case(8, "cyclic", 128, 128, ("--golden", name, "--pr", 1))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "CYCLIC-OK" in r.stdout and "golden=ok" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,c,mode,pr,n,nb,ci", [
    (8, 2, "cyclic", 1, 2048, 128, 1), (8, 2, "cyclic", 1, 2048, 256, 0), (4, 1, "cyclic", 1, 1000, 128, 1),
    (8, 2, "cyclic2d", 2, 2048, 128, -1), (4, 1, "cyclic2d", 2, 1000, 128, -1), (8, 2, "cyclic", 1, 4096, 512, -1),
])
def test_reference_layout_end_to_end_against_the_oracle(nproc, c, mode, pr, n, nb, ci):
    r = _case(nproc, mode, n, nb, ("--c", c, "--pr", pr, "--ci", ci))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "CYCLIC-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,c,M,N,K,chunks", [(4, 1, 384, 256, 200, 0), (8, 2, 512, 384, 0, 2), (9, 1, 300, 210, 150, 0), (4, 1, 301, 203, 97, 3),
                                                   (1, 1, 256, 128, 64, 0)])
def test_summa_trmm_and_syrk_overloads_on_process_grids(nproc, c, M, N, K, chunks):
    """matmult::summa's TRMM (Left / Right x NoTrans / Trans, rect and packed-upper T) and SYRK (Trans / NoTrans, beta, rect and
    packed C) overloads on d x d x c grids sharing one GPU, util::transpose partner exchange included - against the oracle."""
    r = _case(nproc, "summa_tri", M, N, ("--c", c, "--k", K, "--chunks", chunks))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "SUMMATRI-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cholinv_p8_n128_ci1_s1_bc-2.npz", "cholinv_p8_n192_ci0_s1_bc-3.npz", "cholinv_p8_n250_ci1_s1_bc-2.npz"])
def test_reference_recursion_composed_from_the_distributed_operators(name):
    """One level of cholinv's recursion (CI::trsm, CI::tmu, the inverse completion - cholinv.hpp:107-159) composed from
    util::transpose + the distributed TRMM / SYRK on the pieces the REAL reference left on its 8 ranks: R12, the Schur
    complement and Rinv12 come out as the reference's own pieces."""
    r = _case(8, "summa_tri", 128, 128, ("--golden", name))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "SUMMATRI-OK" in r.stdout and "golden=ok" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,pr,n,nb,ci", [
    (4, 2, 2048, 128, -1),       # 2 x 2: the round-trip the drop-in boundary promises (host matrix -> pieces -> factor -> host R)
    (4, 2, 1000, 128, 1),        # ragged n, R^-1 too
    (8, 2, 2049, 256, 0),        # 2 x 4
    (4, 1, 2048, 128, 1),        # 1 x 4 behind cap_cholinv_factor_desc (block columns)
    (3, 1, 1000, 128, -1),
    (1, 1, 1024, 128, 1),
    (8, 2, 250, 128, -1),        # fewer blocks than processes: empty pieces
])
def test_block_cyclic_descriptor_host_round_trip(nproc, pr, n, nb, ci):
    """cap_desc_create_bc + cap_desc_import_host_global / export_host_global + the *_desc entry points: a caller with a host matrix
    reaches the layout the multi-GPU plans run on and gets R / R^-1 back, against the oracle."""
    r = _case(nproc, "desc", n, nb, ("--pr", pr, "--ci", ci))
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "DESC-OK" in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,n,reps", [(4, 2048, 20), (8, 1024, 10)])
def test_one_launch_chain_under_process_time_slicing(nproc, n, reps):
    """The one-launch diagonal-block chain with 4 / 8 processes sharing the GPU, each next to its own saturating stream: bit-identical to the
    launch-per-step chain in every process, every repetition checked (the memory-ordering side of the meeting protocol has
    no CPU model - this is its stress test; release / acquire fences are on by default since round 5)."""
    r = _case(nproc, "chainstress", n, reps)
    assert r.returncode == 0, (r.stdout[-3000:] + r.stderr[-3000:])
    assert "CHAINSTRESS-OK" in r.stdout, r.stdout[-2000:]


# case of every batched test, from its parameters (read by tests/conftest.py at collection time)
test_multirank_schedule_on_one_gpu._dist_case = lambda nproc, n, nb: (nproc, "gpu", n, nb, ())
test_multirank_schedule_variants._dist_case = lambda nproc, n, nb, extra: (nproc, "gpu", n, nb, tuple(extra))
test_multirank_schedule_under_random_stream_delays._dist_case = lambda nproc, n, nb, jitter: (nproc, "gpu", n, nb, ("--jitter", jitter))
test_distributed_inverse_matches_oracle._dist_case = lambda nproc, n, nb, extra: (nproc, "gpu", n, nb, tuple(extra))
test_distributed_factors_match_the_8rank_reference_dumps._dist_case = lambda name: (8, "gpu", 128, 128, ("--golden", name))
test_2d_block_cyclic_schedule_options._dist_case = lambda nproc, pr, n, nb, extra: (nproc, "gpu2d", n, nb, ("--pr", pr) + tuple(extra))
test_distributed_mixed_precision_solve._dist_case = lambda nproc, n, nb, hard: (nproc, "mixed", n, nb, ("--hard", hard))
test_multirank_cacqr_on_one_gpu._dist_case = lambda nproc, m, n: (nproc, "cacqr", m, n, ())
test_summa_gemm_on_process_grids._dist_case = lambda nproc, c, M, N, K, chunks: (nproc, "summa", M, N, ("--c", c, "--k", K, "--chunks", chunks))
test_cacqr_3d_and_tunable_grid._dist_case = lambda nproc, c, m, n: (nproc, "cacqr3d", m, n, ("--c", c))
test_distributed_redistribution_cyclic_block_cyclic._dist_case = lambda nproc, c, pr, n, nb: (nproc, "redist", n, nb, ("--c", c, "--pr", pr))
test_reference_layout_end_to_end_against_the_8rank_piece_dumps._dist_case = lambda mode, pr, name: (8, mode, 128, 128, ("--golden", name, "--pr", pr))
test_reference_layout_follows_the_grids_base_case_rule_and_root_partition._dist_case = lambda name: (8, "cyclic", 128, 128, ("--golden", name, "--pr", 1))
test_reference_layout_end_to_end_against_the_oracle._dist_case = lambda nproc, c, mode, pr, n, nb, ci: (nproc, mode, n, nb, ("--c", c, "--pr", pr, "--ci", ci))
test_summa_trmm_and_syrk_overloads_on_process_grids._dist_case = lambda nproc, c, M, N, K, chunks: (nproc, "summa_tri", M, N, ("--c", c, "--k", K, "--chunks", chunks))
test_reference_recursion_composed_from_the_distributed_operators._dist_case = lambda name: (8, "summa_tri", 128, 128, ("--golden", name))
test_2d_block_cyclic_schedule_on_one_gpu._dist_case = lambda nproc, pr, n, nb: (nproc, "gpu2d", n, nb, ("--pr", pr) + (("--expect-fail", "cap_dist2d_plan_create") if nproc // pr % pr else ()))
test_block_cyclic_descriptor_host_round_trip._dist_case = lambda nproc, pr, n, nb, ci: (nproc, "desc", n, nb, ("--pr", pr, "--ci", ci))
test_one_launch_chain_under_process_time_slicing._dist_case = lambda nproc, n, reps: (nproc, "chainstress", n, reps, ())
