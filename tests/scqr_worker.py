"""Worker of tests/test_gpu_scqr.py::test_two_ranks_unequal_rows: one rank of a shifted CholeskyQR factorization whose ranks share cuda:0
through the host-staged communicator (tests/host_staged.py) and hold UNEQUAL row counts.  Started as a plain child process with the
environment torch.distributed.run would give it (RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT); writes <dir>/rank<r>.npz (R, Q, info, shift)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="holds a.npy (the stacked matrix); the results go here")
    ap.add_argument("--rows", required=True, help="comma-separated row counts of the ranks (contiguous row blocks of a.npy)")
    ap.add_argument("--num-iter", type=int, default=3)
    args = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    from capital_amd import cacqr, cholinv
    from capital_amd.matrix import matrix
    from tests.host_staged import HostStagedComm
    rows = [int(x) for x in args.rows.split(",")]
    assert len(rows) == size
    lo = sum(rows[:rank])
    a = np.ascontiguousarray(np.load(os.path.join(args.dir, "a.npy"))[lo:lo + rows[rank]])
    comm = HostStagedComm()

    class Topo:                      # the fields cacqr reads from topo::rect
        pass
    topo = Topo(); topo.c, topo.d, topo.x, topo.y, topo.z = 1, size, 0, rank, 0
    topo.rank, topo.size, topo.world = rank, size, comm.handle
    A = matrix(a.shape[1], a.shape[0], 1, 1)
    A.from_numpy(a)
    pack = cacqr.info(args.num_iter, cholinv.info(1, 1, 0, 'U'))
    for rep in range(2):             # plan reuse: the row count is summed over the ranks by the first call only
        cacqr.factor(A, pack, topo)
    before = comm.calls["allreduce"]
    cacqr.factor(A, pack, topo)
    assert comm.calls["allreduce"] - before == args.num_iter, "one Gram all-reduce per sweep and nothing else after the first call"
    info = pack.last_info()
    # (construct_Q without the topo: this rank's rows are a block of its own size, not a cyclic piece of a global row count)
    np.savez(os.path.join(args.dir, "rank%d.npz" % rank), R=cacqr.construct_R(pack).to_numpy(), Q=cacqr.construct_Q(pack).to_numpy(),
             info=info, shift=pack.shift())
    dist.barrier()
    pack._release(); comm.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
