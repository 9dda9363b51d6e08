"""Worker of tests/test_msd.py::test_two_ranks_give_the_one_rank_displacements: one rank of a multi-process run on the shared device.

    python msd_worker.py <rank> <world> <port> <px> <py> <pz> <json list of CLI flags> <steps> <out.npz>

Every rank drives the HIP path on device 0 with the gloo transport (as tests/langevin_worker.py does), tracks displacements over the steps and
writes to out.npz: its local atoms' positions by gid (zeros for the other ranks' atoms), which atoms it owned at the start and at the end,
the GLOBAL displacements() and msd() as this rank received them.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    grid = [int(v) for v in sys.argv[4:7]]
    args = json.loads(sys.argv[7]) + ["-i", grid[0], "-j", grid[1], "-k", grid[2]]
    steps = int(sys.argv[8])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    pkg.setup_gpu(0, rank)
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    sim = pkg.Simulation(args)
    own0 = np.abs(sim.gather(1)).sum(axis=1) > 0          # momenta at 150000 K: no owned atom has p = 0
    sim.track_displacement()
    sim.step(steps)
    own1 = np.abs(sim.gather(1)).sum(axis=1) > 0
    total, parts = sim.msd()
    np.savez(sys.argv[9], r=sim.gather(0), own0=own0, own1=own1, d=sim.displacements(), msd=np.array([total, *parts]))
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
