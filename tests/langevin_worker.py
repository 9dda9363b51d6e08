"""Worker of tests/test_langevin.py::test_ranks_give_the_one_rank_trajectory: one rank of a multi-process Langevin run on the shared device.

    python langevin_worker.py <rank> <world> <port> <px> <py> <pz> <json list of CLI flags> <json [temperature, damp_fs, seed, steps]> <out.npz>

Every rank drives the HIP path on device 0 with the gloo transport (as tests/multirank_worker.py does), runs the thermostatted steps and
writes its local atoms' positions and momenta by gid (zeros for the other ranks' atoms) to out.npz: a file, because arrays this size would
fill the stdout pipe of a rank the parent is not reading yet while the other rank waits for it at the closing barrier.
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
    temperature, damp, seed, steps = json.loads(sys.argv[8])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    pkg.setup_gpu(0, rank)
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    sim = pkg.Simulation(args)
    sim.set_langevin(temperature, damp, seed)
    sim.step(steps)
    np.savez(sys.argv[9], step=sim.step_count, r=sim.gather(0), p=sim.gather(1))
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
