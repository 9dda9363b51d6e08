"""Worker of tests/test_born_elastic.py::test_two_ranks_give_the_one_rank_matrix: one rank of a multi-process run on the shared device.

    python born_worker.py <rank> <world> <port> <px> <py> <pz> <output directory> <json list of CLI flags>

Every rank drives the HIP path on device 0 with the gloo transport (as tests/stress_worker.py does) and saves the matrix Simulation.born_matrix()
returns at step 0 as <output directory>/born_rank<rank>.npy.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    import numpy as np
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    grid = [int(v) for v in sys.argv[4:7]]
    out_dir = sys.argv[7]
    args = json.loads(sys.argv[8]) + ["-i", grid[0], "-j", grid[1], "-k", grid[2]]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    pkg.setup_gpu(0, rank)
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    sim = pkg.Simulation(args)
    np.save(os.path.join(out_dir, f"born_rank{rank}.npy"), sim.born_matrix())
    print("BORN saved")
    sys.stdout.flush()
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
