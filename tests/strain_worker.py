"""Worker of tests/test_atomic_strain.py::test_ranks_give_the_one_rank_arrays: one rank of a multi-process run on the shared device.

    python strain_worker.py <rank> <world> <port> <px> <py> <pz> <output directory> <steps> <json list of CLI flags>

Every rank drives the HIP path on device 0 with the gloo transport (as tests/stress_worker.py does): it takes the strain reference on the ranks, runs
<steps> steps so that atoms migrate and pairs straddle ranks, and saves the global arrays Simulation.atomic_strain() returns as
<output directory>/strain_rank<rank>.npz and the summary as strain_rank<rank>.json.
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
    out_dir, steps = sys.argv[7], int(sys.argv[8])
    args = json.loads(sys.argv[9]) + ["-i", grid[0], "-j", grid[1], "-k", grid[2]]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    pkg.setup_gpu(0, rank)
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    sim = pkg.Simulation(args)
    sim.set_strain_reference()
    sim.step(steps)
    e, d2, n = sim.atomic_strain()
    np.savez(os.path.join(out_dir, f"strain_rank{rank}.npz"), e=e, d2=d2, n=n, box0=sim.strain_reference_box)
    with open(os.path.join(out_dir, f"strain_rank{rank}.json"), "w") as f:
        json.dump(sim.strain_summary(), f)
    print("STRAIN saved")
    sys.stdout.flush()
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
