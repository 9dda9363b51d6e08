"""Worker of tests/test_heat_flux.py::test_ranks_give_the_one_rank_array: one rank of a multi-process run on the shared device.

    python heatflux_worker.py <rank> <world> <port> <px> <py> <pz> <output directory> <json list of CLI flags>

Every rank drives the HIP path on device 0 with the gloo transport (as tests/stress_worker.py does), scatters the momenta of
test_heat_flux._new_momenta -- its local slots only: the halo slots keep the momenta of the initial state, and no exchange follows -- and saves the global
array Simulation.atomic_heat_flux() returns and the twelve numbers of heat_flux() as <output directory>/heatflux_rank<rank>.npz.
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
    sim.scatter(1, np.random.default_rng(77).normal(size=(sim.n_global, 3)) * (0.003 * sim.mass))      # test_heat_flux._new_momenta
    sums = sim.heat_flux()
    np.savez(os.path.join(out_dir, f"heatflux_rank{rank}.npz"), j=sim.atomic_heat_flux(),
             sums=np.concatenate([sums[k] for k in ("kinetic", "potential", "virial", "total")]))
    print("HEATFLUX saved")
    sys.stdout.flush()
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
