"""Worker of tests/test_structure_factor.py::test_ranks_agree_with_one_rank: one rank of a multi-process run on the shared device.

    python sk_worker.py <rank> <world> <port> <px> <py> <pz> <k_max> <json stride> <json list of CLI flags>

Every rank drives the HIP path on device 0 with the gloo transport (as tests/rdf_worker.py does) and prints the global amplitudes
Simulation.structure_factor() returns at step 0, as hexadecimal floats: the ranks must agree to the bit.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    grid = [int(v) for v in sys.argv[4:7]]
    k_max, stride = int(sys.argv[7]), json.loads(sys.argv[8])
    args = json.loads(sys.argv[9]) + ["-i", grid[0], "-j", grid[1], "-k", grid[2]]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    pkg.setup_gpu(0, rank)
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    sim = pkg.Simulation(args)
    got = sim.structure_factor(k_max, tuple(stride) if isinstance(stride, list) else stride)
    print("SK", json.dumps([[v.hex() for v in got["rho"].real.tolist()], [v.hex() for v in got["rho"].imag.tolist()], sim.bragg_order().hex()]))
    sys.stdout.flush()
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
