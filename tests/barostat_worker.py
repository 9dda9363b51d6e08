"""Worker of tests/test_barostat.py: one rank of a multi-process host-only run over the gloo transport (as tests/deform_worker.py).

    python barostat_worker.py <rank> <world> <port> <px> <py> <pz> <json list of CLI flags>

Prints this rank's grid, its coordinates in the process grid and the rows of periodic_face_pairs() with the cell ids resolved to grid tuples.  No device is touched.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def tuples(sim):
    """{cell id: (ix, iy, iz)} of every local and halo cell"""
    g = sim.grid
    return {sim.lib.comdSimBoxFromTuple(sim.ptr, ix, iy, iz): (ix, iy, iz)
            for ix in range(-1, g[0] + 1) for iy in range(-1, g[1] + 1) for iz in range(-1, g[2] + 1)}


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    grid = [int(v) for v in sys.argv[4:7]]
    args = json.loads(sys.argv[7]) + ["-i", grid[0], "-j", grid[1], "-k", grid[2]]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    sim = pkg.Simulation(args, host_only=True)
    t = tuples(sim)
    rows = [[list(t[int(r[0])]), list(t[int(r[1])]), int(r[2]), int(r[3]), int(r[4])] for r in sim.periodic_face_pairs()]
    print("FACEPAIRS", json.dumps({"grid": list(sim.grid), "rank": rank, "rows": rows}))
    sys.stdout.flush()
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
