"""Worker of tests/test_deform_coupling.py: one run in a process of its own (as tests/density_worker.py), or one rank of a multi-process run over the
gloo transport (as tests/deform_worker.py and tests/msd_worker.py).

    python deform_coupling_worker.py single <json list of CLI flags> <json job> <out.npz>
    python deform_coupling_worker.py ranks  <json list of CLI flags> <json job> <out.npz> <rank> <world> <port> <px> <py> <pz>

"single": COMD_HALO_MIRROR and COMD_NL_DEFERRED are read once per process, so the test starts one child per value and sets it in the child's environment.
The job: {"rates": [x, y, z] in 1/ps, "steps": n, "track": bool, "analyses": bool, "bins": n, "r_coord": A}.  The child sets the strain rate, tracks the
displacements if asked, runs the steps on device 0 and writes to out.npz: r, p, f, e of its local atoms by gid (zeros for the other ranks' atoms), the
energies, the box, the list builds, which atoms it owned before and after the steps, and -- as every rank receives them -- the GLOBAL displacements() and
msd(), pair_histogram(bins) counts, centro_symmetry(r_coord) and common_neighbor_analysis().
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def run(pkg, args, job, out):
    with pkg.Simulation(args) as sim:
        got = {"own0": np.abs(sim.gather(1)).sum(axis=1) > 0}          # momenta of a hot state: no owned atom has p = 0
        sim.set_strain_rate(job["rates"])
        if job.get("track"):
            sim.track_displacement()
        sim.step(job["steps"])
        sim.sum_atoms()
        got.update(r=sim.gather(0), p=sim.gather(1), f=sim.gather(2), e=sim.gather(3), energy=np.array(sim.energy()), box=sim.box,
                   builds=sim.nl_builds, step=sim.step_count)
        got["own1"] = np.abs(got["p"]).sum(axis=1) > 0
        if job.get("track"):
            total, parts = sim.msd()
            got.update(d=sim.displacements(), msd=np.array([total, *parts]))
        if job.get("analyses"):
            edges, counts = sim.pair_histogram(job["bins"])
            csp, coord = sim.centro_symmetry(job["r_coord"])
            got.update(edges=edges, counts=counts, csp=csp, coord=coord, cna=sim.common_neighbor_analysis())
        np.savez(out, **got)
    print("COUPLING saved")
    sys.stdout.flush()


def main():
    mode, args, job, out = sys.argv[1], json.loads(sys.argv[2]), json.loads(sys.argv[3]), sys.argv[4]
    if mode == "single":
        pkg = ge.load_package()
        pkg.setup_gpu(0, 0)
        pkg.init_parallel(0, 1, None)
        run(pkg, args, job, out)
        return
    rank, world, port = int(sys.argv[5]), int(sys.argv[6]), sys.argv[7]
    grid = [int(v) for v in sys.argv[8:11]]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    pkg.setup_gpu(0, rank)
    transport = pkg.GlooTransport(dist)
    pkg.init_parallel(rank, world, transport.struct)
    run(pkg, args + ["-i", grid[0], "-j", grid[1], "-k", grid[2]], job, out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
