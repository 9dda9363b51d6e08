"""Worker of tests/test_capacities.py: one run in a process of its own, because a capacity that is exceeded ends the process inside the library (comdCheckStatus:
exit(-1)) and because COMD_HALO_MIRROR, COMD_NL_BANK_ORDER, COMD_NL_GLOBAL and COMD_EAM_NL are read from the environment of the process.

    python capacity_worker.py <json job> <out prefix>

job: {"flags": [CLI flags], "steps": [a, b, ...], "momenta": null | {"gid": g, "p": [px, py, pz]}, "host_only": false}

The child creates the simulation on device 0 (the first force evaluation is part of that), prints "created", then for every entry of "steps" calls step(entry)
(0: no call), writes <out prefix>.<k>.npz and prints "reached <k>".  The parent tells how far the run came from those lines and from the files.  With "momenta"
every momentum is set to 0 except the one given, before the first step.  A file holds the per-atom arrays by gid, the energies, every cell's occupancy and gids
(local and halo), the geometry and what comdForceLegReport says about the Verlet rows.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def _save(sim, path, eam):
    ep, ek, n = sim.energy()
    cells = sim.cells()
    rep = sim.force_leg_report()
    extra = dict(rho=sim.gather(4), df=sim.gather(5)) if eam else {}
    np.savez(path, r=sim.gather(0), p=sim.gather(1), f=sim.gather(2), u=sim.gather(3), energy=np.array([ep, ek]), n_global=n, nAtoms=cells["nAtoms"], gid=cells["gid"],
             rx=cells["rx"], grid=np.array(sim.grid), n_local_boxes=sim.n_local_boxes, n_total_boxes=sim.n_total_boxes, max_atoms=sim.max_atoms,
             nl=np.array([rep["neighbor_list_format"], rep["nl_row_capacity"], rep["nl_longest_row"], sim.nl_builds]), **extra)


def main():
    job, out = json.loads(sys.argv[1]), sys.argv[2]
    pkg = ge.load_package()
    if job.get("host_only"):
        with pkg.Simulation(job["flags"], host_only=True):
            print("created", flush=True)
        return
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    eam = "-e" in job["flags"]
    with pkg.Simulation(job["flags"]) as sim:
        print("created", flush=True)
        if job.get("momenta"):
            p = np.zeros((sim.n_global, 3))
            p[job["momenta"]["gid"]] = job["momenta"]["p"]
            sim.scatter(1, p)
        for k, steps in enumerate(job["steps"]):
            if steps:
                sim.step(steps)
            _save(sim, f"{out}.{k}.npz", eam)
            print(f"reached {k}", flush=True)


if __name__ == "__main__":
    main()
