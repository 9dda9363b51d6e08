"""Worker of tests/test_density_regimes.py (test_mirrored_halo_is_the_message_halo_bit_for_bit, and the one run the launch wrapper must refuse, which ends the
process): one run in a process of its own.

    python density_worker.py <json list of CLI flags> <steps> <out.npz>

COMD_HALO_MIRROR is read once per process (halo_exchange.c), so the test starts one child per value and sets it in the child's environment.  The
child runs the steps on device 0 and writes to out.npz every slot array of every cell, local and halo, as Simulation.cells() returns them, and the
energies; the parent compares the occupied slots.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    args, steps, out = json.loads(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    pkg = ge.load_package()
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    with pkg.Simulation(args) as sim:
        sim.step(steps)
        cells = sim.cells()
        ep, ek, n = sim.energy()
        np.savez(out, energy=np.array([ep, ek]), n_global=n, n_local_boxes=sim.n_local_boxes, **cells)


if __name__ == "__main__":
    main()
