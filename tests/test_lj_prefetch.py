"""The vector-side L2 prefetch of LJ thread_atom's list loop (lj_kernels.h ljListLoop, LJ_PREFETCH_D) -- run with `-m gpu` on an MI355X.

The prefetch only asks for memory early: the lanes load list entries ahead of the scalar stream and touch the records they name.  It may not change a bit of
the result, and it may not read past a row's last entry (the tail of a row is uninitialised).  COMD_LJ_PREFETCH=0 launches the kernel without it; which kernel
ran is read from Simulation.force_leg_report(), never from the variable the test set.

The file runs in whichever precision the process is bound to (COMD_PRECISION); test_lj_prefetch_single_build runs it once more in the float build.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_kernel_legs as legs
from test_kernel_legs import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX, DELTA = (12, 10, 11), 0.15
LIST_CAP_MIXED = 2200          # rows of 2200 entries: the longer lists do not fit and their waves walk the stencil, inside the same launch


def _args(n):
    return ["-x", n[0], "-y", n[1], "-z", n[2], "-r", DELTA, "-m", "thread_atom"]


_RUNS = {}


def _run(gpu, monkeypatch, n, prefetch, cap):
    """Forces, per-atom energies (of the last step's energy evaluation) and the leg report after 3 steps; one run per configuration, shared and read-only."""
    key = (n, prefetch, cap)
    if key not in _RUNS:
        monkeypatch.setenv("COMD_LJ_PREFETCH", "1" if prefetch else "0")
        if cap:
            monkeypatch.setenv("COMD_LJ_LIST_CAP", str(cap))
        else:
            monkeypatch.delenv("COMD_LJ_LIST_CAP", raising=False)
        with gpu.Simulation(_args(n)) as sim:
            sim.step(3)
            f, u, rep = sim.gather(2).copy(), sim.gather(3).copy(), sim.force_leg_report()
        f.setflags(write=False)
        u.setflags(write=False)
        print(n, "prefetch", prefetch, "cap", cap, rep)
        _RUNS[key] = (f, u, rep)
    return _RUNS[key]


def _same_bits(gpu, monkeypatch, n, cap):
    f0, u0, rep0 = _run(gpu, monkeypatch, n, False, cap)
    f1, u1, rep1 = _run(gpu, monkeypatch, n, True, cap)
    assert rep0["lj_lists_active"] and rep1["lj_lists_active"] and not rep0["lj_prefetch"] and rep1["lj_prefetch"], (rep0, rep1)
    assert rep1["lj_prefetch_distance"] >= 64
    assert np.abs(f1).max() > 1.0
    assert np.array_equal(f0, f1) and np.array_equal(u0, u1), (np.abs(f0 - f1).max(), np.abs(u0 - u1).max())
    return rep1


def test_prefetch_changes_no_bit(gpu, monkeypatch):
    """LJ thread_atom, 12 x 10 x 11, -r 0.15, 3 steps: forces and per-atom energies with the prefetch are those without it, to the last bit; every wave reads a list."""
    rep = _same_bits(gpu, monkeypatch, BOX, 0)
    assert rep["lj_waves_listed"] > 0 and rep["lj_waves_walking"] == 0 and rep["lj_full_waves_listed"] > 0, rep


@pytest.mark.parametrize("n", [BOX, (10, 10, 10)], ids=["12x10x11", "10x10x10"])
def test_prefetch_changes_no_bit_at_row_edges(gpu, monkeypatch, n):
    """The same comparison with rows of 2200 entries, which mixes listed and walking waves in one launch; 10^3 has 3 x 3 x 3 cells, fuller than the 4 x 3 x 3 of
    12 x 10 x 11, so its rows are longer.

    What the prefetch indexes is clamped to the row's last entry, so the edges are rows that end inside a period of 64 candidates, and rows whose second
    segment (the candidates outside the own cell) starts off the grid of batches.  Both are asserted from the counts LJ_WaveCandidates left (the leg report), over
    the full waves (more than 32 atoms: the ones that run the list loop): rows whose length is no multiple of 64, and rows whose own-cell part is no multiple of 8.
    The clamp itself is reached in every row: its last two periods ask for entries past its end.
    A row SHORTER than LJ_PREFETCH_D = 64 cannot occur for a full wave, in these boxes or in any other: the wave holds more than 32 atoms of one cell, all of them
    candidates of its own list, and at a density at which a cell holds 33 atoms the 26 cells around it hold ~850 more, most of them within 5 sigma of the wave's
    box.  The shortest full row is asserted to be longer than the distance and printed (1681 entries on 12 x 10 x 11); rows that short would only belong to
    the replicated tail waves, which do not run the list loop.  Likewise the own-cell part of a full row is the whole cell here (126 atoms and more)."""
    rep = _same_bits(gpu, monkeypatch, n, LIST_CAP_MIXED)
    assert rep["lj_list_row_capacity"] == LIST_CAP_MIXED and rep["lj_waves_listed"] > 0 and rep["lj_waves_walking"] > 0, rep
    assert rep["lj_full_waves_listed"] > 0 and rep["lj_full_rows_not_multiple_of_64"] > 0, rep
    assert rep["lj_full_rows_own_part_not_multiple_of_8"] > 0, rep
    assert rep["lj_full_rows_min"] > rep["lj_prefetch_distance"], rep
    assert rep["lj_candidates_max"] <= LIST_CAP_MIXED, rep


def test_prefetching_kernel_matches_the_oracle(gpu, orc, monkeypatch):
    """The default leg against the oracle, as test_lj_wave_candidate_lists_and_their_fallbacks compares its legs (same box, steps and tolerances), and the
    report must say that the prefetching kernel ran, with a list for every wave."""
    monkeypatch.delenv("COMD_LJ_PREFETCH", raising=False)
    monkeypatch.delenv("COMD_LJ_LIST_CAP", raising=False)
    with gpu.Simulation(_args(BOX)) as sim:
        o = orc.Oracle(BOX, eam=0, delta=DELTA, cap=max(sim.max_atoms, 64))
        sim.step(2)
        o.step(2)
        f, fo = sim.gather(2), o.gather(orc.F)
        err_f, err_u = np.abs(f - fo).max() / np.abs(fo).max(), np.abs(sim.gather(3) - o.gather(orc.U)).max()
        o.close()
        print(f"prefetch against the oracle: force {err_f:.3e} (<= {TOL['force_rel_to_max']:.1e}), energy {err_u:.3e} (<= {TOL['per_atom_energy_abs']:.1e})")
        assert err_f <= TOL["force_rel_to_max"] and err_u <= TOL["per_atom_energy_abs"]
        c = legs.observe(sim, {"n": BOX, "flags": []})
        assert c.rep["lj_prefetch"], c.rep
        legs.lj_lists_all(c)


N_TESTS = 4      # the tests above, counting the parametrised one twice


def test_lj_prefetch_single_build():
    """Each test of this file in the float build, in a child process (one precision per process), as tests/test_single_precision.py runs the other files.
    (The child deselects this test, so a run that is itself bound to the float build only repeats the others once.)"""
    env = dict(os.environ, COMD_PRECISION="single")
    for k in ("COMD_LJ_PREFETCH", "COMD_LJ_LIST_CAP"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_lj_prefetch.py", "-k", "not single_build"]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-2000:]
    passed = re.search(r"(\d+) passed", proc.stdout)
    assert passed and int(passed.group(1)) == N_TESTS and "skipped" not in proc.stdout and "failed" not in proc.stdout, proc.stdout[-1500:]
