"""Periodic boxes with only two link cells along an axis: the force, list, redistribution and analysis paths where a stencil holds the same cell twice.

Two cells is the least the host accepts (initLinkCells).  On such an axis the 27-cell stencil of every cell holds its neighbour cell twice -- once as itself and once
as its periodic image with a shift -- every local cell is a boundary cell, the interior list of -a 1 is empty, the two faces' send lists together hold every local
cell, the EAM bricks (1 x 4 x 2 cells, staged block 3 x 6 x 4) are larger than the grid, the brick image takes its "grid too small" sizing, and a Verlet row holds
the same atom's slot through two different images.  Every other test file keeps to grids of three cells and more (the seeded LJ sweep of tests/test_gpu_parity.py
and one CSP case aside).

  1. CPU: the states' figures from the checker; the checker against an all-pairs minimum-image sum (exact here: an axis of two cells is at least two cutoffs long).
  2. CPU: what one ulp does to the checker, and the one tolerance that has to follow it (dF/drho, reference_values.json "tolerances_two_cell_boxes").
  3. CPU: eam_hot's motion (cell changes, wraps through the faces of 2-cell axes), the host's refusals, the host's initial state and halo cell lists.
  4. GPU: every method on every state against the checker; the forced legs of tests/test_kernel_legs.py on the 2-cell state of each family; Verlet rows and
     pairlists over rebuilds; redistribution bit for bit; the analyses and the MSD; several ranks whose two neighbours on an axis are one and the same rank.

The file runs in whichever precision COMD_PRECISION selects; tests/test_single_precision.py runs its GPU tests in the float build and counts them (GPU_CASE_COUNT).
"""
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import test_kernel_legs as legs
from multirank_worker import TRAJ_F, TRAJ_R
from test_capacities import FACE_MARGIN
from test_density_regimes import _distances, _eam_all_pairs, _eam_tables, _face_distance, _lj_all_pairs, _snapshot
from test_gpu_parity import _assert_cells_equal
from test_multirank import _launch
from test_pressure import EPS, SIGMA, _interpolate, _pairs, _rel, _tensor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = json.load(open(os.path.join(HERE, "golden", "reference_values.json")))
SINGLE = os.environ.get("COMD_PRECISION", "double") == "single"
PRECISION = "single" if SINGLE else "double"
REAL = np.float32 if SINGLE else np.float64
TOL = G["tolerances_single" if SINGLE else "tolerances"]
TOL_SPLINE = G["tolerances_single_spline"] if SINGLE else TOL
TOL_STATE = G["tolerances_two_cell_boxes"][PRECISION]
SETFL = ["-t", "setfl", "-p", "Cu01.eam.alloy"]

# grid, atoms and occupancy (lowest, highest) are the checker's own figures at step 0; _reference takes them again from the checker before anything relies on them, and
# with them that the axes named in `two` have exactly two cells.  list_skin: the -S the list methods (thread_atom_nl, cta_cell -L) are run with -- their cells are
# cutoff x (1 + skin) wide, and at the default skin of 0.1 the boxes of 3 (EAM) and 7 (LJ) lattice cells would be one cell wide and refused; None: the default.
# list_grid: the grid of those runs (asserted from the host on the CPU and from the run on the GPU).  LJ: 5 sigma = 11.575 A; EAM: Cu_u6.eam, 4.95 A; setfl: 5.507 A.
State = namedtuple("State", "eam n lat delta temp steps grid two atoms occ pot list_skin list_grid")
STATES = {
    "eam_min":   State(1, (3, 3, 3),  3.615, 0.1,  600.0,  5,   (2, 2, 2), (0, 1, 2), 108,  (13, 14),   "Cu_u6.eam",      0.09,   (2, 2, 2)),   # cells of 5.4225 A
    "eam_cube":  State(1, (4, 4, 4),  3.615, 0.1,  600.0,  5,   (2, 2, 2), (0, 1, 2), 256,  (32, 32),   "Cu_u6.eam",      None,   (2, 2, 2)),   # 7.23 A; the EAM list state
    "eam_mixed": State(1, (3, 5, 8),  3.615, 0.15, 600.0,  5,   (2, 3, 5), (0,),      480,  (13, 24),   "Cu_u6.eam",      0.09,   (2, 3, 5)),   # 5.42, 6.03, 5.78 A
    "eam_tight": State(1, (3, 3, 5),  3.301, 0.1,  600.0,  5,   (2, 2, 3), (0, 1),    180,  (13, 18),   "Cu_u6.eam",      0.0002, (2, 2, 3)),   # 4.9515 A: 0.03 % over the cutoff
    "eam_hot":   State(1, (3, 4, 3),  3.615, 0.3,  3000.0, 360, (2, 2, 2), (0, 1, 2), 144,  (18, 18),   "Cu_u6.eam",      0.09,   (2, 2, 2)),   # atoms change cell and wrap (HOT_RUN)
    "eam_setfl": State(1, (4, 4, 4),  3.615, 0.1,  600.0,  5,   (2, 2, 2), (0, 1, 2), 256,  (32, 32),   "Cu01.eam.alloy", None,   (2, 2, 2)),   # 10000-sample tables behind L2
    "lj_cube":   State(0, (7, 7, 7),  3.615, 0.1,  600.0,  5,   (2, 2, 2), (0, 1, 2), 1372, (171, 172), None,             0.03,   (2, 2, 2)),   # 12.65 A
    "lj_mixed":  State(0, (7, 10, 7), 3.615, 0.15, 600.0,  5,   (2, 3, 2), (0, 2),    1960, (147, 172), None,             0.03,   (2, 3, 2)),   # 12.65, 12.05, 12.65 A
    "lj_list":   State(0, (8, 8, 8),  3.615, 0.1,  600.0,  5,   (2, 2, 2), (0, 1, 2), 2048, (256, 256), None,             None,   (2, 2, 2)),   # the LJ list state at the default skin
    # the compressed box of the rows_48 leg (tests/test_kernel_legs.py "eam_l35"): 44 to 53 neighbours, the fourth shell astride the cutoff
    "eam_l35":   State(1, (3, 3, 3),  3.5,   0.1,  600.0,  3,   (2, 2, 2), (0, 1, 2), 108,  (13, 14),   "Cu_u6.eam",      0.05,   (2, 2, 2)),
}
TABLE = [name for name in STATES if name != "eam_l35"]          # the states every test covers; eam_l35 serves one forced leg
# eam_hot, from the checker, step by step over its 360 steps: atoms that changed cell, atoms that wrapped through a periodic face of a 2-cell axis (a coordinate jumps
# by more than half the box), peak occupancy.  The first atom changes cell at step 320, the first wraps at step 349: 360 is the first multiple of 20 with both.
HOT_RUN = (4, 2, 19)
METHODS = {1: ["thread_atom", "cta_cell", "thread_atom_nl"], 0: ["thread_atom", "cta_cell", "thread_atom_nl", "cta_cell -L", "thread_atom -I"]}
HILBERT = [("eam_cube", "cta_cell"), ("lj_cube", "thread_atom")]          # -H


def _extent(st):
    return np.array(st.n, dtype=np.float64) * st.lat


def _make(orc, st, **kw):
    return orc.Oracle(st.n, eam=st.eam, temperature=st.temp, delta=st.delta, lat=st.lat, **(dict(pot_name=st.pot) if st.eam else {}), **kw)


def _listed(method):
    return "_nl" in method or "-L" in method


def _flags(st, method, overlap=0, extra=()):
    m = method.split()
    out = ["-x", st.n[0], "-y", st.n[1], "-z", st.n[2], "-l", st.lat, "-r", st.delta, "-T", st.temp, "-m", m[0], "-a", overlap] + m[1:]
    if st.eam:
        out += ["-e"] + (SETFL if st.pot != "Cu_u6.eam" else [])
    if _listed(method) and st.list_skin is not None:
        out += ["-S", st.list_skin]
    return out + list(extra)


# ---------------------------------------------------------------- the checker's answer, once per state
_REFERENCE = {}


def _cell_of(cells, n_local):
    return {int(gid): b for b in range(n_local) for gid in cells["gid"][b, :cells["nAtoms"][b]]}


def _reference(orc, name):
    """The checker's run of a state: its figures at step 0 (asserted), the state at step 0 and after the state's steps, the cells after the steps, and what moved
    on the way, a step at a time.  Computed once, read-only."""
    if name in _REFERENCE:
        return _REFERENCE[name]
    st = STATES[name]
    o = _make(orc, st)
    grid, n_local, n_total = o.rank_grid(0)
    occ = o.rank_cells(0)["nAtoms"][:n_local].copy()
    rc = orc.lib().oracle_cutoff(o.ptr)
    s0 = _snapshot(orc, o, st.eam)
    print(f"{name}: grid {grid} atoms {o.n_global} occupancy {occ.min()}-{occ.max()} cutoff {rc!r} cell edges {_extent(st) / np.array(grid)} max|f| {np.abs(s0['f']).max():.3e}")
    assert (tuple(grid), o.n_global, (int(occ.min()), int(occ.max()))) == (st.grid, st.atoms, st.occ), name
    assert min(grid) == 2 and st.two == tuple(a for a in range(3) if grid[a] == 2) and len(st.two) >= 1, name
    assert np.all(_extent(st)[list(st.two)] >= 2.0 * rc)          # the minimum image of the numpy references is exact
    tables = _eam_tables(orc, o) if st.eam else None
    cells = o.rank_cells(0)
    home, r_prev = _cell_of(cells, n_local), s0["r"]
    moves, wraps, peak, closest = 0, 0, int(cells["nAtoms"].max()), np.inf
    for _ in range(st.steps):
        o.step(1)
        cells = o.rank_cells(0)
        here, r = _cell_of(cells, n_local), o.gather(orc.R)
        moves += sum(1 for gid, b in here.items() if home[gid] != b)
        wraps += int((np.abs(r - r_prev)[:, list(st.two)] > 0.5 * _extent(st)[list(st.two)]).any(axis=1).sum())
        peak = max(peak, int(cells["nAtoms"].max()))
        home, r_prev = here, r
    sk = _snapshot(orc, o, st.eam)
    for v in cells.values():
        v.setflags(write=False)
    face = _face_distance(sk["r"], _extent(st), grid)
    print(f"{name}: after {st.steps} steps: {moves} cell changes, {wraps} wraps through faces of 2-cell axes, peak occupancy {peak}, least distance from a cell face {face:.3e} A")
    o.close()
    _REFERENCE[name] = dict(st=st, grid=tuple(grid), n_local=n_local, n_total=n_total, rc=rc, s0=s0, sk=sk, cells=cells, moves=moves, wraps=wraps, peak=peak, face=face,
                            tables=tables)
    return _REFERENCE[name]


# ---------------------------------------------------------------- 1. CPU: the figures, the checker against all pairs
@pytest.mark.parametrize("name", list(STATES))
def test_checker_matches_all_pairs(orc, name):
    """Every figure of the table from the checker (_reference asserts them), then the rule of tests/test_density_regimes.py test_checker_matches_all_pairs: step-0
    forces, per-atom energies and (EAM) rhobar against a sum over all pairs that walks no cells, 1e-12 of max|f|, 1e-12 eV, rhobar below the end of the F table
    (measured: <= 9e-15 of max|f|, <= 7e-15 eV, rhobar <= 7e-17, dF/drho <= 3e-14).  In the float build the float checker is compared with the same double sums at
    tolerances_single, which are 4x the distance of the float checker from the double one."""
    ref = _reference(orc, name)
    st, s0 = ref["st"], ref["s0"]
    one = TOL if SINGLE else {"force_rel_to_max": 1e-12, "per_atom_energy_abs": 1e-12, "eam_density_abs": 1e-12, "energy_per_atom_step0": 1e-12}
    if st.eam:
        x0, inv, v = ref["tables"][2]
        xn = x0 + (len(v) - 3) / inv
        assert max(s0["rho"].max(), ref["sk"]["rho"].max()) < xn, (s0["rho"].max(), ref["sk"]["rho"].max(), xn)
        f, u, rho, df = _eam_all_pairs(s0["r"], _extent(st), ref["rc"], ref["tables"])
        print(f"{name}: max|drho| {np.abs(rho - s0['rho']).max():.3e} (rhobar <= {s0['rho'].max():.4f}, the table ends at {xn:.4f})  max|d dF/drho| {np.abs(df - s0['df']).max():.3e}")
        assert np.abs(rho - s0["rho"]).max() <= one["eam_density_abs"]
    else:
        f, u = _lj_all_pairs(s0["r"], _extent(st), ref["rc"])
    fmax = np.abs(s0["f"]).max()
    err_f, err_u, err_total = float(np.abs(f - s0["f"]).max()), float(np.abs(u - s0["u"]).max()), float(abs(u.sum() - s0["ep"])) / st.atoms
    print(f"{name}: max|df| {err_f:.3e} (max|f| {fmax:.3e})  max|de| {err_u:.3e}  |dU|/N {err_total:.3e}")
    assert err_f <= one["force_rel_to_max"] * fmax and err_u <= one["per_atom_energy_abs"] and err_total <= one["energy_per_atom_step0"]


@pytest.mark.parametrize("name", TABLE)
def test_list_methods_run_on_the_recorded_grid(pkg, name):
    """The host's grid for the plain methods is the checker's, and for the list methods (cells of cutoff x (1 + skin)) the recorded one, with two cells on the same
    axes: from a host-only simulation, no device."""
    st = STATES[name]
    pkg.init_parallel(0, 1, None)
    for method in METHODS[st.eam]:
        with pkg.Simulation(_flags(st, method), host_only=True) as sim:
            assert sim.grid == (st.list_grid if _listed(method) else st.grid), (method, sim.grid)
            assert tuple(a for a in range(3) if sim.grid[a] == 2) == st.two


# ---------------------------------------------------------------- 2. CPU: what one ulp does to the checker
def _dfembed_tol(name):
    return TOL_STATE[name]["eam_dfembed_abs"]


@pytest.mark.parametrize("name", TABLE)
def test_checker_moves_less_than_the_tolerances_when_positions_move_one_ulp(orc, name):
    """The checker as created against the checker after every coordinate moved by one ulp (of real_t) in a seeded random direction, at step 0 and after the state's
    steps: forces, per-atom energies, rhobar and E/N move by less than the tolerance each is held to below (step 0: force_rel_to_max; after the steps: the trajectory
    bound of tests/multirank_worker.py, 100 x that).  dF/drho is held to the state's recorded tolerance, by the rule of tolerances_density_regimes: the project's
    value where 4x the distance found here is below it, else a value within [4x, 8x] of that distance."""
    ref = _reference(orc, name)
    st = ref["st"]
    o = _make(orc, st)
    r = o.gather(orc.R)
    assert np.array_equal(r, ref["s0"]["r"]) and np.array_equal(r.astype(REAL).astype(np.float64), r)
    up = np.random.RandomState(20261019).randint(0, 2, size=r.shape).astype(bool)
    rr = r.astype(REAL)
    o.scatter(orc.R, np.where(up, np.nextafter(rr, REAL(np.inf)), np.nextafter(rr, REAL(-np.inf))).astype(np.float64))
    o.redistribute()
    o.compute_force()
    o.kinetic_energy()
    d0 = _distances(ref["s0"], _snapshot(orc, o, st.eam), st.eam, st.atoms)
    o.step(st.steps)
    dk = _distances(ref["sk"], _snapshot(orc, o, st.eam), st.eam, st.atoms)
    o.close()
    print(f"{name}: step 0 " + "  ".join(f"{k} {v:.2e}" for k, v in d0.items()))
    print(f"{name}: step {st.steps} " + "  ".join(f"{k} {v:.2e}" for k, v in dk.items()))
    assert d0["force_rel_to_max"] < TOL["force_rel_to_max"] and dk["force_rel_to_max"] < TRAJ_F
    for d in (d0, dk):
        assert d["per_atom_energy_abs"] < TOL["per_atom_energy_abs"] and d["energy_per_atom"] < TOL["energy_per_atom_trace"], d
        if st.eam:
            assert d["eam_density_abs"] < TOL["eam_density_abs"], d
    if st.eam:
        dist, recorded = max(d0["eam_dfembed_abs"], dk["eam_dfembed_abs"]), _dfembed_tol(name)
        if 4.0 * dist < TOL["eam_dfembed_abs"]:
            assert recorded == TOL["eam_dfembed_abs"], (dist, recorded)
        else:
            assert 4.0 * dist <= recorded <= 8.0 * dist, (dist, recorded)
    else:
        assert name not in TOL_STATE


def test_recorded_tolerances_name_the_eam_states():
    for precision in ("double", "single"):
        block = G["tolerances_two_cell_boxes"][precision]
        assert set(block) == {name for name in TABLE if STATES[name].eam}
        assert all(set(block[name]) == {"eam_dfembed_abs"} for name in block)
        assert all(block[name]["eam_dfembed_abs"] >= G["tolerances_single" if precision == "single" else "tolerances"]["eam_dfembed_abs"] for name in block)


# ---------------------------------------------------------------- 3. CPU: motion, refusals, host logic
def test_atoms_of_eam_hot_change_cell_and_wrap_through_2_cell_axes(orc, pkg):
    """The condition eam_hot's step count is chosen by: in the checker's run atoms change cell AND atoms wrap through a periodic face of a 2-cell axis (both counted
    step by step, both > 0, the counts recorded in HOT_RUN); every step's peak occupancy fits the capacity the host gives the product's run; and no atom ends within
    FACE_MARGIN of a cell face, so the cells can be compared exactly.  The same holds, with 0 moves, for every other state compared cell by cell."""
    ref = _reference(orc, "eam_hot")
    assert (ref["moves"], ref["wraps"], ref["peak"]) == HOT_RUN and ref["moves"] > 0 and ref["wraps"] > 0
    pkg.init_parallel(0, 1, None)
    for name in TABLE:
        ref = _reference(orc, name)
        with pkg.Simulation(_flags(ref["st"], "thread_atom"), host_only=True) as sim:
            assert ref["peak"] <= sim.max_atoms, (name, ref["peak"], sim.max_atoms)
        assert ref["face"] > FACE_MARGIN, (name, ref["face"])


def _host_child(tmp_path, flags):
    return subprocess.run([sys.executable, os.path.join(HERE, "capacity_worker.py"), json.dumps(dict(flags=flags, steps=[], host_only=True)), str(tmp_path / "refused")],
                          cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_one_list_cell_is_refused(tmp_path):
    """EAM 3 x 3 x 3 with thread_atom_nl: cells of cutoff + skin = 5.445 A, of which 10.845 A hold one.  initLinkCells must refuse it; the same box at -S 0.09 (eam_min's
    list runs) has two and is made."""
    proc = _host_child(tmp_path, ["-e", "-x", 3, "-y", 3, "-z", 3, "-m", "thread_atom_nl"])
    assert proc.returncode != 0 and "fewer than 2 link cells along an axis" in proc.stderr and "created" not in proc.stdout, (proc.returncode, proc.stderr[-800:])
    proc = _host_child(tmp_path, ["-e", "-x", 3, "-y", 3, "-z", 3, "-m", "thread_atom_nl", "-S", 0.09])
    assert proc.returncode == 0 and "created" in proc.stdout, (proc.returncode, proc.stderr[-800:])


def test_a_box_of_fewer_than_two_cutoffs_is_refused(tmp_path):
    """An EAM box with (int)(extent / cutoff) = 1 along x (2 x 4 x 4: 7.23 A against 4.95 A).  It never reaches initLinkCells: sanityChecks, which is the reference's
    (CoMD.c sanityChecks: extent < 2 cutoff per rank), ends the run first, so the sentence is that one's ("Simulation too small", on stdout as in the reference) and the
    exit status is non-zero.  No extent passes that check and still gives one cell: (int)(x / c) >= 2 for every x >= 2 c."""
    proc = _host_child(tmp_path, ["-e", "-x", 2, "-y", 4, "-z", 4])
    assert proc.returncode != 0 and "created" not in proc.stdout, (proc.returncode, proc.stdout[-800:])
    assert "Simulation too small" in proc.stdout or "fewer than 2 link cells along an axis" in proc.stderr, (proc.stdout[-800:], proc.stderr[-800:])


@pytest.mark.parametrize("name", ["eam_min", "lj_cube"])
def test_host_initial_state_and_halo_cell_lists(pkg, orc, name):
    """The host's initial state (sites, gids, cells, momenta) and its halo cell lists against the checker, bit for bit, as tests/test_host_logic.py has them on wider
    grids.  On an axis of two cells the atom lists of its two faces together hold every local cell, each cell in exactly one of them, and the force send lists
    likewise."""
    st = STATES[name]
    pkg.init_parallel(0, 1, None)
    with pkg.Simulation(_flags(st, "thread_atom"), host_only=True) as s:
        o = _make(orc, st, cap=s.max_atoms)
        assert s.grid == o.rank_grid(0)[0] == st.grid
        c, oc, nl = s.cells(), o.rank_cells(0), s.n_local_boxes
        assert np.array_equal(c["nAtoms"][:nl], oc["nAtoms"][:nl])
        for b in range(nl):
            k = c["nAtoms"][b]
            assert np.array_equal(c["gid"][b, :k], oc["gid"][b, :k])
            for key in ("rx", "ry", "rz", "px", "py", "pz"):
                assert np.array_equal(c[key][b, :k], oc[key][b, :k]), key
        lists = {(kind, face): s.face_cells(kind, face) for face in range(6) for kind in range(3)}
        for (kind, face), cells in lists.items():
            assert np.array_equal(cells, o.face_cells(0, kind, face)), (kind, face)
        for axis in st.two:
            for kind in (0, 1):
                minus, plus = (set(int(b) for b in lists[(kind, 2 * axis + side)] if b < nl) for side in (0, 1))
                assert minus | plus == set(range(nl)) and not minus & plus and len(minus) == len(plus) == nl // 2, (axis, kind)
        o.close()


# ---------------------------------------------------------------- 4a. GPU: every method on every state
def _compare(sim, name, ref, snap, force_tol, when, interpolated=False):
    """forces, per-atom energies, (EAM) rhobar and dF/drho, U/N, K/N, E/N and the atom count of `sim` against the checker's state `snap`.  -I: the checker has no
    table-interpolated LJ, so forces and energies are those of the restatement of tests/test_lj_interpolation.py at the positions of the run, which are themselves
    held to the checker's (the trajectories of the two differ by the interpolation error, 1e-4 A after these steps)."""
    st = ref["st"]
    f, u = sim.gather(2), sim.gather(3)
    ep, ek, ng = sim.energy()
    assert ng == st.atoms == sim.n_global
    if interpolated:
        from test_lj_interpolation import lj_table, restated_forces
        d = sim.gather(0) - snap["r"]
        d -= np.rint(d / _extent(st)) * _extent(st)
        fo, uo = restated_forces(sim.gather(0), _extent(st), lj_table(), 5.0 * SIGMA)
        err = {"f": float(np.abs(f - fo).max()), "u": float(np.abs(u - uo).max()), "U/N": abs(ep - uo.sum()) / ng, "r": float(np.abs(d).max())}
        print(f"{name} {when} -I: max|f| {np.abs(fo).max():.3e}  " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
        assert err["f"] <= TOL["force_rel_to_max"] * np.abs(fo).max() and err["u"] <= TOL["per_atom_energy_abs"] and err["U/N"] <= TOL["energy_per_atom_step0"], err
        assert err["r"] <= 1e-3, err
        return
    fmax = np.abs(snap["f"]).max()
    err = {"f": float(np.abs(f - snap["f"]).max()), "u": float(np.abs(u - snap["u"]).max()), "U/N": abs(ep - snap["ep"]) / ng, "K/N": abs(ek - snap["ek"]) / ng,
           "E/N": abs((ep + ek) - (snap["ep"] + snap["ek"])) / ng}
    if st.eam:
        err.update(rho=float(np.abs(sim.gather(4) - snap["rho"]).max()), df=float(np.abs(sim.gather(5) - snap["df"]).max()))
    print(f"{name} {when}: max|f| {fmax:.3e}  " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["f"] <= force_tol * fmax, err
    assert err["u"] <= TOL["per_atom_energy_abs"], err
    assert err["U/N"] <= TOL["energy_per_atom_step0"] and err["K/N"] <= TOL["kinetic_per_atom"] and err["E/N"] <= TOL["energy_per_atom_trace"], err
    if st.eam:
        assert err["rho"] <= TOL["eam_density_abs"] and err["df"] <= _dfembed_tol(name), err


def _overlap_lists(sim, overlap):
    """-a 1 on a grid with a 2-cell axis: from the run, the interior list is empty and the boundary list holds every local cell (all of them touch the halo)"""
    counts = sim.overlap_cell_counts()
    print(counts)
    if overlap:
        assert counts == {"boundary": sim.n_local_boxes, "interior": 0, "boundary_ring1": sim.n_local_boxes}, counts


def _cells_hold_the_checkers_atoms(sim, ref, hilbert=False):
    """every local cell holds exactly the checker's gids in ascending order, halo cells are sorted.  -H numbers the cells differently: the same sets of gids."""
    c, oc, nl = sim.cells(), ref["cells"], ref["n_local"]
    assert (sim.grid, sim.n_local_boxes, sim.n_total_boxes) == (ref["grid"], nl, ref["n_total"])
    assert int(c["nAtoms"][:nl].sum()) == ref["st"].atoms
    for b in range(ref["n_total"]):
        assert np.all(np.diff(c["gid"][b, :c["nAtoms"][b]]) > 0), b
    mine, theirs = ([tuple(int(g) for g in x["gid"][b, :x["nAtoms"][b]]) for b in range(nl)] for x in (c, oc))
    if hilbert:
        mine, theirs = sorted(mine), sorted(theirs)
    else:
        assert np.array_equal(c["nAtoms"], oc["nAtoms"])
    assert mine == theirs


def _method_cases():
    out = []
    for name in TABLE:
        for method in METHODS[STATES[name].eam]:
            for overlap in (0, 1):
                out.append(pytest.param(name, method, overlap, [], id=f"{name}-{method.replace(' -', '_')}-a{overlap}"))
    for name, method in HILBERT:
        out.append(pytest.param(name, method, 0, ["-H"], id=f"{name}-{method}-H"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,method,overlap,extra", _method_cases())
def test_every_method_matches_the_checker(gpu, orc, name, method, overlap, extra):
    """Default capacity.  Step 0: forces to force_rel_to_max of the checker's max|f|; after the state's steps: 100 x that (tests/multirank_worker.py TRAJ_F).  Energies,
    rhobar, U/N, K/N, E/N: the project's tolerances; dF/drho: the state's recorded one.  The grid is the run's own and has two cells on the state's axes; after the
    run the cells hold the checker's atoms (list methods aside, which sort their cells at a list build only); -a 1: the run's interior list is empty."""
    ref = _reference(orc, name)
    st = ref["st"]
    table = "-I" in method
    with gpu.Simulation(_flags(st, method, overlap, extra)) as sim:
        assert sim.grid == (st.list_grid if _listed(method) else st.grid) and tuple(a for a in range(3) if sim.grid[a] == 2) == st.two, sim.grid
        _overlap_lists(sim, overlap)
        _compare(sim, name, ref, ref["s0"], TOL["force_rel_to_max"], "step 0", table)
        sim.step(st.steps)
        sim.sum_atoms()
        _compare(sim, name, ref, ref["sk"], TRAJ_F, f"step {st.steps}", table)
        if not _listed(method) and not table:
            _cells_hold_the_checkers_atoms(sim, ref, hilbert=bool(extra))


# ---------------------------------------------------------------- 4b. GPU: the forced legs on the 2-cell state of each family
# The table of tests/test_kernel_legs.py, leg by leg, on 2-cell boxes: lj -> lj_cube, eam -> eam_cube, eam_l35 -> eam_l35 (3 x 3 x 3 at -l 3.5), setfl -> eam_setfl.  A
# shape-independent fact is asserted as it is there.  Where a fact cannot hold on these boxes the nearest one that can is taken, and said so:
#   * the "mixed" legs (both sides of a condition inside one launch) need unequal blocks, stencils or waves.  eam_cube is perfectly even (32 atoms in every cell), so they
#     run on eam_mixed (2 x 3 x 5 cells of 13 to 24 atoms), and the value that splits the launch is not a recorded number but taken from a first run without it: the
#     middle of the widest gap in the populations that run reports (`derive`).  The fact asserted afterwards is the one of test_kernel_legs.py.
#   * budget_1mb runs on lj_list (8^3, 2048 atoms): lj_cube's lists and packed records take 1.05 MB in double but 0.85 MB in float, inside the budget; lj_list's take
#     1.9 and 1.4 MB (ljForceGpuAsync: cells x waves x row x 4 B + all cells x packed cell x (sizeof(LjPos4) + 16 B)).
#   * brick shapes: 2,2 is the whole y-z face here; 3,5 is larger than the grid; 1,1 (a brick of one cell) is added, as is COMD_NL_BANK_ORDER=1.
Leg = namedtuple("Leg", "name state method flags env steps fact derive")


def _split(values):
    """the middle of the widest gap between the sorted distinct values, rounded down to 8"""
    v = np.unique(np.asarray(values))
    assert len(v) >= 2, v
    k = int(np.argmax(np.diff(v)))
    cut = int((int(v[k]) + int(v[k + 1])) // 2 // 8 * 8)
    cut = max(cut, (int(v[k]) + 7) // 8 * 8)
    assert v[k] <= cut < v[k + 1], (v[k], cut, v[k + 1])
    return cut


def _derive_lj_cap(c):
    cap = _split([c.rep["lj_candidates_min"], c.rep["lj_candidates_max"]])
    return {"COMD_LJ_LIST_CAP": str(cap)}, legs.lj_rows_mixed(cap)


def _derive_image(kernel):
    def derive(c):
        image = _split(c.block_populations())
        return {"COMD_EAM_IMAGE": str(image)}, legs.eam_kernel(kernel, extra=legs.brick_some_streamed(image))
    return derive


def _derive_stencil(c):
    records = _split(c.stencil_sums())
    return {"COMD_EAM_CTA": "cell", "COMD_EAM_STENCIL": str(records)}, legs.eam_kernel("cta_cell_round2", extra=legs.stencil_slice(records, "some"))


A0, A1 = ["-a", 0], ["-a", 1]
K = legs.eam_kernel
LEGS = {
    "lj": [
        Leg("default", "lj_cube", "thread_atom", [], {}, 2, legs.lj_lists_all, None),
        Leg("default_interpolated", "lj_cube", "thread_atom", ["-I"], {}, 2, legs.lj_lists_all, None),
        Leg("prune_0", "lj_cube", "thread_atom", [], {"COMD_LJ_PRUNE": "0"}, 2, legs.lj_lists_inactive, None),
        Leg("budget_1mb", "lj_list", "thread_atom", [], {"COMD_LJ_LIST_BUDGET_MB": "1"}, 2, legs.lj_lists_inactive, None),
        Leg("list_cap_64", "lj_cube", "thread_atom", [], {"COMD_LJ_LIST_CAP": "64"}, 2, legs.lj_rows_too_short, None),
        Leg("list_cap_64_interpolated", "lj_cube", "thread_atom", ["-I"], {"COMD_LJ_LIST_CAP": "64"}, 2, legs.lj_rows_too_short, None),
        Leg("list_cap_mixed", "lj_cube", "thread_atom", [], {}, 2, None, _derive_lj_cap),
        Leg("one_wave", "lj_cube", "thread_atom", [], {"COMD_LJ_WAVES": "1"}, 2, legs.lj_one_wave, None),
        Leg("cta_boxes", "lj_cube", "cta_cell", [], {}, 2, legs.lj_cta_form("boxes"), None),
        Leg("cta_slabs", "lj_cube", "cta_cell", [], {"COMD_LJ_CTA_SLABS": "1"}, 2, legs.lj_cta_form("slabs"), None),
    ],
    "eam_cta": [
        Leg("default", "eam_cube", "cta_cell", [], {}, 3, K("brick", extra=legs.brick_none_streamed), None),
        Leg("image_128", "eam_cube", "cta_cell", [], {"COMD_EAM_IMAGE": "128"}, 3, K("brick", extra=legs.brick_all_streamed), None),
        Leg("image_mixed", "eam_mixed", "cta_cell", [], {}, 3, None, _derive_image("brick")),
        Leg("brick_1_1", "eam_cube", "cta_cell", [], {"COMD_EAM_BRICK": "1,1"}, 3, K("brick", extra=legs.brick_shape(1, 1)), None),
        Leg("brick_2_2", "eam_cube", "cta_cell", [], {"COMD_EAM_BRICK": "2,2"}, 3, K("brick", extra=legs.brick_shape(2, 2)), None),
        Leg("brick_3_5", "eam_cube", "cta_cell", [], {"COMD_EAM_BRICK": "3,5"}, 3, K("brick", extra=legs.brick_shape(3, 5)), None),
        Leg("round2_stencil_128", "eam_cube", "cta_cell", [], {"COMD_EAM_CTA": "cell", "COMD_EAM_STENCIL": "128"}, 3, K("cta_cell_round2", extra=legs.stencil_slice(128, "all")), None),
        Leg("round2_stencil_mixed", "eam_mixed", "cta_cell", [], {"COMD_EAM_CTA": "cell"}, 3, None, _derive_stencil),
        Leg("round2_default_slice", "eam_cube", "cta_cell", [], {"COMD_EAM_CTA": "cell"}, 3, K("cta_cell_round2", extra=legs.stencil_slice(0, "none")), None),
        Leg("clamps_kept", "eam_cube", "cta_cell", [], {"COMD_EAM_CLAMP": "1"}, 3, K("brick", extra=legs.clamps_kept), None),
        Leg("overlap_whole_bricks", "eam_cube", "cta_cell", A1, {}, 3, K("brick", "whole_bricks"), None),
        Leg("overlap_groups_0", "eam_cube", "cta_cell", A1, {"COMD_EAM_GROUPS": "0"}, 3, K("brick", "cell_by_cell"), None),
    ],
    "eam_atom": [
        Leg("default", "eam_cube", "thread_atom", A0, {}, 3, K("atom_brick", extra=legs.hand_over(True)), None),
        Leg("default_overlap", "eam_cube", "thread_atom", A1, {}, 3, K("atom_brick", "whole_bricks", extra=legs.hand_over(True)), None),
        Leg("handover_0", "eam_cube", "thread_atom", A0, {"COMD_EAM_ATOM_HANDOVER": "0"}, 3, K("atom_brick", extra=legs.hand_over(False)), None),
        Leg("handover_0_overlap", "eam_cube", "thread_atom", A1, {"COMD_EAM_ATOM_HANDOVER": "0"}, 3, K("atom_brick", "whole_bricks", extra=legs.hand_over(False)), None),
        Leg("image_128", "eam_cube", "thread_atom", A0, {"COMD_EAM_IMAGE": "128"}, 3, K("atom_brick", extra=legs.brick_all_streamed), None),
        Leg("image_mixed", "eam_mixed", "thread_atom", A0, {}, 3, None, _derive_image("atom_brick")),
        Leg("brick_2_3", "eam_cube", "thread_atom", A0, {"COMD_EAM_ATOM_BRICK": "2,3"}, 3, K("atom_brick", extra=legs.atom_shape(2, 3)), None),
        Leg("brick_4_5", "eam_cube", "thread_atom", A0, {"COMD_EAM_ATOM_BRICK": "4,5"}, 3, K("atom_brick", extra=legs.atom_shape(4, 5)), None),
        Leg("rows_16", "eam_cube", "thread_atom", A0, {"COMD_EAM_ATOM_ROWS": "16"}, 3, K("atom_brick", extra=legs.rows_capacity(16, 1.0, 1.0)), None),
        Leg("rows_48_compressed", "eam_l35", "thread_atom", A0, {"COMD_EAM_ATOM_ROWS": "48"}, 3, K("atom_brick", extra=legs.rows_capacity(48, 0.1, 0.9)), None),
        Leg("ablate_16", "eam_cube", "thread_atom", A0, {"COMD_EAM_ABLATE": "16"}, 3, K("atom_brick", extra=legs.offset_limit_64), None),
        Leg("round2", "eam_cube", "thread_atom", A0, {"COMD_EAM_THREAD_ATOM": "cell"}, 3, K("thread_atom_round2"), None),
        Leg("groups_0", "eam_cube", "thread_atom", A0, {"COMD_EAM_GROUPS": "0"}, 3, K("atom_brick", "all_cells"), None),
        Leg("groups_0_overlap", "eam_cube", "thread_atom", A1, {"COMD_EAM_GROUPS": "0"}, 3, K("atom_brick", "cell_by_cell"), None),
    ],
    "lists": [
        Leg("pair_slab_rows", "lj_cube", "thread_atom_nl", [], {}, 2, legs.nl_format(1), None),
        Leg("pair_bank_order", "lj_cube", "thread_atom_nl", [], {"COMD_NL_BANK_ORDER": "1"}, 2, legs.nl_format(1), None),
        Leg("pair_global_slots", "lj_cube", "thread_atom_nl", [], {"COMD_NL_GLOBAL": "1"}, 2, legs.nl_format(0), None),
        Leg("eam_default", "eam_cube", "thread_atom_nl", [], {}, 3, legs.nl_format(4, "listed_rows"), None),
        Leg("eam_global", "eam_cube", "thread_atom_nl", [], {"COMD_NL_GLOBAL": "1"}, 3, legs.nl_format(0, "nl_global"), None),
        Leg("eam_nl_lds", "eam_cube", "thread_atom_nl", [], {"COMD_EAM_NL": "lds"}, 3, legs.nl_format(2, "nl_lds"), None),
    ],
    "tables": [
        Leg("setfl_thread_atom", "eam_setfl", "thread_atom", [], {}, 3, K("atom_brick", extra=legs.tables(legs.SETFL_TABLES_IN_LDS)), None),
        Leg("setfl_cta_cell", "eam_setfl", "cta_cell", [], {}, 3, K("brick", extra=legs.tables(legs.SETFL_TABLES_IN_LDS)), None),
        Leg("spline_thread_atom", "eam_cube", "thread_atom", ["-P"], {}, 3, K("atom_brick", extra=legs.tables(False, True)), None),
        Leg("spline_cta_cell", "eam_cube", "cta_cell", ["-P"], {}, 3, K("brick", extra=legs.tables(False, True)), None),
        Leg("spline_thread_atom_nl", "eam_cube", "thread_atom_nl", ["-P"], {}, 3, K("listed_rows", extra=legs.tables(False, True)), None),
    ],
}
FAMILY_LEG_COUNT = {"lj": 10, "eam_cta": 12, "eam_atom": 14, "lists": 6, "tables": 5}          # stated, not computed: a leg that leaves the table is missed
_LEG_REFERENCE = {}


def _leg_reference(orc, name, steps, spline):
    if (name, steps, spline) not in _LEG_REFERENCE:
        o = _make(orc, STATES[name], spline=spline)
        o.step(steps)
        got = _snapshot(orc, o, STATES[name].eam)
        o.close()
        _LEG_REFERENCE[(name, steps, spline)] = got
    return _LEG_REFERENCE[(name, steps, spline)]


def _run_leg(gpu, orc, monkeypatch, leg):
    st = STATES[leg.state]
    box = {"n": st.n, "flags": ["-l", st.lat]}
    env, fact = leg.env, leg.fact
    overlap, flags = (1, leg.flags[2:]) if leg.flags[:2] == A1 else (0, leg.flags[2:] if leg.flags[:2] == A0 else leg.flags)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if leg.derive:          # a first run without the value that splits the launch: the populations it reports give that value
        with gpu.Simulation(_flags(st, leg.method, overlap, flags)) as sim:
            sim.step(leg.steps)
            env, fact = leg.derive(legs.observe(sim, box))
        print(leg.name, "derived", env)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    with gpu.Simulation(_flags(st, leg.method, overlap, flags)) as sim:
        assert tuple(a for a in range(3) if sim.grid[a] == 2) == st.two, sim.grid
        sim.step(leg.steps)
        f, u = sim.gather(2), sim.gather(3)
        spline = "-P" in leg.flags
        tol = TOL_SPLINE if spline else TOL
        if "-I" in leg.flags:
            from test_lj_interpolation import lj_table, restated_forces
            fo, uo = restated_forces(sim.gather(0), _extent(st), lj_table(), 5.0 * SIGMA)
            ref = {"f": fo, "u": uo}
        else:
            ref = _leg_reference(orc, leg.state, leg.steps, spline)
        err = {"f": np.abs(f - ref["f"]).max() / np.abs(ref["f"]).max(), "u": np.abs(u - ref["u"]).max()}
        if st.eam:
            err.update(rho=np.abs(sim.gather(4) - ref["rho"]).max(), df=np.abs(sim.gather(5) - ref["df"]).max())
        print(f"{leg.state} {leg.method} {leg.name}: " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
        assert err["f"] <= tol["force_rel_to_max"] and err["u"] <= tol["per_atom_energy_abs"], err
        if st.eam:
            df_tol = tol["eam_dfembed_abs"] if spline or leg.state not in TOL_STATE else _dfembed_tol(leg.state)
            assert err["rho"] < tol["eam_density_abs"] and err["df"] < df_tol, err
        fact(legs.observe(sim, box))


def _ids(family):
    assert len(LEGS[family]) == FAMILY_LEG_COUNT[family]
    return dict(argnames="leg", argvalues=LEGS[family], ids=[leg.name for leg in LEGS[family]])


@pytest.mark.gpu
@pytest.mark.parametrize(**_ids("lj"))
def test_lj_leg(gpu, orc, monkeypatch, leg):
    _run_leg(gpu, orc, monkeypatch, leg)


@pytest.mark.gpu
@pytest.mark.parametrize(**_ids("eam_cta"))
def test_eam_cta_leg(gpu, orc, monkeypatch, leg):
    _run_leg(gpu, orc, monkeypatch, leg)


@pytest.mark.gpu
@pytest.mark.parametrize(**_ids("eam_atom"))
def test_eam_atom_leg(gpu, orc, monkeypatch, leg):
    _run_leg(gpu, orc, monkeypatch, leg)


@pytest.mark.gpu
@pytest.mark.parametrize(**_ids("lists"))
def test_lists_leg(gpu, orc, monkeypatch, leg):
    _run_leg(gpu, orc, monkeypatch, leg)


@pytest.mark.gpu
@pytest.mark.parametrize(**_ids("tables"))
def test_tables_leg(gpu, orc, monkeypatch, leg):
    _run_leg(gpu, orc, monkeypatch, leg)


# ---------------------------------------------------------------- 4c. GPU: Verlet rows and pairlists over rebuilds
REBUILD_STEPS = 40
REBUILDS = [("eam_cube", "thread_atom_nl", []), ("lj_cube", "thread_atom_nl", []), ("lj_cube", "cta_cell -L", [])]          # (lj_cube's list runs: -S 0.03, a skin of 0.35 A)


@pytest.mark.gpu
@pytest.mark.parametrize("name,method,extra", REBUILDS, ids=[f"{r[0]}-{r[1].replace(' -', '_')}" for r in REBUILDS])
def test_lists_over_rebuilds(gpu, orc, name, method, extra):
    """40 steps, in which the lists are built more than once and not every step (asserted from the run): rows that hold one atom's slot through two images are made
    from moved positions.  Positions, forces and E/N against the checker at the trajectory tolerances of tests/multirank_worker.py."""
    st = STATES[name]
    with gpu.Simulation(_flags(st, method, 0, extra)) as sim:
        assert sim.grid == st.list_grid
        o = _make(orc, st)
        fo = o.gather(orc.F)
        assert np.abs(sim.gather(2) - fo).max() <= TOL["force_rel_to_max"] * np.abs(fo).max()
        sim.step(REBUILD_STEPS)
        o.step(REBUILD_STEPS)
        e1, eo, fo = sim.energy(), o.energy(), o.gather(orc.F)
        d = sim.gather(0) - o.gather(orc.R)
        d -= np.rint(d / _extent(st)) * _extent(st)
        print(f"{name} {method}: {sim.nl_builds} builds  max|dr| {np.abs(d).max():.3e}  max|df|/max|f| {np.abs(sim.gather(2) - fo).max() / np.abs(fo).max():.3e}  "
              f"|dE|/N {abs((e1[0] + e1[1]) - (eo[0] + eo[1])) / e1[2]:.3e}")
        assert 1 < sim.nl_builds < REBUILD_STEPS, sim.nl_builds
        assert np.abs(d).max() < TRAJ_R
        assert np.abs(sim.gather(2) - fo).max() < TRAJ_F * np.abs(fo).max()
        assert abs((e1[0] + e1[1]) - (eo[0] + eo[1])) / e1[2] < TOL["energy_per_atom_trace"]
        sim.sum_atoms()
        assert sim.energy()[2] == st.atoms
        o.close()


# ---------------------------------------------------------------- 4d. GPU: redistribution, bit for bit
def _displacements(st, kind, r):
    """The moves of a kind, each followed by a redistribution; (displacement, rigid) each.
    both_faces: on every 2-cell axis the atoms of the lower cell move down and those of the upper cell up, by 0.3 of a cell: atoms leave through both faces of the axis
      in ONE exchange and come back in through the opposite ones.  Not a rigid move: the two halves of the crystal are pushed into each other across the periodic face
      (forces of 1e5 eV/A, densities beyond the F table), so only the index work is compared, which is what the move is for.
    out_and_back: a rigid shift of +0.3 of a cell along every axis, then one of -0.6 from where that left the atoms: out through the upper faces, then out through the
      lower ones; forces and energy are the checker's after each.
    deep: a rigid shift of 0.9 of a cell along every 2-cell axis (0.3 along the others): nearly every atom changes cell, and those of the upper cell land deep in the halo
      cell -- as deep as an atom may: the halo is one cell deep, and an atom beyond it is lost (a shift of more than a cell cannot be run)."""
    size = _extent(st) / np.array(st.grid)
    two = np.array([a in st.two for a in range(3)])
    if kind == "both_faces":
        return [(np.where(two[None, :], np.where(r < size[None, :], -0.3, 0.3), 0.3) * size[None, :], False)]
    if kind == "out_and_back":
        return [(np.broadcast_to(0.3 * size, r.shape), True), (np.broadcast_to(-0.6 * size, r.shape), True)]
    return [(np.broadcast_to(np.where(two, 0.9, 0.3) * size, r.shape), True)]


REDISTRIBUTED = ["eam_cube", "eam_mixed", "lj_cube"]
KINDS = ["both_faces", "out_and_back", "deep"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", REDISTRIBUTED)
def test_redistribution_is_bit_exact(gpu, orc, name, kind):
    """tests/test_gpu_parity.py test_redistribution_is_bit_exact on 2-cell axes: after every move each cell, local and halo, holds exactly the checker's atoms in gid
    order with bit-identical r (the periodic shift included) and p; after a rigid move the forces and the energy are the checker's."""
    st = STATES[name]
    extra = ["--maxAtoms", 96 if st.eam else 384]          # a cell transiently holds its old and its incoming atoms
    with gpu.Simulation(_flags(st, "thread_atom", 0, extra)) as sim:
        assert sim.grid == st.grid
        o = _make(orc, st, cap=sim.max_atoms)
        _assert_cells_equal(sim.cells(), o.rank_cells(0), sim.n_total_boxes)
        seen_low = seen_high = False
        for k in range(len(_displacements(st, kind, sim.gather(0)))):
            r = sim.gather(0)
            assert np.array_equal(r, o.gather(orc.R))
            d, rigid = _displacements(st, kind, r)[k]
            moved = r + d
            low, high = (moved < 0.0)[:, list(st.two)], (moved >= _extent(st))[:, list(st.two)]
            print(f"{name} {kind} move {k}: {int(low.any(1).sum())} atoms leave through a lower face of a 2-cell axis, {int(high.any(1).sum())} through an upper one")
            seen_low, seen_high = seen_low or bool(low.any()), seen_high or bool(high.any())
            sim.scatter(0, moved)
            o.scatter(orc.R, moved)
            sim.redistribute(); sim.compute_force(); sim.kinetic_energy()
            o.redistribute(); o.compute_force()
            c = sim.cells()
            _assert_cells_equal(c, o.rank_cells(0), sim.n_total_boxes)
            assert int(c["nAtoms"][:sim.n_local_boxes].sum()) == st.atoms
            if rigid:
                fo = o.gather(orc.F)
                assert np.abs(sim.gather(2) - fo).max() <= TOL["force_rel_to_max"] * np.abs(fo).max()
                assert abs(sim.energy()[0] - o.energy()[0]) / st.atoms <= TOL["energy_per_atom_step0"]
        assert seen_high and (kind == "deep" or seen_low)
        o.close()


# ---------------------------------------------------------------- 4e. analyses
ANALYSED = [("eam_cube", 0), ("eam_mixed", 0), ("lj_cube", 0), ("eam_cube", 5), ("eam_mixed", 5), ("lj_cube", 5), ("eam_hot", 360)]
BINS = 48


def _key(name, steps):
    return ("two_cell_gpu", name) if steps == 0 else None          # the step-0 positions do not depend on the method: one reference for both


def test_analysis_references_stay_inside_their_caps(orc):
    """The numpy references of tests/test_rdf.py, test_csp.py and test_cna.py on the checker's positions of the analysed states, at step 0 and after the steps: the
    atoms and pairs they leave out as near-ties (DELTA) stay inside the caps those files state -- none in double -- so the GPU comparisons below are exact ones."""
    import test_cna, test_csp, test_rdf
    delta = test_csp.DELTA32 if SINGLE else test_csp.DELTA64
    for name, steps in ANALYSED:
        ref = _reference(orc, name)
        st = ref["st"]
        assert steps in (0, st.steps)
        pos = ref["sk"]["r"] if steps else ref["s0"]["r"]
        edges = np.arange(BINS + 1, dtype=np.float64) * (ref["rc"] / BINS)
        cum, near = test_rdf._reference(("two_cell", name, steps), pos, _extent(st), edges, delta)
        assert near.sum() <= (test_rdf.CAP32 * int(cum[-1]) if SINGLE else 0), (name, steps, int(near.sum()))
        test_csp._left_out(test_csp._reference(("two_cell", name, steps), pos, _extent(st), ref["rc"], test_csp.R_COORD, delta), delta, SINGLE)
        test_cna._left_out(test_cna._reference(("two_cell", name, steps), pos, _extent(st), ref["rc"], delta), delta, SINGLE)


def _virial_reference(sim, st, rc):
    """test_pressure.py's restatements at the positions of the run: LJ analytic (test_lj_tensor_matches_the_restatement), EAM from the tables and dF/drho of the run
    (test_eam_setfl_tensor_matches_the_restatement)"""
    pos = sim.gather(0)
    i, j, d, r = _pairs(pos, _extent(st), rc)
    if st.eam:
        df = sim.gather(5)
        _, dphi = _interpolate(*sim.eam_table(0), r)
        _, drho = _interpolate(*sim.eam_table(1), r)
        s = (dphi + (df[i] + df[j]) * drho) / r
        return _tensor(d, -s[:, None] * d)
    s6 = SIGMA ** 6
    fr = 24.0 * EPS * s6 * r ** -8 * (2.0 * s6 * r ** -6 - 1.0)
    return _tensor(d, fr[:, None] * d)


@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", ANALYSED, ids=[f"{a[0]}-step{a[1]}" for a in ANALYSED])
@pytest.mark.parametrize("method", ["thread_atom", "cta_cell"])
def test_analyses_match_numpy(gpu, orc, name, steps, method):
    """Virial and pressure tensor, pair histogram and g(r), centro-symmetry and coordination, CNA on 2-cell grids, where the shared stencil walk meets every
    neighbour cell twice: against the numpy references of test_pressure.py (1e-11 of the largest component; float build: 1e-5, its float rule), test_rdf.py, test_csp.py
    and test_cna.py under their own rules."""
    import test_cna, test_csp, test_rdf
    ref = _reference(orc, name)
    st = ref["st"]
    with gpu.Simulation(_flags(st, method)) as sim:
        assert sim.grid == st.grid
        if steps:
            sim.step(steps)
        else:
            assert np.array_equal(sim.gather(0), ref["s0"]["r"])
        w, k = sim.virial()
        want = _virial_reference(sim, st, sim.cutoff)
        ek = sim.energy()[1]
        print(f"{name} step {steps}: virial relative error {_rel(w, want):.3e}  trace K / 2 eK - 1 {np.trace(k) / (2.0 * ek) - 1.0:.3e}")
        assert _rel(w, want) <= (1e-5 if SINGLE else 1e-11), (w, want)
        assert abs(np.trace(k) - 2.0 * ek) <= (1e-5 if SINGLE else 1e-13) * 2.0 * ek
        assert np.array_equal(w, w.T) and np.array_equal(k, k.T)
        p = sim.pressure_tensor()
        # (the float build holds the box edges in float: the volume is three roundings of 6e-8 away from the product of the double extents)
        assert np.abs(p - (k + w) / np.prod(_extent(st))).max() <= (1e-6 if SINGLE else 1e-13) * np.abs(p).max()
        test_rdf._against_numpy(sim, np.array(st.n, dtype=np.float64), BINS, key=_key(name, steps) or ("two_cell", name, steps, method), single=SINGLE)
        r_centres, g = sim.rdf(BINS)
        assert g.shape == (BINS,) and np.all(g >= 0.0) and g.max() > 1.0
        test_csp._against_numpy(sim, _extent(st), ref["rc"], key=_key(name, steps), single=SINGLE)
        test_cna._against_numpy(sim, _extent(st), ref["rc"], key=_key(name, steps), single=SINGLE)


@pytest.mark.gpu
def test_msd_of_eam_hot(gpu, orc):
    """Tracked displacements over eam_hot's 360 steps against the incremental reference of tests/test_msd.py (the sum of the minimum-image increments of the gathered
    positions, a step at a time), at its bound; the positions themselves show atoms wrapping through the faces of the 2-cell axes."""
    from test_msd import _check_msd, _incremental, tol
    st = STATES["eam_hot"]
    with gpu.Simulation(_flags(st, "cta_cell")) as sim:
        assert sim.grid == st.grid == (2, 2, 2)
        sim.track_displacement()
        ref, r_first, r_last, crossed = _incremental(sim, st.steps, _extent(st))
        d = sim.displacements()
        print(f"eam_hot: {int((crossed > 0).sum())} atoms wrapped, max|d| {np.abs(ref).max():.3f} A, max error {np.abs(d - ref).max():.3e}, bound {tol(st.steps, _extent(st).max()):.3e}")
        assert (crossed > 0).sum() >= 1
        assert np.abs(ref).max() < 0.5 * _extent(st).min()
        assert np.abs(d - ref).max() <= tol(st.steps, _extent(st).max())
        _check_msd(sim, d)


# ---------------------------------------------------------------- 4f. several ranks
RANKS = [((2, 2, 2), "cta_cell", 0), ((2, 2, 2), "cta_cell", 1), ((2, 2, 2), "thread_atom", 0), ((2, 2, 2), "thread_atom", 1),
         ((2, 1, 1), "thread_atom_nl", 0), ((2, 1, 1), "cta_cell+H", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("grid,method,overlap", RANKS, ids=[f"{'x'.join(map(str, r[0]))}-{r[1]}-a{r[2]}" for r in RANKS])
def test_ranks_of_two_cells(orc, grid, method, overlap):
    """EAM 8^3 on 2 x 2 x 2 ranks (eight processes): every rank owns 2 x 2 x 2 cells, and on every axis its two neighbours are one and the same rank, whose two
    messages must not be swapped; on 2 x 1 x 1 ranks the x axis has two cells per rank (thread_atom_nl: cells of 5.445 A, still two).  tests/multirank_worker.py
    compares forces, positions and E/N with the checker; the grids are asserted here, from the checker's ranks."""
    o = orc.Oracle(8, grid, eam=1, delta=0.1)
    assert o.n_ranks == grid[0] * grid[1] * grid[2]
    for rank in range(o.n_ranks):
        assert o.rank_grid(rank)[0] == tuple(2 if grid[a] == 2 else 5 for a in range(3)), o.rank_grid(rank)
    o.close()
    assert int(8 * 3.615 / grid[0] / (4.95 * 1.1)) == 2
    outs = _launch("gpu", grid, 1, 8, extra=(method, overlap))
    assert "gpu-mode OK" in outs[0] and "sized exchanges" in outs[0] and " 0 sized exchanges" not in outs[0]


@pytest.mark.gpu
def test_rccl_loopback_on_two_cells():
    """comm_rccl.hip carries the six halo messages of a 2 x 2 x 2 grid (EAM 4^3, cta_cell): every local cell is in a message to both directions of every axis."""
    outs = _launch("rccl", (1, 1, 1), 1, 4, extra=("cta_cell", 1), env_extra={"COMD_LOOPBACK_TRANSPORT": "1"})
    assert "rccl-loopback OK" in outs[0]


# the GPU tests of this file (tests/test_single_precision.py runs them again in the float build and counts them)
GPU_CASE_COUNT = len(_method_cases()) + sum(FAMILY_LEG_COUNT.values()) + len(REBUILDS) + len(REDISTRIBUTED) * len(KINDS) + 2 * len(ANALYSED) + 1 + len(RANKS) + 1
