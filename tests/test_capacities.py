"""Cell slots, Verlet rows and the halo's depth at exact fit and one unit short.

Every array an atom can be appended to has a fixed capacity: the cell slots (--maxAtoms), the Verlet rows (--maxNeighbors, rounded per list format) and the halo
region (one cell deep).  An append beyond capacity raises a device status word, is dropped, and the run is stopped by comdCheckStatus / comdPollStatus with
exit(-1).  Every case here has two sides.  FIT: the container is exactly full and the run agrees with the checker.  SHORT: the same state with one unit less; the
child process ends with exit status 255 and the rule's sentence on stderr, no later than the step() (or the creation, whose first force evaluation builds the lists)
in which the checker says the capacity is first exceeded.  The states are found on the CPU from the checker and numpy, recorded below and asserted by the `not gpu`
tests before a GPU test relies on them.

  A. cell slots: LJ with every cell full (256 atoms in 256 slots, four full waves); EAM at its natural peak (18 atoms in 18 slots) through s* - 1 steps, stopped at
     step s* by each of the three kernels that write atoms into cells (UpdateLinkCells, UnloadAtomsBufferPacked, MirrorAtomCells); the host's refusal at creation.
  B. Verlet rows: formats 0 (LJ and EAM), 1 (plain and COMD_NL_BANK_ORDER=1), 2 and 4, row lengths counted in numpy.
  C. the halo: an atom that lands a few ulps inside the far edge of a halo cell, and a few ulps beyond it.

A cell needs room for its arrivals BEFORE its leavers are dropped (UpdateLinkCells appends and leaves holes, CompactSortCells drops them later, as the reference's
moveAtom does): the demand of a step is the occupancy before it plus the arrivals, and the states are chosen so that the demand of every step before s* fits.

What runs between a raise and the host's read, and why it is safe (read before the first SHORT run; the run goes on to the end of the step() call that raised):
  * UpdateLinkCells, UnloadAtomsBufferPacked, MirrorAtomCells: an atom that finds no slot is not written (slot >= cap: return) and stays in its source slot.  The
    count of the destination has been raised beyond cap by then, so each of them marks that cell dirty (added with these tests: without it a full local cell
    that nothing else touched kept a count of cap + 1 through the whole force evaluation);
  * CompactSortCells / CompactSortCellsWave visit every dirty cell, clamp n to cap and write back the number of live atoms (<= cap).  sortAtomsGpu runs them over
    all cells before any force kernel, and with -a 1 updateLinkCellsGpu runs them before the interior force launch: no force, list-build, energy or integrator
    kernel sees a count beyond cap;
  * between an overflowing unpack of one axis and the compaction, ScanCellCountsBatch and LoadAtomsBufferPacked of the next axis read the raised count: the pack
    reads slots t < nAtoms[c] with t < blockDim, i.e. at most the first slots of the NEXT cell (send cells are never the last cell of the arrays: the z+ halo is
    sent nowhere), writes inside the message (its positions come from the same counts) and the total is checked against the message capacity (status[2]);
    MirrorAtomCells clamps the source count (cnt < cap ? cnt : cap) and tests every destination slot (k >= cap);
  * a lost atom (comdCoordInHalo fails) is not moved at all: it stays in its slot of a local cell with its far coordinates, which the force kernels read as
    an atom with no neighbour inside the cutoff;
  * Verlet rows: BuildNeighborList (n < nl.maxNbr), BuildNeighborListSlabs (n < nl.rows; bank order: pos < nl.rows), BuildNeighborListCell16 (k < nl.rows) and the
    brick build (kA < b.rows) test every entry they write and store counts clamped to the row; the force kernels loop over those counts.

Out of scope: the row limit of the EAM cta_cell kernel (status[3] bit 1, the compare in EAM_Force_cta_cell: not user-settable, and reached only at a density no
state here has), capacities on 2-cell axes (the force, list and analysis paths on such boxes, at default capacities, are tests/test_two_cell_boxes.py), multi-rank runs.
"""
import json
import os
import subprocess
import sys
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = json.load(open(os.path.join(HERE, "golden", "reference_values.json")))
SINGLE = os.environ.get("COMD_PRECISION", "double") == "single"
TOL = G["tolerances_single" if SINGLE else "tolerances"]
REAL = np.float32 if SINGLE else np.float64
FACE_MARGIN = 1e-4 if SINGLE else 1e-6              # Angstroms: no compared atom is nearer to a cell face (cells are compared exactly; 1e-4: fifty ulps of a float coordinate)
OVERFLOW = "a link cell overflowed its %d slots (raise --maxAtoms)"
LOST = "an atom moved beyond the halo region and was lost"
ROW_OVER = "more than %d neighbours inside cutoff + skin (raise --maxNeighbors)"


# ---------------------------------------------------------------- the child processes
def _child(tmp_path, tag, job, env=None, timeout=120):
    """one run of capacity_worker.py: (exit status, stdout lines, stderr, the snapshots it wrote)"""
    out = str(tmp_path / tag)
    proc = subprocess.run([sys.executable, os.path.join(HERE, "capacity_worker.py"), json.dumps(job), out], cwd=ROOT, env=dict(os.environ, **(env or {})),
                          capture_output=True, text=True, timeout=timeout)
    snaps = []
    while os.path.exists(f"{out}.{len(snaps)}.npz"):
        snaps.append(np.load(f"{out}.{len(snaps)}.npz"))
    return proc.returncode, proc.stdout.split("\n"), proc.stderr, snaps


def _stopped(rc, lines, err, sentence, reached):
    """the child ended by the library's exit(-1) with `sentence`, after exactly the lines `reached`"""
    said = [ln for ln in lines if ln.startswith("created") or ln.startswith("reached")]
    assert rc == 255, (rc, lines[-5:], err[-1500:])
    assert sentence in err, err[-1500:]
    assert said == reached, (said, err[-1500:])


def _flags(st, method, overlap, extra=()):
    m = method.split()
    lat = ["-l", st.lat] if st.lat > 0 else []
    return ["-x", st.n[0], "-y", st.n[1], "-z", st.n[2], "-r", st.delta, "-T", st.temp, "-m", m[0], "-a", overlap] + lat + (["-e"] if st.eam else []) + m[1:] + list(extra)


def _snapshot(orc, o, eam):
    ep, ek = o.energy()
    got = {"r": o.gather(orc.R), "f": o.gather(orc.F), "u": o.gather(orc.U), "ep": ep, "ek": ek}
    if eam:
        got.update(rho=o.gather(orc.RHOBAR), df=o.gather(orc.DFEMBED))
    return got


def _compare(tag, snap, ref, eam, n_atoms):
    """forces, per-atom energies, (EAM) rhobar and dF/drho, U/N, K/N and E/N of a child's snapshot against the checker's state, at the recorded tolerances"""
    fmax = np.abs(ref["f"]).max()
    ep, ek = snap["energy"]
    err = {"f": float(np.abs(snap["f"] - ref["f"]).max() / fmax), "u": float(np.abs(snap["u"] - ref["u"]).max()), "U/N": abs(ep - ref["ep"]) / n_atoms,
           "K/N": abs(ek - ref["ek"]) / n_atoms, "E/N": abs((ep + ek) - (ref["ep"] + ref["ek"])) / n_atoms}
    if eam:
        err.update(rho=float(np.abs(snap["rho"] - ref["rho"]).max()), df=float(np.abs(snap["df"] - ref["df"]).max()))
    print(f"{tag}: max|f| {fmax:.3e}  " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert int(snap["n_global"]) == n_atoms
    assert err["f"] <= TOL["force_rel_to_max"] and err["u"] <= TOL["per_atom_energy_abs"], err
    assert err["U/N"] <= TOL["energy_per_atom_step0"] and err["K/N"] <= TOL["kinetic_per_atom"] and err["E/N"] <= TOL["energy_per_atom_trace"], err
    if eam:
        assert err["rho"] <= TOL["eam_density_abs"] and err["df"] <= TOL["eam_dfembed_abs"], err


def _same_cells(snap, cells, n_local):
    """index work, bit for bit: every cell's occupancy, local and halo; every local cell's gids (ascending); halo cells sorted"""
    assert np.array_equal(snap["nAtoms"], cells["nAtoms"])
    for b in range(len(cells["nAtoms"])):
        k = int(cells["nAtoms"][b])
        assert np.all(np.diff(snap["gid"][b, :k]) > 0), b
        if b < n_local:
            assert np.array_equal(snap["gid"][b, :k], cells["gid"][b, :k]), b


def _face_distance(pos, extent, grid):
    size = extent / np.array(grid, dtype=np.float64)
    t = pos / size
    t = t - np.floor(t)
    return float((np.minimum(t, 1.0 - t) * size).min())


# ================================================================ A. cell slots
# grid, atoms, the peak occupancy over all cells (local and halo) after each of the steps 0 .. steps, the first step whose peak exceeds `cap` (None: none does), the cell it
# happens in and the kernel that must raise it, are the checker's own figures; test_cell_states_are_what_is_recorded takes them again.  LJ: 5 sigma = 11.575 A,
# lat 3.615 A: 12^3 lattice cells make 3^3 link cells of 4 lattice constants, 4 * 4^3 = 256 atoms each, none nearer than 0.25 lat = 0.9 A to a face.  EAM: Cu_u6.eam.
CellState = namedtuple("CellState", "eam n lat delta temp steps grid atoms peaks cap first_over cell writer")
CELL_STATES = {
    "lj_full":   CellState(0, (12, 12, 12), -1.0, 0.1, 600.0,   3,  (3, 3, 3), 6912, (256,) * 4, 256, None, None, None),
    "eam_local": CellState(1, (8, 7, 9),    -1.0, 0.1, 6000.0,  17, (5, 5, 6), 2016, (18,) * 17 + (19,), 18, 17, 107, "local"),      # cell (2, 1, 4): no face of the box
    "eam_cross": CellState(1, (5, 6, 7),    -1.0, 0.1, 15000.0, 24, (3, 4, 5), 840, (18,) * 24 + (19,), 18, 24, 1,   "halo"),       # cell (1, 0, 0): the atom comes in through y or z
}
_CELL_RUNS = {}


def _cell_run(orc, name):
    """The checker's run of a state with roomy cells, a step at a time: peak occupancy and demand (occupancy before the step + arrivals, local cells; the occupancy
    itself for halo cells, which are emptied first) per step; the state at step 0, at the last step that fits and its cells; where and how the first overflow happens."""
    if name in _CELL_RUNS:
        return _CELL_RUNS[name]
    st = CELL_STATES[name]
    o = orc.Oracle(st.n, eam=st.eam, temperature=st.temp, delta=st.delta, lat=st.lat)
    grid, n_local, n_total = o.rank_grid(0)
    extent = np.array(st.n, dtype=np.float64) * orc.lib().oracle_lattice(o.ptr)
    cells = o.rank_cells(0)
    occ = cells["nAtoms"].copy()
    home = {int(g): b for b in range(n_local) for g in cells["gid"][b, :occ[b]]}
    r_prev = o.gather(orc.R)
    run = dict(st=st, grid=tuple(grid), n_local=n_local, n_total=n_total, extent=extent, s0=_snapshot(orc, o, st.eam), cells0=cells, peaks=[int(occ.max())],
               least=[int(occ.min())], demand=[int(occ.max())], moved=[0], over=None)
    last = st.steps if st.first_over is None else st.first_over - 1
    for t in range(1, st.steps + 1):
        o.step(1)
        cells = o.rank_cells(0)
        now = cells["nAtoms"].copy()
        here = {int(g): b for b in range(n_local) for g in cells["gid"][b, :now[b]]}
        r = o.gather(orc.R)
        arrivals, crossed = np.zeros(n_local, dtype=np.int64), {}
        for g, b in here.items():
            if home[g] != b:
                arrivals[b] += 1
                crossed.setdefault(b, []).append(bool((np.abs(r[g] - r_prev[g]) > 0.5 * extent).any()))
        run["peaks"].append(int(now.max()))
        run["least"].append(int(now.min()))
        run["demand"].append(int(max((occ[:n_local] + arrivals).max(), now[n_local:].max())))
        run["moved"].append(int(arrivals.sum()))
        if st.cap is not None and run["over"] is None and now.max() > st.cap:
            full = np.nonzero(now > st.cap)[0]
            local = [int(c) for c in full if c < n_local]
            # local re-binning raises it when an atom arrives from inside the box; the halo path when the atom comes across a periodic face (UpdateLinkCells has put it into
            # a halo cell, which is empty at that point) and for the halo images of the cell
            writers = set()
            for c in local:
                writers |= {"halo" if x else "local" for x in crossed[c]}
            if len(full) > len(local):
                writers.add("halo")
            run["over"] = dict(step=t, cells=local, images=len(full) - len(local), writers=writers)
        if t == last:
            run["sk"], run["cellsk"] = _snapshot(orc, o, st.eam), cells
            run["face"] = _face_distance(r, extent, grid)
        occ, home, r_prev = now, here, r
    o.close()
    print(f"{name}: grid {grid} atoms {o.n_global} peaks {run['peaks']} demand {run['demand']} moved {run['moved']} over {run['over']} "
          f"least face distance at step {last}: {run['face']:.3e} A")
    _CELL_RUNS[name] = run
    return run


@pytest.mark.parametrize("name", list(CELL_STATES))
def test_cell_states_are_what_is_recorded(orc, name):
    """The checker's figures of a state are the recorded ones.  Before the first overflow every step's demand fits the capacity, so a run that stops earlier has
    stopped without cause; the cells compared exactly hold no atom within FACE_MARGIN of a face."""
    run = _cell_run(orc, name)
    st = run["st"]
    assert (run["grid"], len(run["s0"]["r"]), tuple(run["peaks"])) == (st.grid, st.atoms, st.peaks) and min(run["grid"]) >= 3
    assert run["face"] > FACE_MARGIN
    if st.first_over is None:
        # every cell, local and halo, is exactly full at every step and no atom changes cell
        assert set(run["least"]) == {st.cap} and set(run["demand"]) == {st.cap} and not any(run["moved"])
        assert st.cap % 64 == 0
        return
    over = run["over"]
    assert 0 < st.first_over <= 30 and over["step"] == st.first_over and over["cells"] == [st.cell] and over["writers"] == {st.writer}
    assert max(run["demand"][:st.first_over]) == st.cap == max(run["peaks"][:st.first_over]) and st.cap % 4 != 0
    assert sum(run["moved"][:st.first_over]) > 0
    if st.writer == "local":          # nothing but UpdateLinkCells can raise it: the cell touches no face of the box, so it has no halo image
        assert over["images"] == 0
    assert run["peaks"][0] <= st.cap          # the lattice fits at step 0: the host's putAtomInBox does not refuse first


def test_host_refuses_a_capacity_below_the_lattice(tmp_path):
    """--maxAtoms below the lattice's own occupancy (EAM 8 x 7 x 9: cells of up to 18 sites) is refused by the host while it places the lattice."""
    st = CELL_STATES["eam_local"]
    rc, lines, err, _ = _child(tmp_path, "refused", dict(flags=_flags(st, "thread_atom", 0, ["--maxAtoms", 17]), steps=[], host_only=True))
    assert rc == 255 and "created" not in lines and "is full (17 slots); raise --maxAtoms" in err, (rc, err[-800:])
    rc, lines, err, _ = _child(tmp_path, "placed", dict(flags=_flags(st, "thread_atom", 0, ["--maxAtoms", 18]), steps=[], host_only=True))
    assert rc == 0 and "created" in lines, (rc, err[-800:])


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("method", ["thread_atom", "cta_cell", "thread_atom_nl", "cta_cell -L"])
def test_lj_cells_of_four_full_waves(tmp_path, orc, method, overlap):
    """LJ 12^3 with --maxAtoms 256: every local and halo cell holds 256 atoms in 256 slots, no tail lane anywhere.  Forces and energies at step 0 and after 3 steps."""
    run = _cell_run(orc, "lj_full")
    st = run["st"]
    rc, lines, err, snaps = _child(tmp_path, "full", dict(flags=_flags(st, method, overlap, ["--maxAtoms", st.cap]), steps=[0, st.steps]))
    assert rc == 0 and len(snaps) == 2, (rc, err[-1500:])
    for when, snap, ref in (("step 0", snaps[0], run["s0"]), (f"step {st.steps}", snaps[1], run["sk"])):
        assert int(snap["max_atoms"]) == st.cap and tuple(snap["grid"]) == st.grid
        assert np.all(snap["nAtoms"] == st.cap) and len(snap["nAtoms"]) == run["n_total"]
        _compare(f"lj_full {method} -a {overlap} {when}", snap, ref, 0, st.atoms)
    if "_nl" not in method and "-L" not in method:          # (with lists the atoms keep their slots between builds: the cells are sorted at a build only)
        _same_cells(snaps[1], run["cellsk"], run["n_local"])


HALO_PATHS = {"mirror": {"COMD_HALO_MIRROR": "1"}, "message": {"COMD_HALO_MIRROR": "0"}}
WRITER_KERNEL = {("local", "mirror"): "UpdateLinkCells", ("local", "message"): "UpdateLinkCells", ("halo", "mirror"): "MirrorAtomCells", ("halo", "message"): "UnloadAtomsBufferPacked"}


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("halo", list(HALO_PATHS))
@pytest.mark.parametrize("method", ["thread_atom", "cta_cell"])
@pytest.mark.parametrize("name", ["eam_local", "eam_cross"])
def test_eam_cells_exactly_full_then_one_atom_more(tmp_path, orc, name, method, halo, overlap):
    """--maxAtoms = the peak occupancy of the steps 0 .. s* - 1 (18: no multiple of 4).  FIT: step(s* - 1) runs through, the cells are the checker's bit for bit, forces
    and energies within tolerance.  SHORT: the next step puts a 19th atom into a cell -- eam_local: from inside the box, raised by UpdateLinkCells; eam_cross: across
    a periodic face, raised by MirrorAtomCells (default) or UnloadAtomsBufferPacked (COMD_HALO_MIRROR=0) -- and the run ends inside that step() call."""
    run = _cell_run(orc, name)
    st = run["st"]
    assert (st.writer, halo) in WRITER_KERNEL and run["over"]["writers"] == {st.writer}
    rc, lines, err, snaps = _child(tmp_path, "cells", dict(flags=_flags(st, method, overlap, ["--maxAtoms", st.cap]), steps=[0, st.first_over - 1, 1]), HALO_PATHS[halo])
    assert len(snaps) == 2, (rc, lines[-5:], err[-1500:])
    assert int(snaps[0]["max_atoms"]) == st.cap and tuple(snaps[0]["grid"]) == st.grid and int(snaps[1]["nAtoms"].max()) == st.cap
    _compare(f"{name} {method} {halo} -a {overlap} step 0", snaps[0], run["s0"], 1, st.atoms)
    _compare(f"{name} {method} {halo} -a {overlap} step {st.first_over - 1}", snaps[1], run["sk"], 1, st.atoms)
    _same_cells(snaps[1], run["cellsk"], run["n_local"])
    _stopped(rc, lines, err, OVERFLOW % st.cap, ["created", "reached 0", "reached 1"])


# ================================================================ B. Verlet rows
# The lists are built at creation and again at the first step after which an atom has moved more than skin / 2 (skin = 0.1 cutoff) since the last build.  builds: the
# step of every build within `steps` and the longest row it makes -- the most neighbours within cutoff + skin of any atom (formats 0, 2, 4), and for LJ also the most
# of any atom in any one of the three groups of stencil cells of format 1 (nl_kernels.h groupCell).  Found by a search over -l and -r at 3000 K (the energy
# tolerances are absolute and were stated for states of a few hundred K) for a longest row that is a multiple of 8, the only lengths the rounded formats 1 and 4 can be
# given: EAM -l 3.45 .. 3.75 by 0.03 x -r 0.1, 0.2, 0.3 (7 of 33 states qualify); LJ -l 4.80 .. 6.20 by 0.05 x -r 0.1 .. 0.3 by 0.05, of which the state taken is the first
# whose full row also ends, dealt in bank order, with a pair inside the force cutoff (test_bank_order_puts_a_pair_inside_the_cutoff_into_the_last_entry).
RowState = namedtuple("RowState", "eam n lat delta temp steps grid atoms builds")
ROW_STATES = {
    "eam_rows": RowState(1, (6, 7, 8), 3.54, 0.2, 3000.0, 13, (3, 4, 5), 1344, {0: (64, None), 11: (64, None)}),
    "lj_rows":  RowState(0, (8, 9, 8), 5.05, 0.2, 3000.0, 23, (3, 3, 3), 2304, {0: (275, 128), 21: (277, 128)}),
}
NL_GROUP_SHARE = 0.62          # comd_device.hip AllocateGpu: the share of --maxNeighbors one group's rows get (NL_DIAGONAL)


def _longest(st, which):
    """the longest row any build of the state makes: per atom (which = 0) or per atom and group (1)"""
    return max(rows[which] for rows in st.builds.values())


def _rows_for(fmt, max_neighbors):
    """AllocateGpu: the entries of a row as the format derives them from --maxNeighbors"""
    if fmt in (0, 2):
        return max_neighbors
    if fmt == 4:
        return (max_neighbors + 7) // 8 * 8
    assert fmt == 1
    return (int(NL_GROUP_SHARE * max_neighbors) + 7) // 8 * 8


# leg: state, method, environment, list format, which of the state's two row lengths fills its rows, --maxNeighbors for FIT, --maxNeighbors for SHORT (the largest that
# gives the next smaller row)
RowLeg = namedtuple("RowLeg", "state env fmt which fit short")
ROW_LEGS = {
    "eam_format4_brick_rows": RowLeg("eam_rows", {}, 4, 0, 64, 56),
    "eam_format2_lds":        RowLeg("eam_rows", {"COMD_EAM_NL": "lds"}, 2, 0, 64, 63),
    "eam_format0_global":     RowLeg("eam_rows", {"COMD_NL_GLOBAL": "1"}, 0, 0, 64, 63),
    "lj_format0_global":      RowLeg("lj_rows", {"COMD_NL_GLOBAL": "1"}, 0, 0, 277, 276),
    "lj_format1_slabs":       RowLeg("lj_rows", {}, 1, 1, 208, 195),
    "lj_format1_bank_order":  RowLeg("lj_rows", {"COMD_NL_BANK_ORDER": "1"}, 1, 1, 208, 195),
}
_ROW_RUNS = {}


def _row_lengths(pos, extent, r_build, grid):
    """(neighbours within r_build per atom; the same per atom and group of format 1; the least | |r_ij| - r_build | over the pairs of the atoms whose rows are the
    longest or one shorter).  Group of a neighbour: (dx + dy + dz) mod 3 of the offset between its (image's) link cell and the atom's."""
    n = len(pos)
    size = extent / np.array(grid, dtype=np.float64)
    per_atom, per_group, gaps = np.zeros(n, dtype=np.int64), np.zeros((n, 3), dtype=np.int64), np.zeros(n)
    for s in range(0, n, 256):
        d = pos[s:s + 256, None, :] - pos[None, :, :]
        d -= np.rint(d / extent) * extent
        r2 = (d * d).sum(-1)
        hit = (r2 > 0.0) & (r2 <= r_build * r_build)
        per_atom[s:s + 256] = hit.sum(1)
        gaps[s:s + 256] = np.abs(np.sqrt(r2) - r_build).min(1)
        ii, jj = np.nonzero(hit)
        off = np.floor((pos[s + ii] - d[ii, jj]) / size).astype(np.int64) - np.floor(pos[s + ii] / size).astype(np.int64)
        assert np.abs(off).max() <= 1
        np.add.at(per_group, (s + ii, off.sum(1) % 3), 1)
    assert np.array_equal(per_group.sum(1), per_atom)
    return per_atom, per_group, gaps


def _row_run(orc, name):
    """The checker's run of a state: the steps at which the lists are built (displacement since the last build > skin / 2, as the drift kernels test it), the
    longest rows of every build counted in numpy from the checker's positions, the state at step 0 and after the steps."""
    if name in _ROW_RUNS:
        return _ROW_RUNS[name]
    st = ROW_STATES[name]
    o = orc.Oracle(st.n, eam=st.eam, temperature=st.temp, delta=st.delta, lat=st.lat)
    rc = orc.lib().oracle_cutoff(o.ptr)
    extent = np.array(st.n, dtype=np.float64) * orc.lib().oracle_lattice(o.ptr)
    skin = 0.1 * rc
    grid = tuple(int(x) for x in np.floor(extent / (rc + skin)))

    def build(t, r):
        per_atom, per_group, gaps = _row_lengths(r, extent, rc + skin, grid)
        top = per_group.max(1) if not st.eam else per_atom
        return dict(step=t, rows=(int(per_atom.max()), None if st.eam else int(per_group.max())),
                    margin=float(min(gaps[per_atom >= per_atom.max() - 1].min(), gaps[top >= top.max() - 1].min())))
    r_build = o.gather(orc.R)
    run = dict(st=st, grid=grid, rc=rc, s0=_snapshot(orc, o, st.eam), builds=[build(0, r_build)], closest=np.inf)
    for t in range(1, st.steps + 1):
        o.step(1)
        r = o.gather(orc.R)
        d = r - r_build
        d -= np.rint(d / extent) * extent
        moved = float(np.sqrt((d * d).sum(1).max()))
        run["closest"] = min(run["closest"], abs(moved - 0.5 * skin))
        if moved > 0.5 * skin:
            r_build = r
            run["builds"].append(build(t, r))
    run["sk"] = _snapshot(orc, o, st.eam)
    o.close()
    print(f"{name}: list grid {grid} builds {run['builds']} least |displacement - skin / 2| {run['closest']:.3e} A")
    _ROW_RUNS[name] = run
    return run


@pytest.mark.parametrize("name", list(ROW_STATES))
def test_row_states_are_what_is_recorded(orc, name):
    """The numpy row counts of every build are the recorded ones, the longest (per group for LJ) is a multiple of 8, at least one build comes after step 0,
    and neither a count nor the step of a build hangs on rounding: no pair of an atom with a longest row (or one entry less) lies within 1e-5 A of cutoff + skin (a float coordinate of this box is good to 4e-6 A), no
    step's largest displacement within 1e-4 A of skin / 2."""
    run = _row_run(orc, name)
    st = run["st"]
    assert run["grid"] == st.grid and min(st.grid) >= 3 and len(run["s0"]["r"]) == st.atoms
    assert {b["step"]: b["rows"] for b in run["builds"]} == st.builds and len(st.builds) >= 2
    assert min(b["margin"] for b in run["builds"]) > 1e-5 and run["closest"] > 1e-4
    assert _longest(st, 0 if st.eam else 1) % 8 == 0


def test_row_legs_fill_their_rows_exactly():
    """Every leg's --maxNeighbors gives, by AllocateGpu's rule for its format, rows of exactly the state's longest row; SHORT is the largest value that gives the next
    smaller row the format has."""
    for name, leg in ROW_LEGS.items():
        longest = _longest(ROW_STATES[leg.state], leg.which)
        step = 8 if leg.fmt in (1, 4) else 1
        assert _rows_for(leg.fmt, leg.fit) == longest, name
        assert _rows_for(leg.fmt, leg.short) == longest - step and _rows_for(leg.fmt, leg.short + 1) == longest, name


# nl_kernels.h groupCell, group 0: the stencil cells (dx, dy, dz) whose records a workgroup stages, in staging order
GROUP0_CELLS = [(-1, -1, -1), (-1, 0, 1), (-1, 1, 0), (0, -1, 1), (0, 0, 0), (0, 1, -1), (1, -1, 0), (1, 0, -1), (1, 1, 1)]


def test_bank_order_puts_a_pair_inside_the_cutoff_into_the_last_entry(orc):
    """What gives the COMD_NL_BANK_ORDER=1 FIT leg its teeth against `pos < nl.rows`: the one row of 128 entries (group 0 of one atom) is restated here as
    BuildNeighborListSlabs deals it -- records in staging order (the group's cells, each in slot = gid order), entry of record t in bank class 3 t mod 16, the classes
    dealt round-robin from class (slot mod 16) -- and the pair that lands in entry 127 lies inside the force cutoff.  A build that does not write that entry loses
    a pair that carries force."""
    run = _row_run(orc, "lj_rows")
    st = run["st"]
    pos, grid = run["s0"]["r"], np.array(st.grid)
    rc = run["rc"]
    extent = np.array(st.n, dtype=np.float64) * st.lat
    size = extent / grid
    cell = np.floor(pos / size).astype(np.int64)
    _, per_group, _ = _row_lengths(pos, extent, 1.1 * rc, st.grid)
    (atom, group), = np.argwhere(per_group == st.builds[0][1])
    assert group == 0
    members = lambda c: np.nonzero((cell == np.array(c) % grid).all(1))[0]          # ascending gid = slot order
    slot = int(np.nonzero(members(cell[atom]) == atom)[0][0])
    hits = []          # (bank class, inside the cutoff) of every hit, in record order
    t = 0
    for off in GROUP0_CELLS:
        for j in members(cell[atom] + np.array(off)):
            d = pos[atom] - pos[j]
            d -= np.rint(d / extent) * extent
            r2 = float((d * d).sum())
            if j != atom and r2 <= (1.1 * rc) ** 2:
                hits.append(((3 * t) & 15, r2 <= rc * rc))
            t += 1
    assert len(hits) == st.builds[0][1]
    cnt = np.bincount([c for c, _ in hits], minlength=16)
    s0, placed, where = slot & 15, np.zeros(16, dtype=np.int64), {}
    for c, inside in hits:
        m = placed[c]
        placed[c] += 1
        before = [1 if ((cc - s0) & 15) < ((c - s0) & 15) else 0 for cc in range(16)]
        where[m + sum(min(cnt[cc], m + before[cc]) for cc in range(16) if cc != c)] = inside
    assert sorted(where) == list(range(len(hits)))          # the dealing is a permutation of the row
    print(f"atom {atom} slot {slot}: {sum(where.values())} of {len(hits)} entries inside the cutoff; the last one: {where[len(hits) - 1]}")
    assert where[len(hits) - 1]


def _row_flags(leg, max_neighbors):
    st = ROW_STATES[leg.state]
    return _flags(st, "thread_atom_nl", 0, ["--maxNeighbors", max_neighbors] + (["--maxAtoms", 64] if st.eam else []))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROW_LEGS))
def test_rows_exactly_full(tmp_path, orc, name):
    """FIT: the longest row of the run fills its row to the last entry (lj_format0_global: at the second build, the others from the first on).  The format is the leg's, the row capacity in effect and the longest row each build
    wrote are what numpy counts; forces and energies agree with the checker at step 0 and after the state's steps, which include a second build."""
    leg = ROW_LEGS[name]
    run = _row_run(orc, leg.state)
    st = run["st"]
    longest = _longest(st, leg.which)
    rc, lines, err, snaps = _child(tmp_path, "rows", dict(flags=_row_flags(leg, leg.fit), steps=[0, st.steps]), leg.env)
    assert rc == 0 and len(snaps) == 2, (rc, err[-1500:])
    for k, (when, ref) in enumerate((("step 0", run["s0"]), (f"step {st.steps}", run["sk"]))):
        fmt, capacity, written, n_builds = (int(x) for x in snaps[k]["nl"])
        print(f"{name} {when}: format {fmt} row capacity {capacity} longest row {written} builds {n_builds}")
        assert tuple(snaps[k]["grid"]) == st.grid
        assert (fmt, capacity, written) == (leg.fmt, longest, list(st.builds.values())[0 if k == 0 else -1][leg.which])
        assert n_builds == (1 if k == 0 else len(st.builds))
        _compare(f"{name} {when}", snaps[k], ref, st.eam, st.atoms)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROW_LEGS))
def test_rows_one_length_short(tmp_path, orc, name):
    """SHORT: the next smaller row the format can be given.  The run ends in the force evaluation behind the first build that makes a longer row: the one inside
    the creation, or (lj_format0_global) the step() call of the second build, after the steps before it ran through."""
    leg = ROW_LEGS[name]
    st = _row_run(orc, leg.state)["st"]
    over = min(t for t, rows in st.builds.items() if rows[leg.which] > _rows_for(leg.fmt, leg.short))
    steps, reached = ([0], []) if over == 0 else ([0, over - 1, 1], ["created", "reached 0", "reached 1"])
    rc, lines, err, snaps = _child(tmp_path, "short", dict(flags=_row_flags(leg, leg.short), steps=steps), leg.env)
    _stopped(rc, lines, err, ROW_OVER % leg.short, reached)


# ================================================================ C. the halo's depth
# LJ on a lattice so wide (lat 20 A: nearest neighbours 14.1 A apart, cutoff 11.575 A) that every force is exactly 0: with all momenta 0 but one, a step moves one atom
# and nothing else, and its landing point is one product and one sum.  3 x 4 x 3 lattice cells, 5 x 6 x 5 link cells of 12 x 13.3 x 12 A; x sites at 5, 15, .. 55 A.
HaloState = namedtuple("HaloState", "eam n lat delta temp grid atoms")
HALO_STATE = HaloState(0, (3, 4, 3), 20.0, 0.0, 600.0, (5, 6, 5), 144)
HALO_CASES = {"plus_x_mirror": (+1, "mirror"), "plus_x_message": (+1, "message"), "minus_x_mirror": (-1, "mirror")}
_HALO = {}
# the GPU cases of this file (tests/test_single_precision.py runs them again in the float build and counts them): 4 LJ methods x 2 overlap modes, 2 EAM states x 2 methods x
# 2 halo paths x 2 overlap modes, FIT and SHORT of every row leg and of every halo case
GPU_CASE_COUNT = 4 * 2 + 2 * 2 * 2 * 2 + 2 * len(ROW_LEGS) + 2 * len(HALO_CASES)


def _exact(v):
    return Fraction(float(v))


def _round(frac):
    """a rational rounded to the nearest REAL: the nearest of float(frac) as a REAL and its two neighbours, measured exactly"""
    c = REAL(float(frac))
    return min((np.nextafter(c, REAL(-np.inf)), c, np.nextafter(c, REAL(np.inf))), key=lambda v: abs(_exact(v) - frac))


def _landing(x, p, inv_mass):
    """where AdvanceVelocityPosition puts a coordinate with force 0 and dt = 1: x + (1 * p) * invMass -- as written, and with the product fused into the sum (the
    compiler may contract it); the momentum is chosen so that the two agree"""
    plain = REAL(x) + REAL(REAL(p) * REAL(inv_mass))
    fused = _round(_exact(x) + _exact(p) * _exact(inv_mass))
    return REAL(plain), fused


def _halo_plan(orc, side):
    """The atom nearest the face, the far edge of the halo cell behind it as comdCoordInHalo decides it (floor((x - 0) * inv) in [-1, grid]), and two momenta: one
    that lands the atom 1 .. 8 ulps inside that edge, one that lands it 1 .. 8 ulps beyond."""
    if side in _HALO:
        return _HALO[side]
    st = HALO_STATE
    o = orc.Oracle(st.n, eam=0, temperature=st.temp, delta=st.delta, lat=st.lat)
    grid, n_local, _ = o.rank_grid(0)
    r0, f0 = o.gather(orc.R), o.gather(orc.F)
    mass = REAL(orc.lib().oracle_mass(o.ptr))
    o.close()
    assert tuple(grid) == st.grid and len(r0) == st.atoms and not f0.any()
    inv_mass = REAL(1.0) / mass
    length = REAL(st.n[0]) * REAL(st.lat)
    inv = REAL(1.0) / (length / REAL(grid[0]))
    gid = int(np.argmax(r0[:, 0]) if side > 0 else np.argmin(r0[:, 0]))
    x0 = REAL(r0[gid, 0])

    def inside(x):
        k = np.floor(np.float64(REAL(x) * inv))
        return -1 <= k <= grid[0]
    # the last coordinate inside, found from the nominal edge ((grid + 1) cells, or -1 cell) by single ulps
    edge = REAL(length + length / REAL(grid[0])) if side > 0 else REAL(-(length / REAL(grid[0])))
    out = REAL(np.inf * side)
    while inside(edge):
        edge = np.nextafter(edge, out)
    while not inside(edge):
        edge = np.nextafter(edge, -out)
    assert inside(edge) and not inside(np.nextafter(edge, out))
    ulp = abs(np.nextafter(edge, out) - edge)

    def momentum(lo, hi):
        """a momentum whose landing point lies lo .. hi ulps outward of `edge` (negative: inside), the same with and without contraction"""
        centre = REAL((edge + REAL(0.5 * (lo + hi)) * ulp * side - x0) / inv_mass)
        up, down = centre, centre
        for _ in range(256):          # the momenta around the aim, nearest first
            for p in (up, down):
                plain, fused = _landing(x0, p, inv_mass)
                if plain == fused and lo <= (np.float64(plain) - np.float64(edge)) * side / np.float64(ulp) <= hi:
                    return float(p), plain
            up, down = np.nextafter(up, REAL(np.inf)), np.nextafter(down, REAL(-np.inf))
        raise AssertionError("no momentum found")
    p_in, x_in = momentum(-8, -1)
    p_out, x_out = momentum(1, 8)
    assert inside(x_in) and not inside(x_out)
    wrapped = REAL(x_in - length * side)          # the image the halo exchange makes: one sum with the face's shift
    cell_x = int(np.floor(np.float64(wrapped * inv)))          # comdBoxFromCoord
    if wrapped < length and cell_x == grid[0]:
        cell_x = grid[0] - 1
    plan = dict(gid=gid, r0=r0, n_local=n_local, length=float(length), edge=float(edge), p_in=p_in, x_in=float(x_in), p_out=p_out, x_out=float(x_out),
                wrapped=float(wrapped), cell_x=cell_x, inv=float(inv))
    print(f"side {side:+d}: atom {gid} at x = {float(x0)!r}, last coordinate inside {float(edge)!r}; lands at {float(x_in)!r} -> {float(wrapped)!r} in cell column {plan['cell_x']} "
          f"(p = {p_in!r}); lost at {float(x_out)!r} (p = {p_out!r})")
    _HALO[side] = plan
    return plan


@pytest.mark.parametrize("side", [+1, -1])
def test_halo_landing_points(orc, side):
    """The two landing points straddle the edge of the halo by a few ulps, the inner one wraps into the cell column at the opposite face, and the checker, given
    the inner momentum, moves that atom to the same coordinate bit for bit and nothing else."""
    st = HALO_STATE
    plan = _halo_plan(orc, side)
    ulp = float(np.spacing(REAL(abs(plan["edge"]))))
    assert 0 < (plan["edge"] - plan["x_in"]) * side <= 8 * ulp and 0 < (plan["x_out"] - plan["edge"]) * side <= 8 * ulp
    assert plan["cell_x"] == (0 if side > 0 else st.grid[0] - 1)
    assert 0.0 <= plan["wrapped"] < plan["length"] and abs(plan["wrapped"] - (12.0 if side > 0 else 48.0)) < 1e-3
    o = orc.Oracle(st.n, eam=0, temperature=st.temp, delta=st.delta, lat=st.lat)
    p = np.zeros((st.atoms, 3))
    p[plan["gid"], 0] = plan["p_in"]
    o.scatter(orc.P, p)
    o.step(1)
    r = o.gather(orc.R)
    cells = o.rank_cells(0)
    o.close()
    expect = plan["r0"].copy()
    expect[plan["gid"], 0] = plan["wrapped"]
    assert np.array_equal(r, expect)
    b = [int(c) for c in range(plan["n_local"]) if plan["gid"] in cells["gid"][c, :cells["nAtoms"][c]]]
    assert len(b) == 1 and b[0] % st.grid[0] == plan["cell_x"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(HALO_CASES))
def test_atom_lands_just_inside_the_halo(tmp_path, orc, case):
    """FIT: one step carries the atom to 1 .. 8 ulps inside the far edge of the halo cell.  It is wrapped into the cell at the opposite face, its coordinate the numpy
    value bit for bit, every other atom where it was, the atom count unchanged."""
    side, path = HALO_CASES[case]
    st, plan = HALO_STATE, _halo_plan(orc, side)
    job = dict(flags=_flags(st, "thread_atom", 0), steps=[0, 1], momenta=dict(gid=plan["gid"], p=[plan["p_in"], 0.0, 0.0]))
    rc, lines, err, snaps = _child(tmp_path, "inside", job, HALO_PATHS[path])
    assert rc == 0 and len(snaps) == 2, (rc, err[-1500:])
    assert tuple(snaps[0]["grid"]) == st.grid and not snaps[0]["f"].any() and np.array_equal(snaps[0]["r"], plan["r0"])
    expect = plan["r0"].copy()
    expect[plan["gid"], 0] = plan["wrapped"]
    assert np.array_equal(snaps[1]["r"], expect), (snaps[1]["r"][plan["gid"]], expect[plan["gid"]])
    n_local = int(snaps[1]["n_local_boxes"])
    assert int(snaps[1]["n_global"]) == st.atoms == int(snaps[1]["nAtoms"][:n_local].sum())
    b = [c for c in range(n_local) if plan["gid"] in snaps[1]["gid"][c, :snaps[1]["nAtoms"][c]]]
    assert len(b) == 1 and b[0] % st.grid[0] == plan["cell_x"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(HALO_CASES))
def test_atom_lands_just_beyond_the_halo(tmp_path, orc, case):
    """SHORT: the same momentum a hair larger: the atom lands 1 .. 8 ulps beyond the halo and the run ends inside that step() call."""
    side, path = HALO_CASES[case]
    st, plan = HALO_STATE, _halo_plan(orc, side)
    job = dict(flags=_flags(st, "thread_atom", 0), steps=[0, 1], momenta=dict(gid=plan["gid"], p=[plan["p_out"], 0.0, 0.0]))
    rc, lines, err, snaps = _child(tmp_path, "beyond", job, HALO_PATHS[path])
    _stopped(rc, lines, err, LOST, ["created", "reached 0"])
