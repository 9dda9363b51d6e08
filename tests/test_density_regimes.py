"""Sparse, empty-cell and compressed states: every force method against the checker where cells are NOT evenly filled.

Every other GPU test starts from an FCC lattice at (or within 3 % of) the equilibrium lattice constant, so every kernel has been checked where all cells hold
about the same number of atoms and none is empty.  The states here are made with the three knobs the command line and the checker share -- -l (lat) stretches
or compresses the lattice, -r (delta) disorders it, -T heats it -- and reach, through a state that needs them, the legs the other tests only force through
COMD_* switches: LJ tail waves of a few atoms and cells of six waves, empty cells and cells that flip between empty and occupied, a 16-slot EAM capacity,
EAM rows at the most the kernel holds and still shorter than the neighbour count of half the atoms.

  1. CPU: the checker itself against an all-pairs minimum-image sum in numpy that walks no cells (it has only been pinned at lattice density).
  2. CPU: how far the checker moves when every coordinate moves by one ulp, and the one tolerance that has to follow it (dF/drho, see
     tests/golden/reference_values.json "tolerances_density_regimes").
  3. GPU: every method in every regime against the checker, at step 0 and after the regime's steps, with the fact that makes the state worth running.
  4. GPU: the cells' contents after the hot sparse runs, bit for bit.
  5. GPU: the mirrored halo path against the message path, bit for bit (a child process per mode).
"""
import ctypes
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import test_kernel_legs as legs
from test_pressure import EPS, SIGMA, _interpolate, _pairs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = json.load(open(os.path.join(HERE, "golden", "reference_values.json")))
TOL = G["tolerances"]
TOL_REGIME = G["tolerances_density_regimes"]

# grid, atoms, occupancy (lowest, highest), empty cells and neighbours per atom (fewest, most) are the checker's own figures at step 0; every test takes them
# again from the checker (_reference) before it compares anything.  LJ: the default cutoff of 5 sigma = 11.575 A; EAM: Cu_u6.eam, cutoff 4.95 A.
Regime = namedtuple("Regime", "eam n lat delta temp steps grid atoms occ empty nbr")
REGIMES = {
    "lj_void":    Regime(0, (3, 4, 3),    17.0, 0.1, 600.0,   30, (4, 5, 4), 144,  (0, 4),     5,  (0, 0)),         # no pair within the cutoff: forces and energies are 0
    "lj_sparse":  Regime(0, (4, 3, 5),    16.5, 2.0, 20000.0, 30, (5, 4, 7), 240,  (0, 4),     8,  (2, 8)),         # cells flip between empty and occupied
    "lj_dilute":  Regime(0, (5, 5, 6),    8.0,  0.1, 600.0,   5,  (3, 3, 4), 600,  (13, 24),   0,  (54, 54)),       # a cell is one tail wave of <= 32 atoms
    "lj_dense":   Regime(0, (12, 13, 14), 2.9,  0.1, 600.0,   5,  (3, 3, 3), 8736, (288, 360), 0,  (1042, 1060)),   # 6 waves per cell
    "eam_void":   Regime(1, (4, 5, 4),    7.1,  0.1, 20000.0, 30, (5, 7, 5), 320,  (0, 4),     8,  (0, 6)),         # 20 atoms with no neighbour: rhobar = 0
    "eam_sparse": Regime(1, (4, 5, 6),    7.0,  0.5, 20000.0, 30, (5, 7, 8), 480,  (0, 4),     17, (2, 10)),        # peak occupancy 5 in cells of 16 slots
    "eam_dilute": Regime(1, (5, 6, 5),    5.2,  0.1, 600.0,   5,  (5, 6, 5), 600,  (4, 4),     0,  (12, 12)),       # the lattice maximum: 4 atoms per cell
    "eam_dense":  Regime(1, (7, 8, 9),    2.6,  0.1, 600.0,   5,  (3, 4, 4), 2016, (34, 48),   0,  (116, 134)),     # rhobar up to 0.208 of a table that ends at 0.2505
}
HOT = ("lj_void", "lj_sparse", "eam_void", "eam_sparse")            # 30 steps; the others 5
OVERLAP_TOO = HOT + ("lj_dense", "eam_dense")                       # run with -a 1 as well
SPARSE = ("lj_sparse", "eam_sparse")
# the checker's 30 steps of the sparse states: atoms that changed cell, cells that changed between empty and occupied (counted step by step), peak occupancy
SPARSE_RUN = {"lj_sparse": (25, 7, 4), "eam_sparse": (136, 29, 5)}
METHODS = {0: ["thread_atom", "cta_cell", "thread_atom_nl", "cta_cell -L"], 1: ["thread_atom", "cta_cell", "thread_atom_nl"]}
EAM_REGIMES = [name for name, g in REGIMES.items() if g.eam]


def _extent(g):
    return np.array(g.n, dtype=np.float64) * g.lat


def _make(orc, g):
    return orc.Oracle(g.n, eam=g.eam, temperature=g.temp, delta=g.delta, lat=g.lat)


def _snapshot(orc, o, eam):
    ep, ek = o.energy()
    got = {"r": o.gather(orc.R), "f": o.gather(orc.F), "u": o.gather(orc.U), "ep": ep, "ek": ek}
    if eam:
        got.update(rho=o.gather(orc.RHOBAR), df=o.gather(orc.DFEMBED))
    for v in got.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return got


def _eam_tables(orc, o):
    """(x0, invDx, padded samples) of phi, rho and F as the checker holds them"""
    L, out = orc.lib(), []
    for which in range(3):
        n, x0, inv = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        assert L.oracle_eam_table(o.ptr, which, ctypes.byref(n), ctypes.byref(x0), ctypes.byref(inv), None) == 0
        v = np.empty(n.value + 3)
        L.oracle_eam_table(o.ptr, which, ctypes.byref(n), ctypes.byref(x0), ctypes.byref(inv), v.ctypes.data_as(ctypes.c_void_p))
        out.append((x0.value, inv.value, v))
    return out


def _neighbour_counts(pos, extent, rc):
    i = _pairs(pos, extent, rc)[0]
    return np.bincount(i, minlength=len(pos))


def _face_distance(pos, extent, grid):
    """the least distance of any coordinate from a face of its cell"""
    size = extent / np.array(grid, dtype=np.float64)
    t = pos / size
    t = t - np.floor(t)
    return float((np.minimum(t, 1.0 - t) * size).min())


# ---------------------------------------------------------------- the checker's answer, once per regime
_REFERENCE = {}


def _reference(orc, name):
    """The checker's run of a regime: the figures of the state at step 0 (asserted: the regime is what its name says), the state at step 0 and after the
    regime's steps, the cells after the steps, and how often cells changed between empty and occupied on the way.  Computed once, read-only."""
    if name in _REFERENCE:
        return _REFERENCE[name]
    g = REGIMES[name]
    o = _make(orc, g)
    grid, n_local, n_total = o.rank_grid(0)
    occ = o.rank_cells(0)["nAtoms"][:n_local].copy()
    rc = orc.lib().oracle_cutoff(o.ptr)
    s0 = _snapshot(orc, o, g.eam)
    nbr = _neighbour_counts(s0["r"], _extent(g), rc)
    print(f"{name}: grid {grid} atoms {o.n_global} occupancy {occ.min()}-{occ.max()} empty {int((occ == 0).sum())} neighbours {nbr.min()}-{nbr.max()} "
          f"(none: {int((nbr == 0).sum())}) max|f| {np.abs(s0['f']).max():.3e}")
    assert min(grid) >= 3, grid
    assert (tuple(grid), o.n_global, (int(occ.min()), int(occ.max())), int((occ == 0).sum()), (int(nbr.min()), int(nbr.max()))) \
        == (g.grid, g.atoms, g.occ, g.empty, g.nbr), name
    assert g.steps == (30 if name in HOT else 5)
    tables = _eam_tables(orc, o) if g.eam else None
    # one step at a time (oracle_step loops over the same five phases): cells that change between empty and occupied, atoms that change cell
    flips, moves, peak = 0, 0, int(occ.max())
    cells = o.rank_cells(0)
    home = {int(gid): b for b in range(n_local) for gid in cells["gid"][b, :cells["nAtoms"][b]]}
    for _ in range(g.steps):
        o.step(1)
        cells = o.rank_cells(0)
        now = cells["nAtoms"][:n_local]
        flips += int(((now == 0) != (occ == 0)).sum())
        occ = now.copy()
        peak = max(peak, int(occ.max()))
        here = {int(gid): b for b in range(n_local) for gid in cells["gid"][b, :cells["nAtoms"][b]]}
        moves += sum(1 for gid, b in here.items() if home[gid] != b)
        home = here
    sk = _snapshot(orc, o, g.eam)
    for v in cells.values():
        v.setflags(write=False)
    print(f"{name}: after {g.steps} steps: {moves} cell changes, {flips} changes between empty and occupied, peak occupancy {peak}, "
          f"least distance from a cell face {_face_distance(sk['r'], _extent(g), grid):.3e} A")
    assert peak <= o.cap
    o.close()
    _REFERENCE[name] = dict(g=g, grid=tuple(grid), n_local=n_local, n_total=n_total, rc=rc, s0=s0, sk=sk, cells=cells, flips=flips, moves=moves, peak=peak, nbr=nbr,
                            tables=tables)
    return _REFERENCE[name]


# ---------------------------------------------------------------- 1. CPU: the checker against all pairs
def _row_sums(i, values, n):
    """sum of values over the rows of equal i (i ascending), in the precision of values; 0 for an i that does not occur"""
    start = np.searchsorted(i, np.arange(n))
    count = np.bincount(i, minlength=n)
    out = np.zeros((n,) + values.shape[1:], dtype=values.dtype)
    if len(i):
        sums = np.add.reduceat(values, np.minimum(start, len(i) - 1), axis=0)
        out[count > 0] = sums[count > 0]
    return out


def _lj_all_pairs(pos, extent, rc):
    """ljForce.c:146-265 in np.longdouble over all pairs under the minimum image: forces, per-atom energies"""
    ld = np.longdouble
    i, j, _, _ = _pairs(pos, extent, rc)
    assert np.all(np.diff(i) >= 0)
    p, ext = pos.astype(ld), extent.astype(ld)
    d = p[i] - p[j]
    d -= np.rint(d / ext) * ext
    r2 = (d * d).sum(-1)
    s6 = ld(SIGMA) ** 6
    rc6 = s6 / (ld(rc) * ld(rc)) ** 3
    r6 = s6 / (r2 * r2 * r2)
    e = ld(0.5) * ld(4.0) * ld(EPS) * (r6 * (r6 - 1) - rc6 * (rc6 - 1))
    fr = ld(EPS) * r6 / r2 * (48 * r6 - 24)
    n = len(pos)
    return _row_sums(i, fr[:, None] * d, n), _row_sums(i, e, n)


def _eam_all_pairs(pos, extent, rc, tables):
    """eam.c:266-419 on the checker's tables by the quadratic evaluation tests/test_pressure.py restates: forces, per-atom energies, rhobar, dF/drho"""
    i, j, d, r = _pairs(pos, extent, rc)
    n = len(pos)
    phi, dphi = _interpolate(*tables[0], r)
    rho, drho = _interpolate(*tables[1], r)
    rhobar = np.bincount(i, rho, minlength=n)
    emb, demb = _interpolate(*tables[2], rhobar)
    pair = (dphi + (demb[i] + demb[j]) * drho) / r
    f = np.stack([np.bincount(i, -pair * d[:, c], minlength=n) for c in range(3)], axis=1)
    return f, 0.5 * np.bincount(i, phi, minlength=n) + emb, rhobar, demb


@pytest.mark.parametrize("name", list(REGIMES))
def test_checker_matches_all_pairs(orc, name):
    """Step-0 forces, per-atom energies and (EAM) rhobar of the checker against a sum over all pairs that walks no cells: 1e-12 of max|f|, 1e-12 eV (the
    LJ regimes measured <= 1.3e-14 of max|f|, <= 1.5e-13 eV at e = 17 eV, U/N <= 3e-15 eV).  EAM: rhobar stays below the end of the F table."""
    ref = _reference(orc, name)
    g, s0 = ref["g"], ref["s0"]
    if g.eam:
        x0, inv, v = ref["tables"][2]
        xn = x0 + (len(v) - 3) / inv
        assert max(s0["rho"].max(), ref["sk"]["rho"].max()) < xn, (s0["rho"].max(), ref["sk"]["rho"].max(), xn)
        f, u, rho, df = _eam_all_pairs(s0["r"], _extent(g), ref["rc"], ref["tables"])
        assert np.abs(rho - s0["rho"]).max() <= 1e-12, np.abs(rho - s0["rho"]).max()
    else:
        f, u = _lj_all_pairs(s0["r"], _extent(g), ref["rc"])
    fmax = np.abs(s0["f"]).max()
    err_f, err_u, err_total = float(np.abs(f - s0["f"]).max()), float(np.abs(u - s0["u"]).max()), float(abs(u.sum() - s0["ep"])) / g.atoms
    print(f"{name}: max|df| {err_f:.3e} (max|f| {fmax:.3e})  max|de| {err_u:.3e} (max|e| {np.abs(s0['u']).max():.3e})  |dU|/N {err_total:.3e}")
    if name == "lj_void":
        assert fmax == 0.0 and not s0["u"].any() and s0["ep"] == 0.0
    assert err_f <= 1e-12 * fmax and err_u <= 1e-12 and err_total <= 1e-12


def test_no_atom_of_a_sparse_run_ends_near_a_cell_face(orc):
    """The cell contents of section 4 are compared exactly: an atom whose coordinate lay within rounding of a cell face could sit on either side of it.  None
    ends within 1e-6 A of a face (the nearest measured: 3e-3 A), so no atom is excluded there.  The runs do what they are for: cells change between empty and
    occupied on the way, into which the halo paths then append."""
    for name in SPARSE:
        ref = _reference(orc, name)
        assert _face_distance(ref["sk"]["r"], _extent(ref["g"]), ref["grid"]) > 1e-6
        assert (ref["moves"], ref["flips"], ref["peak"]) == SPARSE_RUN[name]


# ---------------------------------------------------------------- 2. CPU: what one ulp does to the checker
def _distances(a, b, eam, n):
    fmax = np.abs(a["f"]).max()
    d = {"force_rel_to_max": float(np.abs(a["f"] - b["f"]).max() / fmax) if fmax > 0 else float(np.abs(b["f"]).max()),
         "per_atom_energy_abs": float(np.abs(a["u"] - b["u"]).max()), "energy_per_atom": abs((a["ep"] + a["ek"]) - (b["ep"] + b["ek"])) / n}
    if eam:
        d.update(eam_density_abs=float(np.abs(a["rho"] - b["rho"]).max()), eam_dfembed_abs=float(np.abs(a["df"] - b["df"]).max()))
    return d


@pytest.mark.parametrize("name", list(REGIMES))
def test_checker_moves_less_than_the_tolerances_when_positions_move_one_ulp(orc, name):
    """The checker as created against the checker after every coordinate moved by one ulp in a seeded random direction, at step 0 and after the regime's steps.
    Forces, per-atom energies, rhobar and E/N move by less than a tenth of the project's tolerances, which therefore hold unchanged in these regimes.  dF/drho does
    not: F'' is steep near rhobar = 0 (|F'| is about 500 there), so a correct implementation misses 1e-12 in the sparse EAM states.  Its tolerance is recorded per
    regime in tolerances_density_regimes by the rule stated there, and every recorded value must lie within [4x, 8x] of the distance measured here (1e-12 where
    4x is below it)."""
    ref = _reference(orc, name)
    g = ref["g"]
    o = _make(orc, g)
    r = o.gather(orc.R)
    assert np.array_equal(r, ref["s0"]["r"])
    up = np.random.RandomState(20261019).randint(0, 2, size=r.shape).astype(bool)
    o.scatter(orc.R, np.where(up, np.nextafter(r, np.inf), np.nextafter(r, -np.inf)))
    o.redistribute()
    o.compute_force()
    o.kinetic_energy()
    d0 = _distances(ref["s0"], _snapshot(orc, o, g.eam), g.eam, g.atoms)
    o.step(g.steps)
    dk = _distances(ref["sk"], _snapshot(orc, o, g.eam), g.eam, g.atoms)
    o.close()
    print(f"{name}: step 0 " + "  ".join(f"{k} {v:.2e}" for k, v in d0.items()))
    print(f"{name}: step {g.steps} " + "  ".join(f"{k} {v:.2e}" for k, v in dk.items()))
    assert d0["force_rel_to_max"] <= 0.1 * TOL["force_rel_to_max"] and dk["force_rel_to_max"] <= 0.1 * 1e-9
    for d in (d0, dk):
        assert d["per_atom_energy_abs"] <= 0.1 * TOL["per_atom_energy_abs"] and d["energy_per_atom"] <= 0.1 * TOL["energy_per_atom_trace"], d
        if g.eam:
            assert d["eam_density_abs"] <= 0.1 * TOL["eam_density_abs"], d
    if g.eam:
        dist, recorded = max(d0["eam_dfembed_abs"], dk["eam_dfembed_abs"]), TOL_REGIME[name]["eam_dfembed_abs"]
        if 4.0 * dist < TOL["eam_dfembed_abs"]:
            assert recorded == TOL["eam_dfembed_abs"], (dist, recorded)
        else:
            assert 4.0 * dist <= recorded <= 8.0 * dist, (dist, recorded)
    else:
        assert name not in TOL_REGIME


def test_recorded_tolerances_name_the_eam_regimes():
    assert set(TOL_REGIME) - {"_about"} == set(EAM_REGIMES)
    assert all(set(TOL_REGIME[name]) == {"eam_dfembed_abs"} for name in EAM_REGIMES)


# ---------------------------------------------------------------- 3. GPU: every method in every regime
def _flags(g, method, overlap):
    m = method.split()
    return ["-x", g.n[0], "-y", g.n[1], "-z", g.n[2], "-l", g.lat, "-r", g.delta, "-T", g.temp, "-m", m[0], "-a", overlap] + (["-e"] if g.eam else []) + m[1:]


def _compare(sim, name, ref, snap, force_tol, when):
    """forces, per-atom energies, (EAM) rhobar and dF/drho, U/N, K/N, E/N and the atom count of `sim` against the checker's state `snap`"""
    g = ref["g"]
    f, u = sim.gather(2), sim.gather(3)
    ep, ek, ng = sim.energy()
    fmax = np.abs(snap["f"]).max()
    err = {"f": float(np.abs(f - snap["f"]).max()), "u": float(np.abs(u - snap["u"]).max()), "U/N": abs(ep - snap["ep"]) / ng, "K/N": abs(ek - snap["ek"]) / ng,
           "E/N": abs((ep + ek) - (snap["ep"] + snap["ek"])) / ng}
    if g.eam:
        err.update(rho=float(np.abs(sim.gather(4) - snap["rho"]).max()), df=float(np.abs(sim.gather(5) - snap["df"]).max()))
    print(f"{name} {when}: max|f| {fmax:.3e}  " + "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert ng == g.atoms == sim.n_global
    if name == "lj_void":
        assert fmax == 0.0 and not f.any() and not u.any() and ep == 0.0, err
    assert err["f"] <= force_tol * fmax, err                        # no floor of 1 eV/A: max|f| is 5e-4 eV/A in lj_sparse
    assert err["u"] <= TOL["per_atom_energy_abs"], err
    assert err["U/N"] <= TOL["energy_per_atom_step0"] and err["K/N"] <= TOL["kinetic_per_atom"] and err["E/N"] <= TOL["energy_per_atom_trace"], err
    if g.eam:
        assert err["rho"] <= TOL["eam_density_abs"] and err["df"] <= TOL_REGIME[name]["eam_dfembed_abs"], err


def _fact(sim, name, ref, method):
    """what makes the state worth running, from the launch wrappers' report of one more evaluation and from the run's own occupancies"""
    g = ref["g"]
    c = legs.observe(sim, {"n": g.n, "flags": ["-l", g.lat]})
    rep, occ = c.rep, c.counts[:sim.n_local_boxes]
    assert int(occ.sum()) == g.atoms
    if method == "thread_atom" and not g.eam:
        if name == "lj_dense":
            assert rep["lj_waves_per_cell"] > 4 and occ.max() > 4 * 64, (rep, occ.max())
        if name in ("lj_void", "lj_sparse", "lj_dilute"):
            assert rep["lj_waves_per_cell"] == 1 and occ.max() <= 32, (rep, occ.max())
        if name in ("lj_void", "lj_sparse"):
            assert (occ == 0).any()
    if name == "eam_dense" and method == "thread_atom":
        # rows follow the density (eam_launch.h eamRowsPerAtom: the cutoff sphere at the lattice constant given, + 50 %) up to the 128 the kernel holds: at -l 2.6 that limit
        # is reached and the atoms of 129-134 neighbours overflow their rows beside atoms of 116-128 that do not, inside one launch
        assert rep["eam_kernel"] == "atom_brick", rep
        legs.rows_capacity(128, 0.1, 0.9)(c)
    if name == "eam_dense" and method == "cta_cell":
        assert rep["eam_kernel"] == "brick" and rep["eam_row_capacity"] >= c.neighbour_counts().max() > 128, rep      # (up to 256 here: no row overflows)
    if name in ("eam_void", "eam_sparse", "eam_dilute") and method != "thread_atom_nl":
        assert sim.max_atoms == 16                                   # the lattice maximum of 4: fewer slots than a wave has lanes


# -L sizes the link cells to cutoff + skin (12.73 A), which leaves the lj_dense box 2 x 2 x 3 cells of 728 atoms: more than the 512 a cta_cell workgroup holds (256
# threads of two atoms).  The launch wrapper refuses that capacity and ends the process, so this one pair runs in a child and must be refused, below.
REFUSED = ("lj_dense", "cta_cell -L")


def _cases():
    out = []
    for name, g in REGIMES.items():
        for method in METHODS[g.eam]:
            if (name, method) == REFUSED:
                continue
            for overlap in (0, 1) if name in OVERLAP_TOO else (0,):
                out.append(pytest.param(name, method, overlap, id=f"{name}-{method.replace(' -', '_')}-a{overlap}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,method,overlap", _cases())
def test_every_method_matches_the_checker(gpu, orc, name, method, overlap):
    """Default capacity (chooseMaxAtoms is part of what runs).  Step 0: forces to TOL force_rel_to_max of the checker's max|f|; after the steps (30 for the hot
    states, 5 for the others): 1e-9 of it.  Energies, rhobar, U/N, K/N, E/N: the project's tolerances; dF/drho: the regime's recorded one."""
    ref = _reference(orc, name)
    g = ref["g"]
    with gpu.Simulation(_flags(g, method, overlap)) as sim:
        assert "_nl" in method or "-L" in method or sim.grid == g.grid, sim.grid
        _compare(sim, name, ref, ref["s0"], TOL["force_rel_to_max"], "step 0")
        sim.step(g.steps)
        sim.sum_atoms()
        _compare(sim, name, ref, ref["sk"], 1e-9, f"step {g.steps}")
        _fact(sim, name, ref, method)


@pytest.mark.gpu
def test_pairlist_cells_of_more_than_512_atoms_are_refused(tmp_path):
    """lj_dense with cta_cell -L: cells of 728 atoms.  The run must end with the wrapper's message and write no result, not compute with half of a cell."""
    name, method = REFUSED
    out = tmp_path / "refused.npz"
    proc = subprocess.run([sys.executable, os.path.join(HERE, "density_worker.py"), json.dumps(_flags(REGIMES[name], method, 0)), "0", str(out)], cwd=ROOT,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode != 0 and "cta_cell supports at most 512 atoms per cell" in proc.stderr and not out.exists(), proc.stdout[-1500:] + proc.stderr[-1500:]


# ---------------------------------------------------------------- 4. GPU: the cells after the hot sparse runs
@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("method", ["thread_atom", "cta_cell"])
@pytest.mark.parametrize("name", SPARSE)
def test_cells_hold_the_checkers_atoms_after_a_sparse_run(gpu, orc, name, method, overlap):
    """After 30 steps in which cells emptied and filled: equal occupancies, every local cell holds exactly the checker's gids in ascending order, halo cells
    are sorted.  Exact, with no atom excluded: none ends within 1e-6 A of a cell face (asserted on the checker's positions)."""
    ref = _reference(orc, name)
    g, oc = ref["g"], ref["cells"]
    assert _face_distance(ref["sk"]["r"], _extent(g), ref["grid"]) > 1e-6
    with gpu.Simulation(_flags(g, method, overlap)) as sim:
        sim.step(g.steps)
        c = sim.cells()
        assert (sim.grid, sim.n_local_boxes, sim.n_total_boxes) == (ref["grid"], ref["n_local"], ref["n_total"])
    assert np.array_equal(c["nAtoms"], oc["nAtoms"])
    assert int(c["nAtoms"][:ref["n_local"]].sum()) == g.atoms and int((c["nAtoms"][:ref["n_local"]] == 0).sum()) > 0
    for b in range(ref["n_total"]):
        k = c["nAtoms"][b]
        assert np.all(np.diff(c["gid"][b, :k]) > 0), b
        if b < ref["n_local"]:
            assert np.array_equal(c["gid"][b, :k], oc["gid"][b, :k]), b


# ---------------------------------------------------------------- 5. GPU: mirrored halo against the message path
@pytest.mark.gpu
@pytest.mark.parametrize("name,method", [("lj_sparse", "thread_atom"), ("eam_sparse", "cta_cell")])
def test_mirrored_halo_is_the_message_halo_bit_for_bit(tmp_path, name, method):
    """COMD_HALO_MIRROR=1 (halo cells filled straight from the cells they are images of, MirrorAtomCells appending into cells that were empty) against =0 (pack,
    message, unpack) on a run whose cells flip between empty and occupied: the same nAtoms, gid, r, p, f in every cell, local and halo, and the same energies."""
    g = REGIMES[name]
    procs = []
    for mode in ("1", "0"):
        out = str(tmp_path / f"mirror{mode}.npz")
        procs.append((out, subprocess.Popen([sys.executable, os.path.join(HERE, "density_worker.py"), json.dumps(_flags(g, method, 0)), str(g.steps), out], cwd=ROOT,
                                            env=dict(os.environ, COMD_HALO_MIRROR=mode), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    got = []
    for out, proc in procs:
        text = proc.communicate(timeout=300)[0]
        assert proc.returncode == 0, text[-3000:]
        got.append(np.load(out))
    a, b = got
    assert int(a["n_global"]) == g.atoms and np.array_equal(a["nAtoms"], b["nAtoms"])
    assert int(a["nAtoms"][:int(a["n_local_boxes"])].sum()) == g.atoms and int(a["nAtoms"][int(a["n_local_boxes"]):].sum()) > 0
    held = np.arange(a["gid"].shape[1])[None, :] < a["nAtoms"][:, None]
    for key in ("gid", "rx", "ry", "rz", "px", "py", "pz", "fx", "fy", "fz", "e"):
        assert np.array_equal(a[key][held], b[key][held]), key
    assert np.array_equal(a["energy"], b["energy"])
