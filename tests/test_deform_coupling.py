"""What else lives on a deforming box (tests/test_deform.py pins energies, forces and the virial on it): the integrator step with the remap in it, the
displacement records, the analyses (g(r), centro-symmetry and coordination, common neighbour analysis), the executable's g(r) normalisation, and the
paths no strained step had gone through (cta_cell -L, the message halo of a self-neighbour rank, -a 1 and -H under a rate, COMD_NL_DEFERRED=1).

The references are the numpy restatements of the modules that test these features on the fixed box (test_langevin, test_msd, test_rdf, test_csp,
test_cna), imported, with sim.box as the extent; their comparison rules and caps are applied as they stand.  Shapes are test_deform.py's: LJ25 (8^3,
2048 atoms, 2.5 sigma) and EAM_BOX (10 x 8 x 6, 1920 atoms): the smallest boxes with 3+ cells per axis and unequal axes.

COMD_PRECISION=single runs the module on the float build, as test_msd.py: SINGLE, EPS and the "tolerances_single" of golden/reference_values.json.

Largest figures observed on an MI355X when the module was written, double | float build, beside their bounds (none of which was fitted to them):
    strained step, r after the minimum image          3.6e-15 A   (1e-12 max|r| = 2.8e-11)   | 6.4e-6 A  (position_abs 1e-5)
    strained step, p relative                         2.3e-16     (1e-12)                    | 8.7e-8    (force_rel_to_max 1e-4)
    strained step, r without the remap (control)      0.17 to 0.21 A
    displacements() against the incremental sum       1.2e-9 A    (tol_strained 4.7e-9)      | 2.4e-5 A  (2.9e-4 to 3.6e-4)
    0 K lattice: bound on one drift                   5.9e-16 A   (2^-33 = 1.2e-10)          | 1.5e-7 A: the premise fails, the records are held to the summed bound
    two ranks: positions, displacements               2.5e-14, 0 A (3.1e-8, 4.5e-8)          | 1.7e-5, 1.5e-5 A (0.31); 8 atoms changed rank
    pair histogram: near-edge pairs, |cum difference| 0, 0        (cap 0)                    | 103 to 173, 0  (cap 0.5 % = 202 to 403)
    csp: atoms left out, largest difference           0 / 0, 7.6e-15 A^2 (1e-10 + 1e-12 csp) | 0 / 0, 2.6e-6 A^2 (5e-3 + 1e-5 csp)
    CNA: atoms left out, wrong types                  0, 0        (cap 0)                    | 5 in the narrowest LJ box, else 0; 0 wrong  (cap 0.5 % = 10)
    ranks against one rank: csp                       2.7e-14 A^2 (1e-10 + 1e-12 csp)        | 1.4e-5 A^2 (5e-3 + 1e-5 csp); counts, coordination, types equal
    comd-hip: header V against N / mean(N / V_k)      0 relative  (1e-12); against the final V it would be 2.0e-2
    cta_cell -L: list builds free / -2 / +2 per ps    2 / 3 / 2;  forces 7.5e-16 of max|f| (1e-11) | 2 / 3 / 2; 1.1e-6 (1e-4)
    COMD_NL_DEFERRED 0 / 1 at -2 per ps               3 / 3 builds (LJ and Adams), states equal to the bit
    -a 1 against -a 0                                 equal to the bit;  -H: r 3.6e-15 A (1e-10), f 2.1e-14 (1e-9), E/N 4.7e-16 (2e-12) | 3.8e-6 (1e-4), 1.1e-5 (1e-2), 4.9e-7 (5e-5)
"""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import test_cna as cna
import test_csp as csp
import test_langevin as lv
import test_msd as msd
import test_rdf as rdf
from test_deform import DISORDER, EAM_BOX, HOT, LJ25, SCALE
from test_msd import EPS, Q, SINGLE
from test_pressure import ADAMS, CSRC, HERE, MISHIN, ROOT, TOL, _child, _rel

KB = lv.KB
SEED = lv.SEED
DELTA = rdf.DELTA32 if SINGLE else rdf.DELTA64
POTS = {"lj": LJ25, "adams": EAM_BOX + ADAMS, "mishin": EAM_BOX + MISHIN}
# centro_symmetry's r_coord, passed explicitly: the default (1/sqrt 2 + 1) lat / 2 is tied to the lattice constant, not to the strained shells.  3.1 A lies above
# the first shell (2.3 to 2.7 A over all states) and below the second of states (a)-(c) and of the narrowest EAM box (>= 3.47 A); in the narrowest LJ box (20 %
# shorter along x) it also takes in the two second-shell atoms along x at 2.89 A.  The value is one a float holds exactly, so both builds count with the same radius.
R_COORD = float(np.float32(3.1))
BINS = 64


def _r(x):
    """a value as the build under test holds it"""
    return float(np.float32(x)) if SINGLE else float(x)


# ================================================================ CPU
def test_generalised_helpers_give_the_cube_what_they_gave_before(pkg):
    """_distances / _reference (test_rdf), _numpy_csp, _numpy_cna, _wrap and _incremental's arithmetic take three extents now: for a cube, given as a scalar
    and as three equal extents, they return the same bits, and the scalar form is the expression of before, restated here."""
    n = 6
    L = n * rdf.LAT
    pos = csp._host_positions(pkg, rdf._cube(n) + ["-r", 0.1] + ADAMS)
    rc = 4.95
    a, b = rdf._distances(pos, L, rc), rdf._distances(pos, (L, L, L), rc)
    before = []
    for s in range(0, len(pos), 256):
        d = pos[s:s + 256, None, :] - pos[None, :, :]
        d -= np.rint(d / L) * L
        r2 = (d * d).sum(-1)
        before.append(np.sqrt(r2[(r2 > 0.0) & (r2 < rc * rc)]))
    assert len(a) > 0 and np.array_equal(a, b) and np.array_equal(a, np.sort(np.concatenate(before)))
    edges = np.arange(49) * (rc / 48)
    c0, n0 = rdf._reference(object(), pos, L, edges, rdf.DELTA64)
    c1, n1 = rdf._reference(object(), pos, np.array([L, L, L]), edges, rdf.DELTA64)
    assert np.array_equal(c0, c1) and np.array_equal(n0, n1) and c0[-1] == len(a) // 2
    x, y = csp._numpy_csp(pos, L, rc, csp.R_COORD, csp.DELTA64), csp._numpy_csp(pos, (L, L, L), rc, csp.R_COORD, csp.DELTA64)
    assert all(np.array_equal(x[k], y[k]) for k in x)
    x, y = cna._numpy_cna(pos, L, rc, cna.DELTA64), cna._numpy_cna(pos, (L, L, L), rc, cna.DELTA64)
    assert all(np.array_equal(x[k], y[k]) for k in x)
    rng = np.random.default_rng(3)
    v = rng.uniform(-2 * L, 2 * L, (500, 3))
    for wrap in (msd._wrap, lv._wrap):
        assert np.array_equal(wrap(v, L), v - np.rint(v / L) * L) and np.array_equal(wrap(v, L), wrap(v, np.array([L, L, L])))


class _FakeSim:
    """positions handed out step by step, for _incremental's arithmetic without a device"""

    def __init__(self, frames, boxes):
        self.frames, self.boxes, self.k = frames, boxes, 0

    def gather(self, which):
        return self.frames[self.k]

    def step(self, n):
        self.k += n

    @property
    def box(self):
        return self.boxes[self.k]


def test_incremental_reference_on_a_cube_and_under_strain():
    """_incremental on made-up frames.  Cube: the sum of the minimum-image increments of before (restated), the same for a scalar and for three extents.
    Strained: frames r_k = wrap(S_k (r_{k-1} + u_k)) return sum u_k, while the end-point difference of the positions holds the affine part too."""
    rng = np.random.default_rng(5)
    L, steps, n = 20.0, 12, 300
    r = [rng.uniform(0, L, (n, 3))]
    for _ in range(steps):
        r.append(np.mod(r[-1] + rng.uniform(-0.3, 0.3, (n, 3)), L))
    want = sum(msd._wrap(r[k + 1] - r[k], L) for k in range(steps))
    got_s = msd._incremental(_FakeSim(r, None), steps, L)
    got_v = msd._incremental(_FakeSim(r, None), steps, (L, L, L))
    assert np.array_equal(got_s[0], want) and np.array_equal(got_v[0], want) and np.array_equal(got_s[3], got_v[3]) and got_s[3].sum() > 0
    boxes = [np.array([20.0, 24.0, 28.0]) * (1 + np.array([0.002, -0.0015, 0.0]) * k) for k in range(steps + 1)]
    frames, moves = [rng.uniform(0, 1, (n, 3)) * boxes[0]], []
    for k in range(steps):
        moves.append(rng.uniform(-0.3, 0.3, (n, 3)))
        frames.append(np.mod((boxes[k + 1] / boxes[k]) * (frames[-1] + moves[-1]), boxes[k + 1]))
    got = msd._incremental(_FakeSim(frames, boxes), steps, boxes[0], strained=True)
    assert np.abs(got[0] - sum(moves)).max() <= steps * 8 * 2.2e-16 * 28.0
    assert np.abs(msd._wrap(frames[-1] - frames[0], boxes[-1]) - sum(moves)).max() > 0.1


RDF_RUN = ["-e", "-x", 10, "-y", 8, "-z", 6, "-N", 40, "-n", 10, "--rdf", 64, "--erateX", 1]


def test_strained_rdf_command_line_is_accepted_host_only(pkg):
    proc = _child(f"s = pkg.Simulation({RDF_RUN + ['--msd', '--csp', '--cna']!r}, host_only=True); print('made', s.n_global, json.dumps(s.box.tolist())); s.close()")
    assert proc.returncode == 0 and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    m = re.search(r"^made (\d+) (.*)$", proc.stdout, flags=re.M)
    assert m and int(m.group(1)) == 1920, proc.stdout[-500:]
    assert np.all(np.abs(np.array(json.loads(m.group(2))) - np.array([10, 8, 6]) * 3.615) <= 4 * EPS * 36.15)


def _narrowest(pkg, pot, method):
    """the narrowest box the grid accepts along x: builtRange * cells * (1 + 1e-12), builtRange the cutoff (plus the default 10 % skin with thread_atom_nl), as
    test_set_box_refuses_cells_narrower_than_the_range reads it.  The float build rounds the extent to 2^-24 relative: there the margin is 4 eps."""
    with pkg.Simulation(POTS[pot] + ["-m", method], host_only=True) as sim:
        box, grid, rc = sim.box, sim.grid, sim.cutoff * (1.1 if method == "thread_atom_nl" else 1.0)
    new = box.copy()
    new[0] = rc * grid[0] * (1.0 + (4 * EPS if SINGLE else 1e-12))
    assert new[0] < box[0]
    return new, box


def _state_scale(pkg, pot, state, method="thread_atom"):
    if state == "a":
        return SCALE
    if state == "c":
        return np.array([1.09, 1.0, 1.0])
    new, box = _narrowest(pkg, pot, method)
    return new / box


_CAPS = {}


def _host_state(pkg, pot, state):
    """(positions, box) of a constructed state from a host-only simulation (-r 0.1), scaled in numpy"""
    if (pot, state) not in _CAPS:
        with pkg.Simulation(POTS[pot], host_only=True) as sim:
            box, rc = sim.box, sim.cutoff
        scale = _state_scale(pkg, pot, state)
        pos = csp._host_positions(pkg, POTS[pot] + ["-r", 0.1]) * scale
        pos.setflags(write=False)
        _CAPS[(pot, state)] = (pos, box * scale, rc)
    return _CAPS[(pot, state)]


@pytest.mark.parametrize("state", ["a", "c", "d"])
@pytest.mark.parametrize("pot", ["lj", "adams", "mishin"])
def test_constructed_states_keep_the_references_inside_their_caps(pkg, pot, state):
    """States (a) deform(SCALE), (c) 9 % along x and (d) the narrowest box, from host-only positions scaled in numpy, through the references alone.  fp64: no pair
    within 1e-9 A of a bin edge (64 bins, and r_max = the cutoff itself), no atom left out of csp, coordination or CNA.  fp32: the modules' share, 0.5 %.
    The references run once, with the 1e-4 A windows; the 1e-9 A question is asked of the same arrays (an atom `unsure` at 1e-9 is unsure at 1e-4)."""
    pos, box, rc = _host_state(pkg, pot, state)
    edges = np.arange(BINS + 1, dtype=np.float64) * (rc / BINS)
    cum, near = rdf._reference(("host", pot, state, 64), pos, box, edges, rdf.DELTA64)
    cum32, near32 = rdf._reference(("host", pot, state, 32), pos, box, edges, rdf.DELTA32)
    ref = csp._numpy_csp(pos, box, rc, R_COORD, csp.DELTA32)
    no_csp, no_coord = csp._left_out(ref, csp.DELTA32, True)
    types = cna._numpy_cna(pos, box, rc, cna.DELTA32)
    out = cna._left_out(types, cna.DELTA32, True)
    print(f"{pot} ({state}): box {box.tolist()} pairs {int(cum[-1])} near-edge {int(near.sum())} (1e-9) {int(near32.sum())} (1e-4, cap {rdf.CAP32 * cum[-1]:.0f}); "
          f"csp left out {int(no_csp.sum())} / {int(no_coord.sum())}, cna {int(out.sum())} (1e-4, cap {csp.CAP32 * len(pos):.1f}); cna {cna._counts(types['type'])}")
    assert cum[-1] > 0 and near.sum() == 0 and near32.sum() <= rdf.CAP32 * cum32[-1]
    assert not ((ref["gap"] < csp.DELTA64) | ref["unsure"]).any() and not (ref["edge"] < csp.DELTA64).any()
    assert not (types["margin"] < cna.DELTA64).any()
    assert np.isfinite(ref["csp"]).all()
    if state != "d":          # the narrowest LJ box is 20 % shorter along x: no longer FCC to the analysis, which is what it should say
        assert cna._counts(types["type"])["fcc"] > 0.9 * len(pos)


# ================================================================ GPU 1: a strained step against the numpy restatement
RATE1 = np.array([3.0, -2.0, 0.0])          # per ps: one step of 1 fs moves a coordinate of 29 A by 0.09 A
STEP_LEGS = {"lj thread_atom": (LJ25 + ["-m", "thread_atom"], 0), "adams cta_cell": (EAM_BOX + ADAMS + ["-m", "cta_cell"], 0),
             "adams thread_atom_nl": (EAM_BOX + ADAMS + ["-m", "thread_atom_nl"], 0), "lj thread_atom -a 1": (LJ25 + ["-m", "thread_atom", "-a", 1], 0),
             "adams cta_cell -H": (EAM_BOX + ADAMS + ["-m", "cta_cell", "-H"], 0), "lj thread_atom --deformStart 1": (LJ25 + ["-m", "thread_atom", "--deformStart", 1], 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("thermostat", ["nve", "langevin"])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("leg", list(STEP_LEGS))
def test_strained_step_matches_the_numpy_restatement(gpu, leg, steps, thermostat):
    """test_langevin.py::test_step_matches_the_numpy_restatement with the remap in it.  The last of `steps` steps from the gathered state before it (a second
    simulation stepped steps - 1) and the forces after it; S = box after / box before, h = dt / 2:
        NVE        r = S (r0 + dt (p0 + h f0) / m)                         p = p0 + h f0 + h f1
        Langevin   r = S (ra + h po / m), ra = r0 + h pb / m, pb = p0 + h f0, po = c1 pb + c2 sqrt(m kT) xi      p = po + h f1
    steps = 1 is the kernel that opens a step() call, steps = 3 the fused closing + opening one; the remap sits behind the drift (behind BOTH half drifts of
    the Langevin kernels) and does not touch p.  --deformStart 1 shifts the counts by one: its last step is the first strained one, after an unstrained one.
    dt = 2 fs.  Tolerances: that test's 1e-12 relative, r after the minimum image in the NEW box; float build: position_abs and force_rel_to_max of
    tolerances_single.  Control: without S the positions miss by a thousand tolerances."""
    args, start = STEP_LEGS[leg]
    args = args + HOT + (["--erateX", RATE1[0], "--erateY", RATE1[1]] if start else [])          # --deformStart goes with the command line's rates
    steps, dt, T, tau = steps + start, 2.0, 300.0, 50.0

    def make():
        sim = gpu.Simulation(args)
        if thermostat == "langevin":
            sim.set_langevin(T, tau, SEED)
        if not start:
            sim.set_strain_rate(RATE1)
        return sim
    with make() as sim:
        if steps > 1:
            sim.step(steps - 1, dt)
        r0, p0, f0 = lv._state(sim)
        m, before = lv._mass(p0, sim.energy()[1]), sim.box
        assert sim.step_count == steps - 1
    with make() as sim:
        sim.step(steps, dt)
        r1, p1, f1 = lv._state(sim)
        after, box0 = sim.box, sim.box0
    assert np.array_equal(after, box0 * (1 + RATE1 * dt * (steps - start) / 1000)) or SINGLE
    S, h = after / before, 0.5 * dt
    assert S[0] > 1.004 and S[1] < 0.997 and S[2] == 1.0
    pb = p0 + h * f0
    if thermostat == "nve":
        flat = r0 + dt * pb / m
        p_want = pb + h * f1
    else:
        c1 = _r(np.exp(-dt / tau))
        c2 = _r(np.sqrt(1.0 - np.exp(-dt / tau) ** 2))
        xi = lv.normals(SEED, np.arange(len(r0)), steps - 1, np.float32 if SINGLE else np.float64)
        po = c1 * pb + c2 * np.sqrt(m * KB * T) * xi
        flat = r0 + h * pb / m + h * po / m
        p_want = po + h * f1
    r_want = S * flat
    tol_r = TOL["position_abs"] if SINGLE else 1e-12 * np.abs(r_want).max()
    tol_p = TOL["force_rel_to_max"] if SINGLE else 1e-12
    err_r, err_p = np.abs(lv._wrap(r1 - r_want, after)).max(), _rel(p1, p_want)
    miss = np.abs(lv._wrap(r1 - flat, after)).max()
    print(f"{leg} {thermostat} steps {steps}: max |dr| {err_r:.2e} (tol {tol_r:.2e})  rel dp {err_p:.2e} (tol {tol_p:.0e})  without the remap {miss:.2e}")
    assert err_r <= tol_r and err_p <= tol_p
    assert miss > 1000 * tol_r and miss > 0.05


# ================================================================ GPU 2: displacement records under strain
RATE2 = np.array([2.0, -1.5, 0.0])          # 20 steps: + 4 % along x, - 3 % along y


def tol_strained(n, box):
    """test_msd.tol(n, L) = n (2^-32 + 2 eps L) is a drift's quantisation plus the roundings of the stored positions the reference is built from.  A strained step
    adds, per component of size <= L: the rounding of the scale L_new / L_old to real_t and that of the product in the remap kernel (half an ulp each, eps L
    together), and in the reference the rounding of S_k and of the division r_k / S_k (eps L together in double, nothing beside eps in the float build):
        tol_strained(n, L) = n (2^-32 + 4 eps L)
    20 steps, L = 37.6 A: 4.7e-9 A (double), 3.6e-4 A (single); a record that followed the remap would be off by strain x coordinate, up to 1.4 A."""
    return n * (Q + 4.0 * EPS * float(np.max(box)))


MSD_LEGS = {"lj thread_atom": (LJ25 + ["-m", "thread_atom"], False), "lj thread_atom_nl langevin": (LJ25 + ["-m", "thread_atom_nl"], True),
            "adams cta_cell langevin": (EAM_BOX + ADAMS + ["-m", "cta_cell"], True), "adams thread_atom_nl": (EAM_BOX + ADAMS + ["-m", "thread_atom_nl"], False)}


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(MSD_LEGS))
def test_displacements_are_the_non_affine_motion(gpu, leg):
    """A 600 K solid strained for 20 x step(1): displacements() against the incremental reference inc_k = minimum_image(r_k / S_k - r_{k-1}, L_{k-1}) of
    test_msd._incremental within tol_strained (above); msd() against the records; and the control that the gathered positions did move with the box."""
    args, thermostat = MSD_LEGS[leg]
    steps = 20
    with gpu.Simulation(args + HOT) as sim:
        if thermostat:
            sim.set_langevin(300.0, 20.0, SEED)
        sim.set_strain_rate(RATE2)
        sim.track_displacement()
        box0 = sim.box
        ref, r_first, r_last, _ = msd._incremental(sim, steps, box0, strained=True)
        d, box1 = sim.displacements(), sim.box
        bound = tol_strained(steps, np.maximum(box0, box1))
        affine = np.abs(msd._wrap(r_last - r_first, box1) - ref).max()
        print(f"{leg}: max |d| {np.abs(ref).max():.3f}  max err {np.abs(d - ref).max():.2e}  tol {bound:.2e}  end-point difference of the positions off by {affine:.3f}")
        assert np.array_equal(box1, box0 * (1 + RATE2 * steps / 1000)) or SINGLE
        assert np.abs(ref).max() > 0.05
        assert np.abs(d - ref).max() <= bound
        assert affine > 0.3
        msd._check_msd(sim, d)


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "adams"])
def test_records_stay_exactly_zero_on_a_strained_perfect_lattice(gpu, pot):
    """-T 0 -r 0 under a strain rate: every site stays a centre of inversion, the forces are rounding noise, and each drift's increment dt p / m rounds to 0 units
    of 2^-32 A -- checked, not assumed: before every step (|p| + dt |f|) dt / m, which bounds its drift, stays below 2^-33 A.  So every record is
    exactly 0 after 20 steps, while the positions moved by strain x coordinate (over 1 A).  In the float build the check says no (see below): there the
    records are held to the sum of those bounds."""
    with gpu.Simulation(POTS[pot] + HOT) as sim:
        p = sim.gather(1)
        m = lv._mass(p, sim.energy()[1])
    with gpu.Simulation(POTS[pot] + ["-T", 0, "-r", 0]) as sim:
        r0, box0 = sim.gather(0).copy(), sim.box
        assert not sim.gather(1).any()
        sim.set_strain_rate(RATE2)
        sim.track_displacement()
        drifts = []
        for _ in range(20):
            drifts.append((np.abs(sim.gather(1)).max() + np.abs(sim.gather(2)).max()) / m)
            sim.step(1)
        worst = max(drifts)
        d, r1, box1 = sim.displacements(), sim.gather(0), sim.box
        print(f"{pot}: largest bound on a drift {worst:.2e} A (2^-33 = {2.0 ** -33:.2e}), max |f| {np.abs(sim.gather(2)).max():.2e}, max |d| {np.abs(d).max():.2e}, "
              f"positions moved by {np.abs(r1 - r0).max():.3f}")
        if SINGLE and worst >= 2.0 ** -33:
            # the float build's forces on these sites are float rounding noise (1e-4 eV/A measured against 1e-13 in double) and its drifts reach 1e-7 A: the
            # premise of the exact zero does not hold there.  What holds is the sum of the bounds, a million times below the 1 A the positions moved.
            assert np.abs(d).max() <= sum(drifts) + 20 * 2.0 ** -33 < 1e-5
        else:
            assert worst < 2.0 ** -33
            assert not d.any() and sim.msd()[0] == 0.0
        moved = msd._wrap(r1 - r0 * (box1 / box0), box1)
        assert np.abs(moved).max() <= 20 * 4 * EPS * box1.max() and np.abs(r1 - r0).max() > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["thread_atom", "thread_atom_nl"])
def test_deform_leaves_the_records_alone(gpu, method):
    with gpu.Simulation(LJ25 + HOT + ["-m", method]) as sim:
        sim.track_displacement()
        sim.step(5)
        before, r0 = sim.displacements(), sim.gather(0).copy()
        sim.deform(SCALE)
        after = sim.displacements()
        assert before.any() and np.array_equal(before, after)
        assert np.abs(sim.gather(0) - r0).max() > 0.1
        sim.step(3)
        assert not np.array_equal(sim.displacements(), after)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _ranks(tmp_path, grid, args, job, timeout=300):
    port, world = _port(), grid[0] * grid[1] * grid[2]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "deform_coupling_worker.py"), "ranks", json.dumps(args), json.dumps(job), str(tmp_path / f"rank{r}.npz"),
                               str(r), str(world), port, *map(str, grid)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "COUPLING saved" in out, f"rank {r} failed:\n{out[-3000:]}"
    return [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]


def _single(tmp_path, name, args, job, env):
    out = str(tmp_path / f"{name}.npz")
    proc = subprocess.run([sys.executable, os.path.join(HERE, "deform_coupling_worker.py"), "single", json.dumps(args), json.dumps(job), out], cwd=ROOT,
                          env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "COUPLING saved" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-2000:]
    return np.load(out)


@pytest.mark.gpu
def test_two_ranks_give_the_one_rank_displacements_under_strain(gpu, tmp_path):
    """2 x 1 x 1 ranks sharing the device (gloo), strain along x (the axis the ranks split).  First the summed positions against the one-rank run at the tolerance
    of test_msd.py::test_two_ranks_give_the_one_rank_displacements, then every rank's displacements() against the one-rank array within that bound, widened by the
    remap's n 4 eps L of tol_strained; at least one atom changed rank.
    The affine remap keeps every atom's fraction of the box, the rank face included, so the remap alone moves no atom to the other rank, and a 600 K solid
    keeps its atoms 0.9 A from the face: the state is -T 20000 for 60 steps (amplitudes of some 0.5 A a component), where thermal motion carries atoms across
    the face while the box under them is stretched by 6 %."""
    args, steps, rates = LJ25 + ["-r", 0.1, "-T", 20000], 60, [1.0, 0.0, 0.0]
    with gpu.Simulation(args) as sim:
        sim.set_strain_rate(rates)
        sim.track_displacement()
        sim.step(steps)
        r0, d0, box = sim.gather(0).copy(), sim.displacements(), sim.box
    parts = _ranks(tmp_path, (2, 1, 1), args, {"rates": rates, "steps": steps, "track": True})
    assert all(np.array_equal(s["box"], box) for s in parts)
    assert np.all(sum(s["own1"].astype(int) for s in parts) == 1) and np.all(sum(s["own0"].astype(int) for s in parts) == 1)
    r = sum(s["r"] for s in parts)
    tol_r = 100 * TOL["force_rel_to_max"] * np.abs(r0).max()
    print("two ranks: positions differ by", np.abs(msd._wrap(r - r0, box)).max(), "bound", tol_r)
    assert np.abs(msd._wrap(r - r0, box)).max() <= tol_r
    bound = tol_r + steps * (Q + 2.0 * EPS * box.max())          # that test's tol_r + steps 2^-32, and the remap kernel's two roundings a step
    for s in parts:
        print("two ranks: displacements differ by", np.abs(s["d"] - d0).max(), "bound", bound)
        assert np.abs(s["d"] - d0).max() <= bound
    assert np.array_equal(parts[0]["d"], parts[1]["d"]) and np.array_equal(parts[0]["msd"], parts[1]["msd"])
    want = (parts[0]["d"] ** 2).sum() / d0.shape[0]
    assert abs(parts[0]["msd"][0] - want) <= 1e-12 * want
    moved = int((parts[0]["own0"] != parts[0]["own1"]).sum())
    print("two ranks: atoms that changed rank", moved, " max |d|", np.abs(d0).max())
    assert moved >= 1


# ================================================================ GPU 3: the analyses on a changed box
_ANALYSIS_REF = {}


def _references(key, pos, box, edges, rc):
    """the three modules' references for one state, computed once per key and shared by the legs that hold the same positions (checked: bit for bit)"""
    held = _ANALYSIS_REF.get(key)
    if held is None or not (np.array_equal(held[0], pos) and np.array_equal(held[1], edges)):
        held = (pos.copy(), edges.copy(), rdf._reference(object(), pos, box, edges, DELTA), csp._numpy_csp(pos, box, rc, R_COORD, DELTA), cna._numpy_cna(pos, box, rc, DELTA))
        _ANALYSIS_REF[key] = held
    return held[2:]


def _check_analyses(sim, what, key, r_max=None):
    """pair_histogram / rdf, centro_symmetry(R_COORD) and common_neighbor_analysis / structure_counts of the current state against the modules' references on the
    gathered positions in sim.box, under the modules' own rules; rdf() against counts / ideal with V = prod(sim.box) restated (1e-14, as test_rdf's lattice test)."""
    pos, box = sim.gather(0), sim.box
    edges, counts = sim.pair_histogram(BINS, r_max)
    (cum, near), ref_csp, ref_cna = _references(key, pos, box, edges, sim.cutoff)
    rdf._check(counts, cum, near, SINGLE, what)
    r, g = sim.rdf(BINS, r_max)
    n, dr, k = float(sim.n_global), edges[-1] / BINS, np.arange(BINS, dtype=np.float64)
    ideal = (0.5 * n) * (n / (box[0] * box[1] * box[2])) * (4.0 * np.pi / 3.0 * dr * dr * dr) * ((k + 1.0) ** 3 - k ** 3)
    assert np.all(np.abs(g - counts / ideal) <= 1e-14 * (counts / ideal)) and g.max() > 1.0, np.abs(g - counts / ideal).max()
    assert np.all(np.abs(r - (k + 0.5) * dr) <= 1e-14 * r)
    c, coord = sim.centro_symmetry(R_COORD)
    csp._check(c, coord, ref_csp, SINGLE, what)
    types = sim.common_neighbor_analysis()
    cna._check(types, ref_cna, SINGLE, what)
    assert sim.structure_counts() == cna._counts(types)
    return counts, c, coord, types


ANALYSIS_LEGS = [(pot, method) for pot in ("lj", "adams") for method in ("thread_atom", "cta_cell", "thread_atom_nl")] + [("mishin", "thread_atom")]


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["a", "b", "c", "d"])
@pytest.mark.parametrize("pot,method", ANALYSIS_LEGS)
def test_analyses_on_a_changed_box(gpu, pot, method, state):
    """(a) after deform((1.03, 0.99, 1.01)); (b) after 10 strained steps of a 600 K solid (with thread_atom_nl the atoms keep the slots of the last list build
    and may sit outside the box); (c) after a 9 % stretch along x, the widest cells the 12-nearest walk sees; (d) at the narrowest box the grid accepts
    along x, builtRange x cells x (1 + 1e-12), where the 27-cell walk only just reaches the cutoff: set_box must accept it and pair_histogram with
    r_max = cutoff must be exact.  Each against the numpy references of test_rdf, test_csp and test_cna with sim.box as the extent."""
    args = POTS[pot] + ["-m", method]
    if state == "b":
        with gpu.Simulation(args + HOT) as sim:
            sim.set_strain_rate(RATE1)
            sim.step(10)
            assert np.array_equal(sim.box, sim.box0 * (1 + RATE1 * 10 / 1000)) or SINGLE
            _check_analyses(sim, f"{pot} {method} (b)", (pot, method, "b"))
        return
    with gpu.Simulation(args + DISORDER) as sim:
        box0 = sim.box
        if state == "d":
            new, _ = _narrowest(gpu, pot, method)
            sim.set_box(new)
            assert np.array_equal(sim.box, [_r(v) for v in new])
            with pytest.raises(ValueError):
                sim.set_box(new * np.array([1.0 - 1e-3, 1.0, 1.0]))
            _check_analyses(sim, f"{pot} {method} (d)", (pot, "nl" if method == "thread_atom_nl" else "cells", "d"), r_max=sim.cutoff)
        else:
            sim.deform(_state_scale(gpu, pot, state))
            assert not np.array_equal(sim.box, box0)
            _check_analyses(sim, f"{pot} {method} ({state})", (pot, state))


@pytest.mark.gpu
@pytest.mark.parametrize("pot,grid", [("lj", (2, 1, 1)), ("adams", (2, 1, 1)), ("adams", (2, 2, 2))])
def test_ranks_give_the_one_rank_analyses_after_strained_steps(gpu, tmp_path, pot, grid):
    """2 and 8 ranks sharing the device (gloo), 10 strained steps of the 600 K solid: every rank returns the global arrays; histogram counts, coordination and CNA
    types are exactly the one-rank ones, csp within test_csp.py's multi-rank tolerance (1e-10 A^2 + 1e-12 csp; float build: its 5e-3 A^2 + 1e-5 csp)."""
    args, job = POTS[pot] + HOT, {"rates": RATE1.tolist(), "steps": 10, "analyses": True, "bins": BINS, "r_coord": R_COORD}
    with gpu.Simulation(args) as sim:
        sim.set_strain_rate(RATE1)
        sim.step(10)
        counts0, c0, coord0, types0 = _check_analyses(sim, f"{pot} one rank", (pot, "ranks"))
        box = sim.box
    got = _ranks(tmp_path, grid, args, job)
    for g in got:
        assert np.array_equal(g["box"], box) and int(g["step"]) == 10
        for key in ("counts", "csp", "coord", "cna"):
            assert np.array_equal(g[key], got[0][key]), key
    diff = np.abs(got[0]["csp"] - c0)
    print(f"{grid} {pot}: largest |csp difference| to one rank {diff.max():.3e}")
    assert np.array_equal(got[0]["counts"], counts0) and np.array_equal(got[0]["coord"], coord0) and np.array_equal(got[0]["cna"], types0)
    assert np.all(diff <= ((5e-3 + 1e-5 * c0) if SINGLE else (1e-10 + 1e-12 * c0)))


# ================================================================ GPU 4: the executable's g(r) under strain
def _comd_hip(tmp_path, extra):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-d", os.path.join(ROOT, "pots")] + [str(a) for a in RDF_RUN[:11] + extra],
                          capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    assert len(yaml) == 1
    text = (tmp_path / yaml[0]).read_text()
    os.remove(tmp_path / yaml[0])
    header, table = rdf._rdf_file(tmp_path / "rdf.dat")
    os.remove(tmp_path / "rdf.dat")
    keys = dict(re.findall(r"\b(bins|rMax|samples|N|V) (\S+)", header.split("|")[0]))
    return proc.stdout, text, keys, table


@pytest.mark.gpu
def test_comd_hip_normalises_the_strained_rdf_with_the_mean_density(gpu, tmp_path):
    """comd-hip --rdf 64 --erateX 1 on 10 x 8 x 6 Adams, -N 40 -n 10 (the double executable, whatever COMD_PRECISION says).  comdMain samples at the top of every
    print interval and once after the loop: steps 0, 10, 20, 30, 40.  The header's V is N over the mean of N / V_k, V_k = prod(box0 (1 + rate step_k / 1000));
    g is the pairs-per-sample column over the ideal count at that V.  Without the rate V is prod(box0), the expression of before, to the bit.  With --msd
    --csp --cna beside the rate the run keeps its atoms and writes all four YAML blocks."""
    box0, rate, sampled = np.array([10 * 3.615, 8 * 3.615, 6 * 3.615]), np.array([1.0, 0.0, 0.0]), [0, 10, 20, 30, 40]
    out, yaml, keys, table = _comd_hip(tmp_path, ["--rdf", 64, "--erateX", 1])
    n, samples, V, r_max = int(keys["N"]), int(keys["samples"]), float(keys["V"]), float(keys["rMax"])
    assert n == 1920 and samples == len(sampled) and int(keys["bins"]) == 64 and table.shape == (64, 4)
    vk = [float(np.prod(box0 * (1 + rate * k / 1000))) for k in sampled]
    want = n / np.mean([n / v for v in vk])
    print(f"strained rdf: V {V!r}  N / mean(N / V_k) {want!r}  rel {abs(V - want) / want:.2e}  (final V {vk[-1]!r}, initial {vk[0]!r})")
    assert abs(V - want) <= 1e-12 * want
    assert abs(V - vk[-1]) > 1e-3 * want and abs(V - vk[0]) > 1e-3 * want          # neither end of the run would pass
    dr, k = r_max / 64, np.arange(64, dtype=np.float64)
    ideal = (0.5 * n) * (n / V) * (4.0 * np.pi / 3.0 * dr ** 3) * ((k + 1.0) ** 3 - k ** 3)
    assert table[:, 3].sum() > 0 and np.all(np.abs(table[:, 1] - table[:, 3] / ideal) <= 1e-12 * (table[:, 3] / ideal))
    assert re.search(r"^  samples: 5$", re.search(r"^RDF:\n((?:  .*\n)+)", yaml, flags=re.M).group(1), flags=re.M)
    _, _, keys0, table0 = _comd_hip(tmp_path, ["--rdf", 64])
    assert float(keys0["V"]) == box0[0] * box0[1] * box0[2] and int(keys0["samples"]) == 5
    ideal0 = ideal * V / float(keys0["V"])
    assert np.all(np.abs(table0[:, 1] - table0[:, 3] / ideal0) <= 1e-12 * (table0[:, 3] / ideal0))
    out, yaml, keys, _ = _comd_hip(tmp_path, ["--rdf", 64, "--erateX", 1, "--msd", "--csp", "--cna"])
    assert "no atoms lost" in out and "atoms lost #" not in out and int(keys["samples"]) == 5
    for block in ("RDF", "MSD", "CSP", "CNA", "Deform"):
        assert re.search(rf"^{block}:\n((?:  .*\n)+)", yaml, flags=re.M), block


# ================================================================ GPU 5: the paths no strained step had gone through
def _strained(gpu, args, rate, steps=40):
    with gpu.Simulation(args + ["--erateX", rate]) as sim:
        sim.step(steps)
        return {"pos": sim.gather(0), "f": sim.gather(2), "e": sim.energy(), "box": sim.box, "builds": sim.nl_builds}


@pytest.mark.gpu
def test_pairlists_stay_valid_under_compression(gpu):
    """test_deform.py::test_lists_stay_valid_under_compression for cta_cell -L (LJ; the pair-list bits share the lists' skin budget): --erateX -2 and +2 for 40 steps.
    The -L grid (4 cells of 7.23 A for a range of 6.37 A) follows the 8 %.  Forces and energy of the final state are those cta_cell computes on the same positions
    in the same box, to the parity tolerance; more builds under compression than free, not more than free + 1 under tension."""
    args = LJ25 + HOT + ["-m", "cta_cell", "-L"]
    free = _strained(gpu, args, 0)
    for rate in (-2, 2):
        run = _strained(gpu, args, rate)
        assert np.array_equal(run["box"], [_r(v) for v in free["box"] * np.array([1 + rate * 40 / 1000, 1, 1])])
        with gpu.Simulation(LJ25 + HOT + ["-m", "cta_cell"]) as ref:
            ref.set_box(run["box"])
            ref.scatter(0, run["pos"])
            ref.redistribute()
            ref.compute_force()
            ref.kinetic_energy()
            fo, eo = ref.gather(2), ref.energy()[0]
        df, dE = np.abs(run["f"] - fo).max() / np.abs(fo).max(), abs(run["e"][0] - eo) / run["e"][2]
        print(f"cta_cell -L rate {rate}: builds {run['builds']} (free {free['builds']})  max|df|/max|f| {df:.2e}  |dE|/N {dE:.2e}")
        assert df <= TOL["force_rel_to_max"] and dE <= TOL["energy_per_atom_step0"], (rate, df, dE)
        if rate < 0:
            assert run["builds"] > free["builds"], (run["builds"], free["builds"])
        else:
            assert run["builds"] <= free["builds"] + 1, (run["builds"], free["builds"])


def _same_bits(a, b, keys=("r", "p", "f", "e", "energy", "box")):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["lj thread_atom", "adams cta_cell", "adams thread_atom_nl"])
def test_message_halo_is_the_mirrored_halo_under_strain(tmp_path, leg):
    """COMD_HALO_MIRROR=0 (pack, message, unpack, with the periodic shifts haloSetBox renews) against the default (halo cells filled from the cells they are images
    of, with its own shift table), 10 strained steps in a child process each: positions, momenta, forces, per-atom and total energies bit for bit, as
    test_density_regimes.py has it for the fixed box.  The thread_atom_nl leg is there for the position exchange, which refreshes the halo copies between list
    builds with shifts of its own."""
    job = {"rates": RATE1.tolist(), "steps": 10}
    a = _single(tmp_path, "mirror", STEP_LEGS[leg][0] + HOT, job, {"COMD_HALO_MIRROR": "1"})
    b = _single(tmp_path, "message", STEP_LEGS[leg][0] + HOT, job, {"COMD_HALO_MIRROR": "0"})
    assert a["f"].any() and int(a["step"]) == 10
    _same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "adams"])
def test_deferred_list_test_falls_back_under_a_rate(tmp_path, pot):
    """COMD_NL_DEFERRED=1 with a rate on must take the blocking rule: list builds and the final state after 40 steps at --erateX -2 are those of
    COMD_NL_DEFERRED=0, bit for bit."""
    job, args = {"rates": [-2.0, 0.0, 0.0], "steps": 40}, POTS[pot] + HOT + ["-m", "thread_atom_nl"]
    a = _single(tmp_path, "blocking", args, job, {"COMD_NL_DEFERRED": "0"})
    b = _single(tmp_path, "deferred", args, job, {"COMD_NL_DEFERRED": "1"})
    print(f"{pot}: list builds {int(a['builds'])} / {int(b['builds'])}")
    assert int(a["builds"]) > 1 and int(a["builds"]) == int(b["builds"])
    _same_bits(a, b)


LAYOUT_LEGS = {"lj thread_atom": LJ25 + ["-m", "thread_atom"], "adams cta_cell": EAM_BOX + ADAMS + ["-m", "cta_cell"], "adams thread_atom": EAM_BOX + ADAMS + ["-m", "thread_atom"]}


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(LAYOUT_LEGS))
def test_stream_modes_and_numbering_agree_under_a_rate(gpu, leg):
    """-a 0, -a 1 and -H through 10 strained step()s (with -a 1 the interior force launch must see the box the remap of the same step has set): the energy to
    energy_per_atom_trace, positions and forces by gid to the multi-rank trajectory tolerances of multirank_worker.py (TRAJ_R, TRAJ_F)."""
    from multirank_worker import TRAJ_F, TRAJ_R
    got = {}
    for name, extra in (("-a 0", ["-a", 0]), ("-a 1", ["-a", 1]), ("-H", ["-H"])):
        with gpu.Simulation(LAYOUT_LEGS[leg] + HOT + extra) as sim:
            sim.set_strain_rate(RATE1)
            sim.step(10)
            got[name] = (sim.gather(0), sim.gather(2), sim.energy(), sim.box)
    r0, f0, e0, box = got["-a 0"]
    for name, (r, f, e, b) in got.items():
        dr, df, dE = np.abs(lv._wrap(r - r0, box)).max(), np.abs(f - f0).max() / np.abs(f0).max(), abs((e[0] + e[1]) - (e0[0] + e0[1])) / e0[2]
        print(f"{leg} {name}: max |dr| {dr:.2e}  max|df|/max|f| {df:.2e}  |dE|/N {dE:.2e}")
        assert np.array_equal(b, box) and dr < TRAJ_R and df < TRAJ_F and dE < TOL["energy_per_atom_trace"], (name, dr, df, dE)
