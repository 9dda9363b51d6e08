"""The per-atom fields -- stress, heat flux, strain (AtomStress_thread_atom, HeatFlux_thread_atom, AtomStrain_thread_atom) -- on 2-cell periodic boxes, on a
straining box driven from Python, and where the image of a reference separation is not the shortest one.

tests/test_atom_stress.py, test_heat_flux.py and test_atomic_strain.py meet one 2-cell state (B / BI: an LJ cube of 2 x 2 x 2 cells with 2.9 A between the cutoff and
half the box) and no straining box; the suites of the awkward geometries (test_two_cell_boxes.py, test_deform_coupling.py) were written before these kernels.  This
module runs the three kernels there.  It adds no restatement: states, restatements, comparison rules and bounds are the imported modules' own, unchanged --
test_atom_stress._restate / _pair_function / _assert_close, test_heat_flux._times_v / _convective and the rules of its docstring, test_atomic_strain._restate /
_assert_within / C_BOUND, the summary rules as test_analysis_regimes.py applies them, reference_values.json tolerances for the per-atom energies.  The one thing new is
the rule that picks the image of a reference separation (test_atomic_strain._image_of_d0, part 4).

  1. Two-cell boxes: the EAM grids (F' of a halo slot read through two images of one cell), the mixed grids, eam_tight (cells 0.03 % wider than the cutoff) and eam_hot
     after atoms have wrapped through 2-cell axes, under thread_atom and cta_cell, at step 0 and after the state's steps.
  2. A straining box: a strain rate with unequal rates (one negative) for 20 steps, and set_box followed by 5 steps; LJ, Adams and Mishin; once with the thermostat,
     the overlap mode and the Hilbert numbering.
  4. strain_half: FCC 4^3 at -l 2.4753, cells of 4.9506 A against the 4.95 A cutoff.  With the strain radius at the cutoff, neighbours are accepted through an image
     whose reference separation lies beyond L0 / 2: the shortest image of d0 is then another one and d0 is off by a box length.  CPU tests show in numpy that the two
     rules differ there (and on eam_hot at the cutoff radius) and nowhere else in the suite; the GPU tests hold the kernel to the image nearest the current separation.
(Part 3, the heat flux in the density regimes, is the heat-flux leg of tests/test_analysis_regimes.py.)

The potential part of the heat flux is e_i v_i.  Every test of test_heat_flux.py takes e_i from gather(3), the array the kernel reads; here e_i comes from an all-pairs
sum in numpy on the gathered positions at the CURRENT box (test_density_regimes._lj_all_pairs / _eam_all_pairs), so an e[] left at the old geometry by a step under a
strain rate or by set_box fails here.

Several ranks need nothing new: test_atom_stress / test_atomic_strain / test_heat_flux test_ranks_give_the_one_rank_array(s) run EAM 8^3 on 2 x 2 x 2 ranks of
2 x 2 x 2 cells each.

The module runs in whichever precision COMD_PRECISION selects; tests/test_single_precision.py runs it in the float build and counts its GPU tests (GPU_CASE_COUNT).
Every GPU test prints its worst error / bound as RATIO lines; no bound is fitted to them.
"""
import math

import numpy as np
import pytest

import test_analysis_regimes as regimes
import test_atom_stress as tas
import test_atomic_strain as strain
import test_density_regimes as dr
import test_heat_flux as thf
import test_two_cell_boxes as tcb
from test_deform import EAM_BOX, LJ25
from test_pressure import ADAMS, MISHIN, SIGMA, _pairs
from test_two_cell_boxes import PRECISION, REAL, SINGLE, STATES, TOL, State, _extent, _flags, _make, _reference

EPS_REAL = tas.EPS24 if SINGLE else tas.EPS53
METHODS = ["thread_atom", "cta_cell"]
# (state, steps): each state at step 0 and after its steps; eam_hot after its 360 steps only
TWO_CELL = [(name, k) for name in ("eam_cube", "eam_mixed", "eam_tight", "eam_setfl", "lj_mixed") for k in (0, STATES[name].steps)] + [("eam_hot", STATES["eam_hot"].steps)]
# part 4: -e -x 4 -y 4 -z 4 -l 2.4753 -r 0.05 -T 600: 256 atoms, grid (2, 2, 2), cells of 4.9506 A against the 4.95 A cutoff (occupancy is not a recorded figure here)
STRAIN_HALF = State(1, (4, 4, 4), 2.4753, 0.05, 600.0, 5, (2, 2, 2), (0, 1, 2), 256, None, "Cu_u6.eam", None, (2, 2, 2))
IMAGE_MAY_DECIDE = ("eam_tight", "eam_hot")       # two-cell states where, at the cutoff radius, a reference separation can pass L0 / 2 (a CPU test counts the pairs)
POTS = {"lj": LJ25, "adams": EAM_BOX + ADAMS, "mishin": EAM_BOX + MISHIN}
HOT = ["-r", 0.1, "-T", 600]                      # disorder and a finite temperature: no velocity component is 0
RATES = (1.0, -0.5, 0.25)                         # 1/ps: 2 %, -1 % and 0.5 % over the 20 steps of history (a)
STRAINED = [(pot, history, []) for pot in POTS for history in ("rate", "set_box")] + [("adams", "rate", ["--langevin", "-a", 1, "-H"])]

RATIOS = {}


def _box(st):
    """the extents as the build under test holds them"""
    return (np.array(st.n, dtype=np.float32) * np.float32(st.lat)).astype(np.float64) if SINGLE else _extent(st)


def _ratio(what, key, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        value = float(np.where(bound > 0.0, np.abs(err) / np.where(bound > 0.0, bound, 1.0), np.where(np.abs(err) > 0.0, np.inf, 0.0)).max())
    RATIOS[(what, key)] = value
    print(f"RATIO {what}: {key} {value:.4g}")
    return value


# ---------------------------------------------------------------- the numpy references of one gathered state, once per state
_NUMPY = {}


def _numpy_of(sim, eam, pos, box, rc):
    """test_atom_stress._restate with the pair function of the run and the all-pairs per-atom energies of test_density_regimes, on the gathered positions at the
    current box; cached by the bits of what they are made from (at step 0 in the double build the positions do not depend on the method)"""
    df = sim.gather(5).copy() if eam else np.zeros(0)
    key = (eam, pos.tobytes(), box.tobytes(), df.tobytes(), rc)
    if key not in _NUMPY:
        if eam:
            tables = [sim.eam_table(k) for k in range(3)]
            fr_of = tas._pair_function("eam", tables[0], tables[1], df)
            e_ref = dr._eam_all_pairs(pos, box, rc, tables)[1]
        else:
            fr_of = tas._pair_function("lj")
            e_ref = dr._lj_all_pairs(pos, box, rc)[1]
        want, big_a, cnt = tas._restate(pos, box, rc, fr_of)
        _NUMPY[key] = dict(want=want, A=big_a, cnt=cnt, e=np.asarray(e_ref, dtype=np.float64))
    return _NUMPY[key]


# ---------------------------------------------------------------- the checks of parts 1 and 2
def _check_stress(sim, what, ref, pos):
    """every atom against the restatement (test_pair_part_matches_the_restatement; float build: test_single_precision_build), the rows against -(K + W) of virial()
    (test_rows_add_up_to_the_virial; float build: the sum rule of test_single_precision_build, the kinetic sums as tests/test_analysis_regimes.py), the reduction
    against numpy on the array (test_summary_is_numpy_on_the_array)"""
    want, big_a, cnt = ref["want"], ref["A"], ref["cnt"]
    s0, s1 = sim.atomic_stress(kinetic=False), sim.atomic_stress(kinetic=True)
    assert s0.shape == (len(pos), 6) and s0.dtype == np.float64 and cnt.min() > 0 and np.all(big_a > 0.0)
    bound = ((cnt[:, None] + 64.0) * tas.EPS24 * big_a) if SINGLE else 1e-11 * big_a
    _ratio(what, "stress", s0 - want, bound)
    tas._assert_close(s0, want, bound, f"{what} pair part")
    w, k = sim.virial()
    w6, k6 = tas._six(w), tas._six(k)
    total = (2.0 * bound.sum(0) + tas.EPS24 * np.abs(w6)) if SINGLE else 1e-11 * big_a.sum(0)
    kin, _, _ = regimes._kinetic(sim)
    kinetic_sums = (1e-5 * np.abs(kin).sum(0)) if SINGLE else 0.0
    _ratio(what, "rows against -W", s0.sum(0) + w6, total)
    _ratio(what, "rows against -(K + W)", s1.sum(0) + (k6 + w6), total + kinetic_sums)
    tas._assert_close(s0.sum(0), -w6, total, f"{what} rows against -W")
    tas._assert_close(s1.sum(0), -(k6 + w6), total + kinetic_sums, f"{what} rows against -(K + W)")
    regimes._check_stress_summary(sim, f"{what} kinetic=False", s0, False)
    regimes._check_stress_summary(sim, f"{what} kinetic=True", s1, True)


def _check_heat_flux(sim, what, ref, mom, need_moving=True):
    """The rules of test_heat_flux.py's docstring.  Virial columns against -s_i v_i of the restatement; kinetic columns by _convective; potential columns against
    e_ref,i v_i with e_ref from numpy at the current box, (per_atom_energy_abs + 8 eps (|e_i| + ke_i)) |v_i,a|; heat_flux() against the column sums
    (test_reduction_is_the_sum_of_the_rows, k recomputed from the run); heat_flux_density() = total / volume."""
    mass = sim.mass
    v = mom / mass
    if need_moving:
        assert np.abs(v).min() > 0.0
    j, sums = sim.atomic_heat_flux(), sim.heat_flux()
    assert j.shape == (len(mom), 9) and j.dtype == np.float64
    b = thf._times_v(ref["A"], np.abs(v))
    bound = ((ref["cnt"][:, None] + 64.0) * tas.EPS24 * b) if SINGLE else 1e-11 * b
    _ratio(what, "flux virial", j[:, 6:9] + thf._times_v(ref["want"], v), bound)
    tas._assert_close(j[:, 6:9], -thf._times_v(ref["want"], v), bound, f"{what} virial columns")
    jk, jp, mag = thf._convective(ref["e"], mom, mass)
    _ratio(what, "flux kinetic", j[:, 0:3] - jk, 8.0 * EPS_REAL * mag)
    tas._assert_close(j[:, 0:3], jk, 8.0 * EPS_REAL * mag, f"{what} kinetic columns")
    bound_p = TOL["per_atom_energy_abs"] * np.abs(v) + 8.0 * EPS_REAL * mag
    _ratio(what, "flux potential", j[:, 3:6] - jp, bound_p)
    tas._assert_close(j[:, 3:6], jp, bound_p, f"{what} potential columns (e from numpy at the current box)")
    k = math.ceil(math.ceil(sim.n_local_boxes * math.ceil(sim.max_atoms / 64) / 2048) / 4)
    assert k == 1, (sim.n_local_boxes, sim.max_atoms)
    rows = np.abs(j).sum(0)
    for part, cols in (("kinetic", slice(0, 3)), ("potential", slice(3, 6)), ("virial", slice(6, 9))):
        _ratio(what, f"flux sum {part}", sums[part] - j[:, cols].sum(0), (k + 2) * EPS_REAL * rows[cols])
        tas._assert_close(sums[part], j[:, cols].sum(0), (k + 2) * EPS_REAL * rows[cols], f"{what} {part} sum")
    total = j[:, 0:3].sum(0) + j[:, 3:6].sum(0) + j[:, 6:9].sum(0)
    tas._assert_close(sums["total"], total, (k + 3) * EPS_REAL * (rows[0:3] + rows[3:6] + rows[6:9]), f"{what} total")
    assert np.array_equal(sums["total"], (sums["kinetic"] + sums["potential"]) + sums["virial"])
    assert np.array_equal(sim.heat_flux_density(), sums["total"] / sim.volume)


def _radius(sim, rs):
    return strain._default_rs(sim.lattice_constant) if rs is None else rs


def _check_strain(sim, what, pos, box, ref, box0, radii=None, want=None):
    """atomic_strain at both radii of test_atomic_strain._radii against its restatement (d0 through the image nearest the current separation) under _assert_within and
    C_BOUND, and strain_summary against numpy on the arrays (test_summary_is_numpy_on_the_arrays).  want: the exact answer (E, D^2) where there is one."""
    for key, rs in (strain._radii(sim) if radii is None else radii).items():
        m = strain._restate(pos, box, ref, box0, _radius(sim, rs), dtype=REAL)
        got = sim.atomic_strain(rs)
        eps = strain._eps(m, PRECISION, box)
        want_e, want_d2 = (m["e"], m["d2"]) if want is None else want
        strain._assert_within(f"{what} {key}", got, want_e, want_d2, m, eps)
        RATIOS[(what, f"strain {key}")] = strain.RATIOS[f"{what} {key}"]
        regimes._check_strain_summary(sim, f"{what} {key}", got, m, rs)


def _check_zero_strain(sim, what, pos, box):
    """test_zero_strain_at_the_reference: E = 0, D^2 = 0, the counts are centro_symmetry's coordination at the same radius"""
    for key, rs in strain._radii(sim).items():
        assert np.array_equal(sim.atomic_strain(rs)[2], sim.centro_symmetry(r_coord=rs)[1]), (what, key)
    _check_strain(sim, f"{what} zero", pos, box, pos, box, want=(np.zeros((len(pos), 6)), np.zeros(len(pos))))


def _check_fields(sim, what, eam, box):
    pos, mom = sim.gather(0).copy(), sim.gather(1).copy()
    ref = _numpy_of(sim, eam, pos, box, sim.cutoff)
    _check_stress(sim, what, ref, pos)
    _check_heat_flux(sim, what, ref, mom)
    return pos


# ================================================================ 4. CPU: the image of a reference separation
def _checker_states(orc, st):
    """the checker's positions at step 0 and after the state's steps"""
    o = _make(orc, st)
    ref = o.gather(orc.R).copy()
    o.step(st.steps)
    pos = o.gather(orc.R).copy()
    rc = orc.lib().oracle_cutoff(o.ptr)
    o.close()
    return ref, pos, rc


def _images(pos, box, ref, box0, rs):
    """the accepted ordered pairs of test_pressure._pairs at radius rs and the integer images of their reference separations under the two rules of
    test_atomic_strain._image_of_d0"""
    box, box0 = np.asarray(box, dtype=np.float64), np.asarray(box0, dtype=np.float64)
    i, j, d, _ = _pairs(pos, box, rs)
    d0 = ref[j] - ref[i]
    return strain._image_of_d0(d0, -d, box, box0, "nearest"), strain._image_of_d0(d0, -d, box, box0, "minimum")


def _differing(pos, box, ref, box0, rs):
    new, old = _images(pos, box, ref, box0, rs)
    return int((new != old).any(axis=1).sum()), len(new)


def test_strain_half_is_accepted_with_two_cells(pkg):
    pkg.init_parallel(0, 1, None)
    for method in METHODS:
        with pkg.Simulation(_flags(STRAIN_HALF, method), host_only=True) as sim:
            assert sim.grid == (2, 2, 2) and sim.n_global == 256
            assert 4.95 < 0.5 * 4 * 2.4753 < 4.95 * 1.0002              # cells of 4.9506 A against the 4.95 A cutoff


def test_the_two_image_rules_differ_on_strain_half(orc):
    """No device here.  The checker's step 0 and step 5 of strain_half, strain radius = the cutoff: at least 20 ordered pairs take different images under the two
    rules; the two restatements differ in E by more than 100 x test_atomic_strain's bound for at least one atom; under the image nearest the current separation the
    largest shear strain stays below a tenth of what the shortest image gives."""
    ref, pos, rc = _checker_states(orc, STRAIN_HALF)
    box = _extent(STRAIN_HALF)
    differ, pairs = _differing(pos, box, ref, box, rc)
    rows_new, rows_old = [], []
    new = strain._restate(pos, box, ref, box, rc, dtype=REAL, image_rows=rows_new)
    old = strain._restate(pos, box, ref, box, rc, dtype=REAL, image="minimum", image_rows=rows_old)
    rows_new, rows_old = np.concatenate(rows_new), np.concatenate(rows_old)
    assert np.array_equal(rows_new[:, :2], rows_old[:, :2]) and int((rows_new[:, 2:] != rows_old[:, 2:]).any(axis=1).sum()) == differ and len(rows_new) == pairs
    assert not new["invalid"].any() and not old["invalid"].any()
    eps = strain._eps(new, PRECISION, box)
    bound = strain.C_BOUND * (new["n"] + 64.0) * eps * new["kappa"] * (1.0 + 2.0 * np.abs(new["e"]).max(1))
    worst = (np.abs(new["e"] - old["e"]).max(1) / bound).max()
    shear_new, shear_old = strain._shear(new["e"]).max(), strain._shear(old["e"]).max()
    print(f"strain_half: {differ} of {pairs} ordered pairs take another image; E differs by {worst:.3g} bounds; largest shear {shear_new:.4g} (nearest) {shear_old:.4g} (shortest)")
    assert differ >= 20 and worst > 100.0 and shear_new < 0.1 * shear_old
    # the rule can be chosen per axis: the shortest image along x alone is wrong on x alone
    rows_x = []
    strain._restate(pos, box, ref, box, rc, dtype=REAL, image=("minimum", "nearest", "nearest"), image_rows=rows_x)
    rows_x = np.concatenate(rows_x)
    assert np.array_equal(rows_x[:, 2], rows_old[:, 2]) and np.array_equal(rows_x[:, 3:], rows_new[:, 3:])


def test_where_else_the_image_rules_can_differ(orc):
    """The two-cell states at the cutoff radius whose margin between the cutoff and half the box is within reach of the atoms' motion, from the checker's step 0 and last
    step.  eam_hot (10.845 A boxes: 0.47 A between the cutoff and L / 2, 360 steps at 3000 K) has such pairs, so its strain comparison at the cutoff radius decides
    between the rules as strain_half's does.  eam_tight (9.903 A: 0.0015 A of margin, but 5 steps at 600 K) has none in the double checker's run: there the two rules
    agree, and the comparison is one more 2-cell state at the largest radius allowed.  Neither state was in a strain test before."""
    found = {}
    for name in IMAGE_MAY_DECIDE:
        r = _reference(orc, name)
        found[name] = _differing(r["sk"]["r"], _extent(r["st"]), r["s0"]["r"], _extent(r["st"]), r["rc"])
        print(f"{name} at the cutoff: {found[name][0]} of {found[name][1]} ordered pairs take another image")
    assert found["eam_hot"][0] > 0
    assert SINGLE or (found["eam_hot"][0], found["eam_tight"][0]) == (18, 0), found


def _histories_of_test_atomic_strain(orc, name):
    """(what, pos, box, ref, box0) of test_atomic_strain's histories on the checker's positions of a state of its NAMES (the checker has the state's lattice and -r; the
    image of a pair does not hang on the potential): the homogeneous deformation, the rigid translation, the restatement history"""
    st = tas.STATES[name]
    o = orc.Oracle(st["n"], eam=1 if st["pair"] == "eam" else 0, delta=0.1, lat=st["lat"], lj_cutoff_sigmas=5.0 if st["pair"] == "eam" else st["rc"] / SIGMA)
    box0 = tas._extent(st)
    r0 = o.gather(orc.R).copy()
    o.step(10)
    r10 = o.gather(orc.R).copy()
    o.step(10)
    r20 = o.gather(orc.R).copy()
    o.close()
    scale = np.array(strain.SCALE)
    moved = r20 * scale
    moved[7] += strain.MOVE
    wrapped = np.mod(r0 + np.array([2.1, -1.9, 2.3]), box0)
    return [("homogeneous", r10 * scale, box0 * scale, r10, box0), ("translation", wrapped, box0, r0, box0), ("restatement", moved, box0 * scale, r0, box0)]


@pytest.mark.parametrize("name", strain.NAMES)
def test_default_image_rule_changes_no_comparison_of_test_atomic_strain(orc, name):
    """The states of test_atomic_strain.NAMES under its histories, at both radii: the two rules choose the same integer image for every accepted pair, so d0 -- and
    with it every existing comparison -- is unchanged to the bit."""
    st = tas.STATES[name]
    for what, pos, box, ref, box0 in _histories_of_test_atomic_strain(orc, name):
        for rs in (strain._default_rs(st["lat"]), st["rc"]):
            differ, pairs = _differing(pos, box, ref, box0, rs)
            print(f"{name} {what} radius {rs:.4f}: {differ} of {pairs}")
            assert differ == 0 and pairs > 0, (name, what, rs, differ)


def test_default_image_rule_changes_nothing_on_the_other_states(orc):
    """The states of parts 1 to 3 (IMAGE_MAY_DECIDE at the cutoff radius aside: test_where_else_the_image_rules_can_differ): the two-cell states at both radii, the straining shapes under both histories (the checker's
    steps, scaled with the box), the density regimes at the cutoff (their strain radius): the two rules choose the same image for every accepted pair."""
    for name in sorted({n for n, _ in TWO_CELL}):
        r = _reference(orc, name)
        for key, rs in (("default", strain._default_rs(r["st"].lat)), ("cutoff", r["rc"])):
            if key == "cutoff" and name in IMAGE_MAY_DECIDE:
                continue
            differ, pairs = _differing(r["sk"]["r"], _extent(r["st"]), r["s0"]["r"], _extent(r["st"]), rs)
            print(f"{name} {key}: {differ} of {pairs}")
            assert differ == 0 and pairs > 0, (name, key, differ)
    for pot, n, rc in (("lj", (8, 8, 8), 2.5 * SIGMA), ("eam", (10, 8, 6), 4.95)):
        o = orc.Oracle(n, eam=int(pot == "eam"), delta=0.1, temperature=600.0, lj_cutoff_sigmas=5.0 if pot == "eam" else 2.5)
        box0 = np.array(n, dtype=np.float64) * 3.615
        r0 = o.gather(orc.R).copy()
        o.step(5)
        r5 = o.gather(orc.R).copy()
        o.step(15)
        r20 = o.gather(orc.R).copy()
        o.close()
        for what, pos, scale in (("rate", r20, 1.0 + np.array(RATES) * 0.02), ("set_box", r5, np.array(strain.SCALE))):
            for rs in (strain._default_rs(3.615), rc):
                differ, pairs = _differing(pos * scale, box0 * scale, r0, box0, rs)
                print(f"{pot} {what} radius {rs:.4f}: {differ} of {pairs}")
                assert differ == 0 and pairs > 0, (pot, what, rs, differ)
    for name in regimes.ALL:
        if name in regimes.PAIR_ONLY or name == "lj_void":              # no strain leg there; no pair at all
            continue
        r = dr._reference(orc, name)
        box = regimes._box(r["g"])
        differ, pairs = _differing(r["sk"]["r"].astype(np.float64), box, r["s0"]["r"].astype(np.float64), box, r["rc"])
        print(f"{name}: {differ} of {pairs}")
        assert differ == 0 and pairs > 0, (name, differ)


# ================================================================ 1. GPU: two-cell boxes
@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,steps", TWO_CELL, ids=[f"{n}-step{k}" for n, k in TWO_CELL])
def test_fields_on_two_cell_boxes(gpu, orc, name, steps, method):
    """Stress, heat flux and strain of every atom on a 2-cell grid, where the stencil walk meets a neighbour cell twice and (EAM) reads F' of a halo slot through two
    images of one cell.  eam_hot at the cutoff radius is a state where the image of d0 decides (part 4)."""
    ref = _reference(orc, name)
    st = ref["st"]
    box = _box(st)
    what = f"{name} {method} step {steps}"
    with gpu.Simulation(_flags(st, method)) as sim:
        assert sim.grid == st.grid and np.array_equal(sim.box, box)
        if not SINGLE:
            assert np.array_equal(sim.gather(0), ref["s0"]["r"])
        sim.set_strain_reference()
        pos0 = sim.gather(0).copy()
        if steps == 0:
            _check_fields(sim, what, st.eam, box)
            _check_zero_strain(sim, what, pos0, box)
        else:
            sim.step(steps)
            pos = _check_fields(sim, what, st.eam, box)
            _check_strain(sim, what, pos, box, pos0, box)


# ================================================================ 2. GPU: a straining box, from Python
@pytest.mark.gpu
@pytest.mark.parametrize("pot,history,extra", STRAINED, ids=[f"{p}-{h}" + ("-langevin-a1-H" if e else "") for p, h, e in STRAINED])
def test_fields_on_a_straining_box(gpu, pot, history, extra):
    """(rate) reference, a strain rate of (1, -0.5, 0.25) / ps, 20 steps; (set_box) reference, set_box to test_atomic_strain.SCALE -- at once the strain is the
    homogeneous answer -- then 5 steps.  The checks of part 1 with sim.box as the extent and sim.strain_reference_box as box0.  The per-atom energies of the potential
    columns come from numpy at the current box: e[] left at the old geometry fails here."""
    what = f"{pot} {history}" + (" langevin -a 1 -H" if extra else "")
    with gpu.Simulation(POTS[pot] + HOT + list(extra)) as sim:
        sim.set_strain_reference()
        pos0, box0 = sim.gather(0).copy(), sim.box
        assert np.array_equal(sim.strain_reference_box, box0)
        if history == "rate":
            sim.set_strain_rate(RATES)
            sim.step(20)
            s = sim.box / box0
            assert np.abs(s - (1.0 + 0.02 * np.array(RATES))).max() <= (1e-6 if SINGLE else 1e-12), s
        else:
            sim.set_box(box0 * np.array(strain.SCALE))
            n = sim.n_global
            if SINGLE:
                s = sim.box / sim.strain_reference_box
                assert np.abs(s - np.array(strain.SCALE)).max() <= 4.0 * tas.EPS24
                want = np.zeros((n, 6))
                want[:, :3] = 0.5 * (s * s - 1.0)
            else:
                want = strain._homogeneous_answer(sim, n)
            _check_strain(sim, f"{what} homogeneous", sim.gather(0).copy(), sim.box, pos0, box0, want=(want, np.zeros(n)))
            _check_fields(sim, f"{what} before the steps", pot != "lj", sim.box)
            sim.step(5)
        box = sim.box
        assert np.array_equal(sim.strain_reference_box, box0) and np.abs(box / box0 - 1.0).max() > 5e-3
        volume = float(np.prod(box))
        assert abs(sim.volume - volume) <= (1e-6 if SINGLE else 1e-14) * volume and abs(sim.volume / float(np.prod(box0)) - 1.0) > 5e-3
        pos = _check_fields(sim, what, pot != "lj", box)
        assert np.array_equal(sim.heat_flux_density(), sim.heat_flux()["total"] / sim.volume)
        _check_strain(sim, what, pos, box, pos0, box0)


# ================================================================ 4. GPU: the image of a reference separation
IMAGE_CASES = [("strain_half", "thread_atom"), ("strain_half", "cta_cell"), ("eam_tight", "thread_atom")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,method", IMAGE_CASES, ids=[f"{n}-{m}" for n, m in IMAGE_CASES])
def test_strain_takes_the_image_the_pair_was_accepted_through(gpu, name, method):
    """Reference at step 0, the state's 5 steps, atomic_strain(cutoff=sim.cutoff) and strain_summary against the restatement with d0 through the image nearest the
    current separation, under the module's bound and C_BOUND.  A kernel that reduces d0 to the shortest image of L0 misses that bound by orders of magnitude (the CPU tests
    above: a shear strain of 0.04 where 0.001 is right)."""
    st = STRAIN_HALF if name == "strain_half" else STATES[name]
    box = _box(st)
    with gpu.Simulation(_flags(st, method)) as sim:
        assert sim.grid == st.grid and sim.n_global == st.atoms and np.array_equal(sim.box, box)
        sim.set_strain_reference()
        pos0 = sim.gather(0).copy()
        sim.step(st.steps)
        pos = sim.gather(0).copy()
        differ, pairs = _differing(pos, box, pos0, box, sim.cutoff)
        print(f"{name} {method}: {differ} of {pairs} ordered pairs of the run take another image than the shortest")
        assert differ >= (20 if name == "strain_half" else 0)              # (eam_tight: none in the double checker's run; the CPU tests say where the rules differ)
        _check_strain(sim, f"image {name} {method}", pos, box, pos0, box, radii={"cutoff": sim.cutoff})


# the GPU tests of this file (tests/test_single_precision.py runs them again in the float build and counts them)
GPU_CASE_COUNT = len(TWO_CELL) * len(METHODS) + len(STRAINED) + len(IMAGE_CASES)
