"""The analysis kernels on sparse, void and dense states: the virial, the pair histogram, centro-symmetry, common neighbour analysis, per-atom stress,
per-atom strain (with the two device reductions) and the heat flux in the eight regimes of tests/test_density_regimes.py, where cells are empty, hold 1 to 4 atoms or
six waves of them, and atoms have no neighbour at all.

Every other test of these kernels runs where all cells are occupied and nearly evenly filled.  What hip/stencil_walk.h and hip/nearest12_walk.h do
there and nowhere else: chunks of 1 to 3 atoms replicated 16 times with idle lanes, stencil cells of no atoms, an atom whose sums stay empty, every atom
of a rank invalid for the strain reduction, a von Mises maximum decided by the "lowest gid of equals" rule alone.

This module adds no restatement.  It imports the regimes and the numpy restatements of test_pressure, test_rdf, test_csp, test_cna, test_atom_stress and
test_atomic_strain and applies their comparison rules and caps as they stand, on the positions gathered from the simulation under test:

  1. CPU: the figures of every regime (FIGURES) from the checker and the restatements, so that a changed regime cannot pass silently; the helpers that
     take three extents on a cube; the masked test_atomic_strain._assert_within on a made-up case; the state with a singular sum d0 d0^T.
  2. GPU: every analysis in every regime at step 0 and after the regime's steps under thread_atom; after the steps under the other layouts too.
  3. GPU: the message halo against the mirrored halo, bit for bit; two ranks against one; one comd-hip run with every analysis flag.

COMD_PRECISION=single runs the module on the float build, as tests/test_msd.py, with each imported module's float rule; tests/test_single_precision.py
runs its GPU tests there and counts them (GPU_CASE_COUNT).

What the states, not the kernels, decide -- each shown in numpy alone by a CPU test of this module, none scaled to what the device returned:
  D^2min in the sparse regimes  the kernel forms D^2 = S - F : A in one pass; F carries a relative error of eps kappa(V_i).  Where atoms fit F to 3 to 10 neighbours (kappa up to
                                1.8e5) numpy's own one-pass form in double misses test_atomic_strain's bound (n + 64) eps S 20 to 500 times and stays within 0.04 of that bound
                                times kappa.  The regimes of D2_BY_KAPPA hold D^2 to the bound times kappa, with the module's C_BOUND; the others to the bound as it stands.
  float build, CSP              FLOAT_LEFT_OUT: the coordination at r_coord = the cutoff leaves out 62 / 58 atoms of eam_dense and 2 of eam_void at step 0 (caps 10 and 1.6).
  float build, stress           FLOAT_STRESS_LEFT_OUT: the restatement's own pair function in float32 misses the float rule 1.6 to 7.4 times in eam_void and eam_sparse.

Largest error / bound observed on an MI355X when the module was written, double | float build (every test prints its own as RATIO lines; no bound is fitted to them):
  virial W, K                   0.019, 0.0035 | 0.082, 0.013             histogram       exact | cumulative counts off by <= 3, near-edge pairs <= 5795 of 4.6e6 (cap 23058)
  csp                           7.2e-5 | 4.5e-4, left out 0 | <= 1       CNA             no wrong type, none left out
  stress pair / kinetic part    0.019, 0.66 | 0.55, 0.70                 rows against -W, -(K + W)    2.1e-4, 0.030 | 6.9e-3, 5.2e-3
  stress reduction              means 3.1e-4, extremes 0.021 | 2.9e-4, 0.021
  strain E, D^2 (C = 1)         0.11, 0.087 | 4.2e-3, 9.6e-4             strain reduction             means 7.8e-4, extremes 0.019 | 6.5e-4, 0
  heat flux columns             kinetic 0.47, potential 6.4e-3, virial 0.018 | 0.40, 0.48, 0.42           sums against the rows 0.33 | 0; two ranks 1.2e-4 | 6.4e-3

The heat-flux leg (_check_heat_flux; lj_dense stays PAIR_ONLY, it is state A of test_heat_flux) runs wherever the stress leg runs: in the regimes at both stages, the layouts,
the message halo (nine planes and four sums), two ranks (tests/heatflux_worker.py) and the executable (--heatflux).  Its rules are test_heat_flux.py's, with the per-atom
energies of the potential columns from an all-pairs sum in numpy, not from gather(3).  An atom without a neighbour has B_i = 0 and virial columns exactly 0 (every atom of
lj_void, whose potential columns are exactly 0 too); the 20 such atoms of eam_void carry F(0) v_i, and F(0) = 0 for Cu_u6.eam.  In the float build the virial columns
inherit FLOAT_STRESS_LEFT_OUT: a CPU test puts the float pair function through -s_i v_i with the checker's momenta (FLOAT_FLUX_FACTORS).

Bounds that are not an imported module's, with the reasoning (none is fitted to a measurement):
  K against sum p p^T / m       1e-12 of the largest component (float build 1e-5, the float rule of the virial): a sum of at most 8736 products in double,
                                each rounded to 2^-53.
  kinetic part of a row         test_atom_stress.py::test_kinetic_part_is_minus_p_p_over_m: 1e-12 |p_a p_b / m| + 2^-53 (|s1| + |s0|) (float build 1e-5 and 2^-24:
                                the mass comes from the float kinetic energy).
  rows of s1 against -(K + W)   test_atom_stress's 1e-11 sum A_i, plus N 2^-53 sum |p_a p_b| / m: where atoms have no or few neighbours A is 0 or tiny, and
                                what is left is the rounding of two sums of N kinetic terms taken in different orders.
"""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import test_atom_stress as stress
import test_atomic_strain as strain
import test_cna as cna
import test_csp as csp
import test_density_regimes as dr
import test_rdf as rdf
from test_density_regimes import HOT, REGIMES, _extent, _flags, _make, _neighbour_counts
from test_pressure import CSRC, EPS as LJ_EPS, HERE, ROOT, SIGMA, SINGLE, TOL, _child, _interpolate, _pairs, _rel, _tensor

DELTA = rdf.DELTA32 if SINGLE else rdf.DELTA64
EPS_REAL = stress.EPS24 if SINGLE else stress.EPS53
REAL = np.float32 if SINGLE else np.float64
BINS = 64
BINS_LJ_DENSE_STEP0 = 63         # 64 bins put one reference pair of lj_dense at step 0 within DELTA64 of an edge; 63 is the largest count <= 64 that puts none (CPU test)
ALL = list(REGIMES)
PAIR_ONLY = ("lj_dense",)        # the virial and the histogram only: CNA alone costs 50 s of numpy there, stress and strain have it as state A of test_atom_stress
STAGES = ("step0", "after")

# The figures of the regimes in the double build, from the checker and the restatements (strain radius = the cutoff, reference = step 0, 64 bins up to the cutoff):
# neighbours per atom (fewest, most), atoms with none, with fewer than 3, with fewer than 12, unordered histogram pairs, reference pairs within DELTA64 of an edge --
# each as (step 0, after the steps) -- the type CNA gives every atom, the atoms invalid for the strain after the steps (all of them by n < 3), the smallest
# det / t^3 of a valid atom and the largest condition number of one (both to two digits).
FIGURES = {
    "lj_void":    dict(atoms=144,  nbr=((0, 0), (0, 0)),             none=(144, 144), few3=(144, 144), few12=(144, 144), pairs=(0, 0),             near=(0, 0), cna="other", invalid=144,  det=None,   kappa=None),
    "lj_sparse":  dict(atoms=240,  nbr=((2, 8), (2, 7)),             none=(0, 0),     few3=(6, 4),     few12=(240, 240), pairs=(614, 610),         near=(0, 0), cna="other", invalid=4,    det=2.0e-5, kappa=1.8e5),
    "lj_dilute":  dict(atoms=600,  nbr=((54, 54), (53, 54)),         none=(0, 0),     few3=(0, 0),     few12=(0, 0),     pairs=(16200, 16198),     near=(0, 0), cna="fcc",   invalid=0,    det=0.99,   kappa=1.1),
    "lj_dense":   dict(atoms=8736, nbr=((1042, 1060), (1052, 1060)), none=(0, 0),     few3=(0, 0),     few12=(0, 0),     pairs=(4604193, 4611631), near=(1, 0), cna=None,    invalid=None, det=None,   kappa=None),
    "eam_void":   dict(atoms=320,  nbr=((0, 6), (0, 9)),             none=(20, 1),    few3=(185, 15),  few12=(320, 320), pairs=(360, 775),         near=(0, 0), cna="other", invalid=15,   det=2.7e-5, kappa=1.3e5),
    "eam_sparse": dict(atoms=480,  nbr=((2, 10), (1, 9)),            none=(0, 0),     few3=(2, 12),    few12=(480, 480), pairs=(1340, 1231),       near=(0, 0), cna="other", invalid=12,   det=5.1e-5, kappa=7.8e4),
    "eam_dilute": dict(atoms=600,  nbr=((12, 12), (12, 12)),         none=(0, 0),     few3=(0, 0),     few12=(0, 0),     pairs=(3600, 3600),       near=(0, 0), cna="fcc",   invalid=0,    det=0.99,   kappa=1.1),
    "eam_dense":  dict(atoms=2016, nbr=((116, 134), (119, 134)),     none=(0, 0),     few3=(0, 0),     few12=(0, 0),     pairs=(127526, 129145),   near=(0, 0), cna="fcc",   invalid=0,    det=0.98,   kappa=1.3),
}
# The float build: the float checker's figures above are the same, after the steps too, and are asserted in both builds.  A leg whose reference alone exceeds a cap of
# the float rules is left out of the float leg here, by regime and stage, with the count found: the coordination at r_coord = the cutoff leaves out the atoms with a
# neighbour within DELTA32 = 1e-4 A of it, and the cap on those is 0.5 % of the atoms.  Only the centro-symmetry leg is left out; the regime's other five legs run.
FLOAT_LEFT_OUT = {("eam_void", 0): 2, ("eam_dense", 0): 62, ("eam_dense", 1): 58}          # (regime, stage): atoms left out; the caps are 1.6 and 10.08
# The float rule of the per-atom stress, (n + 64) 2^-24 A, allows 64 roundings per pair term.  In the sparse EAM regimes the few neighbours sit at 4.5 to 4.95 A, the last
# samples of tables that end at 4.95 A, where a table's value is up to 1e3 times the difference of two neighbouring samples that its derivative is read from: in float the
# restatement's own pair function (test_pressure._interpolate on float32 tables and distances, numpy alone) misses that bound by the factors below at (step 0, after the
# steps).  In the float leg the comparison of the pair part with the restatement is left out in these regimes, by name; what does not hang on that bound stays (atoms
# without neighbours exactly 0, the kinetic part, the rows against virial(), the reduction against numpy).
FLOAT_STRESS_LEFT_OUT = {"eam_void": (7.4, 1.9), "eam_sparse": (4.0, 1.6)}
# The virial columns of the heat flux are -s_i v_i, so their float comparison inherits the omission.  The same float pair function through -s_i v_i with the checker's
# momenta against (n + 64) 2^-24 B (the CPU test that shows the factors above), double checker's positions at (step 0, after the steps); the float checker's give
# 7.4, 0.26 and 1.5, 0.57.
FLOAT_FLUX_FACTORS = {"eam_void": (7.2, 0.71), "eam_sparse": (0.86, 0.36)}
# Regimes in which the one-pass form of D^2 (S - F : A, the kernel's) misses test_atomic_strain's bound (n + 64) eps S when evaluated in numpy in double on the checker's
# positions, by the conditioning of the state alone (CPU test below): there D^2 is held to that bound times kappa(V_i), the factor the bound on E carries already.
D2_BY_KAPPA = ("lj_sparse", "eam_void", "eam_sparse")


def _box(g):
    """the extents as the build under test holds them"""
    if SINGLE:
        return (np.array(g.n, dtype=np.float32) * np.float32(g.lat)).astype(np.float64)
    return _extent(g)


def _bins(name, stage):
    return BINS_LJ_DENSE_STEP0 if (name, stage) == ("lj_dense", "step0") and not SINGLE else BINS


def _edges(bins, rc):
    return np.arange(bins + 1, dtype=np.float64) * (rc / bins)


def _counts_of(pos, box, rc):
    nbr = _neighbour_counts(pos, box, rc)
    return dict(nbr=(int(nbr.min()), int(nbr.max())), none=int((nbr == 0).sum()), few3=int((nbr < 3).sum()), few12=int((nbr < 12).sum()))


def _assert_worth_running(name, k, pos, box, rc, occupancy, exact, regular_cells=True):
    """the figures that make the state worth running, from the gathered positions and the run's own occupancies, before anything is compared: in the double build at step 0
    the table's own (the positions are the checker's, to the bit), else that atoms without neighbours, with fewer than 3 and fewer than 12 occur where the table has them"""
    fig, got = FIGURES[name], _counts_of(pos, box, rc)
    print(f"{name} {STAGES[k]}: {got}, empty local cells {int((occupancy == 0).sum())}, occupancy {int(occupancy.min())}-{int(occupancy.max())}")
    assert int(occupancy.sum()) == fig["atoms"] == len(pos)
    if REGIMES[name].empty and regular_cells:                          # (thread_atom_nl and -L size their cells for cutoff + skin)
        assert (occupancy == 0).any()
    if exact:
        assert got == {key: fig[key][k] for key in got}, (name, got)
    for key in ("none", "few3", "few12"):
        assert (got[key] > 0) == (fig[key][k] > 0), (name, key, got[key])
    if fig["few12"][k] == fig["atoms"]:
        assert got["few12"] == fig["atoms"]
    return got


# ================================================================ the restatements of one state, under the imported rules
def _virial_reference(sim, pos, box, rc, eam):
    """test_pressure.py's restatements at the positions of the run (test_lj_tensor_matches_the_restatement, test_eam_setfl_tensor_matches_the_restatement)"""
    i, j, d, r = _pairs(pos, box, rc)
    if eam:
        df = sim.gather(5)
        s = (_interpolate(*sim.eam_table(0), r)[1] + (df[i] + df[j]) * _interpolate(*sim.eam_table(1), r)[1]) / r
        return _tensor(d, -s[:, None] * d), len(r)
    s6 = SIGMA ** 6
    fr = 24.0 * LJ_EPS * s6 * r ** -8 * (2.0 * s6 * r ** -6 - 1.0)
    return _tensor(d, fr[:, None] * d), len(r)


def _kinetic(sim):
    """(-p p^T / m per atom as six components, sum p p^T / m as a 3 x 3 tensor, m), m from the kinetic energy as test_atom_stress.py has it"""
    p = sim.gather(1)
    mass = (p * p).sum() / (2.0 * sim.energy()[1])
    rows = -np.stack([p[:, a] * p[:, b] for a, b in stress.COMP], axis=1) / mass
    return rows, np.einsum("ia,ib->ab", p, p) / mass, mass


RATIOS = {}


def _ratio(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


def _check_virial(sim, name, what, pos, box, rc):
    g = REGIMES[name]
    w, k = sim.virial()
    want, n_pairs = _virial_reference(sim, pos, box, rc, g.eam)
    _, k_want, _ = _kinetic(sim)
    assert np.array_equal(w, w.T) and np.array_equal(k, k.T)
    if n_pairs == 0:
        assert name == "lj_void" and not want.any()
        assert all(w[a, b] == 0.0 for a, b in stress.COMP), w          # no pair at all: exactly 0, not a sum of roundings
        err_w = 0.0
    else:
        err_w = _rel(w, want)
    err_k = _rel(k, k_want)
    print(f"RATIO virial {what}: W {err_w / (1e-5 if SINGLE else 1e-11):.4g} K {err_k / (1e-5 if SINGLE else 1e-12):.4g} (pairs {n_pairs // 2})")
    _ratio("virial W", err_w / (1e-5 if SINGLE else 1e-11))
    _ratio("virial K", err_k / (1e-5 if SINGLE else 1e-12))
    assert err_w <= (1e-5 if SINGLE else 1e-11), (what, w, want)
    assert err_k <= (1e-5 if SINGLE else 1e-12), (what, k, k_want)
    return w, k


def _check_histogram(sim, name, what, pos, box, rc, bins):
    edges, counts = sim.pair_histogram(bins)
    assert edges.shape == (bins + 1,) and counts.dtype == np.int64 and abs(edges[-1] - rc) <= 1e-15 * rc
    cum, near = rdf._reference(object(), pos, box, edges, DELTA)
    r, g = sim.rdf(bins)
    if cum[-1] == 0:
        # rdf._check asserts that there are pairs; with none every count is 0 and g(r) is 0 / ideal, finite
        assert name == "lj_void" and near.sum() == 0
        assert not counts.any() and np.all(np.isfinite(g)) and not g.any()
    else:
        rdf._check(counts, cum, near, SINGLE, what)
        n, dr_, k = float(sim.n_global), edges[-1] / bins, np.arange(bins, dtype=np.float64)
        ideal = (0.5 * n) * (n / (box[0] * box[1] * box[2])) * (4.0 * np.pi / 3.0 * dr_ * dr_ * dr_) * ((k + 1.0) ** 3 - k ** 3)
        assert np.all(np.abs(g - counts / ideal) <= (1e-6 if SINGLE else 1e-14) * (counts / ideal)), np.abs(g - counts / ideal).max()
    return counts


def _check_csp(sim, name, what, pos, box, rc):
    c, coord = sim.centro_symmetry(r_coord=rc)
    ref = csp._numpy_csp(pos, box, rc, rc, DELTA)
    csp._check(c, coord, ref, SINGLE, what)
    no_csp, no_coord = csp._left_out(ref, DELTA, SINGLE)
    few = ref["coord"] < 12
    assert np.all(np.isinf(c[few & ~no_coord & ~no_csp])) and np.all(c[np.isinf(c)] > 0)
    bad = sim.defects(r_coord=rc)
    want = np.nonzero(ref["csp"] > 0.25 * sim.lattice_constant ** 2)[0]
    if not SINGLE:
        assert np.array_equal(coord, ref["coord"])                     # coordination at the cutoff is the restatement's neighbour count
        assert np.array_equal(np.isinf(c), few)
        assert np.array_equal(bad, want), what
    assert set(np.nonzero(few & ~no_coord & ~no_csp)[0].tolist()) <= set(bad.tolist())
    finite = np.isfinite(ref["csp"]) & ~no_csp
    if finite.any():
        _ratio("csp", (np.abs(c[finite] - ref["csp"][finite]) / ((5e-3 + 1e-5 * ref["csp"][finite]) if SINGLE else (1e-10 + 1e-12 * ref["csp"][finite]))).max())
    return c, coord


def _check_cna(sim, name, what, pos, box, rc):
    types = sim.common_neighbor_analysis()
    ref = cna._numpy_cna(pos, box, rc, DELTA)
    cna._check(types, ref, SINGLE, what)
    counts = sim.structure_counts()
    assert counts == cna._counts(types)
    if not cna._left_out(ref, DELTA, SINGLE).any():
        assert counts == cna._counts(ref["type"])
        if not SINGLE:
            assert counts[FIGURES[name]["cna"]] == FIGURES[name]["atoms"], (what, counts)
    return types


def _numpy_stress_summary(s, omega):
    p = -(s[:, 0] + s[:, 1] + s[:, 2]) / (3.0 * omega)
    return p, stress._von_mises(s) / omega


def _check_stress_summary(sim, what, s, kinetic):
    """test_atom_stress.py::test_summary_is_numpy_on_the_array: means to 1e-12 relative, extremes to 1e-14 relative, the gid of the maximum -- the lowest of equals; where
    the two largest differ by less than that margin without being equal, the gid may be either"""
    got, omega = sim.stress_summary(kinetic=kinetic), sim.atomic_volume
    p, vm = _numpy_stress_summary(s, omega)
    order = np.sort(vm)
    assert got["n"] == len(s)
    if order[-1] == order[-2] or order[-1] - order[-2] > 1e-14 * order[-1]:
        assert got["max_von_mises_gid"] == int(np.argmax(vm)), (what, got["max_von_mises_gid"], int(np.argmax(vm)))
    else:
        assert vm[got["max_von_mises_gid"]] >= order[-2]
    for key, want, tol in (("mean_pressure", p.mean(), 1e-12), ("mean_von_mises", vm.mean(), 1e-12), ("min_pressure", p.min(), 1e-14),
                           ("max_pressure", p.max(), 1e-14), ("max_von_mises", vm.max(), 1e-14)):
        if want != 0.0:
            _ratio(f"stress summary {key.split('_')[0]}", abs(got[key] - want) / (tol * abs(want)))
        assert abs(got[key] - want) <= tol * abs(want), (what, key, got[key], want)
    return got


def _check_stress(sim, name, what, pos, box, rc, w, k):
    g = REGIMES[name]
    fr_of = stress._pair_function("eam", sim.eam_table(0), sim.eam_table(1), sim.gather(5).copy()) if g.eam else stress._pair_function("lj")
    want, big_a, cnt = stress._restate(pos, box, rc, fr_of)
    s0, s1 = sim.atomic_stress(kinetic=False), sim.atomic_stress(kinetic=True)
    assert s0.shape == (len(pos), 6) and s0.dtype == np.float64
    bound = ((cnt[:, None] + 64.0) * stress.EPS24 * big_a) if SINGLE else 1e-11 * big_a
    lone = cnt == 0
    assert not big_a[lone].any()
    if not (SINGLE and name in FLOAT_STRESS_LEFT_OUT):
        stress._assert_close(s0, want, bound, f"{what} pair part")
    assert not s0[lone].any()                                           # no neighbour: the virial part is exactly 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0.0, np.abs(s0 - want) / np.where(bound > 0.0, bound, 1.0), 0.0)
    if not (SINGLE and name in FLOAT_STRESS_LEFT_OUT):
        _ratio("stress", ratio.max())
    kin, _, _ = _kinetic(sim)
    floor = EPS_REAL * (np.abs(s1) + np.abs(s0))
    stress._assert_close(s1 - s0, kin, (1e-5 if SINGLE else 1e-12) * np.abs(kin) + floor, f"{what} kinetic part")
    # the rows add up to -W and -(K + W) of virial(): test_rows_add_up_to_the_virial (float build: test_single_precision_build's sum rule)
    w6, k6 = stress._six(w), stress._six(k)
    total = (2.0 * bound.sum(0) + stress.EPS24 * np.abs(w6)) if SINGLE else 1e-11 * big_a.sum(0)
    stress._assert_close(s0.sum(0), -w6, total, f"{what} rows against -W")
    kinetic_sums = (1e-5 if SINGLE else len(pos) * stress.EPS53) * np.abs(kin).sum(0)
    stress._assert_close(s1.sum(0), -(k6 + w6), total + kinetic_sums, f"{what} rows against -(K + W)")
    summary0 = _check_stress_summary(sim, f"{what} kinetic=False", s0, False)
    summary1 = _check_stress_summary(sim, f"{what} kinetic=True", s1, True)
    if name == "lj_void":
        # every von Mises stress is 0: the gid is decided by the "lowest gid of equals" rule alone, across the workgroups of the reduction
        assert not s0.any()
        assert summary0 == {"mean_pressure": 0.0, "min_pressure": 0.0, "max_pressure": 0.0, "mean_von_mises": 0.0, "max_von_mises": 0.0, "max_von_mises_gid": 0, "n": 144}
    return s0, s1, summary0, summary1, (want, big_a, cnt)


def _check_heat_flux(sim, name, what, pos, box, rc, restated):
    """The rules of test_heat_flux.py's docstring on the restatement _check_stress has made (want, A, n): the virial columns against -s_i v_i within 1e-11 B_i,a (float
    build (n_i + 64) 2^-24 B_i,a; the regimes of FLOAT_STRESS_LEFT_OUT aside, as the stress they are made of), and exactly 0 for an atom without a neighbour, whose B is
    0; the kinetic columns by test_heat_flux._convective; the potential columns against e_ref,i v_i with e_ref from the all-pairs sums of test_density_regimes on the
    gathered positions -- not gather(3), the array the kernel reads -- within (per_atom_energy_abs + 8 eps (|e_i| + ke_i)) |v_i,a|; heat_flux() against the column sums
    (test_reduction_is_the_sum_of_the_rows, k from the run); heat_flux_density().  lj_void: every potential and virial column is exactly 0.  An EAM atom without
    a neighbour carries F(0) v_i."""
    import math
    import test_heat_flux as hf
    g = REGIMES[name]
    want, big_a, cnt = restated
    mom, mass = sim.gather(1).copy(), sim.mass
    v = mom / mass
    assert np.abs(v).min() > 0.0                                        # no velocity component is 0: every column is there to be seen
    j, sums = sim.atomic_heat_flux(), sim.heat_flux()
    assert j.shape == (len(pos), 9) and j.dtype == np.float64
    lone = cnt == 0
    b = hf._times_v(big_a, np.abs(v))
    assert not b[lone].any() and np.all(b[~lone] > 0.0)                 # B_i = 0 for the atoms without a neighbour and for no other (test_figures_of_the_regimes counts them)
    bound = ((cnt[:, None] + 64.0) * stress.EPS24 * b) if SINGLE else 1e-11 * b
    assert not j[lone, 6:9].any()                                       # no neighbour: the virial columns are exactly 0
    if not (SINGLE and name in FLOAT_STRESS_LEFT_OUT):
        stress._assert_close(j[:, 6:9], -hf._times_v(want, v), bound, f"{what} heat flux, virial columns")
        with np.errstate(invalid="ignore", divide="ignore"):
            _ratio("heat flux virial", np.where(bound > 0.0, np.abs(j[:, 6:9] + hf._times_v(want, v)) / np.where(bound > 0.0, bound, 1.0), 0.0).max())
    if g.eam:
        tables = [sim.eam_table(which) for which in range(3)]
        e_ref = dr._eam_all_pairs(pos, box, rc, tables)[1]
        f0 = float(_interpolate(*tables[2], np.zeros(1))[0][0])
        assert np.all(e_ref[lone] == f0)                                # rhobar = 0: the atom carries F(0) v_i (Cu_u6.eam: F(0) = 0, so its potential columns are 0 too)
        if f0 == 0.0:
            assert not j[lone, 3:6].any()
    else:
        e_ref = np.asarray(dr._lj_all_pairs(pos, box, rc)[1], dtype=np.float64)
    jk, jp, mag = hf._convective(e_ref, mom, mass)
    tol = TOL["per_atom_energy_abs"]                                    # reference_values.json tolerances / tolerances_single
    stress._assert_close(j[:, 0:3], jk, 8.0 * EPS_REAL * mag, f"{what} heat flux, kinetic columns")
    stress._assert_close(j[:, 3:6], jp, tol * np.abs(v) + 8.0 * EPS_REAL * mag, f"{what} heat flux, potential columns")
    _ratio("heat flux kinetic", (np.abs(j[:, 0:3] - jk) / (8.0 * EPS_REAL * mag)).max())
    _ratio("heat flux potential", (np.abs(j[:, 3:6] - jp) / (tol * np.abs(v) + 8.0 * EPS_REAL * mag)).max())
    if name == "lj_void":
        assert lone.all() and not e_ref.any() and not j[:, 3:9].any()
    k = math.ceil(math.ceil(sim.n_local_boxes * math.ceil(sim.max_atoms / 64) / 2048) / 4)
    assert k == 1, (sim.n_local_boxes, sim.max_atoms)
    rows = np.abs(j).sum(0)
    for i, part in enumerate(("kinetic", "potential", "virial")):
        cols = slice(3 * i, 3 * i + 3)
        stress._assert_close(sums[part], j[:, cols].sum(0), (k + 2) * EPS_REAL * rows[cols], f"{what} heat flux, {part} sum")
        with np.errstate(invalid="ignore", divide="ignore"):
            _ratio("heat flux sums", np.where(rows[cols] > 0.0, np.abs(sums[part] - j[:, cols].sum(0)) / np.where(rows[cols] > 0.0, (k + 2) * EPS_REAL * rows[cols], 1.0), 0.0).max())
    total = j[:, 0:3].sum(0) + j[:, 3:6].sum(0) + j[:, 6:9].sum(0)
    stress._assert_close(sums["total"], total, (k + 3) * EPS_REAL * (rows[0:3] + rows[3:6] + rows[6:9]), f"{what} heat flux, total")
    assert np.array_equal(sums["total"], (sums["kinetic"] + sums["potential"]) + sums["virial"])
    assert np.array_equal(sim.heat_flux_density(), sums["total"] / sim.volume)
    return j, sums


def _check_strain_summary(sim, what, got, m, rc):
    """strain_summary against numpy on the valid atoms of atomic_strain() under the rules of test_atomic_strain.py::test_summary_is_numpy_on_the_arrays; with no valid
    atom: what comdStrainSummary writes for N = 0"""
    e, d2, cnt = got
    bad = np.isnan(e[:, 0])
    gamma, vol = strain._shear(e[~bad]), (e[~bad, 0] + e[~bad, 1] + e[~bad, 2]) / 3.0
    threshold = float(np.median(gamma)) if len(gamma) and np.median(gamma) > 0.0 else 0.1
    s = sim.strain_summary(cutoff=rc, threshold=threshold)
    assert s["n"] == len(e) and s["invalid"] == int(bad.sum()) == int(m["invalid"].sum())
    if bad.all():
        assert s == {"n": len(e), "invalid": len(e), "mean_shear": 0.0, "max_shear": 0.0, "max_shear_gid": -1, "mean_volumetric": 0.0, "mean_d2min": 0.0,
                     "max_d2min": 0.0, "above_threshold": 0}, s
        return s
    order = np.sort(gamma)
    assert s["above_threshold"] == int((gamma >= threshold).sum())
    if len(order) < 2 or order[-1] == order[-2] or order[-1] - order[-2] > 1e-14 * order[-1]:
        assert s["max_shear_gid"] == int(np.nonzero(~bad)[0][np.argmax(gamma)])
    for key, want, tol in (("mean_shear", gamma.mean(), 1e-12), ("mean_volumetric", vol.mean(), 1e-12), ("mean_d2min", d2[~bad].mean(), 1e-12),
                           ("max_shear", gamma.max(), 1e-14), ("max_d2min", d2[~bad].max(), 1e-14)):
        scale = abs(want)
        if scale > 0.0:
            _ratio(f"strain summary {key.split('_')[0]}", abs(s[key] - want) / (tol * scale))
        assert abs(s[key] - want) <= tol * scale, (what, key, s[key], want)
    return s


def _check_strain(sim, name, what, pos, box, rc, ref, box0):
    m = strain._restate(pos, box, ref, box0, rc, dtype=REAL)
    got = sim.atomic_strain(rc)
    eps = strain._eps(m, "single" if SINGLE else "double", box)
    strain._assert_within(f"regimes {what}", got, m["e"], m["d2"], m, eps, invalid=m["invalid"], d2_by_kappa=name in D2_BY_KAPPA)
    if (~m["invalid"]).any():
        _ratio("strain E", strain.RATIOS[f"regimes {what}"][0])
        _ratio("strain D2", strain.RATIOS[f"regimes {what}"][1])
    summary = _check_strain_summary(sim, what, got, m, rc)
    return got, summary, m


def _analyse(sim, name, k, what, reference=None, exact=False, regular_cells=True):
    """every check of the module on the current state of `sim`; returns what the bit-for-bit and rank comparisons need"""
    g = REGIMES[name]
    pos, box, rc = sim.gather(0).copy(), sim.box, sim.cutoff
    assert np.array_equal(box, _box(g)), (box, _box(g))
    assert rc < 0.5 * box.min()                                        # the restatements' minimum image is the kernels'
    occupancy = sim.cells()["nAtoms"][:sim.n_local_boxes]
    _assert_worth_running(name, k, pos, box, rc, occupancy, exact, regular_cells)
    out = dict(pos=pos)
    out["w"], out["k"] = _check_virial(sim, name, what, pos, box, rc)
    out["counts"] = _check_histogram(sim, name, what, pos, box, rc, _bins(name, STAGES[k]))
    if name in PAIR_ONLY:
        return out
    if not (SINGLE and (name, k) in FLOAT_LEFT_OUT):
        out["csp"], out["coord"] = _check_csp(sim, name, what, pos, box, rc)
    out["cna"] = _check_cna(sim, name, what, pos, box, rc)
    out["s0"], out["s1"], out["stress_summary0"], out["stress_summary1"], restated = _check_stress(sim, name, what, pos, box, rc, out["w"], out["k"])
    out["j"], out["heat_flux"] = _check_heat_flux(sim, name, what, pos, box, rc, restated)
    if reference is not None:
        (out["e"], out["d2"], out["n"]), out["strain_summary"], out["m"] = _check_strain(sim, name, what, pos, box, rc, *reference)
    return out


# ================================================================ CPU
_CPU = {}
_MOMENTA = {}


def _cpu_momenta(orc, name):
    """the checker's momenta at step 0 and after the regime's steps (dr._reference keeps none); once per regime"""
    if name not in _MOMENTA:
        g = REGIMES[name]
        o = _make(orc, g)
        p0 = o.gather(orc.P).copy()
        o.step(g.steps)
        _MOMENTA[name] = (p0, o.gather(orc.P).copy())
        o.close()
    return _MOMENTA[name]


def _checker_pair_function(ref, snap):
    if ref["g"].eam:
        return stress._pair_function("eam", ref["tables"][0], ref["tables"][1], snap["df"])
    return stress._pair_function("lj")


def _cpu_figures(orc, name):
    """the figures of FIGURES from the checker's positions at step 0 and after the regime's steps, through the restatements alone; once per regime"""
    if name in _CPU:
        return _CPU[name]
    ref = dr._reference(orc, name)
    g, rc, box = ref["g"], ref["rc"], _box(ref["g"])
    states = (ref["s0"]["r"], ref["sk"]["r"])
    out = {key: [] for key in ("nbr", "none", "few3", "few12", "pairs", "near", "near32")}
    for pos in states:
        for key, v in _counts_of(pos, box, rc).items():
            out[key].append(v)
        cum, near = rdf._reference(object(), pos, box, _edges(BINS, rc), rdf.DELTA64)
        _, near32 = rdf._reference(object(), pos, box, _edges(BINS, rc), rdf.DELTA32)
        out["pairs"].append(int(cum[-1]))
        out["near"].append(int(near.sum()))
        out["near32"].append(int(near32.sum()))
    out["left_out"] = []
    if name not in PAIR_ONLY:
        types = []
        for pos in states:
            c = csp._numpy_csp(pos, box, rc, rc, DELTA)
            t = cna._numpy_cna(pos, box, rc, DELTA)
            out["left_out"].append((int(((c["gap"] < DELTA) | c["unsure"]).sum()), int((c["edge"] < DELTA).sum()), int((t["margin"] < DELTA).sum())))
            types.append(cna._counts(t["type"]))
        out["cna"] = types
        m = strain._restate(states[1], box, states[0], box, rc, dtype=REAL)
        valid = ~m["invalid"]
        out["invalid"] = int(m["invalid"].sum())
        out["invalid_by_count"] = int((m["n"] < 3).sum())
        out["det"] = float(m["det_ratio"][valid].min()) if valid.any() else None
        out["kappa"] = float(m["kappa"][valid].max()) if valid.any() else None
        # what decides the heat-flux leg: the atoms whose B_i = sum_b A_i,ab |v_i,b| is 0 (their virial columns must be exactly 0) and the velocity components that are 0
        import test_heat_flux as hf
        out["b_zero"], out["v_zero"] = [], []
        for pos, snap, p in zip(states, (ref["s0"], ref["sk"]), _cpu_momenta(orc, name)):
            _, big_a, _ = stress._restate(pos.astype(np.float64), box, rc, _checker_pair_function(ref, snap))
            b = hf._times_v(big_a, np.abs(p))
            assert np.array_equal((b == 0.0).any(1), (b == 0.0).all(1))
            out["b_zero"].append(int((b == 0.0).all(1).sum()))
            out["v_zero"].append(int((p == 0.0).sum()))
    _CPU[name] = out
    return out


@pytest.mark.parametrize("name", ALL)
def test_figures_of_the_regimes(orc, name):
    """Every figure of FIGURES again from the checker and the existing restatements, and the caps of the imported rules on the reference alone: they are conditions, not
    measurements.  Float build: the same figures from the float checker, the float caps, and the legs of FLOAT_LEFT_OUT exceed theirs by the counts written there."""
    fig, got = FIGURES[name], _cpu_figures(orc, name)
    g = REGIMES[name]
    print(name, got)
    assert g.atoms == fig["atoms"] and g.steps == (30 if name in HOT else 5)
    for k in (0, 1):
        for key in ("nbr", "none", "few3", "few12", "pairs"):
            assert got[key][k] == fig[key][k], (name, key, k, got[key][k], fig[key][k])
    for k in (0, 1):
        for key in ("none", "few3", "few12"):
            assert (got[key][k] > 0) == (fig[key][k] > 0), (name, key, k, got[key][k])
        if fig["few12"][k] == fig["atoms"]:
            assert got["few12"][k] == fig["atoms"]
    if SINGLE:
        for k in (0, 1):
            assert got["near32"][k] <= rdf.CAP32 * got["pairs"][k], (name, k, got["near32"][k], got["pairs"][k])
            if name not in PAIR_ONLY:
                no_csp, no_coord, no_cna = got["left_out"][k]
                assert max(no_csp, no_cna) <= csp.CAP32 * fig["atoms"], (name, k, got["left_out"][k])
                if (name, k) in FLOAT_LEFT_OUT:
                    assert no_coord == FLOAT_LEFT_OUT[(name, k)] > csp.CAP32 * fig["atoms"], (name, k, no_coord)       # left out for this, and for no less
                else:
                    assert no_coord <= csp.CAP32 * fig["atoms"], (name, k, got["left_out"][k])
    else:
        assert tuple(got["near"]) == fig["near"], (name, got["near"])
        if name not in PAIR_ONLY:
            assert got["left_out"] == [(0, 0, 0), (0, 0, 0)], (name, got["left_out"])          # CSP, coordination and CNA leave no atom out
    if name in PAIR_ONLY:
        return
    for counts in got["cna"]:
        assert counts[fig["cna"]] == fig["atoms"], (name, counts)
    # the heat-flux leg: B_i = 0 for the atoms without a neighbour and for no other (in lj_void that is every atom), and no velocity component is 0
    assert tuple(got["b_zero"]) == fig["none"] and got["v_zero"] == [0, 0], (name, got["b_zero"], got["v_zero"])
    assert got["invalid"] == got["invalid_by_count"]                    # none by the determinant: the singular state below is the one that is
    if not SINGLE:
        assert got["invalid"] == fig["invalid"], (name, got["invalid"])
    if fig["det"] is None:
        assert got["det"] is None and got["invalid"] == fig["atoms"]
    else:
        # (recorded to two digits) the smallest determinant of a valid atom is 1e4 thresholds away from the threshold: no decision is a rounding matter
        assert abs(got["det"] / fig["det"] - 1.0) <= 0.05 and abs(got["kappa"] / fig["kappa"] - 1.0) <= 0.05 and got["det"] > 1e4 * 1e-9, (name, got["det"], got["kappa"])


def _one_pass_d2(pos, box, ref, rc):
    """D^2 = S - F : A from the sums V, A, S over the pairs of _pairs, F = A adj(V) / det V: the one-pass form of hip/strain_kernels.h, in numpy in double"""
    i, j, d, _ = _pairs(pos, box, rc)
    n = len(pos)
    d = -d                                                              # x_j - x_i
    d0 = ref[j] - ref[i]
    d0 -= box * np.rint(d0 / box)
    v, a = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    for p in range(3):
        for q in range(3):
            v[:, p, q] = np.bincount(i, weights=d0[:, p] * d0[:, q], minlength=n)
            a[:, p, q] = np.bincount(i, weights=d[:, p] * d0[:, q], minlength=n)
    f, _ = strain._adjugate_fit(v, a)
    return np.bincount(i, weights=(d * d).sum(1), minlength=n) - (f * a).sum((1, 2))


@pytest.mark.parametrize("name", [n for n in ALL if n not in PAIR_ONLY and n != "lj_void"])
def test_one_pass_d2_misses_the_bound_without_kappa_by_the_state_alone(orc, name):
    """No device here.  The checker's state after the regime's steps against its step 0, D^2 twice in numpy in double: the direct form sum |d - F d0|^2 of
    test_atomic_strain._restate and the one-pass form S - F : A.  In the regimes of D2_BY_KAPPA, where atoms fit F to three to ten neighbours and kappa(V_i) reaches 1e5,
    the two differ by more than C_BOUND (n + 64) 2^-53 S -- 20 to 500 times that bound -- and by less than that bound times kappa; in the others the bound holds as it
    stands.  So the regimes of D2_BY_KAPPA, and only they, are held to the bound with kappa; C_BOUND is unchanged."""
    ref = dr._reference(orc, name)
    pos0, pos, box, rc = ref["s0"]["r"].astype(np.float64), ref["sk"]["r"].astype(np.float64), _box(ref["g"]), ref["rc"]
    m = strain._restate(pos, box, pos0, box, rc)
    ok = ~m["invalid"]
    bound = ((m["n"] + 64.0) * strain.EPS53 * m["s"])[ok]
    err = np.abs(_one_pass_d2(pos, box, pos0, rc) - m["d2"])[ok]
    plain, by_kappa = (err / bound).max(), (err / (bound * m["kappa"][ok])).max()
    print(f"{name}: one-pass D^2 in numpy against the direct form: error / bound {plain:.4g}, error / (bound kappa) {by_kappa:.4g}, kappa <= {m['kappa'][ok].max():.3g}")
    assert by_kappa <= strain.C_BOUND
    assert (plain > strain.C_BOUND) == (name in D2_BY_KAPPA), (name, plain)


@pytest.mark.parametrize("name", [n for n in ALL if n not in PAIR_ONLY])
def test_float_pair_function_alone_against_the_float_stress_bound(orc, name):
    """No device here.  On the checker's positions, test_atom_stress._restate twice: with the module's pair function in double, and with the same
    function handed float32 tables, F' and distances (numpy then evaluates it in float32, as the float build's kernel does).  Their difference against the float rule
    (n + 64) 2^-24 A: above the bound in the regimes of FLOAT_STRESS_LEFT_OUT, by the factors written there, and inside it in every other regime."""
    f32 = np.float32
    ref = dr._reference(orc, name)
    g, box, rc = ref["g"], _box(ref["g"]), ref["rc"]
    import test_heat_flux as hf
    worst, worst_b = [], []
    for snap, p in zip((ref["s0"], ref["sk"]), _cpu_momenta(orc, name)):
        pos = snap["r"].astype(np.float64)
        if g.eam:
            phi, rho, _ = ref["tables"]
            exact = stress._pair_function("eam", phi, rho, snap["df"])
            rounded = stress._pair_function("eam", (f32(phi[0]), f32(phi[1]), phi[2].astype(f32)), (f32(rho[0]), f32(rho[1]), rho[2].astype(f32)), snap["df"].astype(f32))
        else:
            exact = rounded = stress._pair_function("lj")
        want, big_a, cnt = stress._restate(pos, box, rc, exact)
        got, _, _ = stress._restate(pos, box, rc, lambda i, j, r: rounded(i, j, r.astype(f32)).astype(np.float64))
        bound = (cnt[:, None] + 64.0) * stress.EPS24 * big_a
        worst.append(float(np.where(bound > 0.0, np.abs(got - want) / np.where(bound > 0.0, bound, 1.0), 0.0).max()))
        # the virial columns of the heat flux, -s_i v_i with the checker's momenta (v = p / m: the ratio does not hang on m), against (n + 64) 2^-24 B_i,a
        bound_b = (cnt[:, None] + 64.0) * stress.EPS24 * hf._times_v(big_a, np.abs(p))
        worst_b.append(float(np.where(bound_b > 0.0, np.abs(hf._times_v(got - want, p)) / np.where(bound_b > 0.0, bound_b, 1.0), 0.0).max()))
    print(f"{name}: the pair function in float32 against the float rule, error / bound at step 0 and after the steps: {worst[0]:.3g}, {worst[1]:.3g}; "
          f"through -s v against the B bound: {worst_b[0]:.3g}, {worst_b[1]:.3g}")
    # the heat-flux leg of the float build leaves out what the stress leg leaves out, and no other.  On the float checker's positions -- the build the omission is for --
    # both regimes miss the B bound (7.4, 0.26 and 1.5, 0.57); on the double checker's eam_void does (7.2, 0.71) and eam_sparse comes to 0.86, 0.36 of it: v_i weights
    # the components of s_i, so the worst component of -s_i v_i is relatively better than the worst of s_i
    if name in FLOAT_STRESS_LEFT_OUT:
        assert max(worst_b) > (1.0 if SINGLE or name == "eam_void" else 0.5), (name, worst_b)
        for got, recorded in zip(worst_b, FLOAT_FLUX_FACTORS[name]):
            assert SINGLE or abs(got / recorded - 1.0) <= 0.05, (name, worst_b)
    else:
        assert max(worst_b) <= 1.0, (name, worst_b)
    if name in FLOAT_STRESS_LEFT_OUT:
        assert max(worst) > 1.0, (name, worst)
        for got, recorded in zip(worst, FLOAT_STRESS_LEFT_OUT[name]):          # (recorded from the double checker's positions, to two digits; the float checker's give 8.4, 0.71 and 4.8, 3.4)
            assert SINGLE or (got > 1.0 and abs(got / recorded - 1.0) <= 0.05), (name, worst)
    else:
        assert max(worst) <= 1.0, (name, worst)


def test_lj_dense_bin_count_keeps_the_reference_off_the_edges(orc):
    """lj_dense at step 0 has 4.6 million pairs: with 64 bins one of them lies within DELTA64 of an edge, which the double build's cap of 0 refuses.  From the sorted
    reference distances alone: 63 is the largest count <= 64 with none, and the GPU test of that state uses it.  (The float build's cap is a share of the pairs: 64.)"""
    if SINGLE:
        assert _bins("lj_dense", "step0") == BINS
        return
    ref = dr._reference(orc, "lj_dense")
    r = rdf._distances(ref["s0"]["r"], _box(ref["g"]), ref["rc"] + 2.0 * rdf.DELTA64)
    near = {}
    for bins in range(BINS, BINS - 8, -1):
        edges = _edges(bins, ref["rc"])
        near[bins] = int((np.searchsorted(r, edges + rdf.DELTA64, side="right") - np.searchsorted(r, edges - rdf.DELTA64, side="left")).sum()) // 2
    print("lj_dense step 0: reference pairs within 1e-9 A of an edge, by bin count:", near)
    assert near[BINS] == FIGURES["lj_dense"]["near"][0] == 1
    assert BINS_LJ_DENSE_STEP0 == max(b for b, v in near.items() if v == 0)
    cum, nr = rdf._reference(object(), ref["s0"]["r"], _box(ref["g"]), _edges(BINS_LJ_DENSE_STEP0, ref["rc"]), rdf.DELTA64)
    assert nr.sum() == 0 and cum[-1] == FIGURES["lj_dense"]["pairs"][0]


def test_helpers_that_take_three_extents_give_the_cube_what_they_gave_before(pkg):
    """test_pressure._pairs, test_atom_stress._restate and test_atomic_strain._restate take three extents as they stand (test_rdf._distances, _numpy_csp and _numpy_cna
    were generalised for the deforming box and are pinned by test_deform_coupling.py).  For a cube given as a scalar, where the helper takes one, and as three equal
    extents they return the same bits, and so do the helpers on states with no pair at all and with atoms that have no neighbour, which they had never met."""
    n, lat, rc = 5, 3.615, 4.95
    L = n * lat
    cube = np.array([L, L, L])
    pos = csp._host_positions(pkg, ["-x", n, "-y", n, "-z", n, "-l", repr(lat), "-r", 0.1, "-e"])
    a, b = _pairs(pos, L, rc), _pairs(pos, cube, rc)
    assert len(a[0]) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
    before = pos[a[0]] - pos[a[1]]
    before -= np.rint(before / L) * L
    assert np.array_equal(a[2], before) and np.array_equal(a[3], np.sqrt((before * before).sum(-1)))
    fr_of = stress._pair_function("lj")
    s, big_a, cnt = stress._restate(pos, cube, rc, fr_of)
    assert np.array_equal(cnt, np.bincount(a[0], minlength=len(pos)))
    t = 0.5 * a[2][:, 0] * a[2][:, 1] * fr_of(a[0], a[1], a[3])
    assert np.abs(s[:, 5] + np.bincount(a[0], weights=t, minlength=len(pos))).max() <= 1e-13 * big_a[:, 5].max()
    moved = pos + 0.05 * np.sin(pos)
    m = strain._restate(moved, cube, pos, cube, rc)
    assert np.array_equal(m["n"], np.bincount(_pairs(moved, L, rc)[0], minlength=len(pos))) and not m["invalid"].any()
    # a gas: no pair at all, and one close pair in it
    gas = csp._host_positions(pkg, ["-x", 3, "-y", 3, "-z", 3, "-l", 17.0, "-r", 0.1])
    box = np.array([51.0, 51.0, 51.0])
    assert all(len(x) == 0 for x in _pairs(gas, box, 11.575)) and not _neighbour_counts(gas, box, 11.575).any()
    assert len(rdf._distances(gas, box, 11.575)) == 0
    cum, near = rdf._reference(object(), gas, box, _edges(BINS, 11.575), rdf.DELTA64)
    assert not cum.any() and not near.any()
    s, big_a, cnt = stress._restate(gas, box, 11.575, fr_of)
    assert not s.any() and not big_a.any() and not cnt.any()
    m = strain._restate(gas, box, gas, box, 11.575)
    assert m["invalid"].all() and not m["n"].any() and np.isnan(m["e"]).all() and np.isnan(m["d2"]).all()
    c = csp._numpy_csp(gas, box, 11.575, 11.575, csp.DELTA64)
    assert np.isinf(c["csp"]).all() and not c["coord"].any() and not c["unsure"].any()
    t = cna._numpy_cna(gas, box, 11.575, cna.DELTA64)
    assert not t["type"].any() and np.isinf(t["margin"]).all()
    near_pair = gas.copy()
    near_pair[1] = near_pair[0] + np.array([3.0, 0.0, 0.0])
    s, big_a, cnt = stress._restate(near_pair, box, 11.575, fr_of)
    assert cnt[0] == 1 and cnt[1] >= 1 and 0 < (cnt > 0).sum() < len(cnt) and s[0, 0] != 0.0 and big_a[0, 0] == abs(s[0, 0])
    assert not s[cnt == 0].any() and not big_a[cnt == 0].any() and np.all(big_a[cnt > 0, 0] > 0.0)


def test_masked_assert_within_on_a_made_up_case():
    """test_atomic_strain._assert_within with the mask of invalid atoms, on arrays made up from the restatement itself: a cluster of twelve atoms with one atom that has
    two neighbours and one that has none.  The restatement's own arrays pass; a NaN too many or too few, a wrong count, a valid atom off by more than the bound and a mask
    that is not the restatement's fail; without the mask the call refuses invalid atoms as before."""
    rng = np.random.default_rng(11)
    box = np.array([40.0, 40.0, 40.0])
    ref = np.concatenate([10.0 + 1.5 * rng.uniform(-1, 1, (12, 3)), [[20.0, 20.0, 20.0], [21.5, 20.0, 20.0], [20.0, 21.5, 20.0]], [[32.0, 32.0, 5.0]]])
    pos = ref + 0.05 * rng.uniform(-1, 1, ref.shape)
    m = strain._restate(pos, box, ref, box, 4.0)
    bad = m["invalid"]
    assert m["n"].tolist()[12:] == [2, 2, 2, 0] and bad.tolist() == [False] * 12 + [True] * 4
    good = (m["e"].copy(), m["d2"].copy(), m["n"].astype(np.int32))
    strain._assert_within("made up", good, m["e"], m["d2"], m, strain.EPS53, invalid=bad)
    assert strain.RATIOS["made up"] == (0.0, 0.0)

    def fails(got, invalid=bad, want=(m["e"], m["d2"])):
        with pytest.raises(AssertionError):
            strain._assert_within("made up, broken", got, want[0], want[1], m, strain.EPS53, invalid=invalid)
    fails(good, invalid=None)                                           # the existing calls: no invalid atom at all
    e = good[0].copy()
    e[3, 2] = np.nan
    fails((e, good[1], good[2]))                                        # a NaN in a valid atom
    e = good[0].copy()
    e[13] = 0.0
    fails((e, good[1], good[2]))                                        # an invalid atom that is not NaN
    d2 = good[1].copy()
    d2[15] = 0.0
    fails((good[0], d2, good[2]))
    cnt = good[2].copy()
    cnt[15] = 1
    fails((good[0], good[1], cnt))                                      # the count of an invalid atom is compared too
    e = good[0].copy()
    e[5, 4] += 1e-9
    fails((e, good[1], good[2]))                                        # a valid atom outside the bound with C_BOUND
    d2 = good[1].copy()
    d2[0] += 1e-9
    fails((good[0], d2, good[2]))
    other = bad.copy()
    other[0] = True
    fails(good, invalid=other)                                          # a mask that is not the restatement's
    m_all = strain._restate(pos[12:], box, ref[12:], box, 4.0)          # every atom invalid
    strain._assert_within("made up, all invalid", (m_all["e"], m_all["d2"], m_all["n"].astype(np.int32)), m_all["e"], m_all["d2"], m_all, strain.EPS53,
                          invalid=m_all["invalid"])
    # the mask changes nothing for a state without invalid atoms
    strain._assert_within("made up, valid", tuple(a[:12] for a in good), m["e"][:12], m["d2"][:12], {k: v[:12] for k, v in m.items() if k != "lists7"}, strain.EPS53)


# ---------------------------------------------------------------- the state with a singular sum d0 d0^T
SINGULAR_STEPS = 5
MARGIN = 0.01         # Angstroms: how far inside (the four) and outside (every other atom) the cutoff atom i's distances stay, at the start and after the steps


def _cell_of(r, box, grid):
    return np.floor(r / (box / np.array(grid, dtype=np.float64))).astype(np.int64) % np.array(grid)


def _image(v, box):
    return v - np.rint(v / box) * box


def _singular_candidates(pos, box, rc, grid):
    """(i, c, positions) in ascending gid i: atoms of eam_sparse's step 0 with exactly three neighbours inside the cutoff of which one, c, is moved into the plane through i
    and the other two -- to its projection on the plane, or from there towards the centroid of the three (a point of the plane too) in quarters of the way -- so that all six
    distances of the four lie in (1 A, cutoff - MARGIN), c stays more than 1 A from every other atom and in its cell or a neighbouring one, and no fourth atom is
    within cutoff + MARGIN of i.  The lattice constant of 7 A puts the twelve nearest sites AT the cutoff, so the first projection rarely does."""
    i_all, j_all, _, _ = _pairs(pos, box, rc)
    for i in np.nonzero(np.bincount(i_all, minlength=len(pos)) == 3)[0]:
        three = j_all[i_all == i]
        if np.sort(np.sqrt((_image(pos - pos[i], box) ** 2).sum(1)))[4] <= rc + MARGIN:
            continue
        for c in three:
            a, b = [int(x) for x in three if x != c]
            va, vb, vc = (_image(pos[x] - pos[i], box) for x in (a, b, c))
            normal = np.cross(va, vb)
            normal /= np.sqrt(normal @ normal)
            for t in (0.0, 0.25, 0.5, 0.75, 1.0):
                new = pos.copy()
                new[c] = np.mod(pos[i] + (1.0 - t) * (vc - (vc @ normal) * normal) + t * (va + vb) / 3.0, box)
                four = [int(i), a, b, int(c)]
                dist = [np.sqrt((_image(new[p] - new[q], box) ** 2).sum()) for k, p in enumerate(four) for q in four[k + 1:]]
                others = np.delete(np.sqrt((_image(new - new[c], box) ** 2).sum(1)), four)
                step = np.abs(_cell_of(new[c], box, grid) - _cell_of(pos[c], box, grid))
                step = np.minimum(step, np.array(grid) - step)
                if min(dist) > 1.0 and max(dist) < rc - MARGIN and step.max() <= 1 and others.min() > 1.0:
                    yield int(i), int(c), new
                    break


_SINGULAR = {}


def _singular(orc):
    """the first candidate that keeps its three neighbours, by MARGIN, through the checker's steps: scatter, redistribute, forces, reference, 5 steps, the restatement"""
    if not _SINGULAR:
        ref = dr._reference(orc, "eam_sparse")
        g, box, rc = ref["g"], _box(ref["g"]), ref["rc"]
        for i, c, new in _singular_candidates(ref["s0"]["r"], box, rc, ref["grid"]):
            o = _make(orc, g)
            o.scatter(orc.R, new)
            o.redistribute()
            o.compute_force()
            start = o.gather(orc.R)
            o.step(SINGULAR_STEPS)
            pos = o.gather(orc.R)
            o.close()
            to_i = np.sort(np.sqrt((_image(pos - pos[i], box) ** 2).sum(1)))
            if to_i[3] < rc - MARGIN and to_i[4] > rc + MARGIN:
                _SINGULAR.update(i=i, c=c, new=new, start=start, m=strain._restate(pos, box, start, box, rc, dtype=REAL))
                break
        assert _SINGULAR, "no atom of the state can be made singular"
    return _SINGULAR


def _assert_singular(m, i):
    """atom i has three neighbours and is invalid by the determinant alone, far from the threshold; no other atom with 3+ neighbours is near it"""
    ratio = m["det_ratio"]
    assert m["n"][i] == 3 and m["invalid"][i] and np.isnan(m["e"][i]).all() and np.isnan(m["d2"][i])
    assert abs(ratio[i]) < 1e-12, ratio[i]
    rest = (m["n"] >= 3) & (np.arange(len(ratio)) != i)
    assert not ((ratio[rest] > 1e-10) & (ratio[rest] < 1e-8)).any() and not (ratio[rest] <= 1e-10).any(), np.sort(ratio[rest])[:4]
    assert np.array_equal(m["invalid"], (m["n"] < 3) | (np.arange(len(ratio)) == i))


def test_singular_state_in_numpy_alone(orc):
    """eam_sparse at step 0 with one of an atom's three neighbours moved into the plane of the atom and the other two: the reference vectors d0 of atom i span a plane,
    sum d0 d0^T has rank 2, and the atom is invalid by det <= 1e-9 t^3 with three neighbours -- the branch every other test asserts not to occur.  Its det / t^3 is rounding
    (below 1e-12) and no other atom lies between 1e-10 and 1e-8, so the decision is not a rounding matter."""
    s = _singular(orc)
    ref = dr._reference(orc, "eam_sparse")
    moved = s["new"][s["c"]] - ref["s0"]["r"][s["c"]]
    print(f"singular: atom {s['i']}, moved neighbour {s['c']} by {moved.tolist()}, det / t^3 {s['m']['det_ratio'][s['i']]:.3e}, "
          f"smallest other {np.sort(s['m']['det_ratio'][(s['m']['n'] >= 3) & (np.arange(480) != s['i'])])[0]:.3e}, invalid {int(s['m']['invalid'].sum())}")
    assert np.abs(s["start"] - s["new"]).max() <= (4e-6 if SINGLE else 0.0)
    _assert_singular(s["m"], s["i"])


def test_a_radius_that_names_the_cutoff_in_decimal_is_accepted(pkg):
    """Found by the comd-hip run below: Cu_u6.eam's cutoff comes out of the table arithmetic as 4.949999999999989, and --strainCutoff 4.95 was refused with a message that
    named 4.95 as the largest value allowed.  A radius within 64 ulps (of real_t) above the cutoff is the cutoff, for --strainCutoff, --cspCoord and --rdfMax; one per
    cent more is refused as before."""
    base = ["-e", "-x", 4, "-y", 5, "-z", 6, "-l", 7.0, "--strain", "--csp", "--rdf", 48]
    with pkg.Simulation(base, host_only=True) as sim:
        assert sim.cutoff < 4.95 and 4.95 - sim.cutoff < 1e-6
    proc = _child(f"pkg.Simulation({base!r} + ['--strainCutoff', 4.95, '--cspCoord', 4.95, '--rdfMax', 4.95], host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "Error:" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    for flag in ("--strainCutoff", "--cspCoord", "--rdfMax"):
        proc = _child(f"pkg.Simulation({base!r} + [{flag!r}, 5.0], host_only=True); print('made')")
        assert proc.returncode != 0 and "made" not in proc.stdout and "Error:" in proc.stdout and flag[2:] in proc.stdout, (flag, proc.stdout[-1500:])


# ================================================================ GPU 1: every regime, step 0 and after its steps, thread_atom
_REFERENCE_STATE = {}


def _run(gpu, name, method, overlap=0, extra=()):
    g = REGIMES[name]
    return gpu.Simulation(_flags(g, method, overlap) + list(extra))


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("name", ALL)
def test_analyses_in_every_regime(gpu, orc, name, stage):
    """Checks 1 to 6 of the module under thread_atom, at step 0 and after the regime's steps (30 for the hot regimes, else 5) with the strain reference taken at step 0.
    lj_dense: the virial and the histogram."""
    g = REGIMES[name]
    with _run(gpu, name, "thread_atom") as sim:
        assert sim.grid == g.grid and sim.n_global == g.atoms
        if stage == "step0":
            if not SINGLE:
                assert np.array_equal(sim.gather(0), dr._reference(orc, name)["s0"]["r"])
            _analyse(sim, name, 0, f"{name} step 0", exact=not SINGLE)
            return
        reference = None
        if name not in PAIR_ONLY:
            sim.set_strain_reference()
            reference = (sim.gather(0).copy(), sim.box)
        sim.step(g.steps)
        out = _analyse(sim, name, 1, f"{name} step {g.steps}", reference=reference)
        if name not in PAIR_ONLY:
            fig = FIGURES[name]
            assert (out["strain_summary"]["invalid"] > 0) == (fig["invalid"] > 0)
            if name == "lj_void":
                assert out["strain_summary"]["invalid"] == out["strain_summary"]["n"] == 144 and out["strain_summary"]["max_shear_gid"] == -1
    for key, value in sorted(RATIOS.items()):
        print(f"RATIO so far, largest error / bound: {key} {value:.4g}")


# ================================================================ GPU 2: the other layouts after the steps
LAYOUTS = {"cta_cell -a 1": ("cta_cell", 1, []), "cta_cell -H": ("cta_cell", 0, ["-H"]), "thread_atom_nl": ("thread_atom_nl", 0, []),
           "cta_cell -L -S 0.03": ("cta_cell", 0, ["-L", "-S", 0.03])}


def _layout_cases():
    out = []
    for name, g in REGIMES.items():
        for layout in LAYOUTS:
            if "-L" in layout and (g.eam or (name, "cta_cell -L") == dr.REFUSED):          # pairlists are LJ's; lj_dense's -L cells hold more than a workgroup takes
                continue
            out.append(pytest.param(name, layout, id=f"{name}-{layout.replace(' -', '_').replace(' ', '')}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,layout", _layout_cases())
def test_layouts_after_the_steps(gpu, name, layout):
    """cta_cell with -a 1 and with the Hilbert numbering, thread_atom_nl (cells sized cutoff + skin and not re-binned between list builds) and, for LJ, cta_cell -L: the
    strain reference at step 0, the regime's steps, then every check against the restatement of the layout's own gathered positions."""
    g = REGIMES[name]
    method, overlap, extra = LAYOUTS[layout]
    with _run(gpu, name, method, overlap, extra) as sim:
        reference = None
        if name not in PAIR_ONLY:
            sim.set_strain_reference()
            reference = (sim.gather(0).copy(), sim.box)
        sim.step(g.steps)
        _analyse(sim, name, 1, f"{name} {layout} step {g.steps}", reference=reference, regular_cells=method != "thread_atom_nl" and "-L" not in extra)


# ================================================================ GPU 3: message halo against mirrored halo
ALL_SIX = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    sim.set_strain_reference()
    sim.step({steps})
    rc = sim.cutoff
    w, k = sim.virial()
    e, d2, n = sim.atomic_strain(rc)
    c, coord = sim.centro_symmetry(r_coord=rc)
    flux = sim.heat_flux()
    np.savez({out!r}, pos=sim.gather(0), w=w, k=k, j=sim.atomic_heat_flux(), j_kinetic=flux["kinetic"], j_potential=flux["potential"], j_virial=flux["virial"], j_total=flux["total"], counts=sim.pair_histogram({bins})[1], csp=c, coord=coord, cna=sim.common_neighbor_analysis(),
             s0=sim.atomic_stress(kinetic=False), s1=sim.atomic_stress(kinetic=True), e=e, d2=d2, n=n,
             stress_summary=json.dumps(sim.stress_summary()), strain_summary=json.dumps(sim.strain_summary(cutoff=rc)), halo=int(sim.cells()["nAtoms"][sim.n_local_boxes:].sum()))
    sim.close()
    print("ALL SIX saved")
"""


def _all_six_in_child(tmp_path, tag, args, steps, env):
    out = str(tmp_path / f"{tag}.npz")
    proc = _child(ALL_SIX.format(args=list(args), steps=steps, out=out, bins=BINS), env=env)
    assert proc.returncode == 0 and "ALL SIX saved" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", dr.SPARSE)
def test_message_halo_gives_the_mirrored_halos_bits(tmp_path, name):
    """COMD_HALO_MIRROR=0 (pack, message, unpack) against =1 (MirrorAtomCells, which refills halo cells that were empty) after the 30 hot steps of the sparse regimes, a
    child process each: the six analyses and the two summaries bit for bit."""
    g = REGIMES[name]
    a = _all_six_in_child(tmp_path, "mirror", _flags(g, "thread_atom", 0), g.steps, {"COMD_HALO_MIRROR": "1"})
    b = _all_six_in_child(tmp_path, "message", _flags(g, "thread_atom", 0), g.steps, {"COMD_HALO_MIRROR": "0"})
    assert int(a["halo"]) > 0 and int(a["halo"]) == int(b["halo"]) and a["counts"].sum() > 0 and np.isnan(a["e"]).any() and not np.isnan(a["e"]).all()
    assert a["j"].shape == (g.atoms, 9) and np.abs(a["j"]).max(0).min() > 0.0 and {"j", "j_kinetic", "j_potential", "j_virial", "j_total"} <= set(a.files)
    for key in a.files:
        assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), key


# ================================================================ GPU 4: two ranks sharing the device
RANKS = {"lj_sparse": (1, 1, 2), "eam_sparse": (2, 1, 1), "lj_void": (2, 1, 1)}
WORKERS = ("pressure", "rdf", "csp", "cna", "stress", "heatflux", "strain")
_ONE_RANK = {}


def _rank_flags(name):
    return _flags(REGIMES[name], "thread_atom", 0)


def _one_rank(gpu, name):
    """what the six workers compute, on one rank: at step 0 by the workers' own calls (their default radii are the cutoff in these regimes), the strain after the steps"""
    if name not in _ONE_RANK:
        g = REGIMES[name]
        with gpu.Simulation(_rank_flags(name)) as sim:
            rc, box = sim.cutoff, sim.box
            assert 0.5 * (np.sqrt(0.5) + 1.0) * sim.lattice_constant > rc
            # the rank rule of test_atom_stress.py is 1e-12 max A, A the magnitudes of the PAIR terms: in these regimes they are 1e-3 eV beside kinetic terms of 7 eV, whose
            # ulps depend on the rank count (the initial momenta are scaled by a sum over the ranks).  The rule is applied to what it measures: kinetic=False.
            kinetic = False
            out = dict(virial=sim.virial(), p=sim.pressure_tensor(), hist=sim.pair_histogram(BINS), csp=sim.centro_symmetry(), defects=sim.defects(),
                       cna=sim.common_neighbor_analysis(), cna_counts=sim.structure_counts(), s=sim.atomic_stress(kinetic=kinetic),
                       stress_summary=sim.stress_summary(kinetic=kinetic), omega=sim.atomic_volume, box=box, rc=rc)
            pos = sim.gather(0).copy()
            fr_of = stress._pair_function("eam", sim.eam_table(0), sim.eam_table(1), sim.gather(5).copy()) if g.eam else stress._pair_function("lj")
            _, big_a, cnt = stress._restate(pos, box, rc, fr_of)
            out["a_max"], out["n_max"] = float(big_a.max()), int(cnt.max())
            sim.set_strain_reference()
            sim.step(g.steps)
            out["strain"], out["strain_summary"] = sim.atomic_strain(), sim.strain_summary()
            out["m"] = strain._restate(sim.gather(0).copy(), box, pos, box, rc, dtype=REAL)
        # the heat flux as tests/heatflux_worker.py takes it: at step 0, after a scatter of the seeded momenta of test_heat_flux._new_momenta (the halo slots keep the old ones)
        import test_heat_flux as hf
        with gpu.Simulation(_rank_flags(name)) as sim:
            p = hf._new_momenta(sim.n_global, sim.mass)
            sim.scatter(1, p)
            out["j"], out["j_sums"] = sim.atomic_heat_flux(), sim.heat_flux()
            v = p / sim.mass
            out["b_max"], out["v_max"] = float(hf._times_v(big_a, np.abs(v)).max()), float(np.abs(v).max())
            out["conv_max"] = float(hf._convective(sim.gather(3).copy(), p, sim.mass)[2].max())
        _ONE_RANK[name] = out
    return _ONE_RANK[name]


def _launch(worker, grid, argv, timeout=600):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    assert world == 2                                                   # at most two GPU processes at a time
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, f"{worker}_worker.py"), str(r), str(world), port, *map(str, grid), *argv],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
    return outs


def test_every_rank_keeps_two_cells_per_axis(orc):
    for name, grid in RANKS.items():
        g = REGIMES[name]
        o = orc.Oracle(g.n, grid, eam=g.eam, temperature=g.temp, delta=g.delta, lat=g.lat)
        assert o.n_ranks == 2 and o.n_global == g.atoms
        for rank in range(2):
            cells = o.rank_grid(rank)[0]
            print(name, grid, "rank", rank, "cells", cells)
            assert min(cells) >= 2, (name, rank, cells)
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("worker", WORKERS)
@pytest.mark.parametrize("name", list(RANKS))
def test_two_ranks_give_the_one_rank_results(gpu, tmp_path, name, worker):
    """Two ranks sharing the device (gloo) through the workers of the six modules with the regime's flags, each under its module's rank rule: tensors to 1e-12 of the
    largest component, counts, coordination and types equal, csp within 1e-10 A^2 + 1e-12 csp, stress within 1e-12 max A with the summary's gid equal, strain within the
    masked bound with invalid, n, above_threshold and the gid equal.  lj_void pins the rank loops of the two summaries: no rank has a valid atom for the strain (gid -1),
    and with kinetic=False every von Mises stress is 0 on both ranks, so the gid is the lowest of equals across ranks, 0."""
    grid, args, one = RANKS[name], json.dumps(_rank_flags(name)), _one_rank(gpu, name)
    tol = 1e-5 if SINGLE else 1e-12
    if worker == "pressure":
        for out in _launch(worker, grid, [args]):
            w, k, p = (np.array(x) for x in json.loads(re.search(r"^VIRIAL (.*)$", out, flags=re.M).group(1)))
            if name == "lj_void":
                assert not w.any()
            else:
                assert _rel(w, one["virial"][0]) <= tol
            assert _rel(k, one["virial"][1]) <= tol and _rel(p, one["p"]) <= tol
    elif worker == "rdf":
        for out in _launch(worker, grid, [str(BINS), args]):
            edges, counts = json.loads(re.search(r"^PAIRHIST (.*)$", out, flags=re.M).group(1))
            assert np.array_equal(np.array(edges), one["hist"][0]) and np.array_equal(np.array(counts, dtype=np.int64), one["hist"][1])
        assert (one["hist"][1].sum() == 0) == (name == "lj_void")
    elif worker == "csp":
        _launch(worker, grid, [str(tmp_path), args])
        for r in range(2):
            d = np.load(tmp_path / f"csp_rank{r}.npz")
            c0, coord0 = one["csp"]
            assert np.isinf(c0).all() and np.array_equal(np.isinf(d["csp"]), np.isinf(c0))
            assert np.array_equal(d["coord"], coord0) and np.array_equal(d["defects"], one["defects"]) and len(one["defects"]) == len(c0)
    elif worker == "cna":
        _launch(worker, grid, [str(tmp_path), args])
        for r in range(2):
            d = np.load(tmp_path / f"cna_rank{r}.npz")
            c = one["cna_counts"]
            assert np.array_equal(d["types"], one["cna"]) and d["counts"].tolist() == [c["other"], c["fcc"], c["hcp"], c["ico"]] and c["other"] == len(one["cna"])
    elif worker == "stress":
        _launch(worker, grid, [str(tmp_path), args, "0"])                # kinetic=False: see _one_rank
        # (float build: two runs, each within test_atom_stress's float bound (n + 64) 2^-24 A of the exact sums)
        s0, sum0, bound = one["s"], one["stress_summary"], (2.0 * (one["n_max"] + 64.0) * stress.EPS24 if SINGLE else 1e-12) * one["a_max"]
        vm0 = stress._von_mises(s0)
        order = np.sort(vm0)
        assert (order[-1] == 0.0 and name == "lj_void") or order[-1] - order[-2] > 8.0 * bound      # all equal, or not a near-tie the ranks could resolve differently
        assert sum0["max_von_mises_gid"] == int(np.argmax(vm0))
        for r in range(2):
            s, summary = np.load(tmp_path / f"stress_rank{r}.npy"), json.load(open(tmp_path / f"stress_rank{r}.json"))
            assert s.shape == s0.shape and np.abs(s - s0).max() <= bound
            assert summary["n"] == sum0["n"] == len(s0) and summary["max_von_mises_gid"] == sum0["max_von_mises_gid"]
            for key in ("min_pressure", "max_pressure", "max_von_mises", "mean_pressure", "mean_von_mises"):
                assert abs(summary[key] - sum0[key]) <= 4.0 * bound / one["omega"], key
            if name == "lj_void":
                assert not s.any() and summary == sum0 and summary["max_von_mises_gid"] == 0 and summary["max_von_mises"] == 0.0
    elif worker == "heatflux":
        # test_heat_flux.py::test_ranks_give_the_one_rank_array: every rank returns the global array, the one-rank one within 1e-12 of the largest magnitude of the part,
        # and the sums over the ranks within 1e-12 of the sums of magnitudes.  Float build: two runs, each within the module's float bounds of the exact columns --
        # (n + 64) 2^-24 B for the virial ones, 8 x 2^-24 (|e| + ke) |v| for the convective ones, whose e_i the two runs hold within per_atom_energy_abs each -- and
        # the sums within the sum of the atoms' bounds plus the (k + 3) 2^-24 of the two reductions.
        _launch(worker, grid, [str(tmp_path), args])
        j0, sums0 = one["j"], one["j_sums"]
        if SINGLE:
            conv = 2.0 * (8.0 * stress.EPS24 * one["conv_max"] + TOL["per_atom_energy_abs"] * one["v_max"])
            scale = np.array([conv] * 6 + [2.0 * (one["n_max"] + 64.0) * stress.EPS24 * one["b_max"]] * 3)
        else:
            scale = 1e-12 * np.array([one["conv_max"]] * 6 + [one["b_max"]] * 3)
        mag = np.abs(j0).sum(0)
        sum_bound = (len(j0) * scale + 8.0 * stress.EPS24 * mag) if SINGLE else 1e-12 * mag
        for r in range(2):
            d = np.load(tmp_path / f"heatflux_rank{r}.npz")
            assert d["j"].shape == j0.shape == (REGIMES[name].atoms, 9)
            err = np.abs(d["j"] - j0).max(0)
            print(f"RATIO heat flux ranks {name} rank {r}:", (err / np.where(scale > 0.0, scale, 1.0)).max())
            assert np.all(err <= scale), (name, err, scale)
            for i, part in enumerate(("kinetic", "potential", "virial")):
                assert np.all(np.abs(d["sums"][3 * i:3 * i + 3] - sums0[part]) <= sum_bound[3 * i:3 * i + 3]), part
            assert np.all(np.abs(d["sums"][9:12] - sums0["total"]) <= sum_bound[0:3] + sum_bound[3:6] + sum_bound[6:9])
            if name == "lj_void":
                assert not d["j"][:, 3:9].any() and not d["sums"][3:9].any()          # no pair at all: the potential and virial parts are exactly 0 on both ranks
    else:
        g = REGIMES[name]
        _launch(worker, grid, [str(tmp_path), str(g.steps), args])
        got0, sum0, m = one["strain"], one["strain_summary"], one["m"]
        bad = m["invalid"]
        eps = strain._eps(m, "single" if SINGLE else "double", one["box"])
        strain._assert_within(f"regimes one rank {name}", got0, m["e"], m["d2"], m, eps, invalid=bad, d2_by_kappa=True)
        assert sum0["invalid"] == int(bad.sum()) and (bad.all() == (name == "lj_void")) and bad.any()
        gamma = strain._shear(got0[0][~bad])
        with np.errstate(invalid="ignore"):
            bound_g = (2.0 * strain.C_BOUND * (m["n"] + 64.0) * eps * m["kappa"] * (1.0 + 2.0 * np.abs(got0[0]).max(1)))[~bad]
            bound_d = (strain.C_BOUND * (m["n"] + 64.0) * eps * m["s"] * m["kappa"])[~bad]
        # the gid of the maximum and the count above the threshold are compared where the bound decides them: the maximum is not a near-tie the ranks could resolve
        # differently, no atom is within its bound of the threshold.  Double build: always, asserted.  Float build: with kappa 1e5 its bound on E decides nothing here.
        decided = ["n", "invalid"]
        if len(gamma):
            order = np.sort(gamma)
            if order[-1] - order[-2] > 2.0 * bound_g.max():
                decided.append("max_shear_gid")
            if not (np.abs(gamma - 0.1) <= 2.0 * bound_g).any():
                decided.append("above_threshold")
            assert SINGLE or len(decided) == 4
            assert sum0["max_shear_gid"] == int(np.nonzero(~bad)[0][np.argmax(gamma)])
        else:
            decided += ["max_shear_gid", "above_threshold"]
        for r in range(2):
            d, summary = np.load(tmp_path / f"strain_rank{r}.npz"), json.load(open(tmp_path / f"strain_rank{r}.json"))
            assert np.array_equal(d["box0"], one["box"])
            strain._assert_within(f"regimes ranks {name}", (d["e"], d["d2"], d["n"]), got0[0], got0[1], m, eps, invalid=bad, d2_by_kappa=True)
            for key in decided:
                assert summary[key] == sum0[key], (key, summary[key], sum0[key])
            if name == "lj_void":
                assert summary == sum0 and summary["invalid"] == summary["n"] == 144 and summary["max_shear_gid"] == -1 and summary["max_shear"] == 0.0
                continue
            for key, scale in (("max_shear", bound_g.max()), ("mean_shear", bound_g.max()), ("mean_volumetric", bound_g.max()), ("max_d2min", bound_d.max()),
                               ("mean_d2min", bound_d.max())):
                assert abs(summary[key] - sum0[key]) <= scale, (key, summary[key], sum0[key])


# ================================================================ GPU 5: the executable
EXE_RUN = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    sim.set_strain_reference()
    for _ in range(3):
        sim.step(10)
    flux = sim.heat_flux()
    print("PYTHON", json.dumps([sim.strain_summary(cutoff=sim.cutoff), sim.stress_summary(), sim.structure_counts(), int(np.isinf(sim.centro_symmetry()[0]).sum()),
                                [flux[k].tolist() for k in ("kinetic", "potential", "virial", "total")], sim.volume]))
    sim.close()
"""


@pytest.mark.gpu
def test_comd_hip_with_every_analysis_on_eam_sparse(tmp_path):
    """comd-hip on eam_sparse for 30 steps with --pressure --rdf 48 --csp --cna --stress --strain --strainCutoff 4.95 (the double executable, whatever COMD_PRECISION says):
    exit status 0, no nan in the table -- MaxShear and MaxVM(GPa) stay finite with invalid atoms present -- and the last sample of every file against a Python run of
    the same flags and steps in the double build."""
    g = REGIMES["eam_sparse"]
    flags = [str(a) for a in _flags(g, "thread_atom", 0)]
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-d", os.path.join(ROOT, "pots"), *flags, "-N", "30", "-n", "10", "--pressure", "--rdf", "48", "--csp", "--cna",
                           "--stress", "--strain", "--strainCutoff", "4.95", "--heatflux"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    header = [line for line in proc.stdout.splitlines() if line.startswith("#  Loop")][0].split()
    extra = header[header.index("Atoms") + 1:]                          # the columns behind "# Atoms", as the rows have them
    assert [h for h in extra if h != "Jx(eV/A^2/fs)"][-2:] == ["MaxVM(GPa)", "MaxShear"] and "Pressure(GPa)" in extra and "Jx(eV/A^2/fs)" in extra, header
    vm, shear, jx = (extra.index(h) for h in ("MaxVM(GPa)", "MaxShear", "Jx(eV/A^2/fs)"))
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    assert [r[0] for r in rows] == ["0", "10", "20", "30"] and all(int(r[2]) == g.atoms and len(r[3].split()) == len(extra) for r in rows)
    for r in rows:
        assert "nan" not in " ".join(r).lower() and "inf" not in " ".join(r).lower(), r
        assert np.all(np.isfinite([float(x) for x in r[1].split() + r[3].split()]))
    assert float(rows[0][3].split()[shear]) == 0.0 and float(rows[-1][3].split()[shear]) > 0.0 and float(rows[-1][3].split()[vm]) > 0.0
    assert all(float(r[3].split()[jx]) != 0.0 for r in rows)
    child = _child(EXE_RUN.format(args=_flags(g, "thread_atom", 0)), env={"COMD_PRECISION": "double"})
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    strain_py, stress_py, cna_py, few_py, flux_py, volume_py = json.loads(re.search(r"^PYTHON (.*)$", child.stdout, flags=re.M).group(1))

    def last(name):
        lines = (tmp_path / name).read_text().splitlines()
        assert lines[0].startswith("#") and len(lines) == 5, (name, len(lines))
        return [float(x) for x in lines[-1].split()]
    row = last("csp.dat")
    assert row[0] == 30.0 and row[2] == 480.0 == few_py
    row = last("cna.dat")
    assert row == [30.0, 480.0, 0.0, 0.0, 0.0] and cna_py == {"other": 480, "fcc": 0, "hcp": 0, "ico": 0}
    row = last("strain.dat")
    assert row[0] == 30.0 and row[8] == strain_py["invalid"] > 0 and row[3] == strain_py["max_shear_gid"] and np.all(np.isfinite(row))
    assert abs(row[2] - strain_py["max_shear"]) <= 1e-14 * row[2] and abs(row[2] - float(rows[-1][3].split()[shear])) <= 1e-10
    row = last("stress.dat")
    assert row[0] == 30.0 and row[6] == stress_py["max_von_mises_gid"] and np.all(np.isfinite(row))
    # heatflux.dat: step, time, J V (3), its convective part (3), its virial part (3) -- test_heat_flux.py holds the rows to heat_flux() of a Python run to the bit
    row = np.array(last("heatflux.dat"))
    kin, pot, vir, tot = (np.array(x) for x in flux_py)
    assert row[0] == 30.0 and len(row) == 11 and np.all(np.isfinite(row))
    assert np.array_equal(row[2:5], tot) and np.array_equal(row[8:11], vir) and np.array_equal(row[5:8], kin + pot)
    assert abs(float(rows[-1][3].split()[jx]) - tot[0] / volume_py) <= 1e-10 * abs(tot[0] / volume_py)      # the column prints 11 digits
    table = rdf._rdf_file(tmp_path / "rdf.dat")[1]
    assert table.shape == (48, 4) and np.all(np.isfinite(table)) and table[:, 3].sum() > 0


# ================================================================ GPU 6: a singular sum d0 d0^T
@pytest.mark.gpu
def test_singular_reference_neighbourhood_is_invalid(gpu, orc):
    """The constructed state of test_singular_state_in_numpy_alone on the device: scatter, redistribute, forces, reference, 5 steps.  Atom i is NaN and counted invalid
    with three neighbours, in the kernel and in the restatement of the gathered positions alike, beside the atoms that are invalid by their count."""
    s = _singular(orc)
    g = REGIMES["eam_sparse"]
    with _run(gpu, "eam_sparse", "thread_atom") as sim:
        sim.scatter(0, s["new"])
        sim.redistribute()
        sim.compute_force()
        sim.set_strain_reference()
        start, box, rc = sim.gather(0).copy(), sim.box, sim.cutoff
        assert np.array_equal(start, s["start"])
        sim.step(SINGULAR_STEPS)
        pos = sim.gather(0).copy()
        m = strain._restate(pos, box, start, box, rc, dtype=REAL)
        _assert_singular(m, s["i"])
        got = sim.atomic_strain(rc)
        assert got[2][s["i"]] == 3 and np.isnan(got[0][s["i"]]).all() and np.isnan(got[1][s["i"]])
        strain._assert_within("regimes singular", got, m["e"], m["d2"], m, strain._eps(m, "single" if SINGLE else "double", box), invalid=m["invalid"], d2_by_kappa=True)
        summary = _check_strain_summary(sim, "singular", got, m, rc)
        assert summary["invalid"] == int((m["n"] < 3).sum()) + 1 and summary["n"] == g.atoms


# the GPU tests of this file (tests/test_single_precision.py runs them again in the float build and counts them)
GPU_CASE_COUNT = len(ALL) * len(STAGES) + len(_layout_cases()) + len(dr.SPARSE) + len(RANKS) * len(WORKERS) + 1 + 1
