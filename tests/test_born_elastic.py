"""The Born matrix and the stress-fluctuation elastic constants (computeBornMatrix, comdBornMatrix, Simulation.born_matrix / born_constants,
elastic_constants, comd-hip --elastic).

CoMD computes no elastic property, so nothing here is compared with a recorded number of the reference.  The checks are restatement, identities and
the literature:
  * all 21 entries against an all-pairs minimum-image sum in numpy of
        B_abcd = sum_i [ sum_j (1/2 (phi'' - phi'/r) + F'_i (rho'' - rho'/r)) r_a r_b r_c r_d / r^2 + F''(rhobar_i) g^i_ab g^i_cd ],  g^i_ab = sum_j rho'(r) r_a r_b / r
    with the derivatives of the force the kernels apply (analytic LJ exact; the quadratic tables: the derivative of interpolate's df, constant on the
    segment interpolate lands on), on the states of test_atom_stress.py, which hold every chunk class of hip/stencil_walk.h;
  * the finite-difference identity -dW_bb/d eps_a = B_ab - 2 W_aa delta_ab against virial() on a deformed perfect lattice (analytic LJ and the -P splines);
  * Mishin's published C11, C12, C44 of copper; the Cauchy relation for LJ, and its failure for EAM (the F'' term is there);
  * every method, layout, stream mode, rank count and both precisions give the same matrix; elastic_constants() against numpy; the driver's files.

Tolerances.  An entry can be a cancellation of the terms it is made of, so every comparison is relative to A_IJ, the sum of the magnitudes of all terms
of the entry, which the restatement yields with the matrix; for the F'' term that is |F''_i| G^i_I G^i_J with G the magnitude sums of g.
  double build   |got - want| <= 1e-11 A_IJ                        (the figure of the project's restatement tests)
  single build   |got - want| <= (n + c) 2^-24 A_IJ, c = n + 64    n the largest neighbour count.  A pair term is a sequential real_t sum over at most n
                 neighbours (n roundings) of terms that carry: the three roundings of r^2, amplified 8 times by k ~ r^-16 (24); the reciprocal or the
                 reciprocal square root with its Newton step and the powers formed from it (8); the four coordinate differences of the monomial (4), its
                 products xx ... xy, k xx and the multiply of the fma (4); and, for the tables, the index arithmetic and the three operations of the second
                 difference (8): 48, taken as 64 as test_atom_stress.py takes it.  The F'' term is a product of two such sums, g_I and g_J, each with its own
                 n + 64 / 2 roundings, which is where the second n comes from.  Not fitted to the observed error.
                 The tables add a knot term K_IJ to that bound.  The second derivative is piecewise constant, "on the segment interpolate lands on", and
                 in the float build the argument u = r invDx - x0 invDx carries the roundings of r (three in r^2, halved by the root, and two in r^2 y with
                 its Newton step: at most 4), of the product and of the difference, each of the size 2^-24 r invDx: 8 with the minimum image formed in
                 float on the device.  With invDx = 1816 / A (setfl) that is 5e-3 of a segment, so about one pair in 200 may land on the segment next door,
                 where a table rounded to float has another second difference (they differ by up to 4 x 2^-24 |v| invDx^2 / 2, tenths of an eV/A^2).  The
                 restatement in double cannot know which; K_IJ is the sum of |jump of the term| over the pairs (and the atoms, for F'') whose argument lies
                 within 8 x 2^-24 r invDx of a knot.  Without it state D (setfl) missed entry 11 in the float build: |got - want| = 0.2337 eV against
                 0.2035; every other state and entry passed.  K is at most 0.15 (-I), 1.6 (state F) and 6.8 (state D) times the arithmetic bound, 0 elsewhere.
                 The double build has no knot term.
No entry is left out of a comparison.
"""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import device_isa
from test_atom_stress import COMP, EPS, GPA, LAT, MISHIN, SIGMA, STATES, _assert_close, _child, _chunk_classes, _extent, _pair_function, _restate
from test_lj_interpolation import N_TABLE, interpolate, lj_table
from test_pressure import _interpolate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "comd-cuda-async_amd", "csrc")
KB = 8.6173324e-5
EPS24 = 2.0 ** -24
KNOT_ULPS = 8.0          # roundings of the table argument u = r invDx - x0 invDx in the float build: see the module docstring
TRI = [(i, j) for i in range(6) for j in range(i, 6)]          # the upper triangle, row-major: 21 entries
PUBLISHED = {"C11": 169.9, "C12": 122.6, "C44": 76.2}         # GPa, Mishin et al., PRB 63, 224106


def _axes4(i, j):
    return tuple(sorted(COMP[i] + COMP[j]))


MONO = sorted(set(_axes4(i, j) for i, j in TRI))                # the 15 monomials r_a r_b r_c r_d
assert len(MONO) == 15


def _second(x0, inv, v, n, r, knot_ulps=0.0):
    """the derivative of interpolate's df on the segment interpolate lands on (a table of n intervals, v[0] the leading pad).  With knot_ulps: also the
    magnitude by which it changes when the argument lies within knot_ulps 2^-24 r invDx of a knot and real_t arithmetic may land on the segment next door."""
    xn = x0 + n / inv
    r = np.minimum(np.maximum(r, x0), xn)
    u = r * inv - x0 * inv
    ii = np.floor(u).astype(np.int64)

    def at(k):
        return ((v[k + 3] - v[k + 1]) - (v[k + 2] - v[k])) * (inv * 0.5) * inv
    d2 = at(ii)
    if not knot_ulps:
        return d2
    frac, tol = u - ii, knot_ulps * EPS24 * np.abs(r * inv)
    other = np.where(frac <= tol, np.maximum(ii - 1, 0), np.where(1.0 - frac <= tol, np.minimum(ii + 1, len(v) - 4), ii))
    return d2, np.abs(at(other) - d2)


def _eam_second(table, r, knot_ulps=0.0):
    x0, inv, v = table
    return _second(x0, inv, v, len(v) - 3, r, knot_ulps)


def born_restate(pos, extent, rc, kind, phi=None, rho=None, emb=None, df=None, rhobar=None, block=256, knot_ulps=0.0):
    """All ordered pairs i != j with 0 < r^2 <= rc^2 under the minimum image: the matrix (6, 6), the sum of the magnitudes of its terms (6, 6) and the
    largest neighbour count.  With knot_ulps a fourth result: the knot term K_IJ of the module docstring."""
    n = len(pos)
    s6 = SIGMA ** 6
    table = lj_table() if kind == "ljtable" else None
    b15, a15, k15 = np.zeros(15), np.zeros(15), np.zeros(15)
    g, big_g = np.zeros((n, 6)), np.zeros((n, 6))
    cnt = np.zeros(n, dtype=np.int64)
    xyz = [np.ascontiguousarray(pos[:, a]) for a in range(3)]
    for s0 in range(0, n, block):
        d = []
        for a in range(3):
            da = xyz[a][s0:s0 + block, None] - xyz[a][None, :]
            da -= np.rint(da / extent[a]) * extent[a]
            d.append(da)
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        ii, jj = np.nonzero((r2 > 0.0) & (r2 <= rc * rc))
        dd = [da[ii, jj] for da in d]
        r = np.sqrt(r2[ii, jj])
        ii = ii + s0
        slack = np.zeros_like(r)
        if kind == "lj":
            k = 0.5 * 4.0 * EPS * (168.0 * s6 * s6 * r ** -14 - 48.0 * s6 * r ** -8) / (r * r)
            h = None
        elif kind == "ljtable":
            d2, jump = _second(*table, N_TABLE, r, knot_ulps or 1e-300)
            k = 0.5 * (d2 - interpolate(table, r)[1] / r) / (r * r)
            slack = 0.5 * jump / (r * r)
            h = None
        else:
            drho = _interpolate(*rho, r)[1]
            (d2phi, jump_phi), (d2rho, jump_rho) = _eam_second(phi, r, knot_ulps or 1e-300), _eam_second(rho, r, knot_ulps or 1e-300)
            k = (0.5 * (d2phi - _interpolate(*phi, r)[1] / r) + df[ii] * (d2rho - drho / r)) / (r * r)
            slack = (0.5 * jump_phi + np.abs(df[ii]) * jump_rho) / (r * r)
            h = drho / r
        for m, axes in enumerate(MONO):
            mono = dd[axes[0]] * dd[axes[1]] * dd[axes[2]] * dd[axes[3]]
            t = k * mono
            b15[m] += t.sum()
            a15[m] += np.abs(t).sum()
            if knot_ulps:
                k15[m] += (slack * np.abs(mono)).sum()
        if h is not None:
            for c, (a, b) in enumerate(COMP):
                t = h * dd[a] * dd[b]
                g[:, c] += np.bincount(ii, weights=t, minlength=n)
                big_g[:, c] += np.bincount(ii, weights=np.abs(t), minlength=n)
        cnt += np.bincount(ii, minlength=n)
    born, big_a, knot = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((6, 6))
    d2f, jump_f = _eam_second(emb, rhobar, knot_ulps or 1e-300) if kind == "eam" else (np.zeros(n), np.zeros(n))
    for i, j in TRI:
        m = MONO.index(_axes4(i, j))
        born[i, j] = born[j, i] = b15[m] + (d2f * g[:, i] * g[:, j]).sum()
        big_a[i, j] = big_a[j, i] = a15[m] + (np.abs(d2f) * big_g[:, i] * big_g[:, j]).sum()
        knot[i, j] = knot[j, i] = k15[m] + (jump_f * big_g[:, i] * big_g[:, j]).sum()
    if knot_ulps:
        return born, big_a, int(cnt.max()), knot
    return born, big_a, int(cnt.max())


def _restate_of(st, pos, extent, tables=None, knot_ulps=0.0):
    if st["pair"] == "eam":
        return born_restate(pos, extent, st["rc"], "eam", knot_ulps=knot_ulps, **tables)
    return born_restate(pos, extent, st["rc"], st["pair"], knot_ulps=knot_ulps)


def _eam_tables(sim):
    return dict(phi=sim.eam_table(0), rho=sim.eam_table(1), emb=sim.eam_table(2), df=sim.gather(5).copy(), rhobar=sim.gather(4).copy())


# the two-rank runs need two cells per rank along x: state C (LJ, 4 link cells) and an Adams EAM box of 8^3 unit cells (5 link cells on one rank, 2 per rank on two)
ALL_STATES = dict(STATES, EAM8=dict(flags=["-x", 8, "-y", 8, "-z", 8, "-l", LAT, "-r", 0.1, "-e"], n=(8, 8, 8), lat=LAT, atoms=2048, grid=(5, 5, 5), rc=4.95, pair="eam"))
_CACHE = {}


def _state(gpu, name, steps=0):
    """the matrix of state `name` after `steps` steps with its restatement: one simulation and one restatement per (state, steps), shared by the tests"""
    if (name, steps) not in _CACHE:
        st = ALL_STATES[name]
        with gpu.Simulation(st["flags"]) as sim:
            if steps:
                sim.step(steps)
            m = dict(n_atoms=sim.cells()["nAtoms"][:sim.n_local_boxes].copy(), grid=sim.grid, n=sim.n_global, born=sim.born_matrix(), again=sim.born_matrix(),
                     volume=sim.volume, pos=sim.gather(0).copy())
            tables = _eam_tables(sim) if st["pair"] == "eam" else None
        m["want"], m["A"], m["nbr"] = _restate_of(st, m["pos"], _extent(st), tables)
        _CACHE[(name, steps)] = m
    return _CACHE[(name, steps)]


# ---------------------------------------------------------------- CPU: flags, exports, ISA
def test_elastic_flags_are_listed_accepted_and_refused(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '-N', 20, '--elastic', '--elStart', 10, '--elFile', 'e.dat'], host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("elastic", "elStart", "elFile"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])
    for extra in (["--erateX", 0.01], ["--baro"], ["--elStart", 21], ["--elStart", -1]):
        proc = _child(f"pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '-N', 20, '--elastic'] + {extra!r}, host_only=True); print('made')")
        assert proc.returncode != 0 and "made" not in proc.stdout and "Error:" in proc.stdout, (extra, proc.stdout[-2000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_entry_points_are_exported_and_declared(sfx):
    def defined(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"{lib}{sfx}.so")], capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "computeBornMatrix" in defined("libcomd_hip")
    assert {"comdBornMatrix", "comdElasticConstants"} <= defined("libcomd_host")
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeBornMatrix\(SimGpu\* sim, double\* out21\);", header, flags=re.M)
    header = open(os.path.join(CSRC, "host", "comd_host.h")).read()
    assert re.search(r"^int comdBornMatrix\(SimFlat\* s, double\* born21\);", header, flags=re.M)


def test_host_only_simulation_refuses(pkg):
    sim = pkg.Simulation(["-x", 8, "-y", 8, "-z", 8], host_only=True)
    for call in (sim.born_matrix, sim.born_constants):
        with pytest.raises(RuntimeError):
            call()
    assert sim.lib.comdBornMatrix(sim.ptr, (ctypes.c_double * 21)()) == -1
    sim.close()


@pytest.mark.parametrize("precision", ["double", "single"])
def test_born_kernels_use_no_scratch_and_keep_four_waves(precision):
    """Every pair function has its instance and the final kernel exists; none spills to scratch, and each instance fits 4 waves per SIMD (128 VGPRs)."""
    blocks = device_isa.blocks(precision, r"BornMatrix_\w+")
    names = sorted(blocks)
    assert len(names) == 5, names
    assert len([n for n in names if "BornMatrix_thread_atom" in n]) == 4 and any("BornMatrix_Final" in n for n in names)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    for pair in ("6BornLjE", "11BornLjTableE", "7BornEamILb0EEE", "7BornEamILb1EEE"):
        device_isa.assert_keeps_waves(blocks, f"BornMatrix_thread_atomI{pair}", 4)


# ---------------------------------------------------------------- CPU: elastic_constants
def _elastic_numpy(born, stress, volume, temperature, n_atoms):
    b = born.mean(0) / volume
    fl, kin = np.zeros((6, 6)), np.zeros((6, 6))
    if temperature > 0.0 and len(born) >= 2:
        dev = stress - stress.mean(0)
        fl = -volume / (KB * temperature) * (dev[:, :, None] * dev[:, None, :]).mean(0)
        kin = n_atoms * KB * temperature / volume * np.diag([2.0, 2.0, 2.0, 1.0, 1.0, 1.0])
    return b, fl, kin


def _random_samples(rng, s):
    born = rng.normal(size=(s, 6, 6)) * 50.0 + 4000.0
    born = 0.5 * (born + born.transpose(0, 2, 1))
    return born, rng.normal(size=(s, 6)) * 0.01 + 0.02


def test_elastic_constants_against_numpy(pkg):
    rng = np.random.default_rng(20261021)
    volume, temperature, n_atoms = 11810.0, 300.0, 1000
    for s in (2, 7, 40):
        born, stress = _random_samples(rng, s)
        got = pkg.elastic_constants(born, stress, volume, temperature, n_atoms)
        b, fl, kin = _elastic_numpy(born, stress, volume, temperature, n_atoms)
        for key, want in (("born", b), ("fluctuation", fl), ("kinetic", kin), ("C", b + fl + kin)):
            assert got[key].shape == (6, 6) and np.array_equal(got[key], got[key].T), key
            assert np.abs(got[key] - want).max() <= 1e-12 * np.abs(want).max(), (s, key)
        c = b + fl + kin
        c11, c12, c44 = (c[0, 0] + c[1, 1] + c[2, 2]) / 3, (c[0, 1] + c[0, 2] + c[1, 2]) / 3, (c[3, 3] + c[4, 4] + c[5, 5]) / 3
        for key, want in (("C11", c11), ("C12", c12), ("C44", c44), ("K", (c11 + 2 * c12) / 3), ("G_V", (c11 - c12 + 3 * c44) / 5), ("A", 2 * c44 / (c11 - c12)),
                          ("cauchy_pressure", c12 - c44)):
            assert abs(got[key] - want) <= 1e-12 * max(abs(want), abs(c11)), (s, key, got[key], want)


def test_elastic_constants_special_cases(pkg):
    rng = np.random.default_rng(7)
    volume, temperature, n_atoms = 11810.0, 300.0, 1000
    born, stress = _random_samples(rng, 6)
    # constant stress: no fluctuation at all
    got = pkg.elastic_constants(born, np.broadcast_to(stress[0], (6, 6)), volume, temperature, n_atoms)
    assert np.all(got["fluctuation"] == 0.0) and got["kinetic"][0, 0] == 2.0 * n_atoms * KB * temperature / volume
    # sigma_1 alternating +-s over an even count: C11 falls by V s^2 / kB T
    s = 0.03
    alt = np.zeros((6, 6))
    alt[:, 0] = s * np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])
    got = pkg.elastic_constants(born, alt, volume, temperature, n_atoms)
    drop = volume * s * s / (KB * temperature)
    assert abs(got["fluctuation"][0, 0] + drop) <= 4.0 * 2.0 ** -53 * drop
    assert np.count_nonzero(got["fluctuation"]) == 1
    # T = 0, or one sample: the Born part alone
    for b, st, t in ((born, stress, 0.0), (born[:1], stress[:1], temperature)):
        got = pkg.elastic_constants(b, st, volume, t, n_atoms)
        assert np.all(got["fluctuation"] == 0.0) and np.all(got["kinetic"] == 0.0) and np.array_equal(got["C"], got["born"])
        assert np.abs(got["born"] - b.mean(0) / volume).max() <= 1e-15 * np.abs(b).max() / volume
    for bad_born, bad_stress in ((born[:, :5], stress), (born, stress[:5]), (born, stress[:, :5]), (born[0], stress[0])):
        with pytest.raises(ValueError):
            pkg.elastic_constants(bad_born, bad_stress, volume, temperature, n_atoms)


# ---------------------------------------------------------------- CPU: the restatement against the literature
def _fcc(n, lat):
    cell = np.array([[0.25, 0.25, 0.25], [0.25, 0.75, 0.75], [0.75, 0.25, 0.75], [0.75, 0.75, 0.25]])
    grid = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), axis=-1).reshape(-1, 1, 3)
    return ((grid + cell[None]) * lat).reshape(-1, 3)


def test_restatement_gives_the_published_constants_of_copper(pkg):
    """Mishin's setfl table read with the quadratic rule, the perfect 4 x 4 x 4 lattice at 3.615 A: Born C11, C12, C44 within 0.5 % of 169.9 / 122.6 /
    76.2 GPa (a stress-free lattice at T = 0 has no other part); the cubic symmetry of the matrix; and the Cauchy relation B12 = B66 for LJ."""
    with pkg.Simulation(["-x", 4, "-y", 4, "-z", 4] + MISHIN, host_only=True) as sim:
        phi, rho, emb = sim.eam_table(0), sim.eam_table(1), sim.eam_table(2)
    pos, extent = _fcc((4, 4, 4), LAT), np.full(3, 4 * LAT)
    rc = 5.50679
    assert rc < 0.5 * extent.min()
    # rhobar and F' of the perfect lattice: one value for every atom
    d = pos[0] - pos
    d -= np.rint(d / extent) * extent
    r = np.sqrt((d * d).sum(1))
    r = r[(r > 0.0) & (r <= rc)]
    rhobar = np.full(len(pos), _interpolate(*rho, r)[0].sum())
    df = _interpolate(*emb, rhobar)[1]
    born, big_a, nbr = born_restate(pos, extent, rc, "eam", phi=phi, rho=rho, emb=emb, df=df, rhobar=rhobar)
    c = born / extent.prod() * GPA
    got = {"C11": c[0, 0], "C12": c[0, 1], "C44": c[3, 3]}
    print(got, nbr)
    for key, want in PUBLISHED.items():
        assert abs(got[key] - want) <= 0.005 * want, (key, got[key], want)
    tol = 1e-11 * big_a / extent.prod() * GPA
    assert abs(c[0, 0] - c[1, 1]) <= tol[0, 0] and abs(c[0, 0] - c[2, 2]) <= tol[0, 0] and abs(c[3, 3] - c[4, 4]) <= tol[3, 3] and abs(c[3, 3] - c[5, 5]) <= tol[3, 3]
    assert abs(c[0, 1] - c[5, 5]) > 1e-3 * abs(c[0, 1])               # EAM breaks the Cauchy relation
    lj, lj_a, _ = born_restate(_fcc((8, 8, 8), LAT), np.full(3, 8 * LAT), 2.5 * SIGMA, "lj")
    assert lj[0, 1] == lj[5, 5] and lj[0, 3] == lj[4, 5] and lj[0, 0] > 0.0


# ---------------------------------------------------------------- GPU: the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", [("A", 0), ("B", 0), ("BI", 0), ("C", 0), ("D", 0), ("E", 0), ("F", 0), ("A", 10), ("E", 10)])
def test_matrix_matches_the_restatement(gpu, name, steps):
    """born_matrix() against the all-pairs sum, all 21 entries within 1e-11 A_IJ; after 10 steps atoms have changed cells.  Two calls give the same bits."""
    m, st = _state(gpu, name, steps), STATES[name]
    m0 = _state(gpu, name, 0)
    assert m0["n"] == st["atoms"] and tuple(m0["grid"]) == st["grid"] and st["classes"] <= _chunk_classes(m0["n_atoms"]), (name, sorted(set(m0["n_atoms"].tolist())))
    assert st["rc"] < 0.5 * _extent(st).min()
    assert m["born"].shape == (6, 6) and m["born"].dtype == np.float64 and np.array_equal(m["born"], m["born"].T)
    assert np.array_equal(m["born"], m["again"])
    assert np.all(m["A"] > 0.0) and m["nbr"] > 0
    _assert_close(m["born"], m["want"], 1e-11 * m["A"], f"{name} step {steps}")


def test_the_states_hold_every_chunk_class():
    assert set().union(*(STATES[n]["classes"] for n in ("A", "B", "BI", "C", "D", "E", "F"))) == {"full", "partial", "reps2", "reps4", "reps8", "reps16"}


@pytest.mark.gpu
def test_embedding_term_breaks_the_cauchy_relation(gpu):
    """State D (EAM): B12 and B66 differ by the F'' term, |B12 - B66| > 1e-3 |B12|.  State B (LJ): they share one pair sum, within the bound."""
    d, b = _state(gpu, "D"), _state(gpu, "B")
    assert abs(d["born"][0, 1] - d["born"][5, 5]) > 1e-3 * abs(d["born"][0, 1])
    for (i, j), (k, l) in (((0, 1), (5, 5)), ((0, 2), (4, 4)), ((1, 2), (3, 3)), ((0, 3), (4, 5)), ((1, 4), (3, 5)), ((2, 5), (3, 4))):
        assert abs(b["born"][i, j] - b["born"][k, l]) <= 1e-11 * b["A"][i, j], ((i, j), (k, l))


# ---------------------------------------------------------------- GPU: the finite-difference identity
@pytest.mark.gpu
@pytest.mark.parametrize("pot,n,lat,flags,rc", [("lj", (5, 6, 7), 3.25, ["--ljCutoffSigmas", 2.5], 2.5 * SIGMA), ("spline", (6, 5, 4), LAT, ["-e", "-P"], 4.95)])
def test_finite_difference_of_the_virial(gpu, pot, n, lat, flags, rc):
    """A perfect lattice in a non-cubic box stretched to 1 +- eps along one axis: -dW_aa/d eps_a = B_aa - 2 W_aa and -dW_bb/d eps_a = B_ab, W the pair
    virial of virial().  Bound: the rounding of the two virials, 2 (1e-11 A_W) / (2 eps), plus the truncation: 1e-8 |B| for analytic LJ, and
    |FD(eps) - FD(2 eps)| for the splines.  pair_histogram(1) counts the same pairs at every box: no shell crosses the cutoff.
    The LJ lattice constant is 3.25 A: 2 x 3 x 3 link cells, none of whose faces holds a lattice plane (nearest shells 2.7 % below and 5 % above the cutoff).
    At 3.615 A the 7 unit cells along z make 4 link cells of 1.75 lattice constants, the planes at z = 1.75 and 5.25 lie exactly on cell faces, and
    set_box() on that state ends the process with "an atom moved beyond the halo region and was lost" (seen on the device; x and y passed there)."""
    if gpu.PRECISION != "double":
        pytest.skip("the identity is checked in the double build")
    eps = 1e-5
    args = ["-x", n[0], "-y", n[1], "-z", n[2], "-l", lat, "-r", 0, "-T", 0] + flags
    with gpu.Simulation(args) as sim:
        sim.compute_force()
        assert rc < 0.5 * sim.box.min()
        box0 = sim.box
        born = sim.born_matrix()
        w0 = np.diag(sim.virial()[0]).copy()
        pairs0 = sim.pair_histogram(1)[1]
        if pot == "lj":
            fr_of = _pair_function("lj")
        else:
            fr_of = _pair_function("eam", sim.eam_table(0), sim.eam_table(1), sim.gather(5).copy())
        _, a_w, _ = _restate(sim.gather(0), box0, rc, fr_of)
        a_w = a_w.sum(0)[:3]
        for a in range(3):
            fd = {}
            for mult in (1.0, 2.0):
                w = {}
                for sign in (+1.0, -1.0):
                    box = box0.copy()
                    box[a] *= 1.0 + sign * mult * eps
                    sim.set_box(box)
                    sim.compute_force()
                    assert np.array_equal(sim.pair_histogram(1)[1], pairs0)
                    w[sign] = np.diag(sim.virial()[0]).copy()
                fd[mult] = -(w[+1.0] - w[-1.0]) / (2.0 * mult * eps)
            sim.set_box(box0)
            for b in range(3):
                want = born[a, b] - (2.0 * w0[a] if a == b else 0.0)
                truncation = 1e-8 * abs(born[a, b]) if pot == "lj" else abs(fd[1.0][b] - fd[2.0][b])
                bound = 2.0 * 1e-11 * a_w[b] / (2.0 * eps) + truncation
                print(pot, a, b, fd[1.0][b], want, abs(fd[1.0][b] - want) / bound)
                assert abs(fd[1.0][b] - want) <= bound, (pot, a, b, fd[1.0][b], want, bound)


# ---------------------------------------------------------------- GPU: methods, layouts, ranks, precisions
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "D"])
def test_methods_and_layouts_agree(gpu, name):
    """thread_atom, thread_atom_nl, cta_cell, -H and -a 1 give the same matrix within twice the bound of the restatement."""
    st, m = STATES[name], _state(gpu, name)
    for method, extra in (("thread_atom", []), ("thread_atom_nl", []), ("cta_cell", []), ("thread_atom", ["-H"]), ("cta_cell", ["-H"]), ("thread_atom", ["-a", 1]),
                          ("cta_cell", ["-a", 1])):
        with gpu.Simulation(st["flags"] + ["-m", method] + extra) as sim:
            got = sim.born_matrix()
        if method == "thread_atom" and not extra:
            assert np.array_equal(got, m["born"])                     # bit-reproducible run to run
        _assert_close(got, m["born"], 2.0 * 1e-11 * m["A"], f"{name} {method} {extra}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C", "EAM8"])
def test_two_ranks_give_the_one_rank_matrix(gpu, tmp_path, name):
    """Two ranks sharing the device (gloo transport): both return the global matrix, the one-rank one within twice the bound of the restatement."""
    import socket
    st, m = ALL_STATES[name], _state(gpu, name)
    assert tuple(m["grid"]) == st["grid"] and m["n"] == st["atoms"]
    _assert_close(m["born"], m["want"], 1e-11 * m["A"], f"{name} one rank")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "born_worker.py"), str(r), "2", port, "2", "1", "1", str(tmp_path), json.dumps(st["flags"])],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
    got = [np.load(os.path.join(tmp_path, f"born_rank{r}.npy")) for r in range(2)]
    assert np.array_equal(got[0], got[1])
    _assert_close(got[0], m["born"], 2.0 * 1e-11 * m["A"], f"{name} two ranks")


SINGLE_RUN = """
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    assert pkg.PRECISION == 'single'
    sim = pkg.Simulation({args!r})
    eam = {eam}
    one = np.zeros(1)
    t = [sim.eam_table(k) for k in range(3)] if eam else None
    np.savez({out!r}, born=sim.born_matrix(), pos=sim.gather(0), box=sim.box, df=sim.gather(5) if eam else one, rhobar=sim.gather(4) if eam else one,
             **({{f"t{{k}}": np.array(t[k][2]) for k in range(3)}} if eam else {{}}), **({{f"x{{k}}": np.array(t[k][:2]) for k in range(3)}} if eam else {{}}))
    sim.close()
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "BI", "C", "D", "E", "F"])
def test_single_precision_build(gpu, tmp_path, name):
    """The float build in a child: all 21 entries against the restatement (in double) of the child's own gathered positions, box, tables, F' and rhobar,
    within (n + c) 2^-24 A_IJ, c = n + 64 (the module docstring derives it).  On analytic LJ (state B) the float matrix also agrees with the double
    build's within that bound.  The tables are left out of that second comparison: rounded to float they are another function, whose second differences
    differ from the double table's by up to 4 x 2^-24 |v| / dx^2, far more than any arithmetic; each build is held to the restatement on its own table."""
    st = STATES[name]
    eam = st["pair"] == "eam"
    out = tmp_path / "single.npz"
    proc = _child(SINGLE_RUN.format(args=list(st["flags"]), out=str(out), eam=eam), env={"COMD_PRECISION": "single"})
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    d = np.load(out)
    tables = None
    if eam:
        t = [(d[f"x{k}"][0], d[f"x{k}"][1], d[f"t{k}"]) for k in range(3)]
        tables = dict(phi=t[0], rho=t[1], emb=t[2], df=d["df"], rhobar=d["rhobar"])
    want, big_a, nbr, knot = _restate_of(st, d["pos"], d["box"], tables, knot_ulps=KNOT_ULPS)
    print(name, "knot term / arithmetic bound", (knot / ((2.0 * nbr + 64.0) * EPS24 * big_a)).max())
    bound = (2.0 * nbr + 64.0) * EPS24 * big_a + knot
    _assert_close(d["born"], want, bound, f"single {name}")
    if name == "B":
        _assert_close(d["born"], _state(gpu, "B")["born"], bound, "single against double, analytic LJ")


# ---------------------------------------------------------------- GPU: the published constants on the device
@pytest.mark.gpu
def test_device_gives_the_published_constants_of_copper(gpu):
    if gpu.PRECISION != "double":
        pytest.skip("checked in the double build")
    with gpu.Simulation(["-x", 6, "-y", 6, "-z", 6, "-l", LAT, "-r", 0, "-T", 0] + MISHIN) as sim:
        got = sim.born_constants()
    for key, want in PUBLISHED.items():
        print(key, got[key] * GPA, want)
        assert abs(got[key] * GPA - want) <= 0.005 * want, (key, got[key] * GPA, want)


# ---------------------------------------------------------------- GPU: comd-hip
def _comd_hip(tmp_path, args, ok=True):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-d", os.path.join(ROOT, "pots")] + [str(a) for a in args], capture_output=True, text=True, cwd=tmp_path,
                          timeout=300)
    assert (proc.returncode == 0) == ok, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    text = ""
    for f in [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]:
        text += (tmp_path / f).read_text()
        os.remove(tmp_path / f)
    return proc.stdout, rows, text


def _elastic_block(yaml):
    block = re.search(r"^Elastic:\n((?:  .*\n)+)", yaml, flags=re.M).group(1)
    return dict(re.findall(r"^  (\w+): (\S+)$", block, flags=re.M))


def _elastic_file(path):
    lines = path.read_text().splitlines()
    data = np.array([[float(x) for x in line.split()] for line in lines if not line.startswith("#")])
    c = np.array([[float(x) for x in line[1:].split()] for line in lines[-6:]])
    return lines, data, c


@pytest.mark.gpu
def test_comd_hip_elastic_at_zero_temperature(gpu, tmp_path):
    """The perfect Mishin lattice at T = 0: five rows, an Elastic block, no fluctuation and no kinetic part, C = Born = the published constants."""
    out, rows, yaml = _comd_hip(tmp_path, ["--elastic"] + MISHIN + ["-T", 0, "-x", 6, "-y", 6, "-z", 6, "-N", 20, "-n", 5])
    header = [line for line in out.splitlines() if line.startswith("#  Loop")][0]
    assert header.split()[-1] == "C11B(GPa)" and len(rows) == 5 and re.search(r"^elastic\s+5\s", out, flags=re.M)
    lines, data, c = _elastic_file(tmp_path / "elastic.dat")
    assert lines[0].startswith("# Elastic: N 864 samples 5 ") and data.shape == (5, 30) and c.shape == (6, 6)
    assert data[:, 0].tolist() == [0.0, 5.0, 10.0, 15.0, 20.0] and np.all(data[:, 1] < 1e-9)
    m = _elastic_block(yaml)
    assert m["samples"] == "5" and m["file"] == "elastic.dat" and float(m["temperature"]) == 0.0
    for key, want in PUBLISHED.items():
        assert float(m[key + "Fluctuation"]) == 0.0 and float(m[key + "Kinetic"]) == 0.0 and float(m[key]) == float(m[key + "Born"])
        assert abs(float(m[key]) - want) <= 0.005 * want
    for r, d in zip(rows, data):
        assert abs(float(r[3].split()[-1]) - (d[9] + d[15] + d[20]) / 3.0) <= 1e-9
    assert abs(c[0, 0] - data[:, 9].mean()) <= 1e-12 * c[0, 0] and np.array_equal(c, c.T)


@pytest.mark.gpu
def test_comd_hip_elastic_at_300_k(gpu, tmp_path, pkg):
    """-T 300 -N 40 -n 2: the rows of elastic.dat fed to elastic_constants() reproduce the YAML figures to 1e-12 relative, and the first eight columns are
    those of the same run without the flag, to the bit."""
    base = MISHIN + ["-T", 300, "-x", 6, "-y", 6, "-z", 6, "-N", 40, "-n", 2]
    out0, rows0, yaml0 = _comd_hip(tmp_path, base)
    assert "C11B" not in out0 and "Elastic" not in yaml0 and not re.search(r"^elastic\s", out0, flags=re.M) and not os.path.exists(tmp_path / "elastic.dat")
    out1, rows1, yaml1 = _comd_hip(tmp_path, base + ["--elastic"])
    assert len(rows1) == 21 and [r[:3] for r in rows1] == [r[:3] for r in rows0]
    lines, data, c = _elastic_file(tmp_path / "elastic.dat")
    assert data.shape == (21, 30)
    born = np.zeros((21, 6, 6))
    for k, (i, j) in enumerate(TRI):
        born[:, i, j] = born[:, j, i] = data[:, 9 + k] / GPA * data[:, 2]
    volume, temperature = data[:, 2].mean(), data[:, 1].mean()
    got = pkg.elastic_constants(born, data[:, 3:9] / GPA, volume, temperature, 864)
    m = _elastic_block(yaml1)
    assert m["samples"] == "21" and abs(float(m["temperature"]) - temperature) <= 1e-12 * temperature
    scale = abs(got["born"][0, 0]) * GPA      # the size of the numbers: C itself can have either sign after 21 correlated samples
    floor = 1e-14 * scale                     # the inputs went through the file: 17 digits of numbers of this size

    def close(key, want):
        assert abs(float(m[key]) - want) <= 1e-12 * abs(want) + floor * (1.0 if key != "anisotropy" else 1.0 / scale), (key, m[key], want)
    for key in ("C11", "C12", "C44"):
        for part, mat in (("", "C"), ("Born", "born"), ("Fluctuation", "fluctuation"), ("Kinetic", "kinetic")):
            x = got[mat]
            close(key + part, {"C11": x[0, 0] + x[1, 1] + x[2, 2], "C12": x[0, 1] + x[0, 2] + x[1, 2], "C44": x[3, 3] + x[4, 4] + x[5, 5]}[key] / 3.0 * GPA)
    for key, want in (("bulkModulus", got["K"] * GPA), ("shearModulusVoigt", got["G_V"] * GPA), ("cauchyPressure", got["cauchy_pressure"] * GPA), ("anisotropy", got["A"])):
        close(key, want)
    assert np.abs(c - got["C"] * GPA).max() <= 1e-12 * scale
    assert float(m["C11Fluctuation"]) < 0.0 and float(m["C11Kinetic"]) > 0.0
