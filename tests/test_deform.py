"""Box deformation (not in the reference, whose box is nx lat for the whole run): comdSetBox / comdRemapBoxGpu, Simulation.set_box / deform /
set_strain_rate, comd-hip --erateX/Y/Z.

CPU: flags, exports, the host geometry after set_box (Domain, LinkCell, periodic shifts; two ranks agree on their shared face), the refusal, the ISA
of the remap kernel.  GPU: after an anisotropic deform the energies and forces are those of an O(N^2) minimum-image restatement on the gathered
positions and the new box; -dU/d(lambda_a) is W_aa of virial(); a round trip returns; every method, cell numbering and stream mode gives the same
state; strain rates give a box that is a pure function of the step count; Verlet lists stay valid under compression; two ranks give the one-rank
state; the executable writes the stress-strain file.  Tolerances are those of tests/golden/reference_values.json and of tests/test_pressure.py.
"""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import device_isa

from test_pressure import (ADAMS, CSRC, GPA, HERE, MISHIN, RC, ROOT, SIGMA, EPS, SINGLE, TOL, _child, _interpolate, _pairs, _rel)

G = json.load(open(os.path.join(HERE, "golden", "reference_values.json")))
SCALE = np.array([1.03, 0.99, 1.01])
EAM_BOX = ["-x", 10, "-y", 8, "-z", 6]                       # unequal axes: a swapped axis shows
LJ25 = ["-x", 8, "-y", 8, "-z", 8, "--ljCutoffSigmas", 2.5]
LJ5 = ["-x", 10, "-y", 10, "-z", 10]
DISORDER = ["-r", 0.1, "-T", 0]
FLAGS = ("erateX", "erateY", "erateZ", "deformStart", "deformFile")


# ---------------------------------------------------------------- CPU: flags, exports, host geometry, ISA
def test_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--erateX', 0.5, '--erateY', -0.2, '--erateZ', 0, '--deformStart', 3, '--deformFile', 'd.dat'],"
                  " host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in FLAGS:
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


def test_profile_mode_refuses_a_strain_rate():
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '-s', '--erateX', 1], host_only=True); print('made')")
    assert proc.returncode != 0 and "made" not in proc.stdout
    lines = [l for l in (proc.stdout + proc.stderr).splitlines() if l.startswith("Error")]
    assert len(lines) == 1 and "-s" in lines[0] and "erate" in lines[0], proc.stdout[-2000:]


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_symbols_are_exported_and_declared(sfx):
    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, lib)], capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"comdRemapBoxGpu", "comdSetListBudgetGpu"} <= exported(f"libcomd_hip{sfx}.so")
    assert {"comdSetBox", "comdDeformTo", "comdSetStrainRate", "comdGetBox", "comdLocalBounds"} <= exported(f"libcomd_host{sfx}.so")
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void comdRemapBoxGpu\(SimGpu\* sim, const double scale\[3\], const real_t localMin\[3\], const real_t localMax\[3\], "
                     r"const real_t boxSize\[3\], comdStream_t stream\);", header, flags=re.M)


@pytest.fixture()
def single_rank(pkg):
    pkg.init_parallel(0, 1, None)
    return pkg


def _face_shift(sim, face):
    import ctypes
    out = (ctypes.c_double * 3)()
    sim.lib.comdFaceShift(sim.ptr, face, out)
    return np.array(out[0:3])


@pytest.mark.parametrize("args", [EAM_BOX + ["-e"], EAM_BOX + ["-e", "-H"], LJ25 + ["-m", "thread_atom_nl"]])
def test_host_only_set_box_updates_every_host_copy(single_rank, args):
    with single_rank.Simulation(args, host_only=True) as sim:
        box0 = sim.box
        assert np.array_equal(box0, sim.box0) and np.array_equal(sim.strain, np.zeros(3))
        rng = np.random.default_rng(7)
        cell_w = box0 / np.array(sim.grid)
        # interior points, away from the cell faces by 5 % of a cell: the scaled point sits at the same fraction of the scaled cell
        frac = rng.uniform(0.05, 0.95, size=(200, 3))
        pts = (rng.integers(0, sim.grid, size=(200, 3)) + frac) * cell_w
        before = [sim.box_from_coord(p) for p in pts]
        new = np.array([float(np.asarray(v, dtype=np.float32)) for v in box0 * SCALE]) if SINGLE else box0 * SCALE
        sim.set_box(new)
        assert np.array_equal(sim.box, new) and np.array_equal(sim.box0, box0)
        assert sim.volume == new[0] * new[1] * new[2]
        assert np.array_equal(sim.strain, new / box0 - 1.0)
        for a in range(3):
            want = np.zeros(3)
            want[a] = new[a]
            assert np.array_equal(_face_shift(sim, 2 * a), want) and np.array_equal(_face_shift(sim, 2 * a + 1), -want)
        lo, hi = sim.local_bounds()
        assert np.array_equal(lo, np.zeros(3)) and np.array_equal(hi, new)
        assert [sim.box_from_coord(p * (new / box0)) for p in pts] == before
        assert len(set(before)) > sim.n_local_boxes // 2                 # the points spread over the grid
        with pytest.raises(RuntimeError):
            sim.deform(1.01)
        with pytest.raises(RuntimeError):
            sim.set_strain_rate((1.0, 0.0, 0.0))


@pytest.mark.parametrize("args,rng_axis", [(EAM_BOX + ["-e"], 0), (LJ25, 1), (LJ25 + ["-m", "thread_atom_nl"], 2)])
def test_set_box_refuses_cells_narrower_than_the_range(single_rank, args, rng_axis):
    with single_rank.Simulation(args, host_only=True) as sim:
        box0 = sim.box
        rc = sim.cutoff * (1.1 if "thread_atom_nl" in args else 1.0)          # the range the grid was built for: the cutoff (+ the default 10 % skin)
        width = box0 / np.array(sim.grid)
        assert np.all(width >= rc)
        bad = box0.copy()
        bad[rng_axis] *= 0.999 * rc / width[rng_axis]
        ok = box0.copy()
        ok[rng_axis] *= 1.001 * rc / width[rng_axis]
        for refused in (bad, box0 * np.array([1.0, -1.0, 1.0]), box0 * np.array([1.0, 1.0, 0.0]), np.array([np.nan, 1.0, 1.0]) * box0):
            with pytest.raises(ValueError):
                sim.set_box(refused)
            assert np.array_equal(sim.box, box0) and np.array_equal(sim.local_bounds()[1], box0)
            assert np.array_equal(_face_shift(sim, 2 * rng_axis)[rng_axis], box0[rng_axis])
        sim.set_box(ok)
        assert not np.array_equal(sim.box, box0)
        sim.set_box(box0)
        assert np.array_equal(sim.box, box0)


def _ranks(mode, grid, args, job, timeout=600):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "deform_worker.py"), str(r), str(world), port, *map(str, grid), mode, json.dumps(args), json.dumps(job)],
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
    return [json.loads(re.search(r"^DEFORM (.*)$", out, flags=re.M).group(1)) for out in outs]


def test_two_host_only_ranks_agree_on_their_shared_face(single_rank):
    with single_rank.Simulation(EAM_BOX + ["-e"], host_only=True) as sim:
        new = (sim.box * SCALE * np.array([1.0 + 1.0 / 3.0, 1.0, 1.0])).tolist()      # an extent whose half is not exact
    r0, r1 = _ranks("host", (2, 1, 1), EAM_BOX + ["-e"], {"box": new})
    assert r0["box"] == r1["box"]
    assert r0["hi"][0] == r1["lo"][0]                                               # the shared face, bit for bit
    assert float.fromhex(r0["lo"][0]) == 0.0 and r1["hi"][0] == r1["box"][0]      # and the periodic one
    assert r0["hi"][1:] == r1["hi"][1:] == r1["box"][1:]


@pytest.mark.parametrize("precision", ["double", "single"])
def test_remap_kernel_exists_and_uses_no_scratch(precision):
    blocks = device_isa.blocks(precision, r"RemapBox\w+")
    assert len(blocks) == 1, sorted(blocks)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
        assert re.search(r"\.amdhsa_group_segment_fixed_size 0\n", block), name          # no LDS


# ---------------------------------------------------------------- numpy restatement: energies and forces
def _lj_restated(pos, extent, rc):
    """ljForce.c:150-220: shifted analytic LJ, per-atom force and energy"""
    i, j, d, r = _pairs(pos, extent, rc)
    s6 = SIGMA ** 6
    rc6 = s6 / rc ** 6
    r6 = s6 / r ** 6
    e = np.zeros(len(pos))
    np.add.at(e, i, 0.5 * 4.0 * EPS * (r6 * (r6 - 1.0) - rc6 * (rc6 - 1.0)))
    fr = 24.0 * EPS * s6 * r ** -8 * (2.0 * s6 * r ** -6 - 1.0)
    f = np.zeros_like(pos)
    np.add.at(f, i, fr[:, None] * d)
    return f, e


def _eam_restated(sim, pos, extent, rc):
    """eam.c:230-400 on the tables the host hands the device: per-atom force and energy"""
    phi, rho, emb = sim.eam_table(0), sim.eam_table(1), sim.eam_table(2)
    i, j, d, r = _pairs(pos, extent, rc)
    vphi, dphi = _interpolate(*phi, r)
    vrho, drho = _interpolate(*rho, r)
    rhobar = np.zeros(len(pos))
    np.add.at(rhobar, i, vrho)
    fe, df = _interpolate(*emb, rhobar)
    e = fe.copy()
    np.add.at(e, i, 0.5 * vphi)
    s = (dphi + (df[i] + df[j]) * drho) / r
    f = np.zeros_like(pos)
    np.add.at(f, i, -s[:, None] * d)
    return f, e


def _restated(kind, sim, pos, extent):
    if kind == "lj":
        return _lj_restated(pos, extent, RC["lj2.5"])
    if kind == "ljI":
        from test_lj_interpolation import lj_table, restated_forces
        return restated_forces(pos, extent, lj_table(), RC["lj5"])
    return _eam_restated(sim, pos, extent, RC[kind])


def _check_restated(kind, sim, where):
    pos, f, e = sim.gather(0), sim.gather(2), sim.gather(3)
    fo, eo = _restated(kind, sim, pos, sim.box)
    ep, _, n = sim.energy()
    df, de, dE = np.abs(f - fo).max() / np.abs(fo).max(), np.abs(e - eo).max(), abs(ep - eo.sum()) / n
    print(f"{kind} {where}: max|df|/max|f| {df:.2e}  max|de| {de:.2e}  |dE|/N {dE:.2e}")
    assert df <= TOL["force_rel_to_max"] and de <= TOL["per_atom_energy_abs"] and dE <= TOL["energy_per_atom_step0"], (kind, where, df, de, dE)


RESTATED = {"lj": LJ25 + DISORDER, "ljI": LJ5 + DISORDER + ["-I"], "adams": EAM_BOX + DISORDER + ADAMS, "mishin": EAM_BOX + DISORDER + MISHIN}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lj", "ljI", "adams", "mishin"])
def test_deformed_state_matches_the_restatement(gpu, kind):
    """Energy, per-atom energies and forces after deform((1.03, 0.99, 1.01)) against the numpy minimum-image sum over the gathered positions in sim.box;
    the same comparison before the deformation is the control that the restatement is sound."""
    with gpu.Simulation(RESTATED[kind]) as sim:
        box0, pos0 = sim.box, sim.gather(0)
        _check_restated(kind, sim, "before")
        sim.deform(SCALE)
        assert np.array_equal(sim.box, box0 * SCALE) and np.array_equal(sim.box0, box0)
        assert abs(sim.volume - np.prod(box0 * SCALE)) <= 1e-15 * sim.volume
        # remap x: every atom at scale * r (one rounding of the scale, one of the product), wrapped into the new box
        pos = sim.gather(0)
        d = pos - pos0 * SCALE
        d -= np.rint(d / sim.box) * sim.box
        assert np.abs(d).max() <= 4 * np.finfo(np.float64).eps * sim.box.max()
        sim.sum_atoms()
        assert sim.n_global == len(pos0)
        _check_restated(kind, sim, "after")


# ---------------------------------------------------------------- strain derivative against the virial
def _energy_at(gpu, args, r0, scale):
    with gpu.Simulation(args) as sim:
        sim.scatter(0, r0)
        sim.redistribute()
        sim.deform(scale)
        return sim.energy()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,h,tol", [("lj", 1e-6, 1e-7), ("mishin", 1e-5, 1e-5)])
def test_strain_derivative_is_the_virial(gpu, kind, h, tol):
    """-dU/d(lambda_a) at lambda = 1 equals W_aa for each axis, U the energy after deform(lambda along a) of a fresh simulation holding the same
    scattered positions; Richardson-extrapolated central differences, tolerances of tests/test_pressure.py's isotropic version.

    The step.  Mishin: the 1e-5 of that test.  LJ: that test's 1e-8 was chosen for trace(W) of LJ 5 sigma; here one diagonal component of the 2.5 sigma
    virial is the signal, W_aa = 128 eV on U = -2.6e3 eV, and a central difference of U costs its rounding, a few ulp = 5e-13 eV, over 2 h W_aa: 2e-7
    relative at h = 1e-8 (measured: 3.2e-7, with W_aa right to every digit the noise leaves), 2e-9 at h = 1e-6, while the truncation error of the
    extrapolation is O(h^4).  What bounds h from above is the kink of the shifted LJ energy at the cutoff: no pair may cross it, so no pair may sit
    within 2 h r of it.  h is therefore 1e-6, or less where the positions demand it: a quarter of the smallest relative gap between a pair distance
    and the cutoff (taken from the positions, never from the result), and at least 1e-7."""
    args = RESTATED[kind]
    with gpu.Simulation(args) as sim:
        r0, box = sim.gather(0).copy(), sim.box
        w, _ = sim.virial()
    if kind == "lj":
        _, _, _, r = _pairs(r0, box, RC["lj2.5"] * 1.001)
        h = min(h, 0.25 * float(np.abs(r / RC["lj2.5"] - 1.0).min()))
        print(f"lj: h = {h:.3e}")
        assert h >= 1e-7, "a pair sits too close to the cutoff for a finite difference of this state"
        assert not np.any(np.abs(r - RC["lj2.5"]) <= 2.0 * h * r), "a pair sits in the finite-difference window of the cutoff"
    for a in range(3):
        def u(lam):
            s = np.ones(3)
            s[a] = lam
            return _energy_at(gpu, args, r0, s)
        d = [(u(1 + s) - u(1 - s)) / (2 * s) for s in (h, 0.5 * h)]
        dU = (4.0 * d[1] - d[0]) / 3.0
        print(f"{kind} axis {a}: W_aa {w[a, a]:.12e}  -dU/dlambda {-dU:.12e}  rel {abs(w[a, a] + dU) / abs(dU):.2e}")
        assert abs(w[a, a] + dU) <= tol * abs(dU), (kind, a, w[a, a], -dU)


# ---------------------------------------------------------------- round trip
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lj", "adams"])
def test_round_trip_returns(gpu, kind):
    with gpu.Simulation(RESTATED[kind]) as sim:
        box0, pos0, (e0, _, n) = sim.box, sim.gather(0), sim.energy()
        sim.deform(SCALE)
        assert abs(sim.energy()[0] - e0) / n > 1e3 * TOL["energy_per_atom_step0"]          # it did go somewhere
        sim.deform(1.0 / SCALE)
        d = sim.gather(0) - pos0
        d -= np.rint(d / box0) * box0
        # two roundings each way (the scale, the product), each of half an ulp of a coordinate below L
        assert np.abs(d).max() <= 4 * np.finfo(np.float64).eps * box0.max(), np.abs(d).max()
        assert abs(sim.energy()[0] - e0) / n <= TOL["energy_per_atom_step0"]
        sim.set_box(box0)
        assert np.array_equal(sim.box, box0) and np.array_equal(sim.strain, np.zeros(3))
        e1, pos1 = sim.energy(), sim.gather(0)
        with pytest.raises(ValueError):
            sim.set_box(box0 * np.array([0.5, 1.0, 1.0]))
        assert np.array_equal(sim.box, box0) and sim.energy() == e1 and np.array_equal(sim.gather(0), pos1)


# ---------------------------------------------------------------- every path, the same state
STATE_RUN = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    out = {{}}
    for name, args in {legs!r}.items():
        with pkg.Simulation(args) as sim:
            sim.deform({scale!r})
            w, k = sim.virial()
            out[name] = [sim.energy()[0], sim.energy()[2], w.tolist()]
    print("STATES", json.dumps(out))
"""


def _legs(base, methods):
    return {" ".join([m] + [str(x) for x in extra]): base + ["-m", m] + extra for m in methods for extra in ([], ["-H"], ["-a", 1])}


def _states(gpu, legs):
    out = {}
    for name, args in legs.items():
        with gpu.Simulation(args) as sim:
            sim.deform(SCALE)
            w, _ = sim.virial()
            out[name] = (sim.energy()[0], sim.energy()[2], w)
    return out


def _assert_same(states, first, e_tol, w_tol):
    e0, n, w0 = states[first]
    for name, (e, _, w) in states.items():
        print(f"{name}: |dE|/N {abs(e - e0) / n:.2e}  virial rel {_rel(w, w0):.2e}")
        assert abs(e - e0) / n <= e_tol and _rel(w, w0) <= w_tol, (name, e, e0, _rel(w, w0))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["lj", "ljI", "eam"])
def test_every_path_gives_the_same_deformed_state(gpu, family):
    """thread_atom, cta_cell and thread_atom_nl, each plain, with -H and with -a 1, after the same deform: the same energy and pair virial to the 1e-12
    of test_pressure.py's test_methods_and_layouts_agree.  The -I table is another potential than the analytic LJ (they differ by the interpolation
    error): its legs (the thread_atom methods, which are the ones -I runs on) are compared with each other."""
    if family == "lj":
        legs = _legs(LJ25 + DISORDER, ["thread_atom", "cta_cell", "thread_atom_nl"])
    elif family == "ljI":
        legs = _legs(LJ5 + DISORDER + ["-I"], ["thread_atom", "thread_atom_nl"])
    else:
        legs = _legs(EAM_BOX + DISORDER + ADAMS, ["cta_cell", "thread_atom", "thread_atom_nl"])
    _assert_same(_states(gpu, legs), next(iter(legs)), TOL["energy_per_atom_step0"], 1e-12)


@pytest.mark.gpu
def test_eam_thread_atom_sizes_do_not_follow_the_stretched_cells(gpu):
    """The launch layer of EAM thread_atom sizes its row threads, and with them the stride of its row buffers, from the atoms a cell holds at the lattice's
    density; an affine stretch widens the cells WITH their atoms, so the estimate must stay the one of the allocation.  11^3 has the cell width of the 40^3
    tensile example (4.97 A; a 4 x 4 brick of 166 atoms, 192 row threads): derived from the stretched volume the count would pass 192 at 8 %.  A 9 % stretch
    along x, then three steps: thread_atom gives cta_cell's energy, forces and pair virial."""
    args = ["-x", 11, "-y", 11, "-z", 11] + DISORDER + ADAMS
    got = {}
    for method in ("cta_cell", "thread_atom"):
        with gpu.Simulation(args + ["-m", method]) as sim:
            sim.deform((1.09, 1.0, 1.0))
            sim.step(3)
            w, _ = sim.virial()
            got[method] = (sim.energy(), sim.gather(2), w)
    (e0, f0, w0), (e1, f1, w1) = got["cta_cell"], got["thread_atom"]
    df = np.abs(f1 - f0).max() / np.abs(f0).max()
    print(f"thread_atom vs cta_cell at 9 %: |dE|/N {abs(e1[0] - e0[0]) / e0[2]:.2e}  max|df|/max|f| {df:.2e}  virial rel {_rel(w1, w0):.2e}")
    assert abs(e1[0] - e0[0]) / e0[2] <= TOL["energy_per_atom_step0"] and df <= 100 * TOL["force_rel_to_max"] and _rel(w1, w0) <= 100 * TOL["force_rel_to_max"]


@pytest.mark.gpu
def test_every_path_gives_the_same_deformed_state_single_precision(gpu):
    """The float build: LJ and EAM legs against each other at the single tolerances (1e-5 of the largest virial component, as test_single_precision_virial),
    and against the double build's state."""
    tol = G["tolerances_single"]
    legs = {**{"lj " + k: v for k, v in _legs(LJ25 + DISORDER, ["thread_atom", "cta_cell", "thread_atom_nl"]).items() if "-" not in k},
            **{"eam " + k: v for k, v in _legs(EAM_BOX + DISORDER + ADAMS, ["cta_cell", "thread_atom", "thread_atom_nl"]).items() if "-" not in k}}
    proc = _child(STATE_RUN.format(legs=legs, scale=SCALE.tolist()), env={"COMD_PRECISION": "single"})
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = {k: (v[0], v[1], np.array(v[2])) for k, v in json.loads(re.search(r"^STATES (.*)$", proc.stdout, flags=re.M).group(1)).items()}
    for pot in ("lj", "eam"):
        mine = {k: v for k, v in got.items() if k.startswith(pot)}
        _assert_same(mine, next(iter(mine)), tol["energy_per_atom_step0"], 1e-5)
        name = next(iter(mine))
        with gpu.Simulation(legs[name]) as sim:
            sim.deform(SCALE)
            w, _ = sim.virial()
            e, _, n = sim.energy()
        assert abs(mine[name][0] - e) / n <= tol["energy_per_atom_step0"] and _rel(mine[name][2], w) <= 1e-5


# ---------------------------------------------------------------- strain rate
RATES = np.array([0.5, -0.2, 0.0])
HOT = ["-r", 0.1, "-T", 600]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [LJ25 + HOT, EAM_BOX + HOT + ADAMS + ["-m", "cta_cell"], EAM_BOX + HOT + ADAMS + ["-m", "thread_atom_nl"]])
def test_strain_rate_box_is_a_function_of_the_step_count(gpu, args):
    with gpu.Simulation(args) as a, gpu.Simulation(args) as b:
        box0, n = a.box, a.n_global
        a.set_strain_rate(RATES)
        b.set_strain_rate(RATES)
        a.step(10)
        assert np.array_equal(a.box, box0 * (1 + RATES * 10 / 1000)), (a.box, box0 * (1 + RATES * 10 / 1000))
        assert np.array_equal(a.box0, box0)
        b.step(4)
        assert np.array_equal(b.box, box0 * (1 + RATES * 4 / 1000))
        b.step(6)
        assert np.array_equal(a.box, b.box)
        (ea, ka, _), (eb, kb, _) = a.energy(), b.energy()
        print(f"step(10) vs step(4); step(6): |dE|/N {abs((ea + ka) - (eb + kb)) / n:.2e}")
        assert abs((ea + ka) - (eb + kb)) / n <= TOL["energy_per_atom_trace"]
        for s in (a, b):
            s.sum_atoms()
            assert s.n_global == n
        assert a.step_count == b.step_count == 10
        with pytest.raises(ValueError):
            a.set_strain_rate(0.5)
        with pytest.raises(ValueError):
            a.set_strain_rate((0.5, float("nan"), 0.0))


@pytest.mark.gpu
def test_deform_start_delays_the_strain(gpu):
    """--erateX with --deformStart 3: the first three steps are those of an unstrained run, to the bit; from then on the strain counts the strained steps."""
    rate = np.array([0.5, 0.0, 0.0])
    with gpu.Simulation(LJ25 + HOT + ["--erateX", 0.5, "--deformStart", 3]) as a, gpu.Simulation(LJ25 + HOT) as b:
        box0 = a.box
        a.step(3)
        b.step(3)
        assert np.array_equal(a.box, box0) and np.array_equal(a.gather(0), b.gather(0)) and a.energy() == b.energy()
        a.step(2)
        assert np.array_equal(a.box, box0 * (1 + rate * 2 / 1000)) and a.step_count == 5


@pytest.mark.gpu
@pytest.mark.parametrize("args", [LJ25 + HOT, EAM_BOX + HOT + ADAMS + ["-m", "thread_atom_nl"]])
def test_zero_rates_change_nothing(gpu, args):
    """A rate set and taken back before any step: the following steps are those of a simulation that never had one, to the bit."""
    with gpu.Simulation(args) as a, gpu.Simulation(args) as b:
        a.set_strain_rate(RATES)
        a.set_strain_rate((0, 0, 0))
        a.step(7)
        b.step(7)
        assert np.array_equal(a.box, b.box)
        for which in (0, 1, 2):
            assert np.array_equal(a.gather(which), b.gather(which)), which
        assert a.energy() == b.energy() and a.nl_builds == b.nl_builds


# ---------------------------------------------------------------- Verlet lists under compression and tension
def _strained_nl(gpu, args, rate):
    with gpu.Simulation(args + ["-m", "thread_atom_nl", "--erateX", rate]) as sim:
        sim.step(40)
        return {"pos": sim.gather(0), "f": sim.gather(2), "e": sim.energy(), "box": sim.box, "builds": sim.nl_builds}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,args", [("lj", LJ25 + HOT), ("adams", EAM_BOX + HOT + ADAMS)])
def test_lists_stay_valid_under_compression(gpu, kind, args):
    """thread_atom_nl at --erateX -2 for 40 steps (8 % compression: the affine share of the skin is used up several times over): the forces and the energy
    of the final state are those a cell method computes on the same positions in the same box, to the parity tolerance; the lists were built more
    often than without strain, and in tension (+2) not more often than that by more than one."""
    free = _strained_nl(gpu, args, 0)
    for rate in (-2, 2):
        run = _strained_nl(gpu, args, rate)
        assert np.array_equal(run["box"], free["box"] * np.array([1 + rate * 40 / 1000, 1, 1]))
        fo = eo = None
        for method in ("cta_cell", "thread_atom_nl"):
            with gpu.Simulation(args + ["-m", method]) as ref:
                try:
                    ref.set_box(run["box"])
                except ValueError:
                    # EAM, compressed: the cells of the cell methods (7 of 5.16 A along x, for a cutoff of 4.95 A) cannot follow 8 % and set_box must refuse;
                    # the reference is then a fresh list simulation (wider cells, lists built on exactly these positions) and the numpy restatement
                    assert kind == "adams" and rate < 0 and method == "cta_cell"
                    continue
                ref.scatter(0, run["pos"])
                ref.redistribute()
                ref.compute_force()
                ref.kinetic_energy()
                fo, eo = ref.gather(2), ref.energy()[0]
                if method == "thread_atom_nl":
                    fr, er = _eam_restated(ref, run["pos"], run["box"], RC["adams"])
                    assert np.abs(fo - fr).max() <= TOL["force_rel_to_max"] * np.abs(fr).max() and abs(eo - er.sum()) / len(er) <= TOL["energy_per_atom_step0"]
                break
        df, dE = np.abs(run["f"] - fo).max() / np.abs(fo).max(), abs(run["e"][0] - eo) / run["e"][2]
        print(f"{kind} rate {rate}: builds {run['builds']} (free {free['builds']})  max|df|/max|f| {df:.2e}  |dE|/N {dE:.2e}")
        assert df <= TOL["force_rel_to_max"] and dE <= TOL["energy_per_atom_step0"], (kind, rate, df, dE)
        if rate < 0:
            assert run["builds"] > free["builds"], (run["builds"], free["builds"])
        else:
            assert run["builds"] <= free["builds"] + 1, (run["builds"], free["builds"])


# ---------------------------------------------------------------- two ranks
@pytest.mark.gpu
@pytest.mark.parametrize("args", [LJ25 + HOT, EAM_BOX + HOT + ADAMS + ["-m", "cta_cell"]])
def test_two_ranks_give_the_one_rank_state(gpu, args):
    """2 x 1 x 1 ranks sharing the device (gloo transport): strain along x for 10 steps, then a deform along y; energy and tensors are the one-rank
    run's at the tolerances of the multi-rank trajectory tests, the box is the same on both ranks, to the bit."""
    job = {"rates": [1.0, 0.0, 0.0], "steps": 10, "scale": [1.0, 1.01, 1.0]}
    with gpu.Simulation(args) as sim:
        sim.set_strain_rate(job["rates"])
        sim.step(job["steps"])
        sim.set_strain_rate((0, 0, 0))
        sim.deform(job["scale"])
        w0, k0 = sim.virial()
        ep, ek, n = sim.energy()
        box = [float.hex(v) for v in sim.box]
    for r in _ranks("gpu", (2, 1, 1), args, job):
        assert r["box"] == box
        assert r["energy"][2] == n
        dE = abs((r["energy"][0] + r["energy"][1]) - (ep + ek)) / n
        print(f"|dE|/N {dE:.2e}  W rel {_rel(np.array(r['w']), w0):.2e}  K rel {_rel(np.array(r['k']), k0):.2e}")
        assert dE <= TOL["energy_per_atom_trace"]
        assert _rel(np.array(r["w"]), w0) <= 100 * TOL["force_rel_to_max"] and _rel(np.array(r["k"]), k0) <= 100 * TOL["force_rel_to_max"]


# ---------------------------------------------------------------- the executable
def _comd_hip(tmp_path, extra, expect_ok=True):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-e", "-x", "10", "-y", "8", "-z", "6", "-T", "300", "-N", "40", "-n", "10", "-d", os.path.join(ROOT, "pots")]
                          + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    text = "".join((tmp_path / y).read_text() for y in yaml)
    for y in yaml:
        os.remove(tmp_path / y)
    if expect_ok:
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    return proc, text


@pytest.mark.gpu
def test_comd_hip_writes_the_stress_strain_file(gpu, tmp_path):
    plain, yaml0 = _comd_hip(tmp_path, [])
    assert "V/V0" not in plain.stdout and "Sxx" not in plain.stdout and "Deform" not in yaml0 and not (tmp_path / "deform.dat").exists()
    assert not re.search(r"^\s*deform\s", plain.stdout, flags=re.M)
    run, yaml1 = _comd_hip(tmp_path, ["--erateX", "1"])
    head = [l for l in run.stdout.splitlines() if "Performance" not in l and "Loop" in l and "Time(fs)" in l]
    assert len(head) == 1 and head[0].rstrip().endswith("V/V0         Sxx(GPa)"), head
    rows = [l.split() for l in run.stdout.splitlines() if re.match(r"^\s+\d+\s+\d+\.\d\d\s", l)]
    rows0 = [l.split() for l in plain.stdout.splitlines() if re.match(r"^\s+\d+\s+\d+\.\d\d\s", l)]
    assert [r[0] for r in rows] == ["0", "10", "20", "30", "40"] and all(len(r) == len(q) + 2 for r, q in zip(rows, rows0))
    assert rows[0][:5] == rows0[0][:5]                                   # step 0 is the unstrained state
    lines = (tmp_path / "deform.dat").read_text().splitlines()
    assert lines[0].startswith("#") and " N 1920 " in lines[0] and "rates" in lines[0] and "L0" in lines[0]
    data = np.array([[float(v) for v in l.split()] for l in lines[1:]])
    assert data.shape == (5, 15)
    lx0 = data[0, 5]
    assert np.array_equal(data[:, 0], [0, 10, 20, 30, 40]) and np.array_equal(data[:, 1], [0, 10, 20, 30, 40])
    for k in range(5):
        assert data[k, 5] == lx0 * (1 + 1.0 * (10 * k) / 1000) and data[k, 2] == data[k, 5] / lx0 - 1.0
        assert abs(data[k, 2] - 0.01 * k) <= 1e-15
        assert np.array_equal(data[k, 3:5], [0.0, 0.0]) and np.array_equal(data[k, 6:8], data[0, 6:8])
        assert abs(data[k, 8] - data[k, 5] * data[k, 6] * data[k, 7]) <= 1e-12 * data[k, 8]
        assert abs(float(rows[k][-2]) - data[k, 8] / data[0, 8]) <= 1e-9 and abs(float(rows[k][-1]) - data[k, 9]) <= 1e-9
    assert data[-1, 9] > 0.0 and data[-1, 9] > data[0, 9], data[:, 9]
    block = re.search(r"^Deform:\n((?:  .*\n)+)", yaml1, flags=re.M)
    assert block, yaml1[-2000:]
    for key in ("rates", "startStep", "finalStrain", "finalBox", "file", "samples"):
        assert re.search(rf"^  {key}: ", block.group(1), flags=re.M), key
    assert re.search(r"^  samples: 5$", block.group(1), flags=re.M) and re.search(r"^  file: deform.dat$", block.group(1), flags=re.M)
    assert re.search(r"^\s*deform\s+40\s", run.stdout, flags=re.M)
    os.remove(tmp_path / "deform.dat")
    # a box the grid cannot follow: an Error line and a non-zero exit, not a device status abort
    bad, _ = _comd_hip(tmp_path, ["--erateX", "-100"], expect_ok=False)
    errors = [l for l in (bad.stdout + bad.stderr).splitlines() if l.startswith("Error")]
    assert bad.returncode != 0 and bad.returncode not in (-6, -11, 134, 139) and len(errors) == 1 and "narrower" in errors[0], (bad.returncode, bad.stdout[-1500:], bad.stderr[-1500:])
    assert "Error in file" not in bad.stderr and "overflow" not in bad.stderr
