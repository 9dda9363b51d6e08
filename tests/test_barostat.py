"""The Berendsen barostat and the per-step pressure it reads (not in the reference, whose box is fixed): computeVirialFdotr / comdVirialFdotr /
Simulation.virial_fdotr, comdPeriodicFacePairs, comdBerendsenScale, comdSetBarostat, comd-hip --baro*.

CPU: flags and refusals, exports, the scale rule against its formula, the work list of the face kernel against the cell tuples (one rank, -H, two gloo ranks),
the ISA of the two new kernels.  GPU: virial_fdotr() against virial(), the pair walk that was there before; the integrated barostat against a replay with
virial() -> berendsen_scale -> deform(); bit-reproducibility across calls; the list method under compression; an NPT direction test; the executable.

Boxes.  The 2-cell EAM box is 3 x 5 x 8 (grid 2, 3, 5), tests/test_two_cell_boxes.py's "eam_mixed": 2 x 4 x 4 is narrower than two cutoffs and is refused by
sanityChecks (that file tests the refusal).  LJ 5 sigma 7 x 10 x 7 (grid 2, 3, 2) has a 2-cell and a 3-cell axis, 10 x 10 x 10 is the 3-cell box.
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

from test_pressure import ADAMS, CSRC, GPA, HERE, MISHIN, ROOT, SINGLE, TOL, _child, _rel

PRECISION = "single" if SINGLE else "double"
REAL = np.float32 if SINGLE else np.float64
EPS_REAL = float(np.finfo(np.float32 if SINGLE else np.float64).eps)
SCALE = np.array([1.03, 0.99, 1.01])
EAM_BOX = ["-e", "-x", 10, "-y", 8, "-z", 6]                    # unequal axes: a swapped axis shows
EAM_2CELL = ["-e", "-x", 3, "-y", 5, "-z", 8]                   # grid 2, 3, 5
LJ25 = ["-x", 8, "-y", 8, "-z", 8, "--ljCutoffSigmas", 2.5]
LJ5_MIXED = ["-x", 7, "-y", 10, "-z", 7]                        # grid 2, 3, 2
LJ5_3CELL = ["-x", 10, "-y", 10, "-z", 10]                      # grid 3, 3, 3
DISORDER = ["-r", 0.1, "-T", 0]
FLAGS = ("baro", "baroP", "baroTau", "baroModulus", "baroEvery", "baroAxes", "baroIso", "baroStart", "baroFile")
# waves per SIMD the two kernels are written for: the atoms kernel is a stream over r, f and p, the face kernel holds one atom and one pair per lane
FDOTR_WAVES = {"double": 7, "single": 8}
# largest |W_fdotr - W_pair| in eV measured on the GPU over the states of test_virial_fdotr_matches_the_pair_walk (DESIGN.md section 3 has the table), x 10
# double: 1.681e-12 (LJ 5 sigma, 2-cell box, 20 steps, strained box).  single: 3.398e-02, the -P state -- the force kernels and the pair functor evaluate the r^2 splines in
# different arithmetic, and in float that shows (tolerances_single_spline of tests/golden/reference_values.json is the same effect); without -P the largest is 8.249e-04
W_TOL = {"double": 10 * 1.681e-12, "single": 10 * 3.398e-02}[PRECISION]
# the caps: what any logic error exceeds by orders of magnitude (a missing or mis-signed face pair is >= L |f| ~ 1 eV), as a share of N eV + max|W| + sum |r||F|
W_CAP = 1e-5 if SINGLE else 1e-11
# the boxes of the integrated barostat against the replay.  Double: the issue's 1e-10.  Single: a box is a float, and each of the 8 couplings rounds mu and L mu once in
# either run: 16 roundings
BOX_TOL = 16 * EPS_REAL if SINGLE else 1e-10
# K: the same terms in another order.  Double: 1e-13.  Single: lanes add in float, a lane of either kernel adds at most 64 terms here and the workgroups add in double, so
# the two sums differ by at most (64 + 8) float roundings of the largest component
K_TOL = 72 * EPS_REAL if SINGLE else 1e-13


# ---------------------------------------------------------------- CPU: flags, refusals, exports
def test_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("s = pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--baro', '--baroP', 1.5, '--baroTau', 500, '--baroModulus', 100, '--baroEvery', 5, '--baroAxes', 'yz',"
                  " '--baroIso', '--baroStart', 3, '--baroFile', 'b.dat', '--erateX', 0.5], host_only=True); print('made', json.dumps(dict(s.barostat, pressure_gpa=None))); s.close()")
    assert proc.returncode == 0 and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = json.loads(re.search(r"^made (.*)$", proc.stdout, flags=re.M).group(1))
    assert got == {"on": True, "pressure_gpa": None, "tau_fs": 500.0, "modulus_gpa": 100.0, "every": 5, "axes": "yz", "iso": True}, got
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in FLAGS:
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


@pytest.mark.parametrize("extra,word", [(["-s"], "-s"), (["--erateY", 0.5], "erate"), (["--baroEvery", 0], "baroEvery"), (["--baroAxes", "xq"], "baroAxes"),
                                        (["--baroAxes", "xx"], "baroAxes"), (["--baroAxes", ""], "baroAxes"), (["--baroTau", 0], "baroTau"), (["--baroModulus", -1], "baroModulus"),
                                        (["--baroEvery", 2000], "baroTau"), (["--baroP", "nan"], "baroP"), (["--baroStart", -1], "baroStart")])
def test_each_refusal_is_one_error_line(extra, word):
    proc = _child(f"pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--baro'] + {extra!r}, host_only=True); print('made')")
    assert proc.returncode != 0 and "made" not in proc.stdout, proc.stdout[-2000:]
    lines = [l for l in (proc.stdout + proc.stderr).splitlines() if l.startswith("Error")]
    assert len(lines) == 1 and word in lines[0], (lines, proc.stdout[-2000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_symbols_are_exported_and_declared(sfx):
    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, lib)], capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"computeVirialFdotr", "comdSetFacePairsGpu"} <= exported(f"libcomd_hip{sfx}.so")
    assert {"comdVirialFdotr", "comdPeriodicFacePairs", "comdBerendsenScale", "comdSetBarostat", "comdGetBarostat"} <= exported(f"libcomd_host{sfx}.so")
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeVirialFdotr\(SimGpu\* sim, const double box\[3\], real_t\* out12\);", header, flags=re.M)
    host = open(os.path.join(CSRC, "host", "comd_host.h")).read()
    assert re.search(r"^int  comdPeriodicFacePairs\(SimFlat\* s, int\* out5, int cap\);", host, flags=re.M)
    assert re.search(r"^void comdVirialFdotr\(SimFlat\* s, double out\[13\]\);", host, flags=re.M)
    assert re.search(r"^int  comdBerendsenScale\(const double p\[3\], const double target\[3\], double dtCoupling, double tau, double modulus, int axesMask, int iso, double mu\[3\]\);",
                     host, flags=re.M)
    assert re.search(r"^int  comdSetBarostat\(SimFlat\* s, int on, const double targetGPa\[3\], double tauFs, double modulusGPa, int every, int axesMask, int iso\);", host, flags=re.M)


@pytest.fixture()
def single_rank(pkg):
    pkg.init_parallel(0, 1, None)
    return pkg


def test_host_only_simulation_has_no_barostat_to_set(single_rank):
    with single_rank.Simulation(LJ5_3CELL, host_only=True) as sim:
        with pytest.raises(RuntimeError):
            sim.set_barostat()
        with pytest.raises(RuntimeError):
            sim.virial_fdotr()
        assert sim.barostat["on"] is False


# ---------------------------------------------------------------- CPU: the scale rule
def _ulp_apart(a, b):
    return np.abs(a - b) <= np.spacing(np.abs(b))


def test_berendsen_scale_is_the_formula(pkg):
    rng = np.random.default_rng(5)
    for _ in range(200):
        p, target = rng.normal(0, 5, 3), rng.normal(0, 2, 3)
        dt, tau, modulus = rng.uniform(1, 50), rng.uniform(50, 2000), rng.uniform(20, 300)
        want = np.cbrt(1.0 - (dt / tau) * (target - p) / modulus)
        assert np.all(_ulp_apart(pkg.berendsen_scale(p, target, dt, tau, modulus), want))
        for axes in ("x", "yz", "zx", "y"):
            on = np.array([c in axes for c in "xyz"])
            got = pkg.berendsen_scale(p, target, dt, tau, modulus, axes=axes)
            assert np.all(got[~on] == 1.0) and np.all(_ulp_apart(got[on], want[on])), (axes, got, want)
            iso = pkg.berendsen_scale(p, target, dt, tau, modulus, axes=axes, iso=True)
            one = np.cbrt(1.0 - (dt / tau) * (target[on].mean() - p[on].mean()) / modulus)
            assert np.all(iso[~on] == 1.0) and np.all(iso[on] == iso[on][0]) and _ulp_apart(iso[on][0], one), (axes, iso, one)
        assert np.array_equal(pkg.berendsen_scale(p, p, dt, tau, modulus), np.ones(3))
        assert np.array_equal(pkg.berendsen_scale(p, p, dt, tau, modulus, axes="xz", iso=True), np.ones(3))
    # compressive excess pressure expands, and a scalar serves all three axes
    assert np.all(pkg.berendsen_scale(3.0, 0.0, 10, 1000, 140) > 1.0) and np.all(pkg.berendsen_scale(-3.0, 0.0, 10, 1000, 140) < 1.0)
    assert np.array_equal(pkg.berendsen_scale(0.0, 0.0, 1000, 1000, 140), np.ones(3))          # dt = tau is allowed


@pytest.mark.parametrize("kw", [dict(p=float("nan")), dict(p=float("inf")), dict(target=float("nan")), dict(dt_coupling=float("nan")), dict(tau=0.0), dict(tau=-5.0),
                                dict(tau=float("inf")), dict(modulus=0.0), dict(modulus=-140.0), dict(modulus=float("nan")), dict(dt_coupling=1000.5), dict(axes="")])
def test_berendsen_scale_refuses(pkg, kw):
    args = dict(p=1.0, target=0.0, dt_coupling=10.0, tau=1000.0, modulus=140.0)
    args.update(kw)
    with pytest.raises(ValueError):
        pkg.berendsen_scale(**args)


# ---------------------------------------------------------------- CPU: the work list
def _tuples(sim):
    g = sim.grid
    return {sim.lib.comdSimBoxFromTuple(sim.ptr, ix, iy, iz): (ix, iy, iz) for ix in range(-1, g[0] + 1) for iy in range(-1, g[1] + 1) for iz in range(-1, g[2] + 1)}


def _sign(c, g):
    return -1 if c == -1 else 1 if c == g else 0


@pytest.mark.parametrize("args,grid", [(EAM_2CELL, (2, 3, 5)), (EAM_2CELL + ["-H"], (2, 3, 5)), (LJ5_MIXED, (2, 3, 2)), (LJ5_3CELL, (3, 3, 3)), (LJ5_3CELL + ["-H"], (3, 3, 3)),
                                       (LJ25 + ["-m", "thread_atom_nl"], (4, 4, 4))])
def test_periodic_face_pairs_on_one_rank(single_rank, args, grid):
    with single_rank.Simulation(args, host_only=True) as sim:
        g = tuple(sim.grid)
        assert g == grid
        n_local = g[0] * g[1] * g[2]
        rows, t = sim.periodic_face_pairs(), _tuples(sim)
        assert rows.dtype == np.int32 and rows.shape == (27 * n_local - (3 * g[0] - 2) * (3 * g[1] - 2) * (3 * g[2] - 2), 5)
        assert len({(int(r[0]), int(r[1])) for r in rows}) == len(rows)                       # no (cell, halo cell) twice
        per_cell = {}
        for i, j, sx, sy, sz in rows.tolist():
            assert 0 <= i < n_local <= j < len(t), (i, j)                                      # the second cell is a halo cell
            ci, cj = t[i], t[j]
            assert all(abs(cj[a] - ci[a]) <= 1 for a in range(3)), (ci, cj)                    # and a stencil neighbour
            assert (sx, sy, sz) == tuple(_sign(cj[a], g[a]) for a in range(3)) != (0, 0, 0), (ci, cj, sx, sy, sz)
            per_cell[i] = per_cell.get(i, 0) + 1
        # every halo neighbour of every local cell is there
        for i in range(n_local):
            want = sum(1 for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
                       if any(not 0 <= t[i][a] + d < g[a] for a, d in enumerate((dx, dy, dz))))
            assert per_cell.get(i, 0) == want, (i, t[i])


def _face_ranks(grid, args, timeout=300):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "barostat_worker.py"), str(r), str(world), port, *map(str, grid), json.dumps(args)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, OMP_NUM_THREADS="2")) for r in range(world)]
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
    return [json.loads(re.search(r"^FACEPAIRS (.*)$", out, flags=re.M).group(1)) for out in outs]


def test_two_ranks_along_x_wrap_at_the_outer_faces_only():
    """EAM 10 x 8 x 6 on 2 x 1 x 1 ranks: a rank's x halo is a periodic image at its outer face only (rank 0 below, rank 1 above); across the shared face the sign is 0,
    and such a row is listed only when it wraps in y or z.  The y and z signs of every row are those of the cell tuples, as on one rank."""
    r0, r1 = _face_ranks((2, 1, 1), EAM_BOX)
    for r, outer in ((r0, -1), (r1, 1)):
        g = r["grid"]
        seen = set()
        for ci, cj, sx, sy, sz in r["rows"]:
            assert (sy, sz) == (_sign(cj[1], g[1]), _sign(cj[2], g[2]))
            assert sx == (outer if _sign(cj[0], g[0]) == outer else 0), (r["rank"], ci, cj, sx)
            assert (sx, sy, sz) != (0, 0, 0)
            seen.add((tuple(ci), tuple(cj)))
        assert len(seen) == len(r["rows"])
        # all halo neighbours but those that lie across the shared face alone
        n_local = g[0] * g[1] * g[2]
        halo_pairs = 27 * n_local - (3 * g[0] - 2) * (3 * g[1] - 2) * (3 * g[2] - 2)
        inner = sum(1 for iy in range(g[1]) for iz in range(g[2]) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if 0 <= iy + dy < g[1] and 0 <= iz + dz < g[2])
        assert len(r["rows"]) == halo_pairs - inner, (len(r["rows"]), halo_pairs, inner)


# ---------------------------------------------------------------- CPU: ISA
@pytest.mark.parametrize("precision", ["double", "single"])
def test_fdotr_kernels_use_no_scratch_and_keep_their_waves(precision):
    blocks = device_isa.blocks(precision, r"Fdotr_\w+")
    names = sorted(blocks)
    assert len(names) == 5, names
    assert sum("Fdotr_atoms" in n for n in names) == 1
    for pair in ("VirialLj", "VirialLjTable", "VirialEamILb0E", "VirialEamILb1E"):
        assert any("Fdotr_face" in n and pair in n for n in names), (pair, names)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    device_isa.assert_keeps_waves(blocks, "Fdotr_atoms", FDOTR_WAVES[precision])
    for pair in ("8VirialLjE", "13VirialLjTableE", "9VirialEamILb0EE", "9VirialEamILb1EE"):
        device_isa.assert_keeps_waves(blocks, f"Fdotr_faceI{pair}", FDOTR_WAVES[precision])


# ---------------------------------------------------------------- GPU: virial_fdotr() against virial()
def _compare(sim, where, worst):
    """W and K of virial_fdotr() against virial() on the current state; prints the figures, then asserts"""
    w0, k0 = sim.virial()
    w1, k1 = sim.virial_fdotr()
    w2, k2 = sim.virial_fdotr()
    r, f = sim.gather(0), sim.gather(2)
    scale = sim.n_global * 1.0 + np.abs(w0).max() + float((np.linalg.norm(r, axis=1) * np.linalg.norm(f, axis=1)).sum())
    dw, dk = float(np.abs(w1 - w0).max()), _rel(k1, k0) if np.abs(k0).max() > 0 else float(np.abs(k1).max())
    print(f"FDOTR {PRECISION} {where}: max|dW| {dw:.3e} eV  cap {W_CAP * scale:.3e}  max|W| {np.abs(w0).max():.3e}  max|F| {np.abs(f).max():.2e}  K rel {dk:.2e}")
    worst.append(dw)
    assert np.array_equal(w1, w2) and np.array_equal(k1, k2), where                            # two calls, the same bits
    assert np.array_equal(w1, w1.T)
    assert dk <= K_TOL, (where, dk)
    assert dw <= W_CAP * scale, (where, dw, W_CAP * scale)
    assert dw <= W_TOL, (where, dw, W_TOL)


BOXES = {"lj5_2cell": LJ5_MIXED, "lj25": LJ25, "eam": EAM_BOX}
LIST_SKIN = {"lj5_2cell": ["-S", 0.03]}          # the 2-cell LJ box holds two list cells at this skin only (tests/test_two_cell_boxes.py)


def _method_flags(box, method):
    return ["-m", method] + (LIST_SKIN.get(box, []) if method == "thread_atom_nl" else [])


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["thread_atom", "cta_cell", "thread_atom_nl"])
@pytest.mark.parametrize("box", list(BOXES))
def test_virial_fdotr_matches_the_pair_walk(gpu, box, method):
    """The step-0 lattice (F ~ 0: the face kernel carries W), the state after 20 steps at 600 K and the strained box after it; -r 0.1 -T 0 disorder (large F, off-diagonals)
    and its strained box.  With lists also after steps that did not rebuild them: the cells are then stale, the identity is not."""
    args, worst = BOXES[box] + _method_flags(box, method), []
    with gpu.Simulation(args) as sim:
        _compare(sim, f"{box} {method} lattice", worst)
        if method == "thread_atom_nl":
            builds = sim.nl_builds
            sim.step(3)
            assert sim.nl_builds == builds
            _compare(sim, f"{box} {method} 3 steps without a rebuild", worst)
            sim.step(17)
        else:
            sim.step(20)
        _compare(sim, f"{box} {method} 20 steps at 600 K", worst)
        sim.set_box(sim.box * SCALE)
        _compare(sim, f"{box} {method} 20 steps, strained box", worst)
    with gpu.Simulation(args + DISORDER) as sim:
        _compare(sim, f"{box} {method} disorder", worst)
        sim.set_box(sim.box * SCALE)
        _compare(sim, f"{box} {method} disorder, strained box", worst)
    print(f"FDOTR-WORST {PRECISION} {box} {method} {max(worst):.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,args", [("-I", LJ5_MIXED + ["-I"]), ("-P", EAM_BOX + MISHIN[1:] + ["-P"]), ("-H", EAM_BOX + ["-H", "-m", "cta_cell"]), ("-a 1", LJ25 + ["-a", 1])])
def test_virial_fdotr_with_tables_splines_hilbert_and_overlap(gpu, name, args):
    worst = []
    with gpu.Simulation(args + DISORDER) as sim:
        _compare(sim, f"{name} disorder", worst)
        sim.step(5)
        sim.set_box(sim.box * SCALE)
        _compare(sim, f"{name} 5 steps, strained box", worst)
    print(f"FDOTR-WORST {PRECISION} {name} {max(worst):.3e}")


# ---------------------------------------------------------------- GPU: the barostat against a replay with virial(), berendsen_scale and deform()
EVERY, TAU, MODULUS = 5, 1000.0, 140.0
COLD = ["-T", 0]


def _p_axes(sim):
    w, k = sim.virial()
    return np.diag(k + w) / sim.volume * GPA


def _replay(gpu, args, prepare, couplings, axes="xyz", iso=False, tau=TAU):
    """the barostat in Python from the pieces that were there before: virial() -> berendsen_scale -> deform(mu); the atoms sit on lattice sites, so steps change nothing"""
    boxes, ps = [], []
    with gpu.Simulation(args) as sim:
        prepare(sim)
        for _ in range(couplings):
            p = _p_axes(sim)
            ps.append(p)
            sim.deform(gpu.berendsen_scale(p, 0.0, EVERY * 1.0, tau, MODULUS, axes=axes, iso=iso))
            boxes.append(sim.box)
    return np.array(boxes), np.array(ps)


def _integrated(gpu, args, prepare, couplings, axes="xyz", iso=False, tau=TAU):
    boxes = []
    with gpu.Simulation(args) as sim:
        prepare(sim)
        sim.set_barostat(0.0, tau_fs=tau, modulus_gpa=MODULUS, every=EVERY, axes=axes, iso=iso)
        assert sim.barostat["on"] and sim.barostat["axes"] == axes and sim.barostat["every"] == EVERY
        sim.step(1)                                                                              # the box a coupling asks for is set by the step after it
        for _ in range(couplings):
            sim.step(EVERY)
            boxes.append(sim.box)
        assert sim.step_count == 1 + couplings * EVERY
    return np.array(boxes)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [EAM_BOX + COLD + ["-m", "cta_cell"], LJ25 + COLD])
def test_barostat_follows_the_replay_on_a_cold_lattice(gpu, args):
    squeeze = lambda sim: sim.deform(0.99)
    want, ps = _replay(gpu, args, squeeze, 8)
    got = _integrated(gpu, args, squeeze, 8)
    print("replay p (GPa):", np.abs(ps).max(axis=1), " box rel:", np.abs(got / want - 1.0).max())
    assert np.abs(ps[0]).max() > 1.0                                                             # several GPa to relax
    assert np.all(np.diff(np.abs(ps), axis=0) < 0.0), ps                                         # |p| falls at every coupling
    assert np.abs(got / want - 1.0).max() <= BOX_TOL
    assert np.all(np.diff(got, axis=0) > 0.0)                                                    # compressed: the box grows back


@pytest.mark.gpu
def test_barostat_on_two_axes_leaves_the_third_alone(gpu):
    args = EAM_BOX + COLD + ["-m", "cta_cell"]
    stretch = lambda sim: sim.set_box(sim.box * np.array([1.01, 1.0, 1.0]))
    want, _ = _replay(gpu, args, stretch, 8, axes="yz")
    got = _integrated(gpu, args, stretch, 8, axes="yz")
    assert np.all(got[:, 0] == want[0, 0]) and np.all(want[:, 0] == want[0, 0])                  # L_x keeps its bits
    assert np.abs(got[:, 1:] / want[:, 1:] - 1.0).max() <= BOX_TOL
    assert np.all(np.diff(got[:, 1:], axis=0) != 0.0)


@pytest.mark.gpu
def test_iso_barostat_scales_all_axes_alike(gpu):
    args = EAM_BOX + COLD + ["-m", "cta_cell"]
    stretch = lambda sim: sim.set_box(sim.box * np.array([1.01, 0.995, 1.0]))
    got = _integrated(gpu, args, stretch, 4, iso=True)
    want, _ = _replay(gpu, args, stretch, 4, iso=True)
    mu = got[1:] / got[:-1]
    assert np.abs(mu - mu[:, :1]).max() <= 4 * EPS_REAL and np.all(mu != 1.0), mu
    assert np.abs(got / want - 1.0).max() <= BOX_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("args", [EAM_BOX + ["-T", 300, "--langevin", "-m", "cta_cell"], LJ25 + ["-T", 300, "--langevin", "-m", "thread_atom_nl"]])
def test_split_calls_give_the_bits_of_one(gpu, args):
    """step(4); step(6) against step(10) with a coupling every 5 steps: couplings are counted by the global step, and a coupling step ends the way the last step of a call
    does, so box, positions and momenta agree to the bit."""
    with gpu.Simulation(args) as a, gpu.Simulation(args) as b:
        box0 = a.box
        for s in (a, b):
            s.deform(0.995)
            s.set_barostat(0.0, tau_fs=100.0, every=5)
        a.step(10)
        a.step(1)
        b.step(4)
        b.step(6)
        b.step(1)
        assert not np.array_equal(a.box, box0 * 0.995)
        assert np.array_equal(a.box, b.box)
        assert np.array_equal(a.gather(0), b.gather(0)) and np.array_equal(a.gather(1), b.gather(1))
        assert a.step_count == b.step_count == 11


@pytest.mark.gpu
def test_barostat_switched_off_is_plain_nve(gpu):
    """After set_barostat(on=False) the steps are those of a simulation that never had one: a fresh simulation given the same box, positions and momenta takes them to the
    same bits, and the coupling that was still waiting for its remap is dropped."""
    args = EAM_BOX + ["-T", 300, "-m", "cta_cell"]
    with gpu.Simulation(args) as a, gpu.Simulation(args) as b:
        a.deform(0.995)
        a.set_barostat(0.0, tau_fs=100.0, every=5)
        a.step(10)                                                                               # ends on a coupling: its box is pending
        a.set_barostat(on=False)
        assert a.barostat["on"] is False
        box = a.box
        b.set_box(box)
        b.scatter(0, a.gather(0))
        b.scatter(1, a.gather(1))
        b.redistribute()
        b.compute_force()
        a.step(7)
        b.step(7)
        assert np.array_equal(a.box, box) and np.array_equal(b.box, box)
        assert np.array_equal(a.gather(0), b.gather(0)) and np.array_equal(a.gather(1), b.gather(1))


@pytest.mark.gpu
def test_barostat_beside_a_strain_rate(gpu):
    """set_strain_rate((0.5, 0, 0)) with the barostat on y and z: L_x is the strain-rate expression of tests/test_deform.py, a pure function of the step count, and the
    lateral axes move; the barostat refuses the strained axis and the rate a coupled one, either with nothing changed."""
    with gpu.Simulation(EAM_BOX + ["-T", 300, "-m", "cta_cell"]) as sim:
        box0 = sim.box
        sim.set_strain_rate((0.5, 0.0, 0.0))
        with pytest.raises(ValueError):
            sim.set_barostat(0.0, every=5, axes="xy")
        assert sim.barostat["on"] is False
        sim.set_barostat(0.0, tau_fs=100.0, every=5, axes="yz")
        with pytest.raises(ValueError):
            sim.set_strain_rate((0.5, 0.1, 0.0))                                                 # and the rate refuses a coupled axis
        sim.step(10)
        sim.step(11)
        assert sim.box[0] == REAL(box0[0] * (1 + 0.5 * 21 / 1000)), (sim.box, box0)          # the host forms the extent in double and stores it as real_t
        assert sim.box[1] != box0[1] and sim.box[2] != box0[2]
        for bad in (dict(every=0), dict(axes=""), dict(tau_fs=0.0), dict(modulus_gpa=0.0), dict(every=200, tau_fs=100.0), dict(pressure_gpa=float("nan"))):
            was = sim.barostat
            with pytest.raises(ValueError):
                sim.set_barostat(**dict(dict(axes="yz"), **bad))
            now = sim.barostat
            assert all(np.array_equal(was[k], now[k]) for k in was), (bad, was, now)


def _compressed(gpu, args, method):
    with gpu.Simulation(args + ["-m", method]) as sim:
        n, box0 = sim.n_global, sim.box
        sim.deform(1.02)
        sim.set_barostat(0.0, tau_fs=25.0, every=5)
        sim.step(41)
        sim.sum_atoms()
        assert sim.n_global == n                                                                 # no lost atom
        return {"f": sim.gather(2), "e": sim.energy(), "box": sim.box, "box0": box0, "builds": sim.nl_builds}


@pytest.mark.gpu
@pytest.mark.parametrize("args", [LJ25 + ["-r", 0.1, "-T", 600], EAM_BOX + ["-r", 0.1, "-T", 600]])
def test_lists_stay_valid_under_the_barostat(gpu, args):
    """thread_atom_nl from a box stretched by 2 % with the target at 0: the barostat compresses it, the list rule looks a step ahead, and the final energy and forces
    are those of cta_cell driven the same way, to the tolerances tests/test_deform.py uses for the list methods."""
    ref, run = _compressed(gpu, args, "cta_cell"), _compressed(gpu, args, "thread_atom_nl")
    df, dE = np.abs(run["f"] - ref["f"]).max() / np.abs(ref["f"]).max(), abs(run["e"][0] - ref["e"][0]) / run["e"][2]
    print(f"builds {run['builds']}  box {run['box']}  max|df|/max|f| {df:.2e}  |dE|/N {dE:.2e}  |dL|/L {np.abs(run['box'] / ref['box'] - 1).max():.2e}")
    assert np.all(run["box"] < run["box0"] * 1.02) and run["builds"] >= 1
    assert df <= TOL["force_rel_to_max"] and dE <= TOL["energy_per_atom_step0"], (df, dE)


@pytest.mark.gpu
def test_npt_moves_towards_the_target(gpu):
    """EAM 10^3 under --langevin at 300 K, target 0: the lattice at 0 K spacing is compressed by the thermal pressure, so the box must grow, and the pressure over the
    last 10 couplings is below half of where it began.  A direction test, not a convergence claim."""
    with gpu.Simulation(["-e", "-x", 10, "-y", 10, "-z", 10, "-T", 300, "--langevin", "-m", "cta_cell"]) as sim:
        v0, p0 = sim.volume, sim.pressure() * GPA
        sim.set_barostat(0.0, tau_fs=50.0, every=10)
        ps = []
        for _ in range(40):
            sim.step(10)
            ps.append(sim.pressure() * GPA)
        print(f"p0 {p0:.4f} GPa  mean of the last 10 {np.mean(ps[-10:]):.4f} GPa  V/V0 {sim.volume / v0:.6f}")
        assert sim.volume / v0 > 1.0
        assert abs(np.mean(ps[-10:])) < 0.5 * abs(p0)


# ---------------------------------------------------------------- GPU: the executable
def _comd_hip(tmp_path, extra):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip-sp" if SINGLE else "comd-hip"), "-e", "-x", "10", "-y", "8", "-z", "6", "-T", "300", "-N", "40", "-n", "10",
                           "-d", os.path.join(ROOT, "pots")] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    text = "".join((tmp_path / y).read_text() for y in yaml)
    for y in yaml:
        os.remove(tmp_path / y)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    return proc, text


@pytest.mark.gpu
def test_comd_hip_writes_the_barostat_file(gpu, tmp_path):
    run, yaml = _comd_hip(tmp_path, ["--baro", "--baroAxes", "yz", "--erateX", "0.5", "--baroTau", "100"])
    head = [l for l in run.stdout.splitlines() if "Performance" not in l and "Loop" in l and "Time(fs)" in l]
    assert len(head) == 1 and "Pressure(GPa)" in head[0] and head[0].count("V/V0") == 1, head
    rows = {int(l.split()[0]): l.split() for l in run.stdout.splitlines() if re.match(r"^\s+\d+\s+\d+\.\d\d\s", l)}
    assert sorted(rows) == [0, 10, 20, 30, 40]
    lines = (tmp_path / "baro.dat").read_text().splitlines()
    assert lines[0].startswith("#") and " N 1920 " in lines[0] and "axes yz" in lines[0] and "tau(fs) 100" in lines[0] and "every 10" in lines[0]
    data = np.array([[float(v) for v in l.split()] for l in lines[1:]])
    assert data.shape == (4, 12) and np.array_equal(data[:, 0], [10, 20, 30, 40]) and np.array_equal(data[:, 1], [10, 20, 30, 40])
    assert np.all(data[:, 5] == 1.0) and np.all(data[:, 6:8] != 1.0)                             # mu_x = 1: x is strained, not coupled
    assert np.all(np.abs(data[:, 11] / (data[:, 8] * data[:, 9] * data[:, 10]) - 1.0) <= 1e-12)
    n, v = 1920, data[:, 11]
    for k, step in enumerate((10, 20, 30, 40)):
        # the table's pressure is the pair walk's on the same state (the remap the coupling asked for comes with the next step)
        tol = W_TOL / v[k] * GPA + 1e-9                                                          # + the table's ten decimals
        print(f"step {step}: file p {data[k, 2:5].mean():.10f} GPa  table {rows[step][8]} GPa  tol {tol:.2e}")
        assert abs(data[k, 2:5].mean() - float(rows[step][8])) <= tol, (step, data[k, 2:5], rows[step][8])
    block = re.search(r"^Barostat:\n((?:  .*\n)+)", yaml, flags=re.M)
    assert block, yaml[-2000:]
    for key in ("target", "tau", "modulus", "every", "axes", "iso", "startStep", "couplings", "finalBox", "meanPressureLastHalf", "file"):
        assert re.search(rf"^  {key}: ", block.group(1), flags=re.M), key
    assert re.search(r"^  couplings: 4$", block.group(1), flags=re.M) and re.search(r"^  file: baro.dat$", block.group(1), flags=re.M)
    assert re.search(r"^\s*barostat\s+4\s", run.stdout, flags=re.M)
    assert re.search(r"^Deform:\n", yaml, flags=re.M) and (tmp_path / "deform.dat").exists()
    assert n == 1920
