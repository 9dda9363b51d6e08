"""Heat flux and Green-Kubo thermal conductivity (computeHeatFlux, comdHeatFlux / comdAtomHeatFlux / comdHeatFluxAcf, Simulation.heat_flux /
atomic_heat_flux / heat_flux_density, heat_flux_acf, comd-hip --heatflux).

CoMD computes no heat flux, so nothing here is compared with a recorded number.  The checks are restatement and physics, on the states of
tests/test_atom_stress.py (together they cover every chunk class of evenly filled cells of hip/stencil_walk.h; the classes with empty stencil cells, atoms
without a neighbour and chunks of 1 to 3 atoms are the heat-flux leg of tests/test_analysis_regimes.py, the 2-cell and straining boxes tests/test_per_atom_fields_edges.py):
  * every atom's virial part jv_i = 1/2 sum_j r_ij (f_ij . v_i) against -s_i v_i, with s_i the all-pairs minimum-image tensor of test_atom_stress._restate
    and, for the -P splines, the tensor of Simulation.atomic_stress(kinetic=False);
  * the convective parts against gather(3), gather(1) and the mass, formed in extended precision;
  * the device reduction against the column sums of the per-atom array;
  * a rigid translation: with v_i = u for every atom, J V = (E_pot + N m |u|^2 / 2) u + W u;
  * every method, layout, stream mode, rank count and both precisions give the same array; comd-hip writes what Python computes.

Bounds (no atom and no component is left out of a comparison).  With A_i,ab = 1/2 sum_j |r_ij,a f_ij,b| of the restatement and
B_i,a = sum_b A_i,ab |v_i,b|, which bounds the sum of the magnitudes of the terms of jv_i,a however they are grouped:
  virial part       double |got - want| <= 1e-11 B_i,a                  single <= (n_i + 64) 2^-24 B_i,a        (n_i neighbours)
  convective parts  |got - want| <= 8 eps (|e_i| + ke_i) |v_i,a|        eps = 2^-53 or 2^-24: the kernel rounds v = p / m once, ke = 1/2 p . v
                                                                        three times more, and the product once: at most 6 eps, the reference none
  totals            |got - sum of the rows| <= (k + 2) eps sum_i |row_i| (test_reduction_is_the_sum_of_the_rows derives k)
"""
import json
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import device_isa
import test_atom_stress as tas
from test_atom_stress import EPS24, EPS53, LAT, SIGMA, STATES, _assert_close, _child, _pair_function, _restate
from test_pressure import EAM_METHODS, LJ_METHODS

ROOT, HERE, CSRC = tas.ROOT, tas.HERE, tas.CSRC
KB_EV = 8.6173324e-5
W_PER_MK = 1.602176634e6                       # 1 eV/(fs A K) in W/(m K)
IDX = np.array([[0, 5, 4], [5, 1, 3], [4, 3, 2]])      # (a, b) -> its place among xx yy zz yz xz xy


def _times_v(six, v):
    """[n, 3]: sum_b t_ab v_b of the symmetric tensors six[n, 6]"""
    return np.stack([(six[:, IDX[a]] * v).sum(1) for a in range(3)], axis=1)


def _convective(e, p, mass):
    """jk, jp [n, 3] and their magnitude (|e_i| + ke_i) |v_i,a| in extended precision (64-bit mantissa where the platform has it): the reference adds no
    rounding of its own to the 8 eps the kernel is allowed"""
    ld = np.longdouble
    pl, el, ml = p.astype(ld), e.astype(ld), ld(mass)
    v = pl / ml
    ke = (pl * pl).sum(1) / (2 * ml)
    return ((ke[:, None] * v).astype(np.float64), (el[:, None] * v).astype(np.float64),
            ((np.abs(el) + ke)[:, None] * np.abs(v)).astype(np.float64))


_CACHE = {}


def _hf(gpu, name, steps=0, extra=()):
    """One simulation per (state, steps, extra flags), shared by the tests: the measurements of test_atom_stress._measure (its restatement included; taken from
    that module's cache, and left there, when the state is the same to the bit) and the heat-flux arrays of the same device state."""
    key = (name, steps, tuple(extra))
    if key in _CACHE:
        return _CACHE[key]
    st = STATES[name]
    with gpu.Simulation(st["flags"] + list(extra)) as sim:
        if steps:
            sim.step(steps)
        out = dict(pos=sim.gather(0).copy(), mom=sim.gather(1).copy(), e=sim.gather(3).copy(), mass=sim.mass, volume=sim.volume, n=sim.n_global,
                   energy=sim.energy(), s0=sim.atomic_stress(kinetic=False), cells=(sim.n_local_boxes, sim.max_atoms))
        out["atoms"], out["sums"] = sim.atomic_heat_flux(), sim.heat_flux()
        out["again"] = (sim.atomic_heat_flux(), sim.heat_flux())
        out["density"] = sim.heat_flux_density()
        if not extra:
            base = tas._CACHE.get((name, steps))
            if base is None or not (np.array_equal(base["pos"], out["pos"]) and np.array_equal(base["mom"], out["mom"]) and np.array_equal(base["s0"], out["s0"])):
                base = tas._measure(sim, st)
                tas._CACHE.setdefault((name, steps), base)
            out["base"] = base
    _CACHE[key] = out
    return out


# ---------------------------------------------------------------- CPU: flags, exports, ACF, ISA
def test_heatflux_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--heatflux', '--hfStart', 10, '--hfWindow', 5, '--hfFile', 'j.dat', '--hfAcfFile', 'c.dat'], "
                  "host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("heatflux", "hfStart", "hfWindow", "hfFile", "hfAcfFile"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])
    for bad in (["--hfStart", -1], ["--hfStart", 101], ["--hfWindow", -1]):
        proc = _child(f"pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--heatflux'] + {bad!r}, host_only=True); print('made')")
        assert proc.returncode != 0 and "made" not in proc.stdout and "Error:" in proc.stdout and bad[0][2:] in proc.stdout, proc.stdout[-2000:]


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_entry_points_are_exported_and_declared(sfx):
    def defined(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"{lib}{sfx}.so")], capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "computeHeatFlux" in defined("libcomd_hip")
    assert {"comdHeatFlux", "comdAtomHeatFlux", "comdHeatFluxAcf"} <= defined("libcomd_host")
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeHeatFlux\(SimGpu\* sim, real_t\* outBySlot9, double\* out9\);", header, flags=re.M)
    assert "Not in the reference" in header[:header.index("void computeHeatFlux(")].rsplit("/*", 1)[1]
    header = open(os.path.join(CSRC, "host", "comd_host.h")).read()
    assert re.search(r"^int comdHeatFlux\(SimFlat\* s, double out9\[9\]\);", header, flags=re.M)
    assert re.search(r"^int comdAtomHeatFlux\(SimFlat\* s, double\* byGid\);", header, flags=re.M)
    assert re.search(r"^int comdHeatFluxAcf\(const double\* j, int samples, int window, double\* acf\);", header, flags=re.M)


def test_host_only_simulation_refuses(pkg):
    import ctypes
    sim = pkg.Simulation(["-x", 8, "-y", 8, "-z", 8], host_only=True)
    for call in (sim.heat_flux, sim.atomic_heat_flux, sim.heat_flux_density):
        with pytest.raises(RuntimeError):
            call()
    out = np.zeros((max(sim.n_global, 2048), 9))
    assert sim.lib.comdHeatFlux(sim.ptr, (ctypes.c_double * 9)()) == -1
    assert sim.lib.comdAtomHeatFlux(sim.ptr, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert sim.mass > 0.0
    sim.close()


def test_acf_is_the_direct_sum(pkg):
    """heat_flux_acf on a seeded series of 200 x 3, window 50, against numpy's direct sums: 200 2^-53 sum |terms| per lag and component.  Window 1 is the
    mean square; window = samples is accepted, a larger one and an empty one are not."""
    j = np.random.default_rng(20261020).normal(size=(200, 3)) * np.array([1.0, 30.0, 1e-3])
    got = pkg.heat_flux_acf(j, 50)
    assert got.shape == (50, 3) and got.dtype == np.float64
    for k in range(50):
        terms = j[:200 - k] * j[k:]
        want, bound = terms.sum(0) / (200 - k), 200 * EPS53 * np.abs(terms).sum(0) / (200 - k)
        assert np.all(np.abs(got[k] - want) <= bound), (k, got[k], want, bound)
    one = pkg.heat_flux_acf(j, 1)
    assert one.shape == (1, 3) and np.all(np.abs(one[0] - (j * j).mean(0)) <= 200 * EPS53 * (j * j).mean(0))
    full = pkg.heat_flux_acf(j, 200)
    assert full.shape == (200, 3) and np.array_equal(full[:50], got) and np.array_equal(full[199], j[0] * j[199])
    for window in (0, 201, -3):
        with pytest.raises(ValueError):
            pkg.heat_flux_acf(j, window)
    with pytest.raises(ValueError):
        pkg.heat_flux_acf(j[:, :2], 10)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_heat_flux_kernels_use_no_scratch(precision):
    """Every pair function has its two instances (planes, rows), HeatFlux_Final exists and none spills to scratch; the instances that store planes use no LDS
    (the rows go through blockSumD alone)."""
    blocks = device_isa.blocks(precision, r"HeatFlux_\w+")
    names = sorted(blocks)
    assert len(names) == 9, names
    for pair in ("VirialLj", "VirialLjTable", "VirialEamILb0E", "VirialEamILb1E"):
        for store in ("Lb0E", "Lb1E"):
            assert any(re.search(rf"HeatFlux_thread_atomI\d*{pair}\w*?{store}Ev", n) for n in names), (pair, store, names)
    assert any("HeatFlux_Final" in n for n in names)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)\n", block).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)\n", block).group(1))
        print(precision, name, vgprs, "VGPRs", lds, "bytes of LDS")
        assert lds == (0 if "Lb1EEv" in name and "thread_atom" in name else 4 * 9 * 8), (name, lds)
        assert vgprs <= 128, (name, vgprs)                   # four waves per SIMD at the least, as the virial kernels


# ---------------------------------------------------------------- GPU: the virial part
def _virial_bounds(m, base):
    v = m["mom"] / m["mass"]
    return -_times_v(base["want"], v), _times_v(base["A"], np.abs(v)), v


@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", [("A", 0), ("B", 0), ("BI", 0), ("C", 0), ("D", 0), ("E", 0), ("F", 0), ("A", 10), ("E", 10)])
def test_virial_part_matches_the_restatement(gpu, name, steps):
    """atomic_heat_flux()[:, 6:9] of every atom against -s_i v_i with s_i the all-pairs tensor, 1e-11 B_i,a; after 10 steps atoms have changed cells."""
    m = _hf(gpu, name, steps)
    tas._assert_state_is_what_it_claims(name, _hf(gpu, name, 0)["base"])
    want, bound, v = _virial_bounds(m, m["base"])
    assert m["atoms"].shape == (STATES[name]["atoms"], 9) and m["atoms"].dtype == np.float64
    assert m["base"]["cnt"].min() > 0 and np.all(bound > 0.0) and np.abs(v).min() > 0.0
    _assert_close(m["atoms"][:, 6:9], want, 1e-11 * bound, f"{name} step {steps}")
    assert np.array_equal(m["again"][0], m["atoms"])            # bit-reproducible run to run
    assert all(np.array_equal(m["again"][1][k], m["sums"][k]) for k in m["sums"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D", "F"])
def test_virial_part_matches_the_stress_api_with_splines(gpu, name):
    """-P: the restatement has no spline, so the columns are held against -atomic_stress(kinetic=False) v of the same simulation.  The positions are those of
    the state without -P, so B_i,a is its (the splines and the quadratic tables are fits of the same functions)."""
    m, p = _hf(gpu, name), _hf(gpu, name, extra=("-P",))
    assert np.array_equal(p["pos"], m["pos"]) and np.array_equal(p["mom"], m["mom"])
    assert np.abs(p["s0"] - m["s0"]).max() > 0.0                # another pair function ran
    _, bound, v = _virial_bounds(m, m["base"])
    _assert_close(p["atoms"][:, 6:9], -_times_v(p["s0"], v), 1e-11 * bound, f"{name} -P")
    _assert_close(m["atoms"][:, 6:9], -_times_v(m["s0"], v), 1e-11 * bound, f"{name}")


# ---------------------------------------------------------------- GPU: the convective parts, the reduction
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "D"])
def test_convective_parts(gpu, name):
    """columns 0-2 = (|p|^2 / 2m) p / m and 3-5 = e p / m with e of gather(3), p of gather(1): 8 x 2^-53 (|e_i| + ke_i) |v_i,a|."""
    m = _hf(gpu, name)
    jk, jp, mag = _convective(m["e"], m["mom"], m["mass"])
    assert np.abs(m["e"]).min() > 0.0 and np.abs(jk).max() > 0.0
    _assert_close(m["atoms"][:, 0:3], jk, 8.0 * EPS53 * mag, f"{name} kinetic")
    _assert_close(m["atoms"][:, 3:6], jp, 8.0 * EPS53 * mag, f"{name} potential")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "E"])
def test_reduction_is_the_sum_of_the_rows(gpu, name):
    """heat_flux() against the column sums of atomic_heat_flux(), (k + 2) 2^-53 sum_i |row_i| per sum.  k: a lane of the sampled path adds in real_t one atom per
    chunk its wave walks; the HEATFLUX_BLOCKS = 2048 workgroups share the nLocalBoxes * ceil(cap / 64) chunks evenly and the 4 waves of a workgroup deal its
    chunks round-robin, so k = ceil(ceil(nLocalBoxes * ceil(cap / 64) / 2048) / 4) -- 1 for both states, whose 27 and 125 cells have fewer chunks than there
    are workgroups.  The + 2 is the double sum of the rows on the device and numpy's."""
    m = _hf(gpu, name)
    cells, cap = m["cells"]
    k = math.ceil(math.ceil(cells * math.ceil(cap / 64) / 2048) / 4)
    assert k == 1
    mag = np.abs(m["atoms"]).sum(0)
    for part, cols in (("kinetic", slice(0, 3)), ("potential", slice(3, 6)), ("virial", slice(6, 9))):
        _assert_close(m["sums"][part], m["atoms"][:, cols].sum(0), (k + 2) * EPS53 * mag[cols], f"{name} {part}")
    total = m["atoms"][:, 0:3].sum(0) + m["atoms"][:, 3:6].sum(0) + m["atoms"][:, 6:9].sum(0)
    _assert_close(m["sums"]["total"], total, (k + 3) * EPS53 * (mag[0:3] + mag[3:6] + mag[6:9]), f"{name} total")
    assert np.array_equal(m["sums"]["total"], (m["sums"]["kinetic"] + m["sums"]["potential"]) + m["sums"]["virial"])
    assert np.array_equal(m["density"], m["sums"]["total"] / m["volume"])


# ---------------------------------------------------------------- GPU: physics
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "D"])
def test_rigid_translation(gpu, name):
    """Every atom moving with u: J V = (E_pot + N m |u|^2 / 2) u + W u, E_pot of energy() and W of virial(), neither of which the restatement enters;
    1e-10 (sum_i (|e_i| + ke_i) |u_a| + sum_i B_i,a).  With all momenta 0 every sum and every per-atom component is exactly 0."""
    m = _hf(gpu, name)
    u = np.array([0.003, -0.002, 0.001])
    with gpu.Simulation(STATES[name]["flags"]) as sim:
        n, mass = sim.n_global, sim.mass
        sim.scatter(1, np.broadcast_to(mass * u, (n, 3)))
        assert np.array_equal(sim.gather(0), m["pos"]) and np.array_equal(sim.gather(3), m["e"])
        got, (w, _) = sim.heat_flux(), sim.virial()
        e_pot = sim.energy()[0]
        sim.scatter(1, np.zeros((n, 3)))
        zero, zero_atoms = sim.heat_flux(), sim.atomic_heat_flux()
    ke = 0.5 * mass * (u * u).sum()
    want = (e_pot + n * ke) * u + w @ u
    bound = 1e-10 * ((np.abs(m["e"]) + ke).sum() * np.abs(u) + _times_v(m["base"]["A"], np.broadcast_to(np.abs(u), (n, 3))).sum(0))
    assert np.abs(w @ u).min() > 1e3 * bound.max()              # the virial part is there to be seen
    _assert_close(got["total"], want, bound, f"{name} rigid")
    _assert_close(got["kinetic"] + got["potential"], (e_pot + n * ke) * u, bound, f"{name} rigid convective")
    for part in ("kinetic", "potential", "virial", "total"):
        assert np.all(zero[part] == 0.0), (part, zero[part])
    assert np.all(zero_atoms == 0.0)


# ---------------------------------------------------------------- GPU: methods, layouts, ranks, single precision
CHILD_RUN = """
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    assert pkg.PRECISION == {precision!r}
    sim = pkg.Simulation({args!r})
    eam = {eam}
    one = np.zeros(1)
    sums = sim.heat_flux()
    np.savez({out!r}, j=sim.atomic_heat_flux(), sums=np.concatenate([sums[k] for k in ("kinetic", "potential", "virial", "total")]), pos=sim.gather(0),
             mom=sim.gather(1), e=sim.gather(3), mass=sim.mass, df=sim.gather(5) if eam else one,
             phi=np.array(sim.eam_table(0)[2]) if eam else one, rho=np.array(sim.eam_table(1)[2]) if eam else one,
             phi_x=np.array(sim.eam_table(0)[:2]) if eam else one, rho_x=np.array(sim.eam_table(1)[:2]) if eam else one)
    sim.close()
"""


def _flux_in_child(args, out, env=None, eam=False, precision="double"):
    proc = _child(CHILD_RUN.format(args=list(args), out=str(out), eam=eam, precision=precision), env=env)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "D"])
def test_methods_and_layouts_agree(gpu, tmp_path, name):
    """The method lists of tests/test_pressure.py on the 2-cell LJ box and the setfl state: every method, cell numbering, stream mode, list format and halo form
    gives thread_atom's per-atom array within 1e-12 of the largest magnitude of the part: max B for the virial columns (the criterion of
    test_atom_stress.test_methods_and_layouts_agree, there 1e-12 max A), max (|e_i| + ke_i) |v_i,a| for the convective ones (the methods sum e_i in their own
    orders)."""
    st, m = STATES[name], _hf(gpu, name)
    lj = st["pair"] != "eam"
    got = {}
    for method, extra in LJ_METHODS if lj else EAM_METHODS:
        with gpu.Simulation(st["flags"] + ["-m", method] + extra) as sim:
            got[" ".join([method] + [str(x) for x in extra])] = sim.atomic_heat_flux()
    for env in [{"COMD_NL_GLOBAL": "1"}] if lj else [{"COMD_EAM_GROUPS": "0"}, {"COMD_HALO_MIRROR": "0"}]:
        method = "thread_atom_nl" if "COMD_NL_GLOBAL" in env else "cta_cell"
        got[f"{method} {env}"] = _flux_in_child(st["flags"] + ["-m", method], tmp_path / f"{len(got)}.npz", env=env)["j"]
    assert np.array_equal(got["thread_atom"], m["atoms"])       # bit-reproducible run to run
    _, b, _ = _virial_bounds(m, m["base"])
    conv = _convective(m["e"], m["mom"], m["mass"])[2].max()
    scale = np.array([conv] * 6 + [b.max()] * 3)
    for key, j in got.items():
        err = np.abs(j - got["thread_atom"]).max(0)
        print(key, (err / scale).max())
        assert np.all(err <= 1e-12 * scale), (key, err / scale)


def _new_momenta(n, mass):
    """the momenta the rank test scatters: seeded, the same on every rank, about 0.003 A/fs"""
    return np.random.default_rng(77).normal(size=(n, 3)) * (0.003 * mass)


def _ranks(grid, args, out_dir, timeout=900):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    assert world <= 8
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "heatflux_worker.py"), str(r), str(world), port, *map(str, grid), str(out_dir), json.dumps(args)],
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
    return [np.load(os.path.join(out_dir, f"heatflux_rank{r}.npz")) for r in range(world)]


_ONE_RANK = {}


def _one_rank(gpu, pot, n):
    """the one-rank arrays of the rank test's state after the scatter of new momenta, checked against the stress API, and the scales of the comparison"""
    if (pot, n) not in _ONE_RANK:
        args = ["-x", n, "-y", n, "-z", n, "-r", 0.1] + (["-e"] if pot == "eam" else [])
        with gpu.Simulation(args) as sim:
            old = sim.gather(1).copy()
            p = _new_momenta(sim.n_global, sim.mass)
            sim.scatter(1, p)
            j, sums, s0, e, mass = sim.atomic_heat_flux(), sim.heat_flux(), sim.atomic_stress(kinetic=False), sim.gather(3).copy(), sim.mass
            fr_of = _pair_function("eam", sim.eam_table(0), sim.eam_table(1), sim.gather(5).copy()) if pot == "eam" else _pair_function("lj")
            _, big_a, _ = _restate(sim.gather(0), sim.box, 4.95 if pot == "eam" else 5.0 * SIGMA, fr_of, rows=np.arange(256))
        v = p / mass
        b = _times_v(big_a, np.abs(v[:256]))
        # the one-rank array itself: its halo slots are periodic images that still hold the OLD momenta
        assert np.abs(p - old).min() > 0.0
        assert np.all(np.abs(j[:256, 6:9] + _times_v(s0, v)[:256]) <= 1e-11 * b)
        assert np.abs(j[:, 6:9] + _times_v(s0, v)).max() <= 1e-11 * b.max()
        _ONE_RANK[(pot, n)] = (args, j, sums, float(b.max()), float(_convective(e, p, mass)[2].max()))
    return _ONE_RANK[(pot, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot,n", [("lj", 14), ("eam", 8)])
def test_ranks_give_the_one_rank_array(gpu, tmp_path, grid, pot, n):
    """2 and 8 ranks sharing the device (gloo transport): every rank returns the global array, the one-rank one within 1e-12 of the largest magnitude of the
    part, and the sums over the ranks.

    This is the test of the one-sided form, and it cannot pass by reading halo momenta: every process first scatters NEW momenta (seeded, the same by gid on
    every rank).  scatter() writes the local slots only and no halo exchange follows, so every halo slot -- another rank's atom, or on one rank a periodic
    image -- still holds the momentum of the initial state.  A kernel that read p_j of a halo slot (the symmetric form 1/2 r_ij f_ij . (v_i + v_j)) would mix
    old and new velocities, differently on every decomposition, and the one-rank array is itself held against -atomic_stress(kinetic=False) v_new."""
    args, j0, sums0, b_max, conv_max = _one_rank(gpu, pot, n)
    scale = np.array([conv_max] * 6 + [b_max] * 3)
    mag = np.abs(j0).sum(0)
    for d in _ranks(grid, args, tmp_path):
        assert d["j"].shape == j0.shape
        err = np.abs(d["j"] - j0).max(0)
        print(grid, pot, (err / scale).max())
        assert np.all(err <= 1e-12 * scale), err / scale
        for i, part in enumerate(("kinetic", "potential", "virial")):
            assert np.all(np.abs(d["sums"][3 * i:3 * i + 3] - sums0[part]) <= 1e-12 * mag[3 * i:3 * i + 3]), part
        assert np.all(np.abs(d["sums"][9:12] - sums0["total"]) <= 1e-12 * (mag[0:3] + mag[3:6] + mag[6:9]))


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
def test_single_precision_build(gpu, tmp_path, pot):
    """The float build (COMD_PRECISION=single, lib*_sp.so) in a child, state B and the Adams 6^3 state: the virial part of every atom against the restatement
    (in double) of the child's own gathered positions, momenta, tables and F', within (n_i + 64) 2^-24 B_i,a; the convective parts within
    8 x 2^-24 (|e_i| + ke_i) |v_i,a|; the sums against the rows within (k + 2) 2^-24 sum_i |row_i|, k = 1 as in test_reduction_is_the_sum_of_the_rows."""
    n = 8 if pot == "lj" else 6
    args = ["-x", n, "-y", n, "-z", n, "-l", LAT, "-r", 0.1] + (["-e"] if pot == "eam" else [])
    d = _flux_in_child(args, tmp_path / "single.npz", env={"COMD_PRECISION": "single"}, eam=pot == "eam", precision="single")
    if pot == "eam":
        fr_of = _pair_function("eam", (d["phi_x"][0], d["phi_x"][1], d["phi"]), (d["rho_x"][0], d["rho_x"][1], d["rho"]), d["df"])
    else:
        fr_of = _pair_function("lj")
    extent = np.float64(np.float32(n * np.float32(LAT))) * np.ones(3)          # the float box of the child
    s, big_a, cnt = _restate(d["pos"], extent, 4.95 if pot == "eam" else 5.0 * SIGMA, fr_of)
    mass = float(d["mass"])
    v = d["mom"] / mass
    bound = (cnt[:, None] + 64.0) * EPS24 * _times_v(big_a, np.abs(v))
    _assert_close(d["j"][:, 6:9], -_times_v(s, v), bound, f"single {pot} virial")
    jk, jp, mag = _convective(d["e"], d["mom"], mass)
    _assert_close(d["j"][:, 0:3], jk, 8.0 * EPS24 * mag, f"single {pot} kinetic")
    _assert_close(d["j"][:, 3:6], jp, 8.0 * EPS24 * mag, f"single {pot} potential")
    _assert_close(d["sums"][:9], d["j"].sum(0), 3.0 * EPS24 * np.abs(d["j"]).sum(0), f"single {pot} sums")


# ---------------------------------------------------------------- GPU: comd-hip
HEADER = tas.HEADER
POTS = {"lj": ["-x", "8", "-y", "8", "-z", "8"], "eam": ["-e", "-x", "6", "-y", "6", "-z", "6"]}


def _comd_hip(tmp_path, extra, ok=True):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-N", "40", "-n", "2", "-d", os.path.join(ROOT, "pots")] + extra,
                          capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert (proc.returncode == 0) == ok, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    text = ""
    for f in [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]:
        text += (tmp_path / f).read_text()
        os.remove(tmp_path / f)
    return proc.stdout, rows, text


def _read_files(tmp_path, flux="heatflux.dat", acf="hfacf.dat"):
    """(header, rows) of the two files; the numbers of a header by the word before them"""
    out = []
    for name in (flux, acf):
        lines = (tmp_path / name).read_text().splitlines()
        assert lines[0].startswith("# HeatFlux") and not any(line.startswith("#") for line in lines[1:])
        out.append((lines[0], np.array([[float(x) for x in line.split()] for line in lines[1:]])))
    return out


def _number(header, word):
    return float(re.search(rf"\b{word} (-?\d\S*)", header).group(1))


def _assert_acf_file(header, acf, jv, n_atoms):
    """the ACF rows against numpy's direct sums of the J V rows, and the running kappa against the trapezoid formula from the file's own C, T and V"""
    samples, window, dt = len(jv), len(acf), _number(header, "dt")
    assert _number(header, "samples") == samples and _number(header, "window") == window and _number(header, "N") == n_atoms
    assert np.array_equal(acf[:, 0], np.arange(window) * dt)
    for k in range(window):
        terms = jv[:samples - k] * jv[k:]
        assert np.all(np.abs(acf[k, 1:4] - terms.sum(0) / (samples - k)) <= samples * EPS53 * np.abs(terms).sum(0) / (samples - k)), k
    c = acf[:, 1:4].sum(1)
    integral = np.concatenate([[0.0], np.cumsum(0.5 * (c[1:] + c[:-1]) * dt)])
    kappa = integral * W_PER_MK / (3.0 * _number(header, "V") * KB_EV * _number(header, "T") ** 2)
    scale = np.concatenate([[0.0], np.cumsum(0.5 * (np.abs(c[1:]) + np.abs(c[:-1])) * dt)]) * W_PER_MK / (3.0 * _number(header, "V") * KB_EV * _number(header, "T") ** 2)
    assert np.all(np.abs(acf[:, 4] - kappa) <= 1e-12 * scale), (acf[:, 4], kappa)
    return kappa


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
def test_comd_hip_heatflux_column_files_and_yaml(gpu, tmp_path, pot):
    """comd-hip -N 40 -n 2 --heatflux on 8^3 LJ and 6^3 EAM: the column, the two files, the YAML block, and the rows of --hfFile equal to heat_flux() of a Python
    run of the same steps, to the printed 17 digits."""
    out0, rows0, yaml0 = _comd_hip(tmp_path, POTS[pot])
    assert [line for line in out0.splitlines() if line.startswith("#  Loop")] == [HEADER]
    assert "Jx(" not in out0 and not re.search(r"^heatflux\s", out0, flags=re.M) and "HeatFlux" not in yaml0
    assert not os.path.exists(tmp_path / "heatflux.dat") and not os.path.exists(tmp_path / "hfacf.dat")

    out1, rows1, yaml1 = _comd_hip(tmp_path, POTS[pot] + ["--heatflux"])
    header = [line for line in out1.splitlines() if line.startswith("#  Loop")][0]
    assert header.startswith(HEADER) and header.split()[-1] == "Jx(eV/A^2/fs)"
    assert len(rows1) == 21 and [r[:3] for r in rows1] == [r[:3] for r in rows0]          # the trajectory is untouched by the flag, to the bit
    assert re.search(r"^heatflux\s+22\s", out1, flags=re.M)                                # 21 samples and the files
    (head, flux), (head_acf, acf) = _read_files(tmp_path)
    n_atoms = int(rows1[0][2])
    assert flux.shape == (21, 11) and np.array_equal(flux[:, 0], np.arange(0, 41, 2)) and np.array_equal(flux[:, 1], flux[:, 0] * 1.0)
    assert _number(head, "N") == n_atoms and _number(head, "samples") == 21 and _number(head, "startStep") == 0 and _number(head, "dt") == 2.0
    assert np.all(np.abs(flux[:, 2:5] - (flux[:, 5:8] + flux[:, 8:11])) <= 2.0 * EPS53 * (np.abs(flux[:, 5:8]) + np.abs(flux[:, 8:11])))
    col = np.array([float(r[3].split()[-1]) for r in rows1])
    assert np.all(np.abs(col - flux[:, 2] / _number(head, "V")) <= 1e-10 * np.abs(col) + 1e-300)      # the column prints 11 digits

    with gpu.Simulation([int(x) if x.isdigit() else x for x in POTS[pot]]) as sim:
        for k in range(21):
            if k:
                sim.step(2)
            j = sim.heat_flux()
            assert np.array_equal(flux[k, 2:5], j["total"]) and np.array_equal(flux[k, 8:11], j["virial"]), (k, flux[k], j)
            assert np.array_equal(flux[k, 5:8], j["kinetic"] + j["potential"])
        assert abs(_number(head, "V") - sim.volume) <= 22 * EPS53 * sim.volume            # the mean of 21 equal volumes: 20 additions and a division

    assert acf.shape == (10, 5) and "clipped" not in head_acf            # the default window: half the samples
    kappa = _assert_acf_file(head_acf, acf, flux[:, 2:5], n_atoms)
    block = re.search(r"^HeatFlux:\n((?:  .*\n)+)", yaml1, flags=re.M).group(1)
    m = dict(re.findall(r"^  (\w+): (.+)$", block, flags=re.M))
    assert m["startStep"] == "0" and m["samples"] == "21" and m["window"] == "10" and m["file"] == "heatflux.dat" and m["acfFile"] == "hfacf.dat"
    mean = [float(x) for x in m["meanJV"].strip("[] ").split(",")]
    assert np.all(np.abs(np.array(mean) - flux[:, 2:5].mean(0)) <= 1e-11 * np.abs(flux[:, 2:5]).mean(0))
    assert abs(float(m["kappa"]) - kappa[-1]) <= 1e-11 * abs(kappa[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
def test_comd_hip_heatflux_with_the_other_flags(gpu, tmp_path, pot):
    """--heatflux beside --stress --csp, a straining box, the thermostat, the Hilbert numbering and the overlap mode, from step 10 on with a window larger than
    the samples: the column is the last one, the flag leaves the other columns and the trajectory as they are, the window is clipped and the header says so,
    V of the headers is the mean volume of the samples."""
    extra = POTS[pot] + ["--stress", "--csp", "--erateX", "0.01", "--langevin", "-H", "-a", "1"]
    out0, rows0, _ = _comd_hip(tmp_path, extra)
    out1, rows1, yaml1 = _comd_hip(tmp_path, extra + ["--heatflux", "--hfStart", "10", "--hfWindow", "100", "--hfFile", "j.dat", "--hfAcfFile", "c.dat"])
    header0, header1 = [[line for line in out.splitlines() if line.startswith("#  Loop")][0] for out in (out0, out1)]
    assert header1.split()[:-1] == header0.split() and header1.split()[-1] == "Jx(eV/A^2/fs)"
    assert len(rows1) == 21 and [r[:3] for r in rows1] == [r[:3] for r in rows0]
    for r0, r1 in zip(rows0, rows1):
        assert r1[3].split()[:-1] == r0[3].split()
        assert (float(r1[3].split()[-1]) == 0.0) == (int(r1[0]) < 10)          # no sample before --hfStart
    (head, flux), (head_acf, acf) = _read_files(tmp_path, "j.dat", "c.dat")
    assert flux.shape == (16, 11) and np.array_equal(flux[:, 0], np.arange(10, 41, 2)) and _number(head, "startStep") == 10
    assert acf.shape == (16, 5) and "clipped" in head_acf
    _assert_acf_file(head_acf, acf, flux[:, 2:5], int(rows1[0][2]))
    side = float(POTS[pot][-1]) * LAT
    volumes = side ** 3 * (1.0 + 0.01 * 1e-3 * np.arange(10, 41, 2))            # 0.01 / ps for t fs along x
    assert abs(_number(head, "V") - volumes.mean()) <= 1e-9 * volumes.mean() and _number(head_acf, "V") == _number(head, "V")
    block = re.search(r"^HeatFlux:\n((?:  .*\n)+)", yaml1, flags=re.M).group(1)
    m = dict(re.findall(r"^  (\w+): (.+)$", block, flags=re.M))
    assert m["startStep"] == "10" and m["samples"] == "16" and m["window"] == "16" and m["file"] == "j.dat" and m["acfFile"] == "c.dat" and m["kappa"] != "n/a"
    assert re.search(r"^heatflux\s+17\s", out1, flags=re.M) and "Stress:" in yaml1


@pytest.mark.gpu
def test_comd_hip_refuses_bad_values_and_reports_one_sample(gpu, tmp_path):
    for bad in (["--hfStart", "41"], ["--hfStart", "-1"], ["--hfWindow", "-1"]):
        out, rows, _ = _comd_hip(tmp_path, POTS["lj"] + ["--heatflux"] + bad, ok=False)
        assert "Error:" in out and bad[0][2:] in out and rows == [], out[-1000:]
    # one sample (the last step): a window of one lag, kappa n/a
    out, rows, yaml = _comd_hip(tmp_path, POTS["lj"] + ["--heatflux", "--hfStart", "40"])
    (head, flux), (head_acf, acf) = _read_files(tmp_path)
    assert flux.shape == (1, 11) and flux[0, 0] == 40 and acf.shape == (1, 5) and acf[0, 4] == 0.0
    assert np.all(np.abs(acf[0, 1:4] - flux[0, 2:5] ** 2) <= 2.0 * EPS53 * flux[0, 2:5] ** 2)
    assert re.search(r"^  kappa: n/a$", yaml, flags=re.M)
