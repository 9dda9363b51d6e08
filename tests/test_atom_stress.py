"""Per-atom virial stress (computeAtomStress / computeAtomStressSummary, Simulation.atomic_stress / atomic_pressure / von_mises / stress_summary,
comd-hip --stress).

CoMD computes no stress, so nothing here is compared with a recorded number.  The checks are restatement and physics:
  * every atom's six components against an all-pairs minimum-image sum in numpy (LJ analytic, LJ -I, EAM funcfl and setfl), on states chosen so that
    every chunk class of hip/stencil_walk.h occurs (full chunks, replicated chunks of 2, 4, 8 and 16 copies, partial chunks, a 2-cell periodic box);
  * the sum rule: the rows add up to -(W) or -(K + W) of Simulation.virial() (this is also the check of the -P splines);
  * the kinetic part is -p p^T / m; a perfect lattice has one tensor, -W / N, with no shear, before and after a deformation of the box;
  * every method, layout, stream mode, rank count and both precisions give the same array; the device reduction gives numpy's figures.

Tolerances.  A per-atom component can be a cancellation to 1e-6 of the magnitudes it is made of, so every per-atom comparison is relative to
A_i,ab = 1/2 sum_j |r_ij,a f_ij,b|, the sum of the magnitudes of the atom's own terms, which the restatement yields with the tensor:
  double build   |got - want| <= 1e-11 A_i,ab                     (the figure of the project's restatement tests)
  single build   |got - want| <= (n_i + 64) 2^-24 A_i,ab          (n_i neighbours: a sequential real_t sum, plus 64 roundings per term for the
                                                                   pair arithmetic and the r^-14 amplification of the rounding of r^2)
No atom and no component is left out of a comparison.
"""
import functools
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import device_isa
from test_lj_interpolation import interpolate, lj_table
from test_pressure import EAM_METHODS, LJ_METHODS, VIRIAL_WAVES, _interpolate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "comd-cuda-async_amd", "csrc")

SIGMA, EPS, LAT = 2.315, 0.167, 3.615
GPA = 160.21766208
MISHIN = ["-e", "-t", "setfl", "-p", "Cu01.eam.alloy"]
COMP = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))      # xx yy zz yz xz xy
EPS53, EPS24 = 2.0 ** -53, 2.0 ** -24

# flags, cells, atoms, cutoff, pair function of the restatement, and the chunk classes of stencil_walk.h the state is there for (asserted on the device's
# occupancies at step 0; together the states cover every class)
STATES = {
    "A": dict(flags=["-x", 12, "-y", 13, "-z", 14, "-l", 2.9, "-r", 0.1], n=(12, 13, 14), lat=2.9, atoms=8736, grid=(3, 3, 3), rc=5.0 * SIGMA, pair="lj",
              classes={"full", "reps16", "reps2", "partial"}),
    "B": dict(flags=["-x", 8, "-y", 8, "-z", 8, "-l", LAT, "-r", 0.1], n=(8, 8, 8), lat=LAT, atoms=2048, grid=(2, 2, 2), rc=5.0 * SIGMA, pair="lj",
              classes={"full"}),
    "BI": dict(flags=["-x", 8, "-y", 8, "-z", 8, "-l", LAT, "-r", 0.1, "-I"], n=(8, 8, 8), lat=LAT, atoms=2048, grid=(2, 2, 2), rc=5.0 * SIGMA,
               pair="ljtable", classes={"full"}),
    "C": dict(flags=["-x", 8, "-y", 8, "-z", 8, "-l", LAT, "-r", 0.1, "--ljCutoffSigmas", 2.5], n=(8, 8, 8), lat=LAT, atoms=2048, grid=(4, 4, 4),
              rc=2.5 * SIGMA, pair="lj", classes={"reps2"}),
    "D": dict(flags=["-x", 6, "-y", 6, "-z", 6, "-l", LAT, "-r", 0.1] + MISHIN, n=(6, 6, 6), lat=LAT, atoms=864, grid=(3, 3, 3), rc=5.50679, pair="eam",
              classes={"reps2"}),
    "E": dict(flags=["-x", 6, "-y", 6, "-z", 6, "-l", 4.4, "-r", 0.1, "-e"], n=(6, 6, 6), lat=4.4, atoms=864, grid=(5, 5, 5), rc=4.95, pair="eam",
              classes={"reps16", "reps8", "reps4"}),
    "F": dict(flags=["-x", 7, "-y", 8, "-z", 9, "-l", 2.6, "-r", 0.1, "-e"], n=(7, 8, 9), lat=2.6, atoms=2016, grid=(3, 4, 4), rc=4.95, pair="eam",
              classes={"partial"}),
}
# F: the lattice fills its cells with 32, 40 and 50 atoms, but the seeded displacement is re-binned before the first force evaluation and leaves 34 to 50
# per cell on the device, so its chunks are partial ones with one copy; the replicated EAM chunks of two copies are D's, as its test asserts.


assert set().union(*(st["classes"] for st in STATES.values())) == {"full", "partial", "reps2", "reps4", "reps8", "reps16"}


def _chunk_classes(n_atoms):
    """the classes forEachChunk (hip/stencil_walk.h) sorts the 64-slot chunks of cells of these occupancies into"""
    out = set()
    for n in set(int(v) for v in n_atoms):
        for first in range(0, n, 64):
            m = min(64, n - first)
            reps = 1
            while reps < 16 and 2 * reps * m <= 64:
                reps *= 2
            out.add("full" if m == 64 else f"reps{reps}" if reps > 1 else "partial")
    return out


def _extent(st):
    return np.array(st["n"], dtype=np.float64) * st["lat"]


def _restate(pos, extent, rc, fr_of, rows=None, block=256):
    """All pairs i != j with 0 < r^2 <= rc^2 under the minimum image, f_ij = fr_of(i, j, r) (r_i - r_j): per atom of `rows` (default all) the
    tensor s = -1/2 sum_j r_ij f_ij^T, the sum of magnitudes A = 1/2 sum_j |r_ij,a f_ij,b| (both [n, 6]) and the neighbour count.  With all atoms
    asked for, every pair is formed once, i < j, and its term -- the same from either side -- goes to both atoms."""
    half = rows is None
    rows = np.arange(len(pos)) if half else np.asarray(rows)
    n = len(rows)
    s, big_a, cnt = np.zeros((n, 6)), np.zeros((n, 6)), np.zeros(n, dtype=np.int64)
    xyz = [np.ascontiguousarray(pos[:, a]) for a in range(3)]
    for s0 in range(0, n, block):
        idx = rows[s0:s0 + block]
        j0 = s0 if half else 0                                  # i < j: the columns before the block have been paired with it already
        d = []
        for a in range(3):
            da = xyz[a][idx, None] - xyz[a][None, j0:]
            da -= np.rint(da / extent[a]) * extent[a]
            d.append(da)
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        hit = (r2 > 0.0) & (r2 <= rc * rc)
        if half:
            hit &= np.arange(j0, len(pos))[None, :] > idx[:, None]
        ii, jj = np.nonzero(hit)
        dd = [da[ii, jj] for da in d]
        fr = fr_of(idx[ii], jj + j0, np.sqrt(r2[ii, jj]))
        ii, jj = ii + s0, jj + j0
        for c, (a, b) in enumerate(COMP):
            t = 0.5 * dd[a] * dd[b] * fr
            s[:, c] -= np.bincount(ii, weights=t, minlength=n)
            big_a[:, c] += np.bincount(ii, weights=np.abs(t), minlength=n)
            if half:
                s[:, c] -= np.bincount(jj, weights=t, minlength=n)
                big_a[:, c] += np.bincount(jj, weights=np.abs(t), minlength=n)
        cnt += np.bincount(ii, minlength=n)
        if half:
            cnt += np.bincount(jj, minlength=n)
    return s, big_a, cnt


def _pair_function(kind, phi=None, rho=None, df=None):
    """f_ij / (r_i - r_j) of the force kernels: ljPair, ljTablePair, the EAM pair term with F' of both atoms"""
    if kind == "lj":
        s6 = SIGMA ** 6
        return lambda i, j, r: 24.0 * EPS * s6 * r ** -8 * (2.0 * s6 * r ** -6 - 1.0)
    if kind == "ljtable":
        table = lj_table()
        return lambda i, j, r: -interpolate(table, r)[1] / r
    return lambda i, j, r: -(_interpolate(*phi, r)[1] + (df[i] + df[j]) * _interpolate(*rho, r)[1]) / r


def _von_mises(s):
    d0, d1, d2 = s[..., 0] - s[..., 1], s[..., 1] - s[..., 2], s[..., 2] - s[..., 0]
    return np.sqrt(0.5 * (d0 * d0 + d1 * d1 + d2 * d2) + 3.0 * (s[..., 3] ** 2 + s[..., 4] ** 2 + s[..., 5] ** 2))


def _six(t):
    return np.array([t[a, b] for a, b in COMP])


def _measure(sim, st):
    """everything the tests ask of one state of one simulation, the restatement included"""
    out = dict(n_atoms=sim.cells()["nAtoms"][:sim.n_local_boxes].copy(), grid=sim.grid, n=sim.n_global, pos=sim.gather(0).copy(), mom=sim.gather(1).copy(),
               ek=sim.energy()[1], omega=sim.atomic_volume, volume=sim.volume)
    out["s0"], out["s1"] = sim.atomic_stress(kinetic=False), sim.atomic_stress(kinetic=True)
    w, k = sim.virial()
    out["w"], out["k"] = _six(w), _six(k)
    out["summary"] = sim.stress_summary()
    if st["pair"] == "eam":
        fr_of = _pair_function("eam", sim.eam_table(0), sim.eam_table(1), sim.gather(5).copy())
    else:
        fr_of = _pair_function(st["pair"])
    out["want"], out["A"], out["cnt"] = _restate(out["pos"], _extent(st), st["rc"], fr_of)
    return out


_CACHE = {}


def _state(gpu, name, steps=0):
    """the measurements of state `name` after `steps` steps: one simulation and one restatement per (state, steps), shared by the tests"""
    if (name, steps) not in _CACHE:
        st = STATES[name]
        with gpu.Simulation(st["flags"]) as sim:
            if steps:
                sim.step(steps)
            _CACHE[(name, steps)] = _measure(sim, st)
    return _CACHE[(name, steps)]


def _assert_state_is_what_it_claims(name, m):
    st = STATES[name]
    assert m["n"] == st["atoms"] and tuple(m["grid"]) == st["grid"], (name, m["n"], m["grid"])
    assert st["classes"] <= _chunk_classes(m["n_atoms"]), (name, sorted(set(m["n_atoms"].tolist())))
    assert st["rc"] < 0.5 * _extent(st).min()            # the minimum image is exact


def _assert_close(got, want, bound, what):
    err = np.abs(got - want)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(what, "max |got - want| / bound", float((err / np.maximum(bound, 1e-300)).max()), "at", worst)
    assert np.all(err <= bound), (what, worst, float(got[worst]), float(want[worst]), float(bound[worst]))


PRELUDE = f"import sys, json\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\nimport numpy as np\n"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


# ---------------------------------------------------------------- CPU: flag, exports, ISA
def test_stress_flag_is_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--stress', '--stressFile', 's.dat', '--stressDump', 's.xyz', '--stressDumpMin', 1.5], "
                  "host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("stress", "stressFile", "stressDump", "stressDumpMin"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--stress', '--stressDumpMin', -1], host_only=True); print('made')")
    assert proc.returncode != 0 and "made" not in proc.stdout and "Error:" in proc.stdout, proc.stdout[-2000:]


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_entry_points_are_exported_and_declared(sfx):
    def defined(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"{lib}{sfx}.so")], capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"computeAtomStress", "computeAtomStressSummary"} <= defined("libcomd_hip")
    assert {"comdAtomStress", "comdStressSummary"} <= defined("libcomd_host")
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeAtomStress\(SimGpu\* sim, int withKinetic, real_t\* outBySlot6\);", header, flags=re.M)
    assert re.search(r"^void computeAtomStressSummary\(SimGpu\* sim, double atomVolume, double\* out\);", header, flags=re.M)
    header = open(os.path.join(CSRC, "host", "comd_host.h")).read()
    assert re.search(r"^int comdAtomStress\(SimFlat\* s, int withKinetic, double\* stressByGid\);", header, flags=re.M)
    assert re.search(r"^int comdStressSummary\(SimFlat\* s, int withKinetic, double\* out7\);", header, flags=re.M)


def test_host_only_simulation_refuses(pkg):
    assert pkg.GPA_PER_EV_A3 == GPA
    sim = pkg.Simulation(["-x", 8, "-y", 8, "-z", 8], host_only=True)
    for call in (sim.atomic_stress, sim.atomic_pressure, sim.von_mises, sim.stress_summary):
        with pytest.raises(RuntimeError):
            call()
    # the C entries themselves return -1 without device state
    out = np.zeros((max(sim.n_global, 2048), 6))
    import ctypes
    assert sim.lib.comdAtomStress(sim.ptr, 1, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert sim.lib.comdStressSummary(sim.ptr, 1, (ctypes.c_double * 7)()) == -1
    sim.close()


@pytest.mark.parametrize("precision", ["double", "single"])
def test_stress_kernels_use_no_scratch_and_keep_the_waves_of_the_virial(precision):
    """Every pair function has its instance, the two summary kernels exist, none spills to scratch, and each instance keeps at least the waves per
    SIMD test_pressure.py pins for the Virial_thread_atom instance of the same functor (it carries six accumulators fewer)."""
    blocks = device_isa.blocks(precision, r"AtomStress_\w+")
    names = sorted(blocks)
    assert len(names) == 6, names
    assert len([n for n in names if "AtomStress_thread_atom" in n]) == 4
    for pair in ("VirialLj", "VirialLjTable", "VirialEamILb0E", "VirialEamILb1E"):
        assert any("AtomStress_thread_atom" in n and pair in n for n in names), (pair, names)
    assert any(re.search(r"AtomStress_SummaryP", n) for n in names) and any("AtomStress_SummaryFinal" in n for n in names)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    for pair, waves in VIRIAL_WAVES[precision].items():
        device_isa.assert_keeps_waves(blocks, f"AtomStress_thread_atomI{pair}Ev", waves)


# ---------------------------------------------------------------- GPU: the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", [("A", 0), ("B", 0), ("BI", 0), ("C", 0), ("D", 0), ("E", 0), ("F", 0), ("A", 10), ("E", 10)])
def test_pair_part_matches_the_restatement(gpu, name, steps):
    """atomic_stress(kinetic=False) of every atom against the all-pairs sum, 1e-11 A_i,ab; after 10 steps atoms have changed cells."""
    m = _state(gpu, name, steps)
    _assert_state_is_what_it_claims(name, _state(gpu, name, 0))
    assert m["s0"].shape == (STATES[name]["atoms"], 6) and m["s0"].dtype == np.float64
    assert m["cnt"].min() > 0 and np.all(m["A"] > 0.0)
    _assert_close(m["s0"], m["want"], 1e-11 * m["A"], f"{name} step {steps}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "BI", "C", "D", "E", "F"])
def test_rows_add_up_to_the_virial(gpu, name):
    """sum_i atomic_stress(kinetic) = -(W) or -(K + W) of virial() on the same state, within 1e-11 sum_i A_i per component."""
    m = _state(gpu, name)
    bound = 1e-11 * m["A"].sum(0)
    _assert_close(m["s0"].sum(0), -m["w"], bound, f"{name} pair")
    _assert_close(m["s1"].sum(0), -(m["k"] + m["w"]), bound, f"{name} pair + kinetic")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D", "F"])
def test_spline_rows_add_up_to_the_virial(gpu, name):
    """-P: the splines have no pinned restatement, the sum rule is their check.  The positions are those of the state without -P, so the bound is its
    sum_i A_i (the splines and the quadratic tables are fits of the same functions)."""
    m = _state(gpu, name)
    with gpu.Simulation(STATES[name]["flags"] + ["-P"]) as sim:
        assert np.array_equal(sim.gather(0), m["pos"])
        s0, s1 = sim.atomic_stress(kinetic=False), sim.atomic_stress(kinetic=True)
        w, k = sim.virial()
    assert np.abs(s0 - m["s0"]).max() > 0.0                    # another pair function ran
    bound = 1e-11 * m["A"].sum(0)
    _assert_close(s0.sum(0), -_six(w), bound, f"{name} -P pair")
    _assert_close(s1.sum(0), -_six(k + w), bound, f"{name} -P pair + kinetic")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "D"])
def test_kinetic_part_is_minus_p_p_over_m(gpu, name):
    """atomic_stress(True) - atomic_stress(False) = -p_i p_i^T / m per atom to 1e-12 of the component, with m = sum |p|^2 / (2 eKinetic).  Both arrays
    are stored doubles, so their difference also carries the rounding of each, 2^-53 (|s1| + |s0|), which is part of the bound.  The trace of the
    difference summed over the atoms is -2 eKinetic."""
    m = _state(gpu, name)
    p = m["mom"]
    mass = (p * p).sum() / (2.0 * m["ek"])
    want = -np.stack([p[:, a] * p[:, b] for a, b in COMP], axis=1) / mass
    assert np.abs(want).max() > 1e-3                            # eV: there is a kinetic part
    floor = EPS53 * (np.abs(m["s1"]) + np.abs(m["s0"]))
    _assert_close(m["s1"] - m["s0"], want, 1e-12 * np.abs(want) + floor, f"{name} kinetic")
    trace = (m["s1"] - m["s0"])[:, :3].sum()
    assert abs(trace + 2.0 * m["ek"]) <= 1e-12 * 2.0 * m["ek"] + 2.0 * floor[:, :3].sum(), (trace, -2.0 * m["ek"])


# ---------------------------------------------------------------- GPU: physics on a perfect lattice
@pytest.mark.gpu
@pytest.mark.parametrize("lat", [3.5, 3.7])
@pytest.mark.parametrize("pot,n,rc", [("lj", 8, 5.0 * SIGMA), ("eam", 6, 4.95)])
def test_perfect_lattice_has_one_tensor_without_shear(gpu, pot, n, rc, lat):
    """-r 0 -T 0: every atom's tensor is -W / N within 1e-11 A (A of atom 0, by symmetry every atom's), the off-diagonals and the von Mises stress
    are 0 within that.  After deform((1.02, 1, 1)) the atoms still agree with each other and von_mises() is the von Mises figure of the global tensor
    over N Omega = V; it is Lipschitz in the components with constant sqrt(15) < 4, which turns the bound on the components into one on it."""
    flags = ["-x", n, "-y", n, "-z", n, "-l", lat, "-r", 0, "-T", 0] + (["-e"] if pot == "eam" else [])
    with gpu.Simulation(flags) as sim:
        for scale in (None, (1.02, 1.0, 1.0)):
            if scale:
                sim.deform(scale)
            s, big_n = sim.atomic_stress(), sim.n_global
            w, k = sim.virial()
            vm, omega = sim.von_mises(), sim.atomic_volume
            assert abs(omega * big_n - sim.volume) <= 1e-14 * sim.volume
            fr_of = _pair_function("eam", sim.eam_table(0), sim.eam_table(1), sim.gather(5).copy()) if pot == "eam" else _pair_function("lj")
            _, big_a, cnt = _restate(sim.gather(0), sim.box, rc, fr_of, rows=[0])
            assert cnt[0] > 12 and np.abs(k).max() == 0.0
            bound = np.broadcast_to(1e-11 * big_a[0], s.shape)
            _assert_close(s, np.broadcast_to(-_six(w) / big_n, s.shape), bound, f"{pot} {lat} {scale} tensor")
            assert np.all(np.abs(s[:, 3:]) <= bound[:, 3:])
            vm_global = _von_mises(-_six(w)) / sim.volume
            assert np.all(np.abs(vm - vm_global) <= 4.0 * 1e-11 * big_a[0].max() / omega), (vm.min(), vm.max(), vm_global)
            if scale is None:
                assert vm_global <= 4.0 * 1e-11 * big_a[0].max() / omega
            else:
                assert vm_global * GPA > 0.1                    # the strained lattice carries a deviatoric stress of GPa size


# ---------------------------------------------------------------- GPU: methods, layouts, ranks
CHILD_RUN = """
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    assert pkg.PRECISION == {precision!r}
    sim = pkg.Simulation({args!r})
    eam = {eam}
    one = np.zeros(1)
    np.savez({out!r}, s=sim.atomic_stress(kinetic=False), w=np.array(sim.virial()[0]), pos=sim.gather(0), df=sim.gather(5) if eam else one,
             phi=np.array(sim.eam_table(0)[2]) if eam else one, rho=np.array(sim.eam_table(1)[2]) if eam else one,
             phi_x=np.array(sim.eam_table(0)[:2]) if eam else one, rho_x=np.array(sim.eam_table(1)[:2]) if eam else one)
    sim.close()
"""


def _stress_in_child(args, out, env=None, eam=False, precision="double"):
    """atomic_stress(kinetic=False), W, the positions and (EAM) F' and the tables of a simulation made in a process of its own"""
    proc = _child(CHILD_RUN.format(args=list(args), out=str(out), eam=eam, precision=precision), env=env)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "D"])
def test_methods_and_layouts_agree(gpu, tmp_path, name):
    """The method lists of tests/test_pressure.py on the 2-cell LJ box and the setfl state: every method, cell numbering, stream mode, list format and
    halo form gives thread_atom's per-atom array within 1e-12 max A."""
    st, m = STATES[name], _state(gpu, name)
    lj = st["pair"] != "eam"
    got = {}
    for method, extra in LJ_METHODS if lj else EAM_METHODS:
        with gpu.Simulation(st["flags"] + ["-m", method] + extra) as sim:
            got[" ".join([method] + [str(x) for x in extra])] = sim.atomic_stress(kinetic=False)
    for env in [{"COMD_NL_GLOBAL": "1"}] if lj else [{"COMD_EAM_GROUPS": "0"}, {"COMD_HALO_MIRROR": "0"}]:
        method = "thread_atom_nl" if "COMD_NL_GLOBAL" in env else "cta_cell"
        got[f"{method} {env}"] = _stress_in_child(st["flags"] + ["-m", method], tmp_path / f"{len(got)}.npz", env=env)["s"]
    assert np.array_equal(got["thread_atom"], m["s0"])          # bit-reproducible run to run
    for key, s in got.items():
        err = np.abs(s - got["thread_atom"]).max()
        print(key, err / m["A"].max())
        assert err <= 1e-12 * m["A"].max(), (key, err)


def _ranks(grid, args, out_dir, timeout=900):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    assert world <= 8
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "stress_worker.py"), str(r), str(world), port, *map(str, grid), str(out_dir), json.dumps(args)],
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
    return [(np.load(os.path.join(out_dir, f"stress_rank{r}.npy")), json.load(open(os.path.join(out_dir, f"stress_rank{r}.json")))) for r in range(world)]


@functools.lru_cache(maxsize=None)
def _one_rank(pot, n):
    """the one-rank array and summary of the rank test's state, and max A over its first 256 atoms (at most the max over all: the stricter bound)"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    args = ["-x", n, "-y", n, "-z", n, "-r", 0.1] + (["-e"] if pot == "eam" else [])
    with pkg.Simulation(args) as sim:
        s, summary, omega = sim.atomic_stress(), sim.stress_summary(), sim.atomic_volume
        fr_of = _pair_function("eam", sim.eam_table(0), sim.eam_table(1), sim.gather(5).copy()) if pot == "eam" else _pair_function("lj")
        _, big_a, _ = _restate(sim.gather(0), sim.box, 4.95 if pot == "eam" else 5.0 * SIGMA, fr_of, rows=np.arange(256))
    return args, s, summary, float(big_a.max()), omega


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot,n", [("lj", 14), ("eam", 8)])
def test_ranks_give_the_one_rank_array(gpu, tmp_path, grid, pot, n):
    """2 and 8 ranks sharing the device (gloo transport): every rank returns the global array, the one-rank one within 1e-12 max A, and the summary
    reduced over the ranks: the same gid of the maximum, the extremes and the means within 4 x 1e-12 max A / Omega (what the bound on the components
    allows the pressure and the von Mises stress of an atom: the latter is Lipschitz in the components with constant sqrt(15) < 4)."""
    args, s0, sum0, a_max, omega = _one_rank(pot, n)
    vm0 = _von_mises(s0)
    order = np.sort(vm0)
    assert order[-1] - order[-2] > 8.0 * 1e-12 * a_max              # the maximum is not a near-tie the ranks could resolve differently
    for s, summary in _ranks(grid, args, tmp_path):
        assert s.shape == s0.shape and np.abs(s - s0).max() <= 1e-12 * a_max, np.abs(s - s0).max() / a_max
        assert summary["n"] == sum0["n"] == len(s0) and summary["max_von_mises_gid"] == sum0["max_von_mises_gid"] == int(np.argmax(vm0))
        for key in ("min_pressure", "max_pressure", "max_von_mises", "mean_pressure", "mean_von_mises"):
            assert abs(summary[key] - sum0[key]) <= 4.0 * 1e-12 * a_max / omega, key


# ---------------------------------------------------------------- GPU: the device reduction
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "E"])
def test_summary_is_numpy_on_the_array(gpu, name):
    """stress_summary() against numpy on atomic_stress() of the same state: means to 1e-12 relative, extremes to 1e-14 relative, the same gid of the
    maximum (the two largest von Mises stresses differ by more than that margin)."""
    m = _state(gpu, name)
    s, omega, got = m["s1"], m["omega"], m["summary"]
    p = -(s[:, 0] + s[:, 1] + s[:, 2]) / (3.0 * omega)
    vm = _von_mises(s) / omega
    order = np.sort(vm)
    assert order[-1] - order[-2] > 1e-14 * order[-1]
    assert got["n"] == len(s) and got["max_von_mises_gid"] == int(np.argmax(vm))
    for key, want, tol in (("mean_pressure", p.mean(), 1e-12), ("mean_von_mises", vm.mean(), 1e-12), ("min_pressure", p.min(), 1e-14),
                           ("max_pressure", p.max(), 1e-14), ("max_von_mises", vm.max(), 1e-14)):
        print(name, key, got[key], want, abs(got[key] - want) / abs(want))
        assert abs(got[key] - want) <= tol * abs(want), (key, got[key], want)
    with gpu.Simulation(STATES[name]["flags"]) as sim:
        assert np.array_equal(sim.atomic_pressure(), -((s[:, 0] + s[:, 1]) + s[:, 2]) * ((1.0 / omega) / 3.0))
        assert np.abs(sim.von_mises() - vm).max() <= 1e-14 * vm.max()
        assert sim.stress_summary() == got                                  # bit-reproducible run to run
        assert sim.stress_summary(kinetic=False)["mean_pressure"] != got["mean_pressure"]


# ---------------------------------------------------------------- GPU: single precision
@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
def test_single_precision_build(gpu, tmp_path, pot):
    """The float build (COMD_PRECISION=single, lib*_sp.so) in a child, state B and the Adams 6^3 state: every component of every atom against the
    restatement (in double) of the child's own gathered positions, tables and F', within (n_i + 64) 2^-24 A_i,ab.  The sum rule against the child's
    virial(): the rows carry that bound each, computeVirial's sum carries the same per atom and is rounded to real_t once more."""
    n = 8 if pot == "lj" else 6
    args = ["-x", n, "-y", n, "-z", n, "-l", LAT, "-r", 0.1] + (["-e"] if pot == "eam" else [])
    d = _stress_in_child(args, tmp_path / "single.npz", env={"COMD_PRECISION": "single"}, eam=pot == "eam", precision="single")
    if pot == "eam":
        fr_of = _pair_function("eam", (d["phi_x"][0], d["phi_x"][1], d["phi"]), (d["rho_x"][0], d["rho_x"][1], d["rho"]), d["df"])
    else:
        fr_of = _pair_function("lj")
    extent = np.float64(np.float32(n * np.float32(LAT))) * np.ones(3)          # the float box of the child
    want, big_a, cnt = _restate(d["pos"], extent, 4.95 if pot == "eam" else 5.0 * SIGMA, fr_of)
    bound = (cnt[:, None] + 64.0) * EPS24 * big_a
    _assert_close(d["s"], want, bound, f"single {pot}")
    w = _six(d["w"])
    _assert_close(d["s"].sum(0), -w, 2.0 * bound.sum(0) + EPS24 * np.abs(w), f"single {pot} sum rule")


# ---------------------------------------------------------------- GPU: comd-hip
HEADER = "#  Loop   Time(fs)       Total Energy   Potential Energy     Kinetic Energy  Temperature   (us/atom)     # Atoms"


def _comd_hip(tmp_path, extra, ok=True):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-N", "20", "-n", "10", "-x", "8", "-y", "8", "-z", "8", "-d", os.path.join(ROOT, "pots")] + extra,
                          capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert (proc.returncode == 0) == ok, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    text = ""
    for f in yaml:
        text += (tmp_path / f).read_text()
        os.remove(tmp_path / f)
    return proc.stdout, rows, text


@pytest.mark.gpu
def test_comd_hip_stress_column_file_dump_and_yaml(gpu, tmp_path):
    out0, rows0, yaml0 = _comd_hip(tmp_path, [])
    # without the flag: the table of before (no column, no timer row, no file, nothing in the YAML)
    assert [line for line in out0.splitlines() if line.startswith("#  Loop")] == [HEADER]
    assert all(r[3].strip() == "" for r in rows0) and [r[0] for r in rows0] == ["0", "10", "20"]
    assert "MaxVM" not in out0 and not re.search(r"^stress\s", out0, flags=re.M) and "Stress" not in yaml0 and not os.path.exists(tmp_path / "stress.dat")

    out1, rows1, yaml1 = _comd_hip(tmp_path, ["--stress", "--pressure", "--stressDump", "dump.xyz"])
    header = [line for line in out1.splitlines() if line.startswith("#  Loop")][0]
    assert header.startswith(HEADER) and header.split()[-2:] == ["Pressure(GPa)", "MaxVM(GPa)"]
    assert [r[:3] for r in rows1] == [r[:3] for r in rows0]                  # the trajectory is untouched by the flag, to the bit
    cols = [[float(x) for x in r[3].split()] for r in rows1]
    assert all(len(c) == 2 for c in cols)
    assert re.search(r"^stress\s+4\s", out1, flags=re.M)                     # three samples and the dump
    lines = (tmp_path / "stress.dat").read_text().splitlines()
    assert lines[0].startswith("# Stress: N 2048 ") and "samples 3" in lines[0]
    data = [[float(x) for x in line.split()] for line in lines[1:]]
    assert [d[0] for d in data] == [0.0, 10.0, 20.0] and all(len(d) == 7 for d in data)
    for d, c in zip(data, cols):
        assert abs(d[1] - c[0]) <= 1e-10, (d[1], c[0])                       # mean hydrostatic pressure = the Pressure(GPa) column, to its 10 decimals
        assert abs(d[5] - c[1]) <= 1e-10 and d[2] <= d[1] <= d[3] and 0.0 < d[4] <= d[5]
        assert 0 <= d[6] < 2048 and d[6] == int(d[6])
    dump = (tmp_path / "dump.xyz").read_text().splitlines()
    assert dump[0] == "2048" and len(dump) == 2 + 2048 and "Properties=species:S:1:pos:R:3:stress:R:6:vm:R:1:gid:I:1" in dump[1] and "step=20" in dump[1]
    atoms = np.array([[float(x) for x in line.split()[1:]] for line in dump[2:]])
    assert atoms.shape == (2048, 11) and np.array_equal(atoms[:, 10], np.arange(2048))
    assert np.abs(_von_mises(atoms[:, 3:9]) - atoms[:, 9]).max() <= 1e-12 * atoms[:, 9].max()
    assert abs(atoms[:, 9].max() - data[-1][5]) <= 1e-12 * data[-1][5] and int(np.argmax(atoms[:, 9])) == int(data[-1][6])
    assert abs(-(atoms[:, 3:6].sum(1) / 3.0).mean() - data[-1][1]) <= 1e-10
    block = re.search(r"^Stress:\n((?:  .*\n)+)", yaml1, flags=re.M).group(1)
    m = dict(re.findall(r"^  (\w+): (\S+)$", block, flags=re.M))
    assert m["samples"] == "3" and m["file"] == "stress.dat"
    assert abs(float(m["finalMeanPressure"]) - data[-1][1]) <= 1e-11 * abs(data[-1][1])
    assert abs(float(m["finalMeanVonMises"]) - data[-1][4]) <= 1e-11 * data[-1][4] and abs(float(m["finalMaxVonMises"]) - data[-1][5]) <= 1e-11 * data[-1][5]

    # --stressDumpMin: only the atoms at or above the threshold; a negative one is refused before any step
    cut = float(np.median(atoms[:, 9]))
    _comd_hip(tmp_path, ["--stress", "--stressDump", "cut.xyz", "--stressDumpMin", repr(cut), "--stressFile", "other.dat"])
    kept = (tmp_path / "cut.xyz").read_text().splitlines()
    assert int(kept[0]) == len(kept) - 2 == int((atoms[:, 9] >= cut).sum()) and os.path.exists(tmp_path / "other.dat")
    out2, rows2, _ = _comd_hip(tmp_path, ["--stress", "--stressDumpMin", "-1"], ok=False)
    assert "Error:" in out2 and "stressDumpMin" in out2 and rows2 == []


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--csp", "--cna", "--pressure", "--erateX", "0.01", "--langevin", "-H", "-a", "1"],
                                   ["-e", "--csp", "--cna", "--erateX", "0.01", "--langevin", "-m", "cta_cell", "-a", "1", "-x", "6", "-y", "6", "-z", "6"],
                                   ["-I", "-m", "thread_atom_nl"], ["-e", "-P", "-H", "-x", "6", "-y", "6", "-z", "6"]])
def test_comd_hip_stress_with_the_other_flags(gpu, tmp_path, extra):
    """--stress beside the other analyses, a straining box, the thermostat, both numberings, the overlap mode, -I and -P: the column is the last one,
    three samples, and the flag leaves the other columns and the trajectory as they are without it, to the bit."""
    out0, rows0, _ = _comd_hip(tmp_path, extra)
    out1, rows1, yaml1 = _comd_hip(tmp_path, extra + ["--stress"])
    header0, header1 = [[line for line in out.splitlines() if line.startswith("#  Loop")][0] for out in (out0, out1)]
    assert header1.split()[:-1] == header0.split() and header1.split()[-1] == "MaxVM(GPa)"
    assert len(rows1) == 3 and [r[:3] for r in rows1] == [r[:3] for r in rows0]
    for r0, r1 in zip(rows0, rows1):
        assert r1[3].split()[:-1] == r0[3].split() and float(r1[3].split()[-1]) > 0.0
    lines = (tmp_path / "stress.dat").read_text().splitlines()
    assert len(lines) == 4 and [float(line.split()[5]) for line in lines[1:]] == pytest.approx([float(r[3].split()[-1]) for r in rows1], abs=1e-10)
    assert "Stress:" in yaml1 and re.search(r"^stress\s+4\s", out1, flags=re.M)            # three samples and the files
