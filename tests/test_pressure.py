"""Pressure and the virial stress tensor (computeVirial, Simulation.virial / pressure_tensor / pressure, comd-hip --pressure).

CoMD computes no virial, so nothing here is compared with a recorded number.  The checks are physics and restatement:
  * the kinetic half: trace(K) = 2 eKinetic of the existing energy path;
  * the pair virial is the strain derivative of the existing potential energy: on a perfect lattice P = -dU/dV, and on a disordered
    state scaled isotropically by lambda, -dU/dlambda = trace(W) -- both by Richardson-extrapolated central differences, as in
    tests/test_finite_difference.py, with the tolerances that file states for the interpolated EAM tables;
  * the full tensor against an O(N^2) minimum-image restatement in numpy (LJ analytic, LJ -I, EAM setfl);
  * every method, layout, stream mode and rank count gives the same tensor for the same state.
Tensors are compared component by component against the largest component of the reference tensor (off-diagonals included).
"""
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import device_isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "comd-cuda-async_amd", "csrc")
SINGLE = os.environ.get("COMD_PRECISION", "double") == "single"
TOL = json.load(open(os.path.join(HERE, "golden", "reference_values.json")))["tolerances_single" if SINGLE else "tolerances"]

SIGMA, EPS, LAT = 2.315, 0.167, 3.615
GPA = 160.21766208                                   # GPa per eV/A^3
MISHIN = ["-e", "-t", "setfl", "-p", "Cu01.eam.alloy"]
ADAMS = ["-e"]
RC = {"lj5": 5.0 * SIGMA, "lj2.5": 2.5 * SIGMA, "adams": 4.95, "mishin": 5.50679}
POT = {"lj5": [], "lj2.5": ["--ljCutoffSigmas", 2.5], "adams": ADAMS, "mishin": MISHIN}
# waves per SIMD of the instances of Virial_thread_atom, by the mangled name of the pair functor (VirialEam<false>: the quadratic tables)
VIRIAL_WAVES = {"double": {"8VirialLj": 6, "13VirialLjTable": 5, "9VirialEamILb1EE": 5, "9VirialEamILb0EE": 4},
                "single": {"8VirialLj": 8, "13VirialLjTable": 7, "9VirialEamILb1EE": 7, "9VirialEamILb0EE": 7}}


def _cube(n):
    return ["-x", n, "-y", n, "-z", n]


def _rel(a, b):
    """max |a - b| over the components, relative to the largest component of b"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


PRELUDE = f"import sys, json\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\n"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


VIRIAL_RUN = """
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    sim.step({steps}) if {steps} else None
    w, k = sim.virial()
    print("VIRIAL", json.dumps([w.tolist(), k.tolist()]))
    sim.close()
"""


def _virial_in_child(args, steps=0, env=None):
    proc = _child(VIRIAL_RUN.format(args=list(args), steps=steps), env=env)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    w, k = json.loads(re.search(r"^VIRIAL (.*)$", proc.stdout, flags=re.M).group(1))
    return np.array(w), np.array(k)


# ---------------------------------------------------------------- CPU: flag, export, ISA
def test_pressure_flag_is_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--pressure'], host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    assert re.search(r"^\s+--pressure\s", proc.stdout, flags=re.M), proc.stdout[-3000:]


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_compute_virial_is_exported_and_declared(sfx):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_hip{sfx}.so")], capture_output=True, text=True).stdout
    assert "computeVirial" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_host{sfx}.so")], capture_output=True, text=True).stdout
    assert "comdVirial" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeVirial\(SimGpu\* sim, real_t\* out12\);", header, flags=re.M)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_virial_kernels_use_no_scratch(precision):
    """Every pair function has its instance (LJ analytic, LJ table, EAM quadratic tables, EAM splines), none spills to scratch, and each keeps
    the registers of its waves per SIMD."""
    blocks = device_isa.blocks(precision, r"Virial_\w+")
    names = sorted(blocks)
    assert len(names) == 5, names
    for pair in ("VirialLj", "VirialLjTable", "VirialEamILb0E", "VirialEamILb1E"):
        assert any(pair in n for n in names), (pair, names)
    assert any("Virial_Final" in n for n in names)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    for pair, waves in VIRIAL_WAVES[precision].items():
        device_isa.assert_keeps_waves(blocks, f"Virial_thread_atomI{pair}Ev", waves)


# ---------------------------------------------------------------- numpy restatement
def _pairs(pos, extent, rc):
    """all pairs i != j within rc under the minimum image: (i index, d = r_i - r_j, r)"""
    out = []
    for s in range(0, len(pos), 512):
        d = pos[s:s + 512, None, :] - pos[None, :, :]
        d -= np.rint(d / extent) * extent
        r2 = (d * d).sum(-1)
        hit = (r2 > 0.0) & (r2 <= rc * rc)
        ii, jj = np.nonzero(hit)
        out.append((ii + s, jj, d[ii, jj], np.sqrt(r2[ii, jj])))
    return [np.concatenate(x) for x in zip(*out)]


def _tensor(d, f):
    """1/2 sum over ordered pairs of d f^T (every unordered pair appears twice)"""
    return 0.5 * np.einsum("pa,pb->ab", d, f)


def _interpolate(x0, inv, v, r):
    """device_common.h interpolate<CLAMP> on a padded table (v[0] the leading pad), value and derivative"""
    n = len(v) - 3
    xn = x0 + n / inv
    r = np.minimum(np.maximum(r, x0), xn)
    r = r * inv - x0 * inv
    ri = np.floor(r)
    ii = ri.astype(np.int64)
    r = r - ri
    v0, v1, v2, v3 = v[ii], v[ii + 1], v[ii + 2], v[ii + 3]
    g1, g2 = v2 - v0, v3 - v1
    return v1 + 0.5 * r * (g1 + r * (v2 + v0 - 2.0 * v1)), (g1 + r * (g2 - g1)) * (inv * 0.5)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj5", "adams"])
def test_kinetic_tensor_trace_is_twice_the_kinetic_energy(gpu, pot):
    with gpu.Simulation(_cube(10) + ["-r", 0.05] + POT[pot]) as sim:
        for steps in (0, 10):
            sim.step(steps) if steps else None
            w, k = sim.virial()
            ek = sim.energy()[1]
            assert abs(np.trace(k) - 2.0 * ek) <= 1e-13 * 2.0 * ek, (steps, np.trace(k), 2.0 * ek)
            assert np.array_equal(k, k.T) and np.array_equal(w, w.T)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["thread_atom", "cta_cell"])
@pytest.mark.parametrize("a", [3.5, 3.7])
@pytest.mark.parametrize("pot,n,tol", [("lj5", 8, 1e-7), ("lj2.5", 8, 1e-7), ("mishin", 6, 1e-5), ("adams", 6, 3e-3)])
def test_lattice_pressure_is_minus_dU_dV(gpu, pot, n, tol, a, method):
    """Perfect lattice at T = 0: P = trace(W) / 3V against -dU/dV = -(dU/da) / (3 n^3 a^2), U the potential energy of the existing path at
    a (1 +- h) and a (1 +- h/2), Richardson-extrapolated.  No lattice shell lies within 0.03 A of the LJ cutoffs at these lattice constants."""
    base = _cube(n) + ["-T", 0, "-r", 0, "-m", method] + POT[pot]

    def energy(lat):
        with gpu.Simulation(base + ["-l", repr(lat)]) as sim:
            return sim.energy()[0]

    h = 1e-4
    d = [(energy(a * (1 + s)) - energy(a * (1 - s))) / (2 * a * s) for s in (h, 0.5 * h)]
    dU = (4.0 * d[1] - d[0]) / 3.0
    p_fd = -dU / (3.0 * n ** 3 * a * a)
    with gpu.Simulation(base + ["-l", repr(a)]) as sim:
        w, k = sim.virial()
        p = sim.pressure()
        v = (n * a) ** 3
    assert abs(np.trace(k)) <= 1e-12 * abs(np.trace(w))
    assert abs(p - np.trace(w + k) / (3.0 * v)) <= 1e-13 * abs(p)
    assert abs(p * GPA) > 0.5                                   # GPa-sized
    if pot == "adams" and a == 3.5:
        # At 3.5 A the Adams pressure is a 16:1 cancellation of the pair and the embedding terms, and the value/derivative mismatch of its
        # 500-sample tables is 3 % of P (the numpy lattice sum of the same tables: -dU/dV of the interpolated values vs the interpolated
        # derivatives).  The check there is the lattice sum with the tables' derivatives, and that the gap to -dU/dV is the tables' own.
        with gpu.Simulation(base + ["-l", repr(a)]) as sim:
            p_tab = _eam_lattice_pressure(sim, a, RC[pot])
        assert abs(p - p_tab) <= 1e-10 * abs(p_tab), (p, p_tab)
        assert abs(p - p_fd) <= 0.06 * abs(p_fd), (pot, a, method, p * GPA, p_fd * GPA)
    else:
        assert abs(p - p_fd) <= tol * abs(p_fd), (pot, a, method, p * GPA, p_fd * GPA)


def _eam_lattice_pressure(sim, a, rc):
    """virial pressure of a perfect fcc lattice from the EAM tables of `sim`: interpolated derivatives, the lattice sum over one atom's shells"""
    c = np.array([(i + u, j + v, k + w) for i in range(-3, 4) for j in range(-3, 4) for k in range(-3, 4)
                  for u, v, w in ((0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5))]) * a
    r = np.sqrt((c * c).sum(1))
    r = r[(r > 0) & (r <= rc)]
    rb = _interpolate(*sim.eam_table(1), r)[0].sum()
    df = _interpolate(*sim.eam_table(2), np.array([rb]))[1][0]
    w_atom = -(0.5 * _interpolate(*sim.eam_table(0), r)[1] * r).sum() - df * (_interpolate(*sim.eam_table(1), r)[1] * r).sum()
    return w_atom / (3.0 * a ** 3 / 4.0)


def _scaled_energy(gpu, args, lat, r0, lam):
    with gpu.Simulation(args + ["-l", repr(lat * lam)]) as sim:
        sim.scatter(0, lam * r0)
        sim.redistribute()
        sim.compute_force()
        sim.kinetic_energy()
        return sim.energy()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("pot,h,tol", [("lj5", 1e-8, 1e-7), ("mishin", 1e-5, 1e-5)])
def test_isotropic_scaling_of_a_disordered_state(gpu, pot, h, tol):
    """trace(W) = -dU/dlambda at lambda = 1 for positions lambda r0 in a box lambda L.  The shifted LJ energy has a kink at the cutoff: no pair
    of the state may be within 2 h r of it (asserted from the positions; h is small enough that this holds for the seeded displacement)."""
    n, lat = 8, 3.5
    args = _cube(n) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args + ["-l", repr(lat)]) as sim:
        r0 = sim.gather(0).copy()
        w, _ = sim.virial()
    if pot.startswith("lj"):
        _, _, _, r = _pairs(r0, n * lat, RC[pot] * 1.001)
        assert not np.any(np.abs(r - RC[pot]) <= 2.0 * h * r), "a pair sits in the finite-difference window of the cutoff"
    d = [(_scaled_energy(gpu, args, lat, r0, 1 + s) - _scaled_energy(gpu, args, lat, r0, 1 - s)) / (2 * s) for s in (h, 0.5 * h)]
    dU = (4.0 * d[1] - d[0]) / 3.0
    assert abs(np.trace(w) + dU) <= tol * abs(dU), (pot, np.trace(w), -dU)


@pytest.mark.gpu
def test_lj_tensor_matches_the_restatement(gpu):
    n = 8
    with gpu.Simulation(_cube(n) + ["-r", 0.1, "-l", repr(LAT)]) as sim:
        pos = sim.gather(0)
        w, _ = sim.virial()
    i, j, d, r = _pairs(pos, n * LAT, RC["lj5"])
    s6 = SIGMA ** 6
    fr = 24.0 * EPS * s6 * r ** -8 * (2.0 * s6 * r ** -6 - 1.0)
    want = _tensor(d, fr[:, None] * d)
    assert _rel(w, want) <= 1e-11, (w, want)


@pytest.mark.gpu
def test_lj_table_tensor_matches_the_restatement(gpu):
    from test_lj_interpolation import interpolate, lj_table
    n = 8
    with gpu.Simulation(_cube(n) + ["-r", 0.1, "-l", repr(LAT), "-I"]) as sim:
        pos = sim.gather(0)
        w, _ = sim.virial()
    i, j, d, r = _pairs(pos, n * LAT, RC["lj5"])
    _, dv = interpolate(lj_table(), r)
    want = _tensor(d, (-dv / r)[:, None] * d)
    assert _rel(w, want) <= 1e-11, (w, want)


@pytest.mark.gpu
def test_eam_setfl_tensor_matches_the_restatement(gpu):
    n = 6
    with gpu.Simulation(_cube(n) + ["-r", 0.1, "-l", repr(LAT)] + MISHIN) as sim:
        pos, df = sim.gather(0), sim.gather(5)
        phi, rho = sim.eam_table(0), sim.eam_table(1)
        w, _ = sim.virial()
    i, j, d, r = _pairs(pos, n * LAT, RC["mishin"])
    _, dphi = _interpolate(*phi, r)
    _, drho = _interpolate(*rho, r)
    s = (dphi + (df[i] + df[j]) * drho) / r
    want = _tensor(d, -s[:, None] * d)
    assert _rel(w, want) <= 1e-11, (w, want)


LJ_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("cta_cell", ["-L", "-S", 0.03]), ("thread_atom_nl", []),
              ("thread_atom", ["-H"]), ("thread_atom", ["-a", 1]), ("cta_cell", ["-a", 1])]
EAM_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("thread_atom_nl", []), ("cta_cell", ["-H"]), ("cta_cell", ["-a", 1]),
               ("thread_atom", ["-a", 1])]


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 12), ("mishin", 10)])
def test_methods_and_layouts_agree(gpu, pot, n):
    """Step 0, the same state under every method, cell numbering, stream mode, list format and halo form: the same tensors to 1e-12."""
    base = _cube(n) + ["-r", 0.1] + POT[pot]
    got = {}
    for method, extra in LJ_METHODS if pot.startswith("lj") else EAM_METHODS:
        with gpu.Simulation(base + ["-m", method] + extra) as sim:
            got[" ".join([method] + [str(x) for x in extra])] = sim.virial()
    envs = [{"COMD_NL_GLOBAL": "1"}] if pot.startswith("lj") else [{"COMD_EAM_GROUPS": "0"}, {"COMD_HALO_MIRROR": "0"}]
    for env in envs:
        method = "thread_atom_nl" if "COMD_NL_GLOBAL" in env else "cta_cell"
        got[f"{method} {env}"] = _virial_in_child(base + ["-m", method], env=env)
    w0, k0 = got["thread_atom"]
    for name, (w, k) in got.items():
        assert _rel(w, w0) <= 1e-12, (name, w, w0)
        assert _rel(k, k0) <= 1e-12, name


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 12), ("adams", 10)])
def test_neighbor_list_trajectory_agrees(gpu, pot, n):
    """20 steps of thread_atom_nl against thread_atom, at the tolerance of the existing multi-step comparisons (100 x the one-evaluation force bound)."""
    got = {}
    for method in ("thread_atom", "thread_atom_nl"):
        with gpu.Simulation(_cube(n) + ["-r", 0.1, "-m", method] + POT[pot]) as sim:
            sim.step(20)
            got[method] = sim.virial()
    for c in range(2):
        assert _rel(got["thread_atom_nl"][c], got["thread_atom"][c]) <= 100 * TOL["force_rel_to_max"], c


def _ranks(grid, args, timeout=900):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "pressure_worker.py"), str(r), str(world), port, *map(str, grid), json.dumps(args)],
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
    return [json.loads(re.search(r"^VIRIAL (.*)$", out, flags=re.M).group(1)) for out in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot,n", [("lj5", 14), ("adams", 8)])
def test_ranks_give_the_one_rank_tensor(gpu, grid, pot, n):
    """2 and 8 ranks sharing the device (gloo transport): every rank returns the global tensors, equal to the one-rank ones."""
    args = _cube(n) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args) as sim:
        w0, k0 = sim.virial()
        p0 = sim.pressure_tensor()
    for w, k, p in _ranks(grid, args):
        assert _rel(w, w0) <= 1e-12 and _rel(k, k0) <= 1e-12
        assert _rel(p, p0) <= 1e-12


def _comd_hip(tmp_path, extra, exe="comd-hip"):
    proc = subprocess.run([os.path.join(CSRC, exe), "-N", "20", "-n", "10", "-d", os.path.join(ROOT, "pots")] + extra,
                          capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    assert len(yaml) == 1
    text = (tmp_path / yaml[0]).read_text()
    os.remove(tmp_path / yaml[0])
    return proc.stdout, rows, text


@pytest.mark.gpu
def test_comd_hip_pressure_column(gpu, tmp_path):
    out0, rows0, yaml0 = _comd_hip(tmp_path, [])
    out1, rows1, yaml1 = _comd_hip(tmp_path, ["--pressure"])
    out2, rows2, _ = _comd_hip(tmp_path, ["--pressure"])
    assert [r[0] for r in rows0] == ["0", "10", "20"]
    # without the flag: the table of before (no column, no timer row, nothing in the YAML)
    assert "Pressure" not in out0 and not re.search(r"^pressure\s", out0, flags=re.M) and "Pressure" not in yaml0 and "pressure" not in yaml0
    assert all(r[3].strip() == "" for r in rows0)
    # the energies are untouched by the flag, to the bit; the pressure column is reproducible to the bit
    assert [r[:3] for r in rows1] == [r[:3] for r in rows0]
    assert "Pressure(GPa)" in out1 and re.search(r"^pressure\s+3\s", out1, flags=re.M)
    col1, col2 = [float(r[3]) for r in rows1], [float(r[3]) for r in rows2]
    assert [r[3] for r in rows1] == [r[3] for r in rows2] and len(col1) == 3
    with gpu.Simulation(["-x", 20, "-y", 20, "-z", 20]) as sim:
        p = sim.pressure() * GPA
    assert abs(col1[0] - p) <= 1e-10 + 1e-12 * abs(p), (col1[0], p)
    m = {k: float(v) for k, v in re.findall(r"^  (P\w*|Pressure): (\S+)$", yaml1, flags=re.M)}
    assert set(m) == {"Pressure", "Pxx", "Pyy", "Pzz", "Pyz", "Pxz", "Pxy"}
    assert abs(m["Pressure"] - col1[-1]) <= 1e-10 + 1e-12 * abs(col1[-1])
    assert abs((m["Pxx"] + m["Pyy"] + m["Pzz"]) / 3.0 - m["Pressure"]) <= 1e-11 * abs(m["Pressure"]) + 1e-14


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj5", "adams"])
def test_single_precision_virial(gpu, pot):
    """The float build (COMD_PRECISION=single, lib*_sp.so) on LJ and EAM 20^3 against the double build, 1e-5 of the largest component."""
    args = _cube(20) + ["-r", 0.1, "-l", 3.5] + POT[pot]
    with gpu.Simulation(args) as sim:
        w0, k0 = sim.virial()
    w, k = _virial_in_child(args, env={"COMD_PRECISION": "single"})
    assert _rel(w, w0) <= 1e-5 and _rel(k, k0) <= 1e-5, (w, w0)
