"""The BAOAB Langevin thermostat (comd-hip --langevin, Simulation.set_langevin; hip/langevin_kernels.h).  The reference integrates NVE only.

The noise is Philox4x32-10 keyed by the seed and counted by (gid, step), mapped to normals by Box-Muller exactly as DESIGN.md states; philox()
and normals() below restate it in numpy.  Runs are bit-reproducible, so nothing here is flaky: every statistical bound is at least 4 sigma of
the estimated error of what it bounds (derivations in the docstrings), i.e. a correct implementation passes with any seed.
"""
import json
import os
import re
import shutil
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

KB = 8.6173324e-5                                   # eV/K, comd_host.h kB_eV
LAT = 3.615
POT = {"lj": [], "eam": ["-e"]}
SMALL = {"lj": 7, "eam": 6}                        # the smallest cubes the cutoffs allow at LAT (LJ 5 sigma: 2 x 11.6 A)
SEED = 0x9E3779B97F4A7C15                           # high and low key words both non-zero


def _cube(n):
    return ["-x", n, "-y", n, "-z", n]


def _rel(a, b):
    """max |a - b| over the components, relative to the largest component of b"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _wrap(d, box):
    return d - np.rint(d / box) * box


PRELUDE = f"import sys, json\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\n"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


# ---------------------------------------------------------------- numpy restatement of the noise ("Langevin thermostat")
M32 = np.uint64(0xFFFFFFFF)


def philox(ctr, key):
    """Philox4x32-10: ctr = 4 arrays (or ints) of uint32 words, key = 2 ints -> 4 uint64 arrays holding the uint32 outputs"""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in ctr]
    k0, k1 = np.uint64(key[0]) & M32, np.uint64(key[1]) & M32
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
    return c


def normals(seed, gid, step, dtype=np.float64):
    """xi (n, 3) of atoms `gid` at global step `step`: one Philox call, u_i = (x_i + 0.5) 2^-32, Box-Muller in `dtype`"""
    gid = np.asarray(gid, dtype=np.uint64)
    x = philox([gid, np.uint64(step & 0xFFFFFFFF), np.uint64(step >> 32), np.uint64(0)], [seed & 0xFFFFFFFF, seed >> 32])
    u = [(np.broadcast_to(w, gid.shape).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -32) for w in x]
    two_pi = dtype(2.0 * np.pi)
    ra, rb = np.sqrt(dtype(-2.0) * np.log(u[0])), np.sqrt(dtype(-2.0) * np.log(u[2]))
    return np.stack([ra * np.cos(two_pi * u[1]), ra * np.sin(two_pi * u[1]), rb * np.cos(two_pi * u[3])], axis=1).astype(np.float64)


KAT = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


# ---------------------------------------------------------------- CPU
def test_philox_matches_the_random123_known_answers():
    for ctr, key, want in KAT:
        assert [int(w) for w in philox(ctr, key)] == want


def test_philox_header_matches_on_the_host(tmp_path):
    """hip/philox.h is plain C as well: compiled into a host program it gives the known answers and the numpy words for 4096 (gid, step)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler on PATH"
    src = tmp_path / "kat.c"
    src.write_text(textwrap.dedent("""
        #include <stdio.h>
        #include <stdlib.h>
        #include "philox.h"
        int main(int argc, char** argv) {
           if (argc < 8) return 1;
           uint32_t c[4], k0 = (uint32_t)strtoul(argv[1], 0, 0), k1 = (uint32_t)strtoul(argv[2], 0, 0), o[4];
           for (int a = 0; a < 4; ++a) c[a] = (uint32_t)strtoul(argv[3 + a], 0, 0);
           for (int i = 0; i < atoi(argv[7]); ++i) {
              comdPhilox4x32_10(c, k0, k1, o);
              printf("%u %u %u %u\\n", o[0], o[1], o[2], o[3]);
              c[0] += 977u;
           }
           return 0;
        }
    """))
    exe = tmp_path / "kat"
    proc = subprocess.run([cc, "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(CSRC, "hip"), str(src), "-o", str(exe)],
                          capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr

    def run(ctr, key, n):
        out = subprocess.run([str(exe), *map(str, key), *map(str, ctr), str(n)], capture_output=True, text=True, check=True).stdout
        return np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.uint64)

    for ctr, key, want in KAT:
        assert run(ctr, key, 1)[0].tolist() == want
    step = 0x123456789
    got = run([5, step & 0xFFFFFFFF, step >> 32, 0], [SEED & 0xFFFFFFFF, SEED >> 32], 4096)
    gid = (5 + 977 * np.arange(4096, dtype=np.uint64)) & M32
    want = np.stack(philox([gid, step & 0xFFFFFFFF, step >> 32, 0], [SEED & 0xFFFFFFFF, SEED >> 32]), axis=1)
    assert np.array_equal(got, want)


def test_normals_are_standard_normal():
    """The mapping itself on 10^6 draws: mean, variance, excess kurtosis within 5 sigma of N(0,1) (sigma = 1/sqrt(n), sqrt(2/n), sqrt(24/n))."""
    xi = normals(SEED, np.arange(1 << 18), 7).ravel()
    n = xi.size
    assert abs(xi.mean()) < 5 / np.sqrt(n)
    assert abs(xi.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs(((xi - xi.mean()) ** 4).mean() / xi.var() ** 2 - 3) < 5 * np.sqrt(24 / n)


def test_langevin_flags_are_listed_and_accepted_host_only():
    proc = _child("""
        s = pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '-T', 450, '--langevin', '--langevinDamp', 25, '--seed', 12345678901234567], host_only=True)
        print('A', json.dumps(s.langevin()), s.step_count); s.close()
        s = pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '-T', 450, '--langevinTemp', 300], host_only=True)
        print('B', json.dumps(s.langevin())); s.close()
        s = pkg.Simulation(['-x', 8, '-y', 8, '-z', 8], host_only=True)
        print('C', json.dumps(s.langevin()))
        s.set_langevin(250.0, 40.0)
        print('D', json.dumps(s.langevin()))
        s.set_langevin(250.0, 40.0, seed=3, on=False)
        print('E', json.dumps(s.langevin()))
        for bad in ((-1.0, 40.0), (250.0, 0.0)):
            try:
                s.set_langevin(*bad)
                print('accepted', bad)
            except ValueError:
                pass
        print('F', json.dumps(s.langevin()))
    """)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    assert "invalid switch" not in proc.stdout and "accepted" not in proc.stdout, proc.stdout[-2000:]
    got = {m.group(1): m.group(2) for m in re.finditer(r"^([A-F]) (.*)$", proc.stdout, flags=re.M)}
    a, steps = got["A"].rsplit(" ", 1)
    assert json.loads(a) == {"on": True, "temperature": 450.0, "damp_fs": 25.0, "seed": 12345678901234567} and steps == "0"
    b, c = json.loads(got["B"]), json.loads(got["C"])
    assert b["on"] is False and b["temperature"] == 300.0 and b["damp_fs"] == 100.0
    assert c == {"on": False, "temperature": 600.0, "damp_fs": 100.0, "seed": b["seed"]}         # defaults: -T, 100 fs, a fixed key
    assert json.loads(got["D"]) == {"on": True, "temperature": 250.0, "damp_fs": 40.0, "seed": c["seed"]}
    assert json.loads(got["E"]) == {"on": False, "temperature": 250.0, "damp_fs": 40.0, "seed": 3}
    assert json.loads(got["F"]) == json.loads(got["E"])                                              # refused: nothing changed
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("langevin", "langevinTemp", "langevinDamp", "seed"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


@pytest.mark.parametrize("bad", [["--langevinDamp", 0], ["--langevinDamp", -5], ["--langevinTemp", -1], ["--langevin", "-T", -1]])
def test_invalid_thermostat_settings_are_refused(bad):
    proc = _child(f"pkg.Simulation(['-x', 8, '-y', 8, '-z', 8] + {bad!r}, host_only=True); print('made')")
    assert proc.returncode != 0 and "made" not in proc.stdout, proc.stdout[-2000:]
    assert re.search(r"^Error: --langevin(Damp|Temp)", proc.stdout, flags=re.M), proc.stdout[-2000:]


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_langevin_entries_are_exported_and_declared(sfx):
    syms = {}
    for lib in ("hip", "host"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_{lib}{sfx}.so")], capture_output=True, text=True).stdout
        syms[lib] = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"advanceVelocityPositionLangevinGpu", "advanceVelocityVelocityPositionLangevinGpu"} <= syms["hip"]
    assert {"comdSetLangevin", "comdGetLangevin", "comdStepCount"} <= syms["host"]
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void advanceVelocityPositionLangevinGpu\(SimGpu\* sim, real_t dtKick, real_t dtHalfDrift, real_t c1, real_t c2, real_t kT, "
                     r"uint64_t seed, uint64_t step\);", header, flags=re.M)
    assert re.search(r"^void advanceVelocityVelocityPositionLangevinGpu\(SimGpu\* sim, real_t dtKick1, real_t dtKick2, real_t dtHalfDrift, "
                     r"real_t c1, real_t c2, real_t kT,\s+uint64_t seed, uint64_t step\);", header, flags=re.M)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_langevin_kernels_use_no_scratch(precision):
    blocks = device_isa.blocks(precision, r"AdvanceVelocity\w*Langevin\w*")
    assert len(blocks) == 2 and any("VelocityVelocity" in n for n in blocks), sorted(blocks)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name


# ---------------------------------------------------------------- GPU helpers
def _mass(p, ek):
    """the (single) species mass from the momenta and the kinetic energy the device reduced: sum p^2 / 2 eK"""
    return float((p * p).sum() / (2.0 * ek))


def _state(sim):
    return sim.gather(0).copy(), sim.gather(1).copy(), sim.gather(2).copy()


# ---------------------------------------------------------------- GPU: exact restatement of a step
@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
@pytest.mark.parametrize("steps", [1, 3])
def test_step_matches_the_numpy_restatement(gpu, pot, steps):
    """B A O A [force] B of global step `steps` - 1 from the gathered state before it and the forces after it, in numpy with the restated noise.
    steps = 1: the first-step kernel (B A O A); steps = 3: the between-steps kernel (B B A O A), against the state after step(2) of a second
    simulation (step(2); step(1) is bit-identical to step(3), checked in test_runs_are_reproducible).  dt = 2 fs: c1, c2 come from the call."""
    T, tau, dt, n = 300.0, 50.0, 2.0, SMALL[pot]
    args = _cube(n) + ["-r", 0.1, "-l", LAT] + POT[pot]
    with gpu.Simulation(args) as sim:
        sim.set_langevin(T, tau, SEED)
        if steps > 1:
            sim.step(steps - 1, dt)
        r0, p0, f0 = _state(sim)
        m = _mass(p0, sim.energy()[1])
        assert sim.step_count == steps - 1
    with gpu.Simulation(args) as sim:
        sim.set_langevin(T, tau, SEED)
        sim.step(steps, dt)
        r1, p1, f1 = _state(sim)
        assert sim.step_count == steps
    h = 0.5 * dt
    c1 = np.exp(-dt / tau)
    c2 = np.sqrt(1.0 - c1 * c1)
    xi = normals(SEED, np.arange(len(r0)), steps - 1)
    pb = p0 + h * f0
    ra = r0 + h * pb / m
    po = c1 * pb + c2 * np.sqrt(m * KB * T) * xi
    r_want = ra + h * po / m
    p_want = po + h * f1
    box = n * LAT
    assert np.abs(_wrap(r1 - r_want, box)).max() <= 1e-12 * np.abs(r_want).max()
    assert _rel(p1, p_want) <= 1e-12
    # the noise is a real part of the step: without it the momenta would be off by far more than the tolerance
    assert _rel(p1, c1 * pb + h * f1) > 1e-3


# ---------------------------------------------------------------- GPU: free particles
@pytest.mark.gpu
def test_free_particles_at_zero_kelvin_decay_geometrically(gpu):
    """-l 20: nearest neighbours at 14.1 A, beyond the 5 sigma = 11.6 A cutoff, so every force is exactly 0 (asserted) and BAOAB at target 0 K
    is p_n = c1^n p_0 (the noise term is c2 sqrt(m * 0) xi = 0 exactly)."""
    tau = 40.0
    with gpu.Simulation(_cube(6) + ["-l", 20, "-T", 600]) as sim:
        p0 = sim.gather(1).copy()
        sim.set_langevin(0.0, tau)
        for n in (1, 10, 50, 100):
            sim.step(n - sim.step_count)
            p, f = sim.gather(1), sim.gather(2)
            assert not f.any() and sim.energy()[0] == 0.0, (n, np.abs(f).max(), sim.energy())
            assert _rel(p, np.exp(-n / tau) * p0) <= 1e-12, (n, _rel(p, np.exp(-n / tau) * p0))


@pytest.mark.gpu
def test_free_particles_relax_to_the_target(gpu):
    """Per component, E[p_n^2/m | p_0] = c1^2n p_0^2/m + (1 - c1^2n) kT; the mean over the M = 3N components of one run has variance
    sum_i [4 c1^2n (p_0i^2/m)(1 - c1^2n) kT + 2 (1 - c1^2n)^2 (kT)^2] / M^2 (p_n = c1^n p_0 + sqrt(1 - c1^2n) sqrt(m kT) g, g ~ N(0,1)).
    Bound: 5 sigma at each checked n."""
    T, tau = 300.0, 50.0
    kT = KB * T
    with gpu.Simulation(_cube(6) + ["-l", 20, "-T", 100]) as sim:
        p0 = sim.gather(1).copy()
        m = _mass(p0, sim.energy()[1])
        q0 = (p0 * p0 / m).ravel()
        sim.set_langevin(T, tau, SEED)
        for n in (10, 25, 50, 100, 200):
            sim.step(n - sim.step_count)
            p, f = sim.gather(1), sim.gather(2)
            assert not f.any()
            a = np.exp(-2.0 * n / tau)
            want = a * q0.mean() + (1.0 - a) * kT
            sigma = np.sqrt((4.0 * a * q0 * (1.0 - a) * kT + 2.0 * (1.0 - a) ** 2 * kT ** 2).sum()) / q0.size
            got = (p * p / m).mean()
            assert abs(got - want) <= 5.0 * sigma, (n, got / KB, want / KB, sigma / KB)


@pytest.mark.gpu
def test_free_particles_have_the_ideal_gas_pressure(gpu):
    """Simulation.pressure() of thermostatted free particles averages to N kB T / V (W = 0 exactly).  -l 30 keeps every pair > 9.6 A outside the
    cutoff over the whole run (rms displacement < 3 A, forces asserted 0), while atoms do move between link cells (asserted from the
    positions).  Samples 100 steps = 4 tau apart (autocorrelation of p^2 e^-8): tr K / 3 of one sample has sigma = N kT sqrt(2 / 3N); bound
    5 sigma / sqrt(samples)."""
    T, tau, samples = 300.0, 25.0, 40
    with gpu.Simulation(_cube(6) + ["-l", 30, "-T", T]) as sim:
        r0 = sim.gather(0).copy()
        sim.set_langevin(T, tau, SEED)
        sim.step(200)
        ps = []
        for _ in range(samples):
            sim.step(100)
            w, _ = sim.virial()
            assert not w.any()
            ps.append(sim.pressure())
        assert not sim.gather(2).any()
        nat = sim.n_global
        cell = 180.0 / sim.grid[0]
        assert (np.floor(np.mod(sim.gather(0), 180.0) / cell) != np.floor(np.mod(r0, 180.0) / cell)).any()
    v = (6 * 30.0) ** 3
    want = nat * KB * T / v
    sigma = want * np.sqrt(2.0 / (3.0 * nat)) / np.sqrt(samples)
    assert abs(np.mean(ps) - want) <= 5.0 * sigma, (np.mean(ps), want, sigma)


# ---------------------------------------------------------------- GPU: temperature control
def _thermalise(sim, T, tau, equil, window, every=10, snap_every=200):
    """equil steps, then `window` steps: the kinetic temperature every `every` steps and p / sqrt(m kT) every `snap_every` steps"""
    nat = sim.n_global
    p = sim.gather(1)
    sim.set_langevin(T, tau, SEED)
    sim.step(equil)
    temps, z = [], []
    m = None
    for i in range(window // every):
        sim.step(every)
        ek = sim.energy()[1]
        temps.append(ek / nat / (1.5 * KB))
        if (i + 1) * every % snap_every == 0:
            p = sim.gather(1).copy()
            m = m or _mass(p, ek)
            z.append((p / np.sqrt(m * KB * T)).ravel())
    return np.array(temps), np.concatenate(z)


def _check_thermal(temps, z, T, tau, window, nat):
    """Mean kinetic temperature: one sample's sigma is T sqrt(2 / 3N) (canonical kinetic-energy fluctuation); its integrated autocorrelation
    time is at most tau (the energy part relaxes at 1/tau, half of the variance; the kinetic-potential exchange part decorrelates at phonon
    times), so the window holds at least window / 2 tau independent samples: bound 5 sigma / sqrt(window / 2 tau).  Pooled z = p / sqrt(m kT)
    of snapshots 4 tau apart (p autocorrelation e^-4): mean, variance and excess kurtosis within 5 sigma of N(0,1) for M samples
    (1 / sqrt M, sqrt(2 / M), sqrt(24 / M)); the O(dt^2) kinetic bias of BAOAB (< 1e-3 at the Cu phonon band) is well inside."""
    sigma_t = T * np.sqrt(2.0 / (3.0 * nat)) / np.sqrt(window / (2.0 * tau))
    assert abs(temps.mean() - T) <= 5.0 * sigma_t, (temps.mean(), T, sigma_t)
    M = z.size
    assert abs(z.mean()) <= 5.0 / np.sqrt(M), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / M), z.var()
    assert abs(((z - z.mean()) ** 4).mean() / z.var() ** 2 - 3.0) <= 5.0 * np.sqrt(24.0 / M)


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
@pytest.mark.parametrize("T0", [0, 600])
def test_temperature_control(gpu, pot, T0):
    """Heat from 0 K and cool from 600 K to 300 K with tau = 50 fs, 8^3 cells: after 20 tau, the mean over 2000 steps is the target."""
    T, tau, window = 300.0, 50.0, 2000
    with gpu.Simulation(_cube(8) + ["-T", T0, "-l", LAT] + POT[pot]) as sim:
        temps, z = _thermalise(sim, T, tau, int(20 * tau), window)
        _check_thermal(temps, z, T, tau, window, sim.n_global)


@pytest.mark.gpu
def test_configurational_equipartition(gpu):
    """LJ crystal at 20 K (kT / epsilon = 0.01): <U> - U_lattice = (3N - 3)/2 kB T, the harmonic value (the centre of mass is free).  U of the
    harmonic crystal fluctuates by kT sqrt((3N - 3)/2); its autocorrelation time is at most tau as for the kinetic energy, so the statistical
    sigma of the mean excess is sqrt(2 / (3N - 3)) / sqrt(window / 2 tau) of it: bound 5 sigma + 2 % for the first anharmonic correction,
    which at kT / epsilon = 0.01 is of order 1 %.  This checks the positions the thermostat samples, not only the momenta."""
    T, tau, window, n = 20.0, 50.0, 4000, 8
    with gpu.Simulation(_cube(n) + ["-T", 0, "-l", LAT]) as sim:
        u0 = sim.energy()[0]
        nat = sim.n_global
        sim.set_langevin(T, tau, SEED)
        sim.step(int(20 * tau))
        us = []
        for _ in range(window // 10):
            sim.step(10)
            us.append(sim.energy()[0])
    want = (3 * nat - 3) / 2.0 * KB * T
    rel = (np.mean(us) - u0) / want - 1.0
    sigma = np.sqrt(2.0 / (3 * nat - 3)) / np.sqrt(window / (2.0 * tau))
    assert abs(rel) <= 5.0 * sigma + 0.02, (rel, sigma)


# ---------------------------------------------------------------- GPU: reproducibility
@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
def test_runs_are_reproducible(gpu, pot):
    """Same seed: the same bits.  Another seed: another trajectory.  step(10); step(10) is step(20) to the bit.  Switched off mid-run, the
    simulation continues as NVE: the total energy per atom is conserved over 20 steps to the bound of the NVE checks (5e-6 relative),
    while the thermostat, left on, moves it by far more."""
    args = _cube(SMALL[pot]) + ["-r", 0.1, "-T", 0, "-l", LAT] + POT[pot]

    def run(chunks, seed=SEED):
        with gpu.Simulation(args) as sim:
            sim.set_langevin(600.0, 20.0, seed)
            for c in chunks:
                sim.step(c)
            assert sim.step_count == sum(chunks)
            return _state(sim)

    a, b, c, d = run([20]), run([20]), run([10, 10]), run([20], seed=SEED + 1)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert _rel(d[1], a[1]) > 1e-2

    with gpu.Simulation(args) as sim:
        sim.set_langevin(600.0, 20.0, SEED)
        sim.step(40)
        e0 = sum(sim.energy()[:2])
        nat = sim.n_global
        sim.set_langevin(600.0, 20.0, on=False)
        assert sim.langevin()["on"] is False
        sim.step(20)
        e1 = sum(sim.energy()[:2])
        assert abs(e1 - e0) / nat < 5e-6 * abs(e0) / nat, (e0, e1)
        sim.set_langevin(600.0, 20.0)
        sim.step(20)
        e2 = sum(sim.energy()[:2])
        assert abs(e2 - e1) > 100 * 5e-6 * abs(e1)


# ---------------------------------------------------------------- GPU: methods, layouts, ranks
LAYOUTS = [("thread_atom", []), ("cta_cell", []), ("thread_atom_nl", []), ("thread_atom", ["-H"]), ("thread_atom", ["-a", 1]),
           ("cta_cell", ["-a", 1])]


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj", 12), ("eam", 10)])
def test_methods_and_layouts_agree(gpu, pot, n):
    """20 thermostatted steps under every method, cell numbering and stream mode: positions (modulo the box) and momenta agree at the tolerance
    of test_neighbor_list_trajectory_agrees (100 x the one-evaluation force bound) -- the noise depends on (seed, gid, step) only."""
    base = _cube(n) + ["-r", 0.1, "-l", LAT] + POT[pot]
    got = {}
    for method, extra in LAYOUTS:
        with gpu.Simulation(base + ["-m", method] + extra) as sim:
            sim.set_langevin(300.0, 20.0, SEED)
            sim.step(20)
            got[" ".join([method] + [str(x) for x in extra])] = _state(sim)[:2]
    r0, p0 = got["thread_atom"]
    tol = 100 * TOL["force_rel_to_max"]
    for name, (r, p) in got.items():
        assert np.abs(_wrap(r - r0, n * LAT)).max() <= tol * np.abs(r0).max(), name
        assert _rel(p, p0) <= tol, name


def _ranks(grid, args, settings, tmp_path, timeout=300):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "langevin_worker.py"), str(r), str(world), port, *map(str, grid),
                               json.dumps(args), json.dumps(settings), str(tmp_path / f"rank{r}.npz")],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r in range(world)]
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
    return [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj", 14), ("eam", 8)])
def test_ranks_give_the_one_rank_trajectory(gpu, pot, n, tmp_path):
    """2 ranks (2x1x1) sharing the device over gloo: 20 thermostatted steps give the one-rank positions and momenta (every atom on exactly
    one rank), at the tolerance of test_methods_and_layouts_agree."""
    args = _cube(n) + ["-r", 0.1, "-l", LAT] + POT[pot]
    settings = [300.0, 20.0, SEED, 20]
    with gpu.Simulation(args) as sim:
        sim.set_langevin(*settings[:3])
        sim.step(settings[3])
        r0, p0 = _state(sim)[:2]
    parts = _ranks((2, 1, 1), args, settings, tmp_path)
    assert all(int(s["step"]) == settings[3] for s in parts)
    r, p = sum(s["r"] for s in parts), sum(s["p"] for s in parts)
    owned = sum((np.abs(s["p"]).sum(1) > 0).astype(int) for s in parts)
    assert np.all(owned == 1)
    tol = 100 * TOL["force_rel_to_max"]
    assert np.abs(_wrap(r - r0, n * LAT)).max() <= tol * np.abs(r0).max()
    assert _rel(p, p0) <= tol


# ---------------------------------------------------------------- GPU: single precision, CLI
@pytest.mark.gpu
def test_single_precision_temperature_control():
    """test_temperature_control (LJ, heating and cooling) in the float build (COMD_PRECISION=single, lib*_sp.so): float noise, same bounds."""
    env = dict(os.environ, COMD_PRECISION="single")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(HERE, "test_langevin.py"),
           "-k", "test_temperature_control and lj and not single"]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-2000:]
    assert "2 passed" in proc.stdout, proc.stdout[-1000:]


def _comd_hip(tmp_path, extra):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-x", "8", "-y", "8", "-z", "8", "-N", "200", "-n", "20", "-d", os.path.join(ROOT, "pots")]
                          + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+\d+\.\d+\s+\S+\s+\S+\s+\S+\s+(\S+)\s+\S+\s+(\d+)$", proc.stdout, flags=re.M)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    assert len(yaml) == 1
    text = (tmp_path / yaml[0]).read_text()
    os.remove(tmp_path / yaml[0])
    return proc.stdout, [(int(s), float(t)) for s, t, _ in rows], text


def _flags(*args):
    return [str(a) for a in args]


@pytest.mark.gpu
def test_comd_hip_langevin(gpu, tmp_path):
    """comd-hip --langevin --langevinTemp 300 -T 0, 8^3, tau = 20 fs: from step 100 (5 tau) on, every printed Temperature is within 5 sigma of
    300 K (one sample's sigma T sqrt(2 / 3N) = 5.4 K); the settings are in the YAML and on stdout.  Without --langevin: no thermostat lines."""
    out, rows, yaml = _comd_hip(tmp_path, _flags("--langevin", "--langevinTemp", 300, "-T", 0, "--langevinDamp", 20, "--seed", 99))
    assert [s for s, _ in rows] == list(range(0, 220, 20))
    assert rows[0][1] == 0.0
    sigma = 300.0 * np.sqrt(2.0 / (3.0 * 4 * 8 ** 3))
    assert all(abs(t - 300.0) <= 5.0 * sigma for s, t in rows if s >= 100), rows
    for text in (out, yaml):
        assert "Langevin thermostat: 1" in text and "Langevin temperature: 300 K" in text
        assert "Langevin damping: 20 fs" in text and "Langevin seed: 99" in text
    out0, rows0, yaml0 = _comd_hip(tmp_path, _flags("-T", 0))
    assert "Langevin" not in out0 and "Langevin" not in yaml0
    assert all(t < 30.0 for _, t in rows0)            # NVE from the lattice at 0 K: only the -r 0 round-off to heat it
