"""The static structure factor and the Bragg order (not in the reference): computeStructureFactor / comdStructureFactor / comdStructureFactorRadial /
comdBraggOrder, Simulation.structure_factor / structure_factor_radial / bragg_order, comd-hip --sk.

CPU: flags and refusals, exports, the kernel descriptors, the powder average against a numpy restatement.  GPU: the density amplitudes against numpy on the
gathered positions and the current box.

The reference: rho_ref(h, k, l) = sum_j exp(-2 pi i sum_a frac(s_a m_a u_a)), u = r / L and the fractions in float64; the three exponentials per atom and the sum
over the atoms are taken in extended precision, so that the reference's own rounding (a few float64 eps per atom otherwise, the size of the double build's
budget) is out of the picture.

The bound, per component: |rho - rho_ref| <= N eps(real_t) (16 + 2 pi Hmax), Hmax the largest |stride index| of the grid: the two roundings of u and of
(s m) u, at most 2 pi Hmax eps / 2 each, and 16 eps for the rounding of the tables, two complex products, the rotation and the sum.  It is a condition too: every
test asserts that its bound stays below 0.05, so that one atom missed, doubled or given a wrong phase (|d rho| up to 1) fails.  Every test prints its largest
error over N eps.  Measured on the MI355X: 0.2 to 3.0 N eps in the double build (5.9 with COMD_SK_CHUNKS=1, one chain of additions over all atoms of a grid
point; 3 between two and eight ranks and one) against bounds of 22 to 167 N eps, and 0.14 to 0.38 N eps in the float build.
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

from test_pressure import CSRC, HERE, POT, ROOT, SINGLE, _child, _cube

REAL = np.float32 if SINGLE else np.float64
EPS = float(np.finfo(REAL).eps)
EPS32 = float(np.finfo(np.float32).eps)
FLAGS = ("sk", "skStride", "skBins", "skStart", "skFile")
TWO_PI_LONG = np.longdouble(8) * np.arctan(np.longdouble(1))      # 2 pi in extended precision (np.pi is the float64)
EXE = os.path.join(CSRC, "comd-hip-sp" if SINGLE else "comd-hip")


def _index(m):
    h, k, l = np.meshgrid(np.arange(m + 1), np.arange(-m, m + 1), np.arange(-m, m + 1), indexing="ij")
    return np.stack([h.ravel(), k.ravel(), l.ravel()], axis=1)


def _strides(stride):
    return np.broadcast_to(np.asarray(stride, dtype=np.int64), (3,))


def _reference(pos, box, m, stride):
    """complex128 (K,): rho_ref on the half grid, separable per atom as the sum itself is"""
    u = np.asarray(pos, dtype=np.float64) / np.asarray(box, dtype=np.float64)[None, :]
    st = _strides(stride)
    tables = []
    for a, idx in enumerate((np.arange(m + 1), np.arange(-m, m + 1), np.arange(-m, m + 1))):
        x = (st[a] * idx).astype(np.float64)[None, :] * u[:, a][:, None]      # the integer product exact, one rounding
        f = (x - np.floor(x)).astype(np.longdouble)
        tables.append(np.exp(-1j * TWO_PI_LONG * f))
    ex, ey, ez = tables
    w = 2 * m + 1
    yz = (ey[:, :, None] * ez[:, None, :]).reshape(len(u), w * w)
    return (ex.T @ yz).astype(np.complex128).ravel()


def _bound(n, m, stride, eps=EPS):
    b = n * eps * (16.0 + 2.0 * np.pi * float(np.max(_strides(stride)) * m))
    assert b < 0.05, ("the bound must see a single atom", b)
    return b


def _worst(got, want):
    return float(max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()))


def _check(sim, m, stride, label=""):
    """structure_factor(m, stride) of the current state against numpy, within the bound; returns the result"""
    got = sim.structure_factor(m, stride)
    n, box = sim.n_global, sim.box
    w = 2 * m + 1
    assert got["shape"] == (m + 1, w, w) and got["rho"].shape == ((m + 1) * w * w,) and got["rho"].dtype == np.complex128
    assert got["index"].dtype == np.int32 and np.array_equal(got["index"], _index(m))
    assert np.array_equal(got["k"], 2.0 * np.pi * (_index(m) * _strides(stride)[None, :]) / box[None, :])
    assert np.array_equal(got["s"], (got["rho"].real ** 2 + got["rho"].imag ** 2) / n)
    bound = _bound(n, m, stride)
    err = _worst(got["rho"], _reference(sim.gather(0), box, m, stride))
    print(f"{label} M {m} stride {stride}: N {n}, max error {err / (n * EPS):.3f} N eps, bound {bound / (n * EPS):.1f} N eps")
    assert err <= bound, (label, m, stride, err, bound)
    assert got["rho"][m * w + m] == complex(n, 0.0)          # exactly N
    return got


# ---------------------------------------------------------------- CPU: flags, refusals, exports, descriptors
def test_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("s = pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '-N', 50, '--sk', 6, '--skStride', '2,3,4', '--skBins', 12, '--skStart', 10, '--skFile', 's.dat'], host_only=True);"
                  " print('made'); s.close()")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in FLAGS:
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


@pytest.mark.parametrize("extra,word", [(["--sk", 65], "--sk "), (["--sk", -1], "--sk "), (["--sk", 4, "--skStride", "0"], "skStride"), (["--sk", 4, "--skStride", "1,2"], "skStride"),
                                        (["--sk", 4, "--skStride", "2,x,2"], "skStride"), (["--sk", 64, "--skStride", "1025"], "skStride"),
                                        (["--sk", 4, "--skStride", "1,1,16385"], "skStride"), (["--sk", 4, "--skBins", 0], "skBins"), (["--sk", 4, "--skBins", 4097], "skBins"),
                                        (["--sk", 4, "--skStart", -1], "skStart"), (["--sk", 4, "--skStart", 101], "skStart")])
def test_each_refusal_is_one_error_line(extra, word):
    proc = _child(f"pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '-N', 100] + {extra!r}, host_only=True); print('made')")
    assert proc.returncode != 0 and "made" not in proc.stdout, proc.stdout[-2000:]
    lines = [l for l in (proc.stdout + proc.stderr).splitlines() if l.startswith("Error")]
    assert len(lines) == 1 and word in lines[0], (lines, proc.stdout[-2000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_symbols_are_exported_and_declared(sfx):
    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, lib)], capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "computeStructureFactor" in exported(f"libcomd_hip{sfx}.so")
    assert {"comdStructureFactor", "comdStructureFactorRadial", "comdBraggOrder"} <= exported(f"libcomd_host{sfx}.so")
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeStructureFactor\(SimGpu\* sim, int M, const int\* stride3, const double\* extent3, double\* outKx2\);", header, flags=re.M)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_kernels_use_no_scratch_and_64k_of_lds_at_most(precision):
    blocks = device_isa.blocks(precision, r"SK_\w+")
    assert {n for n in blocks if "SK_amplitudes" in n} and {n for n in blocks if "SK_sum" in n}, sorted(blocks)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
        assert re.search(r"\.amdhsa_group_segment_fixed_size 0\n", block), name          # dynamic LDS only: the launcher sizes it and refuses more than 64 KiB
        print(name, "VGPRs", re.search(r"\.amdhsa_next_free_vgpr (\d+)\n", block).group(1))
    device_isa.assert_keeps_waves(blocks, "SK_amplitudes", 4)


def test_lds_of_the_largest_grid_fits(pkg):
    """the launcher's sizing rule restated: a batch of atoms x (the h and |k| of the fullest tile + the l-blocks + 1) complex values + the batch's u, at every M;
    the batch is 64 atoms where that stays within 32 KiB and 32 atoms elsewhere"""
    lb = 8
    worst = 0
    for m in range(1, 65):
        w, n_lb = 2 * m + 1, -(-m // lb) + m // lb + 1
        items = (m + 1) * w * n_lb
        most = 0
        for tile in range(-(-items // 256)):
            p0, p1 = tile * 256 // n_lb, min(tile * 256 + 255, items - 1) // n_lb
            n_h = p1 // w - p0 // w + 1
            if n_h == 1:
                k0, k1 = p0 % w - m, p1 % w - m
                lo = 0 if k0 <= 0 <= k1 else min(abs(k0), abs(k1))
                n_k = max(abs(k0), abs(k1)) - lo + 1
            else:
                n_k = m + 1
            most = max(most, n_h + n_k)
        batch = 64 if 3 * 64 * 8 + 64 * (most + n_lb + 1) * 16 <= 32768 else 32
        worst = max(worst, 3 * batch * 8 + batch * (most + n_lb + 1) * 16)
    print("largest LDS request of the double build:", worst, "bytes")
    assert worst <= 65536


def test_bad_grids_are_value_errors_before_anything_is_launched(pkg):
    pkg.init_parallel(0, 1, None)
    with pkg.Simulation(_cube(8), host_only=True) as sim:
        for k_max, stride in ((0, 1), (65, 1), (-3, 1), (4, 0), (4, (1, 0, 1)), (4, -2), (64, 1025), (2, (1, 1, 32769)), (4, (1, 2)), (2.5, 1), (4, 1.5)):
            for call in (sim.structure_factor, sim.structure_factor_radial):
                with pytest.raises(ValueError):
                    call(k_max, stride)
        for bins in (0, 4097):
            with pytest.raises(ValueError):
                sim.structure_factor_radial(4, 1, bins)
        # a good grid: the host-only simulation has no device state
        for call in (sim.structure_factor, sim.structure_factor_radial, sim.bragg_order):
            with pytest.raises(RuntimeError):
                call()


# ---------------------------------------------------------------- CPU: the powder average
def _radial_restated(rho, m, stride, box, bins):
    idx, st, box = _index(m), _strides(stride), np.asarray(box, dtype=np.float64)
    w = 2 * m + 1
    n = rho[m * w + m].real
    kv = (6.283185307179586 * (idx * st[None, :]).astype(np.float64)) / box[None, :]
    kk = np.sqrt((kv[:, 0] * kv[:, 0] + kv[:, 1] * kv[:, 1]) + kv[:, 2] * kv[:, 2])
    k_top = float(np.min((6.283185307179586 * (st * m).astype(np.float64)) / box))
    dk = k_top / bins
    keep = (kk <= k_top) & np.any(idx != 0, axis=1)
    b = np.minimum(np.floor(kk / dk).astype(np.int64), bins - 1)
    weight = np.where(idx[:, 0] > 0, 2.0, 1.0)
    s = (rho.real ** 2 + rho.imag ** 2) / n
    sums, counts = np.zeros(bins), np.zeros(bins)
    np.add.at(sums, b[keep], (weight * s)[keep])
    np.add.at(counts, b[keep], weight[keep])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.arange(bins) + 0.5) * dk, np.where(counts > 0, sums / counts, np.nan), counts.astype(np.int64)


@pytest.mark.parametrize("m,stride,box,bins", [(4, 1, (28.92, 28.92, 28.92), 50), (6, (2, 3, 5), (28.92, 14.46, 21.69), 37), (9, (8, 4, 6), (30.1, 13.9, 22.4), 200),
                                               (1, 1, (10.0, 10.0, 10.0), 10), (3, (1, 1, 4), (12.0, 12.5, 13.0), 1), (64, 1, (300.0, 310.0, 290.0), 4096)])
def test_powder_average_is_the_restated_rule(pkg, m, stride, box, bins):
    rng = np.random.default_rng(1234 + m)
    w = 2 * m + 1
    rho = rng.normal(size=(m + 1) * w * w) * 30.0 + 1j * rng.normal(size=(m + 1) * w * w) * 30.0
    rho[m * w + m] = 864.0
    centres, s, counts = pkg.structure_factor_radial(rho, m, stride, box, bins)
    want_c, want_s, want_n = _radial_restated(rho, m, stride, box, bins)
    assert counts.dtype == np.int64 and np.array_equal(counts, want_n)
    assert np.all(np.abs(centres - want_c) <= 1e-12 * want_c)
    filled = want_n > 0
    assert filled.any() and np.all(np.isnan(s[~filled])) and np.all(np.abs(s[filled] - want_s[filled]) <= 1e-12 * np.abs(want_s[filled]))
    assert np.array_equal(pkg.structure_factor_radial(rho.reshape(m + 1, w, w), m, stride, box, bins)[2], counts)


def test_powder_average_weights_and_empty_bins(pkg):
    """M = 1 on a cube: the sphere |k| <= 2 pi / L holds the six axis vectors -- (1, 0, 0) twice for its mirror image, the four of the h = 0 plane once each -- in
    the last of ten bins; k = 0 is left out; the other bins are empty"""
    rho = np.zeros(2 * 3 * 3, dtype=np.complex128)
    shaped = rho.reshape(2, 3, 3)
    shaped[0, 1, 1] = 100.0                      # N
    shaped[1, 1, 1] = 30.0 + 40.0j               # (1, 0, 0): S = 25, weight 2
    shaped[0, 2, 1] = shaped[0, 0, 1] = 10.0j    # (0, +-1, 0): S = 1
    shaped[0, 1, 2] = shaped[0, 1, 0] = 20.0     # (0, 0, +-1): S = 4
    shaped[1, 2, 2] = 1000.0                     # (1, 1, 1): outside the sphere
    centres, s, counts = pkg.structure_factor_radial(rho, 1, 1, (10.0, 10.0, 10.0), 10)
    assert counts.tolist() == [0] * 9 + [6] and np.all(np.isnan(s[:9]))
    assert abs(s[9] - (2 * 25.0 + 2 * 1.0 + 2 * 4.0) / 6.0) <= 1e-12 * s[9]
    assert np.allclose(centres, (np.arange(10) + 0.5) * (2.0 * np.pi / 10.0) / 10, rtol=1e-14)
    # a flat box: only the short reciprocal axis... the long real axis has the short vector
    _, _, counts = pkg.structure_factor_radial(rho, 1, 1, (10.0, 20.0, 20.0), 1)
    assert counts.tolist() == [4]                # k_top = 2 pi / 20: (0, +-1, 0) and (0, 0, +-1)
    for bad in (dict(box=(10.0, 0.0, 10.0)), dict(box=(10.0, -1.0, 10.0)), dict(n_bins=0), dict(n_bins=4097), dict(k_max=2)):
        kw = dict(rho=rho, k_max=1, stride=1, box=(10.0, 10.0, 10.0), n_bins=10)
        kw.update(bad)
        with pytest.raises(ValueError):
            pkg.structure_factor_radial(**kw)
    rho[1 * 3 + 1] = 0.0
    with pytest.raises(ValueError):              # N = Re rho(0, 0, 0) must be positive
        pkg.structure_factor_radial(rho, 1, 1, (10.0, 10.0, 10.0), 10)


# ---------------------------------------------------------------- GPU: the perfect lattice
@pytest.mark.gpu
def test_perfect_lattice_has_the_fcc_reflections(gpu):
    with gpu.Simulation(_cube(4) + POT["adams"]) as sim:
        n = sim.n_global
        assert n == 256
        got = _check(sim, 2, 4, "adams 4^3 lattice")
        bound = _bound(n, 2, 4)
        idx, mod = got["index"], np.abs(got["rho"])
        fcc = np.all(idx % 2 == 0, axis=1) | np.all(idx % 2 != 0, axis=1)
        print("| |rho| - N | on the reflections:", np.abs(mod[fcc] - n).max() / (n * EPS), "N eps; |rho| elsewhere:", mod[~fcc].max() / (n * EPS), "N eps")
        assert fcc.sum() > 1 and np.all(np.abs(mod[fcc] - n) <= bound) and np.all(mod[~fcc] <= bound)
        assert got["rho"][2 * 5 + 2].real == float(n) and got["rho"][2 * 5 + 2].imag == 0.0
        bragg = sim.bragg_order()
        print("bragg order - 1:", bragg - 1.0, "bound / N", _bound(n, 1, 4) / n)
        assert abs(bragg - 1.0) <= _bound(n, 1, 4) / n
        # stride 1: the box's own reciprocal lattice; the crystal's is every 4th point of it
        got = _check(sim, 4, 1, "adams 4^3 lattice")
        idx, mod = got["index"], np.abs(got["rho"])
        on = np.all(idx % 4 == 0, axis=1)
        assert np.all(mod[~on] <= _bound(n, 4, 1))
        cell = idx[on] // 4
        fcc = np.all(cell % 2 == 0, axis=1) | np.all(cell % 2 != 0, axis=1)
        assert np.all(np.abs(mod[on][fcc] - n) <= _bound(n, 4, 1)) and np.all(mod[on][~fcc] <= _bound(n, 4, 1)) and fcc.sum() == 5


# ---------------------------------------------------------------- GPU: against numpy
GRIDS = [(1, 1), (3, 1), (9, 1), (4, (2, 3, 5)), (3, (8, 8, 8))]
STATES = {"lj5_thread_atom": _cube(8) + ["-m", "thread_atom"], "lj5_cta_cell": _cube(8) + ["-m", "cta_cell"], "lj2.5": _cube(8) + POT["lj2.5"],
          "adams": _cube(6) + POT["adams"], "mishin": _cube(6) + POT["mishin"], "lj2.5_flat_box": ["-x", 8, "-y", 4, "-z", 6] + POT["lj2.5"]}


@pytest.mark.gpu
@pytest.mark.parametrize("state", sorted(STATES))
def test_amplitudes_against_numpy(gpu, state):
    with gpu.Simulation(STATES[state] + ["-r", 0.1]) as sim:
        assert sim.n_global <= 2048
        for steps in (0, 10):
            if steps:
                sim.step(steps)
            for m, stride in GRIDS:
                _check(sim, m, stride, f"{state} step {steps}")


@pytest.mark.gpu
def test_many_tiles_on_every_axis(gpu):
    """M = 17: K = 22 050 vectors, 5 l-blocks, tiles that span several h and tiles inside one h"""
    with gpu.Simulation(_cube(4) + POT["adams"] + ["-r", 0.1]) as sim:
        got = _check(sim, 17, 1, "adams 4^3")
        assert got["rho"].shape == (22050,)


@pytest.mark.gpu
def test_positions_outside_the_box_need_no_wrap(gpu):
    with gpu.Simulation(_cube(8) + POT["adams"] + ["-m", "thread_atom_nl", "-S", 0.1, "-T", 3000]) as sim:
        sim.step(20)
        pos, box = sim.gather(0), sim.box
        print("atoms outside [0, L):", int(np.any((pos < 0.0) | (pos >= box[None, :]), axis=1).sum()))
        for m, stride in ((9, 1), (3, (8, 8, 8))):
            _check(sim, m, stride, "adams 8^3 thread_atom_nl")
        # whatever the run left inside: periodic images of some atoms, written into their slots as they are
        before = sim.structure_factor(9, 1)["rho"]
        pos[::7, 0] -= box[0]
        pos[::5, 1] += box[1]
        pos[::3, 2] += 2.0 * box[2]
        sim.scatter(0, pos)
        pos = sim.gather(0)
        outside = int(np.any((pos < 0.0) | (pos >= box[None, :]), axis=1).sum())
        print("atoms outside [0, L) after the shift:", outside)
        assert outside > 1000
        for m, stride in ((9, 1), (3, (8, 8, 8))):
            got = _check(sim, m, stride, "adams 8^3 thread_atom_nl, images")
        assert _worst(sim.structure_factor(9, 1)["rho"], before) <= 2.0 * _bound(sim.n_global, 9, 1)


# ---------------------------------------------------------------- GPU: chunks, determinism, symmetry, box, purity
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 3, 1000000])
def test_chunk_counts_and_bitwise_repeatability(gpu, monkeypatch, chunks):
    monkeypatch.setenv("COMD_SK_CHUNKS", str(chunks))      # read when the simulation is created
    runs = []
    for _ in range(2):
        with gpu.Simulation(STATES["adams"] + ["-r", 0.1]) as sim:
            assert chunks < sim.n_local_boxes or chunks == 1000000
            runs.append(_check(sim, 9, 1, f"adams 6^3, {chunks} chunks")["rho"])
            assert np.array_equal(sim.structure_factor(9, 1)["rho"], runs[-1])
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.gpu
def test_zero_plane_is_hermitian(gpu):
    with gpu.Simulation(STATES["lj2.5"] + ["-r", 0.1]) as sim:
        got = _check(sim, 9, 1, "lj2.5 8^3")
        plane = got["rho"].reshape(got["shape"])[0]
        err = _worst(plane, np.conj(plane[::-1, ::-1]))
        print("h = 0 plane against its mirror image:", err / (sim.n_global * EPS), "N eps")
        assert err <= 2.0 * _bound(sim.n_global, 9, 1)


@pytest.mark.gpu
def test_wave_vectors_follow_a_deformed_box(gpu):
    with gpu.Simulation(STATES["adams"] + ["-r", 0.1]) as sim:
        before, box0 = sim.structure_factor(3, 6), sim.box
        sim.set_box(box0 * np.array([1.03, 0.98, 1.01]))
        assert not np.array_equal(sim.box, box0)
        got = _check(sim, 3, 6, "adams 6^3 deformed")          # k and the reference on the new sim.box
        assert not np.array_equal(got["k"], before["k"])
        # the indices follow the box: an affine remap leaves the amplitudes where they were, to the rounding of the remap
        print("amplitudes after the affine remap:", _worst(got["rho"], before["rho"]) / (sim.n_global * EPS), "N eps from before")
    # the perfect crystal keeps its Bragg order under strain: S / N = (|rho| / N)^2 doubles the relative error, and the remap rounds every position once more,
    # by no more than the two roundings of u in the bound together
    with gpu.Simulation(_cube(6) + POT["adams"]) as sim:
        sim.set_box(sim.box * np.array([1.03, 0.98, 1.01]))
        print("bragg order - 1 on the strained lattice:", sim.bragg_order() - 1.0)
        assert abs(sim.bragg_order() - 1.0) <= 4.0 * _bound(sim.n_global, 1, 6) / sim.n_global


def _same_cells(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["lj2.5", "adams"])
def test_calls_change_nothing(gpu, state):
    args = STATES[state] + ["-r", 0.1]
    with gpu.Simulation(args) as sim:
        cells, energy = sim.cells(), sim.energy()
        sim.structure_factor(9, 1), sim.structure_factor(2, (6, 6, 6)), sim.bragg_order(), sim.structure_factor_radial(4, 1, 20)
        assert _same_cells(cells, sim.cells()) and energy == sim.energy()
        for _ in range(5):
            sim.step(1)
            sim.structure_factor(3, 2), sim.bragg_order()
        with_calls = (sim.cells(), sim.energy())
    with gpu.Simulation(args) as sim:
        for _ in range(5):
            sim.step(1)
        assert _same_cells(with_calls[0], sim.cells()) and with_calls[1] == sim.energy()


# ---------------------------------------------------------------- GPU: ranks
def _ranks(grid, m, stride, args, timeout=900):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "sk_worker.py"), str(r), str(world), port, *map(str, grid), str(m), json.dumps(stride), json.dumps(args)],
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
    found = [json.loads(re.search(r"^SK (.*)$", out, flags=re.M).group(1)) for out in outs]
    return [(np.array([float.fromhex(v) for v in re_]) + 1j * np.array([float.fromhex(v) for v in im]), float.fromhex(bragg)) for re_, im, bragg in found]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_ranks_agree_with_one_rank(gpu, grid):
    args = _cube(8) + POT["adams"] + ["-r", 0.1]
    m, stride = 3, [8, 8, 8]
    with gpu.Simulation(args) as sim:
        one = _check(sim, m, tuple(stride), "adams 8^3, one rank")["rho"]
        n, bragg = sim.n_global, sim.bragg_order()
    got = _ranks(grid, m, stride, args)
    for rho, b in got:
        assert np.array_equal(rho, got[0][0]) and b == got[0][1]
    err = _worst(got[0][0], one)
    print(f"{grid} ranks against one rank:", err / (n * EPS), "N eps")
    assert err <= 2.0 * _bound(n, m, stride) and abs(got[0][1] - bragg) <= 2.0 * _bound(n, 1, 8) / n


# ---------------------------------------------------------------- GPU: the float build
SINGLE_RUN = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    sim.step(5)
    a, b = sim.structure_factor(9, 1), sim.structure_factor(3, (8, 8, 8))
    np.savez({path!r}, pos=sim.gather(0), box=sim.box, a=a["rho"], b=b["rho"], bragg=sim.bragg_order())
    sim.close()
    print("saved")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 8), ("adams", 6)])
def test_single_precision(gpu, tmp_path, pot, n):
    """The float build (COMD_PRECISION=single) against numpy on its own gathered positions, with the float's eps in the bound"""
    path = str(tmp_path / "sp.npz")
    proc = _child(SINGLE_RUN.format(args=_cube(n) + ["-r", 0.1] + POT[pot], path=path), env={"COMD_PRECISION": "single"})
    assert proc.returncode == 0 and "saved" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = np.load(path)
    atoms = len(got["pos"])
    assert atoms == 4 * n ** 3
    for key, m, stride in (("a", 9, 1), ("b", 3, (8, 8, 8))):
        bound = _bound(atoms, m, stride, EPS32)
        err = _worst(got[key], _reference(got["pos"], got["box"], m, stride))
        print(f"float build, {pot} {n}^3 M {m} stride {stride}: max error {err / (atoms * EPS32):.3f} N eps32, bound {bound / (atoms * EPS32):.1f}")
        assert err <= bound
        w = 2 * m + 1
        assert got[key][m * w + m] == complex(atoms, 0.0)
    assert 0.0 < float(got["bragg"]) < 1.0


# ---------------------------------------------------------------- GPU: the executable
def _comd_hip(tmp_path, extra):
    proc = subprocess.run([EXE, "-d", os.path.join(ROOT, "pots")] + [str(a) for a in extra], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    assert len(yaml) == 1
    text = (tmp_path / yaml[0]).read_text()
    os.remove(tmp_path / yaml[0])
    return proc.stdout, rows, text


def _sk_file(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#") and not any(line.startswith("#") for line in lines[1:])
    return lines[0], np.array([[float(x) for x in line.split()] for line in lines[1:]])


def _block(yaml):
    block = re.search(r"^StructureFactor:\n((?:  .*\n)+)", yaml, flags=re.M)
    assert block, yaml[-2000:]
    return dict(re.findall(r"^  (\w+): (.+)$", block.group(1), flags=re.M))


@pytest.mark.gpu
def test_comd_hip_sk_of_the_initial_state(gpu, tmp_path):
    out, rows, yaml = _comd_hip(tmp_path, ["-N", 0, "--sk", 4])
    header, table = _sk_file(tmp_path / "sk.dat")
    with gpu.Simulation(_cube(20)) as sim:
        centres, s, counts = sim.structure_factor_radial(4, 1, 50)
        n = sim.n_global
    assert re.search(rf"\bN {n} M 4 stride 1 1 1 bins 50 samples 1\b", header), header
    assert table.shape == (50, 3)
    assert np.all(np.abs(table[:, 0] - centres) <= 1e-12 * centres) and np.array_equal(table[:, 2], counts.astype(np.float64))
    filled = counts > 0
    assert filled.sum() > 10 and np.all(np.isnan(table[~filled, 1])) and np.all(np.abs(table[filled, 1] - s[filled]) <= 1e-12 * np.abs(s[filled]) + 1e-300)
    assert "S111/N" in out and [r[0] for r in rows] == ["0"] and float(rows[0][3].split()[-1]) == 1.0, out[-2000:]
    m = _block(yaml)
    assert float(m["braggFirst"]) == 1.0 and float(m["braggFinal"]) == 1.0 and float(m["braggMean"]) == 1.0


@pytest.mark.gpu
def test_comd_hip_sk_run(gpu, tmp_path):
    run = ["-x", 10, "-y", 10, "-z", 10, "-T", 3000, "-N", 20, "-n", 5]
    out0, rows0, yaml0 = _comd_hip(tmp_path, run)
    assert [r[0] for r in rows0] == ["0", "5", "10", "15", "20"]
    assert "S111/N" not in out0 and not re.search(r"^sk\s", out0, flags=re.M) and "StructureFactor" not in yaml0 and "Structure factor" not in yaml0 and not re.search(r"Timer:\s+sk", yaml0)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".dat")]
    # five samples: the energies untouched to the bit, the timer row, the YAML block
    out1, rows1, yaml1 = _comd_hip(tmp_path, run + ["--sk", 2, "--skStride", 10, "--skBins", 30, "--skFile", "x.dat"])
    assert [r[:3] for r in rows1] == [r[:3] for r in rows0] and all(r[3].strip() == "" for r in rows0)
    assert re.search(r"^sk\s+5\s", out1, flags=re.M), out1[-3000:]
    header, table = _sk_file(tmp_path / "x.dat")
    assert re.search(r"\bM 2 stride 10 10 10 bins 30 samples 5\b", header) and table.shape == (30, 3) and not os.path.exists(tmp_path / "sk.dat")
    m = _block(yaml1)
    assert set(m) == {"kMaxIndex", "stride", "bins", "samples", "file", "kOfHighestS", "braggFirst", "braggFinal", "braggMean"}, m
    assert m["kMaxIndex"] == "2" and m["stride"] == "[ 10, 10, 10 ]" and m["bins"] == "30" and m["samples"] == "5" and m["file"] == "x.dat"
    best = table[np.nanargmax(table[:, 1]), 0]
    assert abs(float(m["kOfHighestS"]) - best) <= 1e-9 * best
    column = [float(r[3].split()[-1]) for r in rows1]
    first, final, mean = float(m["braggFirst"]), float(m["braggFinal"]), float(m["braggMean"])
    print("S111/N of the printed steps:", column)
    assert 0.0 < final < first <= 1.0 and abs(column[0] - first) <= 1e-9 and abs(column[-1] - final) <= 1e-9 and abs(mean - np.mean(column)) <= 1e-9
    # --skStart 10: the column prints 0 before step 10, and three samples are taken
    out2, rows2, yaml2 = _comd_hip(tmp_path, run + ["--sk", 2, "--skStride", 10, "--skStart", 10])
    late = [float(r[3].split()[-1]) for r in rows2]
    assert late[:2] == [0.0, 0.0] and late[2:] == column[2:] and _block(yaml2)["samples"] == "3" and re.search(r"^sk\s+3\s", out2, flags=re.M)
    assert [r[:3] for r in rows2] == [r[:3] for r in rows0]
