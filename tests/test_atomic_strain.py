"""Per-atom strain and non-affine displacement (comdStrainReferenceGpu / computeAtomStrain / computeAtomStrainSummary, Simulation.set_strain_reference /
atomic_strain / shear_strain / volumetric_strain / strain_summary, comd-hip --strain).

CoMD computes no strain, so nothing here is compared with a recorded number.  The checks are physics with exact answers and restatement:
  * no motion, a homogeneous deformation of the box, a rigid translation across the periodic boundary, one displaced atom;
  * every atom's six components, D^2min and neighbour count against an all-pairs minimum-image fit in numpy, on states chosen so that every chunk class
    of hip/stencil_walk.h occurs (full chunks, replicated chunks of 2, 4, 8 and 16 copies, partial chunks, a 2-cell periodic box);
  * every method, layout, stream mode, rank count and both precisions give the same arrays; the device reduction gives numpy's figures.

Bounds.  With n_i neighbours, V_i = sum d0 d0^T of condition kappa(V_i), S_i = sum |d|^2 (all from the restatement):
  |dE_ab| <= C (n_i + 64) eps kappa(V_i) (1 + 2 max|E_i|)          |dD^2| <= C (n_i + 64) eps S_i
  eps = 2^-53 in the double build, 2^-24 (largest box extent / the atom's shortest neighbour distance) in the single build (the halo shift is applied to
  positions in real_t; the sums are in double).
No atom and no component is left out of a comparison.  C = 4 x the worst ratio err / (bound at C = 1) measured on the MI355X, rounded up to a power of two.
Measured on the MI355X, worst err / (bound at C = 1) over all atoms, states and both radii, E / D^2 (every test prints its own as a RATIO line):
  at the reference        0.18 / 0.068      homogeneous deformation   0.34 / 0.100      rigid translation   0.27 / 0.085      one displaced atom   0.079 / 0.064
  restatement             0.12 / 0.097      methods and layouts       0.047 / 0.064     2 and 8 ranks       0.15 / 0.108
  single build            0.0070 / 2.7e-5   (its eps carries the factor box / distance, about 12, for a rounding that mostly cancels in d)
The worst is 0.34 (the default radius on the 12 x 13 x 14 state, 12 neighbours): C = 4 x 0.34 = 1.4 -> 2.
"""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import device_isa
from test_atom_stress import CSRC, HEADER, HERE, LAT, ROOT, STATES, _child, _chunk_classes, _comd_hip, _extent
from test_pressure import EAM_METHODS, LJ_METHODS

EPS53, EPS24 = 2.0 ** -53, 2.0 ** -24
C_BOUND = 2.0             # 4 x the worst measured ratio, 0.34, rounded up to a power of two (the docstring has the figures)
MOVE = np.array([0.4, -0.3, 0.2])
SCALE = (1.02, 0.99, 1.0)
NAMES = ["A", "B", "C", "E", "F"]


def _default_rs(lat):
    return 0.5 * (np.sqrt(0.5) + 1.0) * lat


def _radii(sim):
    """the two radii of every test: the default (None to the calls) and the force cutoff as the simulation has it"""
    return {"default": None, "cutoff": sim.cutoff}


def _adjugate_fit(vm, am):
    """F = A adj(V) / det V for stacks of symmetric V and of A; det V too"""
    c = np.empty_like(vm)
    c[:, 0, 0] = vm[:, 1, 1] * vm[:, 2, 2] - vm[:, 1, 2] ** 2
    c[:, 1, 1] = vm[:, 0, 0] * vm[:, 2, 2] - vm[:, 0, 2] ** 2
    c[:, 2, 2] = vm[:, 0, 0] * vm[:, 1, 1] - vm[:, 0, 1] ** 2
    c[:, 0, 1] = c[:, 1, 0] = vm[:, 0, 2] * vm[:, 1, 2] - vm[:, 0, 1] * vm[:, 2, 2]
    c[:, 0, 2] = c[:, 2, 0] = vm[:, 0, 1] * vm[:, 1, 2] - vm[:, 0, 2] * vm[:, 1, 1]
    c[:, 1, 2] = c[:, 2, 1] = vm[:, 0, 1] * vm[:, 0, 2] - vm[:, 0, 0] * vm[:, 1, 2]
    det = vm[:, 0, 0] * c[:, 0, 0] + vm[:, 0, 1] * c[:, 0, 1] + vm[:, 0, 2] * c[:, 0, 2]
    return am @ c / np.where(det != 0.0, det, 1.0)[:, None, None], det


def _image_of_d0(d0, dd, box, box0, image):
    """the integer image per pair and axis that d0 = ref_j - ref_i is reduced by.  "nearest" (per axis; the kernel's): the image nearest the current separation
    mapped back to the reference box, rint((d0 - d box0 / box) / box0) -- the image the pair was accepted through.  "minimum": the shortest one, rint(d0 / box0),
    the rule before; another image where |d0| passes box0 / 2 on an axis, which takes a 2-cell axis and rs near the force cutoff.  A sequence of three names
    selects the rule per axis."""
    rules = (image,) * 3 if isinstance(image, str) else tuple(image)
    assert len(rules) == 3 and all(r in ("nearest", "minimum") for r in rules), image
    k = np.empty_like(d0)
    for a, rule in enumerate(rules):
        k[:, a] = np.rint(((d0[:, a] - dd[:, a] * box0[a] / box[a]) if rule == "nearest" else d0[:, a]) / box0[a])
    return k


def _restate(pos, box, ref, box0, rs, dtype=np.float64, block=256, image="nearest", image_rows=None):
    """The definitions of the issue, all pairs under the minimum image: for atom i the neighbours j with 0 < |d|^2 <= rs^2, d = x_j - x_i of the CURRENT
    positions formed in `dtype` (the periodic shift applied to x_j, as the halo copies carry it), d0 = ref_j - ref_i reduced in double to the image of box0
    that `image` selects per axis (_image_of_d0; default: the one nearest d mapped back to the reference box), V = sum d0 d0^T, A = sum d d0^T,
    F = A adj(V) / det V, E = 1/2 (F^T F - I), D^2 = sum |d - F d0|^2 (the direct form).  Invalid
    (n < 3 or det V <= 1e-9 (tr V / 3)^3): NaN.  Returns a dict with e, d2, n and what the bounds need: kappa, s, rmin, det_ratio.  image_rows: a list
    that receives arrays of rows (i, j, kx, ky, kz), the accepted ordered pairs with the integer images their d0 was reduced by."""
    n = len(pos)
    p = [np.ascontiguousarray(pos[:, a].astype(dtype)) for a in range(3)]
    lc = [dtype(box[a]) for a in range(3)]
    rs2 = dtype(rs) * dtype(rs)
    box, box0 = np.asarray(box, dtype=np.float64), np.asarray(box0, dtype=np.float64)

    def pairs(s0, m):
        d = []
        for a in range(3):
            da = p[a][None, :] - p[a][s0:s0 + m, None]
            k = np.rint(da / lc[a])
            d.append((p[a][None, :] - k * lc[a]) - p[a][s0:s0 + m, None])
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        ii, jj = np.nonzero((r2 > 0) & (r2 <= rs2))
        dd = np.stack([da[ii, jj].astype(np.float64) for da in d], axis=1)
        d0 = ref[jj] - ref[s0 + ii]
        k = _image_of_d0(d0, dd, box, box0, image)
        d0 -= box0[None, :] * k
        images.append(np.column_stack([s0 + ii, jj, k.astype(np.int64)]))
        return ii, jj, dd, d0

    vm, am = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    s, cnt, rmin = np.zeros(n), np.zeros(n, dtype=np.int64), np.full(n, np.inf)
    lists7, images = [], []
    for s0 in range(0, n, block):
        m = min(block, n - s0)
        ii, jj, dd, d0 = pairs(s0, m)
        for a in range(3):
            for b in range(3):
                vm[s0:s0 + m, a, b] = np.bincount(ii, weights=d0[:, a] * d0[:, b], minlength=m)
                am[s0:s0 + m, a, b] = np.bincount(ii, weights=dd[:, a] * d0[:, b], minlength=m)
        rr = (dd * dd).sum(1)
        s[s0:s0 + m] = np.bincount(ii, weights=rr, minlength=m)
        cnt[s0:s0 + m] = np.bincount(ii, minlength=m)
        np.minimum.at(rmin, s0 + ii, np.sqrt(rr))
        lists7.append(s0 + ii[jj == 7])
    f, det = _adjugate_fit(vm, am)
    tr3 = (vm[:, 0, 0] + vm[:, 1, 1] + vm[:, 2, 2]) / 3.0
    invalid = (cnt < 3) | (det <= 1e-9 * tr3 ** 3)
    g = 0.5 * (np.swapaxes(f, 1, 2) @ f - np.eye(3)[None])
    e = np.stack([g[:, 0, 0], g[:, 1, 1], g[:, 2, 2], g[:, 1, 2], g[:, 0, 2], g[:, 0, 1]], axis=1)
    if image_rows is not None:                                  # (before the second walk, which forms the same rows again)
        image_rows.extend(images)
    d2 = np.zeros(n)
    for s0 in range(0, n, block):                               # second walk: the direct form of D^2 needs F
        m = min(block, n - s0)
        ii, jj, dd, d0 = pairs(s0, m)
        res = dd - np.einsum("pab,pb->pa", f[s0 + ii], d0)
        d2[s0:s0 + m] = np.bincount(ii, weights=(res * res).sum(1), minlength=m)
    e[invalid], d2[invalid] = np.nan, np.nan
    with np.errstate(all="ignore"):
        kappa = np.where(cnt >= 3, np.linalg.cond(np.where(cnt[:, None, None] >= 3, vm, np.eye(3)[None])), np.inf)
        det_ratio = det / np.maximum(tr3, 1e-300) ** 3
    return dict(e=e, d2=d2, n=cnt, kappa=kappa, s=s, rmin=rmin, det_ratio=det_ratio, invalid=invalid, lists7=np.unique(np.concatenate(lists7)))


def _third_nearest(pos, box, block=256):
    """the median over the atoms of the distance to the third-nearest neighbour under the minimum image"""
    out = []
    for s0 in range(0, len(pos), block):
        d = pos[None, :, :] - pos[s0:s0 + block, None, :]
        d -= box * np.rint(d / box)
        out.append(np.sqrt(np.partition((d * d).sum(2), 3, axis=1)[:, 3]))
    return float(np.median(np.concatenate(out)))


def _eps(m, precision, box):
    return EPS53 if precision == "double" else EPS24 * (float(np.max(box)) / m["rmin"])


RATIOS = {}


def _assert_within(what, got, want_e, want_d2, m, eps, c=C_BOUND, invalid=None, d2_by_kappa=False):
    """got = (E, d2, n) of the device against want_e (n, 6) / want_d2 (n,), with n, kappa and S of the restatement m: every atom, every component.
    invalid (default: no atom may be): the mask of the atoms the restatement holds invalid.  With it the neighbour counts of all atoms and the NaN pattern
    must be the restatement's exactly, and the valid atoms are held to the same bound.
    d2_by_kappa (default off; tests/test_analysis_regimes.py, which shows in numpy alone where it is needed): |dD^2| <= C (n_i + 64) eps kappa(V_i) S_i.  The kernel has
    one pass over the pairs and forms D^2 = S - F : A from the sums; F = A V^-1 carries a relative error of eps kappa(V_i), so F : A, of the size of S, carries
    eps kappa S.  Where three to ten neighbours leave V_i nearly singular (kappa 1e5) that is what any one-pass form gives, numpy's in double included."""
    e, d2, cnt = got
    assert e.shape == (len(m["n"]), 6) and e.dtype == np.float64 and d2.dtype == np.float64 and cnt.dtype == np.int32
    assert np.array_equal(cnt, m["n"]), (what, np.nonzero(cnt != m["n"])[0][:8])
    if invalid is None:
        assert not m["invalid"].any() and not np.isnan(e).any() and not np.isnan(d2).any(), what
        ok = np.ones(len(m["n"]), dtype=bool)
    else:
        ok = ~np.asarray(invalid, dtype=bool)
        assert np.array_equal(~ok, m["invalid"]), (what, np.nonzero(~ok != m["invalid"])[0][:8])
        assert np.array_equal(np.isnan(e), np.broadcast_to(~ok[:, None], e.shape)) and np.array_equal(np.isnan(d2), ~ok), (what, np.nonzero(np.isnan(d2) != ~ok)[0][:8])
    if not ok.any():
        RATIOS[what] = (0.0, 0.0)
        print(f"RATIO {what}: no valid atom (n {m['n'].min()}..{m['n'].max()})")
        return
    e, d2, want_e, want_d2 = e[ok], d2[ok], want_e[ok], want_d2[ok]
    eps = eps[ok] if np.ndim(eps) else eps
    bound_e = (m["n"][ok] + 64.0) * eps * m["kappa"][ok] * (1.0 + 2.0 * np.abs(want_e).max(1))
    bound_d = (m["n"][ok] + 64.0) * eps * m["s"][ok] * (m["kappa"][ok] if d2_by_kappa else 1.0)
    ratio_e, ratio_d = (np.abs(e - want_e) / bound_e[:, None]).max(), (np.abs(d2 - want_d2) / bound_d).max()
    RATIOS[what] = (float(ratio_e), float(ratio_d))
    print(f"RATIO {what}: E {ratio_e:.4g} D2 {ratio_d:.4g} (bound at C = 1; n {m['n'].min()}..{m['n'].max()}, kappa <= {m['kappa'][ok].max():.3g})")
    assert ratio_e <= c and ratio_d <= c, (what, ratio_e, ratio_d)


def _shear(e):
    d0, d1, d2 = e[:, 0] - e[:, 1], e[:, 1] - e[:, 2], e[:, 2] - e[:, 0]
    return np.sqrt(((e[:, 3] * e[:, 3] + e[:, 4] * e[:, 4]) + e[:, 5] * e[:, 5]) + ((d0 * d0 + d1 * d1) + d2 * d2) / 6.0)


def _displace_one(sim, g=7):
    r = sim.gather(0).copy()
    r[g] += MOVE
    sim.scatter(0, r)
    sim.redistribute()
    sim.compute_force()


def _assert_state(name, sim):
    st = STATES[name]
    assert sim.n_global == st["atoms"] and tuple(sim.grid) == st["grid"], (name, sim.n_global, sim.grid)
    assert st["classes"] <= _chunk_classes(sim.cells()["nAtoms"][:sim.n_local_boxes]), name
    assert st["rc"] < 0.5 * 0.99 * _extent(st).min()            # the restatement's image is the kernel's, after the deformation too


# ---------------------------------------------------------------- CPU: flags, exports, refusals, ISA
def test_strain_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--strain', '--strainRef', 5, '--strainCutoff', 3.0, '--strainThreshold', 0.2, '--strainFile', 's.dat', "
                  "'--strainDump', 's.xyz', '--strainDumpMin', 0.05], host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("strain", "strainRef", "strainCutoff", "strainThreshold", "strainFile", "strainDump", "strainDumpMin"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])
    for bad in (["--strainThreshold", 0], ["--strainThreshold", -0.1], ["--strainCutoff", 0], ["--strainCutoff", 100.0], ["--strainDumpMin", -1],
                ["--strainRef", 101], ["--strainRef", -1]):
        proc = _child(f"pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--strain'] + {bad!r}, host_only=True); print('made')")
        assert proc.returncode != 0 and "made" not in proc.stdout and "Error:" in proc.stdout and bad[0][2:] in proc.stdout, (bad, proc.stdout[-2000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_entry_points_are_exported_and_declared(sfx):
    def defined(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"{lib}{sfx}.so")], capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"comdStrainReferenceGpu", "computeAtomStrain", "computeAtomStrainSummary"} <= defined("libcomd_hip")
    assert {"comdStrainReference", "comdAtomStrain", "comdStrainSummary"} <= defined("libcomd_host")
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^int comdStrainReferenceGpu\(SimGpu\* sim, int nGlobal, int on\);", header, flags=re.M)
    assert re.search(r"^void computeAtomStrain\(SimGpu\* sim, real_t rCut, real_t\* outBySlot7, int\* outCountBySlot\);", header, flags=re.M)
    assert re.search(r"^void computeAtomStrainSummary\(SimGpu\* sim, double threshold, double\* out\);", header, flags=re.M)
    header = open(os.path.join(CSRC, "host", "comd_host.h")).read()
    assert re.search(r"^int comdStrainReference\(SimFlat\* s, int on\);", header, flags=re.M)
    assert re.search(r"^int comdAtomStrain\(SimFlat\* s, double rCut, double\* strainByGid7, int\* countByGid\);", header, flags=re.M)
    assert re.search(r"^int comdStrainSummary\(SimFlat\* s, double rCut, double threshold, double\* out9\);", header, flags=re.M)


def test_host_only_simulation_refuses(pkg):
    import ctypes
    sim = pkg.Simulation(["-x", 8, "-y", 8, "-z", 8], host_only=True)
    for call in (sim.set_strain_reference, sim.atomic_strain, sim.shear_strain, sim.volumetric_strain, sim.strain_summary):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        sim.strain_reference_box
    # the C entries themselves return -1 without device state
    out, cnt = np.zeros((max(sim.n_global, 2048), 7)), np.zeros(max(sim.n_global, 2048), dtype=np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    assert sim.lib.comdStrainReference(sim.ptr, 1) == -1
    assert sim.lib.comdAtomStrain(sim.ptr, 0.0, out.ctypes.data_as(dp), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == -1
    assert sim.lib.comdStrainSummary(sim.ptr, 0.0, 0.1, (ctypes.c_double * 9)()) == -1
    sim.close()


@pytest.mark.parametrize("precision", ["double", "single"])
def test_strain_kernels_exist_and_use_no_scratch(precision):
    """The pair walk, the reference store and the two summary kernels exist in both builds and none spills to scratch; the VGPR counts are printed."""
    blocks = device_isa.blocks(precision, r"(?:AtomStrain|StrainReference)_\w+")
    names = sorted(blocks)
    assert len(names) == 4, names
    for part in ("AtomStrain_thread_atom", "AtomStrain_SummaryP", "AtomStrain_SummaryFinal", "StrainReference_Store"):
        assert any(part in n for n in names), (part, names)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
        print(precision, name, "VGPRs", re.search(r"\.amdhsa_next_free_vgpr (\d+)\n", block).group(1))
    device_isa.assert_keeps_waves(blocks, "AtomStrain_thread_atom", 4)


# ---------------------------------------------------------------- GPU: refusals before a launch
@pytest.mark.gpu
def test_refusals_come_before_a_launch(gpu):
    with gpu.Simulation(STATES["D"]["flags"]) as sim:
        for call in (sim.atomic_strain, sim.shear_strain, sim.volumetric_strain, sim.strain_summary):
            with pytest.raises(ValueError):
                call()                                           # no reference
        with pytest.raises(ValueError):
            sim.strain_reference_box
        sim.set_strain_reference()
        assert np.array_equal(sim.strain_reference_box, sim.box) and sim.strain_reference_box.dtype == np.float64
        for cutoff in (0.0, -1.0, sim.cutoff * 1.0001):
            with pytest.raises(ValueError):
                sim.atomic_strain(cutoff)
            with pytest.raises(ValueError):
                sim.strain_summary(cutoff=cutoff)
        for threshold in (0.0, -0.1):
            with pytest.raises(ValueError):
                sim.strain_summary(threshold=threshold)
        assert sim.atomic_strain(sim.cutoff)[2].min() > 12
        sim.set_strain_reference(False)
        with pytest.raises(ValueError):
            sim.atomic_strain()
        assert np.all(sim.strain == 0.0)                         # the box-strain property keeps its meaning


# ---------------------------------------------------------------- GPU: physics with exact answers
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_zero_strain_at_the_reference(gpu, name):
    """Reference, then atomic_strain() at once: E = 0, D^2 = 0, and the counts are centro_symmetry's coordination at the same radius, exactly."""
    with gpu.Simulation(STATES[name]["flags"]) as sim:
        _assert_state(name, sim)
        sim.set_strain_reference()
        pos, box = sim.gather(0).copy(), sim.box
        for key, rs in _radii(sim).items():
            got = sim.atomic_strain(rs)
            assert np.array_equal(got[2], sim.centro_symmetry(r_coord=rs)[1])
            m = _restate(pos, box, pos, box, _default_rs(STATES[name]["lat"]) if rs is None else rs)
            _assert_within(f"zero {name} {key}", got, np.zeros((len(pos), 6)), np.zeros(len(pos)), m, EPS53)


def _homogeneous_answer(sim, n):
    s = sim.box / sim.strain_reference_box
    assert np.abs(s - np.array(SCALE)).max() <= 4.0 * EPS53
    want = np.zeros((n, 6))
    want[:, :3] = 0.5 * (s * s - 1.0)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_homogeneous_deformation(gpu, name):
    """10 steps, reference, deform((1.02, 0.99, 1)): every atom has E = diag(1/2 (s^2 - 1)), no shear components, D^2 = 0; the shear invariant is 0.0153626."""
    with gpu.Simulation(STATES[name]["flags"]) as sim:
        sim.step(10)
        sim.set_strain_reference()
        ref, box0 = sim.gather(0).copy(), sim.box
        sim.deform(SCALE)
        pos, box = sim.gather(0).copy(), sim.box
        want = _homogeneous_answer(sim, len(pos))
        assert abs(_shear(want)[0] - 0.0153626) < 5e-8
        for key, rs in _radii(sim).items():
            m = _restate(pos, box, ref, box0, _default_rs(STATES[name]["lat"]) if rs is None else rs)
            got = sim.atomic_strain(rs)
            _assert_within(f"homogeneous {name} {key}", got, want, np.zeros(len(pos)), m, EPS53)
            # the shear invariant is Lipschitz in the components with constant sqrt(3) < 2
            bound = 2.0 * C_BOUND * (m["n"] + 64.0) * EPS53 * m["kappa"] * (1.0 + 2.0 * np.abs(want).max())
            assert np.all(np.abs(sim.shear_strain(rs) - _shear(want)) <= bound)
            assert np.all(np.abs(sim.volumetric_strain(rs) - want[:, :3].sum(1) / 3.0) <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_rigid_translation_across_the_boundary(gpu, name):
    """Reference, then every atom moved by (2.1, -1.9, 2.3): many wrap and change cells; E = 0, D^2 = 0, counts unchanged."""
    # the device appends movers to a cell before it squeezes the holes they leave: with most atoms changing cell at once (never the case in MD) a cell
    # transiently holds its old and its incoming atoms and needs twice the usual head-room (tests/test_gpu_parity.py test_redistribution_is_bit_exact)
    room = {"A": 768, "B": 512, "C": 128, "E": 64, "F": 128}[name]
    with gpu.Simulation(STATES[name]["flags"] + ["--maxAtoms", room]) as sim:
        _assert_state(name, sim)
        sim.set_strain_reference()
        ref, box = sim.gather(0).copy(), sim.box
        before = {key: sim.atomic_strain(rs)[2] for key, rs in _radii(sim).items()}
        sim.scatter(0, ref + np.array([2.1, -1.9, 2.3]))
        sim.redistribute()
        sim.compute_force()
        pos = sim.gather(0).copy()
        assert int(sim.cells()["nAtoms"][:sim.n_local_boxes].sum()) == len(pos)  # no atom was lost to a full cell
        assert (np.abs(pos - ref).max(1) > 3.0).sum() > len(pos) // 20          # atoms have wrapped
        for key, rs in _radii(sim).items():
            m = _restate(pos, box, ref, box, _default_rs(STATES[name]["lat"]) if rs is None else rs)
            got = sim.atomic_strain(rs)
            assert np.array_equal(got[2], before[key])
            _assert_within(f"translation {name} {key}", got, np.zeros((len(pos), 6)), np.zeros(len(pos)), m, EPS53)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [["-x", 8, "-y", 8, "-z", 8], ["-x", 6, "-y", 6, "-z", 6, "-e"]])
def test_one_displaced_atom(gpu, flags):
    """Perfect lattice, reference, atom 7 moved by (0.4, -0.3, 0.2): it and the atoms that list it have D^2 > 0.1 A^2, every other atom is unstrained."""
    with gpu.Simulation(flags + ["-r", 0, "-T", 0]) as sim:
        sim.set_strain_reference()
        ref, box = sim.gather(0).copy(), sim.box
        _displace_one(sim)
        pos = sim.gather(0).copy()
        m = _restate(pos, box, ref, box, _default_rs(sim.lattice_constant))
        e, d2, cnt = sim.atomic_strain()
        hit = np.zeros(len(pos), dtype=bool)
        hit[7] = True
        hit[m["lists7"]] = True
        assert 10 <= hit.sum() <= 15 and np.all(d2[hit] > 0.1), (hit.sum(), d2[hit].min())
        print("D2 of the displaced atom and of those that list it:", d2[hit].min(), d2[hit].max())
        rest = ~hit
        mr = {k: v[rest] for k, v in m.items() if k != "lists7"}
        _assert_within(f"one atom {flags[-1]}", (e[rest], d2[rest], cnt[rest]), np.zeros((rest.sum(), 6)), np.zeros(rest.sum()), mr, EPS53)
        summary = sim.strain_summary()
        assert summary["max_shear_gid"] in np.nonzero(hit)[0] and summary["n"] == len(pos) and summary["invalid"] == 0


# ---------------------------------------------------------------- GPU: the restatement
def _history(sim, steps=20):
    """reference at step 0, `steps` steps, the deformation, the one-atom displacement"""
    sim.set_strain_reference()
    ref, box0 = sim.gather(0).copy(), sim.box
    if steps:
        sim.step(steps)
    sim.deform(SCALE)
    _displace_one(sim)
    return ref, box0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C", "E", "F", "B"])
def test_matches_the_restatement(gpu, name):
    """Reference at step 0, 20 steps, deform, one displaced atom: every atom and every component against the all-pairs fit, at both radii."""
    with gpu.Simulation(STATES[name]["flags"]) as sim:
        _assert_state(name, sim)
        ref, box0 = _history(sim)
        pos, box = sim.gather(0).copy(), sim.box
        for key, rs in _radii(sim).items():
            r = _default_rs(STATES[name]["lat"]) if rs is None else rs
            assert r < 0.5 * box.min()
            m = _restate(pos, box, ref, box0, r)
            assert m["n"].min() >= 3 and m["det_ratio"].min() > 10.0 * 1e-9, (m["n"].min(), m["det_ratio"].min())
            got = sim.atomic_strain(rs)
            assert np.abs(m["e"]).max() > 5e-3 and m["d2"].max() > 0.1
            _assert_within(f"restatement {name} {key}", got, m["e"], m["d2"], m, EPS53)


# ---------------------------------------------------------------- GPU: methods, layouts, ranks
CHILD_RUN = """
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    assert pkg.PRECISION == {precision!r}
    sim = pkg.Simulation({args!r})
    steps, out = {steps}, {{}}
    sim.step(10)
    sim.set_strain_reference()
    out["h_ref"], out["h_box0"] = sim.gather(0).copy(), sim.box
    sim.deform({scale!r})
    out["h_pos"], out["h_box"] = sim.gather(0).copy(), sim.box
    for key, rs in (("default", None), ("cutoff", sim.cutoff)):
        out["h_e_" + key], out["h_d2_" + key], out["h_n_" + key] = sim.atomic_strain(rs)
    sim.set_strain_reference()
    out["ref"], out["box0"] = sim.gather(0).copy(), sim.box
    if steps:
        sim.step(steps)
    sim.deform({scale!r})
    r = sim.gather(0).copy()
    r[7] += np.array({move!r})
    sim.scatter(0, r)
    sim.redistribute()
    sim.compute_force()
    out["pos"], out["box"] = sim.gather(0).copy(), sim.box
    for key, rs in (("default", None), ("cutoff", sim.cutoff)):
        out["e_" + key], out["d2_" + key], out["n_" + key] = sim.atomic_strain(rs)
    np.savez({out!r}, cutoff=sim.cutoff, **out)
    sim.close()
"""


def _strain_in_child(args, out, env=None, precision="double", steps=0):
    proc = _child(CHILD_RUN.format(args=list(args), out=str(out), precision=precision, steps=steps, scale=SCALE, move=MOVE.tolist()), env=env)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "D"])
def test_methods_and_layouts_agree(gpu, tmp_path, name):
    """Every method, cell numbering, stream mode, list format and halo form on the 2-cell LJ box and the setfl state, after the deformation and the
    one-atom displacement of a step-0 reference (the positions are the same bits under every method): identical counts, E and D^2 within the bound of
    thread_atom's, which is bit-identical run to run."""
    st = STATES[name]
    lj = st["pair"] != "eam"
    got, state = {}, None
    for method, extra in (LJ_METHODS if lj else EAM_METHODS) + [("thread_atom", [])]:
        with gpu.Simulation(st["flags"] + ["-m", method] + extra) as sim:
            ref, box0 = _history(sim, steps=0)
            key = " ".join([method] + [str(x) for x in extra])
            res = {k: sim.atomic_strain(rs) for k, rs in _radii(sim).items()}
            if key in got:                                       # thread_atom again: bit-reproducible run to run
                for k in res:
                    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(res[k], got[key][k]))
                assert sim.strain_summary() == state["summary"]
                continue
            got[key] = res
            if state is None:
                state = dict(ref=ref, box0=box0, pos=sim.gather(0).copy(), box=sim.box, summary=sim.strain_summary(), radii=_radii(sim))
            else:
                assert np.array_equal(sim.gather(0), state["pos"])
    for env in [{"COMD_NL_GLOBAL": "1"}] if lj else [{"COMD_EAM_GROUPS": "0"}, {"COMD_HALO_MIRROR": "0"}]:
        method = "thread_atom_nl" if "COMD_NL_GLOBAL" in env else "cta_cell"
        d = _strain_in_child(st["flags"] + ["-m", method], tmp_path / f"{len(got)}.npz", env=env)
        got[f"{method} {env}"] = {k: (d["e_" + k], d["d2_" + k], d["n_" + k]) for k in ("default", "cutoff")}
    child_keys = [k for k in got if "{" in k]
    for k, rs in state["radii"].items():
        m = _restate(state["pos"], state["box"], state["ref"], state["box0"], _default_rs(st["lat"]) if rs is None else rs)
        base = got["thread_atom"][k]
        for key, res in got.items():
            if key in child_keys:
                continue                                         # another history (10 steps before the reference): compared below
            _assert_within(f"methods {name} {key} {k}", res[k], base[0], base[1], m, EPS53)
    # the children ran CHILD_RUN's history: against thread_atom on that history
    base = _strain_in_child(st["flags"] + ["-m", "thread_atom"], tmp_path / "base.npz")
    for k, rs in state["radii"].items():
        m = _restate(base["pos"], base["box"], base["ref"], base["box0"], _default_rs(st["lat"]) if rs is None else rs)
        for key in child_keys:
            _assert_within(f"methods {name} {key} {k}", got[key][k], base["e_" + k], base["d2_" + k], m, EPS53)


def _ranks(grid, args, out_dir, steps, timeout=900):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    assert world <= 8
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "strain_worker.py"), str(r), str(world), port, *map(str, grid), str(out_dir), str(steps),
                               json.dumps(args)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
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
    return [(np.load(os.path.join(out_dir, f"strain_rank{r}.npz")), json.load(open(os.path.join(out_dir, f"strain_rank{r}.json")))) for r in range(world)]


@functools.lru_cache(maxsize=None)
def _one_rank(pot):
    """the one-rank arrays, summary and restatement of the rank test's history: reference at step 0, 20 steps"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    args = ["-x", 12, "-y", 12, "-z", 12, "-r", 0.1, "--ljCutoffSigmas", 2.5] if pot == "lj" else ["-x", 8, "-y", 8, "-z", 8, "-r", 0.1, "-e"]
    with pkg.Simulation(args) as sim:
        sim.set_strain_reference()
        ref, box = sim.gather(0).copy(), sim.box
        sim.step(20)
        got, summary = sim.atomic_strain(), sim.strain_summary()
        m = _restate(sim.gather(0).copy(), box, ref, box, _default_rs(sim.lattice_constant))
    return args, got, summary, m, box


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot", ["lj", "eam"])
def test_ranks_give_the_one_rank_arrays(gpu, tmp_path, grid, pot):
    """2 and 8 ranks sharing the device (gloo transport), the reference taken on the ranks, then 20 steps: every rank returns the global arrays, the
    one-rank ones within the bound, and the summary reduced over the ranks with the same gid of the maximum."""
    args, got0, sum0, m, box = _one_rank(pot)
    gamma = _shear(got0[0])
    order = np.sort(gamma)
    g = int(np.argmax(gamma))
    bound_g = 2.0 * C_BOUND * (m["n"] + 64.0) * EPS53 * m["kappa"] * (1.0 + 2.0 * np.abs(got0[0]).max(1))
    assert order[-1] - order[-2] > 2.0 * bound_g.max()              # the maximum is not a near-tie the ranks could resolve differently
    assert sum0["max_shear_gid"] == g
    for d, summary in _ranks(grid, args, tmp_path, 20):
        assert np.array_equal(d["box0"], box)
        _assert_within(f"ranks {pot} {grid}", (d["e"], d["d2"], d["n"]), got0[0], got0[1], m, EPS53)
        assert summary["n"] == sum0["n"] == len(gamma) and summary["invalid"] == 0 and summary["max_shear_gid"] == g
        assert summary["above_threshold"] == sum0["above_threshold"]
        for key, scale in (("max_shear", bound_g.max()), ("mean_shear", bound_g.max()), ("mean_volumetric", bound_g.max()),
                           ("max_d2min", (C_BOUND * (m["n"] + 64.0) * EPS53 * m["s"]).max()), ("mean_d2min", (C_BOUND * (m["n"] + 64.0) * EPS53 * m["s"]).max())):
            assert abs(summary[key] - sum0[key]) <= scale, (key, summary[key], sum0[key])


# ---------------------------------------------------------------- GPU: the device reduction
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "E"])
def test_summary_is_numpy_on_the_arrays(gpu, name):
    """strain_summary() against numpy on atomic_strain() of the same state: means to 1e-12 relative, extremes to 1e-14 relative, the same gid of the
    maximum, the same threshold and invalid counts; a radius that leaves atoms with fewer than 3 neighbours gives NaNs and an invalid count."""
    with gpu.Simulation(STATES[name]["flags"]) as sim:
        _history(sim)
        e, d2, cnt = sim.atomic_strain()
        gamma, vol = _shear(e), (e[:, 0] + e[:, 1] + e[:, 2]) / 3.0
        assert np.array_equal(sim.shear_strain(), gamma) and np.abs(sim.volumetric_strain() - vol).max() <= 1e-15
        threshold = float(np.median(gamma))
        got = sim.strain_summary(threshold=threshold)
        order = np.sort(gamma)
        assert order[-1] - order[-2] > 1e-14 * order[-1]
        assert got["n"] == len(e) and got["invalid"] == 0 and got["max_shear_gid"] == int(np.argmax(gamma))
        assert got["above_threshold"] == int((gamma >= threshold).sum())
        for key, want, tol in (("mean_shear", gamma.mean(), 1e-12), ("mean_volumetric", vol.mean(), 1e-12), ("mean_d2min", d2.mean(), 1e-12),
                               ("max_shear", gamma.max(), 1e-14), ("max_d2min", d2.max(), 1e-14)):
            print(name, key, got[key], want, abs(got[key] - want) / abs(want))
            assert abs(got[key] - want) <= tol * abs(want), (key, got[key], want)
        assert sim.strain_summary(threshold=threshold) == got                  # bit-reproducible run to run
        assert sim.strain_summary()["above_threshold"] == int((gamma >= 0.1).sum())
        # the median distance to the third-nearest neighbour as the radius: about half the atoms have fewer than 3; they are NaN, counted and left out
        small = _third_nearest(sim.gather(0), sim.box)
        e, d2, cnt = sim.atomic_strain(small)
        bad = np.isnan(e[:, 0])
        assert bad.any() and not bad.all() and np.all(np.isnan(d2) == bad) and np.all(np.isnan(e) == bad[:, None])
        assert np.all(bad[cnt < 3])
        got = sim.strain_summary(cutoff=small)
        gamma = _shear(e[~bad])
        assert got["n"] == len(e) and got["invalid"] == int(bad.sum()) and got["max_shear_gid"] == int(np.nonzero(~bad)[0][np.argmax(gamma)])
        assert abs(got["mean_shear"] - gamma.mean()) <= 1e-12 * gamma.mean() and abs(got["max_d2min"] - d2[~bad].max()) <= 1e-14 * d2[~bad].max()


# ---------------------------------------------------------------- GPU: single precision
@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj", "eam"])
def test_single_precision_build(gpu, tmp_path, pot):
    """The float build (COMD_PRECISION=single, lib*_sp.so) in a child, state B and the Adams 6^3 state: the homogeneous deformation and the restatement
    history (20 steps), both radii, against the restatement in double of the child's own gathered float positions, with d formed in float as the
    kernel forms it; eps = 2^-24 (largest box extent / the atom's shortest neighbour distance)."""
    n = 8 if pot == "lj" else 6
    args = ["-x", n, "-y", n, "-z", n, "-l", LAT, "-r", 0.1] + (["-e"] if pot == "eam" else [])
    d = _strain_in_child(args, tmp_path / "single.npz", env={"COMD_PRECISION": "single"}, precision="single", steps=20)
    cutoff = float(d["cutoff"])
    assert abs(cutoff - (4.95 if pot == "eam" else STATES["B"]["rc"])) <= 4.0 * EPS24 * cutoff
    s = d["h_box"] / d["h_box0"]
    want = np.zeros((len(d["pos"]), 6))
    want[:, :3] = 0.5 * (s * s - 1.0)
    assert np.abs(s - np.array(SCALE)).max() <= 4.0 * EPS24
    for key, rs in (("default", _default_rs(LAT)), ("cutoff", cutoff)):
        assert rs < 0.5 * d["box"].min()
        m = _restate(d["h_pos"], d["h_box"], d["h_ref"], d["h_box0"], rs, dtype=np.float32)
        _assert_within(f"single homogeneous {pot} {key}", (d["h_e_" + key], d["h_d2_" + key], d["h_n_" + key]), want, np.zeros(len(want)), m,
                       _eps(m, "single", d["h_box"]))
        m = _restate(d["pos"], d["box"], d["ref"], d["box0"], rs, dtype=np.float32)
        assert m["n"].min() >= 3 and m["det_ratio"].min() > 10.0 * 1e-9
        _assert_within(f"single restatement {pot} {key}", (d["e_" + key], d["d2_" + key], d["n_" + key]), m["e"], m["d2"], m, _eps(m, "single", d["box"]))


# ---------------------------------------------------------------- GPU: comd-hip
def _strain_file(path):
    lines = path.read_text().splitlines()
    return lines[0], [[float(x) for x in line.split()] for line in lines[1:]]


@pytest.mark.gpu
def test_comd_hip_strain_column_file_dump_and_yaml(gpu, tmp_path):
    out0, rows0, yaml0 = _comd_hip(tmp_path, [])
    # without the flag: the table of before (no column, no timer row, no file, nothing in the YAML)
    assert [line for line in out0.splitlines() if line.startswith("#  Loop")] == [HEADER]
    assert all(r[3].strip() == "" for r in rows0) and [r[0] for r in rows0] == ["0", "10", "20"]
    assert "MaxShear" not in out0 and not re.search(r"^strain\s", out0, flags=re.M) and not re.search(r"^Strain:", yaml0, flags=re.M)
    assert "Strain reference" not in yaml0 and not os.path.exists(tmp_path / "strain.dat")

    out1, rows1, yaml1 = _comd_hip(tmp_path, ["--strain", "--strainDump", "dump.xyz"])
    header = [line for line in out1.splitlines() if line.startswith("#  Loop")][0]
    assert header.startswith(HEADER) and header.split()[-1] == "MaxShear" and len(header.split()) == len(HEADER.split()) + 1
    assert [r[:3] for r in rows1] == [r[:3] for r in rows0]                  # the trajectory is untouched by the flag, to the bit
    cols = [[float(x) for x in r[3].split()] for r in rows1]
    assert all(len(c) == 1 for c in cols) and cols[0][0] == 0.0 and cols[1][0] > 0.0 and cols[2][0] > 0.0
    assert re.search(r"^strain\s+4\s", out1, flags=re.M)                     # three samples and the files
    head, data = _strain_file(tmp_path / "strain.dat")
    assert head.startswith("# Strain: N 2048 L0 ") and "reference step 0 " in head and "samples 3" in head and "threshold 0.1" in head
    assert [d[0] for d in data] == [0.0, 10.0, 20.0] and all(len(d) == 9 for d in data)
    assert data[0][2] < 1e-12 and data[0][5] < 1e-10                          # the reference's own sample is zero
    for d, c in zip(data, cols):
        assert abs(d[2] - c[0]) <= 1e-10 and 0.0 <= d[1] <= d[2] and 0.0 <= d[5] <= d[6] and d[8] == 0.0
        assert 0 <= d[3] < 2048 and d[3] == int(d[3]) and d[7] == int(d[7])
    dump = (tmp_path / "dump.xyz").read_text().splitlines()
    assert dump[0] == "2048" and len(dump) == 2 + 2048 and "step=20" in dump[1]
    assert "Properties=species:S:1:pos:R:3:strain:R:6:shear:R:1:vol:R:1:d2min:R:1:n:I:1:gid:I:1" in dump[1]
    atoms = np.array([[float(x) for x in line.split()[1:]] for line in dump[2:]])
    assert atoms.shape == (2048, 14) and np.array_equal(atoms[:, 13], np.arange(2048)) and atoms[:, 12].min() >= 3
    assert np.abs(_shear(atoms[:, 3:9]) - atoms[:, 9]).max() <= 1e-15
    assert np.abs(atoms[:, 3:6].sum(1) / 3.0 - atoms[:, 10]).max() <= 1e-15
    assert abs(atoms[:, 9].max() - data[-1][2]) <= 1e-14 * data[-1][2] and int(np.argmax(atoms[:, 9])) == int(data[-1][3])
    assert abs(atoms[:, 9].mean() - data[-1][1]) <= 1e-12 * data[-1][1] and abs(atoms[:, 11].max() - data[-1][6]) <= 1e-14 * data[-1][6]
    assert int((atoms[:, 9] >= 0.1).sum()) == int(data[-1][7])
    block = re.search(r"^Strain:\n((?:  .*\n)+)", yaml1, flags=re.M).group(1)
    m = dict(re.findall(r"^  (\w+): (\S+)$", block, flags=re.M))
    assert m["samples"] == "3" and m["file"] == "strain.dat" and m["referenceStep"] == "0"
    assert abs(float(m["finalMaxShear"]) - data[-1][2]) <= 1e-11 * data[-1][2] and abs(float(m["finalMeanD2min"]) - data[-1][5]) <= 1e-11 * data[-1][5]

    # --strainDumpMin: only the atoms at or above the threshold
    cut = float(np.median(atoms[:, 9]))
    _comd_hip(tmp_path, ["--strain", "--strainDump", "cut.xyz", "--strainDumpMin", repr(cut), "--strainFile", "other.dat"])
    kept = (tmp_path / "cut.xyz").read_text().splitlines()
    assert int(kept[0]) == len(kept) - 2 == int((atoms[:, 9] >= cut).sum()) and os.path.exists(tmp_path / "other.dat")
    # --strainRef 10: 0 before the reference and at it; --strainRef 15 lies between two printed steps
    out2, rows2, _ = _comd_hip(tmp_path, ["--strain", "--strainRef", "10"])
    cols = [float(r[3].split()[-1]) for r in rows2]
    assert [r[:3] for r in rows2] == [r[:3] for r in rows0] and cols[0] == 0.0 and cols[1] == 0.0 and cols[2] > 0.0
    head, data = _strain_file(tmp_path / "strain.dat")
    assert "reference step 10 " in head and "samples 2" in head and [d[0] for d in data] == [10.0, 20.0] and data[0][2] < 1e-12
    out3, rows3, _ = _comd_hip(tmp_path, ["--strain", "--strainRef", "15"])
    cols3 = [float(r[3].split()[-1]) for r in rows3]
    assert [r[:3] for r in rows3] == [r[:3] for r in rows0] and cols3[:2] == [0.0, 0.0] and 0.0 < cols3[2] < cols[2]
    for bad in (["--strainThreshold", "0"], ["--strainCutoff", "50"], ["--strainDumpMin", "-1"], ["--strainRef", "21"]):
        out4, rows4, _ = _comd_hip(tmp_path, ["--strain"] + bad, ok=False)
        assert "Error:" in out4 and bad[0][2:] in out4 and rows4 == []


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--stress", "--csp", "--cna", "--pressure", "--erateX", "0.01", "--langevin", "-H", "-a", "1"],
                                   ["-e", "-m", "cta_cell", "-x", "6", "-y", "6", "-z", "6"]])
def test_comd_hip_strain_with_the_other_flags(gpu, tmp_path, extra):
    """--strain beside the other analyses, a straining box, the thermostat, the Hilbert numbering and the overlap mode, and with EAM cta_cell: the column
    is the last one, three samples, and the flag leaves the other columns and the trajectory as they are without it, to the bit."""
    out0, rows0, _ = _comd_hip(tmp_path, extra)
    out1, rows1, yaml1 = _comd_hip(tmp_path, extra + ["--strain"])
    header0, header1 = [[line for line in out.splitlines() if line.startswith("#  Loop")][0] for out in (out0, out1)]
    assert header1.split()[:-1] == header0.split() and header1.split()[-1] == "MaxShear"
    assert len(rows1) == 3 and [r[:3] for r in rows1] == [r[:3] for r in rows0]
    for k, (r0, r1) in enumerate(zip(rows0, rows1)):
        assert r1[3].split()[:-1] == r0[3].split() and (float(r1[3].split()[-1]) > 0.0) == (k > 0)
    head, data = _strain_file(tmp_path / "strain.dat")
    assert len(data) == 3 and [d[2] for d in data] == pytest.approx([float(r[3].split()[-1]) for r in rows1], abs=1e-10)
    assert re.search(r"^Strain:", yaml1, flags=re.M) and re.search(r"^strain\s+4\s", out1, flags=re.M)
