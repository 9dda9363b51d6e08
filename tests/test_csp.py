"""The centro-symmetry parameter and the coordination number (computeCentroSymmetry, comdCentroSymmetry, Simulation.centro_symmetry / defects,
comd-hip --csp).

CoMD has no structural analysis, so nothing here is compared with a recorded number.  The reference is an O(N^2) minimum-image computation on
the gathered positions in float64 numpy.  Two decisions of the kernel are discrete, and the device (which subtracts shifted halo images) may
round a distance differently from numpy (which applies the minimum image):

    which neighbour is the 12th    an atom whose 13th and 12th nearest distances differ by less than DELTA (`gap`), or whose count of neighbours
                                   inside the cutoff passes 12 within DELTA of the cutoff, is left out of the csp comparison;
    who is inside rCoord           an atom with a neighbour within DELTA of rCoord (`edge`) is left out of the coordination comparison.

    build   DELTA      cap on the atoms left out (asserted before anything is compared)
    fp64    1e-9 A     0
    fp32    1e-4 A     0.5 %

Tolerance on csp, derived: an offset sum R_a + R_b carries about 4 roundings of a coordinate of the box extent (<= 51 A).  fp64: 7e-15 each,
|R_a + R_b| <= 6 A, 6 terms: <= 3e-12, the tests allow 1e-10 A^2 + 1e-12 csp.  fp32: the shifted halo image is rounded to 3.8e-6, which gives
<= 1.1e-3, the tests allow 5e-3 A^2 + 1e-5 csp.  Coordination and the +inf masks are compared exactly.
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

SIGMA, LAT = 2.315, 3.615
MISHIN = ["-e", "-t", "setfl", "-p", "Cu01.eam.alloy"]
ADAMS = ["-e"]
RC = {"lj5": 5.0 * SIGMA, "lj2.5": 2.5 * SIGMA, "adams": 4.95, "mishin": 5.506786}
POT = {"lj5": [], "lj2.5": ["--ljCutoffSigmas", 2.5], "adams": ADAMS, "mishin": MISHIN}
DELTA64, DELTA32, CAP32 = 1e-9, 1e-4, 0.005
R_COORD = 0.5 * (np.sqrt(0.5) + 1.0) * LAT                       # the default: halfway between the first two FCC shells
SPARSE = ["-e", "-x", 4, "-y", 5, "-z", 6, "-l", 7.0, "-r", 0.5]          # test_density_regimes' eam_sparse: 2 to 10 neighbours, empty cells
# Frenkel pairs: where the moved atom goes, in lat from the vacated site.  "close": the interstitial stays 1.88 A from the site and
# stands in for the missing neighbour of the ring atoms on its side, whose broken pair then sums to about the offset, |R_a + R_b|^2 = 3.55 A^2 before the
# -r 0.1 noise against the threshold of 3.27 A^2 -- in the numpy reference alone 5 or 6 of the 12 ring atoms come out as defects (5.3 to 5.8 A^2), the others
# at 1.8 to 3.6 A^2.  So "the 12 atoms around the vacated site are defects" is asserted on "apart", the same offset one lattice constant further, and on
# "close" the device set must equal the numpy set, the moved atom in it.
INTERSTITIAL = {"close": (0.5, 0.13, 0.07), "apart": (1.5, 0.13, 0.07)}
LJ_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("cta_cell", ["-L", "-S", 0.03]), ("thread_atom_nl", []),
              ("thread_atom", ["-H"]), ("thread_atom", ["-a", 1]), ("cta_cell", ["-a", 1])]
EAM_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("thread_atom_nl", []), ("cta_cell", ["-H"]), ("cta_cell", ["-a", 1]),
               ("thread_atom", ["-a", 1])]                       # test_rdf's lists


def _cube(n):
    return ["-x", n, "-y", n, "-z", n, "-l", repr(LAT)]


PRELUDE = f"import sys, json\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\n"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


# ---------------------------------------------------------------- numpy restatement
_PAIRS = np.triu_indices(12, 1)


def _numpy_csp(pos, extent, rc, r_coord, delta):
    """dict of per-atom csp, coord, gap (13th - 12th nearest distance), edge (least | |r_ij| - r_coord |) and unsure (the count of neighbours inside
    the cutoff passes 12 within delta of the cutoff), in blocks of 256 rows as test_rdf._distances"""
    n = len(pos)
    extent = np.broadcast_to(np.asarray(extent, dtype=np.float64), (3,))
    csp, coord = np.full(n, np.inf), np.zeros(n, dtype=np.int32)
    gap, edge, unsure = np.full(n, np.inf), np.full(n, np.inf), np.zeros(n, dtype=bool)
    for s in range(0, n, 256):
        d = pos[None, :, :] - pos[s:s + 256, None, :]                # R = r_j - r_i
        d -= np.rint(d / extent) * extent
        r2 = (d * d).sum(-1)
        rows = np.arange(len(r2))
        r2[rows, s + rows] = np.inf                                   # j != i
        r = np.sqrt(r2)
        coord[s:s + 256] = (r < r_coord).sum(1)
        edge[s:s + 256] = np.abs(r - r_coord).min(1)
        near = np.argpartition(r2, 13, axis=1)[:, :14]
        near = np.take_along_axis(near, np.argsort(np.take_along_axis(r2, near, axis=1), axis=1), axis=1)[:, :13]
        r13 = np.take_along_axis(r, near, axis=1)
        gap[s:s + 256] = r13[:, 12] - r13[:, 11]
        inside = (r < rc).sum(1)
        unsure[s:s + 256] = ((r < rc + delta).sum(1) >= 12) != ((r < rc - delta).sum(1) >= 12)
        vec = np.take_along_axis(d, near[:, :12, None], axis=1)       # (rows, 12, 3)
        sums = vec[:, _PAIRS[0], :] + vec[:, _PAIRS[1], :]
        val = np.sort((sums * sums).sum(-1), axis=1)[:, :6]
        acc = val[:, 0].copy()
        for k in range(1, 6):
            acc += val[:, k]                                          # ascending order
        csp[s:s + 256] = np.where(inside >= 12, acc, np.inf)
    out = {"csp": csp, "coord": coord, "gap": gap, "edge": edge, "unsure": unsure}
    for a in out.values():
        a.setflags(write=False)
    return out


_REF = {}


def _reference(key, pos, extent, rc, r_coord, delta):
    """computed once per key, never modified"""
    if key is None:
        return _numpy_csp(pos, extent, rc, r_coord, delta)
    if key not in _REF:
        _REF[key] = _numpy_csp(pos, extent, rc, r_coord, delta)
    return _REF[key]


def _left_out(ref, delta, single):
    """the atoms outside the two comparisons, after the cap of the module docstring"""
    n = len(ref["csp"])
    no_csp, no_coord = (ref["gap"] < delta) | ref["unsure"], ref["edge"] < delta
    cap = CAP32 * n if single else 0
    assert no_csp.sum() <= cap and no_coord.sum() <= cap, (int(no_csp.sum()), int(no_coord.sum()), n)
    return no_csp, no_coord


def _check(csp, coord, ref, single=False, what=""):
    assert csp.dtype == np.float64 and coord.dtype == np.int32 and csp.shape == coord.shape == ref["csp"].shape
    no_csp, no_coord = _left_out(ref, DELTA32 if single else DELTA64, single)
    keep = ~no_csp
    finite = keep & np.isfinite(ref["csp"])
    diff = np.abs(csp[finite] - ref["csp"][finite]) if finite.any() else np.zeros(1)
    tol = (5e-3 + 1e-5 * ref["csp"][finite]) if single else (1e-10 + 1e-12 * ref["csp"][finite])
    print(f"{what}: atoms {len(csp)}, left out {int(no_csp.sum())} / {int(no_coord.sum())}, +inf {int(np.isinf(ref['csp']).sum())}, "
          f"largest |csp difference| {diff.max():.3e} (largest csp {ref['csp'][finite].max() if finite.any() else 0.0:.3e})")
    assert np.array_equal(np.isinf(csp[keep]), np.isinf(ref["csp"][keep])), what
    assert not np.isnan(csp).any() and np.all(csp >= 0.0)
    assert np.all(diff <= tol), (what, diff.max())
    assert np.array_equal(coord[~no_coord], ref["coord"][~no_coord]), what


def _against_numpy(sim, extent, rc, r_coord=None, key=None, single=False):
    pos = sim.gather(0)
    csp, coord = sim.centro_symmetry(r_coord)
    assert abs(sim.cutoff - rc) <= 1e-6
    ref = _reference(key, pos, extent, sim.cutoff, R_COORD if r_coord is None else r_coord, DELTA32 if single else DELTA64)
    _check(csp, coord, ref, single, str(key))
    return csp, coord


def _host_positions(pkg, args):
    """positions by gid of the initial state, from a host-only simulation (no device)"""
    with pkg.Simulation(args, host_only=True) as sim:
        c, ng = sim.cells(), sim.n_global
    pos = np.zeros((ng, 3))
    for b in range(sim.n_local_boxes):
        for o in range(c["nAtoms"][b]):
            pos[c["gid"][b, o]] = (c["rx"][b, o], c["ry"][b, o], c["rz"][b, o])
    return pos


_SITES = {}


def _frenkel(pkg, pot, n, where):
    """(gid moved, positions with the Frenkel pair, the 12 gids around the vacated site): a site in the middle of the box, from host-only states"""
    if (pot, n, where) not in _SITES:
        sites = _host_positions(pkg, _cube(n) + POT[pot])
        pos = _host_positions(pkg, _cube(n) + ["-r", 0.1] + POT[pot])
        g = int(np.argmin(((sites - 0.5 * n * LAT + 0.25 * LAT) ** 2).sum(1)))
        pos[g] = sites[g] + np.array(INTERSTITIAL[where]) * LAT
        d = sites - sites[g]
        d -= np.rint(d / (n * LAT)) * (n * LAT)
        ring = np.argsort((d * d).sum(1))[1:13]
        pos.setflags(write=False)
        _SITES[(pot, n, where)] = (g, pos, np.sort(ring))
    return _SITES[(pot, n, where)]


# ---------------------------------------------------------------- CPU: flags, exports, ISA, the reference's own caps
def test_csp_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--csp', '--cspThreshold', 2.5, '--cspCoord', 3.0, '--cspFile', 'x.dat', '--cspDump', 'd.xyz'], "
                  "host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("csp", "cspThreshold", "cspCoord", "cspFile", "cspDump"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_centro_symmetry_is_exported_and_declared(sfx):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_hip{sfx}.so")], capture_output=True, text=True).stdout
    assert "computeCentroSymmetry" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_host{sfx}.so")], capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "comdCentroSymmetry" in names and "comdLatticeConstant" in names
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeCentroSymmetry\(SimGpu\* sim, real_t rCoord, real_t\* outCspBySlot, int\* outCoordBySlot\);", header, flags=re.M)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_centro_symmetry_kernels_use_no_scratch(precision):
    """... and CentroSym_thread_atom keeps the registers of its 4 waves per SIMD"""
    blocks = device_isa.blocks(precision, r"CentroSym\w+")
    assert len(blocks) >= 1 and any("CentroSym_thread_atom" in n for n in blocks), sorted(blocks)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    device_isa.assert_keeps_waves(blocks, "CentroSym_thread_atom", 4)


def test_host_only_simulation_refuses(pkg):
    with pkg.Simulation(_cube(6) + ADAMS, host_only=True) as sim:
        assert abs(sim.lattice_constant - LAT) <= 1e-15
        with pytest.raises(RuntimeError):
            sim.centro_symmetry()
        with pytest.raises(RuntimeError):
            sim.defects()


@pytest.mark.parametrize("where", ["close", "apart"])
@pytest.mark.parametrize("pot,n", [("adams", 6), ("lj5", 8)])
def test_frenkel_state_keeps_the_reference_inside_the_fp64_cap(pkg, pot, n, where):
    """The interstitial states of the GPU test, in numpy alone: no atom within DELTA64 of a tie or of rCoord, the moved atom above the default
    threshold and, with the pair apart, the 12 atoms around the vacated site too."""
    g, pos, ring = _frenkel(pkg, pot, n, where)
    ref = _reference(("frenkel", pot, n, where), pos, n * LAT, RC[pot], R_COORD, DELTA64)
    _left_out(ref, DELTA64, False)
    bad = set(np.nonzero(ref["csp"] > 0.25 * LAT * LAT)[0].tolist())
    print(f"{pot} {where}: csp of the moved atom {ref['csp'][g]:.3f}, of the ring {np.round(ref['csp'][ring], 3).tolist()}, defects {len(bad)}")
    assert g in bad and len(bad) < 60
    if where == "apart":
        assert set(ring.tolist()) <= bad


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("pot,n,method", [("lj5", 8, "thread_atom"), ("lj2.5", 8, "thread_atom"), ("adams", 6, "thread_atom"),
                                          ("mishin", 6, "thread_atom"), ("lj5", 8, "cta_cell"), ("adams", 6, "cta_cell")])
def test_matches_numpy(gpu, pot, n, method):
    """Step 0 and after 10 steps.  lj5: cells of several 64-slot chunks, 2 cells per axis; lj2.5 and EAM: the replicated small-chunk path."""
    with gpu.Simulation(_cube(n) + ["-r", 0.1, "-m", method] + POT[pot]) as sim:
        assert abs(sim.cutoff - RC[pot]) <= 1e-6 and abs(sim.lattice_constant - LAT) <= 1e-15
        _against_numpy(sim, n * LAT, RC[pot], key=(pot, n, 0))          # step 0: the state does not depend on the method
        sim.step(10)
        _against_numpy(sim, n * LAT, RC[pot])


@pytest.mark.gpu
def test_perfect_fcc_lattice(gpu):
    with gpu.Simulation(_cube(6) + ADAMS) as sim:
        csp, coord = sim.centro_symmetry()
        bad = sim.defects()
    assert csp.shape == (864,) and np.all(csp <= 1e-20) and np.all(coord == 12), (csp.max(), coord.min(), coord.max())
    assert bad.dtype == np.int64 and bad.size == 0


@pytest.mark.gpu
def test_one_displaced_atom(gpu):
    n, shift = 6, np.array([0.10, 0.05, -0.02])
    with gpu.Simulation(_cube(n) + ADAMS) as sim:
        pos = sim.gather(0)
        g = int(np.argmin(((pos - 0.5 * n * LAT + 0.25 * LAT) ** 2).sum(1)))
        d = pos - pos[g]
        d -= np.rint(d / (n * LAT)) * (n * LAT)
        ring = np.argsort((d * d).sum(1))[1:13]
        pos[g] += shift
        sim.scatter(0, pos)
        sim.redistribute()
        sim.compute_force()
        csp, coord = _against_numpy(sim, n * LAT, RC["adams"])
    want = 24.0 * float(shift @ shift)
    print(f"displaced atom: csp {csp[g]!r}, 24 |d|^2 {want!r}")
    assert abs(csp[g] - want) <= 1e-12
    assert np.all(csp[ring] > 1e-6) and np.all(coord == 12)
    rest = np.ones(len(csp), dtype=bool)
    rest[ring] = False
    rest[g] = False
    assert np.all(csp[rest] <= 1e-20)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["close", "apart"])
@pytest.mark.parametrize("pot,n", [("adams", 6), ("lj5", 8)])
def test_frenkel_pair(gpu, pot, n, where):
    g, pos, ring = _frenkel(gpu, pot, n, where)
    with gpu.Simulation(_cube(n) + ["-r", 0.1] + POT[pot]) as sim:
        sim.scatter(0, pos)
        sim.redistribute()
        sim.compute_force()
        assert np.array_equal(sim.gather(0), pos)
        csp, coord = _against_numpy(sim, n * LAT, RC[pot], key=("frenkel", pot, n, where))
        bad = sim.defects()
    ref = _REF[("frenkel", pot, n, where)]
    assert g in bad and (where == "close" or set(ring.tolist()) <= set(bad.tolist()))
    assert np.array_equal(bad, np.nonzero(ref["csp"] > 0.25 * LAT * LAT)[0])


@pytest.mark.gpu
def test_fewer_than_twelve_neighbours(gpu):
    with gpu.Simulation(SPARSE) as sim:
        assert sim.max_atoms == 16 and abs(sim.lattice_constant - 7.0) <= 1e-15
        pos = sim.gather(0)
        csp, coord = sim.centro_symmetry()                           # the default radius is the cutoff here: (1/sqrt 2 + 1) 7 / 2 lies beyond it
        bad = sim.defects()
        ng, rc = sim.n_global, sim.cutoff
    assert ng == 480 and abs(rc - RC["adams"]) <= 1e-6
    ref = _reference(None, pos, (28.0, 35.0, 42.0), rc, rc, DELTA64)
    _check(csp, coord, ref, what="eam_sparse")
    assert np.all(np.isinf(csp)) and 2 <= coord.min() and coord.max() <= 10, (coord.min(), coord.max())
    assert np.array_equal(bad, np.arange(ng, dtype=np.int64))


@pytest.mark.gpu
def test_coordination_counts_the_pairs_of_the_histogram(gpu):
    """The analysis kernels share one stencil walk, so they see one pair set: for a radius r handed to both, the coordination numbers add up to
    twice the unordered pairs the histogram counts below r.  Both test r2 < r * r on the same bits of r2: the identity is exact.  lj5: cells of
    several chunks, one partly filled and one empty; lj2.5 and EAM: replicated chunks; SPARSE: empty cells.  Each with one stream and with -a 1.
    (Measured on these states in both builds.  The float build rounds a pair across the periodic boundary differently from its two sides -- the
    shifted halo image -- so there one pair in 1e7 at the radius can be seen from one side only: met on a 20^3 thermal state, not on these.)"""
    states = [(_cube(8) + ["-r", 0.1] + POT["lj5"], "thread_atom"), (_cube(8) + ["-r", 0.1] + POT["lj2.5"], "thread_atom"),
              (_cube(6) + ["-r", 0.1] + ADAMS, "cta_cell"), (SPARSE, "thread_atom")]
    for args, method in states:
        for extra in ([], ["-a", 1]):
            with gpu.Simulation(args + ["-m", method] + extra) as sim:
                for r in sorted({min(0.5 * (np.sqrt(0.5) + 1.0) * sim.lattice_constant, sim.cutoff), sim.cutoff}):
                    coord = sim.centro_symmetry(r_coord=r)[1]
                    pairs = sim.pair_histogram(1, r_max=r)[1]
                    print(args, method, extra, f"r {r!r}: sum of coordination {int(coord.sum(dtype=np.int64))}, pairs {int(pairs.sum())}")
                    assert coord.sum(dtype=np.int64) > 0
                    assert int(coord.sum(dtype=np.int64)) == 2 * int(pairs.sum()), (args, method, extra, r)


@pytest.mark.gpu
@pytest.mark.parametrize("method,extra", [("thread_atom_nl", ["-S", 0.1]), ("cta_cell", ["-L", "-S", 0.03])])
def test_cells_that_are_not_rebinned(gpu, method, extra):
    """Between list builds the atoms keep their cells (sized cutoff + skin): the 27-cell walk still sees every neighbour within the cutoff."""
    n = 12
    with gpu.Simulation(_cube(n) + ["-T", 3000, "-m", method] + extra) as sim:
        sim.step(20)
        _against_numpy(sim, n * LAT, RC["lj5"])


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 12), ("mishin", 10)])
def test_methods_and_layouts_agree(gpu, pot, n):
    """Step 0, the same state and halo images under every method, cell size, cell numbering and stream mode: the same bits.  The 66 values do not
    depend on the order of the 12, and the 6 smallest are added in ascending order."""
    got = {}
    for method, extra in LJ_METHODS if pot.startswith("lj") else EAM_METHODS:
        with gpu.Simulation(_cube(n) + ["-r", 0.1, "-m", method] + extra + POT[pot]) as sim:
            got[" ".join([method] + [str(x) for x in extra])] = sim.centro_symmetry()
    first = got["thread_atom"]
    assert np.isfinite(first[0]).all() and first[0].max() > 0.0
    for name, (csp, coord) in got.items():
        assert np.array_equal(csp, first[0]) and np.array_equal(coord, first[1]), name


@pytest.mark.gpu
def test_arguments(gpu):
    n = 8
    with gpu.Simulation(_cube(n) + ["-r", 0.1]) as sim:
        before = sim.centro_symmetry()
        bad = sim.defects()
        for r_coord in (0.0, -1.0, float(np.nextafter(sim.cutoff, np.inf)), sim.cutoff * 1.001):
            with pytest.raises(ValueError):
                sim.centro_symmetry(r_coord)
            with pytest.raises(ValueError):
                sim.defects(None, r_coord)
        for threshold in (0.0, -2.0):
            with pytest.raises(ValueError):
                sim.defects(threshold)
        after = sim.centro_symmetry()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(bad, sim.defects())
        csp, coord = _against_numpy(sim, n * LAT, RC["lj5"], r_coord=sim.cutoff, key=("lj5", n, "cutoff"))
        assert np.array_equal(csp, before[0]) and coord.min() > 400
        assert np.array_equal(sim.defects(1e-3), np.nonzero(csp > 1e-3)[0]) and sim.defects(1e-3).size > sim.defects().size


def _same_cells(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj5", "adams"])
def test_purity_and_reproducibility(gpu, pot):
    args = _cube(8) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args) as sim:
        cells, energy = sim.cells(), sim.energy()
        a = sim.centro_symmetry()
        b = sim.centro_symmetry()
        sim.centro_symmetry(2.0)
        c = sim.centro_symmetry()
        assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) for k in (0, 1))
        assert _same_cells(cells, sim.cells()) and energy == sim.energy()
        for _ in range(5):
            sim.step(1)
            sim.centro_symmetry()
            sim.defects()
        with_calls = (sim.cells(), sim.energy())
    with gpu.Simulation(args) as sim:
        for _ in range(5):
            sim.step(1)
        assert _same_cells(with_calls[0], sim.cells()) and with_calls[1] == sim.energy()


def _ranks(tmp_path, grid, args, timeout=900):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    assert world <= 8
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "csp_worker.py"), str(r), str(world), port, *map(str, grid), str(tmp_path), json.dumps(args)],
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
        assert p.returncode == 0 and "CSP saved" in out, f"rank {r} failed:\n{out[-3000:]}"
    return [np.load(os.path.join(str(tmp_path), f"csp_rank{r}.npz")) for r in range(world)]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot,n", [("lj5", 14), ("adams", 8)])
def test_ranks_give_the_one_rank_result(gpu, tmp_path, grid, pot, n):
    """2 and 8 ranks sharing the device (gloo transport): every rank returns the same global arrays; coordination and the +inf mask are the
    one-rank ones, csp agrees within the fp64 tolerance (a rank boundary is one more shifted image)."""
    args = _cube(n) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args) as sim:
        csp0, coord0 = sim.centro_symmetry()
        bad0 = sim.defects()
    assert np.isfinite(csp0).all() and csp0.max() > 0.0
    got = _ranks(tmp_path, grid, args)
    for g in got:
        assert np.array_equal(g["csp"], got[0]["csp"]) and np.array_equal(g["coord"], got[0]["coord"]) and np.array_equal(g["defects"], got[0]["defects"])
    diff = np.abs(got[0]["csp"] - csp0)
    print(f"{grid} {pot}: largest |csp difference| to one rank {diff.max():.3e}")
    assert np.array_equal(got[0]["coord"], coord0) and np.array_equal(np.isinf(got[0]["csp"]), np.isinf(csp0))
    assert np.all(diff <= 1e-10 + 1e-12 * csp0) and np.array_equal(got[0]["defects"], bad0)


SINGLE_RUN = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    csp, coord = sim.centro_symmetry()
    np.savez({path!r}, pos=sim.gather(0), csp=csp, coord=coord, cutoff=sim.cutoff)
    sim.close()
    print("saved")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 8), ("adams", 6)])
def test_single_precision(gpu, tmp_path, pot, n):
    """The float build (COMD_PRECISION=single) against numpy on its own gathered positions, under the fp32 rules."""
    path = str(tmp_path / "sp.npz")
    proc = _child(SINGLE_RUN.format(args=_cube(n) + ["-r", 0.1] + POT[pot], path=path), env={"COMD_PRECISION": "single"})
    assert proc.returncode == 0 and "saved" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = np.load(path)
    assert abs(float(got["cutoff"]) - RC[pot]) <= 1e-6 * RC[pot]
    ref = _numpy_csp(got["pos"], n * LAT, float(got["cutoff"]), float(np.float32(R_COORD)), DELTA32)
    _check(got["csp"], got["coord"], ref, single=True, what=f"single {pot}")


def _comd_hip(tmp_path, extra, ok=True):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-d", os.path.join(ROOT, "pots")] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    text = ""
    for f in yaml:
        text = (tmp_path / f).read_text()
        os.remove(tmp_path / f)
    if not ok:
        return proc, [], text
    assert proc.returncode == 0 and len(yaml) == 1, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    return proc.stdout, rows, text


def _csp_file(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#") and not any(line.startswith("#") for line in lines[1:])
    return lines[0], np.array([[float(x) for x in line.split()] for line in lines[1:]])


def _row(csp, coord, threshold):
    finite = np.isfinite(csp)
    return [int((csp > threshold).sum()), int((~finite).sum()), float(csp[finite].mean()), float(csp[finite].max()), float(coord.mean()), int((coord != 12).sum())]


@pytest.mark.gpu
def test_comd_hip_csp(gpu, tmp_path):
    hot = ["-N", "20", "-n", "10", "-T", "3000"]
    with gpu.Simulation(["-x", 20, "-y", 20, "-z", 20, "-T", 3000]) as sim:
        first = sim.centro_symmetry()
        ng = sim.n_global
        sim.step(10)
        sim.step(10)
        last = sim.centro_symmetry()
        pos = sim.gather(0)
    threshold = float(np.median(last[0]))                               # half the atoms are "defects": the dump has something to say
    # one sample of the initial state: Python's
    _comd_hip(tmp_path, ["-N", "0", "--csp", "-T", "3000"])
    header, table = _csp_file(tmp_path / "csp.dat")
    assert re.search(rf"\bN {ng}\b", header) and re.search(r"\bsamples 1\b", header) and re.search(r"\bthreshold (\S+)", header), header
    assert abs(float(re.search(r"\bthreshold (\S+)", header).group(1)) - 0.25 * LAT * LAT) <= 1e-12
    assert abs(float(re.search(r"\brCoord (\S+)", header).group(1)) - R_COORD) <= 1e-12
    want = _row(first[0], first[1], 0.25 * LAT * LAT)
    assert table.shape == (1, 7) and table[0, 0] == 0 and [table[0, 1], table[0, 2], table[0, 6]] == [want[0], want[1], want[5]]
    assert abs(table[0, 3] - want[2]) <= 1e-10 * want[2] + 1e-300 and table[0, 4] == want[3] and abs(table[0, 5] - want[4]) <= 1e-12
    os.remove(tmp_path / "csp.dat")
    # without the flag: the report of before, and no file
    out0, rows0, yaml0 = _comd_hip(tmp_path, hot)
    assert [r[0] for r in rows0] == ["0", "10", "20"]
    assert "Defects" not in out0 and "CSP" not in out0 and "CSP" not in yaml0 and not re.search(r"^csp\s", out0, flags=re.M) and not re.search(r"Timer:\s+csp", yaml0)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".dat") or f.endswith(".xyz")]
    # three samples: the energies untouched to the bit, the YAML block, the timer row, the dump
    out1, rows1, yaml1 = _comd_hip(tmp_path, hot + ["--csp", "--cspFile", "x.dat", "--cspDump", "d.xyz", "--cspThreshold", repr(threshold)])
    assert [r[:3] for r in rows1] == [r[:3] for r in rows0] and "Defects" in out1
    assert re.search(r"^csp\s+3\s", out1, flags=re.M), out1[-3000:]
    header, table = _csp_file(tmp_path / "x.dat")
    assert re.search(r"\bsamples 3\b", header) and table.shape == (3, 7) and table[:, 0].tolist() == [0, 10, 20] and not os.path.exists(tmp_path / "csp.dat")
    assert [int(r[3].split()[-1]) for r in rows1] == table[:, 1].astype(int).tolist()
    block = re.search(r"^CSP:\n((?:  .*\n)+)", yaml1, flags=re.M)
    assert block, yaml1[-2000:]
    m = dict(re.findall(r"^  (\w+): (\S+)$", block.group(1), flags=re.M))
    assert set(m) == {"threshold", "rCoord", "samples", "file", "finalDefects", "finalMeanCsp"}
    want = _row(last[0], last[1], threshold)
    assert m["samples"] == "3" and m["file"] == "x.dat" and int(m["finalDefects"]) == want[0] == int(table[2, 1]) and 0 < want[0] < ng
    assert abs(float(m["threshold"]) - threshold) <= 1e-11 * threshold and abs(float(m["finalMeanCsp"]) - want[2]) <= 1e-10 * want[2]
    dump = open(tmp_path / "d.xyz").read().splitlines()
    assert int(dump[0]) == want[0] == len(dump) - 2 and "Properties=species:S:1:pos:R:3:csp:R:1:coordination:I:1:gid:I:1" in dump[1]
    atoms = [line.split() for line in dump[2:]]
    assert all(a[0] == "Cu" and len(a) == 7 for a in atoms)
    gids = np.array([int(a[6]) for a in atoms])
    assert np.array_equal(gids, np.nonzero(last[0] > threshold)[0])
    assert np.array_equal(np.array([float(a[4]) for a in atoms]), last[0][gids]) and np.array_equal(np.array([int(a[5]) for a in atoms]), last[1][gids])
    assert np.array_equal(np.array([[float(x) for x in a[1:4]] for a in atoms]), pos[gids])
    # refused before any step
    for bad in (["--cspCoord", "100"], ["--cspThreshold", "0"], ["--cspThreshold", "-1"], ["--cspCoord", "0"]):
        proc, _, _ = _comd_hip(tmp_path, hot + ["--csp"] + bad, ok=False)
        assert proc.returncode != 0 and re.search(r"^Error:", proc.stdout, flags=re.M) and not re.search(r"^\s+0\s+0\.00\s", proc.stdout, flags=re.M), proc.stdout[-1500:]
