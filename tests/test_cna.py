"""Adaptive common neighbour analysis (computeCommonNeighbors, comdCommonNeighbors, Simulation.common_neighbor_analysis / structure_counts,
comd-hip --cna).

CoMD has no structural analysis, so nothing here is compared with a recorded number.  The reference is an O(N^2) minimum-image computation on the
gathered positions in float64 numpy, which finds l_cb of every signature by a connected-component search (the kernel reads it off the degrees).  The
result is an integer and is compared exactly.  Three decisions are discrete, and the device (which subtracts shifted halo images) may round a
distance differently from numpy (which applies the minimum image); the reference returns per atom the `margin` by which they are taken, the least of

    the gap between the 13th and the 12th nearest distance         (which neighbour is the 12th)
    the least | |R_a - R_b| - r_loc | over the 66 pairs              (which neighbours are bonded)
    0 when the count of neighbours inside the cutoff passes 12 within DELTA of the cutoff ("unsure")

and an atom with margin < DELTA is left out.  DELTAs and caps are those of test_csp.py, asserted before anything is compared:

    build   DELTA      cap on the atoms left out
    fp64    1e-9 A     0
    fp32    1e-4 A     0.5 %
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
OTHER, FCC, HCP, ICO = 0, 1, 2, 4
LJ_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("cta_cell", ["-L", "-S", 0.03]), ("thread_atom_nl", []),
              ("thread_atom", ["-H"]), ("thread_atom", ["-a", 1]), ("cta_cell", ["-a", 1])]
EAM_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("thread_atom_nl", []), ("cta_cell", ["-H"]), ("cta_cell", ["-a", 1]),
               ("thread_atom", ["-a", 1])]                       # test_csp's lists
ICO_ARGS = ["-e", "-x", 4, "-y", 5, "-z", 6, "-l", 7.2]
ICO_EXTENT = (4 * 7.2, 5 * 7.2, 6 * 7.2)
ICO_CENTRE = np.array([17.3, 20.6, 21.65])                      # near the box centre and near a corner of the link cells: the 13 atoms spread over 8 cells


def _cube(n):
    return ["-x", n, "-y", n, "-z", n, "-l", repr(LAT)]


PRELUDE = f"import sys, json\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\n"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


# ---------------------------------------------------------------- numpy restatement
_PAIRS = np.triu_indices(12, 1)


def _largest_cluster(members, bonded):
    """bonds in the largest connected cluster of the bonds among `members`: a component search, not the kernel's degree rule"""
    left, best = set(members), 0
    while left:
        stack, seen = [left.pop()], set()
        while stack:
            u = stack.pop()
            seen.add(u)
            for w in members:
                if bonded[u, w] and w not in seen and w in left:
                    left.discard(w)
                    stack.append(w)
        comp = sorted(seen)
        best = max(best, sum(1 for i, u in enumerate(comp) for w in comp[i + 1:] if bonded[u, w]))
    return best


def _signature(a, bonded):
    members = [int(b) for b in np.nonzero(bonded[a])[0]]
    n_b = sum(1 for i, u in enumerate(members) for w in members[i + 1:] if bonded[u, w])
    return len(members), n_b, _largest_cluster(members, bonded)


def _classify(bonded):
    n_cn = bonded.sum(1)
    if not (np.all(n_cn == 4) or np.all(n_cn == 5)):                # every signature of a recognised type has 4, or every one has 5, common neighbours
        return OTHER
    sig = [_signature(a, bonded) for a in range(12)]
    if all(s == (4, 2, 1) for s in sig):
        return FCC
    if sorted(sig) == [(4, 2, 1)] * 6 + [(4, 2, 2)] * 6:
        return HCP
    if all(s == (5, 5, 5) for s in sig):
        return ICO
    return OTHER


def _numpy_cna(pos, extent, rc, delta):
    """dict of per-atom type and margin (module docstring), in blocks of 256 rows as test_csp._numpy_csp"""
    n = len(pos)
    extent = np.broadcast_to(np.asarray(extent, dtype=np.float64), (3,))
    types, margin = np.zeros(n, dtype=np.int32), np.full(n, np.inf)
    for s in range(0, n, 256):
        d = pos[None, :, :] - pos[s:s + 256, None, :]                # R = r_j - r_i
        d -= np.rint(d / extent) * extent
        r2 = (d * d).sum(-1)
        rows = np.arange(len(r2))
        r2[rows, s + rows] = np.inf                                   # j != i
        r = np.sqrt(r2)
        near = np.argpartition(r2, 13, axis=1)[:, :14]
        near = np.take_along_axis(near, np.argsort(np.take_along_axis(r2, near, axis=1), axis=1), axis=1)[:, :13]
        r13 = np.take_along_axis(r, near, axis=1)
        gap = r13[:, 12] - r13[:, 11]
        inside = (r < rc).sum(1)
        unsure = ((r < rc + delta).sum(1) >= 12) != ((r < rc - delta).sum(1) >= 12)
        vec = np.take_along_axis(d, near[:, :12, None], axis=1)       # (rows, 12, 3)
        total = r13[:, 0].copy()
        for k in range(1, 12):
            total += r13[:, k]                                        # ascending order
        r_loc = 0.5 * (1.0 + np.sqrt(2.0)) * (total / 12.0)
        sep = np.sqrt(((vec[:, :, None, :] - vec[:, None, :, :]) ** 2).sum(-1))          # (rows, 12, 12)
        bonded = sep <= r_loc[:, None, None]
        bonded[:, np.arange(12), np.arange(12)] = False
        pair = np.abs(sep[:, _PAIRS[0], _PAIRS[1]] - r_loc[:, None]).min(1)
        for i in range(len(r2)):
            if inside[i] >= 12:
                types[s + i] = _classify(bonded[i])
                margin[s + i] = min(gap[i], pair[i])
            if unsure[i]:
                margin[s + i] = 0.0
    out = {"type": types, "margin": margin}
    for a in out.values():
        a.setflags(write=False)
    return out


_REF = {}


def _reference(key, pos, extent, rc, delta):
    """computed once per key, never modified"""
    if key is None:
        return _numpy_cna(pos, extent, rc, delta)
    if key not in _REF:
        _REF[key] = _numpy_cna(pos, extent, rc, delta)
    return _REF[key]


def _left_out(ref, delta, single):
    n = len(ref["type"])
    out = ref["margin"] < delta
    cap = CAP32 * n if single else 0
    assert out.sum() <= cap, (int(out.sum()), n)
    return out


def _counts(types):
    return {"other": int((types == OTHER).sum()), "fcc": int((types == FCC).sum()), "hcp": int((types == HCP).sum()), "ico": int((types == ICO).sum())}


def _check(types, ref, single=False, what=""):
    assert types.dtype == np.int32 and types.shape == ref["type"].shape
    out = _left_out(ref, DELTA32 if single else DELTA64, single)
    finite = ref["margin"][np.isfinite(ref["margin"])]
    print(f"{what}: atoms {len(types)}, left out {int(out.sum())}, reference {_counts(ref['type'])}, least margin {finite.min() if finite.size else np.inf:.3e}")
    assert np.all(np.isin(types, (OTHER, FCC, HCP, ICO)))
    bad = np.nonzero((types != ref["type"]) & ~out)[0]
    assert bad.size == 0, (what, bad[:10].tolist(), types[bad[:10]].tolist(), ref["type"][bad[:10]].tolist())


def _against_numpy(sim, extent, rc, key=None, single=False):
    pos = sim.gather(0)
    types = sim.common_neighbor_analysis()
    assert abs(sim.cutoff - rc) <= 1e-6
    ref = _reference(key, pos, extent, sim.cutoff, DELTA32 if single else DELTA64)
    _check(types, ref, single, str(key))
    return types


def _host_positions(pkg, args):
    """positions by gid of the initial state, from a host-only simulation (no device)"""
    with pkg.Simulation(args, host_only=True) as sim:
        c, ng = sim.cells(), sim.n_global
    pos = np.zeros((ng, 3))
    for b in range(sim.n_local_boxes):
        for o in range(c["nAtoms"][b]):
            pos[c["gid"][b, o]] = (c["rx"][b, o], c["ry"][b, o], c["rz"][b, o])
    return pos


_STATES = {}


def _stacking_fault(pkg, n=8):
    """(positions, gids that must be HCP, gids that must be FCC): every atom above a plane halfway between two (111) planes in mid-box is shifted by
    lat/6 (1, 1, -2), wrapped, +-0.05 A of noise (the unperturbed state has exact ties).  The two sets: sites more than 1.5 lat from every box face,
    within 0.75 lat / sqrt 3 of the plane or not."""
    if ("fault", n) not in _STATES:
        sites = _host_positions(pkg, _cube(n) + ADAMS)
        height = sites.sum(1) / np.sqrt(3.0)                          # the CoMD basis puts the (111) planes at (k + 0.75) lat / sqrt 3
        plane = (1.5 * n + 0.25) * LAT / np.sqrt(3.0)
        pos = sites + np.where(height > plane, 1.0, 0.0)[:, None] * (LAT / 6.0) * np.array([1.0, 1.0, -2.0])
        pos += np.random.default_rng(20120521).uniform(-0.05, 0.05, pos.shape)
        pos = np.mod(pos, n * LAT)
        inner = np.all((sites > 1.5 * LAT) & (sites < (n - 1.5) * LAT), axis=1)
        close = np.abs(height - plane) < 0.75 * LAT / np.sqrt(3.0)
        pos.setflags(write=False)
        _STATES[("fault", n)] = (pos, np.nonzero(inner & close)[0], np.nonzero(inner & ~close)[0])
    return _STATES[("fault", n)]


def _icosahedron(pkg):
    """(positions, gid of the centre, gids of the 12 vertices): the sparse lattice (no atom has a neighbour inside the cutoff) with +-0.02 A of noise,
    the 13 atoms nearest ICO_CENTRE moved onto a centre and the 12 vertices of an icosahedron of radius 2.5 A"""
    if "ico" not in _STATES:
        pos = _host_positions(pkg, ICO_ARGS)
        rng = np.random.default_rng(2012)
        order = np.argsort(((pos - ICO_CENTRE) ** 2).sum(1))[:13]
        phi = 0.5 * (1.0 + np.sqrt(5.0))
        verts = np.array([p for a in (-1.0, 1.0) for b in (-phi, phi) for p in ((0.0, a, b), (a, b, 0.0), (b, 0.0, a))])
        verts *= 2.5 / np.sqrt(1.0 + phi * phi)
        pos[order[0]] = ICO_CENTRE
        pos[order[1:]] = ICO_CENTRE + verts
        pos += rng.uniform(-0.02, 0.02, pos.shape)
        pos.setflags(write=False)
        _STATES["ico"] = (pos, int(order[0]), np.sort(order[1:]))
    return _STATES["ico"]


def _apply(sim, pos):
    sim.scatter(0, pos)
    sim.redistribute()
    sim.compute_force()
    assert np.array_equal(sim.gather(0), pos)


# ---------------------------------------------------------------- CPU: flags, exports, ISA, the reference on the constructed states
def test_cna_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--cna', '--cnaFile', 'x.dat', '--cnaDump', 'd.xyz'], host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("cna", "cnaFile", "cnaDump"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_common_neighbors_is_exported_and_declared(sfx):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_hip{sfx}.so")], capture_output=True, text=True).stdout
    assert "computeCommonNeighbors" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_host{sfx}.so")], capture_output=True, text=True).stdout
    assert "comdCommonNeighbors" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computeCommonNeighbors\(SimGpu\* sim, int\* outTypeBySlot\);", header, flags=re.M)
    header = open(os.path.join(CSRC, "host", "comd_host.h")).read()
    assert re.search(r"^int comdCommonNeighbors\(SimFlat\* s, int\* typeByGid, long long counts\[5\]\);", header, flags=re.M)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_cna_kernels_use_no_scratch(precision):
    """... and Cna_thread_atom keeps the registers of its 4 waves per SIMD"""
    blocks = device_isa.blocks(precision, r"Cna_\w+")
    assert len(blocks) >= 1 and any("Cna_thread_atom" in n for n in blocks), sorted(blocks)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    device_isa.assert_keeps_waves(blocks, "Cna_thread_atom", 4)


def test_host_only_simulation_refuses(pkg):
    assert (pkg.CNA_OTHER, pkg.CNA_FCC, pkg.CNA_HCP, pkg.CNA_ICO) == (0, 1, 2, 4)
    with pkg.Simulation(_cube(6) + ADAMS, host_only=True) as sim:
        with pytest.raises(RuntimeError):
            sim.common_neighbor_analysis()
        with pytest.raises(RuntimeError):
            sim.structure_counts()


def test_constructed_states_in_numpy_alone(pkg):
    """Every constructed state of the GPU tests, from host-only positions: the reference's own caps and what each state is built to show, so that a
    failure on the GPU cannot be the reference's."""
    pos = _host_positions(pkg, _cube(6) + ADAMS)
    ref = _reference(("perfect", 6), pos, 6 * LAT, RC["adams"], DELTA64)
    _left_out(ref, DELTA64, False)
    assert np.all(ref["type"] == FCC) and ref["margin"].min() > 0.5, ref["margin"].min()
    for pot, n in (("lj5", 8), ("lj2.5", 8), ("adams", 6), ("mishin", 6)):
        pos = _host_positions(pkg, _cube(n) + ["-r", 0.3] + POT[pot])
        ref = _reference((pot, n, 0), pos, n * LAT, RC[pot], DELTA64)
        _left_out(ref, DELTA64, False)
        assert (ref["margin"] < DELTA32).sum() <= CAP32 * len(pos)
        c = _counts(ref["type"])
        print(pot, n, c, "under 1e-4:", int((ref["margin"] < DELTA32).sum()))
        assert c["fcc"] > 0.1 * len(pos) and c["other"] > 0.1 * len(pos), c
    pos, hcp, fcc = _stacking_fault(pkg)
    ref = _reference("fault", pos, 8 * LAT, RC["adams"], DELTA64)
    _left_out(ref, DELTA64, False)
    print("stacking fault:", len(hcp), "HCP and", len(fcc), "FCC sites inside;", _counts(ref["type"]))
    assert len(hcp) > 100 and len(fcc) > 300 and np.all(ref["type"][hcp] == HCP) and np.all(ref["type"][fcc] == FCC)
    pos, centre, verts = _icosahedron(pkg)
    ref = _reference("ico", pos, ICO_EXTENT, RC["adams"], DELTA64)
    _left_out(ref, DELTA64, False)
    print("icosahedron: margin of the centre", ref["margin"][centre])
    assert ref["type"][centre] == ICO and ref["margin"][centre] > 0.3 and _counts(ref["type"]) == {"other": 479, "fcc": 0, "hcp": 0, "ico": 1}


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("pot,n,method", [("lj5", 8, "thread_atom"), ("lj2.5", 8, "thread_atom"), ("adams", 6, "thread_atom"), ("adams", 6, "cta_cell"),
                                          ("mishin", 6, "thread_atom"), ("mishin", 6, "cta_cell")])
def test_matches_numpy(gpu, pot, n, method):
    """Step 0 and after 10 steps.  lj5: cells of several 64-slot chunks plus a tail chunk; lj2.5 and EAM: the replicated small-chunk path."""
    with gpu.Simulation(_cube(n) + ["-r", 0.3, "-m", method] + POT[pot]) as sim:
        types = _against_numpy(sim, n * LAT, RC[pot], key=(pot, n, 0))          # step 0: the state does not depend on the method
        c = _counts(types)
        assert c["fcc"] > 0.1 * len(types) and c["other"] > 0.1 * len(types), c
        assert sim.structure_counts() == c
        sim.step(10)
        _against_numpy(sim, n * LAT, RC[pot])


@pytest.mark.gpu
def test_perfect_fcc_lattice(gpu, tmp_path):
    with gpu.Simulation(_cube(6) + ADAMS) as sim:
        types = sim.common_neighbor_analysis()
        counts = sim.structure_counts()
    assert types.shape == (864,) and types.dtype == np.int32 and np.all(types == gpu.CNA_FCC)
    assert counts == {"other": 0, "fcc": 864, "hcp": 0, "ico": 0}
    out, rows, _ = _comd_hip(tmp_path, ["-e", "-N", "0", "--cna", "-x", "6", "-y", "6", "-z", "6"])
    assert "NonFCC" in out and len(rows) == 1 and rows[0][3].split()[-1] == "0", out[-2000:]


@pytest.mark.gpu
def test_stacking_fault(gpu):
    pos, hcp, fcc = _stacking_fault(gpu)
    with gpu.Simulation(_cube(8) + ADAMS) as sim:
        _apply(sim, pos)
        types = _against_numpy(sim, 8 * LAT, RC["adams"], key="fault")
        defects = sim.defects()
    print(f"stacking fault: {len(hcp)} HCP and {len(fcc)} FCC sites inside; device {_counts(types)}")
    assert len(hcp) > 100 and len(fcc) > 300
    assert np.all(types[hcp] == HCP) and np.all(types[fcc] == FCC)
    assert set(hcp.tolist()) <= set(defects.tolist())                 # centro-symmetry sees them as defects; CNA says which kind


@pytest.mark.gpu
def test_icosahedron(gpu):
    pos, centre, verts = _icosahedron(gpu)
    with gpu.Simulation(ICO_ARGS) as sim:
        _apply(sim, pos)
        pos_now = sim.gather(0)
        types = sim.common_neighbor_analysis()
        counts = sim.structure_counts()
        rc = sim.cutoff
    ref = _reference("ico", pos_now, ICO_EXTENT, rc, DELTA64)
    _check(types, ref, what="icosahedron")
    assert types[centre] == ICO and counts == {"other": 479, "fcc": 0, "hcp": 0, "ico": 1}


@pytest.mark.gpu
@pytest.mark.parametrize("method,extra", [("thread_atom_nl", ["-S", 0.1]), ("cta_cell", ["-L", "-S", 0.03])])
def test_cells_that_are_not_rebinned(gpu, method, extra):
    """Between list builds the atoms keep their cells (sized cutoff + skin): the 27-cell walk still sees every neighbour within the cutoff."""
    n = 10
    with gpu.Simulation(_cube(n) + ["-T", 3000, "-m", method] + extra) as sim:
        sim.step(10)
        _against_numpy(sim, n * LAT, RC["lj5"])


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 12), ("mishin", 10)])
def test_methods_and_layouts_agree(gpu, pot, n):
    """Step 0, the same state and halo images under every method, cell size, cell numbering and stream mode: the same integers."""
    got = {}
    for method, extra in LJ_METHODS if pot.startswith("lj") else EAM_METHODS:
        with gpu.Simulation(_cube(n) + ["-r", 0.3, "-m", method] + extra + POT[pot]) as sim:
            got[" ".join([method] + [str(x) for x in extra])] = sim.common_neighbor_analysis()
    first = got["thread_atom"]
    assert (first == FCC).any() and (first == OTHER).any()
    for name, types in got.items():
        assert np.array_equal(types, first), name


def _same_cells(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj5", "adams"])
def test_purity_and_reproducibility(gpu, pot):
    args = _cube(8) + ["-r", 0.3] + POT[pot]
    with gpu.Simulation(args) as sim:
        cells, energy = sim.cells(), sim.energy()
        csp = sim.centro_symmetry()
        a = sim.common_neighbor_analysis()
        b = sim.common_neighbor_analysis()
        after = sim.centro_symmetry()
        assert np.array_equal(a, b) and np.array_equal(csp[0], after[0]) and np.array_equal(csp[1], after[1])
        assert _same_cells(cells, sim.cells()) and energy == sim.energy()
        for _ in range(5):
            sim.step(1)
            sim.common_neighbor_analysis()
            sim.structure_counts()
        with_calls = (sim.gather(0), sim.energy())
    # the next steps' energies and positions by gid to the bit (the slot order inside a cell is not compared: at -r 0.3 atoms change cells
    # in these steps, and two plain runs of the EAM state differ in it)
    with gpu.Simulation(args) as sim:
        for _ in range(5):
            sim.step(1)
        assert np.array_equal(with_calls[0], sim.gather(0)) and with_calls[1] == sim.energy()


def _ranks(tmp_path, grid, args, timeout=900):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    assert world <= 8
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "cna_worker.py"), str(r), str(world), port, *map(str, grid), str(tmp_path), json.dumps(args)],
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
        assert p.returncode == 0 and "CNA saved" in out, f"rank {r} failed:\n{out[-3000:]}"
    return [np.load(os.path.join(str(tmp_path), f"cna_rank{r}.npz")) for r in range(world)]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot,n", [("lj5", 14), ("adams", 8)])
def test_ranks_give_the_one_rank_result(gpu, tmp_path, grid, pot, n):
    """2 and 8 ranks sharing the device (gloo transport): every rank returns the one-rank array and counts."""
    args = _cube(n) + ["-r", 0.3] + POT[pot]
    with gpu.Simulation(args) as sim:
        types0 = sim.common_neighbor_analysis()
        c = sim.structure_counts()
    assert c["fcc"] > 0 and c["other"] > 0
    for g in _ranks(tmp_path, grid, args):
        assert np.array_equal(g["types"], types0) and g["counts"].tolist() == [c["other"], c["fcc"], c["hcp"], c["ico"]]


SINGLE_RUN = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    types = sim.common_neighbor_analysis()
    np.savez({path!r}, pos=sim.gather(0), types=types, cutoff=sim.cutoff)
    sim.close()
    print("saved")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 8), ("adams", 6)])
def test_single_precision(gpu, tmp_path, pot, n):
    """The float build (COMD_PRECISION=single) against numpy on its own gathered positions, under the fp32 rules."""
    path = str(tmp_path / "sp.npz")
    proc = _child(SINGLE_RUN.format(args=_cube(n) + ["-r", 0.3] + POT[pot], path=path), env={"COMD_PRECISION": "single"})
    assert proc.returncode == 0 and "saved" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = np.load(path)
    assert abs(float(got["cutoff"]) - RC[pot]) <= 1e-6 * RC[pot]
    ref = _numpy_cna(got["pos"], n * LAT, float(got["cutoff"]), DELTA32)
    _check(got["types"], ref, single=True, what=f"single {pot}")


def _comd_hip(tmp_path, extra):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-d", os.path.join(ROOT, "pots")] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    text = ""
    for f in yaml:
        text = (tmp_path / f).read_text()
        os.remove(tmp_path / f)
    assert proc.returncode == 0 and len(yaml) == 1, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    return proc.stdout, rows, text


@pytest.mark.gpu
def test_comd_hip_cna(gpu, tmp_path):
    hot = ["-N", "20", "-n", "10", "-T", "3000", "-r", "0.3"]
    with gpu.Simulation(["-x", 20, "-y", 20, "-z", 20, "-T", 3000, "-r", 0.3]) as sim:
        ng = sim.n_global
        samples = [sim.structure_counts()]
        sim.step(10)
        samples.append(sim.structure_counts())
        sim.step(10)
        samples.append(sim.structure_counts())
        last = sim.common_neighbor_analysis()
        pos = sim.gather(0)
    assert 0 < samples[-1]["fcc"] < ng and _counts(last) == samples[-1]
    # without the flag: the report of before, and no file
    out0, rows0, yaml0 = _comd_hip(tmp_path, hot)
    assert [r[0] for r in rows0] == ["0", "10", "20"] and all(r[3].strip() == "" for r in rows0)
    assert "NonFCC" not in out0 and "CNA" not in out0 and "CNA" not in yaml0 and not re.search(r"^cna\s", out0, flags=re.M) and not re.search(r"Timer:\s+cna", yaml0)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".dat") or f.endswith(".xyz")]
    # three samples: the energies untouched to the bit, the column, the timer row, the file, the YAML block, the dump
    out1, rows1, yaml1 = _comd_hip(tmp_path, hot + ["--cna", "--cnaDump", "d.xyz"])
    assert [r[:3] for r in rows1] == [r[:3] for r in rows0] and "NonFCC" in out1
    assert re.search(r"^cna\s+3\s", out1, flags=re.M), out1[-3000:]
    assert [int(r[3].split()[-1]) for r in rows1] == [ng - s["fcc"] for s in samples]
    lines = open(tmp_path / "cna.dat").read().splitlines()
    assert lines[0].startswith("#") and re.search(rf"\bN {ng}\b", lines[0]) and re.search(r"\bsamples 3\b", lines[0]) and len(lines) == 4
    table = [[int(x) for x in line.split()] for line in lines[1:]]
    assert table == [[step, s["other"], s["fcc"], s["hcp"], s["ico"]] for step, s in zip((0, 10, 20), samples)]
    block = re.search(r"^CNA:\n((?:  .*\n)+)", yaml1, flags=re.M)
    assert block, yaml1[-2000:]
    m = dict(re.findall(r"^  (\w+): (\S+)$", block.group(1), flags=re.M))
    assert set(m) == {"samples", "file", "finalOther", "finalFCC", "finalHCP", "finalICO", "finalHCPFraction"}
    assert m["samples"] == "3" and m["file"] == "cna.dat"
    assert [int(m[k]) for k in ("finalOther", "finalFCC", "finalHCP", "finalICO")] == table[2][1:]
    assert abs(float(m["finalHCPFraction"]) - samples[-1]["hcp"] / ng) <= 1e-11
    dump = open(tmp_path / "d.xyz").read().splitlines()
    want = np.nonzero(last != FCC)[0]
    assert int(dump[0]) == len(want) == len(dump) - 2 and "Properties=species:S:1:pos:R:3:type:I:1:gid:I:1" in dump[1]
    atoms = [line.split() for line in dump[2:]]
    assert all(a[0] == "Cu" and len(a) == 6 for a in atoms)
    gids = np.array([int(a[5]) for a in atoms])
    assert np.array_equal(gids, want) and np.array_equal(np.array([int(a[4]) for a in atoms]), last[gids])
    assert np.array_equal(np.array([[float(x) for x in a[1:4]] for a in atoms]), pos[gids])
    for f in ("cna.dat", "d.xyz"):
        os.remove(tmp_path / f)
    # with --csp: both columns, the csp one as it is without --cna
    out2, rows2, _ = _comd_hip(tmp_path, hot + ["--csp"])
    out3, rows3, yaml3 = _comd_hip(tmp_path, hot + ["--csp", "--cna"])
    assert re.search(r"Defects\s+NonFCC\s*$", out3, flags=re.M) and "CSP:" in yaml3 and "CNA:" in yaml3
    assert [r[:3] for r in rows3] == [r[:3] for r in rows0]
    assert [r[3].split()[0] for r in rows3] == [r[3].split()[0] for r in rows2] and [r[3].split()[1] for r in rows3] == [r[3].split()[-1] for r in rows1]
