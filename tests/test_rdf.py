"""The pair-distance histogram and g(r) (computePairHistogram, comdPairHistogram, Simulation.pair_histogram / rdf, comd-hip --rdf).

CoMD has no structural analysis, so nothing here is compared with a recorded number.  The reference is an O(N^2) minimum-image histogram of
the gathered positions in float64 numpy.  Counts are integers and the comparison is exact, with one exception: a pair whose reference
distance lies within DELTA of a bin edge may fall on either side of it (the device subtracts shifted halo images, numpy applies the minimum
image).  For every edge k the cumulative counts may therefore differ by at most near[k], the number of reference pairs within DELTA of
that edge -- and the sum of near[] is itself capped, so that a loose input fails instead of hiding a miscount:

    build   DELTA      cap on sum(near)
    fp64    1e-9 A     0                  (the comparison is plain array_equal)
    fp32    1e-4 A     0.5 % of the pairs
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
RC = {"lj5": 5.0 * SIGMA, "lj2.5": 2.5 * SIGMA, "adams": 4.95, "mishin": 5.506786}      # mishin: the cutoff in the header of Cu01.eam.alloy
POT = {"lj5": [], "lj2.5": ["--ljCutoffSigmas", 2.5], "adams": ADAMS, "mishin": MISHIN}
DELTA64, DELTA32, CAP32 = 1e-9, 1e-4, 0.005


def _cube(n):
    return ["-x", n, "-y", n, "-z", n, "-l", repr(LAT)]


PRELUDE = f"import sys, json\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\n"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


# ---------------------------------------------------------------- CPU: flags, exports, ISA
def test_rdf_flags_are_listed_and_accepted_host_only(pkg):
    proc = _child("pkg.Simulation(['-x', 8, '-y', 8, '-z', 8, '--rdf', 64, '--rdfMax', 6.5, '--rdfFile', 'x.dat'], host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout and "invalid switch" not in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    proc = _child("pkg.Simulation(['--help'], host_only=True)")
    for flag in ("rdf", "rdfMax", "rdfFile"):
        assert re.search(rf"^\s+--{flag}\s", proc.stdout, flags=re.M), (flag, proc.stdout[-3000:])


@pytest.mark.parametrize("sfx", ["", "_sp"])
def test_pair_histogram_is_exported_and_declared(sfx):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_hip{sfx}.so")], capture_output=True, text=True).stdout
    assert "computePairHistogram" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, f"libcomd_host{sfx}.so")], capture_output=True, text=True).stdout
    assert "comdPairHistogram" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "comd_hip.h")).read()
    assert re.search(r"^void computePairHistogram\(SimGpu\* sim, int nBins, real_t rMax, uint64_t\* outCounts\);", header, flags=re.M)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_pair_histogram_kernels_use_no_scratch(precision):
    """... and PairHist_thread_atom keeps the registers of its 7 (double) or 8 (single) waves per SIMD"""
    blocks = device_isa.blocks(precision, r"PairHist_\w+")
    assert len(blocks) >= 1 and any("PairHist_thread_atom" in n for n in blocks), sorted(blocks)
    for name, block in blocks.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name
    device_isa.assert_keeps_waves(blocks, "PairHist_thread_atom", {"double": 7, "single": 8}[precision])


def test_halved_counts_keep_every_pair(pkg):
    """A pair seen in two neighbouring bins from its two sides leaves halves: it goes whole into the upper bin, whatever the parity of the rest."""
    for halved, want in (([10.5, 8.5, 3.0], [10, 9, 3]), ([9.5, 7.5, 3.0], [9, 8, 3]), ([0.5, 0.5, 0.0, 1.5, 2.5], [0, 1, 0, 1, 3]), ([4.0, 0.0, 7.0], [4, 0, 7])):
        got = pkg._whole_pairs(np, np.array(halved))
        assert got.dtype == np.int64 and got.tolist() == want and got.sum() == sum(halved)


# ---------------------------------------------------------------- numpy restatement
def _distances(pos, extent, rc):
    """sorted distances of all ordered pairs i != j with r < rc under the minimum image (every unordered pair appears twice, with the same bits);
    extent: the edge of a cube, or the three extents of the box"""
    extent = np.broadcast_to(np.asarray(extent, dtype=np.float64), (3,))
    out = []
    for s in range(0, len(pos), 256):
        d = pos[s:s + 256, None, :] - pos[None, :, :]
        d -= np.rint(d / extent) * extent
        r2 = (d * d).sum(-1)
        out.append(np.sqrt(r2[(r2 > 0.0) & (r2 < rc * rc)]))
    return np.sort(np.concatenate(out))


_REF = {}


def _reference(key, pos, extent, edges, delta):
    """(cum, near): unordered reference pairs below each edge, and within delta of each edge.  Computed once per key, never modified."""
    if key not in _REF:
        r = _distances(pos, extent, edges[-1] + 2.0 * delta)
        cum = np.searchsorted(r, edges, side="left")
        near = np.searchsorted(r, edges + delta, side="right") - np.searchsorted(r, edges - delta, side="left")
        assert np.all(cum % 2 == 0) and np.all(near % 2 == 0)
        cum, near = cum // 2, near // 2
        cum.setflags(write=False)
        near.setflags(write=False)
        _REF[key] = (cum, near)
    return _REF[key]


def _check(counts, cum, near, single=False, what=""):
    """the comparison rule of the module docstring"""
    got = np.concatenate([[0], np.cumsum(counts)])
    total = int(cum[-1])
    print(f"{what}: pairs {total}, near-edge {int(near.sum())}, largest |cum difference| {int(np.abs(got - cum).max())}")
    assert total > 0
    assert near.sum() <= (CAP32 * total if single else 0), (what, int(near.sum()), total)
    assert np.all(np.abs(got - cum) <= near), (what, np.nonzero(np.abs(got - cum) > near)[0][:10], got[-1], cum[-1])
    if not single:
        assert np.array_equal(counts, np.diff(cum)), what


def _against_numpy(sim, n, bins, r_max=None, key=None, single=False):
    pos = sim.gather(0)
    edges, counts = sim.pair_histogram(bins, r_max)
    assert edges.dtype == np.float64 and edges.shape == (bins + 1,) and counts.dtype == np.int64 and counts.shape == (bins,)
    assert edges[0] == 0.0 and abs(edges[-1] - (sim.cutoff if r_max is None else r_max)) <= 1e-15 * edges[-1]
    cum, near = _reference(key, pos, n * LAT, edges, DELTA32 if single else DELTA64) if key else _reference(object(), pos, n * LAT, edges, DELTA64)
    _check(counts, cum, near, single, str(key))
    return counts


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("pot,n,bins,method", [("lj5", 8, 64, "thread_atom"), ("lj2.5", 8, 40, "thread_atom"), ("adams", 6, 48, "thread_atom"),
                                               ("mishin", 6, 48, "thread_atom"), ("lj5", 8, 64, "cta_cell"), ("adams", 6, 48, "cta_cell")])
def test_counts_match_numpy(gpu, pot, n, bins, method):
    """Step 0 and after 10 steps.  lj5: cells of several 64-slot chunks; lj2.5 and EAM: the replicated small-chunk path."""
    with gpu.Simulation(_cube(n) + ["-r", 0.1, "-m", method] + POT[pot]) as sim:
        assert abs(sim.cutoff - RC[pot]) <= 1e-6
        _against_numpy(sim, n, bins, key=(pot, n, bins, 0))          # step 0: the state does not depend on the method
        sim.step(10)
        _against_numpy(sim, n, bins)


@pytest.mark.gpu
def test_perfect_fcc_lattice(gpu):
    n, bins = 6, 48
    with gpu.Simulation(_cube(n) + ADAMS) as sim:
        edges, counts = sim.pair_histogram(bins)
        r, g = sim.rdf(bins)
        ng = sim.n_global
    assert ng == 4 * n ** 3
    dr = RC["adams"] / bins
    want = np.zeros(bins, dtype=np.int64)
    for shell, pairs in ((LAT / np.sqrt(2.0), 6 * ng), (LAT, 3 * ng), (LAT * np.sqrt(1.5), 12 * ng)):
        want[int(shell / dr)] = pairs
    assert np.array_equal(counts, want), (counts, want)
    assert 2 * counts.sum() == 42 * ng
    k = np.arange(bins, dtype=np.float64)
    volume = (n * LAT) ** 3
    g_want = counts / ((ng / 2.0) * (ng / volume) * (4.0 * np.pi / 3.0) * ((k + 1.0) ** 3 - k ** 3) * dr ** 3)
    assert np.allclose(r, (k + 0.5) * dr, rtol=1e-14, atol=0.0)
    assert np.all(np.abs(g - g_want) <= 1e-14 * g_want), np.abs(g - g_want).max()


@pytest.mark.gpu
@pytest.mark.parametrize("method,extra", [("thread_atom_nl", ["-S", 0.1]), ("cta_cell", ["-L", "-S", 0.03])])
def test_cells_that_are_not_rebinned(gpu, method, extra):
    """Between list builds the atoms keep their cells (sized cutoff + skin): the 27-cell walk still sees every pair within the cutoff."""
    n = 12
    with gpu.Simulation(_cube(n) + ["-T", 3000, "-m", method] + extra) as sim:
        sim.step(20)
        _against_numpy(sim, n, 64)


LJ_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("cta_cell", ["-L", "-S", 0.03]), ("thread_atom_nl", []),
              ("thread_atom", ["-H"]), ("thread_atom", ["-a", 1]), ("cta_cell", ["-a", 1])]
EAM_METHODS = [("thread_atom", []), ("warp_atom", []), ("cta_cell", []), ("thread_atom_nl", []), ("cta_cell", ["-H"]), ("cta_cell", ["-a", 1]),
               ("thread_atom", ["-a", 1])]


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n", [("lj5", 12), ("mishin", 10)])
def test_methods_and_layouts_agree(gpu, pot, n):
    """Step 0, the same state under every method, cell size, cell numbering and stream mode: the same counts."""
    got = {}
    for method, extra in LJ_METHODS if pot.startswith("lj") else EAM_METHODS:
        with gpu.Simulation(_cube(n) + ["-r", 0.1, "-m", method] + extra + POT[pot]) as sim:
            got[" ".join([method] + [str(x) for x in extra])] = sim.pair_histogram(64)[1]
    assert got["thread_atom"].sum() > 0
    for name, counts in got.items():
        assert np.array_equal(counts, got["thread_atom"]), name


@pytest.mark.gpu
def test_arguments(gpu):
    """4096 bins: of P pairs spread over a range R, 2 DELTA64 P bins / R lie within DELTA64 of an edge -- 0.4 expected for lj5 8^3 (568,456
    pairs up to 11.6 A), 0.08 for lj2.5 8^3 and 0.03 for adams 6^3.  The -r 0.1 state of lj5 8^3 has two such reference pairs, which the cap
    on sum(near) refuses; its -r 0.08 state has none (counted in numpy alone), so the cells of several chunks run 4096 bins on that one."""
    for pot, n, amp in (("lj5", 8, 0.08), ("lj2.5", 8, 0.1), ("adams", 6, 0.1)):
        with gpu.Simulation(_cube(n) + ["-r", amp] + POT[pot]) as sim:
            _against_numpy(sim, n, 4096, key=(pot, n, 4096, amp))
    n = 8
    with gpu.Simulation(_cube(n) + ["-r", 0.1]) as sim:
        _against_numpy(sim, n, 1, key=("lj5", n, 1, 0))
        _against_numpy(sim, n, 30, r_max=3.0, key=("lj5", n, 30, 3.0))
        before = sim.pair_histogram(64)[1]
        for bins, r_max in ((64, float(np.nextafter(sim.cutoff, np.inf))), (64, sim.cutoff * 1.001), (64, 0.0), (64, -1.0), (0, None), (4097, None), (-3, None)):
            with pytest.raises(ValueError):
                sim.pair_histogram(bins, r_max)
            with pytest.raises(ValueError):
                sim.rdf(bins, r_max)
        assert np.array_equal(sim.pair_histogram(64)[1], before)
        assert np.array_equal(sim.pair_histogram(64, sim.cutoff)[1], before)


def _same_cells(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.gpu
@pytest.mark.parametrize("pot", ["lj5", "adams"])
def test_purity_and_reproducibility(gpu, pot):
    args = _cube(8) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args) as sim:
        cells, energy = sim.cells(), sim.energy()
        a = sim.pair_histogram(64)
        b = sim.pair_histogram(64)
        sim.pair_histogram(1000)
        c = sim.pair_histogram(64)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], c[1])
        assert _same_cells(cells, sim.cells()) and energy == sim.energy()
        for _ in range(5):
            sim.step(1)
            sim.pair_histogram(64)
            sim.rdf(200)
        with_calls = (sim.cells(), sim.energy())
    with gpu.Simulation(args) as sim:
        for _ in range(5):
            sim.step(1)
        assert _same_cells(with_calls[0], sim.cells()) and with_calls[1] == sim.energy()


def _ranks(grid, bins, args, timeout=900):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    world = grid[0] * grid[1] * grid[2]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "rdf_worker.py"), str(r), str(world), port, *map(str, grid), str(bins), json.dumps(args)],
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
    return [json.loads(re.search(r"^PAIRHIST (.*)$", out, flags=re.M).group(1)) for out in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("pot,n", [("lj5", 14), ("adams", 8)])
def test_ranks_give_the_one_rank_counts(gpu, grid, pot, n):
    """2 and 8 ranks sharing the device (gloo transport): every rank returns the global counts, exactly the one-rank ones."""
    args = _cube(n) + ["-r", 0.1] + POT[pot]
    with gpu.Simulation(args) as sim:
        edges0, counts0 = sim.pair_histogram(64)
    assert counts0.sum() > 0
    for edges, counts in _ranks(grid, 64, args):
        assert np.array_equal(np.array(edges), edges0)
        assert np.array_equal(np.array(counts, dtype=np.int64), counts0)


SINGLE_RUN = """
    import numpy as np
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation({args!r})
    edges, counts = sim.pair_histogram({bins})
    np.savez({path!r}, pos=sim.gather(0), edges=edges, counts=counts)
    sim.close()
    print("saved")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("pot,n,bins", [("lj5", 8, 64), ("adams", 6, 48)])
def test_single_precision(gpu, tmp_path, pot, n, bins):
    """The float build (COMD_PRECISION=single) against numpy on its own gathered positions, under the DELTA = 1e-4 rule."""
    path = str(tmp_path / "sp.npz")
    proc = _child(SINGLE_RUN.format(args=_cube(n) + ["-r", 0.1] + POT[pot], bins=bins, path=path), env={"COMD_PRECISION": "single"})
    assert proc.returncode == 0 and "saved" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = np.load(path)
    assert abs(got["edges"][-1] - RC[pot]) <= 1e-6 * RC[pot]
    cum, near = _reference(object(), got["pos"], n * LAT, got["edges"], DELTA32)
    _check(got["counts"], cum, near, single=True, what=f"single {pot}")


def _comd_hip(tmp_path, extra):
    proc = subprocess.run([os.path.join(CSRC, "comd-hip"), "-d", os.path.join(ROOT, "pots")] + extra, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d+\s+\S+\s+\S+\s+\S+\s+\S+)\s+\S+\s+(\d+)(.*)$", proc.stdout, flags=re.M)
    yaml = [f for f in os.listdir(tmp_path) if f.startswith("CoMD-hip") and f.endswith(".yaml")]
    assert len(yaml) == 1
    text = (tmp_path / yaml[0]).read_text()
    os.remove(tmp_path / yaml[0])
    return proc.stdout, rows, text


def _rdf_file(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#") and not any(line.startswith("#") for line in lines[1:])
    return lines[0], np.array([[float(x) for x in line.split()] for line in lines[1:]])


@pytest.mark.gpu
def test_comd_hip_rdf(gpu, tmp_path):
    # one sample of the initial state: Python's g(r)
    _comd_hip(tmp_path, ["-N", "0", "--rdf", "64"])
    header, table = _rdf_file(tmp_path / "rdf.dat")
    with gpu.Simulation(["-x", 20, "-y", 20, "-z", 20]) as sim:
        r, g = sim.rdf(64)
        edges, counts = sim.pair_histogram(64)
        ng = sim.n_global
    assert re.search(r"\bbins 64\b", header) and re.search(r"\bsamples 1\b", header) and re.search(rf"\bN {ng}\b", header), header
    assert table.shape == (64, 4)
    assert np.all(np.abs(table[:, 0] - r) <= 1e-12 * r)
    assert g.max() > 1.0 and np.all(np.abs(table[:, 1] - g) <= 1e-12 * g)
    assert np.array_equal(table[:, 3], counts.astype(np.float64))
    assert np.all(np.abs(table[:, 2] - 2.0 * np.cumsum(counts) / ng) <= 1e-12 * table[-1, 2])
    os.remove(tmp_path / "rdf.dat")
    # without the flag: the report of before, and no file
    run = ["-N", "20", "-n", "10"]
    out0, rows0, yaml0 = _comd_hip(tmp_path, run)
    assert [r[0] for r in rows0] == ["0", "10", "20"]
    assert not re.search(r"^rdf\s", out0, flags=re.M) and "RDF" not in out0 and "RDF" not in yaml0 and not re.search(r"Timer:\s+rdf", yaml0)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".dat")]
    # three samples: the energies untouched to the bit, the YAML block, the timer row
    out1, rows1, yaml1 = _comd_hip(tmp_path, run + ["--rdf", "64", "--rdfFile", "x.dat"])
    assert rows1 == rows0
    assert re.search(r"^rdf\s+3\s", out1, flags=re.M), out1[-3000:]
    header, table = _rdf_file(tmp_path / "x.dat")
    assert re.search(r"\bsamples 3\b", header) and table.shape == (64, 4) and not os.path.exists(tmp_path / "rdf.dat")
    block = re.search(r"^RDF:\n((?:  .*\n)+)", yaml1, flags=re.M)
    assert block, yaml1[-2000:]
    m = dict(re.findall(r"^  (\w+): (\S+)$", block.group(1), flags=re.M))
    assert set(m) == {"bins", "rMax", "samples", "file", "rOfHighestG"}
    assert m["bins"] == "64" and m["samples"] == "3" and m["file"] == "x.dat" and abs(float(m["rMax"]) - RC["lj5"]) <= 1e-9
    assert abs(float(m["rOfHighestG"]) - table[np.argmax(table[:, 1]), 0]) <= 1e-9
