"""-I: Lennard-Jones by table interpolation (the reference's initLJinterpolation, gpu_utility.c:349-372, and
LJ_Force_thread_atom_interpolation, gpu_lj_thread_atom.h:145-226) on thread_atom, warp_atom and thread_atom_nl.

The checker has no -I, so the restatement lives here: the table in numpy, the quadratic interpolate() of gpu_common.h:48-86, all pairs
under the minimum image.  Every simulation with -I in the CPU part is made in a child process: a build without the feature exits on the
flag, which must fail one test, not end the session.
"""
import ctypes
import json
import math
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "comd-cuda-async_amd", "csrc")
G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_values.json")))
SINGLE = os.environ.get("COMD_PRECISION", "double") == "single"
TOL = G["tolerances_single" if SINGLE else "tolerances"]

SIGMA, EPS, LAT = 2.315, 0.167, 3.615            # ljForce.c:102-120 (Cu), lattice constant 3.615 A
N_TABLE = 1000


# ---------------------------------------------------------------- the restatement
def lj_table(cutoff_sigmas=5.0):
    """gpu_utility.c:349-372 with one trailing pad: (x0, invDx, n + 4 values), values[0] the sample at x0 - dx."""
    sigma, eps = SIGMA, EPS
    cutoff = cutoff_sigmas * sigma
    x0 = 0.5 * sigma
    inv = N_TABLE / (cutoff - x0)
    rc2 = cutoff * cutoff
    s6 = sigma * sigma * sigma * sigma * sigma * sigma
    rc6 = s6 / (rc2 * rc2 * rc2)
    shift = rc6 * (rc6 - 1.0)
    i = np.arange(N_TABLE + 3)
    x = x0 + (i - 1) / inv
    r2 = 1.0 / (x * x)
    r6 = s6 * r2 * r2 * r2
    v = 4 * eps * (r6 * (r6 - 1.0) - shift)
    return x0, inv, np.append(v, v[-1])


def interpolate(table, r):
    """gpu_common.h:48-86, vectorised: value and derivative."""
    x0, inv, v = table
    xn = x0 + N_TABLE / inv
    r = np.minimum(np.maximum(r, x0), xn)
    r = r * inv - inv * x0
    ri = np.floor(r)
    ii = ri.astype(np.int64)
    r = r - ri
    v0, v1, v2, v3 = v[ii], v[ii + 1], v[ii + 2], v[ii + 3]
    g1, g2 = v2 - v0, v3 - v1
    return v1 + 0.5 * r * (g1 + r * (v2 + v0 - 2.0 * v1)), (g1 + r * (g2 - g1)) * (inv * 0.5)


def restated_forces(pos, extent, table, cutoff):
    """All pairs, minimum image (boxes wider than two cutoffs): per-atom force and energy."""
    f = np.zeros_like(pos)
    e = np.zeros(len(pos))
    for s in range(0, len(pos), 512):
        d = pos[s:s + 512, None, :] - pos[None, :, :]
        d -= np.rint(d / extent) * extent
        r2 = (d * d).sum(-1)
        hit = (r2 > 0.0) & (r2 <= cutoff * cutoff)
        r = np.sqrt(np.where(hit, r2, 1.0))
        v, dv = interpolate(table, r)
        v, fr = np.where(hit, v, 0.0), np.where(hit, -dv / r, 0.0)
        e[s:s + 512] = 0.5 * v.sum(1)
        f[s:s + 512] = (fr[..., None] * d).sum(1)
    return f, e


def _args(n, delta, method, extra=()):
    nx, ny, nz = (n, n, n) if isinstance(n, int) else n
    return ["-x", nx, "-y", ny, "-z", nz, "-r", delta, "-m", method, "-I"] + list(extra)


# ---------------------------------------------------------------- CPU: flags, table, ISA, export
PRELUDE = f"import sys\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as ge\npkg = ge.load_package()\n"


def _child(code, env=None, timeout=300):
    return subprocess.run([sys.executable, "-c", PRELUDE + textwrap.dedent(code)], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("method", ["thread_atom", "warp_atom", "thread_atom_nl"])
def test_flag_is_accepted_on_the_thread_atom_methods(method):
    proc = _child(f"pkg.Simulation({_args(8, 0.0, method)!r}, host_only=True).close(); print('made')")
    assert proc.returncode == 0 and "made" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-2000:]


@pytest.mark.parametrize("extra,reason", [(["-m", "thread_atom", "-e"], "EAM"), (["-m", "cta_cell"], "cta_cell"), (["-m", "cta_cell", "-L"], "cta_cell")])
def test_flag_is_refused_where_it_would_not_be_computed(extra, reason):
    """-e (the reference has no EAM table path for -I) and cta_cell (the reference silently runs the analytic kernel there)."""
    proc = _child(f"pkg.Simulation({['-x', 8, '-y', 8, '-z', 8, '-I'] + extra!r}, host_only=True); print('made')")
    assert proc.returncode != 0 and "made" not in proc.stdout
    lines = [l for l in (proc.stdout + proc.stderr).splitlines() if l.startswith("Error")]
    assert len(lines) == 1 and "-I" in lines[0] and reason in lines[0], proc.stdout[-2000:]


@pytest.mark.parametrize("sigmas", [5.0, 2.5])
def test_table_is_the_reference_table(tmp_path, sigmas):
    """lj_table() is gpu_utility.c:349-372 to the bit (5 sigma and --ljCutoffSigmas 2.5), plus the trailing pad; xn is the cutoff."""
    out = tmp_path / "table.npy"
    proc = _child(f"""
        import numpy as np
        sim = pkg.Simulation({_args(10, 0.0, 'thread_atom', ['--ljCutoffSigmas', sigmas])!r}, host_only=True)
        x0, inv, v = sim.lj_table()
        np.save({str(out)!r}, np.concatenate([[x0, inv], v]))
        sim.close()
    """)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    got = np.load(out)
    x0, inv, v = lj_table(sigmas)
    assert (got[0], got[1]) == (x0, inv)
    assert len(got) - 2 == N_TABLE + 4 and np.array_equal(got[2:], v)
    assert got[-1] == got[-2]                                    # the pad a pair at r == xn reads
    if sigmas == 5.0:
        assert x0 + N_TABLE / inv == 5.0 * SIGMA                 # such a pair exists: xn is the cutoff exactly


def test_no_table_without_the_flag(pkg):
    sim = pkg.Simulation(["-x", 8, "-y", 8, "-z", 8], host_only=True)
    assert sim.lj_table() is None
    sim.close()


@pytest.fixture(scope="module")
def device_isa():
    import device_isa as isa
    return isa.assembly("double")


def test_table_kernel_keeps_the_scalar_load_stream(device_isa):
    """As test_lj_thread_atom_keeps_its_scalar_load_stream for the analytic kernel: the table gather must not cost the s_load stream."""
    kernels = re.findall(r"^(_Z26LJ_Force_thread_atom_tableILb[01]ELb([01])EEv6LjArgsi11LjWaveLists9TableView):[^\n]*\n(.*?)s_endpgm",
                         device_isa, flags=re.S | re.M)
    assert len(kernels) == 4
    for name, listed, body in kernels:
        assert body.count("s_load_dwordx16") >= 3, name
        if listed == "1":
            assert len(re.findall(r"s_load_dwordx8 s\[\d+:\d+\], s\[\d+:\d+\], s\d+", body)) >= 16, name


def test_table_kernels_use_no_scratch(device_isa):
    blocks = re.findall(r"^\s*\.amdhsa_kernel (_Z\d+LJ_Force_(?:thread_atom|nl_slabs|thread_atom_nl)_table\w+)\n(.*?)\.end_amdhsa_kernel", device_isa, flags=re.S | re.M)
    assert len(blocks) == 8, [b[0] for b in blocks]
    for name, block in blocks:
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", block), name


def test_init_lj_interpolation_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, "libcomd_hip.so")], capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"initLJinterpolation", "comdLjInterpolationTable"} <= defined


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n,delta", [(10, 0.1), ((10, 14, 11), 0.2)])
@pytest.mark.parametrize("leg", ["thread_atom-lists", "prune-off", "one-wave", "list-cap-8", "thread_atom_nl"])
def test_one_evaluation_matches_the_restatement(gpu, monkeypatch, n, delta, leg):
    env = {"prune-off": {"COMD_LJ_PRUNE": "0"}, "one-wave": {"COMD_LJ_WAVES": "1"}, "list-cap-8": {"COMD_LJ_LIST_CAP": "8"}}.get(leg, {})
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    method = "thread_atom_nl" if leg == "thread_atom_nl" else "thread_atom"
    with gpu.Simulation(_args(n, delta, method)) as sim:
        pos, f, e = sim.gather(0), sim.gather(2), sim.gather(3)
    extent = np.array([n, n, n] if isinstance(n, int) else n, dtype=float) * LAT
    fo, eo = restated_forces(pos, extent, lj_table(), 5.0 * SIGMA)
    assert np.abs(f - fo).max() <= TOL["force_rel_to_max"] * np.abs(fo).max()
    assert np.abs(e - eo).max() <= TOL["per_atom_energy_abs"]


@pytest.mark.gpu
@pytest.mark.parametrize("env,fmt", [({}, 1), ({"COMD_NL_GLOBAL": "1"}, 0)])
def test_both_verlet_list_formats(gpu, monkeypatch, env, fmt):
    """Cells of cutoff + skin: 12^3 has three per axis (at most 512 slots: the 16-bit slab rows of LJ_Force_nl_slabs_table); COMD_NL_GLOBAL=1,
    and the boxes of two cells per axis above, take the global-slot rows of LJ_Force_thread_atom_nl_table."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with gpu.Simulation(_args(12, 0.15, "thread_atom_nl")) as sim:
        assert sim.force_path_info()["neighbor_list_format"] == fmt
        pos, f, e = sim.gather(0), sim.gather(2), sim.gather(3)
    fo, eo = restated_forces(pos, np.full(3, 12 * LAT), lj_table(), 5.0 * SIGMA)
    assert np.abs(f - fo).max() <= TOL["force_rel_to_max"] * np.abs(fo).max()
    assert np.abs(e - eo).max() <= TOL["per_atom_energy_abs"]


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["thread_atom", "thread_atom_nl"])
def test_perfect_lattice_energy(gpu, method):
    """Step 0 of a perfect lattice: the 554 neighbours within 5 sigma, each with half of the interpolated pair energy."""
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    r2 = (((cells + basis) * LAT) ** 2).sum(-1).ravel()
    r = np.sqrt(r2[(r2 > 0) & (r2 <= (5.0 * SIGMA) ** 2)])
    assert len(r) == 554
    want = math.fsum(0.5 * interpolate(lj_table(), r)[0])
    assert abs(want - -1.4065960317826) < 1e-12
    with gpu.Simulation(_args(10, 0.0, method, ["-T", 0])) as sim:
        ep, _, ng = sim.energy()
    assert abs(ep / ng - want) < 1e-10
    assert abs(ep / ng - -1.406590686465) > 5e-6          # the analytic value: the table is a different potential by 5.35e-6 eV/atom


LOOPBACK_RUN = """
    import json
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, pkg.rccl_transport(0, 1, pkg.rccl_unique_id()))
    assert pkg.lib_host().loopbackParallel() == 1
    sim = pkg.Simulation({args!r})
    sim.step({steps})
    print("ENERGY", json.dumps(list(sim.energy())))
    sim.close()
    pkg.lib_hip().comdCommFinalize()
"""


@pytest.mark.gpu
def test_trajectories_agree_across_paths(gpu):
    """50 steps of LJ 14^3 with -I: thread_atom, thread_atom_nl, the overlap mode (-a 1: interior and boundary cells on two streams, the second
    packed-position array) and the overlap mode over the RCCL loopback transport agree in energy per atom as the analytic paths do; two
    identical runs agree to the bit."""
    steps, n = 50, 14
    runs = {}
    for name, method, extra in (("thread_atom", "thread_atom", []), ("thread_atom_nl", "thread_atom_nl", []), ("async", "thread_atom", ["-a", 1])):
        with gpu.Simulation(_args(n, 0.1, method, extra)) as sim:
            sim.step(steps)
            runs[name] = sim.energy()
            if name == "thread_atom":
                first = (sim.gather(0), sim.gather(1))
    with gpu.Simulation(_args(n, 0.1, "thread_atom")) as sim:
        sim.step(steps)
        assert np.array_equal(sim.gather(0), first[0]) and np.array_equal(sim.gather(1), first[1])
        assert sim.energy() == runs["thread_atom"]
    proc = _child(LOOPBACK_RUN.format(args=_args(n, 0.1, "thread_atom", ["-a", 1]), steps=steps), env={"COMD_LOOPBACK_TRANSPORT": "1"}, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    runs["loopback"] = tuple(json.loads(re.search(r"^ENERGY (.*)$", proc.stdout, flags=re.M).group(1)))
    ref = runs["thread_atom"]
    for name, (ep, ek, ng) in runs.items():
        assert ng == ref[2] == 4 * n ** 3, name
        assert abs((ep + ek) - (ref[0] + ref[1])) / ng < TOL["energy_per_atom_trace"], (name, (ep + ek) / ng, (ref[0] + ref[1]) / ng)


@pytest.mark.gpu
def test_single_precision_build():
    """The force test (all five legs, both boxes) and both Verlet-list formats in the float build (lib*_sp.so), at the float tolerances."""
    env = dict(os.environ, COMD_PRECISION="single")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_lj_interpolation.py",
           "-k", "test_one_evaluation_matches_the_restatement or test_both_verlet_list_formats"]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "12 passed" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-2000:]


FORCE_CALL = """
    import ctypes
    pkg.setup_gpu(0, 0)
    pkg.init_parallel(0, 1, None)
    sim = pkg.Simulation(["-x", 8, "-y", 8, "-z", 8, "-r", 0.1, "-m", "thread_atom"])
    hip = pkg.lib_hip()
    hip.ljForceGpu.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, pkg.c_real, ctypes.c_int]
    hip.ljForceGpu(ctypes.c_void_p(sim.lib.comdSimGpu(sim.ptr)), 1, sim.n_local_boxes, None, 0.0, 0)
    print("returned")
"""

C_CALLER = r"""
#include "comd_hip.h"
/* what the reference's host code does with -I (gpu_utility.c:509-510, ljForce.c:141) */
void tableForce(SimGpu* g, int method)
{
   initLJinterpolation(&g->lj_pot);
   ljForceGpu(g, 1, g->boxes.nLocalBoxes, 0, g->lj_pot.cutoff, method);
   comdDeviceSynchronize();
}
"""


@pytest.mark.gpu
def test_c_abi_interpolation_flag(gpu, tmp_path):
    """ljForceGpu(..., interpolation = 1, ...): without a table it stops and names initLJinterpolation; after initLJinterpolation it computes
    what a simulation made with -I computes."""
    proc = _child(FORCE_CALL)
    assert proc.returncode != 0 and "returned" not in proc.stdout and "initLJinterpolation" in proc.stderr, proc.stdout[-1000:] + proc.stderr[-1000:]

    src, so = tmp_path / "caller.c", tmp_path / "libcaller.so"
    src.write_text(C_CALLER)
    cc = subprocess.run(["gcc", "-std=gnu11", "-O1", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                         "-o", str(so), "-L" + CSRC, "-lcomd_hip", "-Wl,-rpath," + CSRC], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    caller = ctypes.CDLL(str(so))
    caller.tableForce.argtypes = [ctypes.c_void_p, ctypes.c_int]
    args = ["-x", 8, "-y", 8, "-z", 8, "-r", 0.1, "-m", "thread_atom"]
    with gpu.Simulation(args + ["-I"]) as sim:
        want = (sim.gather(2), sim.gather(3))
    for method in (0, 1):                                     # THREAD_ATOM, and THREAD_ATOM_NL on a simulation that keeps lists
        with gpu.Simulation(args if method == 0 else ["-x", 8, "-y", 8, "-z", 8, "-r", 0.1, "-m", "thread_atom_nl"]) as sim:
            caller.tableForce(ctypes.c_void_p(sim.lib.comdSimGpu(sim.ptr)), method)
            f, e = sim.gather(2), sim.gather(3)
        if method == 0:
            assert np.array_equal(f, want[0]) and np.array_equal(e, want[1])
        else:
            assert np.abs(f - want[0]).max() <= TOL["force_rel_to_max"] * np.abs(want[0]).max()
            assert np.abs(e - want[1]).max() <= TOL["per_atom_energy_abs"]
