"""The single-precision build (make PRECISION=single: real_t = float, the reference's DOUBLE_PRECISION = OFF, mytype.h:8-21, Makefile:12).

A process binds one precision (the two builds export the same symbols), so every leg runs the ordinary test files in a child process
with COMD_PRECISION=single: the product loads lib*_sp.so, the checker loads oracle/liboracle_sp.so (the same restatement compiled with
real_t = float) and the tolerances are tests/golden/reference_values.json "tolerances_single" (their derivation is written there).
Index work -- lattice, momenta, cell membership, gid order, halo images -- stays bit-exact in either precision.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_analysis_regimes import GPU_CASE_COUNT as ANALYSIS_REGIMES_GPU_CASE_COUNT
from test_capacities import GPU_CASE_COUNT
from test_kernel_legs import FAMILY_LEG_COUNT
from test_per_atom_fields_edges import GPU_CASE_COUNT as PER_ATOM_EDGES_GPU_CASE_COUNT
from test_two_cell_boxes import GPU_CASE_COUNT as TWO_CELL_GPU_CASE_COUNT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "comd-cuda-async_amd", "csrc")


def _run(files, k, marker, timeout):
    env = dict(os.environ, COMD_PRECISION="single")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", marker, "-p", "no:cacheprovider", *files] + (["-k", k] if k else [])
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    tail = proc.stdout[-3000:] + proc.stderr[-2000:]
    assert proc.returncode == 0, tail
    return proc.stdout


def test_single_precision_libraries_exist_and_export_the_abi():
    """libcomd_hip_sp.so exports what include/comd_hip.h declares, same as the double build (checked in a child: one precision per process)."""
    for lib in ("libcomd_hip_sp.so", "libcomd_host_sp.so"):
        assert os.path.exists(os.path.join(CSRC, lib)), f"{lib} missing: make -C {CSRC} PRECISION=single"
    assert os.path.exists(os.path.join(ROOT, "oracle", "liboracle_sp.so"))
    out = _run(["tests/test_host_logic.py"], "test_abi_exports_every_declared_symbol or test_product_never_links_the_oracle", "not gpu", 300)
    assert "passed" in out


def test_single_precision_host_logic_is_bit_exact_against_the_checker():
    """Lattice, Maxwell-Boltzmann momenta (mixed float / double expressions evaluated as the reference's C does), cell numbering incl. tie
    rules, halo cell lists, and the multi-process exchange driver (2 and 8 ranks): bit for bit against the float build of the checker."""
    out = _run(["tests/test_host_logic.py", "tests/test_multirank.py"],
               "test_initial_state or test_displaced_state or test_cell_numbering or test_halo_cell_lists or test_host_logic", "not gpu", 900)
    assert "passed" in out


def test_single_precision_checker_meets_the_reference_held_energies():
    """liboracle_sp.so itself against the values the reference holds (CoMD.c:897-899, the step-0 row of the K20 log), at the float tolerances:
    the float checker is pinned by more than being the same source as the double one."""
    out = _run(["tests/test_oracle_golden.py"], "repo_native or step0_row_of_k20_log or setfl_mishin_cohesive_energy", "not gpu", 600)
    assert "4 passed" in out, out[-800:]


@pytest.mark.gpu
def test_single_precision_gpu_parity():
    """Forces, energies, densities, redistribution, lists, pairlists, setfl tables and reproducibility of the float kernels on the GPU."""
    k = ("test_forces_match_oracle or test_eam_any_cell_capacity or test_overlap_mode_small_interior or test_neighbor_list_forces_match_oracle "
         "or test_redistribution_is_bit_exact or test_pairlist_forces_match_oracle or test_setfl_forces_match_oracle or test_runs_are_bit_reproducible "
         "or test_halo_cells_are_periodic_images or test_neighbor_list_global_slot_format")
    out = _run(["tests/test_gpu_parity.py"], k, "gpu", 1500)
    assert "passed" in out and "failed" not in out


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["lj", "eam_cta", "eam_atom", "lists", "tables", "pairloss"])
def test_single_precision_kernel_legs(family):
    """Every forced leg of tests/test_kernel_legs.py in the float build, a family per child process.  Float changes which leg a run takes (every LDS size is
    n * sizeof(real_t)), so each leg asserts its fact there as well; the count of passed tests must be the family's leg count from the same table: none skipped."""
    out = _run(["tests/test_kernel_legs.py"], family, "gpu", 300)
    passed = re.search(r"(\d+) passed", out)
    assert passed and int(passed.group(1)) == FAMILY_LEG_COUNT[family] and "skipped" not in out and "failed" not in out, out[-1500:]


@pytest.mark.gpu
def test_single_precision_capacities():
    """tests/test_capacities.py in the float build: cells, Verlet rows and the halo exactly full and one unit short.  The states' figures are the same in float
    (its CPU tests assert them on the float checker first), the halo's edge and the landing points are computed in float32; none skipped."""
    _run(["tests/test_capacities.py"], None, "not gpu", 300)
    out = _run(["tests/test_capacities.py"], None, "gpu", 600)
    passed = re.search(r"(\d+) passed", out)
    assert passed and int(passed.group(1)) == GPU_CASE_COUNT and "skipped" not in out and "failed" not in out, out[-1500:]


@pytest.mark.gpu
def test_single_precision_two_cell_boxes():
    """tests/test_two_cell_boxes.py in the float build: every method, the forced legs, the lists over rebuilds, redistribution, the analyses and the multi-rank runs on
    boxes with two link cells along an axis.  Its CPU tests assert the states' figures on the float checker first; none skipped."""
    _run(["tests/test_two_cell_boxes.py"], None, "not gpu", 300)
    out = _run(["tests/test_two_cell_boxes.py"], None, "gpu", 900)
    passed = re.search(r"(\d+) passed", out)
    assert passed and int(passed.group(1)) == TWO_CELL_GPU_CASE_COUNT and "skipped" not in out and "failed" not in out, out[-1500:]


@pytest.mark.gpu
def test_single_precision_analysis_regimes():
    """tests/test_analysis_regimes.py in the float build: the virial, g(r), CSP, CNA, per-atom stress and strain in the void, sparse, dilute and dense regimes, the layouts,
    the message halo, two ranks, the executable and the singular strain reference, each under its module's float rule.  Its CPU tests assert the regimes' figures and the float
    caps on the float checker first (and name the legs whose reference alone exceeds a cap); none skipped."""
    _run(["tests/test_analysis_regimes.py"], None, "not gpu", 900)
    out = _run(["tests/test_analysis_regimes.py"], None, "gpu", 900)
    passed = re.search(r"(\d+) passed", out)
    assert passed and int(passed.group(1)) == ANALYSIS_REGIMES_GPU_CASE_COUNT and "skipped" not in out and "failed" not in out, out[-1500:]


@pytest.mark.gpu
def test_single_precision_per_atom_fields_edges():
    """tests/test_per_atom_fields_edges.py in the float build: per-atom stress, heat flux and strain on the 2-cell boxes, on a straining box driven from Python and where
    the image of a reference separation decides, each under its module's float rule.  Its CPU tests show on the float checker first where the two image rules differ;
    none skipped."""
    _run(["tests/test_per_atom_fields_edges.py"], None, "not gpu", 900)
    out = _run(["tests/test_per_atom_fields_edges.py"], None, "gpu", 900)
    passed = re.search(r"(\d+) passed", out)
    assert passed and int(passed.group(1)) == PER_ATOM_EDGES_GPU_CASE_COUNT and "skipped" not in out and "failed" not in out, out[-1500:]


SPLINE_CASE = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
import oracle_binding as ob
o = ob.Oracle((8, 7, 9), eam=1, delta=0.1, spline=True)
np.savez(sys.argv[1], f=o.gather(ob.F), u=o.gather(ob.U), rho=o.gather(ob.RHOBAR), df=o.gather(ob.DFEMBED), e=o.energy()[0] / o.n_global)
"""


def test_single_precision_spline_tolerances_are_four_times_the_checkers_distance(tmp_path):
    """tests/golden/reference_values.json "tolerances_single_spline" states its rule: 4x the distance of the float checker from the double checker on EAM 8 x 7 x 9, -r 0.1,
    -P.  Both checkers are run here (a child process each: one precision per process) and every recorded value must lie within [4x, 8x] of the distance found."""
    got = {}
    for precision in ("double", "single"):
        path = str(tmp_path / f"{precision}.npz")
        proc = subprocess.run([sys.executable, "-c", SPLINE_CASE % os.path.join(ROOT, "tests"), path], cwd=ROOT, env=dict(os.environ, COMD_PRECISION=precision),
                              capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, proc.stderr[-1500:]
        got[precision] = np.load(path)
    d, s = got["double"], got["single"]
    distance = {"force_rel_to_max": np.abs(d["f"] - s["f"]).max() / np.abs(d["f"]).max(), "per_atom_energy_abs": np.abs(d["u"] - s["u"]).max(),
                "eam_density_abs": np.abs(d["rho"] - s["rho"]).max(), "eam_dfembed_abs": np.abs(d["df"] - s["df"]).max(), "energy_per_atom_step0": abs(float(d["e"]) - float(s["e"]))}
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_values.json")))["tolerances_single_spline"]
    assert set(recorded) - {"_about"} == set(distance)
    for key, dist in distance.items():
        assert 4.0 * dist <= recorded[key] <= 8.0 * dist, (key, float(dist), recorded[key])


@pytest.mark.gpu
def test_single_precision_multi_rank():
    out = _run(["tests/test_multirank.py"], "test_gpu_path_multi_rank_shared_device and (cta_cell-0 or thread_atom-1 or thread_atom_nl-0) or test_rccl_transport_loopback and cta_cell", "gpu", 1500)
    assert "passed" in out and "failed" not in out
