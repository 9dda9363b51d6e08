"""The run-time reports of comd-hip taken together: one run with every sampler on pins what the driver's report table (csrc/host/reports.c) encodes and the
tests of the single reports state only piecewise -- the order of the columns, the order of the YAML blocks, the calls of every report's timer, the zeros a
column prints before its report's origin -- and that no report changes the trajectory.

The run: 2048 LJ atoms, 20 steps printed every 5, the box strained along x.  --msdStart 11 and --strainRef 13 fall inside the same print interval, so that
interval is taken as three timestep() calls with the two origins in between; --hfStart and --profStart fall on a printed step.
"""
import os
import re
import subprocess

import pytest

from test_pressure import CSRC, ROOT, SINGLE

RUN = ["-x", "8", "-y", "8", "-z", "8", "-N", "20", "-n", "5", "--erateX", "0.01"]      # the strain rate is a load, not a report: the bare run keeps it
REPORTS = ["--pressure", "--rdf", "64", "--msd", "--msdStart", "11", "--csp", "--cspDump", "c.xyz", "--cna", "--cnaDump", "n.xyz", "--stress", "--stressDump", "s.xyz",
           "--strain", "--strainRef", "13", "--strainDump", "e.xyz", "--heatflux", "--hfStart", "10", "--profile", "--profBins", "8", "--profStart", "10"]
BASE = ["#", "Loop", "Time(fs)", "Total", "Energy", "Potential", "Energy", "Kinetic", "Energy", "Temperature", "(us/atom)", "#", "Atoms"]
COLUMNS = ["Pressure(GPa)", "MSD(A^2)", "Defects", "NonFCC", "V/V0", "Sxx(GPa)", "MaxVM(GPa)", "MaxShear", "Jx(eV/A^2/fs)"]
BLOCKS = ["Pressure", "RDF", "MSD", "CSP", "CNA", "Deform", "Barostat", "Stress", "Strain", "HeatFlux", "Profile", "MullerPlathe"]
STEPS = [0, 5, 10, 15, 20]
# samples, + 1 where the write runs under the report's timer too (stress, strain, heatflux, profile).  msd and strain sample at 15 and 20 only: their origins at
# 11 and 13 are taken between printed steps, inside the timestep timer; heatflux and profile sample from step 10
CALLS = {"pressure": 5, "rdf": 5, "csp": 5, "cna": 5, "stress": 5 + 1, "msd": 2, "strain": 2 + 1, "heatflux": 3 + 1, "profile": 3 + 1}
MSD, MAXSHEAR, JX = 9, 15, 16      # fields of a row; the first eight are those of a run without reports


def _comd_hip(cwd, args):
    os.makedirs(cwd)
    proc = subprocess.run([os.path.join(CSRC, "comd-hip-sp" if SINGLE else "comd-hip"), "-d", os.path.join(ROOT, "pots")] + args, capture_output=True, text=True, cwd=cwd, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    yaml = "".join(open(os.path.join(cwd, f)).read() for f in sorted(os.listdir(cwd)) if f.startswith("CoMD-hip") and f.endswith(".yaml"))
    rows = {int(l.split()[0]): l.split() for l in proc.stdout.splitlines() if re.match(r"^\s+\d+\s+\d+\.\d\d\s", l)}
    return proc.stdout, yaml, rows


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    top = tmp_path_factory.mktemp("driver_reports")
    return _comd_hip(str(top / "all"), RUN + REPORTS), _comd_hip(str(top / "bare"), RUN)


@pytest.mark.gpu
def test_columns_come_in_the_order_of_the_reports(runs):
    (out, _, rows), _ = runs
    head = [l for l in out.splitlines() if "Loop" in l and "Time(fs)" in l]
    print(head)
    assert len(head) == 1 and head[0].split() == BASE + COLUMNS
    assert sorted(rows) == STEPS and all(len(r) == 8 + len(COLUMNS) for r in rows.values())


@pytest.mark.gpu
def test_yaml_blocks_come_in_the_order_of_the_reports(runs):
    (_, yaml, _), _ = runs
    blocks = [k for k in re.findall(r"^(\w+):\s*$", yaml, flags=re.M) if k in BLOCKS]
    print(blocks)
    assert blocks == [b for b in BLOCKS if b not in ("Barostat", "MullerPlathe")]


@pytest.mark.gpu
def test_every_report_timer_counts_its_samples_and_its_timed_write(runs):
    (out, _, _), (bare, _, _) = runs
    table = out[out.index("Timings for Rank 0"):out.index("Timing Statistics Across")]
    calls = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*(\w+)\s+(\d+)\s", table, flags=re.M)}
    print(calls)
    assert {k: calls.get(k) for k in CALLS} == CALLS
    table = bare[bare.index("Timings for Rank 0"):bare.index("Timing Statistics Across")]
    calls = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*(\w+)\s+(\d+)\s", table, flags=re.M)}
    print(calls)
    assert calls.get("pressure") == 5 and not any(k in calls for k in CALLS if k != "pressure")      # the strained box alone needs the virial


@pytest.mark.gpu
def test_columns_are_zero_before_the_origin_of_their_report(runs):
    (_, _, rows), _ = runs
    print({s: (rows[s][MSD], rows[s][MAXSHEAR], rows[s][JX]) for s in STEPS})
    for s in STEPS:
        assert (float(rows[s][MSD]) == 0.0) == (s < 15) and (float(rows[s][MAXSHEAR]) == 0.0) == (s < 15), (s, rows[s])
        assert (float(rows[s][JX]) == 0.0) == (s < 10), (s, rows[s])
        assert float(rows[s][MSD]) >= 0.0 and float(rows[s][MAXSHEAR]) >= 0.0


@pytest.mark.gpu
def test_no_report_changes_the_trajectory(runs):
    (_, _, rows), (_, _, bare) = runs
    assert sorted(bare) == STEPS
    for s in STEPS:
        print(rows[s][:8], bare[s][:8])
        assert rows[s][:6] + rows[s][7:8] == bare[s][:6] + bare[s][7:8], s
