"""The by-slot to by-gid pass of the by-gid analyses (csrc/host/slot_gather.h) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/slot_gather_main.c says what it sets up and asserts.  No GPU, no library of the project."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "comd-cuda-async_amd", "csrc", "host")


@pytest.mark.parametrize("precision", ["double", "single"])
def test_slot_gather_reads_no_unoccupied_slot_and_skips_foreign_gids(precision, tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc not on PATH")
    exe = str(tmp_path / "slot_gather_main")
    cc = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "slot_gather_main.c"), "-o", exe, "-lm"]
                        + {"double": [], "single": ["-DCOMD_SINGLE"]}[precision], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "slot_gather_main OK" in run.stdout, run.stderr[-2000:]
