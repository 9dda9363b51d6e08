"""The device assembly of comd_device.hip for gfx950 -- TEST INFRASTRUCTURE.

One `hipcc -S --cuda-device-only` per precision per process, with the flags of csrc/Makefile; the tests that look at kernel descriptors
(scratch, LDS, registers) share the text.
"""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "comd-cuda-async_amd", "csrc", "hip", "comd_device.hip")


@functools.lru_cache(maxsize=None)
def assembly(precision):
    """the device assembly text of the `double` or `single` build"""
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        proc = subprocess.run(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-Wno-comment", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.dirname(SRC), "-S", "--cuda-device-only", "-o", out, SRC]
                              + {"double": [], "single": ["-DCOMD_SINGLE"]}[precision], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-2000:]
        return open(out).read()


def blocks(precision, pattern=r"\w+"):
    """{mangled kernel name: its descriptor, the text between .amdhsa_kernel and .end_amdhsa_kernel} of the kernels `_Z<digits>` + pattern"""
    return dict(re.findall(rf"^\s*\.amdhsa_kernel (_Z\d+{pattern})\n(.*?)\.end_amdhsa_kernel", assembly(precision), flags=re.S | re.M))


def assert_keeps_waves(found, name_part, waves):
    """The one kernel of `found` with name_part in its name asks for no more VGPRs than fit `waves` times into a SIMD.  A SIMD has 512 VGPRs per
    lane and hands them out in granules of 8: a wave gets ceil(next_free_vgpr / 8) * 8, and min(8, floor(512 / that)) waves fit.  The largest
    allocation that still holds w waves is floor(512 / w) rounded down to a multiple of 8: 8 waves 64, 7 waves 72, 6 waves 80, 5 waves 96, 4 waves 128."""
    (block,) = [b for n, b in found.items() if name_part in n]
    vgprs, most = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)\n", block).group(1)), 512 // waves // 8 * 8
    print(name_part, vgprs, "VGPRs, at most", most, "for", waves, "waves per SIMD")
    assert vgprs <= most, (name_part, vgprs, most)
