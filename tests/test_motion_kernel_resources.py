"""CPU: the compiler's resource report for the kernel of csrc/motion.hip, through tools/kernel_resources.py.  motion_fit_k spills
nothing and uses no scratch; its LDS is the eight partial sums of its four waves and the six words lane 0 hands to the others (DESIGN.md
section 25).  Needs hipcc (the device side is cross-compiled), no GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = os.path.join("pyannote-video_amd", "csrc", "motion.hip")


@pytest.fixture(scope="module")
def report():
    if kernel_resources.hipcc() is None:
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, SOURCE)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads(out.stdout)
    assert list(doc) == [SOURCE]
    return {k["kernel"]: k for k in doc[SOURCE]}


def test_the_file_holds_the_one_kernel(report):
    assert sorted(report) == ["motion_fit_k"]


def test_motion_fit_spills_nothing(report):
    k = report["motion_fit_k"]
    print(k)
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["scratch_bytes_per_lane"] == 0


def test_lds_is_the_partial_sums_and_the_broadcast(report):
    assert report["motion_fit_k"]["lds_bytes_per_block"] == (4 * 8 + 6) * 8
