"""CPU: the compiler's resource report for the two kernels of csrc/blend.hip, through tools/kernel_resources.py.  Both spill nothing and
use no scratch; blend_measure_k reduces within its wave and holds no LDS, blend_luma_k the eight partial sums of its four waves (DESIGN.md
section 24).  Needs hipcc (the device side is cross-compiled), no GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = os.path.join("pyannote-video_amd", "csrc", "blend.hip")


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


def test_the_file_holds_the_two_kernels(report):
    assert sorted(report) == ["blend_luma_k", "blend_measure_k"]


@pytest.mark.parametrize("kernel", ["blend_luma_k", "blend_measure_k"])
def test_blend_kernels_spill_nothing(report, kernel):
    k = report[kernel]
    print(kernel, k)
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["scratch_bytes_per_lane"] == 0
    assert k["occupancy_waves_per_simd"] == 8


def test_lds_is_the_partial_sums_and_nothing_else(report):
    assert report["blend_measure_k"]["lds_bytes_per_block"] == 0
    assert report["blend_luma_k"]["lds_bytes_per_block"] == 2 * 4 * 4
