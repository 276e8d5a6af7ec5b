"""CPU: the compiler's resource report for the kernels of csrc/clothes.hip, through tools/kernel_resources.py.  box_hist_k and hist_zero_k
spill nothing and use no scratch; box_hist_k's LDS is the 16 staged rows of a piece, 784 bytes each, and a 256-bin table for each of its
four waves.  Needs hipcc (the device side is cross-compiled), no GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = os.path.join("pyannote-video_amd", "csrc", "clothes.hip")


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
    assert sorted(report) == ["box_hist_k", "hist_zero_k"]


@pytest.mark.parametrize("kernel", ("box_hist_k", "hist_zero_k"))
def test_the_kernels_spill_nothing(report, kernel):
    k = report[kernel]
    print(k)
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["scratch_bytes_per_lane"] == 0


def test_lds_is_the_staged_rows_and_the_four_tables(report):
    assert report["box_hist_k"]["lds_bytes_per_block"] == 16 * 784 + 4 * 256 * 4    # what DESIGN.md section 27 states: 16640
    assert report["hist_zero_k"]["lds_bytes_per_block"] == 0
