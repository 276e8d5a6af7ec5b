"""CPU: the compiler's resource report for the kernels of csrc/repeat.hip, through tools/kernel_resources.py.  All three spill nothing
and use no scratch; print_runs_k's LDS is exactly the tile it stages -- PVF_RUNS_STRIP + 256 prints of B, 16 bytes each, and as many
4-byte penalties -- which leaves six workgroups a CU.  Needs hipcc (the device side is cross-compiled), no GPU."""
import json
import os
import subprocess
import sys

import pytest

from tests import repeat_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = os.path.join("pyannote-video_amd", "csrc", "repeat.hip")


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


@pytest.mark.parametrize("kernel", ["frame_print_k", "print_finish_k", "print_runs_k"])
def test_repeat_kernels_spill_nothing(report, kernel):
    k = report[kernel]
    print(kernel, k)
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["scratch_bytes_per_lane"] == 0


def test_the_runs_kernel_holds_its_tile_and_nothing_else_in_lds(report):
    k = report["print_runs_k"]
    assert k["lds_bytes_per_block"] == (rc.S + rc.GROUP) * (16 + 4)
    assert 160 * 1024 // k["lds_bytes_per_block"] >= 6 and k["vgprs"] + k["agprs"] <= 64


def test_the_print_kernel_keeps_eight_waves_a_simd(report):
    k = report["frame_print_k"]
    assert k["occupancy_waves_per_simd"] == 8 and k["lds_bytes_per_block"] == 16 * 27 * 8
