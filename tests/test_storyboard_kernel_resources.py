"""CPU: the compiler's resource report for the kernels of csrc/board.hip, through tools/kernel_resources.py.  frame_thumbs_k is a stream
that hides HBM latency behind other resident blocks: it is held to no spilled register, no scratch, and to the LDS and register budget
of eight blocks of 256 lanes a CU (20 KB of LDS a block, eight waves a SIMD), and its LDS size to the constant the
case table's row bands are derived from.  Needs hipcc (the device side is cross-compiled), no GPU."""
import json
import os
import subprocess
import sys

import pytest

from tests import storyboard_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = os.path.join("pyannote-video_amd", "csrc", "board.hip")


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


@pytest.mark.parametrize("kernel", ["frame_thumbs_k", "thumb_tiles_k"])
def test_board_kernels_spill_nothing(report, kernel):
    k = report[kernel]
    print(kernel, k)
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["scratch_bytes_per_lane"] == 0


def test_the_thumbnail_kernel_keeps_eight_blocks_a_cu(report):
    k = report["frame_thumbs_k"]
    assert k["lds_bytes_per_block"] == sc.LDS_BYTES <= 160 * 1024 // 8
    assert k["occupancy_waves_per_simd"] == 8 and k["vgprs"] + k["agprs"] <= 64
