"""CPU: the compiler's resource report for the kernels of csrc/search.hip, through tools/kernel_resources.py.  search_tiles_k keeps the
32 A fragments of a query block in registers (64 VGPRs) like cross_tiles_k and is held to that kernel's budget -- amdgpu_waves_per_eu(3, 4):
at most 168 registers, three waves per SIMD -- with no spilled register and no scratch: the selection (bounds, ballots, the bitonic sort
of a list) must fit beside the fragments.  Needs hipcc (the device side is cross-compiled), no GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = os.path.join("pyannote-video_amd", "csrc", "search.hip")


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


@pytest.mark.parametrize("kernel", ["search_quant_k", "search_tiles_k", "search_merge_k"])
def test_search_kernels_spill_nothing(report, kernel):
    k = report[kernel]
    print(kernel, k)
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["scratch_bytes_per_lane"] == 0


def test_the_tile_kernel_keeps_the_budget_of_cross_tiles_k(report):
    k = report["search_tiles_k"]
    assert k["vgprs"] + k["agprs"] <= 168 and k["occupancy_waves_per_simd"] >= 3
    # static LDS: two staged blocks of 16 x 130 doubles + per-column and per-row tables; the sort workspace is dynamic (4 waves x 2 kp x 12 bytes)
    assert 2 * 16 * 130 * 8 <= k["lds_bytes_per_block"] <= 36 * 1024
