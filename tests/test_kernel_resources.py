"""CPU: the compiler's resource report for the two fused tracker kernels (csrc/dsst.hip), through tools/kernel_resources.py.
Both are held to 128 registers by amdgpu_waves_per_eu(4, 4) -- 512 threads, four waves per SIMD, two blocks per CU beside 66.5 KB of LDS
each.  With the transform's twiddles in scalar registers they fit that budget; a spilled register is stored and reloaded around the
transform of each of the 32 planes, so the count is held at zero here.  Needs hipcc (the device side is cross-compiled), no GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

SOURCE = os.path.join("pyannote-video_amd", "csrc", "dsst.hip")


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


@pytest.mark.parametrize("kernel", ["start_fused_k", "update_fused_k"])
def test_fused_tracker_kernels_spill_nothing(report, kernel):
    k = report[kernel]
    print(kernel, k)
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["scratch_bytes_per_lane"] == 0
    assert k["occupancy_waves_per_simd"] == 4
    assert k["vgprs"] <= 128


def test_the_report_names_every_kernel_of_the_source(report):
    for name in ("trans_planes_fft_k", "corr_k", "peak_k", "filter_update_k", "scale_fft_k", "scale_start_k", "scale_update_k"):
        assert name in report and report[name]["vgprs"] > 0, name


def test_parse_reads_the_compiler_remarks():
    tail = " [-Rpass-analysis=kernel-resource-usage]\n"
    text = "".join("x.hip:1:1: remark: " + s + tail for s in (
        "Function Name: _Z6corr_kPK6TrkJob", "    TotalSGPRs: 18", "    VGPRs: 64", "    AGPRs: 0", "    ScratchSize [bytes/lane]: 80",
        "    Occupancy [waves/SIMD]: 8", "    SGPRs Spill: 0", "    VGPRs Spill: 19", "    LDS Size [bytes/block]: 1024"))
    assert kernel_resources.parse(text + "warning: something else\n") == [
        {"kernel": "corr_k", "symbol": "_Z6corr_kPK6TrkJob", "sgprs": 18, "vgprs": 64, "agprs": 0, "scratch_bytes_per_lane": 80,
         "occupancy_waves_per_simd": 8, "sgpr_spill": 0, "vgpr_spill": 19, "lds_bytes_per_block": 1024}]
