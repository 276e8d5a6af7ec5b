"""Registers, spills, scratch and occupancy of every kernel of a HIP source, as the compiler reports them -- no GPU needed:
    python tools/kernel_resources.py [pyannote-video_amd/csrc/dsst.hip ...]        (default: dsst.hip)
Compiles the device side only, with the flags of csrc/Makefile, under -Rpass-analysis=kernel-resource-usage and prints one JSON
object: {source: [{"kernel", "symbol", "vgprs", "agprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch_bytes_per_lane",
"occupancy_waves_per_simd", "lds_bytes_per_block"}, ...]}.  tests/test_kernel_resources.py holds the fused tracker kernels to zero
spills with it; profiles/tracker_registers.txt is its output before and after the twiddles moved to scalar registers."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyannote-video_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]          # csrc/Makefile's, less -fPIC / warnings

FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill",
          "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
          "LDS Size [bytes/block]": "lds_bytes_per_block"}
REMARK = re.compile(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]")


def hipcc():
    """the compiler csrc/Makefile uses ($HIPCC, /opt/rocm/bin/hipcc), else one on PATH; None: there is none"""
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isfile(c) and os.access(c, os.X_OK):
            return c
    return None


def short_name(symbol):
    """_Z13start_fused_kPK6TrkJob... -> start_fused_k (kernels here live in no namespace); anything else stays as it is"""
    m = re.match(r"_Z(\d+)", symbol)
    if not m:
        return symbol
    n = int(m.group(1))
    return symbol[m.end():m.end() + n]


def parse(report):
    """the compiler's remarks -> one record per kernel, in the order reported"""
    out = []
    for line in report.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            out.append({"kernel": short_name(val), "symbol": val})
        elif key in FIELDS and out:
            out[-1][FIELDS[key]] = int(val)
    return out


def resources(source, compiler=None):
    compiler = compiler or hipcc()
    if compiler is None:
        raise RuntimeError("no hipcc found ($HIPCC, /opt/rocm/bin/hipcc, PATH)")
    with tempfile.TemporaryDirectory() as d:
        cmd = [compiler] + FLAGS + ["-I", os.path.join(ROOT, "include"), "-I", CSRC, "--offload-device-only", "-c", source,
                                    "-o", os.path.join(d, "device.o"), "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stderr[-4000:]))
    return parse(r.stderr)


def main(argv):
    sources = argv or [os.path.join(CSRC, "dsst.hip")]
    print(json.dumps({os.path.relpath(os.path.abspath(s), ROOT): resources(s) for s in sources}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
