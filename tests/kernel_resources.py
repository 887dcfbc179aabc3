"""The device assembly and the compiler's resource remarks of one kernel unit of csrc/ (msnake_kernels, msnake_opponents,
msnake_views), compiled once per process with the Makefile's flags.  For the CPU tests that read register budgets: each
asks for the unit that holds its kernels.  No GPU: hipcc cross-compiles to assembly, nothing runs."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "self-play-on-multi-snakes-environment_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["-Os", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-kernarg-preload-count=16"]

_REMARK = re.compile(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|"
                     r"LDS Size \[bytes/block\]): (\S+)")


def parse_remarks(stderr):
    """{mangled kernel name: {"TotalSGPRs": n, "VGPRs": n, "ScratchSize [bytes/lane]": n, "SGPRs Spill": n,
    "VGPRs Spill": n, "LDS Size [bytes/block]": n}} from -Rpass-analysis=kernel-resource-usage."""
    res, cur = {}, None
    for line in stderr.split("\n"):
        m = _REMARK.search(line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = res.setdefault(v, {})
        else:
            cur[k] = int(v)
    return res


@functools.lru_cache(maxsize=None)
def unit_resources(unit):
    """(resource table, assembly text) of csrc/<unit>.hip."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, unit + ".s")
        r = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", out,
                                              os.path.join(CSRC, unit + ".hip")], check=True, capture_output=True, text=True)
        with open(out) as f:
            return parse_remarks(r.stderr), f.read()
