"""AddressSanitizer + UBSan over the HOST side of msnake_copy_envs (csrc/msnake_capi.hip), device code left
uninstrumented (-fno-gpu-sanitize), like tests/test_capi_sanitizers.py.  No GPU is needed or used: the driver
exercises what runs before the first device call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "self-play-on-multi-snakes-environment_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_copy_envs_host_validation_is_clean_under_asan_ubsan(tmp_path):
    if not os.path.exists(HIPCC) or shutil.which("gcc") is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path / "capi_copy_asan")
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-omit-frame-pointer", "-Wno-everything", "-mllvm", "-amdgpu-kernarg-preload-count=16", "-o", exe,
           os.path.join(ROOT, "tests", "capi_copy_asan_check.cpp"), os.path.join(CSRC, "msnake_kernels.hip"),
           os.path.join(CSRC, "msnake_opponents.hip"), os.path.join(CSRC, "msnake_views.hip"), os.path.join(CSRC, "msnake_capi.hip")]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    if build.returncode != 0 and ("sanitize" in build.stderr or "asan" in build.stderr.lower()):
        pytest.skip("sanitizer runtime for clang not usable here: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", HIP_VISIBLE_DEVICES="")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "CAPI COPY ASAN/UBSAN run clean" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
