"""The launch plan of k_horisun_coarse (horayzon_amd/csrc/hz_horisun_coarse_plan.h: plain C++, no HIP) walked by a stand-alone
host program built with AddressSanitizer and UndefinedBehaviorSanitizer: every cell of every block is added once and in
row-major order, LDS indices and bytes stay inside their caps, the grid fits a launch.  No GPU, and nothing here is loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path / "horisun_coarse_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "scripts", "horisun_coarse_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "horisun coarse plan: all checks passed" in run.stdout
