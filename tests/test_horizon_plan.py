"""The sizes of a gridded horizon call (horayzon_amd/csrc/hz_horizon_plan.h: plain C++, no HIP) walked by a stand-alone host
program built with AddressSanitizer and UndefinedBehaviorSanitizer: the chunks of rows tile the slab once and in order and stay
inside their byte target, the regions of the leftover records follow each other in multiples of 64 records, and a plan that
is on fits the 32-bit record numbers.  No GPU, and nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    exe = str(tmp_path / "horizon_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "scripts", "horizon_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "horizon plan: all checks passed" in run.stdout
