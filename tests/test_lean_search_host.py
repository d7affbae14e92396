"""The lean search state of the flat guess_constant refill (horayzon_amd/csrc/hz_search.h: SearchLean, advance_az0_lean,
advance_guess_flat) against the state machine it stands for, advance<ALG_GUESS>, in a stand-alone host program built with
AddressSanitizer and UndefinedBehaviorSanitizer (scripts/lean_search_check.cpp): several million transitions with the same hit /
miss answers -- table ends, azimuth 0, and hand-overs through a 16-word record written by one form and restored by the other --
must give the same states and the same emitted values.  No GPU, and nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lean_search_check_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if gxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("g++ or the HIP headers are not installed")
    exe = str(tmp_path / "lean_search_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "scripts", "lean_search_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "lean search: all checks passed" in run.stdout
