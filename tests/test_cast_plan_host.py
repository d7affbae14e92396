"""The chunk plan of Terrain.cast (horayzon_amd/csrc/hz_cast_plan.h) as a stand-alone host program under ASan + UBSan:
tests/cast_plan_host.cpp includes the header as it stands and checks the rays per chunk at the edges -- N = 1, 64, 65,
2^31 - 64, every combination of staged inputs and outputs with and without the sort, budgets down to one wave and below --
and in a sweep against the clause restated in 128-bit integers.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "cast_plan_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cast_plan_host.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "cast plan ok" in run.stdout


def test_the_header_includes_nothing():
    text = open(os.path.join(ROOT, "horayzon_amd", "csrc", "hz_cast_plan.h")).read()
    assert "#include" not in text
