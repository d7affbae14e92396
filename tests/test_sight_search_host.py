"""The per-lane search of Terrain.sight_height (horayzon_amd/csrc/hz_sight_search.h) as a stand-alone host program under
ASan + UBSan: tests/sight_search_host.cpp includes the header as it stands, drives the state machine one lane at a time
through every table length and first visible index, and holds it to the clause written down as it reads.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_state_machine_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sight_search_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "sight_search_host.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "sight search ok" in run.stdout
