"""hz_n_leave (horayzon_amd/csrc/hz_common.h): how many lanes of a wave must still be traversing for hz_trace's loop to go on.
Rule 0 is the absolute threshold min(regroup, n_entry), rule 1 scales it with the lanes that entered with a ray,
(regroup * n_entry + round) >> 6.  The header compiles on the host, so the function is checked there, for every regroup and n_entry
in 1 ... 64 and every rounding 0 ... 63:
  * 1 <= n_leave <= n_entry -- the progress guarantee: the loop is only left after a lane's ray is decided (or when none traverses),
  * rule 1 equals rule 0 for a full wave,
  * rule 1 is monotone in n_entry."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include "hz_common.h"
int main() {
    for (int rule = 0; rule < 2; rule++)
        for (int round = 0; round < 64; round++)
            for (int regroup = 1; regroup <= 64; regroup++)
                for (int n = 1; n <= 64; n++) std::printf("%d\n", hz_n_leave(regroup, n, rule, round));
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """t[rule, round, regroup - 1, n_entry - 1]"""
    # (a host-only program: hipcc -- the compiler of horayzon_amd/csrc/Makefile -- compiles a .cpp file as plain C++ and knows
    #  where <hip/hip_runtime.h>, which the header includes, lives)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed (as for the build)"
    d = tmp_path_factory.mktemp("regroup_rule")
    src, exe = d / "rule.cpp", d / "rule"
    src.write_text(PROGRAM)
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "horayzon_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    t = np.array(out.split(), dtype=np.int64)
    assert t.size == 2 * 64 * 64 * 64
    return t.reshape(2, 64, 64, 64)


REGROUP = np.arange(1, 65)[:, None]
N_ENTRY = np.arange(1, 65)[None, :]


def test_rule_0_is_the_absolute_threshold(table):
    for rnd in range(64):      # (rule 0 does not depend on the rounding)
        assert np.array_equal(table[0, rnd], np.maximum(np.minimum(REGROUP, N_ENTRY), 1))


def test_rule_1_is_the_rounded_share(table):
    for rnd in range(64):
        assert np.array_equal(table[1, rnd], np.maximum((REGROUP * N_ENTRY + rnd) >> 6, 1))


@pytest.mark.parametrize("rule", (0, 1))
def test_progress_guarantee(table, rule):
    assert np.all(table[rule] >= 1) and np.all(table[rule] <= N_ENTRY[None])


def test_rules_agree_for_a_full_wave(table):
    for rnd in range(64):
        assert np.array_equal(table[1, rnd, :, 63], table[0, rnd, :, 63]) and np.array_equal(table[1, rnd, :, 63], np.arange(1, 65))


def test_rule_1_is_monotone_in_the_lanes_that_entered(table):
    assert np.all(np.diff(table[1], axis=2) >= 0)
