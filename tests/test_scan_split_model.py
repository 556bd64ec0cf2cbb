"""The rule of the scan kernel's split walk (sregex_amd/csrc/sre_scan_split.h: K sub-chains of lookups side by side, the
chains behind the first from a guessed row, validated in order, the first wrong one and all behind it walked again)
against the serial walk, on the CPU: tests/scan_split_sim.cpp, a stand-alone program over random small tables (rows, a
trap row, count bytes) and random index strings of 8, 16, 32 and 64 lookups, K = 1, 2 and 4.  The kernel mirrors that
header line by line; tests/test_gpu_scan_split.py checks the kernel itself against the oracle."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def sim():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "scan_split_sim")
    srcs = [os.path.join(HERE, "scan_split_sim.cpp"), os.path.join(ROOT, "sregex_amd", "csrc", "sre_scan_split.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", exe, srcs[0],
                               "-I" + os.path.join(ROOT, "sregex_amd", "csrc")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 20261020])
def test_split_walk_equals_serial_walk(sim, seed):
    """(t, cnt) of the split walk with K = 2 and 4 equal the serial walk's in every case, and the cases cover what the
    rule distinguishes: rounds whose guesses all hit, rounds with a miss, a chain that ends in the trap row in the first
    chain and in a later one, rounds that count matches."""
    p = subprocess.run([sim, str(seed), "30000"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    m = re.match(r"ok cases=(\d+) hit=(\d+) miss=(\d+) slow=(\d+) slow_later=(\d+) counted=(\d+)", p.stdout)
    assert m, p.stdout
    cases, hit, miss, slow, slow_later, counted = map(int, m.groups())
    assert cases == 30000
    for n in (hit, miss, slow, slow_later, counted):
        assert n > cases // 100, p.stdout
