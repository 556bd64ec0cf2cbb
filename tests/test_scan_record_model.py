"""The rule by which a FIRST / Thompson scan lane's record is kept as a 16-byte digest and read back
(sregex_amd/csrc/sre_scan_record.h: pack, plain, load), on the CPU: tests/scan_record_sim.cpp, a stand-alone program that
includes the header the kernels include.  Random records, plain records, and records that differ from a plain one in
exactly one field (each of the 24 fields in turn), segment lengths 64, 256 and 16 896, written into one reused summary
buffer so that stale records lie behind plain digests.  tests/test_gpu_scan_records.py checks the kernels that use the
rule against the oracle."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRCS = [os.path.join(HERE, "scan_record_sim.cpp"), os.path.join(ROOT, "sregex_amd", "csrc", "sre_scan_record.h")]


def build(name, extra):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SRCS):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra"] + extra
                              + ["-o", exe, SRCS[0], "-I" + os.path.join(ROOT, "sregex_amd", "csrc")])
    return exe


def check(exe, seed, cases):
    p = subprocess.run([exe, str(seed), str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    m = re.match(r"ok cases=(\d+) plain=(\d+) one_field=(\d+) full=(\d+)", p.stdout)
    assert m, p.stdout
    n, plain, one_field, full = map(int, m.groups())
    assert n == cases and plain + full == cases
    # a quarter of the cases are plain records, half differ from one in a single field and must all be stored in full
    assert plain > cases // 5 and one_field > cases // 3 and full >= one_field, p.stdout


@pytest.mark.parametrize("seed", [1, 2, 20261021])
def test_load_of_pack_is_the_record(seed):
    check(build("scan_record_sim", []), seed, 300000)


def test_under_address_and_undefined_sanitizers():
    """the same program as a stand-alone sanitizer build"""
    check(build("scan_record_sim_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), 3, 100000)
