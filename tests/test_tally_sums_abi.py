"""The line tally with sums (sre_hip_tally_sums_lines, sre_hip_tally_number): the header declares the entry points, the
enum and the aggregate, libsregex.so exports them, the Python mirror has them, and the number rule (host only) takes and
refuses what the header says.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest

import sregex_amd as S
import harness

NAMES = ["sre_hip_tally_sums_lines", "sre_hip_tally_number"]


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_entry_points():
    text = header()
    for name in NAMES:
        assert re.search(r"SRE_API\s+int\s+%s\s*\(" % name, text), name
    assert re.search(r"enum\s*\{\s*SRE_HIP_TALLY_MAX_VALUES = 8\s*\}", text)
    assert re.search(r"typedef struct \{\s*int64_t\s+sum;[^}]*int64_t\s+min;[^}]*int64_t\s+max;[^}]*uint64_t\s+n;[^}]*\}"
                     r"\s*sre_hip_tally_sum_t;", text)
    assert re.search(r"sre_hip_tally_sums_lines\s*\(\s*sre_hip_scanner_t \*sc,\s*const void \*d_buf,\s*size_t len,\s*int delim,"
                     r"\s*const int \*groups,\s*size_t ngroups,\s*const int \*vgroups,\s*size_t nvgroups,\s*int fsep,\s*int flags,"
                     r"\s*size_t max_keys,\s*void \*d_out,\s*size_t out_cap,\s*uint64_t \*d_counts,\s*size_t counts_cap,"
                     r"\s*sre_hip_tally_sum_t \*d_sums,\s*size_t sums_cap,\s*sre_int_t \*d_keyid,\s*size_t keyid_cap,"
                     r"\s*sre_int_t \*d_index,\s*size_t index_cap,\s*sre_hip_tally_info_t \*info,\s*void \*hip_stream\)", text)
    assert re.search(r"sre_hip_tally_number\s*\(\s*const void \*text,\s*size_t len,\s*int64_t \*value\)", text)


def test_the_tally_no_longer_disclaims_sums():
    text = header()
    tally = text[text.index("Line tally: `extract | sort | uniq -c`"):text.index("SRE_API int sre_hip_tally_lines")]
    assert "Not offered" in tally and "sums of a field" not in tally


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(S.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in S.API, name
    assert len(S.API["sre_hip_tally_sums_lines"][1]) == 23
    assert len(S.API["sre_hip_tally_sums_lines"][1]) == len(S.API["sre_hip_tally_lines"][1]) + 4
    assert len(S.API["sre_hip_tally_number"][1]) == 3
    assert S.HIP_TALLY_MAX_VALUES == 8


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.tally_sums_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "groups", "vgroups", "max_keys", "delim", "fsep",
                                    "flags", "counts_ptr", "counts_cap", "sums_ptr", "sums_cap", "keyid_ptr", "keyid_cap",
                                    "index_ptr", "index_cap", "hip_stream"]
    defaults = [p.default for p in sig.parameters.values() if p.default is not inspect.Parameter.empty]
    assert defaults == [0x0A, 0x09, 0, None, 0, None, 0, None, 0, None, 0, None]
    assert list(inspect.signature(S.tally_number).parameters) == ["text"]
    assert [(n, t) for n, t in S.TallySumStruct._fields_] == [("sum", ctypes.c_int64), ("min", ctypes.c_int64),
                                                              ("max", ctypes.c_int64), ("n", ctypes.c_uint64)]
    assert ctypes.sizeof(S.TallySumStruct) == 32


NINES = b"9" * 18
NUMBERS = [(b"0", 0), (b"-0", 0), (b"007", 7), (NINES, 10 ** 18 - 1), (b"-" + NINES, -(10 ** 18 - 1))]
NOT_NUMBERS = [b"", b"-", b"--1", b"+1", b"1 ", b" 1", b"12a", b"1-", b"1" * 19, b"-" + b"1" * 19, NINES + b"\0"]


@pytest.mark.parametrize("text,want", NUMBERS, ids=[repr(t) for t, _ in NUMBERS])
def test_numbers(text, want):
    value = ctypes.c_int64(-4242)
    assert S.load_library().sre_hip_tally_number(text, len(text), ctypes.byref(value)) == 1
    assert value.value == want
    assert S.tally_number(text) == want


@pytest.mark.parametrize("text", NOT_NUMBERS, ids=[repr(t) for t in NOT_NUMBERS])
def test_not_numbers_leave_the_value_untouched(text):
    value = ctypes.c_int64(-4242)
    assert S.load_library().sre_hip_tally_number(text, len(text), ctypes.byref(value)) == 0
    assert value.value == -4242
    assert S.tally_number(text) is None


def test_the_length_counts_not_a_terminator():
    lib = S.load_library()
    value = ctypes.c_int64(-4242)
    assert lib.sre_hip_tally_number(b"123456", 3, ctypes.byref(value)) == 1 and value.value == 123
    assert lib.sre_hip_tally_number(b"12a", 2, ctypes.byref(value)) == 1 and value.value == 12
    assert lib.sre_hip_tally_number(None, 0, ctypes.byref(value)) == 0 and value.value == 12
    assert lib.sre_hip_tally_number(b"1", 1, None) == 0
