"""Key sets and the line lookup (sre_hip_keyset_*, sre_hip_lookup_lines): the header declares the entry points and the
info struct, libsregex.so exports them, the Python mirror has them, the argument checks that need no device refuse what
the header says, and the host hash (sre_hip_keyset_hash) equals the tally's hash written out in Python.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest

import sregex_amd as S
import harness

NAMES = ["sre_hip_keyset_create", "sre_hip_keyset_destroy", "sre_hip_keyset_rows", "sre_hip_keyset_distinct",
         "sre_hip_keyset_fields", "sre_hip_keyset_slots", "sre_hip_keyset_device_bytes", "sre_hip_keyset_hash",
         "sre_hip_lookup_lines"]
M64 = (1 << 64) - 1


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_entry_points():
    text = header()
    assert "typedef struct sre_hip_keyset_s sre_hip_keyset_t;" in text
    assert re.search(r"sre_hip_keyset_t \*sre_hip_keyset_create\(const void \*d_rows, size_t len, size_t nfields,\s*int fsep, "
                     r"int delim, void \*hip_stream\);", text)
    assert re.search(r"uint64_t sre_hip_keyset_hash\(const void \*row, size_t len, size_t nfields, int fsep\);", text)
    assert re.search(r"typedef struct \{\s*size_t nlines;[^}]*size_t nkeyed;[^}]*size_t nmembers;[^}]*size_t nselected;[^}]*"
                     r"size_t need_bytes;[^}]*size_t nwritten;[^}]*size_t out_bytes;\s*\}\s*sre_hip_lookup_info_t;", text)
    assert re.search(r"sre_hip_lookup_lines\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim,\s*const int \*groups, "
                     r"size_t ngroups, const sre_hip_keyset_t \*ks, int flags,\s*void \*d_out, size_t out_cap,\s*sre_int_t \*d_keyid, "
                     r"size_t keyid_cap,\s*sre_int_t \*d_index, size_t index_cap,\s*sre_hip_lookup_info_t \*info, void \*hip_stream\);",
                     text)
    doc = text[text.index("A key set: the distinct keys"):text.index("SRE_API int sre_hip_lookup_lines")]
    assert "hash & (slots - 1)" in doc and doc.count("Not offered") == 2


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(S.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in S.API, name
    assert len(S.API["sre_hip_lookup_lines"][1]) == 16 and len(S.API["sre_hip_keyset_create"][1]) == 6
    assert S.API["sre_hip_keyset_hash"][0] is ctypes.c_uint64


def test_the_mirror_has_the_calls():
    sig = inspect.signature(S.Scanner.lookup_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "groups", "keyset", "delim", "invert", "keyid_ptr",
                                    "keyid_cap", "index_ptr", "index_cap", "hip_stream"]
    assert S.LookupInfo._fields == ("nlines", "nkeyed", "nmembers", "nselected", "need_bytes", "nwritten", "out_bytes")
    for name in ("close", "rows", "distinct", "fields", "slots", "device_bytes"):
        assert hasattr(S.KeySet, name), name
    assert list(inspect.signature(S.keyset_hash).parameters) == ["row", "nfields", "fsep"]


def test_create_refuses_bad_arguments_without_a_device():
    lib = S.load_library()
    text = ctypes.create_string_buffer(b"a\tb\n")       # (never read: every call is refused in front of the device)
    ptr = ctypes.addressof(text)
    for nfields, fsep, delim in ((0, 9, 10), (S.HIP_EXTRACT_MAX_FIELDS + 1, 9, 10), (2, -1, 10), (2, 256, 10), (2, 9, -1),
                                 (2, 9, 256), (1, 300, 10), (2, 10, 10), (32, 0, 0)):
        assert lib.sre_hip_keyset_create(ptr, 4, nfields, fsep, delim, None) is None, (nfields, fsep, delim)
    assert lib.sre_hip_keyset_create(None, 4, 1, 9, 10, None) is None
    with pytest.raises(ValueError):
        S.KeySet(ptr, 4, 0)
    # the getters and destroy take a NULL set
    assert lib.sre_hip_keyset_rows(None) == lib.sre_hip_keyset_distinct(None) == lib.sre_hip_keyset_fields(None) == 0
    assert lib.sre_hip_keyset_slots(None) == lib.sre_hip_keyset_device_bytes(None) == 0
    lib.sre_hip_keyset_destroy(None)


def test_lookup_refuses_a_null_set_without_a_device():
    lib = S.load_library()
    arr = (ctypes.c_int * 1)(0)
    info = (ctypes.c_size_t * 7)(*([77] * 7))
    for flags in (0, S.HIP_LINES_INVERT, S.HIP_LINES_ALL):
        assert lib.sre_hip_lookup_lines(None, None, 0, 10, arr, 1, None, flags, None, 0, None, 0, None, 0, info, None) == -1
    assert list(info) == [77] * 7


# ------------------------------------------------------------------ the hash

def mix(h):
    h ^= h >> 32
    h = h * 0xD6E8FEB86659FD93 & M64
    return h ^ (h >> 29)


def tally_hash(fields):
    """sre_lt_hash (sregex_amd/csrc/sre_lines_tally.h) over a tuple of field texts"""
    h = 0xCBF29CE484222325
    for f in fields:
        h = mix(h ^ ((len(f) + 0x9E3779B97F4A7C15) & M64))
        for b in f:
            h = (h ^ b) * 0x100000001B3 & M64
    return mix(h)


ROWS = [((b"",), 9), ((b"a",), 9), ((b"10.0.0.1",), 9), ((b"with\ttab",), 9), ((b"ab", b"c"), 9), ((b"a", b"bc"), 9),
        ((b"", b""), 9), ((b"abc", b""), 9), ((b"", b"abc"), 9), ((b"x", b"y", b"z"), ord("|")), ((b"\x00\xff", b"\n"), 0x1F),
        (tuple(b"%d" % i for i in range(32)), 9), ((bytes(range(256)) * 5,), 9)]


@pytest.mark.parametrize("fields,fsep", ROWS, ids=[str(i) for i in range(len(ROWS))])
def test_hash_vectors(fields, fsep):
    row = bytes([fsep]).join(fields)
    got = S.load_library().sre_hip_keyset_hash(row, len(row), len(fields), fsep)
    assert got == tally_hash(fields) == S.keyset_hash(row, len(fields), fsep)


FIXED_EMPTY, FIXED_ADDR = 0x579D1306F92EFE2B, 0xFEA27AF7E82275DC      # of (b"",) and (b"10.0.0.1",)


def test_hash_fixed_values():
    """(so that the Python text above cannot drift together with the header)"""
    assert tally_hash((b"",)) == S.keyset_hash(b"") and tally_hash((b"ab", b"c")) != tally_hash((b"a", b"bc"))
    assert S.keyset_hash(b"ab\tc", 2) != S.keyset_hash(b"a\tbc", 2) != S.keyset_hash(b"ab\tc", 1)
    assert S.keyset_hash(b"a\tb", 1) == tally_hash((b"a\tb",)) != S.keyset_hash(b"a\tb", 2)        # K = 1: nothing is split
    assert S.keyset_hash(b"") == FIXED_EMPTY and S.keyset_hash(b"10.0.0.1") == FIXED_ADDR


def test_hash_of_a_row_that_breaks_the_field_rule_is_zero():
    lib = S.load_library()
    assert S.keyset_hash(b"a", 2) == 0 and S.keyset_hash(b"a\tb\tc", 2) == 0 and S.keyset_hash(b"a\tb\tc", 3) != 0
    assert S.keyset_hash(b"a\tb", 0) == 0 and S.keyset_hash(b"a\tb", 33) == 0 and S.keyset_hash(b"a", 1, 256) == 0
    assert lib.sre_hip_keyset_hash(None, 3, 1, 9) == 0 and lib.sre_hip_keyset_hash(None, 0, 1, 9) == tally_hash((b"",))
    assert lib.sre_hip_keyset_hash(b"abcdef", 3, 1, 9) == tally_hash((b"abc",))        # the length counts, not a terminator
