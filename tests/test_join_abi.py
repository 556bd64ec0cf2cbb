"""Key maps and the line join (sre_hip_keyset_create_map, sre_hip_keyset_values, sre_hip_join_lines): the header declares
the entry points, libsregex.so exports them, the Python mirror has them, and the argument checks that need no device
refuse what the header says.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest

import sregex_amd as S
import harness

NAMES = ["sre_hip_keyset_create_map", "sre_hip_keyset_values", "sre_hip_join_lines"]


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_entry_points():
    text = header()
    assert re.search(r"sre_hip_keyset_t \*sre_hip_keyset_create_map\(const void \*d_rows, size_t len, size_t nfields,\s*size_t nkeys, "
                     r"int fsep, int delim, void \*hip_stream\);", text)
    assert re.search(r"size_t sre_hip_keyset_values\(const sre_hip_keyset_t \*ks\);", text)
    assert re.search(r"enum \{ SRE_HIP_JOIN_MAX_VALUES = 31 \};", text)
    assert re.search(r"int sre_hip_join_lines\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim,\s*const int \*groups, "
                     r"size_t ngroups, const sre_hip_keyset_t \*ks,\s*const int \*vcols, size_t nvcols, int jsep, int flags,\s*"
                     r"void \*d_out, size_t out_cap,\s*sre_int_t \*d_keyid, size_t keyid_cap,\s*sre_int_t \*d_index, size_t index_cap,\s*"
                     r"sre_hip_lookup_info_t \*info, void \*hip_stream\);", text)
    sets = text[text.index("A key set: the distinct keys"):text.index("SRE_API int sre_hip_lookup_lines")]
    assert "a value column joined into" not in sets             # the two lists name what is still missing instead
    assert "last-row-wins" in sets and "the first row wins" in sets
    join = text[text.index("Line join: every line of d_buf"):text.index("SRE_API int sre_hip_join_lines")]
    for missing in ("a default text for missing", "last-row-wins", "joining extracted fields", "INVERT", "caseless keys"):
        assert missing in join, missing


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(S.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in S.API, name
    assert len(S.API["sre_hip_join_lines"][1]) == 19 and len(S.API["sre_hip_keyset_create_map"][1]) == 7
    assert S.HIP_JOIN_MAX_VALUES == 31 == S.HIP_EXTRACT_MAX_FIELDS - 1


def test_the_mirror_has_the_calls():
    sig = inspect.signature(S.Scanner.join_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "groups", "keyset", "vcols", "jsep", "delim",
                                    "all_lines", "keyid_ptr", "keyid_cap", "index_ptr", "index_cap", "hip_stream"]
    assert (sig.parameters["jsep"].default, sig.parameters["delim"].default, sig.parameters["all_lines"].default) == (9, 10, False)
    init = inspect.signature(S.KeySet.__init__)
    assert list(init.parameters)[:6] == ["self", "ptr", "length", "nfields", "fsep", "delim"]
    assert init.parameters["nkeys"].default is None
    assert isinstance(S.KeySet.values, property)


def test_create_map_refuses_bad_arguments_without_a_device():
    lib = S.load_library()
    text = ctypes.create_string_buffer(b"a\tb\n")       # (never read: every call is refused in front of the device)
    ptr = ctypes.addressof(text)
    top = S.HIP_EXTRACT_MAX_FIELDS
    # nkeys outside 1 .. nfields, nfields outside 1 .. the extract's limit
    for nfields, nkeys in ((2, 0), (2, 3), (1, 2), (0, 0), (0, 1), (top + 1, 1), (top + 1, top + 1), (top, top + 1)):
        assert lib.sre_hip_keyset_create_map(ptr, 4, nfields, nkeys, 9, 10, None) is None, (nfields, nkeys)
    # everything create refuses
    for nfields, fsep, delim in ((2, -1, 10), (2, 256, 10), (2, 9, -1), (2, 9, 256), (1, 300, 10), (2, 10, 10), (32, 0, 0)):
        assert lib.sre_hip_keyset_create_map(ptr, 4, nfields, 1, fsep, delim, None) is None, (nfields, fsep, delim)
    assert lib.sre_hip_keyset_create_map(None, 4, 2, 1, 9, 10, None) is None
    with pytest.raises(ValueError):
        S.KeySet(ptr, 4, 2, nkeys=0)
    with pytest.raises(ValueError):
        S.KeySet(ptr, 4, 2, nkeys=3)
    assert lib.sre_hip_keyset_values(None) == 0


def test_join_refuses_a_null_set_without_a_device():
    lib = S.load_library()
    arr, cols = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0)
    info = (ctypes.c_size_t * 7)(*([77] * 7))
    for flags in (0, S.HIP_LINES_ALL, S.HIP_LINES_INVERT):
        assert lib.sre_hip_join_lines(None, None, 0, 10, arr, 1, None, cols, 1, 9, flags, None, 0, None, 0, None, 0, info, None) == -1
    assert list(info) == [77] * 7
