"""The line substitute (sre_hip_substitute_lines, sre_hip_subst_template_check): the header declares the entry points,
libsregex.so exports them, the Python mirror has them, and the template parser (host only) accepts and refuses what
the header says.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest

import sregex_amd as S
import harness

NAMES = ["sre_hip_subst_template_check", "sre_hip_substitute_lines"]


def test_header_declares_the_entry_points():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        text = f.read()
    for name in NAMES:
        assert re.search(r"SRE_API\s+int\s+%s\s*\(" % name, text), name
    assert re.search(r"enum\s*\{\s*SRE_HIP_SUBST_MAX_PIECES = 30,\s*SRE_HIP_SUBST_MAX_LITERAL = 4096\s*\}", text)
    assert re.search(r"sre_hip_subst_template_check\s*\(\s*const void \*tmpl,\s*size_t tmpl_len,\s*int max_group,"
                     r"\s*int \*piece_groups,\s*size_t \*npieces\)", text)
    assert re.search(r"sre_hip_substitute_lines\s*\(\s*sre_hip_scanner_t \*sc,\s*const void \*d_buf,\s*size_t len,\s*int delim,"
                     r"\s*const void \*tmpl,\s*size_t tmpl_len,\s*int flags,\s*void \*d_out,\s*size_t out_cap,"
                     r"\s*sre_int_t \*d_index,\s*size_t index_cap,\s*sre_hip_filter_info_t \*info,\s*void \*hip_stream\)", text)


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(S.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in S.API, name
    assert len(S.API["sre_hip_substitute_lines"][1]) == 13
    assert len(S.API["sre_hip_subst_template_check"][1]) == 5
    assert (S.HIP_SUBST_MAX_PIECES, S.HIP_SUBST_MAX_LITERAL) == (30, 4096)


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.substitute_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "template", "out_ptr", "out_cap", "delim", "all_lines", "index_ptr",
                                    "index_cap", "hip_stream"]
    assert [sig.parameters[k].default for k in ("delim", "all_lines", "index_ptr", "index_cap", "hip_stream")] == [
        0x0A, False, None, 0, None]
    assert list(inspect.signature(S.template_pieces).parameters) == ["template", "max_group"]


VALID = [
    (b"", 0, []),
    (b"", 9, []),
    (b"abc", 0, [-1]),
    (b"$1", 1, [1]),
    (b"$1", 9, [1]),
    (b"${1}0", 4, [1, -1]),
    (b"a$$b", 0, [-1]),
    (b"$$", 0, [-1]),
    (b"$0-$2$2", 2, [0, -1, 2, 2]),
    (b"$0-$2$2", 9, [0, -1, 2, 2]),
    (b"a\x00b$1\x00", 1, [-1, 1, -1]),
    (b"${10}$10", 10, [10, 10]),
    (b"$007", 7, [7]),
    (b"{$1}", 1, [-1, 1, -1]),
]


@pytest.mark.parametrize("template,max_group,want", VALID, ids=[repr(v[0]) for v in VALID])
def test_template_pieces(template, max_group, want):
    assert S.template_pieces(template, max_group) == want


INVALID = [(b"$10", 4), (b"$", 9), (b"$x", 9), (b"${1", 9), (b"${}", 9), (b"x$", 9), (b"${", 9), (b"${1x}", 9), (b"$ 1", 9),
           (b"$1", 0), (b"${2}", 1), (b"$0", -1), (b"$99999999999999999999", 9)]


@pytest.mark.parametrize("template,max_group", INVALID, ids=[repr(v[0]) for v in INVALID])
def test_invalid_templates(template, max_group):
    with pytest.raises(ValueError):
        S.template_pieces(template, max_group)


def test_the_limits():
    # 30 pieces: groups and literals alternate, so no two merge
    assert S.template_pieces(b"$1x" * 15, 1) == [1, -1] * 15
    assert S.template_pieces(b"$1" * 30, 1) == [1] * 30
    for bad in (b"$1x" * 15 + b"$1", b"x" + b"$1x" * 15, b"$1" * 31):
        with pytest.raises(ValueError):
            S.template_pieces(bad, 1)
    # adjacent literals are one piece however long, up to 4096 bytes in all pieces together
    assert S.template_pieces(b"y" * 4096, 0) == [-1]
    assert S.template_pieces(b"y" * 4000 + b"$0" + b"$$" * 96, 0) == [-1, 0, -1]
    for bad in (b"y" * 4097, b"y" * 4000 + b"$0" + b"z" * 97, b"$$" * 4097):
        with pytest.raises(ValueError):
            S.template_pieces(bad, 0)


def test_the_c_entry_point_takes_null_outputs():
    lib = S.load_library()
    n = ctypes.c_size_t(77)
    assert lib.sre_hip_subst_template_check(b"a$1", 3, 1, None, ctypes.byref(n)) == 0 and n.value == 2
    assert lib.sre_hip_subst_template_check(b"a$1", 3, 1, None, None) == 0
    assert lib.sre_hip_subst_template_check(None, 0, 1, None, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sre_hip_subst_template_check(b"a$1", 3, 0, None, ctypes.byref(n)) == -1
