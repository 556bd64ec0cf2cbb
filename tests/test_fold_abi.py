"""The line fold (sre_hip_fold_lines): the header declares the enum, the struct and the entry point, libsregex.so exports
it, the Python mirror has it, and the argument checks that need no device refuse what the header says and leave info
untouched.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest

import sregex_amd as S
import harness

NAME = "sre_hip_fold_lines"
FIELDS = ("nlines", "nmarked", "nrecords", "longest", "need_bytes", "nwritten", "out_bytes")


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_enum_the_struct_and_the_entry_point():
    text = header()
    assert re.search(r"enum \{ SRE_HIP_FOLD_NEXT = 8 \};", text)
    m = re.search(r"typedef struct \{([^}]*)\} sre_hip_fold_info_t;", text)
    assert m
    assert tuple(re.findall(r"(\w+)[,;]", m.group(1).replace("size_t", ""))) == FIELDS
    assert re.search(r"int sre_hip_fold_lines\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim, int flags, int join,\s*"
                     r"size_t max_lines, void \*d_out, size_t out_cap, sre_int_t \*d_recid, size_t recid_cap,\s*"
                     r"sre_int_t \*d_records, size_t records_cap, sre_hip_fold_info_t \*info, void \*hip_stream\);", text)


def test_the_header_lists_the_idioms_and_what_is_not_offered():
    text = header()
    mine = text[text.index("Line fold: the lines of d_buf"):text.index("SRE_API int sre_hip_fold_lines")]
    flat = " ".join(mine.replace("*", " ").split())
    for idiom in ("multiline codec", "multiline.pattern / negate / match", "Fluent Bit", "awk '/^[0-9]{4}-/{if (r) print r; r=$0; next}",
                  r"pattern ^\d{4}-\d\d-\d\d, flags SRE_HIP_LINES_INVERT", r"pattern ^(\s|Caused by:), flags 0",
                  r"pattern \\$, flags SRE_HIP_FOLD_NEXT", "flags SRE_HIP_FOLD_NEXT | SRE_HIP_LINES_INVERT", "what => previous",
                  "what => next"):
        assert idiom in flat, idiom
    own = flat[flat.index("Not offered:"):]
    for missing in ("SRE_HIP_LINES_ALL", "a join string of more or fewer than one byte", "a cap on a record's bytes", "unfolding",
                    "records across calls or stream sets", "selecting records in the same call"):
        assert missing in own, missing


def test_library_exports_the_entry_point():
    lib = ctypes.CDLL(S.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in S.API and len(S.API[NAME][1]) == 15 and S.API[NAME][0] is ctypes.c_int
    assert S.HIP_FOLD_NEXT == 8 and S.HIP_FOLD_NEXT & (S.HIP_LINES_ALL | S.HIP_LINES_INVERT | S.HIP_SORT_DESC) == 0
    assert S.FoldInfo._fields == FIELDS
    assert [n for n, _ in S.FoldInfoStruct._fields_] == list(FIELDS)
    assert ctypes.sizeof(S.FoldInfoStruct) == 7 * ctypes.sizeof(ctypes.c_size_t)


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.fold_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "join", "max_lines", "delim", "invert", "fold_next",
                                    "recid_ptr", "recid_cap", "records_ptr", "records_cap", "hip_stream"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"join": 0x01, "max_lines": 0, "delim": 0x0A, "invert": False, "fold_next": False, "recid_ptr": None, "recid_cap": 0,
                 "records_ptr": None, "records_cap": 0, "hip_stream": None}


def test_refusals_that_need_no_device():
    """Every one of these is refused in front of the first look at the scanner or the device: sc stands for a scanner here
    and is zeroed host memory."""
    lib = S.load_library()
    sc = ctypes.create_string_buffer(4096)
    text = ctypes.create_string_buffer(b"a\n b\nc\n")         # (never read)
    side = ctypes.create_string_buffer(256)
    tab = ctypes.create_string_buffer(256)
    info = (ctypes.c_size_t * 7)(*([77] * 7))
    ok = dict(sc=ctypes.addressof(sc), buf=ctypes.addressof(text), delim=10, flags=0, join=1, max_lines=0,
              out=(ctypes.addressof(side), 64), recid=(None, 0), records=(None, 0))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sre_hip_fold_lines(a["sc"], a["buf"], 7, a["delim"], a["flags"], a["join"], a["max_lines"], a["out"][0], a["out"][1],
                                      a["recid"][0], a["recid"][1], a["records"][0], a["records"][1], info, None)
    assert call(sc=None) == -1
    ALL, INV, NEXT = S.HIP_LINES_ALL, S.HIP_LINES_INVERT, S.HIP_FOLD_NEXT
    for flags in (ALL, ALL | INV, ALL | NEXT, 4, 4 | NEXT, 16, 1 << 30, -1):
        assert call(flags=flags) == -1, flags
    for join in (-1, 256, 1 << 20):
        assert call(join=join) == -1, join
    for delim in (-1, 256):
        assert call(delim=delim) == -1, delim
    for name in ("recid", "records"):
        assert call(**{name: (None, 3)}) == -1, name                        # a capacity without a table
        assert call(**{name: (ctypes.addressof(tab), 0)}) == -1, name       # a table without a capacity
    assert call(out=(None, 3)) == -1
    assert call(buf=None) == -1
    assert call(out=(ctypes.addressof(text) + 2, 4)) == -1          # the output overlaps the buffer
    assert list(info) == [77] * 7


def test_the_mirror_raises_value_error_without_a_device():
    """the Python method refuses the same arguments in front of the library: `self` is never looked at"""
    for kw in (dict(join=-1), dict(join=256), dict(recid_cap=2), dict(records_cap=2), dict(recid_ptr=64), dict(records_ptr=64),
               dict(out_cap=2)):
        a = dict(dict(ptr=1, length=8, out_ptr=None, out_cap=0), **kw)
        with pytest.raises(ValueError):
            S.Scanner.fold_lines(None, **a)
