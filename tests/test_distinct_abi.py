"""The line distinct (sre_hip_distinct_lines): the header declares the enum, the struct and the entry point,
libsregex.so exports it, the Python mirror has it, and the argument checks that need no device refuse what the header
says and leave info untouched.  No GPU needed."""
import ctypes
import inspect
import os
import re

import pytest

import sregex_amd as S
import harness

NAME = "sre_hip_distinct_lines"
FIELDS = ("nlines", "nkeyed", "nkeys", "nkeys_kept", "nselected", "need_bytes", "nwritten", "out_bytes")


def header():
    with open(os.path.join(harness.ROOT, "include", "sregex_hip.h")) as f:
        return f.read()


def test_header_declares_the_enum_the_struct_and_the_entry_point():
    text = header()
    assert re.search(r"enum \{ SRE_HIP_DISTINCT_FIRST = 0, SRE_HIP_DISTINCT_LAST = 1, SRE_HIP_DISTINCT_EVERY = 2 \};", text)
    m = re.search(r"typedef struct \{([^}]*)\} sre_hip_distinct_info_t;", text)
    assert m
    assert tuple(re.findall(r"size_t (\w+);", m.group(1))) == FIELDS
    assert re.search(r"int sre_hip_distinct_lines\(sre_hip_scanner_t \*sc, const void \*d_buf, size_t len, int delim,\s*"
                     r"const int \*groups, size_t ngroups, int which, size_t min_count, size_t max_count, int flags,\s*"
                     r"size_t max_keys, void \*d_out, size_t out_cap,\s*uint64_t \*d_keycount, size_t keycount_cap,\s*"
                     r"sre_int_t \*d_keyline, size_t keyline_cap,\s*sre_int_t \*d_index, size_t index_cap,\s*"
                     r"sre_hip_distinct_info_t \*info, void \*hip_stream\);", text)


def test_the_header_lists_the_idioms_and_what_is_not_offered():
    text = header()
    mine = text[text.index("Line distinct: the lines of d_buf"):text.index("SRE_API int sre_hip_distinct_lines")]
    flat = " ".join(mine.replace("*", " ").split())
    for idiom in ("awk '!seen[k]++'", "sort -u", "latest record per key", "uniq -u", "uniq -d", "uniq -D", "HAVING COUNT( ) >= n"):
        assert idiom in flat, idiom
    own = flat[flat.index("Not offered:"):]
    for missing in ("SRE_HIP_LINES_ALL", "adjacency-only uniq semantics", "caseless keys", "key numbers in first-appearance order",
                    "a fifth index word", "every match of a line", "Thompson and COUNT scanners", "stream sets"):
        assert missing in own, missing


def test_library_exports_the_entry_point():
    lib = ctypes.CDLL(S.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in S.API and len(S.API[NAME][1]) == 21 and S.API[NAME][0] is ctypes.c_int
    assert (S.HIP_DISTINCT_FIRST, S.HIP_DISTINCT_LAST, S.HIP_DISTINCT_EVERY) == (0, 1, 2)
    assert S.DistinctInfo._fields == FIELDS
    assert [n for n, _ in S.DistinctInfoStruct._fields_] == list(FIELDS)
    assert ctypes.sizeof(S.DistinctInfoStruct) == 8 * ctypes.sizeof(ctypes.c_size_t)


def test_the_mirror_has_the_call():
    sig = inspect.signature(S.Scanner.distinct_lines)
    assert list(sig.parameters) == ["self", "ptr", "length", "out_ptr", "out_cap", "groups", "max_keys", "which", "min_count",
                                    "max_count", "delim", "invert", "keycount_ptr", "keycount_cap", "keyline_ptr", "keyline_cap",
                                    "index_ptr", "index_cap", "hip_stream"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == {"which": S.HIP_DISTINCT_FIRST, "min_count": 1, "max_count": 0, "delim": 0x0A, "invert": False, "keycount_ptr": None,
                 "keycount_cap": 0, "keyline_ptr": None, "keyline_cap": 0, "index_ptr": None, "index_cap": 0, "hip_stream": None}


def test_refusals_that_need_no_device():
    """Every one of these is refused in front of the first look at the scanner or the device: sc stands for a scanner here
    and is zeroed host memory."""
    lib = S.load_library()
    sc = ctypes.create_string_buffer(4096)
    text = ctypes.create_string_buffer(b"k=a\nk=b\n")        # (never read)
    side = ctypes.create_string_buffer(256)
    arr = (ctypes.c_int * 33)(*([1] * 33))
    info = (ctypes.c_size_t * 8)(*([77] * 8))
    ok = dict(sc=ctypes.addressof(sc), buf=ctypes.addressof(text), delim=10, groups=arr, ngroups=1, which=S.HIP_DISTINCT_FIRST,
              min_count=1, max_count=0, flags=0, max_keys=16, out=(ctypes.addressof(side), 64), keycount=(None, 0), keyline=(None, 0),
              index=(None, 0))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sre_hip_distinct_lines(a["sc"], a["buf"], 8, a["delim"], a["groups"], a["ngroups"], a["which"], a["min_count"],
                                          a["max_count"], a["flags"], a["max_keys"], a["out"][0], a["out"][1], a["keycount"][0],
                                          a["keycount"][1], a["keyline"][0], a["keyline"][1], a["index"][0], a["index"][1], info, None)
    assert call(sc=None) == -1
    for which in (3, -1, 1 << 20):
        assert call(which=which) == -1, which
    assert call(min_count=0) == -1 and call(min_count=0, max_count=5) == -1
    assert call(min_count=3, max_count=2) == -1 and call(min_count=2, max_count=1) == -1
    for flags in (S.HIP_LINES_ALL, 8, S.HIP_LINES_ALL | S.HIP_LINES_INVERT, 4, 1 << 30):
        assert call(flags=flags) == -1, flags
    for max_keys in (0, (1 << 30) + 1):
        assert call(max_keys=max_keys) == -1, max_keys
    for ngroups in (0, 33):
        assert call(ngroups=ngroups) == -1, ngroups
    assert call(groups=None) == -1
    for name in ("out", "keycount", "keyline", "index"):
        assert call(**{name: (None, 3)}) == -1, name
    for delim in (-1, 256):
        assert call(delim=delim) == -1, delim
    assert call(buf=None) == -1
    assert call(out=(ctypes.addressof(text) + 2, 4)) == -1          # the output overlaps the buffer
    assert list(info) == [77] * 8


def test_the_mirror_raises_value_error_without_a_device():
    """the Python method refuses the same arguments in front of the library: `self` is never looked at"""
    for kw in (dict(which=3), dict(min_count=0), dict(min_count=3, max_count=2), dict(max_keys=0), dict(max_keys=(1 << 30) + 1),
               dict(groups=[]), dict(groups=[1] * 33), dict(keycount_cap=2), dict(keyline_cap=2), dict(index_cap=2), dict(out_cap=2)):
        a = dict(dict(ptr=1, length=8, out_ptr=None, out_cap=0, groups=[1], max_keys=4), **kw)
        with pytest.raises(ValueError):
            S.Scanner.distinct_lines(None, **a)
